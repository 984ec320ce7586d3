#!/usr/bin/env python
"""Cost of the distillation loss at the headline batch (8 x 512 x 512 pixels, C = 23, ldc = 24) on one MI355X.

Seeded student and teacher logits in padded NHWC buffers (bench_pseudo.py's recipe: unit noise plus a winner per 8 x 8 block), an
image weight per image and a pixel weight map.  HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE
inside every round, all in ONE process:
  * soft_ce_ms / soft_kl_ms / soft_sym_ms    udaseg_soft_ce_fwd_bwd with dlogits and column sums, teacher logits, both weights, 'mean'
  * soft_ce_probs_ms                         the same, soft cross entropy against teacher probabilities
  * soft_ce_loss_only_ms                     the same kernel without dlogits (a no-grad forward)
  * weight_sum_ms                            udaseg_pixel_weight_sum (what 'weighted_mean' adds)
  * ce_fwd_bwd_ms                            udaseg_ce_fwd_bwd on the student logits with hard labels: the loss this one sits beside
  * torch_soft_ce_ms                         the torch composition, forward and backward: log_softmax, softmax of the teacher,
                                             weighted product, sum, autograd
  * copy3_ms                                 device copies of the same bytes: two reads and one write of pixels x ldc x 4
                                             (one copy_ of the logits plus one read-only sum of the teacher buffer)
  * conf_share_ms / copy_scores_ms           udaseg_conf_share beside a copy of the score buffer
  * distill_step_ms / advent_step_ms         one DistillTrainer.distill_step beside one AdventTrainer.advent_step (r18, --step-batch
                                             x 3 x --step-size^2, the same two batches)
Reported, not judged (there is no speed gate).  One JSON line; --out also writes it to a file together with the git HEAD.

    python tools/bench_distill.py [--reps 10 --warmup 2 --out profiles/distill_bench.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.advent_trainer import AdventTrainer  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.distill import DistillTrainer  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.losses import SoftCrossEntropyLoss  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def alternating(legs, reps, warmup):
    """{name: sorted HIP-event times in ms}: every round runs each leg once, in order, each between its own pair of events."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in ms.items()}


def logits(n, h, w, c, ldc, g):
    tb = torch.randint(0, c, (n, h // 8, w // 8), generator=g)
    winner = tb.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    z = 1.5 * torch.randn(n, h, w, ldc, generator=g)
    z.scatter_add_(3, winner[..., None], 12.0 * torch.rand(n, h, w, 1, generator=g))
    z[..., c:] = 0.0
    return z, winner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--step-size", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c = a.batch, a.size, a.size, a.classes
    ldc = (c + 3) // 4 * 4
    pixels, ppi = n * h * w, h * w
    g = torch.Generator().manual_seed(2)
    z, winner = logits(n, h, w, c, ldc, g)
    t, _ = logits(n, h, w, c, ldc, g)
    student, teacher = z.to(dev), t.to(dev)
    tprobs = torch.zeros_like(teacher)
    tprobs[..., :c] = torch.softmax(teacher[..., :c], -1)
    labels = winner.reshape(-1).to(dev)
    wpx = (0.25 + 1.5 * torch.rand(pixels, generator=g)).to(dev)
    wimg = (0.5 + torch.rand(n, generator=g)).to(dev)
    np_ = K.seg_partials()
    parts = torch.empty(np_, dtype=torch.float64, device=dev)
    cparts = torch.empty(np_ * ldc, dtype=torch.float32, device=dev)
    ce_parts = torch.empty(_lib.load().udaseg_ce_partials(), dtype=torch.float64, device=dev)
    ce_cparts = torch.empty(_lib.load().udaseg_ce_partials() * ldc, dtype=torch.float32, device=dev)
    colsum = torch.empty(ldc, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dl = torch.empty(pixels, ldc, dtype=torch.float32, device=dev)
    stats = torch.zeros(3, dtype=torch.int64, device=dev)
    denom = torch.empty(1, dtype=torch.float64, device=dev)
    wparts = torch.empty(3 * np_, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    above, nonfinite = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    share = torch.empty(n, dtype=torch.float32, device=dev)
    dst = torch.empty_like(student)
    held = {}

    def soft(kind, tbuf, probs, grad=True):
        K.soft_ce_fwd_bwd(student, tbuf, wpx, wimg, n, ppi, c, ldc, ldc, probs, kind, 1.0, 1.0, 1.0, -4.0, True, None, parts, loss,
                          dl if grad else None, cparts if grad else None, colsum if grad else None, stats)

    srows, trows = student.view(pixels, ldc)[:, :c], teacher.view(pixels, ldc)[:, :c]
    wrow = wpx * wimg.repeat_interleave(ppi)

    def torch_soft_ce():
        x = srows.detach().requires_grad_()
        l = -(torch.softmax(trows, 1) * torch.log_softmax(x, 1)).sum(1)
        (wrow * l).mean().backward()
        held["grad"] = x.grad

    def copy3():
        dst.copy_(student)
        held["sum"] = teacher.sum()

    # one trainer iteration of each kind on the same batches
    sn, ss = a.step_batch, a.step_size
    torch.manual_seed(0)
    src = torch.randn(sn, 3, ss, ss, generator=g).to(dev)
    tgt = torch.randn(sn, 3, ss, ss, generator=g).to(dev)
    masks = torch.randint(0, c, (sn, ss, ss), generator=g).to(dev)
    net_d = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c)
    tr_d = DistillTrainer(net_d, dev, MeanTeacher(net_d.to(dev)), lambda_soft=1.0, loss=SoftCrossEntropyLoss("ce"), tau=0.5)
    opt_d = FusedAdam(net_d.parameters(), lr=1e-4)
    net_a = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c)
    tr_a = AdventTrainer(net_a, dev, lambda_adv=0.001, lambda_ent=0.0)
    opt_a = FusedAdam(net_a.parameters(), lr=1e-4)
    tr_a.discriminator_optimizer = FusedAdam(tr_a.discriminator.parameters(), lr=1e-4)
    for net in (net_d, net_a, tr_a.discriminator):
        net.train()

    legs = {
        "soft_ce": lambda: soft("ce", teacher, 0),
        "soft_kl": lambda: soft("kl", teacher, 0),
        "soft_sym": lambda: soft("symmetric", teacher, 0),
        "soft_ce_probs": lambda: soft("ce", tprobs, 1),
        "soft_ce_loss_only": lambda: soft("ce", teacher, 0, grad=False),
        "weight_sum": lambda: K.pixel_weight_sum(wpx, wimg, n, ppi, wparts, denom, counts),
        "ce_fwd_bwd": lambda: K.ce_fwd_bwd(student, labels, pixels, c, ldc, ce_parts, loss, dl, ce_cparts, colsum),
        "torch_soft_ce": torch_soft_ce,
        "copy3": copy3,
        "conf_share": lambda: K.conf_share(teacher, n, ppi, c, ldc, 0, 0.968, above, nonfinite, share),
        "copy_scores": lambda: dst.copy_(teacher),
        "distill_step": lambda: tr_d.distill_step(src, masks, tgt, opt_d),
        "advent_step": lambda: tr_a.advent_step(src, masks, tgt, opt_a, update_metrics=False),
    }
    ms = alternating(legs, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    soft("ce", teacher, 0)
    agree = float((held["grad"] - dl[:, :c]).abs().max())
    nbytes = pixels * ldc * 4
    copy_rate = 3 * nbytes / (med["copy3"] * 1e-3) / 1e12
    rate = lambda k: 3 * nbytes / (med[k] * 1e-3) / 1e12          # noqa: E731  (two reads and one write of pixels x ldc x 4)
    share_rate = nbytes / (med["conf_share"] * 1e-3) / 1e12
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r4 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "pixels": [n, h, w], "classes": c, "ldc": ldc, "reps": a.reps, "warmup": a.warmup, "step_batch": [sn, 3, ss, ss],
        "device": torch.cuda.get_device_name(0),
        **{f"{k}_ms": r4(v) for k, v in med.items()},
        **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in legs},
        "copy3_TB_per_s": r4(copy_rate),
        **{f"{k}_TB_per_s": r4(rate(k)) for k in ("soft_ce", "soft_kl", "soft_sym", "soft_ce_probs")},
        **{f"{k}_fraction_of_copy_rate": r4(rate(k) / copy_rate) for k in ("soft_ce", "soft_kl", "soft_sym", "soft_ce_probs")},
        "soft_ce_over_torch": r4(med["soft_ce"] / med["torch_soft_ce"]),
        "soft_ce_over_ce_fwd_bwd": r4(med["soft_ce"] / med["ce_fwd_bwd"]),
        "conf_share_TB_per_s": r4(share_rate),
        "conf_share_fraction_of_copy_rate": r4(share_rate / (2 * nbytes / (med["copy_scores"] * 1e-3) / 1e12)),
        "distill_step_over_advent_step": r4(med["distill_step"] / med["advent_step"]),
        "soft_ce_max_abs_diff_to_torch": agree,
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(f"# python tools/bench_distill.py: the distillation loss at {n} x {h} x {w} pixels, C = {c} on 1 x MI355X "
                     "(HIP-event medians, legs alternating in one process).  One run; nothing is gated on these figures.\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write("# soft_*: loss, dlogits and column sums in one pass (two reads and one write of pixels x ldc x 4 bytes, plus 4 bytes\n"
                     "# of pixel weight); ce_fwd_bwd reads one such buffer and 8 bytes of label per pixel and writes one.\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
