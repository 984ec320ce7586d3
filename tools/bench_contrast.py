#!/usr/bin/env python
"""Cost of the prototype contrast loss at the headline batch (8 x 512 x 512 pixels, D = 16 decoder channels, C = 23) on one MI355X.

Seeded decoder features in the padded NHWC buffer forward_parts hands out (ldf = 16), as tools/bench_proto.py makes them: a
unit-normal prototype per class plus unit-normal noise, labels constant on 96 x 96 blocks; the bank is filled from them (one class
is left unseen).  The soft target is the assignment of a second, independently drawn feature field (the teacher's weak view).
HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE inside every round, all in ONE process:
  * contrast_hard_ms / contrast_soft_ms     udaseg_proto_contrast_fwd_bwd, loss AND feature gradient in one pass
  * contrast_hard_loss_only_ms              the same entry point without dfeat (what a lambda of 0 costs)
  * assign_ms                               udaseg_proto_assign
  * rectify_ms                              udaseg_proto_rectify on the same features (tools/bench_proto.py's leg)
  * torch_contrast_hard_ms / _soft_ms       cross_entropy(-(dist - dist.min) * inv_tau, t) over the seen classes with the
                                            [pixels, C, D] broadcast, forward and autograd backward to the features
  * torch_contrast_hard_matmul_ms           the same with |f|^2 - 2 f P^T + |P|^2 for the distances (less exact, no broadcast)
  * torch_assign_ms                         softmax(-(dist - dist.min) * inv_tau) with the broadcast, no gradient
  * copy_features_ms                        a device-to-device copy of the feature buffer: the same bytes in, the same bytes out
  * structure_step_ms / distill_step_ms     one StructureTrainer iteration (both lambdas on) beside one DistillTrainer iteration
                                            (same bank) of r18 at --train-batch x 3 x --train-size^2
Reported, not judged (the only condition: the fused pass is faster than the torch composition of the same run): every ratio as
measured, and each pixel kernel's rate over its bytes as a fraction of the copy's rate.  The legs run back to back on buffers of
32 MB that the 256 MB last-level cache can hold, so the rates are cache-assisted and not HBM figures; a training step touches
far more memory between two calls of the loss.  One JSON line; --out also writes it to a file together with the git HEAD.

    python tools/bench_contrast.py [--reps 10 --warmup 2 --out profiles/contrast_bench.txt]
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
import torch.nn.functional as F  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import proto as PR  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.distill import DistillTrainer  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.structure import StructureTrainer  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--train-size", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c, d = a.batch, a.size, a.size, a.classes, a.dim
    ldc = (c + 3) // 4 * 4
    pixels = n * h * w
    g = torch.Generator().manual_seed(2)
    blocks = torch.randint(0, c - 1, (n, (h + 95) // 96, (w + 95) // 96), generator=g)          # class c - 1 stays unseen
    regions = blocks.repeat_interleave(96, 1).repeat_interleave(96, 2)[:, :h, :w].contiguous()
    centres = torch.randn(c, d, generator=g)
    feat = (centres[regions.reshape(-1)] + torch.randn(pixels, d, generator=g)).to(dev)
    weak = (centres[regions.reshape(-1)] + torch.randn(pixels, d, generator=g)).to(dev)
    labels = regions.reshape(-1).to(torch.uint8).to(dev)
    labels_long = labels.long()
    z = 1.5 * torch.randn(pixels, ldc, generator=g)
    z[:, c:] = 0.0
    scores = z.to(dev)

    bank = PR.PrototypeBank(c, d, min_pixels=1)
    bank._ensure(dev)
    K.proto_accumulate(feat, d, d, labels, pixels, c, bank.sums, bank.sq, bank.counts)
    bank.update()
    seen = bank.seen != 0
    assert int(seen.sum()) == c - 1
    target = torch.empty(pixels, ldc, dtype=torch.float32, device=dev)
    K.proto_assign(weak, d, d, c, ldc, bank.prototypes, bank.seen, bank.inv_tau, pixels, target)
    out = torch.empty(pixels, ldc, dtype=torch.float32, device=dev)
    rect = torch.empty(pixels, ldc, dtype=torch.float32, device=dev)
    dfeat = torch.empty(pixels, d, dtype=torch.float32, device=dev)
    f_dst = torch.empty_like(feat)
    partials = torch.empty(K.seg_partials(), dtype=torch.float64, device=dev)
    loss = {k: torch.empty((), dtype=torch.float32, device=dev) for k in ("hard", "soft", "hard_loss_only")}
    p32 = bank.prototypes.float()
    ps = p32[seen]
    inv_tau = bank.inv_tau
    t_hard = F.one_hot(labels_long, c).float()[:, seen]
    t_soft = target[:, :c][:, seen].contiguous()
    held = {}

    def fused(name, lab, tgt, grad):
        K.proto_contrast_fwd_bwd(feat, d, d, lab, tgt, ldc if tgt is not None else 0, None, None, n, h * w, c, bank.prototypes,
                                 bank.seen, bank.inv_tau, True, None, partials, loss[name], dfeat if grad else None, None)

    def torch_contrast(t, name, matmul=False):
        x = feat.detach().requires_grad_()
        if matmul:
            dist = (x * x).sum(1, keepdim=True) - 2.0 * x @ ps.t() + (ps * ps).sum(1)[None, :]
        else:
            dist = ((x[:, None, :] - ps[None, :, :]) ** 2).sum(2)
        logits = -(dist - dist.min(1, keepdim=True).values) * inv_tau
        l = F.cross_entropy(logits, t, reduction="sum") / pixels
        l.backward()
        held[name] = (l.detach(), x.grad)

    def torch_assign():
        dist = ((weak[:, None, :] - ps[None, :, :]) ** 2).sum(2)
        held["assign"] = torch.softmax(-(dist - dist.min(1, keepdim=True).values) * inv_tau, dim=1)

    # ---- the two trainers: the same frozen teacher and bank, students with the same weights
    tn, ts = a.train_batch, a.train_size
    torch.manual_seed(0)
    teacher = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    src = torch.randn(tn, 3, ts, ts, generator=g).to(dev)
    tgt_img = torch.randn(tn, 3, ts, ts, generator=g).to(dev)
    masks = torch.randint(0, c, (tn, ts, ts), generator=g).to(dev)
    tbank = PR.PrototypeBank(c, min_pixels=1)
    with torch.no_grad():
        _, dec = teacher.forward_parts(tgt_img, ("logits", "decoder"))
        tbank.accumulate(dec, masks.to(torch.uint8)).update()
    trainers = {}
    for name in ("structure", "distill"):
        torch.manual_seed(1)
        net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).train()
        if name == "structure":
            tr = StructureTrainer(net, dev, teacher, tbank, lambda_src=0.1, lambda_tgt=0.1, tau=0.0)
        else:
            tr = DistillTrainer(net, dev, teacher, tau=0.0, bank=tbank)
        trainers[name] = (tr, FusedAdam(net.parameters(), lr=1e-4))

    legs = {
        "contrast_hard": lambda: fused("hard", labels, None, True),
        "contrast_soft": lambda: fused("soft", None, target, True),
        "contrast_hard_loss_only": lambda: fused("hard_loss_only", labels, None, False),
        "assign": lambda: K.proto_assign(weak, d, d, c, ldc, bank.prototypes, bank.seen, bank.inv_tau, pixels, out),
        "rectify": lambda: K.proto_rectify(feat, d, d, scores, ldc, c, 0, bank.prototypes, bank.seen, bank.inv_tau, pixels, rect),
        "torch_contrast_hard": lambda: torch_contrast(t_hard, "hard"),
        "torch_contrast_soft": lambda: torch_contrast(t_soft, "soft"),
        "torch_contrast_hard_matmul": lambda: torch_contrast(t_hard, "hard_mm", matmul=True),
        "torch_assign": torch_assign,
        "copy_features": lambda: f_dst.copy_(feat),
        "structure_step": lambda: trainers["structure"][0].distill_step(src, masks, tgt_img, trainers["structure"][1]),
        "distill_step": lambda: trainers["distill"][0].distill_step(src, masks, tgt_img, trainers["distill"][1]),
    }
    ms = alternating(legs, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}

    # agreement of the last fused calls with the last torch compositions (fp32 both; the broadcast form)
    fused("hard", labels, None, True)
    agree = {"hard_loss_abs_diff_to_torch": abs(float(loss["hard"]) - float(held["hard"][0])),
             "hard_grad_max_abs_diff_to_torch": float((dfeat - held["hard"][1]).abs().max()),
             "hard_grad_max_abs": float(held["hard"][1].abs().max())}
    fused("soft", None, target, True)
    agree.update({"soft_loss_abs_diff_to_torch": abs(float(loss["soft"]) - float(held["soft"][0])),
                  "soft_grad_max_abs_diff_to_torch": float((dfeat - held["soft"][1]).abs().max()),
                  "assign_max_abs_diff_to_torch": float((out[:, :c][:, seen] - held["assign"]).abs().max()),
                  "loss_hard": float(loss["hard"]), "loss_soft": float(loss["soft"])})
    losses = {k: {kk: round(float(v), 6) for kk, v in trainers[k][0].last_losses.items()} for k in trainers}

    feat_bytes, score_bytes = pixels * d * 4, pixels * ldc * 4
    copy_f = 2 * feat_bytes / (med["copy_features"] * 1e-3) / 1e12
    rate = {
        "contrast_hard": (2 * feat_bytes + pixels) / (med["contrast_hard"] * 1e-3) / 1e12,
        "contrast_soft": (2 * feat_bytes + score_bytes) / (med["contrast_soft"] * 1e-3) / 1e12,
        "assign": (feat_bytes + score_bytes) / (med["assign"] * 1e-3) / 1e12,
        "rectify": (feat_bytes + 2 * score_bytes) / (med["rectify"] * 1e-3) / 1e12,
    }
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r4 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "pixels": [n, h, w], "dim": d, "classes": c, "seen": c - 1, "ldc": ldc, "reps": a.reps, "warmup": a.warmup,
        "train_shape": [tn, 3, ts, ts], "device": torch.cuda.get_device_name(0),
        **{f"{k}_ms": r4(v) for k, v in med.items()},
        **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in legs},
        "contrast_hard_over_torch": r4(med["contrast_hard"] / med["torch_contrast_hard"]),
        "contrast_soft_over_torch": r4(med["contrast_soft"] / med["torch_contrast_soft"]),
        "contrast_hard_over_torch_matmul": r4(med["contrast_hard"] / med["torch_contrast_hard_matmul"]),
        "assign_over_torch": r4(med["assign"] / med["torch_assign"]),
        "contrast_hard_over_copy": r4(med["contrast_hard"] / med["copy_features"]),
        "contrast_soft_over_copy": r4(med["contrast_soft"] / med["copy_features"]),
        "contrast_hard_over_rectify": r4(med["contrast_hard"] / med["rectify"]),
        "assign_over_rectify": r4(med["assign"] / med["rectify"]),
        "structure_step_over_distill_step": r4(med["structure_step"] / med["distill_step"]),
        "copy_features_TB_per_s": r4(copy_f),
        **{f"{k}_TB_per_s": r4(v) for k, v in rate.items()},
        **{f"{k}_fraction_of_copy_rate": r4(v / copy_f) for k, v in rate.items()},
        **agree, "last_losses": losses,
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_contrast.py: prototype contrast loss at 8 x 512 x 512 pixels, D = 16, C = 23 (22 seen) on "
                     "1 x MI355X (HIP-event medians, legs alternating in one process)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write("# The legs run back to back on 32 MB buffers that the last-level cache can hold: the TB/s figures are cache-assisted,\n"
                     "# not HBM rates, and a training step touches far more memory between two calls of the loss.\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
