#!/usr/bin/env python
"""Cost of the device-side class-balanced pseudo-labels at the headline batch (8 x 23 x 512 x 512 logits) on one MI355X.

Seeded logits in the padded NHWC buffer Unet.forward hands out (ldc = 24; bench_curves.py's recipe: 1.5 * randn plus 12 * rand on
a block-constant winner, so confident pixels pile into the top bins of their class).  HIP-event medians over --reps rounds after
--warmup rounds; the legs ALTERNATE inside every round, all in ONE process, so that the ratios compare like with like:
  * conf_hist_ms           udaseg_conf_hist (accumulating into the same table)
  * pseudo_thresholds_ms   udaseg_pseudo_thresholds
  * pseudo_labels_ms       udaseg_pseudo_labels (uint8 masks, no confidence map)
  * torch_ms               the torch composition of the same result on the same buffer, sync-free: softmax -> max -> ONE sort of
                           the float64 key 2 * class + p over all pixels (per-class order in one go; torch.quantile per class would
                           need a boolean gather, i.e. a host sync per class, and refuses more than 2^24 elements) -> per-class
                           quantile element by bincount offsets -> where -> uint8.  No subsampling: every pixel is sorted.
  * forward_eval_ms        ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch
  * copy_ms                a device-to-device copy of the same buffer (reads and writes its bytes once each)
Bars, judged on this run's own numbers: conf_hist + pseudo_labels < torch composition, and < one eval forward.  Reported, not
judged: each pixel kernel's rate over the scores as a fraction of the copy's rate (bytes moved / time).  One JSON line; --out also
writes it to a file together with the git HEAD.

    python tools/bench_pseudo.py [--reps 30 --warmup 5 --out profiles/pseudo_bench.txt]
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
from uda_aerial_semantic_segmentation_research_amd import pseudo as P  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--bins", type=int, default=P.BINS)
    ap.add_argument("--portion", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c = a.batch, a.size, a.size, a.classes
    ldc = (c + 3) // 4 * 4
    pixels = n * h * w
    g = torch.Generator().manual_seed(2)
    tb = torch.randint(0, c, (n, h // 8, w // 8), generator=g)
    winner = tb.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    z = 1.5 * torch.randn(n, h, w, ldc, generator=g)
    z.scatter_add_(3, winner[..., None], 12.0 * torch.rand(n, h, w, 1, generator=g))
    z[..., c:] = 0.0
    buf = z.to(dev)
    table = torch.zeros(c * a.bins + 1, dtype=torch.int64, device=dev)
    hist, nonfinite = table[:-1], table[-1:]
    portion = torch.full((c,), a.portion, dtype=torch.float64, device=dev)
    k_cap = P.bin_of(0.9, a.bins)
    thr = torch.zeros(c, dtype=torch.int32, device=dev)
    support = torch.zeros(c, dtype=torch.int64, device=dev)
    labels = torch.empty(pixels, dtype=torch.uint8, device=dev)
    counts = torch.zeros(c + 2, dtype=torch.int64, device=dev)
    dst = torch.empty_like(buf)
    K.conf_hist(buf, pixels, c, ldc, 0, a.bins, hist, nonfinite)                      # a table for the threshold leg to read
    K.pseudo_thresholds(hist, c, a.bins, portion, 0, k_cap, thr, support)
    table.zero_()
    rows = buf.view(pixels, ldc)[:, :c]
    cap = torch.tensor(0.9, device=dev)
    void = torch.tensor(255, device=dev)
    held = {}

    def torch_leg():
        p, cls = torch.softmax(rows, dim=1).max(dim=1)
        key, _ = torch.sort(2.0 * cls.double() + p.double())
        n_c = torch.bincount(cls, minlength=c)
        end = torch.cumsum(n_c, 0)
        need = torch.ceil(a.portion * n_c.double()).long().clamp(min=1)
        at = (end - need).clamp(min=0, max=pixels - 1)
        t = (key[at] - 2.0 * torch.arange(c, device=dev, dtype=torch.float64)).float()
        t = torch.minimum(t, cap)
        held["labels"] = torch.where(p >= t[cls], cls, void).to(torch.uint8)

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)

    def forward_leg():
        with torch.no_grad():
            net(x)

    legs = {
        "conf_hist": lambda: K.conf_hist(buf, pixels, c, ldc, 0, a.bins, hist, nonfinite),
        "pseudo_thresholds": lambda: K.pseudo_thresholds(hist, c, a.bins, portion, 0, k_cap, thr, support),
        "pseudo_labels": lambda: K.pseudo_labels(buf, pixels, c, ldc, 0, a.bins, thr, 255, labels, None, counts),
        "torch": torch_leg,
        "forward_eval": forward_leg,
        "copy": lambda: dst.copy_(buf),
    }
    ms = alternating(legs, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    calls = a.reps + a.warmup
    assert int(hist.sum()) + int(nonfinite) == calls * pixels and int(counts[:c + 1].sum()) == calls * pixels
    agree = float((held["labels"] == labels).float().mean())     # the two differ only where p sits within a bin of its threshold
    kept_share = float(counts[:c].sum()) / float(counts[:c + 1].sum())
    score_bytes = pixels * ldc * 4
    copy_rate = 2 * score_bytes / (med["copy"] * 1e-3) / 1e12
    hist_rate = score_bytes / (med["conf_hist"] * 1e-3) / 1e12
    label_rate = (score_bytes + pixels) / (med["pseudo_labels"] * 1e-3) / 1e12
    ours = med["conf_hist"] + med["pseudo_labels"]
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r4 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "logits": [n, c, h, w], "ldc": ldc, "bins": a.bins, "portion": a.portion, "reps": a.reps, "warmup": a.warmup,
        "device": torch.cuda.get_device_name(0),
        **{f"{k}_ms": r4(v) for k, v in med.items()},
        **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ("conf_hist", "pseudo_labels", "torch", "forward_eval", "copy")},
        "hist_plus_labels_ms": r4(ours), "pipeline_ms": r4(ours + med["pseudo_thresholds"]),
        "over_torch": r4(ours / med["torch"]), "faster_than_torch": bool(ours < med["torch"]),
        "over_forward": r4(ours / med["forward_eval"]), "below_one_eval_forward": bool(ours < med["forward_eval"]),
        "copy_TB_per_s": r4(copy_rate), "conf_hist_TB_per_s": r4(hist_rate), "pseudo_labels_TB_per_s": r4(label_rate),
        "conf_hist_fraction_of_copy_rate": r4(hist_rate / copy_rate),
        "pseudo_labels_fraction_of_copy_rate": r4(label_rate / copy_rate),
        "kept_share": r4(kept_share), "labels_agree_with_torch": r4(agree),
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_pseudo.py: class-balanced pseudo-labels at 8 x 23 x 512 x 512 on 1 x MI355X "
                     "(HIP-event medians, legs alternating in one process)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
