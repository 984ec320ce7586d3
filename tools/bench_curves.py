#!/usr/bin/env python
"""Cost of the device-side ROC / PR curves at the headline batch (cfg 2: 8 x 23 x 512 x 512 logits) on one MI355X.

Seeded logits (padded NHWC, ldc = 24, the buffer Unet.forward hands out) and seeded targets on the device.  HIP-event medians
over --reps calls after --warmup calls, all in ONE process so that the ratios compare like with like:
  * score_hist_ms     udaseg_score_hist (accumulating into the same two tables)
  * curve_finish_ms   udaseg_curve_finish
  * ce_fwd_ms         the cross-entropy forward (udaseg_ce_fwd) over the same buffer: one read of the logits + one lse write
  * segmenter_forward_ms   ONE training-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch
  * confusion_ms      udaseg_argmax_confusion over the same buffer (the other per-batch metric kernel), for scale
The bar: score_hist + curve_finish < one segmenter forward.  hist_over_ce is reported, not judged: with G class groups the
histogram reads the logits and the targets G times, the cross-entropy forward reads them once and writes one float per pixel;
memory_floor_ratio is that ratio of bytes.  hist_over_ce near it means the pass is at its memory floor; a much larger one means
the LDS atomics set the time.  One JSON line; --out also writes it to a file
together with the git HEAD.

    python tools/bench_curves.py [--reps 50 --warmup 10 --out profiles/curves_bench.txt]
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
from uda_aerial_semantic_segmentation_research_amd.curves import SCORE_BINS, SCORE_RANGE  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def evented(fn, reps, warmup):
    """Median (and min / max) HIP-event time of ``fn()`` over ``reps`` calls, each bracketed by its own pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--bins", type=int, default=SCORE_BINS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c = a.batch, a.size, a.size, a.classes
    ldc = (c + 3) // 4 * 4
    pixels = n * h * w
    g = torch.Generator().manual_seed(2)
    tb = torch.randint(0, c, (n, h // 8, w // 8), generator=g)
    target = tb.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    z = 1.5 * torch.randn(n, h, w, ldc, generator=g)
    z.scatter_add_(3, target[..., None], 12.0 * torch.rand(n, h, w, 1, generator=g))
    z[..., c:] = 0.0
    buf, tgt = z.to(dev), target.reshape(-1).to(dev)
    tables = torch.zeros(2, c, a.bins, dtype=torch.int64, device=dev)
    f = torch.empty(3, c, dtype=torch.float64, device=dev)
    support = torch.empty(c, 2, dtype=torch.int64, device=dev)
    lse = torch.empty(pixels, dtype=torch.float32, device=dev)
    partials = torch.empty(lib.udaseg_ce_partials(), dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    cm = torch.zeros(c * c, dtype=torch.int64, device=dev)
    hist = evented(lambda: K.score_hist(buf, tgt, pixels, c, ldc, a.bins, SCORE_RANGE, tables[0], tables[1]), a.reps, a.warmup)
    fin = evented(lambda: K.curve_finish(tables[0], tables[1], c, a.bins, f[0], f[1], f[2], support), a.reps, a.warmup)
    ce = evented(lambda: K.ce_fwd(buf, tgt, pixels, c, ldc, lse, partials, loss), a.reps, a.warmup)
    conf = evented(lambda: K.argmax_confusion(buf, tgt, pixels, c, ldc, cm), a.reps, a.warmup)
    calls = a.reps + a.warmup
    assert int(tables.sum()) == calls * pixels * c and int(support.sum()) == calls * pixels * c
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).train()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)
    with torch.no_grad():
        fwd = evented(lambda: net(x), a.reps, a.warmup)
    cg = 8192 // a.bins
    groups = (c + cg - 1) // cg
    logits_bytes = pixels * ldc * 4
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r3 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "logits": [n, c, h, w], "ldc": ldc, "bins": a.bins, "score_range": SCORE_RANGE, "class_groups": groups,
        "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
        "score_hist_ms": r3(hist[0]), "score_hist_ms_min_max": [r3(hist[1]), r3(hist[2])],
        "curve_finish_ms": r3(fin[0]), "ce_fwd_ms": r3(ce[0]), "confusion_ms": r3(conf[0]),
        "segmenter_forward_ms": r3(fwd[0]), "segmenter_forward_ms_min_max": [r3(fwd[1]), r3(fwd[2])],
        "curves_ms": r3(hist[0] + fin[0]), "curves_over_forward": r3((hist[0] + fin[0]) / fwd[0]),
        "curves_below_one_forward": bool(hist[0] + fin[0] < fwd[0]),
        "hist_over_ce": r3(hist[0] / ce[0]), "memory_floor_ratio": r3(groups * (logits_bytes + 8 * pixels) / (logits_bytes + 12 * pixels)),
        "hist_logit_reads_TB_per_s": r3(groups * logits_bytes / (hist[0] * 1e-3) / 1e12),
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_curves.py: device-side ROC / PR curves at the cfg 2 shape on 1 x MI355X (HIP-event medians, one process)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
