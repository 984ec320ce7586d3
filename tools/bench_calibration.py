#!/usr/bin/env python
"""Cost of the device-side calibration kernels at the headline batch (cfg 2: 8 x 23 x 512 x 512 logits) on one MI355X.

Seeded logits (padded NHWC, ldc = 24, the buffer Unet.forward hands out) and seeded targets on the device.  HIP-event medians
over --reps calls after --warmup calls, all in ONE process so that the ratios compare like with like:
  * calib_hist_ms     udaseg_calib_hist (accumulating into the same tables), at beta = 1 (NULL) and at a device beta
  * calib_nll_ms      udaseg_calib_nll (kernel + its single-wave finish)
  * calib_finish_ms, calib_step_ms   the two one-block kernels
  * copy_ms           a device copy of the logits' bytes (one read + one write: the memory rate for scale)
  * score_hist_ms     udaseg_score_hist over the same buffer
  * conf_share_ms     udaseg_conf_share over the same buffer: calib_hist reads what it reads plus the targets, and issues three LDS
                      atomics per pixel
  * ce_fwd_ms         udaseg_ce_fwd: `classes` exponentials per pixel, like calib_nll
  * torch_hist_ms     the torch composition of the tables: softmax, max, bucketize, three bincounts
  * torch_fit_iter_ms one autograd iteration of the fit: cross entropy of logits * beta, first and second derivative in beta
  * segmenter_eval_forward_ms   ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch
One JSON line; --out also writes it to a file together with the git HEAD.

    python tools/bench_calibration.py [--reps 50 --warmup 10 --out profiles/calibration_bench.txt]
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
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c, bins = a.batch, a.size, a.size, a.classes, a.bins
    ldc = (c + 3) // 4 * 4
    pixels = n * h * w
    g = torch.Generator().manual_seed(2)
    tb = torch.randint(0, c, (n, h // 8, w // 8), generator=g)
    target = tb.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    z = 1.5 * torch.randn(n, h, w, ldc, generator=g)
    z.scatter_add_(3, target[..., None], 12.0 * torch.rand(n, h, w, 1, generator=g))
    z[..., c:] = 0.0
    buf, tgt = z.to(dev), target.reshape(-1).to(dev)
    tables = torch.zeros(3 * c * bins, dtype=torch.int64, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    inv = torch.full((1,), 0.9, dtype=torch.float32, device=dev)
    f = torch.empty(6 + 4 * c, dtype=torch.float64, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.float64, device=dev)
    ncnt = torch.zeros(3, dtype=torch.int64, device=dev)
    parts = torch.empty(4 * K.seg_partials(), dtype=torch.float64, device=dev)
    hist1 = evented(lambda: K.calib_hist(buf, tgt, pixels, c, ldc, False, None, bins, tables, counters), a.reps, a.warmup)
    histb = evented(lambda: K.calib_hist(buf, tgt, pixels, c, ldc, False, inv, bins, tables, counters), a.reps, a.warmup)
    calls = 2 * (a.reps + a.warmup)
    assert int(counters.sum()) == calls * pixels and int(tables[:c * bins].sum()) == int(counters[0])
    fin = evented(lambda: K.calib_finish(tables, c, bins, f[:6], f[6:]), a.reps, a.warmup)
    nll = evented(lambda: K.calib_nll(buf, tgt, pixels, c, ldc, inv, parts, sums, ncnt), a.reps, a.warmup)
    step_inv = inv.clone()
    step = evented(lambda: K.calib_step(sums, step_inv, state), a.reps, a.warmup)    # one thread: its time is the launch
    dst = torch.empty_like(buf)
    copy = evented(lambda: dst.copy_(buf), a.reps, a.warmup)
    st = torch.zeros(2, c, SCORE_BINS, dtype=torch.int64, device=dev)
    sh = evented(lambda: K.score_hist(buf, tgt, pixels, c, ldc, SCORE_BINS, SCORE_RANGE, st[0], st[1]), a.reps, a.warmup)
    cs_counts = torch.zeros(2, n, dtype=torch.int64, device=dev)
    share = torch.empty(n, dtype=torch.float32, device=dev)
    cs = evented(lambda: K.conf_share(buf, n, h * w, c, ldc, False, 0.9, cs_counts[0], cs_counts[1], share), a.reps, a.warmup)
    lse = torch.empty(pixels, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ce_parts = torch.empty(lib.udaseg_ce_partials(), dtype=torch.float64, device=dev)
    ce = evented(lambda: K.ce_fwd(buf, tgt, pixels, c, ldc, lse, ce_parts, loss), a.reps, a.warmup)

    flat = buf.view(pixels, ldc)[:, :c]
    edges = torch.arange(1, bins, device=dev, dtype=torch.float32) / bins

    def torch_hist():
        p, cls = torch.softmax(flat, dim=1).max(dim=1)
        cell = cls * bins + torch.bucketize(p, edges, right=True)
        return (torch.bincount(cell, minlength=c * bins), torch.bincount(cell, weights=(cls == tgt).double(), minlength=c * bins),
                torch.bincount(cell, weights=p.double(), minlength=c * bins))

    beta = torch.ones((), device=dev, requires_grad=True)

    def torch_fit_iter():
        nll_t = torch.nn.functional.cross_entropy(flat * beta, tgt, reduction="sum")
        g1, = torch.autograd.grad(nll_t, beta, create_graph=True)
        g2, = torch.autograd.grad(g1, beta)
        return g1, g2

    reps_t, warm_t = max(a.reps // 5, 3), max(a.warmup // 5, 2)
    th = evented(torch_hist, reps_t, warm_t)
    tf = evented(torch_fit_iter, reps_t, warm_t)
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)
    with torch.no_grad():
        fwd = evented(lambda: net(x), a.reps, a.warmup)
    logits_bytes = pixels * ldc * 4
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r3 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "logits": [n, c, h, w], "ldc": ldc, "bins": bins, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
        "calib_hist_ms": r3(hist1[0]), "calib_hist_ms_min_max": [r3(hist1[1]), r3(hist1[2])], "calib_hist_beta_ms": r3(histb[0]),
        "calib_nll_ms": r3(nll[0]), "calib_nll_ms_min_max": [r3(nll[1]), r3(nll[2])],
        "calib_finish_ms": r3(fin[0]), "calib_step_ms": r3(step[0]),
        "copy_ms": r3(copy[0]), "score_hist_ms": r3(sh[0]), "conf_share_ms": r3(cs[0]), "ce_fwd_ms": r3(ce[0]),
        "torch_hist_ms": r3(th[0]), "torch_fit_iter_ms": r3(tf[0]), "segmenter_eval_forward_ms": r3(fwd[0]),
        "hist_over_copy": r3(hist1[0] / copy[0]), "hist_over_conf_share": r3(hist1[0] / cs[0]), "hist_over_score_hist": r3(hist1[0] / sh[0]),
        "nll_over_copy": r3(nll[0] / copy[0]), "nll_over_ce_fwd": r3(nll[0] / ce[0]),
        "torch_hist_over_calib_hist": r3(th[0] / hist1[0]), "torch_fit_iter_over_calib_nll": r3(tf[0] / nll[0]),
        "hist_logit_reads_TB_per_s": r3(logits_bytes / (hist1[0] * 1e-3) / 1e12),
        "nll_logit_reads_TB_per_s": r3(logits_bytes / (nll[0] * 1e-3) / 1e12),
        "fit_8_iters_over_eval_forward": r3(8 * (nll[0] + step[0]) / fwd[0]),
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_calibration.py: device-side calibration at the cfg 2 shape on 1 x MI355X (HIP-event medians, one process)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
