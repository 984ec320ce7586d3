#!/usr/bin/env python
"""Cost of the label boundary products at the headline batch (8 x 512 x 512 uint8 masks, 23 classes) on one MI355X, for the radii
1, 5, 15 and 32.

Seeded block-constant masks (16 x 16 blocks of one class, 5 % of the blocks void) as in tools/bench_mix.py; the prediction of the
counters' leg is the mask moved by (2, 1) pixels.  HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE
inside every round, all in ONE process, and every leg runs --inner back-to-back calls between its two events and reports the time
PER CALL.  Back-to-back calls on the same 2 MB of masks are cache-assisted: the figures are those of a mask that is already in
L2 / Infinity Cache, which is how a loader meets it (the labeler has just written it).  Per radius:
  * d2_ms / lookup_ms / erode_ms / stats_ms   the four entry points (udaseg_boundary_*), outputs preallocated
  * torch_erode_ms   the exact torch composition of erode: boundary flags by shifted compares, conv2d of the flags with the disc of
                     the radius (fp32, sums of at most 3209 ones: exact), > 0, where.  Its result is compared with erode's (equal).
and once, beside them in every round:
  * copy5_ms / copy2_ms   a device-to-device copy that reads and writes what d2 and lookup (1 + 4 bytes per pixel) and what erode and
                          the counters (1 + 1 and 2 + 0 bytes per pixel) read and write
  * forward_eval_ms       ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch (its own rounds)
Reported, not judged.  One JSON line; --out also writes it to a file together with the git HEAD.  The process ends itself after
--time-limit seconds.

    python tools/bench_boundary.py [--reps 20 --warmup 3 --inner 10 --out profiles/boundary_bench.txt]
"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import boundary as B  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402

RADII = (1, 5, 15, 32)


def alternating(legs, reps, warmup, inner):
    """{name: sorted HIP-event times per call in ms}: every round runs each leg once, in order, `inner[name]` calls between two events."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner[k]):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / inner[k])
    return {k: sorted(v) for k, v in ms.items()}


def torch_erode(m, r, disc, void=255):
    """The exact torch composition of boundary.erode(m, r, void): void is no label, the frame's edge no boundary."""
    live = m != void
    f = torch.zeros_like(live)
    d = (m[:, :, 1:] != m[:, :, :-1]) & live[:, :, 1:] & live[:, :, :-1]
    f[:, :, 1:] |= d
    f[:, :, :-1] |= d
    d = (m[:, 1:] != m[:, :-1]) & live[:, 1:] & live[:, :-1]
    f[:, 1:] |= d
    f[:, :-1] |= d
    hit = torch.nn.functional.conv2d(f[:, None].float(), disc, padding=r)[:, 0] > 0.5
    return torch.where(hit & live, torch.full_like(m, void), m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-inner", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    signal.alarm(a.time_limit)
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c = a.batch, a.size, a.size, a.classes
    pixels = n * h * w
    g = torch.Generator().manual_seed(2)
    blocks = torch.randint(0, c, (n, h // 16, w // 16), generator=g)
    blocks[torch.rand(n, h // 16, w // 16, generator=g) < 0.05] = 255
    masks = blocks.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().to(torch.uint8).to(dev)
    pred = torch.roll(masks, (2, 1), (1, 2)).contiguous()
    d2 = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    wm = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    er = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    counts = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    stats = torch.zeros(3 * c + 2, dtype=torch.int64, device=dev)
    copy5_src = torch.randint(0, 256, (pixels * 5 // 2,), generator=g, dtype=torch.uint8).to(dev)
    copy5_dst = torch.empty_like(copy5_src)
    copy2_src = torch.randint(0, 256, (pixels,), generator=g, dtype=torch.uint8).to(dev)
    copy2_dst = torch.empty_like(copy2_src)
    held = {}
    res = {}
    for r in RADII:
        tab = torch.from_numpy(B.unet_table(r)).to(dev)
        yy, xx = torch.meshgrid(torch.arange(-r, r + 1), torch.arange(-r, r + 1), indexing="ij")
        disc = ((yy * yy + xx * xx) <= r * r).float()[None, None].to(dev)

        def torch_leg():
            held["torch"] = torch_erode(masks, r, disc)

        legs = {
            "d2": lambda: K.boundary_d2(masks, r, 255, d2),
            "lookup": lambda: K.boundary_lookup(masks, r, 255, tab, wm),
            "erode": lambda: K.boundary_erode(masks, r, 255, 255, er, counts),
            "stats": lambda: K.boundary_stats(pred, masks, r, c, 255, stats[:3 * c], stats[3 * c:]),
            "torch_erode": torch_leg,
            "copy5": lambda: copy5_dst.copy_(copy5_src),
            "copy2": lambda: copy2_dst.copy_(copy2_src),
        }
        inner = {k: a.inner for k in legs}
        inner["torch_erode"] = a.torch_inner
        ms = alternating(legs, a.reps, a.warmup, inner)
        assert torch.equal(held["torch"], er), f"radius {r}: the torch composition and erode differ"
        assert torch.equal(er, B.erode(masks, r)) and int((d2 == 0).sum()) > 0
        med = {k: statistics.median(v) for k, v in ms.items()}
        r4 = lambda v: round(v, 4)      # noqa: E731
        res[f"r{r}"] = {
            **{f"{k}_ms": r4(v) for k, v in med.items()},
            **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
            "d2_over_copy5": r4(med["d2"] / med["copy5"]), "lookup_over_copy5": r4(med["lookup"] / med["copy5"]),
            "erode_over_copy2": r4(med["erode"] / med["copy2"]), "stats_over_copy2": r4(med["stats"] / med["copy2"]),
            "erode_over_torch": r4(med["erode"] / med["torch_erode"]),
            "tile": list(K.boundary_tile(r)), "voided_share": r4(float((er != masks).sum()) / pixels),
        }
        print(f"radius {r}: " + json.dumps(res[f"r{r}"]), flush=True)

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)

    def forward_leg():
        with torch.no_grad():
            net(x)

    fwd = alternating({"forward_eval": forward_leg}, a.reps, a.warmup, {"forward_eval": 3})["forward_eval"]
    fwd_ms = statistics.median(fwd)
    for r in RADII:
        v = res[f"r{r}"]
        v["erode_over_forward"] = round(v["erode_ms"] / fwd_ms, 4)
        v["stats_over_forward"] = round(v["stats_ms"] / fwd_ms, 4)
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = json.dumps({"masks": [n, h, w], "classes": c, "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
                       "torch_inner": a.torch_inner, "device": torch.cuda.get_device_name(0),
                       "forward_eval_ms": round(fwd_ms, 4), "forward_eval_ms_min_max": [round(fwd[0], 4), round(fwd[-1], 4)], **res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_boundary.py: label boundary products at 8 x 512 x 512 uint8 masks, 23 classes, on 1 x MI355X "
                     "(HIP-event medians per call, legs alternating in one process, back-to-back calls: cache-assisted)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
