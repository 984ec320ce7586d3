#!/usr/bin/env python
"""Cost of the region products at the headline batch (8 x 512 x 512 uint8 masks, 23 classes) on one MI355X, for a smooth and a
speckled map.

Seeded masks: "smooth" is block-constant (16 x 16 blocks of one class, 5 % of the blocks void) as in tools/bench_boundary.py;
"speckled" is the same map with a tenth of its pixels relabelled one by one, the islands a sieve is for.  HIP-event medians over
--reps rounds after --warmup rounds; the legs ALTERNATE inside every round, all in ONE process, and every leg runs --inner
back-to-back calls between its two events and reports the time PER CALL.  Back-to-back calls on the same 2 MB of masks are
cache-assisted: the figures are those of a mask that is already in L2 / Infinity Cache, which is how a loader meets it (the labeler
has just written it).  Per map, at 4- and at 8-connectivity:
  * label_ms         udaseg_regions_label with areas (every launch of it: tile, merge levels, resolve, finish), outputs preallocated
  * sieve_ms         regions.sieve: the labelling, then udaseg_regions_sieve with its counters (allocates ids, area and the mask)
  * stats_ms         RegionStats.update: the labelling, then udaseg_regions_stats
and once per map, beside them in every round:
  * copy_ms          a device-to-device copy that reads and writes what label reads and writes (1 + 4 + 4 bytes per pixel)
  * erode3_ms        boundary.erode at radius 3 of the same mask
  * scipy_ms         where scipy imports: the mask copied to the host and scipy.ndimage.label run per image and class (wall clock,
                     --scipy-reps runs, the copy included): the only way to the same partition without this module
and once:
  * forward_eval_ms  ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch (its own rounds)
Reported, not judged.  One JSON line; --out also writes it to a file together with the git HEAD.  The process ends itself after
--time-limit seconds.

    python tools/bench_regions.py [--reps 20 --warmup 3 --inner 10 --out profiles/regions_bench.txt]
"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import boundary as B, regions as G  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402

MIN_AREA = 32


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


def scipy_components(masks, connectivity, reps):
    """(median wall-clock ms of host copy + scipy.ndimage.label per image and class, components found) or (None, None)."""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None, None
    st = np.ones((3, 3), dtype=int) if connectivity == 8 else None
    times, total = [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = masks.cpu().numpy()
        total = 0
        for img in host:
            for c in np.unique(img):
                if c != 255:
                    total += ndi.label(img == c, structure=st)[1]
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--scipy-reps", type=int, default=2)
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
    smooth = blocks.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().to(torch.uint8)
    speck = smooth.clone()
    hit = torch.rand(n, h, w, generator=g) < 0.1
    speck[hit] = torch.randint(0, c, (int(hit.sum()),), generator=g).to(torch.uint8)
    ids = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    area = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    er = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    counts = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    copy_src = torch.randint(0, 256, (pixels * 9 // 2,), generator=g, dtype=torch.uint8).to(dev)
    copy_dst = torch.empty_like(copy_src)
    r4 = lambda v: round(v, 4)      # noqa: E731
    res = {}
    for name, host in (("smooth", smooth), ("speckled", speck)):
        masks = host.to(dev)
        out = {}
        for conn in (4, 8):
            stats = G.RegionStats(c, conn, 255, dev)
            legs = {
                "label": lambda: K.regions_label(masks, conn, 255, ids, area),
                "sieve": lambda: G.sieve(masks, MIN_AREA, conn, counts=counts),
                "stats": lambda: stats.update(masks),
                "copy": lambda: copy_dst.copy_(copy_src),
                "erode3": lambda: K.boundary_erode(masks, 3, 255, 255, er, None),
            }
            ms = alternating(legs, a.reps, a.warmup, {k: a.inner for k in legs})
            med = {k: statistics.median(v) for k, v in ms.items()}
            counts.zero_()
            sieved = G.sieve(masks, MIN_AREA, conn, counts=counts)
            cnt = counts.sum(0).tolist()
            sc_ms, sc_total = scipy_components(masks, conn, a.scipy_reps)
            if sc_total is not None:
                assert sc_total == cnt[1] + cnt[2], f"{name}/{conn}: scipy finds {sc_total} components, the sieve counted {cnt[1] + cnt[2]}"
            out[f"c{conn}"] = {
                **{f"{k}_ms": r4(v) for k, v in med.items()},
                **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
                "label_over_copy": r4(med["label"] / med["copy"]), "label_over_erode3": r4(med["label"] / med["erode3"]),
                "sieve_over_erode3": r4(med["sieve"] / med["erode3"]),
                "scipy_ms": None if sc_ms is None else r4(sc_ms), "scipy_over_label": None if sc_ms is None else r4(sc_ms / med["label"]),
                "components": cnt[1] + cnt[2], "removed": cnt[1], "voided_share": r4(float((sieved != masks).sum()) / pixels),
            }
            print(f"{name} connectivity {conn}: " + json.dumps(out[f"c{conn}"]), flush=True)
        res[name] = out

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)

    def forward_leg():
        with torch.no_grad():
            net(x)

    fwd = alternating({"forward_eval": forward_leg}, a.reps, a.warmup, {"forward_eval": 3})["forward_eval"]
    fwd_ms = statistics.median(fwd)
    for out in res.values():
        for v in out.values():
            v["label_over_forward"] = round(v["label_ms"] / fwd_ms, 4)
            v["sieve_over_forward"] = round(v["sieve_ms"] / fwd_ms, 4)
            v["stats_over_forward"] = round(v["stats_ms"] / fwd_ms, 4)
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = json.dumps({"masks": [n, h, w], "classes": c, "min_area": MIN_AREA, "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
                       "scipy_reps": a.scipy_reps, "tile": list(K.regions_tile()), "device": torch.cuda.get_device_name(0),
                       "forward_eval_ms": round(fwd_ms, 4), "forward_eval_ms_min_max": [round(fwd[0], 4), round(fwd[-1], 4)], **res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_regions.py: region labelling, sieve and statistics at 8 x 512 x 512 uint8 masks, 23 classes, "
                     "on 1 x MI355X (HIP-event medians per call, legs alternating in one process, back-to-back calls: cache-assisted; "
                     "scipy_ms is wall clock on the host, copy included)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
