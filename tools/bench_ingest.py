#!/usr/bin/env python
"""Device time of the frame-ingest kernels (ingest.py, csrc/resize.hip) on one MI355X, full-size drone frames.

Seeded uint8 frames of --height x --width (4000 x 6000: 72 MB each) and label masks (24 MB each) already on the device, every
output preallocated: the legs time the kernels, not the allocator.  Legs, alternating call by call in ONE process (every round
times each leg once), per leg the median HIP-event time over --reps rounds with min / max, the leg's algorithmic bytes (what it
has to read and write at least: source once, destination once) and GB/s:
  * area_256 / area_512        -- udaseg_resize_area_u8 of one frame to 256 x 256 / 512 x 512;
  * nearest_256 / nearest_512  -- udaseg_resize_nearest_u8 of one mask (algorithmic bytes: the h*w bytes it picks + writes);
  * mask_hist                  -- udaseg_mask_hist_u8 of one mask;
  * normalized_256             -- udaseg_resize_aa_u8 (antialiased bilinear + normalise) of one frame to 256 x 256, fp32;
  * copy                       -- a device-to-device copy of one frame's bytes, THE YARDSTICK: 2 x 72 MB moved.  A kernel's rate
                                  is reported as a share of this copy's measured rate, never of a datasheet figure;
  * segmenter_forward          -- ONE eval-mode r18 Unet forward at 8 x 256 x 256, for scale.
Rotation.  The frames form one pool (--frames, 5 x 72 MB = 360 MB) and the masks another (--masks, 15 x 24 MB = 360 MB), each
with ONE running counter shared by all legs: every frame-reading CALL (area_256, area_512, normalized_256, copy) takes the
next frame of the pool, every mask-reading call (nearest_256, nearest_512, mask_hist) the next mask -- no two calls in a row
read the same source, whichever leg they belong to.  Reuse distance: between two reads of one frame lie the reads of the
four other frames (288 MB) and the copy leg's 72 MB of stores, 360 MB and more against the 256 MiB Infinity Cache; a round has
three mask-reading calls, so a pool of 15 masks meets a mask again after five rounds, each of which moves those 360 MB of
frame traffic besides the masks themselves (more than 1.8 GB between two reads of one mask).  The same legs repeated back to back on
ONE fixed frame / mask are reported too, labelled cache_resident_single_frame: there the source may come from the Infinity
Cache.

    python tools/bench_ingest.py [--reps 30 --warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, data as D, ingest, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


class Pool:
    """Sources handed out in turn from one running counter, or always the first (``fixed``, the cache-resident legs)."""

    def __init__(self, items):
        self.items, self.calls, self.fixed = items, 0, False

    def next(self):
        k = 0 if self.fixed else self.calls % self.items.shape[0]
        self.calls += 1
        return self.items[k:k + 1]


def alternating(legs, reps, warmup):
    """{name: [ms]} with the legs taking turns, each call between its own pair of events."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    return ms


def back_to_back(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [timed(fn) for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--width", type=int, default=6000)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--masks", type=int, default=15)
    a = ap.parse_args()
    _lib.require_gpu()
    H, W = a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(2024)
    frames = torch.randint(0, 256, (a.frames, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    # label masks of large uniform regions (blocks of 125 x 125 pixels), as aerial masks are
    coarse = torch.randint(0, 23, (a.masks, (H + 124) // 125, (W + 124) // 125), generator=g, device="cuda", dtype=torch.uint8)
    masks = coarse.repeat_interleave(125, 1).repeat_interleave(125, 2)[:, :H, :W].contiguous()
    fbytes, mbytes = H * W * 3, H * W
    out = {s: torch.empty((1, s, s, 3), device="cuda", dtype=torch.uint8) for s in (256, 512)}
    out_m = {s: torch.empty((1, s, s), device="cuda", dtype=torch.uint8) for s in (256, 512)}
    hist = torch.zeros((1, 256), device="cuda", dtype=torch.int64)
    out_n = torch.empty((1, 256, 256, 4), device="cuda", dtype=torch.float32)
    ty, tx = ingest._aa_tables(H, W, 256, 256, frames.device)
    m255, r255 = D.normalize_constants()
    dst = torch.empty((H, W, 3), device="cuda", dtype=torch.uint8)
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda().eval()
    x, _ = D.prepare_batch(*D.synthetic_u8_batch(8, 256, 256, seed=1)[:1])

    def forward():
        with torch.no_grad():
            return net(x)

    f, m = Pool(frames), Pool(masks)
    legs = {
        "area_256": lambda: K.resize_area_u8(f.next(), out[256]),
        "area_512": lambda: K.resize_area_u8(f.next(), out[512]),
        "nearest_256": lambda: K.resize_nearest_u8(m.next(), out_m[256]),
        "nearest_512": lambda: K.resize_nearest_u8(m.next(), out_m[512]),
        "mask_hist": lambda: K.mask_hist_u8(m.next(), hist),
        "normalized_256": lambda: K.resize_aa_u8(f.next(), ty, tx, m255, r255, out_n),
        "copy": lambda: dst.copy_(f.next()[0]),
        "segmenter_forward": forward,
    }
    nbytes = {"area_256": fbytes + 256 * 256 * 3, "area_512": fbytes + 512 * 512 * 3, "nearest_256": 2 * 256 * 256,
              "nearest_512": 2 * 512 * 512, "mask_hist": mbytes + 2048, "normalized_256": fbytes + 256 * 256 * 16,
              "copy": 2 * fbytes, "segmenter_forward": None}
    rot = alternating(legs, a.reps, a.warmup)
    f.fixed = m.fixed = True
    res = {k: back_to_back(fn, a.reps, a.warmup) for k, fn in legs.items() if k != "segmenter_forward"}

    def summary(ms):
        med = {k: statistics.median(v) for k, v in ms.items()}
        rate = {k: nbytes[k] / med[k] / 1e6 for k in med if nbytes[k]}
        return {"ms": {k: round(v, 4) for k, v in med.items()},
                "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                "gb_per_s": {k: round(v, 1) for k, v in rate.items()},
                "share_of_copy_rate": {k: round(v / rate["copy"], 3) for k, v in rate.items()
                                       if k in ("area_256", "area_512", "mask_hist", "normalized_256")}}

    print(json.dumps({"frame": [H, W], "frames": a.frames, "masks": a.masks, "reps": a.reps,
                      "source_bytes_rotated": {"frames": a.frames * fbytes, "masks": a.masks * mbytes},
                      "algorithmic_bytes": nbytes, "rotating": summary(rot), "cache_resident_single_frame": summary(res)}),
          flush=True)


if __name__ == "__main__":
    main()
