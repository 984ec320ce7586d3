#!/usr/bin/env python
"""Device time of the labelled training augmentation (data.train_batch) on one MI355X, against what it has to keep up with.

8 x 512 x 512 seeded uint8 frames and masks already on the device, fp32 and bf16 output.  Per leg, one JSON line with the median
HIP-event time (ms) of --reps calls, each bracketed by its own pair of events:
  * train_batch_drawn     -- fresh records from draw_training_params every call (the host-side draw is inside the bracket, as in
                             training; the device waits for it only if it is idle);
  * train_batch_drawn_fixed -- the same with one set of drawn records reused (kernel time of a typical batch);
  * train_batch_off       -- every stage off (one pass, prepare_batch's arithmetic plus the record load);
  * train_batch_worst     -- every sample on elastic + affine (field pass, then the composed gather: the distortion stage at its dearest);
  * prepare_batch         -- D4 + Normalize alone;
  * segmenter_forward     -- ONE training-mode r18 Unet forward of the same batch.
The claim to check: the drawn-records call costs less device time than that forward (ratio reported, worst case too).

    python tools/bench_train_aug.py [--reps 20 --warmup 3 --dtypes float32,bfloat16]
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

from uda_aerial_semantic_segmentation_research_amd import _lib, data as D  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def evented(fn, reps, warmup):
    """Median HIP-event time of ``fn()`` over ``reps`` calls, each bracketed by its own pair of events."""
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
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--encoder", default="resnet18")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    a = ap.parse_args()
    _lib.require_gpu()
    n, h, w = a.batch, a.size, a.size
    frames, masks = D.synthetic_u8_batch(n, h, w, seed=2024)
    off = D.TrainAugParams(n, h, w)
    worst = D.TrainAugParams(n, h, w)
    for i in range(n):
        t = i / max(n - 1, 1)
        worst.set_affine(i, (2 * t - 1) * 0.06 * w + 0.1372, (1 - 2 * t) * 0.06 * h - 0.0913, 0.81 + 0.37 * t, -43.0 + 83.0 * t)
        worst.set_elastic(i, 120.0, (1234 + i, 5678))
    fixed = D.draw_training_params(n, h, w, torch.Generator().manual_seed(1))
    for name in a.dtypes.split(","):
        dtype = getattr(torch, name)
        torch.manual_seed(0)
        net = Unet(a.encoder, encoder_weights=None, in_channels=3, classes=23, compute_dtype=dtype).cuda().train()
        g = torch.Generator().manual_seed(7)
        legs = {
            "train_batch_drawn": lambda: D.train_batch(frames, masks, None, g, dtype),
            "train_batch_drawn_fixed": lambda: D.train_batch(frames, masks, fixed, dtype=dtype),
            "train_batch_off": lambda: D.train_batch(frames, masks, off, dtype=dtype),
            "train_batch_worst": lambda: D.train_batch(frames, masks, worst, dtype=dtype),
            "prepare_batch": lambda: D.prepare_batch(frames, masks, dtype=dtype),
        }
        ms = {k: evented(fn, a.reps, a.warmup) for k, fn in legs.items()}
        x, _ = D.prepare_batch(frames, masks, dtype=dtype)
        with torch.no_grad():
            ms["segmenter_forward"] = evented(lambda: net(x), a.reps, a.warmup)
        fwd = ms["segmenter_forward"]
        print(json.dumps({
            "encoder": a.encoder, "dtype": name, "batch": [n, h, w], "reps": a.reps,
            "ms": {k: round(v, 3) for k, v in ms.items()},
            "drawn_over_forward": round(ms["train_batch_drawn"] / fwd, 3),
            "worst_over_forward": round(ms["train_batch_worst"] / fwd, 3),
            "drawn_below_one_forward": bool(ms["train_batch_drawn"] < fwd),
            "worst_below_one_forward": bool(ms["train_batch_worst"] < fwd),
            "stage_flags_fixed": [int(f) for f in fixed.flags], "distortion_fixed": [int(k) for k in fixed.distortion],
        }), flush=True)
        del net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
