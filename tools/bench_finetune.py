#!/usr/bin/env python
"""Phase-3 (unsupervised fine-tuning) iteration rate on one MI355X: UnsupervisedTrainer.finetune_step.

Unet r18 (23 classes, random init) + the domain discriminator, 8 x 512 x 512 seeded uint8 target frames already on the device,
fresh augmentation records every iteration, FusedAdam, fp32 and bf16 storage.  Per leg, one JSON line:
  * iters_per_s      -- iterations / host-clock seconds around a synchronised window of --steps iterations (after --warmup);
  * device_ms        -- HIP-event time of the phases of --reps further iterations (median per phase): augment (both views + the
                        normalised plain batch), forward (two segmenter forwards + the discriminator), loss (FineTuningLoss and
                        the iteration's one host read), backward, clip, adam;
  * augment_ms       -- data.strong_views alone (both views), and segmenter_forward_ms -- ONE training-mode segmenter forward of
                        the same batch alone, both as medians of --reps evented calls: the augmentation of both views has to
                        cost less than that forward.

    python tools/bench_finetune.py [--steps 30 --warmup 5 --reps 10 --dtypes float32,bfloat16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, data as D  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unsupervised_trainer import UnsupervisedTrainer  # noqa: E402


def split(events):
    """[(phase, event)] -> {phase: ms}: each interval is charged to the mark that opens it ("end" closes the iteration)."""
    torch.cuda.synchronize()
    out = {}
    for (kind, a), (_, b) in zip(events, events[1:]):
        if kind != "end":
            out[kind] = out.get(kind, 0.0) + a.elapsed_time(b)
    return out


def evented(fn, reps):
    """Median HIP-event time of ``fn()`` over ``reps`` calls, each bracketed by its own pair of events."""
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--encoder", default="resnet18")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w = a.batch, a.size, a.size
    frames, _ = D.synthetic_u8_batch(n, h, w, seed=2024)
    for name in a.dtypes.split(","):
        dtype = getattr(torch, name)
        torch.manual_seed(0)
        net = Unet(a.encoder, encoder_weights=None, in_channels=3, classes=23, compute_dtype=dtype)
        tr = UnsupervisedTrainer(net, dev, rampup_length=1, seed=7)
        tr.model.train()
        opt = FusedAdam(tr.model.parameters(), lr=1e-4)
        step = lambda ev=None: tr.finetune_step(frames, opt, 1, update_metrics=False, _events=ev)      # noqa: E731
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        phases = {}
        for _ in range(a.reps):
            ev = []
            step(ev)
            for k, v in split(ev).items():
                phases.setdefault(k, []).append(v)
        device = {k: statistics.median(v) for k, v in phases.items()}
        g = torch.Generator().manual_seed(1)
        pa, pb = D.draw_strong_params(n, h, w, g), D.draw_strong_params(n, h, w, g)
        off = D.StrongAugParams(n, h, w)
        aug_ms = evented(lambda: D.strong_views(frames, pa, pb, dtype=dtype), a.reps)
        aug_off_ms = evented(lambda: D.strong_views(frames, off, off, dtype=dtype), a.reps)
        x, _ = D.prepare_batch(frames, dtype=dtype)
        seg = tr.model.segmentation_model
        with torch.no_grad():
            fwd_ms = evented(lambda: seg(x), a.reps)
        print(json.dumps({
            "encoder": a.encoder, "dtype": name, "batch": [n, h, w], "steps": a.steps, "skipped": tr.skipped,
            "iters_per_s": round(a.steps / wall, 2), "iter_ms_host_clock": round(1e3 * wall / a.steps, 3),
            "device_ms": {k: round(v, 3) for k, v in sorted(device.items())}, "device_ms_total": round(sum(device.values()), 3),
            "augment_ms_both_views": round(aug_ms, 3), "augment_ms_both_views_all_stages_off": round(aug_off_ms, 3),
            "segmenter_forward_ms": round(fwd_ms, 3), "augment_below_one_forward": bool(aug_ms < fwd_ms),
            "stage_flags_view_a": [int(f) for f in pa.flags], "stage_flags_view_b": [int(f) for f in pb.flags],
        }), flush=True)
        del tr, net, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
