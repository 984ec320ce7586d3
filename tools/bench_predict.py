#!/usr/bin/env python
"""Large-frame prediction throughput (predict.predict_large) on one MI355X.

A seeded 4000 x 6000 uint8 frame already on the device; Unet r18 and r50 (23 classes, fp32, random init), tile 512,
overlap 0.25, batch 8, tta None and "d4".  Per leg, one JSON line:
  * mpix_per_s     -- frame megapixels / host-clock seconds around a synchronised call (warmed up, median of --reps);
  * device_ms      -- HIP-event time of the call's phases: model forwards, and the new kernels (gather, blend, finish);
  * kernel_share   -- gather + blend + finish over the device total;
  * blend_gbs      -- the blend's bytes (computed from shapes: logits read once, accumulator + weight read and written over
                      each batch's bounding box) over its event time.

    python tools/bench_predict.py [--h 4000 --w 6000 --reps 5 --encoders resnet18,resnet50 --tta none,d4]
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

from uda_aerial_semantic_segmentation_research_amd import _lib, predict as P  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.engine import ceil4  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def blend_bytes(g, views, per_fwd, classes, ldc):
    """Bytes the blend kernel moves over one call: every view's logits row (ldc fp32) read once, and per batch the
    accumulator row (ceil4(C) fp32) + weight read and written over the batch's bounding box (as the kernel's launch grid)."""
    ldp = ceil4(classes)
    n = g.rows * g.cols
    total = n * views * g.th * g.tw * ldc * 4
    org = lambda i, s, L, t: max(0, min(i * s, L - t))                  # noqa: E731
    for first in range(0, n, per_fwd):
        last = min(n, first + per_fwd) - 1
        i0, i1 = first // g.cols, last // g.cols
        y0, y1 = org(i0, g.sy, g.h, g.th), min(g.h, org(i1, g.sy, g.h, g.th) + g.th)
        x0, x1 = 0, g.w
        if i0 == i1:
            x0, x1 = org(first % g.cols, g.sx, g.w, g.tw), min(g.w, org(last % g.cols, g.sx, g.w, g.tw) + g.tw)
        total += (y1 - y0) * (x1 - x0) * (ldp + 1) * 4 * 2
    return total


def split(events):
    """[(kind, event)] -> {kind: ms}: each interval is charged to the mark that opens it ("end" closes a phase)."""
    torch.cuda.synchronize()
    out = {}
    for (kind, a), (_, b) in zip(events, events[1:]):
        if kind != "end":
            out[kind] = out.get(kind, 0.0) + a.elapsed_time(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=4000)
    ap.add_argument("--w", type=int, default=6000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--encoders", default="resnet18,resnet50")
    ap.add_argument("--tta", default="none,d4")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=float, default=0.25)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    g0 = torch.Generator(device=dev).manual_seed(2024)
    frame = torch.randint(0, 256, (a.h, a.w, 3), generator=g0, device=dev, dtype=torch.uint8)
    mpix = a.h * a.w / 1e6
    for enc in a.encoders.split(","):
        torch.manual_seed(0)
        model = Unet(enc, encoder_weights=None, in_channels=3, classes=23).to(dev).eval()
        for tta in a.tta.split(","):
            tta = None if tta == "none" else tta
            kw = dict(tile=a.tile, overlap=a.overlap, batch_size=a.batch, tta=tta)
            for _ in range(a.warmup):
                P.predict_large(model, frame, **kw)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                P.predict_large(model, frame, **kw)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            ev = []
            P.predict_large(model, frame, _events=ev, **kw)
            ms = split(ev)
            total = sum(ms.values())
            new = ms.get("gather", 0.0) + ms.get("blend", 0.0) + ms.get("finish", 0.0)
            g = P.plan_grid(a.h, a.w, a.tile, a.overlap)
            views = len(P.VIEWS[tta])
            per_fwd = max(1, a.batch // views)
            bb = blend_bytes(g, views, per_fwd, 23, model.segmentation_head[0].cout_p)
            med = statistics.median(times)
            print(json.dumps({
                "encoder": enc, "tta": tta or "none", "frame": [a.h, a.w], "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
                "tiles": g.rows * g.cols, "forwards": -(-g.rows * g.cols // per_fwd),
                "call_s_median": round(med, 4), "call_s_all": [round(t, 4) for t in times],
                "mpix_per_s": round(mpix / med, 3),
                "device_ms": {k: round(v, 3) for k, v in sorted(ms.items())}, "device_ms_total": round(total, 3),
                "kernel_share": round(new / total, 4) if total else None,
                "blend_bytes": bb, "blend_gbs": round(bb / (ms["blend"] * 1e6), 1) if ms.get("blend") else None,
                "accumulator_bytes": P.accumulator_bytes(a.h, a.w, 23),
            }), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
