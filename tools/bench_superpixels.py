#!/usr/bin/env python
"""Cost of the superpixel products at the headline batch (8 x 512 x 512 uint8 frames, 23 classes) on one MI355X, at step 8 / 16 / 32.

Seeded frames: block-constant colours (24 x 24 blocks) under a smooth ramp plus uniform noise of +-6, so that the assignment has
both edges to follow and fragments to absorb.  HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE inside
every round, all in ONE process, and every leg runs --inner back-to-back calls between its two events and reports the time PER
CALL.  Back-to-back calls on the same 6 MB of frames are cache-assisted: the figures are those of a batch that is already in L2 /
Infinity Cache, which is how a loader meets it.  Per step, with compactness 10:
  * assign_ms        udaseg_superpixel_assign: ONE assign-and-accumulate pass and its centre finish, labels written
  * slic_ms          superpixels.slic at 10 iterations (the defaults; step 16 is the default step), connect step included
  * connect_ms       udaseg_superpixel_connect alone on slic's labels before that step
  * vote_ms          superpixels.vote of a 23-class mask (count, decide, apply)
  * mean_ms          superpixels.mean of a score map
  * select_ms        superpixels.select at a budget of 1 % of the clusters (mean, radix select per image, select, gather)
and once, beside them in every round:
  * copy_ms          a device-to-device copy that reads and writes what one assign pass reads and writes (3 + 4 bytes per pixel)
  * label_ms         udaseg_regions_label of the 23-class mask with areas, 4-connectivity
  * crf_ms           crf.refine of the batch's scores at its defaults
and once:
  * forward_eval_ms  ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch (its own rounds)
Reported, not judged.  One JSON line; --out also writes it to a file together with the git HEAD.  The process ends itself after
--time-limit seconds.

    python tools/bench_superpixels.py [--reps 20 --warmup 3 --inner 5 --out profiles/superpixels_bench.txt]
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
from uda_aerial_semantic_segmentation_research_amd import crf, superpixels as SP  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402

STEPS = (8, 16, 32)
COMPACTNESS, ITERATIONS = 10, 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
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
    g = torch.Generator().manual_seed(3)
    bh, bw = -(-h // 24), -(-w // 24)
    blocks = torch.randint(30, 226, (n, bh, bw, 3), generator=g)
    frames = blocks.repeat_interleave(24, 1).repeat_interleave(24, 2)[:, :h, :w]
    ramp = (torch.arange(h)[:, None] + torch.arange(w)[None, :]) * 20 // (h + w)
    frames = (frames + ramp[None, :, :, None] + torch.randint(-6, 7, (n, h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    frames = frames.contiguous().to(dev)
    masks = torch.randint(0, c, (n, -(-h // 16), -(-w // 16)), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
    masks = masks[:, :h, :w].contiguous().to(torch.uint8).to(dev)
    key = torch.rand(n, h, w, generator=g).to(dev)
    scores = torch.randn(n, c, h, w, generator=g).to(dev)
    ids_r = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    area_r = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    copy_src = torch.randint(0, 256, (pixels * 7,), generator=g, dtype=torch.uint8).to(dev)
    copy_dst = torch.empty_like(copy_src)
    r4 = lambda v: round(v, 4)      # noqa: E731
    res = {}
    shared = {
        "copy": lambda: copy_dst.copy_(copy_src),
        "label": lambda: K.regions_label(masks, 4, 255, ids_r, area_r),
        "crf": lambda: crf.refine(scores, frames),
    }
    for S in STEPS:
        counts = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        seg = SP.slic(frames, S, COMPACTNESS, ITERATIONS, counts=counts)
        gh, gw = seg.grid
        centres = seg.centres.clone()
        labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
        K.superpixel_assign(frames, S, COMPACTNESS, centres, labels)          # labels before a connect step, for the connect leg
        out_ids = torch.empty_like(labels)
        work = seg.centres.clone()
        budget = max(1, gh * gw // 100)
        legs = {
            "assign": lambda: K.superpixel_assign(frames, S, COMPACTNESS, work, labels),
            "slic": lambda: SP.slic(frames, S, COMPACTNESS, ITERATIONS),
            "connect": lambda: K.superpixel_connect(labels, S, 0, out_ids),
            "vote": lambda: SP.vote(seg, masks, c),
            "mean": lambda: SP.mean(key, seg),
            "select": lambda: SP.select(key, seg, budget),
            **shared,
        }
        inner = {k: (1 if k in ("slic", "crf", "select") else a.inner) for k in legs}
        ms = alternating(legs, a.reps, a.warmup, inner)
        med = {k: statistics.median(v) for k, v in ms.items()}
        cnt = counts.sum(0).tolist()
        res[f"step{S}"] = {
            "clusters": gh * gw,
            **{f"{k}_ms": r4(v) for k, v in med.items()},
            **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
            "assign_over_copy": r4(med["assign"] / med["copy"]), "slic_over_crf": r4(med["slic"] / med["crf"]),
            "connect_over_label": r4(med["connect"] / med["label"]), "vote_over_crf": r4(med["vote"] / med["crf"]),
            "components": cnt[0], "absorbed": cnt[1], "relabelled_share": r4(cnt[2] / pixels), "clusters_left": cnt[3],
        }
        print(f"step {S}: " + json.dumps(res[f"step{S}"]), flush=True)

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)

    def forward_leg():
        with torch.no_grad():
            net(x)

    fwd = alternating({"forward_eval": forward_leg}, a.reps, a.warmup, {"forward_eval": 3})["forward_eval"]
    fwd_ms = statistics.median(fwd)
    for v in res.values():
        for k in ("assign", "slic", "connect", "vote", "mean", "select", "crf"):
            v[f"{k}_over_forward"] = round(v[f"{k}_ms"] / fwd_ms, 4)
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = json.dumps({"frames": [n, h, w], "classes": c, "compactness": COMPACTNESS, "iterations": ITERATIONS, "reps": a.reps,
                       "warmup": a.warmup, "inner": a.inner, "device": torch.cuda.get_device_name(0),
                       "forward_eval_ms": round(fwd_ms, 4), "forward_eval_ms_min_max": [round(fwd[0], 4), round(fwd[-1], 4)], **res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_superpixels.py: integer SLIC, connect, vote, mean and select at 8 x 512 x 512 uint8 frames, "
                     "23 classes, on 1 x MI355X (HIP-event medians per call, legs alternating in one process, back-to-back calls: "
                     "cache-assisted; ONE run)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
