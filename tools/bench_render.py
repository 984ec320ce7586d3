#!/usr/bin/env python
"""Cost of the device-side rendering of label maps (render.py, csrc/render.hip) on one MI355X, at a batch of model-size frames
(8 x 512 x 512) and at one 4000 x 6000 frame.

Seeded block-constant labels (23 classes in 16 x 16 blocks with 2 % of the pixels redrawn, so that outlines are sparse as in a
real prediction) and a random uint8 frame.  HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE inside
every round, all in ONE process.  Three variants, each with uint8 and with int64 labels:
  * mask      colorize(labels)                                         reads the labels, writes 3 bytes per pixel
  * overlay   overlay(frame, labels, alpha=0.5)                        + 3 bytes of frame per pixel
  * full      overlay(..., outline=white, counts accumulating)         + neighbour reads (cache), + the histogram
each against
  * copy_*    a device-to-device copy of as many bytes as the variant reads plus writes (half read, half written)
  * torch_*   the torch composition of the same picture, sync-free: table[labels.long()], a float32 blend, round, clamp,
              to(uint8); for `full` also four shifted compares for the outline, a where, and one bincount of
              labels + 256 * image
and, for context, predict_large of the frame with a random-weight r18 (once per shape, outside the rounds; skipped with
--no-predict: at 4000 x 6000 it needs 2.4 GB).  The torch blend is a float blend: it is compared for time, and for agreement within one level.
The condition, judged on this run's own numbers: every variant faster than its torch composition.  Reported, not judged: each
variant's rate (bytes read + written over time) as a fraction of its copy's rate.  One JSON line per shape; --out also writes
them to a file together with the git HEAD.

    python tools/bench_render.py [--reps 30 --warmup 5 --out profiles/render_bench.txt]
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

from uda_aerial_semantic_segmentation_research_amd import _lib  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import render as R  # noqa: E402

CLASSES = 23


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


def torch_outline(lab):
    e = torch.zeros_like(lab, dtype=torch.bool)
    d = lab[:, :, 1:] != lab[:, :, :-1]
    e[:, :, 1:] |= d
    e[:, :, :-1] |= d
    d = lab[:, 1:, :] != lab[:, :-1, :]
    e[:, 1:, :] |= d
    e[:, :-1, :] |= d
    return e


def bench_shape(n, h, w, reps, warmup, dev, predict):
    g = torch.Generator().manual_seed(4)
    coarse = torch.randint(0, CLASSES, (n, (h + 15) // 16, (w + 15) // 16), generator=g)
    lab = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :h, :w].contiguous()
    redo = torch.rand(n, h, w, generator=g) < 0.02
    lab = torch.where(redo, torch.randint(0, CLASSES, (n, h, w), generator=g), lab)
    lab8 = lab.to(torch.uint8).to(dev)
    lab64 = lab.to(dev)
    frame = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    table = R.palette_table(R.default_palette(), CLASSES, device=dev)
    table_f = table.float()
    white = torch.tensor([255, 255, 255], dtype=torch.uint8, device=dev)
    image_offset = (256 * torch.arange(n, device=dev)).view(n, 1, 1)
    px = n * h * w
    counts = torch.zeros(n, 256, dtype=torch.int64, device=dev)
    outs = {k: torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev) for k in ("mask", "overlay", "full")}
    held = {}

    def torch_mask(l):
        held["mask"] = table[l.long()]

    def torch_overlay(l):
        c = table_f[l.long()]
        held["overlay"] = (frame.float() * 0.5 + c * 0.5).round().clamp(0, 255).to(torch.uint8)

    def torch_full(l):
        ll = l.long()
        c = table_f[ll]
        o = (frame.float() * 0.5 + c * 0.5).round().clamp(0, 255).to(torch.uint8)
        held["full"] = torch.where(torch_outline(l)[..., None], white, o)
        held["counts"] = torch.bincount((ll + image_offset).reshape(-1), minlength=256 * n).view(n, 256)

    legs = {}
    copies = {}
    for tag, l, lb in (("u8", lab8, 1), ("i64", lab64, 8)):
        for variant, nbytes in (("mask", px * (lb + 3)), ("overlay", px * (lb + 6)), ("full", px * (lb + 6))):
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copies[f"{variant}_{tag}"] = nbytes
            legs[f"copy_{variant}_{tag}"] = (lambda s=src, d=dst: d.copy_(s))
        legs[f"mask_{tag}"] = (lambda l=l: R.colorize(l, table, CLASSES, out=outs["mask"]))
        legs[f"overlay_{tag}"] = (lambda l=l: R.overlay(frame, l, table, alpha=0.5, classes=CLASSES, out=outs["overlay"]))
        legs[f"full_{tag}"] = (lambda l=l: R.overlay(frame, l, table, alpha=0.5, classes=CLASSES, outline=(255, 255, 255),
                                                     counts=counts, out=outs["full"]))
        legs[f"torch_mask_{tag}"] = (lambda l=l: torch_mask(l))
        legs[f"torch_overlay_{tag}"] = (lambda l=l: torch_overlay(l))
        legs[f"torch_full_{tag}"] = (lambda l=l: torch_full(l))
    ms = alternating(legs, reps, warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the results agree: masks and counts exactly, the float blend within one level
    assert torch.equal(outs["mask"], held["mask"])
    calls = 2 * (reps + warmup)
    assert torch.equal(counts, calls * held["counts"])
    blend_dev = int((outs["overlay"].int() - held["overlay"].int()).abs().max())
    full_dev = int((outs["full"].int() - held["full"].int()).abs().max())
    assert blend_dev <= 1 and full_dev <= 1
    r4 = lambda v: round(v, 4)      # noqa: E731
    res = {"shape": [n, h, w], "classes": CLASSES, "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0),
           "outline_share": r4(float(torch_outline(lab8).float().mean())), "max_level_difference_to_float_blend": max(blend_dev, full_dev)}
    ok = True
    for key, nbytes in copies.items():
        ours, ref, cp = med[key], med[f"torch_{key}"], med[f"copy_{key}"]
        res[f"{key}_ms"] = r4(ours)
        res[f"{key}_ms_min_max"] = [r4(ms[key][0]), r4(ms[key][-1])]
        res[f"torch_{key}_ms"] = r4(ref)
        res[f"copy_{key}_ms"] = r4(cp)
        res[f"{key}_over_torch"] = r4(ours / ref)
        res[f"{key}_TB_per_s"] = r4(nbytes / (ours * 1e-3) / 1e12)
        res[f"{key}_fraction_of_copy_rate"] = r4(cp / ours)
        ok = ok and ours < ref
    res["every_variant_faster_than_torch"] = bool(ok)
    if predict:
        from uda_aerial_semantic_segmentation_research_amd.predict import predict_large
        from uda_aerial_semantic_segmentation_research_amd.unet import Unet
        torch.manual_seed(0)
        net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=CLASSES).to(dev).eval()
        times = []
        for i in range(3):                                        # the first call warms up; the median of the rest is reported
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for j in range(n):
                predict_large(net, frame[j], tile=512, overlap=0.25)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        res["predict_large_r18_ms"] = r4(statistics.median(times[1:]))
        res["full_u8_over_predict_large"] = r4(med["full_u8"] / res["predict_large_r18_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x512x512,1x4000x6000")
    ap.add_argument("--no-predict", action="store_true", help="skip the predict_large context leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    lines = []
    for spec in a.shapes.split(","):
        n, h, w = (int(v) for v in spec.split("x"))
        line = json.dumps(bench_shape(n, h, w, a.reps, a.warmup, dev, not a.no_predict))
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if a.out:
        head = a.head
        if head is None:
            try:
                head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
            except OSError:
                pass
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_render.py: rendering of label maps on 1 x MI355X (HIP-event medians, legs alternating in "
                     "one process)\n")
            fh.write(f"# git HEAD {head}\n")
            for line in lines:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
