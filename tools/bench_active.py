#!/usr/bin/env python
"""Cost of the active-labelling products at the headline batch (8 x 512 x 512, 23 classes) on one MI355X, for the radii 1, 2, 4, 16.

Seeded block-constant masks (16 x 16 blocks of one class, 5 % of the blocks void, 10 % of the pixels relabelled at random so that
windows are impure) as in tools/bench_boundary.py; the scores are noise plus a bonus on the mask's class.  HIP-event medians over
--reps rounds after --warmup rounds; the legs ALTERNATE inside every round, all in ONE process, and every leg runs --inner
back-to-back calls between its two events and reports the time PER CALL.  Back-to-back calls on the same maps are cache-assisted.
Per radius:
  * mode_ms / impurity_ms / score_ms   udaseg_window_mode (with agreement and counts), udaseg_window_impurity, udaseg_acquire_score
  * erode_ms          boundary.erode's entry point at the same radius, on the same masks
  * torch_impurity_ms the torch composition of impurity: one_hot, avg_pool2d(divisor_override=1) over [N,C,H,W], the entropy
                      arithmetic.  Its result is compared with impurity's (to 1e-5).
  * select_ms         one active.select of 1 % of the pixels on that radius's key (a Python loop over the 8 images)
and once, beside them:
  * prepare_ms        udaseg_acquire_prepare on the [N,H,W,24] scores
  * copy2 / copy5 / copy13 / copy101   device copies that move what mode (1 + 1 bytes per pixel), impurity (1 + 4), the score pass
                      (1 + 4 in, 8 out) and the prepare pass (96 in, 5 out) read and write
  * forward_eval_ms   ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch
  * query_ms          a whole ActivePool.query at radius 1 (forward, prepare, score, select into the pool's maps)
Only impurity has a torch leg: the vote, the score pass, prepare and select are reported against copies, erode and the forward.
Reported, not judged.  One JSON line; --out also writes it to a file together with the git HEAD.  The process ends itself after
--time-limit seconds.

    python tools/bench_active.py [--reps 20 --warmup 3 --inner 10 --out profiles/active_bench.txt]
"""
import argparse
import json
import math
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
from uda_aerial_semantic_segmentation_research_amd import active as A  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402

RADII = (1, 2, 4, 16)


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


def torch_impurity(m, r, classes):
    """The torch composition of active.impurity(m, r, classes): labels >= classes are void."""
    live = m < classes
    onehot = torch.nn.functional.one_hot(torch.where(live, m, torch.zeros_like(m)).long(), classes).permute(0, 3, 1, 2).float()
    onehot = onehot * live[:, None]
    nc = torch.nn.functional.avg_pool2d(onehot, 2 * r + 1, stride=1, padding=r, divisor_override=1)
    n = nc.sum(1)
    s = (nc * torch.log(nc.clamp_min(1.0))).sum(1)
    imp = (torch.log(n.clamp_min(1.0)) - s / n.clamp_min(1.0)) / math.log(classes)
    return torch.where(n > 1, imp, torch.zeros_like(imp)).clamp_(0.0, 1.0)


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
    masks = blocks.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    noisy = torch.rand(n, h, w, generator=g) < 0.1
    masks = torch.where(noisy & (masks != 255), torch.randint(0, c, (n, h, w), generator=g), masks).to(torch.uint8).to(dev)
    ldc = (c + 3) // 4 * 4
    scores = torch.randn(n, h, w, ldc, generator=g).to(dev)
    scores += 3.0 * torch.nn.functional.one_hot(masks.long().clamp_max(ldc - 1), ldc) * torch.rand(n, h, w, 1, generator=g).to(dev)
    scores_nchw = scores.permute(0, 3, 1, 2)[:, :c]                      # the strided view a Unet returns: read in place
    lab = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    ent = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    K.acquire_prepare(scores, ldc, c, False, pixels, lab, ent, counters)
    out_u8 = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    er = torch.empty_like(out_u8)
    agr = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    imp = torch.empty_like(agr)
    score = torch.empty_like(agr)
    key = torch.empty_like(agr)
    counts3 = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    counts2 = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    copies = {}
    for name, per_pixel in (("copy2", 2), ("copy5", 5), ("copy13", 13), ("copy101", 101)):
        src = torch.randint(0, 256, (pixels * per_pixel // 2,), generator=g, dtype=torch.uint8).to(dev)
        copies[name] = (src, torch.empty_like(src))
    held = {}
    res = {}
    r4 = lambda v: round(v, 4)      # noqa: E731
    for r in RADII:
        tab = torch.from_numpy(A.table_of(r)).to(dev)

        def torch_leg():
            held["torch"] = torch_impurity(masks, r, c)

        def select_leg():
            held["select"] = A.select(key, 0.01)

        K.acquire_score(lab, ent, None, r, c, 0, tab, score, key)
        legs = {
            "mode": lambda: K.window_mode(masks, r, c, 255, False, 255, out_u8, agr, counts3),
            "impurity": lambda: K.window_impurity(masks, r, c, 255, tab, imp),
            "score": lambda: K.acquire_score(lab, ent, None, r, c, 0, tab, score, key),
            "erode": lambda: K.boundary_erode(masks, r, 255, 255, er, counts2),
            "torch_impurity": torch_leg,
            "select": select_leg,
            **{k: (lambda s=s, d=d: d.copy_(s)) for k, (s, d) in copies.items() if k != "copy101"},
        }
        inner = {k: a.inner for k in legs}
        inner["torch_impurity"] = inner["select"] = a.torch_inner
        ms = alternating(legs, a.reps, a.warmup, inner)
        diff = float((held["torch"] - imp).abs().max())
        assert diff < 1e-5, f"radius {r}: the torch composition and impurity differ by {diff}"
        med = {k: statistics.median(v) for k, v in ms.items()}
        sel_counts = held["select"][1].sum(0).tolist()
        res[f"r{r}"] = {
            **{f"{k}_ms": r4(v) for k, v in med.items()},
            **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
            "mode_over_copy2": r4(med["mode"] / med["copy2"]), "impurity_over_copy5": r4(med["impurity"] / med["copy5"]),
            "score_over_copy13": r4(med["score"] / med["copy13"]), "impurity_over_torch": r4(med["impurity"] / med["torch_impurity"]),
            "mode_over_erode": r4(med["mode"] / med["erode"]), "tile": list(K.window_tile(r)),
            "changed_share": r4(float((out_u8 != masks).sum()) / pixels), "mean_impurity": r4(float(imp.mean())),
            "selected": sel_counts[0], "candidates": sel_counts[1], "torch_max_abs_diff": diff,
        }
        print(f"radius {r}: " + json.dumps(res[f"r{r}"]), flush=True)

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)
    frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    pool = A.ActivePool(c, radius=1, budget=0.001)

    def forward_leg():
        with torch.no_grad():
            net(x)

    once = alternating({"forward_eval": forward_leg, "query": lambda: pool.query(net, list(range(n)), frames),
                        "prepare": lambda: K.acquire_prepare(scores, ldc, c, False, pixels, lab, ent, counters),
                        "prepare_strided": lambda: A.prepare(scores_nchw),
                        "copy101": lambda: copies["copy101"][1].copy_(copies["copy101"][0])},
                       a.reps, a.warmup, {"forward_eval": 3, "query": 1, "prepare": a.inner, "prepare_strided": a.inner, "copy101": a.inner})
    med = {k: statistics.median(v) for k, v in once.items()}
    for r in RADII:
        v = res[f"r{r}"]
        v["score_over_forward"] = r4(v["score_ms"] / med["forward_eval"])
        v["mode_over_forward"] = r4(v["mode_ms"] / med["forward_eval"])
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = json.dumps({"masks": [n, h, w], "classes": c, "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
                       "torch_inner": a.torch_inner, "device": torch.cuda.get_device_name(0),
                       **{f"{k}_ms": r4(v) for k, v in med.items()},
                       **{f"{k}_ms_min_max": [r4(once[k][0]), r4(once[k][-1])] for k in once},
                       "prepare_over_copy101": r4(med["prepare"] / med["copy101"]),
                       "query_over_forward": r4(med["query"] / med["forward_eval"]),
                       "query_requested_share": r4(pool.coverage()["total"] / pixels), "query_rounds": pool.rounds, **res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_active.py: active-labelling products at 8 x 512 x 512, 23 classes, on 1 x MI355X "
                     "(HIP-event medians per call, legs alternating in one process, back-to-back calls: cache-assisted)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
