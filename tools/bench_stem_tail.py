"""The tail of the backward pass on its own: what does the stem's weight gradient cost with the apply half of its BatchNorm backward in
its staging?  In one process, at the training shape (8 x 3(4) x 512 x 512 images, 64 channels at 256 x 256), legs alternating round by
round, HIP-event medians:

  (a) bn_bwd_apply (writes dy over dz) + conv2d_wgrad (the split-K kernel)      -- the two launches of the old path
  (b) conv2d_wgrad_stem_bn (csrc/conv_stem_wgrad.hip)                          -- the one launch that replaces them
  (c) a device copy of the bytes (b) reads (dz + y + x), read + write

and (b) again at a sweep of block counts (udaseg_stem_wgrad_set_blocks).  All legs accumulate onto the same kind of gradient buffer and
take the same bn_bwd_reduce sums.  Writes the report to --out (default profiles/stem_tail_bench.txt) and prints one JSON line.
Usage (GPU box; fails without a GPU): python tools/bench_stem_tail.py [--batch 8 --size 512 --rounds 30]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternated(legs, rounds, warmup):
    """{name: (median us, min us)}: every round runs every leg once, in order, an event pair around each."""
    ts = {name: [] for name, _ in legs}
    for r in range(warmup + rounds):
        for name, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: (statistics.median(t), min(t)) for name, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", default="64,96,128,192,256,384,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_tail_bench.txt"))
    a = ap.parse_args()
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K
    _lib.require_gpu()
    K.ensure_workspace(torch.device("cuda", 0))
    n, s = a.batch, a.size
    d = K.conv_desc(n, s, s, 4, 64, 7, 2, 3)
    if not K.conv_stem_wgrad_bn_ok(d):
        raise RuntimeError("udaseg_conv_stem_wgrad_bn_ok answers no for this shape / device")
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, s, s, 4, device="cuda", generator=g)
    x[..., 3] = 0.0
    y = torch.randn(n, d.ho, d.wo, 64, device="cuda", generator=g)
    dz0 = torch.randn(n, d.ho, d.wo, 64, device="cuda", generator=g)
    mean, var = y.reshape(-1, 64).mean(0), y.reshape(-1, 64).var(0, unbiased=False)
    rstd = torch.rsqrt(var + 1e-5)
    gamma = torch.rand(64, device="cuda", generator=g) + 0.5
    beta = torch.randn(64, device="cuda", generator=g) * 0.1
    bsums = torch.zeros(2 * 64 * K.bn_replicas(), dtype=torch.float64, device="cuda")
    K.bn_bwd_reduce(dz0, None, y, mean, rstd, bsums, 1, 0.0, gamma=gamma, beta=beta)
    dz, dw_a, dw_b = dz0.clone(), torch.zeros(64, 7, 7, 4, device="cuda"), torch.zeros(64, 7, 7, 4, device="cuda")
    dg, db = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    read_b = (dz.numel() + y.numel() + x.numel()) * 4
    src = torch.empty(read_b // 4, device="cuda")
    dst = torch.empty_like(src)

    def old():          # dz becomes dy in place, as the engine ran it (its values drift from round to round: the time does not care)
        K.bn_bwd_apply(dz, None, y, mean, rstd, gamma, bsums, dz, None, dg, db, 1, 0.0, beta=beta)
        K.conv2d_wgrad(d, x, dz, dw_a, True)

    def new():
        K.conv2d_wgrad_stem_bn(d, x, dz0, y, mean, rstd, gamma, beta, bsums, 1, 0.0, dw_b, dg, db, True, False)

    legs = [("(a) bn_bwd_apply + conv2d_wgrad", old), ("(b) conv2d_wgrad_stem_bn", new), ("(c) device copy of the bytes (b) reads", lambda: dst.copy_(src))]
    res = alternated(legs, a.rounds, a.warmup)
    flops = 2.0 * n * d.ho * d.wo * 64 * 147
    lines = [f"stem tail, {n} x {s} x {s} x 4 images -> {n} x {d.ho} x {d.wo} x 64; median (min) of {a.rounds} alternated rounds, device events; "
             f"{torch.cuda.get_device_name(0)}"]
    for name, _ in legs:
        us, mn = res[name]
        lines.append(f"  {name:46s} {us:8.1f} us (min {mn:8.1f})")
    ua, ub, uc = (res[name][0] for name, _ in legs)
    lines.append(f"  (b) / (a) = {ub / ua:.3f}   (b): {flops / ub / 1e6:.1f} TFLOP/s over 147 live columns, {read_b / ub / 1e6:.2f} TB/s of its {read_b / 1e6:.0f} MB; "
                 f"the copy moves them (read + write) at {2 * read_b / uc / 1e6:.2f} TB/s: (b) / (c) = {ub / uc:.2f}")
    sweep = {}
    lines.append("  block-count sweep of (b) (0: one per CU):")
    for blocks in [0] + [int(b) for b in a.blocks.split(",") if b]:
        K.stem_wgrad_set_blocks(blocks)
        try:
            us, mn = alternated([("b", new)], a.rounds, a.warmup)["b"]
        finally:
            K.stem_wgrad_set_blocks(0)
        sweep[blocks] = round(us, 1)
        lines.append(f"    {blocks:5d} blocks {us:8.1f} us (min {mn:8.1f})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"workload": f"stem tail {n}x{s}x{s}", "rounds": a.rounds, "us": {k: round(v[0], 1) for k, v in res.items()}, "sweep": sweep}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
