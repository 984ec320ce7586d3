"""What does hard-pixel mining cost on top of the one-pass cross entropy?  Times ``losses.OhemCrossEntropyLoss`` at the training
shape (8 x 23 x 512 x 512 logits in the padded NHWC buffer Unet hands over) on TWO confidence fields, one after the other in one
process:

  smooth   the target class's confidence varies slowly along a row: a wave's 64 pixels share one or two level-0 bins
  random   logits 3 * randn, target = argmax at 70 % of the pixels: neighbours land in unrelated bins (the easy pixels' nine)

Per field: every launch of the loss, timed inside its sequence (a device event between every two: udaseg_ohem_conf, the three udaseg_kth_select,
the two udaseg_kth_hist, udaseg_ohem_denom, udaseg_ce_ohem_fwd_bwd with its finish kernels), the whole loss forward + backward
through the module, and for comparison on the same build: CrossEntropyLoss(ignore_index=255) forward + backward
(udaseg_ce_opt_fwd_bwd), a device copy of the logits (read + write of the same bytes as the fused pass), the torch composition
(softmax, gather, kthvalue, masked cross_entropy, backward), and one r18 train step with either criterion.
Writes the report to --out (default profiles/ohem_bench.txt) and prints one JSON line.
Usage (GPU box; fails without a GPU): python tools/bench_ohem.py [--batch 8 --size 512 --classes 23 --rounds 20]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, rounds, warmup):
    ts = []
    for r in range(warmup + rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts)


def pipeline_times(ws, fns, rounds, warmup):
    """The launches in the module's order on a freshly zeroed workspace, an event between every two: (median, min) per launch."""
    ts = [[] for _ in fns]
    for r in range(warmup + rounds):
        ws.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        for e, fn in zip(ev, fns):
            e.record()
            fn()
        ev[-1].record()
        ev[-1].synchronize()
        if r >= warmup:
            for i in range(len(fns)):
                ts[i].append(ev[i].elapsed_time(ev[i + 1]) * 1e3)
    return [(statistics.median(t), min(t)) for t in ts]


def fields(n, c, s, ldc, g):
    """name -> (padded NHWC logits buffer, targets)."""
    t = torch.randint(0, c, (n, s // 64, s // 64), device="cuda", generator=g).repeat_interleave(64, 1).repeat_interleave(64, 2)
    x = torch.arange(s, device="cuda", dtype=torch.float32)
    ramp = 3.0 + 2.5 * torch.sin(2 * math.pi * x / s)[None, None, :] + 0.5 * torch.cos(2 * math.pi * x / s)[None, :, None]
    smooth = torch.zeros(n, s, s, ldc, device="cuda")
    smooth.scatter_(3, t[..., None], ramp.expand(n, s, s)[..., None].contiguous())
    rnd = torch.randn(n, s, s, ldc, device="cuda", generator=g) * 3.0
    t_rnd = rnd[..., :c].argmax(3)
    flip = torch.rand(n, s, s, device="cuda", generator=g) < 0.3
    t_rnd = torch.where(flip, torch.randint(0, c, (n, s, s), device="cuda", generator=g), t_rnd)
    out = {}
    for name, buf, tt in (("smooth", smooth, t), ("random", rnd, t_rnd)):
        tt = tt.clone()
        tt[torch.rand(n, s, s, device="cuda", generator=g) < 0.1] = 255
        out[name] = (buf, tt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.7)
    ap.add_argument("--min-kept", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ohem_bench.txt"))
    a = ap.parse_args()
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K, losses as L
    _lib.require_gpu()
    n, c, s = a.batch, a.classes, a.size
    ldc = (c + 3) // 4 * 4
    pixels = n * s * s
    np_ = _lib.load().udaseg_ce_partials()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"hard-pixel mining, {n} x {c} x {s} x {s} logits (ldc {ldc}, {pixels} pixels, 10 % void), thresh {a.thresh}, "
             f"min_kept {a.min_kept}; median (min) of {a.rounds} rounds, device events; {torch.cuda.get_device_name(0)}"]
    logit_b = pixels * ldc * 4
    result = {}
    for name, (buf, t) in fields(n, c, s, ldc, g).items():
        z = buf.permute(0, 3, 1, 2)[:, :c].detach().requires_grad_(True)     # the zero-copy form: no layout kernel in any leg
        ohem = L.OhemCrossEntropyLoss(thresh=a.thresh, min_kept=a.min_kept, ignore_index=255)
        ce = L.CrossEntropyLoss(ignore_index=255)
        tgt = t.reshape(-1)
        ws = torch.zeros(3 * K.KTH_BINS + K.KTH_STATE + 5, device="cuda", dtype=torch.int64)
        hist, state, stats = ws[:3 * K.KTH_BINS].view(3, K.KTH_BINS), ws[3 * K.KTH_BINS:3 * K.KTH_BINS + K.KTH_STATE], ws[-5:]
        conf = torch.empty(pixels, device="cuda")
        denom = torch.empty(1, device="cuda", dtype=torch.float64)
        dpart = torch.empty(3 * np_, device="cuda", dtype=torch.float64)
        part = torch.empty(np_, device="cuda", dtype=torch.float64)
        loss = torch.empty((), device="cuda")
        dl, cpart, colsum = torch.empty(pixels, ldc, device="cuda"), torch.empty(np_ * ldc, device="cuda"), torch.empty(ldc, device="cuda")
        copy_dst = torch.empty_like(buf)
        # the launches in the module's order, timed inside that sequence (each reads what the one before it wrote)
        launches = [
            ("udaseg_ohem_conf", lambda: K.ohem_conf(buf, tgt, pixels, c, ldc, 255, conf, hist[0], stats[2:5]), logit_b + 12 * pixels),
            ("udaseg_kth_select 0", lambda: K.kth_select(hist[0], 0, state, min_kept=a.min_kept), 0),
            ("udaseg_kth_hist 1", lambda: K.kth_hist(conf, 1, state, hist[1]), 4 * pixels),
            ("udaseg_kth_select 1", lambda: K.kth_select(hist[1], 1, state), 0),
            ("udaseg_kth_hist 2", lambda: K.kth_hist(conf, 2, state, hist[2]), 4 * pixels),
            ("udaseg_kth_select 2", lambda: K.kth_select(hist[2], 2, state), 0),
            ("udaseg_ohem_denom", lambda: K.ohem_denom(conf, tgt, None, pixels, c, a.thresh, state, dpart, denom, stats[0:2]), 12 * pixels),
            ("udaseg_ce_ohem_fwd_bwd", lambda: K.ce_ohem_fwd_bwd(buf, tgt, None, conf, state, a.thresh, pixels, c, ldc, True, denom, part,
                                                                 loss, dl, cpart, colsum), 2 * logit_b + 4 * pixels),
        ]

        def torch_composition():
            zz = z.detach().requires_grad_(True)
            valid = t != 255
            p = torch.softmax(zz.detach(), 1).gather(1, t.clamp(0, c - 1)[:, None])[:, 0]
            pv = p[valid]
            q = torch.kthvalue(pv, min(a.min_kept, pv.numel())).values
            keep = valid & ((p < a.thresh) | (p <= q))
            lo = torch.nn.functional.cross_entropy(zz, torch.where(keep, t, torch.full_like(t, 255)), ignore_index=255)
            return torch.autograd.grad(lo, zz)[0]

        legs = [("OhemCrossEntropyLoss forward + backward", lambda: torch.autograd.grad(ohem(z, t), z)[0]),
                ("CrossEntropyLoss(ignore_index) forward + backward (udaseg_ce_opt_fwd_bwd)", lambda: torch.autograd.grad(ce(z, t), z)[0]),
                ("device copy of the logits (read + write)", lambda: copy_dst.copy_(buf)),
                ("torch composition (softmax, gather, kthvalue, masked cross_entropy, backward)", torch_composition)]
        lines.append(f"\n== {name} confidence field")
        res = {}
        per_launch = pipeline_times(ws, [fn for _, fn, _ in launches], a.rounds, a.warmup)
        for (what, _, nbytes), (us, mn) in zip(launches, per_launch):
            res[what] = round(us, 1)
            rate = f"{nbytes / 1e6:8.1f} MB {nbytes / us / 1e3:8.1f} GB/s" if nbytes else ""
            lines.append(f"  {what:82s} {us:9.1f} us (min {mn:8.1f}) {rate}")
        for what, fn in legs:
            us, mn = timed(fn, a.rounds, a.warmup)
            res[what.split(" (")[0]] = round(us, 1)
            lines.append(f"  {what:82s} {us:9.1f} us (min {mn:8.1f})")
        st = ohem.last_ohem_stats.tolist()
        thr = ohem.last_threshold.tolist()
        lines.append(f"  stats [valid finite, kept, void, invalid, non-finite] = {st}   q = {thr[0]:.6f}   keep below {thr[1]:.6f}")
        lines.append(f"  whole loss / udaseg_ce_opt_fwd_bwd loss = {res['OhemCrossEntropyLoss forward + backward'] / res['CrossEntropyLoss(ignore_index) forward + backward']:.2f}"
                     f"   conf pass / copy = {res['udaseg_ohem_conf'] / res['device copy of the logits']:.2f} of the time for "
                     f"{(logit_b + 12 * pixels) / (2 * logit_b):.2f} of the bytes")
        result[name] = res
        del buf, z, dl, copy_dst
    # one r18 train step with either criterion
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    x = torch.randn(n, 3, s, s, device="cuda", generator=g)
    y = torch.randint(0, c, (n, s, s), device="cuda", generator=g)
    y[torch.rand(n, s, s, device="cuda", generator=g) < 0.1] = 255
    lines.append("\n== one train step, r18 Unet, fp32")
    for what, crit in (("CrossEntropyLoss(ignore_index=255)", L.CrossEntropyLoss(ignore_index=255)),
                       ("OhemCrossEntropyLoss", L.OhemCrossEntropyLoss(thresh=a.thresh, min_kept=a.min_kept, ignore_index=255))):
        torch.manual_seed(0)
        net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c)
        tr = SegmentationTrainer(net, torch.device("cuda", 0), criterion=crit)
        net.train()
        opt = FusedAdam(net.parameters(), lr=1e-4)
        us, mn = timed(lambda: tr.train_step(x, y, opt), a.rounds, a.warmup)
        result[f"train step {what.split('(')[0]}"] = round(us, 1)
        lines.append(f"  {what:82s} {us:9.1f} us (min {mn:8.1f})")
        del net, tr, opt
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"workload": f"{n}x{c}x{s}x{s} logits, hard-pixel mining", "rounds": a.rounds, "us": result}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
