"""What does the Lovasz-softmax loss on a grid cost?  Times ``losses.LovaszSoftmaxLoss`` at the training shape (8 x 23 x 512 x 512
logits in the padded NHWC buffer Unet hands over) on TWO confidence fields, one after the other in one process:

  random     logits 3 * randn, target = argmax at 70 % of the pixels: the errors spread over the bins
  confident  95 % of the pixels with p_t > 0.99 (a trained model): nearly every error falls into bin 0, the contended case of the
             histogram pass (one LDS address takes most of a wave's atomics)

Per field: the three launches of the loss at bins = 1024, timed inside their sequence (a device event between every two:
udaseg_lovasz_hist, udaseg_lovasz_table, udaseg_lovasz_fwd_bwd with its finish kernels); the whole loss forward + backward
through the module at bins = 256 / 1024 / 4096 with the measured sum of ``last_slack`` beside 1 / bins; and for comparison on the
same build: udaseg_ce_fwd_bwd, DiceLoss forward + backward, a device copy of the logits (read + write of the bytes of the fused
pass), and the sort-based torch composition on the device (softmax, per-class torch.sort, cumsums, backward).  Then one r18
train step with ``CrossEntropyLoss`` against ``LovaszSoftmaxLoss(ce_weight=1.0)``.

Every figure is the median of --rounds back-to-back calls of ONE run: the 200 MB of logits do not fit the caches, the tables
(188 KiB a group) do and are cache-assisted.  Writes the report to --out (default profiles/lovasz_bench.txt) and prints one JSON
line.  Usage (GPU box; fails without a GPU): python tools/bench_lovasz.py [--batch 8 --size 512 --classes 23 --rounds 20]"""
import argparse
import json
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


def pipeline_times(zero, fns, rounds, warmup):
    """The launches in the module's order on freshly zeroed tables, an event between every two: (median, min) per launch."""
    ts = [[] for _ in fns]
    for r in range(warmup + rounds):
        zero()
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
    """name -> (padded NHWC logits buffer, targets); 10 % of the targets void."""
    rnd = torch.randn(n, s, s, ldc, device="cuda", generator=g) * 3.0
    t_rnd = rnd[..., :c].argmax(3)
    flip = torch.rand(n, s, s, device="cuda", generator=g) < 0.3
    t_rnd = torch.where(flip, torch.randint(0, c, (n, s, s), device="cuda", generator=g), t_rnd)
    t_conf = torch.randint(0, c, (n, s // 32, s // 32), device="cuda", generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)
    conf = torch.randn(n, s, s, ldc, device="cuda", generator=g)
    sure = torch.rand(n, s, s, device="cuda", generator=g) < 0.95
    conf.scatter_add_(3, t_conf[..., None], (sure.float() * 11.0 + 1.0)[..., None])     # margin 12 over unit noise: p_t > 0.99
    out = {}
    for name, buf, tt in (("random", rnd, t_rnd), ("confident", conf, t_conf)):
        tt = tt.clone()
        tt[torch.rand(n, s, s, device="cuda", generator=g) < 0.1] = 255
        out[name] = (buf, tt)
    return out


def sort_based(z, t, c):
    """The paper's loss as a torch composition on the device: classes 'present', the whole batch one group."""
    zz = z.detach().requires_grad_(True)
    valid = (t != 255).reshape(-1)
    p = torch.softmax(zz, 1).permute(0, 2, 3, 1).reshape(-1, c)[valid]
    tv = t.reshape(-1)[valid]
    total, count = 0.0, 0
    for k in range(c):
        fg = (tv == k).float()
        if fg.sum() == 0:
            continue
        err = (fg - p[:, k]).abs()
        es, perm = torch.sort(err, descending=True)
        fs = fg[perm]
        G = fs.sum()
        inter = G - fs.cumsum(0)
        union = G + (1 - fs).cumsum(0)
        jac = 1.0 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        total = total + (es * jac).sum()
        count += 1
    return torch.autograd.grad(total / count, zz)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lovasz_bench.txt"))
    a = ap.parse_args()
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K, losses as L
    _lib.require_gpu()
    n, c, s = a.batch, a.classes, a.size
    ldc = (c + 3) // 4 * 4
    pixels = n * s * s
    np_ = _lib.load().udaseg_ce_partials()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"Lovasz-softmax on a grid, {n} x {c} x {s} x {s} logits (ldc {ldc}, {pixels} pixels, 10 % void); ONE run, median (min) of "
             f"{a.rounds} back-to-back rounds, device events; {torch.cuda.get_device_name(0)}"]
    logit_b = pixels * ldc * 4
    result = {}
    for name, (buf, t) in fields(n, c, s, ldc, g).items():
        z = buf.permute(0, 3, 1, 2)[:, :c].detach().requires_grad_(True)     # the zero-copy form: no layout kernel in any leg
        tgt = t.reshape(-1)
        part = torch.empty(np_, device="cuda", dtype=torch.float64)
        loss = torch.empty((), device="cuda")
        dl, cpart, colsum = torch.empty(pixels, ldc, device="cuda"), torch.empty(np_ * ldc, device="cuda"), torch.empty(ldc, device="cuda")
        copy_dst = torch.empty_like(buf)
        lines.append(f"\n== {name} confidence field")
        res = {}
        p_t = torch.softmax(z.detach(), 1).gather(1, t.clamp(0, c - 1)[:, None])[:, 0][t != 255]
        lines.append(f"  share of the valid pixels with p_t > 0.99: {float((p_t > 0.99).float().mean()):.3f}")
        del p_t
        B = 1024
        tables = torch.zeros((1, c, 2, B), device="cuda", dtype=torch.int32)
        counters = torch.zeros(4, device="cuda", dtype=torch.int64)
        coef = torch.empty((1, c, 2, B), device="cuda")
        present = torch.empty((1, c), device="cuda", dtype=torch.int32)
        slack, sparts = torch.empty(c, device="cuda", dtype=torch.float64), torch.empty(c, device="cuda", dtype=torch.float64)
        groups = -(-c // min(32, 8192 // B))
        launches = [
            ("udaseg_lovasz_hist (bins 1024)", lambda: K.lovasz_hist(buf, tgt, pixels, c, ldc, 255, 1, B, tables, counters),
             groups * (logit_b + 8 * pixels)),
            ("udaseg_lovasz_table (three tiny launches)", lambda: K.lovasz_table(tables, 1, c, B, False, coef, present, sparts, slack), 0),
            ("udaseg_lovasz_fwd_bwd, ce_weight 1 (with its finish kernels)",
             lambda: K.lovasz_fwd_bwd(buf, tgt, coef, counters, pixels, c, ldc, 255, 1, B, 1.0, part, loss, dl, cpart, colsum),
             2 * logit_b + 8 * pixels),
        ]

        def zero():
            tables.zero_()
            counters.zero_()

        per_launch = pipeline_times(zero, [fn for _, fn, _ in launches], a.rounds, a.warmup)
        for (what, _, nbytes), (us, mn) in zip(launches, per_launch):
            res[what.split(" (")[0].split(",")[0]] = round(us, 1)
            rate = f"{nbytes / 1e6:8.1f} MB {nbytes / us / 1e3:8.1f} GB/s" if nbytes else ""
            lines.append(f"  {what:82s} {us:9.1f} us (min {mn:8.1f}) {rate}")
        legs = []
        crits = {}
        for bins in (256, 1024, 4096):
            crits[bins] = L.LovaszSoftmaxLoss(ignore_index=255, bins=bins, ce_weight=1.0)
            legs.append((f"LovaszSoftmaxLoss(bins={bins}, ce_weight=1) forward + backward",
                         lambda cr=crits[bins]: torch.autograd.grad(cr(z, t), z)[0]))
        ce, dice = L.CrossEntropyLoss(), L.DiceLoss(ignore_index=255)
        t_ce = t.clamp(0, c - 1)
        legs += [("CrossEntropyLoss() forward + backward (udaseg_ce_fwd_bwd)", lambda: torch.autograd.grad(ce(z, t_ce), z)[0]),
                 ("DiceLoss(ignore_index) forward + backward", lambda: torch.autograd.grad(dice(z, t), z)[0]),
                 ("device copy of the logits (read + write)", lambda: copy_dst.copy_(buf)),
                 ("torch composition (softmax, per-class torch.sort, cumsums, backward)", lambda: sort_based(z, t, c))]
        for what, fn in legs:
            us, mn = timed(fn, a.rounds if "torch composition" not in what else max(3, a.rounds // 5), a.warmup if "torch" not in what else 1)
            res[what.split(" (")[0] if what.startswith(("Cross", "device", "torch")) else what.split(" forward")[0]] = round(us, 1)
            lines.append(f"  {what:82s} {us:9.1f} us (min {mn:8.1f})")
        for bins, cr in crits.items():
            sl = float(cr.last_slack.sum())
            res[f"slack bins={bins}"] = sl
            lines.append(f"  bins {bins:5d}: sum(last_slack) = {sl:.3e}   1 / bins = {1.0 / bins:.3e}   "
                         f"stats [valid finite, void, invalid, non-finite] = {cr.last_target_stats.tolist()}   "
                         f"present classes {int(cr.last_present.sum())}")
        result[name] = res
        del buf, z, dl, copy_dst
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    x = torch.randn(n, 3, s, s, device="cuda", generator=g)
    y = torch.randint(0, c, (n, s, s), device="cuda", generator=g)
    y[torch.rand(n, s, s, device="cuda", generator=g) < 0.1] = 255
    lines.append("\n== one train step, r18 Unet, fp32 (an untrained net: the random-field regime)")
    for what, crit in (("CrossEntropyLoss(ignore_index=255)", L.CrossEntropyLoss(ignore_index=255)),
                       ("LovaszSoftmaxLoss(ignore_index=255, ce_weight=1.0)", L.LovaszSoftmaxLoss(ignore_index=255, ce_weight=1.0))):
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
    print(json.dumps({"workload": f"{n}x{c}x{s}x{s} logits, Lovasz-softmax on a grid", "rounds": a.rounds, "us": result}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
