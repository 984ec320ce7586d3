#!/usr/bin/env python
"""Cost of the prototype rectification at the headline batch (8 x 512 x 512 pixels, D = 16 decoder channels, C = 23) on one MI355X.

Seeded decoder features in the padded NHWC buffer forward_parts hands out (ldf = 16): a unit-normal prototype per class plus
unit-normal noise; labels constant on 96 x 96 blocks (a smooth label map: two 64-pixel chunks in three carry one class, the third
straddles a boundary) and, for a second accumulate leg, independent per pixel (about 21 classes per chunk: the LDS-atomic
route).  Logits as in bench_pseudo.py.  HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE inside
every round, all in ONE process:
  * accumulate_ms / accumulate_random_ms   udaseg_proto_accumulate under the smooth / the per-pixel random labels
  * update_ms                              udaseg_proto_update (clear = 0, so that every round sees the same sums)
  * rectify_ms                             udaseg_proto_rectify (logits in, padded NHWC probabilities out)
  * torch_accumulate_ms                    sums.index_add_(0, labels, features.double()), sq.index_add_, bincount
  * torch_accumulate_onehot_ms             the same sums as one_hot(labels).double().t() @ features.double() (no atomics)
  * torch_rectify_ms                       softmax, the [pixels, C, D] broadcast of squared distances, exp of the shifted
                                           distances (the second softmax's numerator), product, normalisation
  * torch_rectify_matmul_ms                the same with |f|^2 - 2 f P^T + |P|^2 for the distances (less exact, no broadcast)
  * forward_eval_ms                        ONE eval-mode r18 forward_parts(("logits", "decoder")) of an 8 x 3 x 512 x 512 batch
  * copy_features_ms / copy_scores_ms      device-to-device copies of the feature / the score buffer
  * label_proto_ms / label_online_ms       one PrototypeLabeler.label call beside one OnlineLabeler.label call, same frames
Reported, not judged (there is no speed gate): each pixel kernel's rate over its bytes as a fraction of a copy's rate.
One JSON line; --out also writes it to a file together with the git HEAD.

    python tools/bench_proto.py [--reps 10 --warmup 2 --out profiles/proto_bench.txt]
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

from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import proto as PR, teacher  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c, d = a.batch, a.size, a.size, a.classes, a.dim
    ldc = (c + 3) // 4 * 4
    pixels = n * h * w
    g = torch.Generator().manual_seed(2)
    tb = torch.randint(0, c, (n, h // 8, w // 8), generator=g)
    winner = tb.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    blocks = torch.randint(0, c, (n, (h + 95) // 96, (w + 95) // 96), generator=g)
    regions = blocks.repeat_interleave(96, 1).repeat_interleave(96, 2)[:, :h, :w].contiguous()
    centres = torch.randn(c, d, generator=g)
    feat = (centres[regions.reshape(-1)] + torch.randn(pixels, d, generator=g)).to(dev)
    z = 1.5 * torch.randn(n, h, w, ldc, generator=g)
    z.scatter_add_(3, winner[..., None], 12.0 * torch.rand(n, h, w, 1, generator=g))
    z[..., c:] = 0.0
    scores = z.to(dev)
    smooth = regions.reshape(-1).to(torch.uint8).to(dev)
    noisy = torch.randint(0, c, (pixels,), generator=g).to(torch.uint8).to(dev)
    noisy_long = noisy.long()

    bank = PR.PrototypeBank(c, d, min_pixels=1)
    bank._ensure(dev)
    K.proto_accumulate(feat, d, d, smooth, pixels, c, bank.sums, bank.sq, bank.counts)
    bank.update(clear=False)                                   # prototypes and a temperature for the rectify leg to read
    scratch = PR.PrototypeBank(c, d)._ensure(dev)              # the accumulators the timed legs add into
    out = torch.empty(pixels, ldc, dtype=torch.float32, device=dev)
    f_dst, s_dst = torch.empty_like(feat), torch.empty_like(scores)
    rows = scores.view(pixels, ldc)[:, :c]
    t_sums = torch.zeros(c, d, dtype=torch.float64, device=dev)
    t_sq = torch.zeros(c, dtype=torch.float64, device=dev)
    p32 = bank.prototypes.float()
    inv_tau = bank.inv_tau
    held = {}

    def torch_accumulate():
        f64 = feat.double()
        t_sums.index_add_(0, noisy_long, f64)
        t_sq.index_add_(0, noisy_long, (f64 * f64).sum(1))
        held["counts"] = torch.bincount(noisy_long, minlength=c)

    def torch_accumulate_onehot():
        f64 = feat.double()
        hot = torch.nn.functional.one_hot(noisy_long, c).double()
        held["sums"] = hot.t() @ f64
        held["sq"] = hot.t() @ (f64 * f64).sum(1)
        held["counts"] = hot.sum(0)

    def torch_rectify():
        p = torch.softmax(rows, dim=1)
        dist = ((feat[:, None, :] - p32[None, :, :]) ** 2).sum(2)
        u = torch.exp(-(dist - dist.min(1, keepdim=True).values) * inv_tau)
        r = p * u
        held["rect"] = r / r.sum(1, keepdim=True)

    def torch_rectify_matmul():
        p = torch.softmax(rows, dim=1)
        dist = (feat * feat).sum(1, keepdim=True) - 2.0 * feat @ p32.t() + (p32 * p32).sum(1)[None, :]
        u = torch.exp(-(dist - dist.min(1, keepdim=True).values) * inv_tau)
        r = p * u
        held["rect_mm"] = r / r.sum(1, keepdim=True)

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)
    frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    lab_proto = PR.PrototypeLabeler(net, c, portion=0.2, cap=0.9)
    lab_online = teacher.OnlineLabeler(net, c, portion=0.2, cap=0.9)

    def forward_leg():
        with torch.no_grad():
            net.forward_parts(x, ("logits", "decoder"))

    legs = {
        "accumulate": lambda: K.proto_accumulate(feat, d, d, smooth, pixels, c, scratch.sums, scratch.sq, scratch.counts),
        "accumulate_random": lambda: K.proto_accumulate(feat, d, d, noisy, pixels, c, scratch.sums, scratch.sq, scratch.counts),
        "update": lambda: bank.update(clear=False),
        "rectify": lambda: K.proto_rectify(feat, d, d, scores, ldc, c, 0, bank.prototypes, bank.seen, bank.inv_tau, pixels, out),
        "torch_accumulate": torch_accumulate,
        "torch_accumulate_onehot": torch_accumulate_onehot,
        "torch_rectify": torch_rectify,
        "torch_rectify_matmul": torch_rectify_matmul,
        "forward_eval": forward_leg,
        "copy_features": lambda: f_dst.copy_(feat),
        "copy_scores": lambda: s_dst.copy_(scores),
        "label_proto": lambda: lab_proto.label(frames),
        "label_online": lambda: lab_online.label(frames),
    }
    ms = alternating(legs, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    calls = a.reps + a.warmup
    assert int(scratch.counts.sum()) == 2 * calls * pixels
    agree = float((held["rect"] - out[:, :c]).abs().max())
    feat_bytes, score_bytes = pixels * d * 4, pixels * ldc * 4
    copy_f = 2 * feat_bytes / (med["copy_features"] * 1e-3) / 1e12
    copy_s = 2 * score_bytes / (med["copy_scores"] * 1e-3) / 1e12
    acc_rate = (feat_bytes + pixels) / (med["accumulate"] * 1e-3) / 1e12
    acc_rand_rate = (feat_bytes + pixels) / (med["accumulate_random"] * 1e-3) / 1e12
    rect_rate = (feat_bytes + 2 * score_bytes) / (med["rectify"] * 1e-3) / 1e12
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r4 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "pixels": [n, h, w], "dim": d, "classes": c, "ldc": ldc, "reps": a.reps, "warmup": a.warmup,
        "device": torch.cuda.get_device_name(0),
        **{f"{k}_ms": r4(v) for k, v in med.items()},
        **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in legs},
        "accumulate_over_torch": round(med["accumulate"] / med["torch_accumulate"], 6),
        "accumulate_random_over_torch": round(med["accumulate_random"] / med["torch_accumulate"], 6),
        "accumulate_over_torch_onehot": r4(med["accumulate"] / med["torch_accumulate_onehot"]),
        "accumulate_random_over_torch_onehot": r4(med["accumulate_random"] / med["torch_accumulate_onehot"]),
        "rectify_over_torch": r4(med["rectify"] / med["torch_rectify"]),
        "rectify_over_torch_matmul": r4(med["rectify"] / med["torch_rectify_matmul"]),
        "accumulate_plus_rectify_over_forward": r4((med["accumulate"] + med["update"] + med["rectify"]) / med["forward_eval"]),
        "label_proto_over_label_online": r4(med["label_proto"] / med["label_online"]),
        "copy_features_TB_per_s": r4(copy_f), "copy_scores_TB_per_s": r4(copy_s),
        "accumulate_TB_per_s": r4(acc_rate), "accumulate_random_TB_per_s": r4(acc_rand_rate), "rectify_TB_per_s": r4(rect_rate),
        "accumulate_fraction_of_copy_rate": r4(acc_rate / copy_f),
        "accumulate_random_fraction_of_copy_rate": r4(acc_rand_rate / copy_f),
        "rectify_fraction_of_copy_rate": r4(rect_rate / copy_s),
        "rectify_max_abs_diff_to_torch": agree,
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_proto.py: prototype rectification at 8 x 512 x 512 pixels, D = 16, C = 23 on 1 x MI355X "
                     "(HIP-event medians, legs alternating in one process)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write("# accumulate: labels constant on 96 x 96 blocks -- two 64-pixel chunks in three carry one class (one reduce-scatter\n"
                     "# round), the third straddles a boundary (two rounds); accumulate_random: labels independent per pixel, about 21\n"
                     "# classes per chunk, so four rounds and then per-lane LDS float64 atomics (dim + 2 per pixel, lanes of one class\n"
                     "# serialise on one address): the label-divergent worst case.\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
