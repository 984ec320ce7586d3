#!/usr/bin/env python
"""Cost of the device-side Fourier style transfer at the headline batch (8 x 512 x 512 uint8 frames) on one MI355X, at the band
half-widths b = 5, 23, 46 (beta = 0.01, 0.045, 0.09; K = 11, 47, 93).

Frames of the tests' recipe (tests/_fda_ref.py: noise, a colour cast, a low-frequency wave).  HIP-event medians over --reps rounds
after --warmup rounds; the legs ALTERNATE inside every round, all in ONE process, so that the ratios compare like with like.
Every leg runs --inner back-to-back calls between its two events and reports the time PER CALL.  Per band:
  * spectrum_ms   udaseg_fda_spectrum_u8 of the source batch (row stage + column stage, float64)
  * delta_ms      udaseg_fda_delta
  * apply_ms      udaseg_fda_apply_u8 to uint8 with counts, 16-byte aligned operands (column-part pre-kernel + streaming pass)
  * ours_ms       fda.transfer as a loader calls it with an AmplitudeBank (fresh outputs, workspaces and counts every call)
  * torch_ms      the torch composition of the same step: fft2 of source and target, abs, angle, the four corner blocks of the
                  unshifted spectrum assigned, polar, ifft2, real, round, clamp, to uint8 (None if this torch build has no FFT)
and once:
  * copy_ms          a device-to-device copy of the bytes the apply pass moves (3 per pixel read, 3 written)
  * forward_eval_ms  ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch
Reported, not judged.  One JSON line; --out also writes it to a file together with the git HEAD.

    python tools/bench_fda.py [--reps 20 --warmup 3 --inner 10 --out profiles/fda_bench.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _fda_ref as R  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import _lib, fda, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def alternating(legs, reps, warmup, inner):
    """{name: sorted HIP-event times per call in ms}: every round runs each leg once, in order, `inner` calls between two events."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: sorted(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--bands", type=int, nargs="+", default=[5, 23, 46])
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w = a.batch, a.size, a.size
    s_np, t_np = R.frames(n, h, w)
    src, tgt = torch.from_numpy(s_np).to(dev), torch.from_numpy(t_np).to(dev)
    lam = torch.ones(n, device=dev)
    pick = torch.arange(n, dtype=torch.int32, device=dev)
    out = torch.empty_like(src)
    counts = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    copy_dst = torch.empty_like(src)
    tw_h64, tw_h32 = fda._tables(h, dev)
    tw_w64, tw_w32 = fda._tables(w, dev)
    held, legs, state = {}, {}, {}
    fft_ok = True
    try:
        torch.fft.fft2(torch.zeros(4, 4, device=dev))
    except RuntimeError:
        fft_ok = False

    def torch_leg(b):
        fs = torch.fft.fft2(src.permute(0, 3, 1, 2).float())
        ft = torch.fft.fft2(tgt.permute(0, 3, 1, 2).float())
        amp, pha, amp_t = fs.abs(), fs.angle(), ft.abs()
        for ys in (slice(0, b + 1), slice(h - b, h)):
            for xs in (slice(0, b + 1), slice(w - b, w)):
                amp[:, :, ys, xs] = amp_t[:, :, ys, xs]
        res = torch.fft.ifft2(torch.polar(amp, pha)).real
        held["torch"] = res.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    for b in a.bands:
        k = 2 * b + 1
        st = state[b] = {
            "b": torch.full((n,), b, dtype=torch.int32, device=dev),
            "rows": torch.empty((n, 3, h, k, 2), dtype=torch.float64, device=dev),
            "coeffs": torch.empty((n, 3, k, k, 2), dtype=torch.float64, device=dev),
            "amps": fda.amplitudes(tgt, b),
            "delta": torch.empty((n, 3, k, k, 2), dtype=torch.float32, device=dev),
            "cols": torch.empty((n, 3, k, w, 2), dtype=torch.float32, device=dev),
            "bank": fda.AmplitudeBank(b, n),
        }
        st["bank"].add(tgt)
        legs[f"spectrum_b{b}"] = lambda st=st, b=b: K.fda_spectrum_u8(src, tw_h64, tw_w64, n, h, w, b, st["rows"], st["coeffs"])
        legs[f"delta_b{b}"] = lambda st=st, b=b: K.fda_delta(st["coeffs"], st["amps"], pick, st["b"], lam, n, n, h, w, b, st["delta"])
        legs[f"apply_b{b}"] = lambda st=st, b=b: K.fda_apply_u8(src, st["delta"], st["b"], tw_h32, tw_w32, n, h, w, b, st["cols"], out, None,
                                                                counts)
        legs[f"ours_b{b}"] = lambda st=st: held.__setitem__("ours", fda.transfer(src, st["bank"], st["b"], lam, pick))
        if fft_ok:
            legs[f"torch_b{b}"] = lambda b=b: torch_leg(b)
    legs["copy"] = lambda: copy_dst.copy_(src)
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).to(dev).eval()
    x = torch.randn(n, 3, h, w).to(dev)

    def forward_leg():
        with torch.no_grad():
            net(x)

    legs["forward_eval"] = forward_leg
    ms = alternating(legs, a.reps, a.warmup, a.inner)
    med = {k: statistics.median(v) for k, v in ms.items()}
    r4 = lambda v: round(v, 4)      # noqa: E731
    agree = None
    if fft_ok:                      # the last band ran last in both legs: the two compositions differ by float32 rounding alone
        d = (held["ours"][0].int() - held["torch"].int()).abs()
        agree = {"values_that_differ": int((d != 0).sum()), "largest_difference": int(d.max())}
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = json.dumps({
        "frames": [n, h, w, 3], "bands": a.bands, "reps": a.reps, "warmup": a.warmup, "inner": a.inner,
        "device": torch.cuda.get_device_name(0), "torch_fft": fft_ok,
        **{f"{k}_ms": r4(v) for k, v in med.items()},
        **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
        **{f"apply_b{b}_over_copy": r4(med[f"apply_b{b}"] / med["copy"]) for b in a.bands},
        **{f"ours_b{b}_over_forward": r4(med[f"ours_b{b}"] / med["forward_eval"]) for b in a.bands},
        **({f"ours_b{b}_over_torch": r4(med[f"ours_b{b}"] / med[f"torch_b{b}"]) for b in a.bands} if fft_ok else {}),
        "ours_against_torch_last_band": agree,
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_fda.py: Fourier style transfer at 8 x 512 x 512 on 1 x MI355X (HIP-event medians per call, "
                     "legs alternating in one process).  One run.\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
