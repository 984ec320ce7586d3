#!/usr/bin/env python
"""Measured error of the Fourier style transfer kernels (csrc/fda.hip) against the float64 mirror tests/_fda_ref.py on the cases of
tests/test_gpu_fda.py, on one MI355X: the spectrum (relative to 255 H W), the float32 field (grey levels), the uint8 frames (values
that differ from clip(rint(mirror)), and how far from a rounding boundary the mirror lies there) and the counters.  The bar of the
tests is chosen from this table (four times the worst field error, rounded up to one digit, at most 2e-3); the table is one run.

    python tools/grade_fda.py [--out profiles/fda_grade.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _fda_ref as R  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import _lib, fda  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    t = lambda v: torch.from_numpy(np.array(v))      # noqa: E731  (a copy: the shared reference arrays are read-only)
    lines = [f"{'case':<20} {'K':>3} {'spectrum/255HW':>15} {'field err':>10} {'u8 differ':>10} {'of':>8} {'worst gap':>10} "
             f"{'counts differ':>14}"]
    worst = 0.0
    for case in R.CASES:
        n, h, w, b = case
        ref = R.reference(case)
        bmax = max(max(b), 0)
        g = fda.low_spectrum(t(ref["src"]), bmax).cpu().numpy()
        spec = float(np.abs((g[..., 0] + 1j * g[..., 1]) - R.low_spectrum(ref["src"], bmax)).max()) / (255.0 * h * w)
        args = tuple(t(ref[k]) for k in ("src", "tgt", "b", "lam"))
        field = fda.transfer(*args, dtype=torch.float32)[0].cpu().numpy().astype(np.float64)
        err = float(np.abs(field - ref["field"]).max())
        worst = max(worst, err)
        frames, counts = fda.transfer(*args)
        off = frames.cpu().numpy() != R.to_u8(ref["field"])
        gap = float(np.abs(ref["field"] - np.floor(ref["field"]) - 0.5)[off].max()) if off.any() else 0.0
        dc = int(np.abs(counts.cpu().numpy() - R.counts(ref["field"])).sum())
        lines.append(f"{R.case_id(case):<20} {2 * bmax + 1:>3} {spec:>15.2e} {err:>10.3e} {int(off.sum()):>10} {off.size:>8} {gap:>10.2e} "
                     f"{dc:>14}")
    tau = 4.0 * worst
    digit = 10.0 ** np.floor(np.log10(tau))
    tau = float(np.ceil(tau / digit - 1e-9) * digit)
    lines.append(f"worst field error {worst:.3e} grey levels; four times that, rounded up to one digit: tau = {tau:.0e} (cap 2e-3)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        head = a.head
        if head is None:
            try:
                head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
            except OSError:
                pass
        with open(a.out, "w") as fh:
            fh.write("# python tools/grade_fda.py: the Fourier style transfer kernels against the float64 full-FFT mirror "
                     f"(tests/_fda_ref.py) on 1 x {torch.cuda.get_device_name(0)}.  One run.\n")
            fh.write("# 'worst gap': the largest distance of the mirror from a half-integer among the uint8 values that differ "
                     "(each by exactly 1)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
