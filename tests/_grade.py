"""The verdict collector of the element-wise grade files (tests/test_gpu_norm_grade.py, tests/test_gpu_pool_grade.py): the one bar
max(e) <= max(4 x max(d), 2^-22) of tests/_norm_ref.py, every figure logged before the first assertion fires.

Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import os

import numpy as np

import _norm_ref as N


def log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Grader:
    """Collects the verdicts of one case so that every figure is logged before the first assertion fires."""
    PREFIX = "norm-grade"

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def grade(self, what, got, r64, r32, mag, bf16_out=False):
        b, dmax = N.bar(r32, r64, mag)
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got - r64)
        if bf16_out:
            err = np.maximum(err - N.bf16_half_ulp(r64, b * mag), 0.0)
        e = float(N.normalised(err, mag).max()) if np.isfinite(got).all() else float("inf")
        log(f"{self.PREFIX} {self.tag} {what}: kernel-vs-f64 {e:.3e}  f32-vs-f64 {dmax:.3e}  bar {b:.3e}  e/bar {e / b:.3f}")
        if not e <= b:
            self.bad.append(f"{what}: {e:.3e} > bar {b:.3e}")

    def ulp2(self, what, got, r64, operand):
        """|got - f64| <= 2 ulp of fp32 at the larger of |f64| and the operand's magnitude."""
        ulp = np.spacing(np.maximum(np.abs(r64), operand).astype(np.float32)).astype(np.float64)
        e = float((np.abs(np.asarray(got, dtype=np.float64) - r64) / ulp).max())
        log(f"{self.PREFIX} {self.tag} {what}: kernel-vs-f64 {e:.3f} ulp  bar 2 ulp")
        if not e <= 2.0:
            self.bad.append(f"{what}: {e:.3f} ulp > 2")

    def done(self):
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)
