#!/usr/bin/env python
"""Measured error of the distillation kernels (csrc/distill.hip) on the cases of tests/test_gpu_distill.py and of the trainer on
the cases of tests/test_gpu_distill_trainer.py, on one MI355X.

Kernel level: every case of the test through tests/_distill_ref.py's grading; per case the worst kernel-vs-float64 and
fp32-leg-vs-float64 deviation (normalised by the magnitudes defined there) for the loss, the gradient and the column sums, the bar
max(4 x the leg's, 2^-22) as the worst ratio e / bar, and whether every bit-exact statement held.
Network level: the trainer test's figures as it logs them -- the reported losses against the float64 composition, and per
parameter tensor the kernel leg against the float64-gradient leg beside d (the fp32 composition leg) and the run-to-run spread.

    python tools/grade_distill.py [--out profiles/distill_grade.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import _distill_ref as D  # noqa: E402
import test_gpu_distill as T  # noqa: E402
import test_gpu_distill_trainer as TT  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import _lib  # noqa: E402

FIG = re.compile(r"loss-grade (.*?) (loss|dlogits|colsum): kernel-vs-f64 (\S+)\s+f32-vs-f64 (\S+)\s+bar (\S+)\s+e/bar (\S+)")


def summarise(tag, run):
    """One line per case: worst e, d and e / bar per output kind, and the count of failed statements."""
    got = []
    g = run(got.append)
    worst = {}
    for line in got:
        m = FIG.match(line)
        if m and m.group(1).startswith("distill"):
            what = m.group(2)
            e, d, ratio = float(m.group(3)), float(m.group(4)), float(m.group(6))
            w = worst.setdefault(what, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], e), max(w[1], d), max(w[2], ratio)
    cells = "  ".join(f"{k} e {worst[k][0]:.2e} d {worst[k][1]:.2e} e/bar {worst[k][2]:.3f}" for k in ("loss", "dlogits", "colsum")
                      if k in worst)
    return f"{tag:<34} {cells}  statements {len(got)} failed {len(g.bad)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    be = T.GpuBackend()
    lines = ["kernel level: worst normalised deviation per case (e: kernel vs float64, d: fp32 leg vs float64, bar max(4 d, 2^-22))"]
    for shape in D.SHAPES:
        for c in D.CLASSES:
            lines.append(summarise(f"{shape[0]}x{shape[1]} C={c}",
                                   lambda log: D.grade_case(be, shape[0], shape[1], c, 100 * c + shape[1], log)))
    for kind in D.ROW_KINDS:
        for c in (5, 23):
            lines.append(summarise(f"1x1 C={c} {kind}", lambda log: D.grade_case(be, 1, 1, c, 7 * c, log, row_kind=kind)))
    for c, ldc, ldt in ((5, 8, 32), (5, 16, 8), (23, 24, 32)):
        lines.append(summarise(f"3x85 C={c} ldc={ldc} ldt={ldt}",
                               lambda log: D.grade_case(be, 3, 85, c, 41, log, ldc=ldc, ldt=ldt, combos=D.COVER)))
    lines.append(summarise(f"{D.BIG[0]}x{D.BIG[1]} C=23", lambda log: D.grade_case(be, D.BIG[0], D.BIG[1], 23, 5, log, combos=D.COVER[:3],
                                                                                  weight_variants=False)))
    got = []
    bad = sum(len(D.grade_share(be, b, p, c, 11 * c + p, got.append).bad) for c in D.CLASSES for b, p in ((1, 1), (3, 85), (2, 1025)))
    lines.append(f"conf_share: {len(got)} exact statements (above, nonfinite, share against the mirror), failed {bad}")
    lines.append("")
    lines.append("network level: tests/test_gpu_distill_trainer.py (r18, 2 x 3 x 64 x 64, 5 classes, symmetric, lambda_soft 0.7)")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "dev.log")
        old = os.environ.get("UDASEG_DEVIATION_LOG")
        os.environ["UDASEG_DEVIATION_LOG"] = path
        try:
            TT.test_one_distill_step_reports_the_textbook_losses_and_leaves_the_teacher_alone()
            TT.test_parameter_gradients_meet_the_network_level_bar()
        finally:
            if old is None:
                del os.environ["UDASEG_DEVIATION_LOG"]
            else:
                os.environ["UDASEG_DEVIATION_LOG"] = old
        lines += [l.rstrip("\n") for l in open(path)]
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
            fh.write("# python tools/grade_distill.py: the distillation kernels against their float64 restatement (tests/_distill_ref.py) "
                     f"and one DistillTrainer step on 1 x {torch.cuda.get_device_name(0)}.  One run.\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
