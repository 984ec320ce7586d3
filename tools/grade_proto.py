#!/usr/bin/env python
"""Measured error of the prototype kernels (csrc/proto.hip) on the cases of tests/test_gpu_proto.py, on one MI355X.

Sums: udaseg_proto_accumulate's float64 cells against the numpy float64 mirror at 65537 pixels of randn + 2 under every label
pattern of the tests, as the worst ratio error / bar over the cells (bar: n_c 2^-52 sum|x|, derived), beside the same ratio of an
fp32 accumulation (torch index_add_ in fp32 on the device): what the bar would catch.
Rectified probabilities: per case the torch fp32 composition's error against the float64 mirror, the bar max(2 x that, 4 x 2^-23),
the kernel's error, the share of pixels whose float64 top-two gap is within twice the bar (excluded from the winner check), whether
the winner agrees elsewhere, and the share of pixels whose rectified winner differs from the raw one.

    python tools/grade_proto.py [--out profiles/proto_grade.txt]
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

import _proto_ref as R  # noqa: E402
import test_gpu_proto as T  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    lines = [f"{'sums: C, D, ldf':<18} {'pattern':<12} {'kernel err/bar':>15} {'sq err/bar':>11} {'fp32 index_add_ err/bar':>24}"]
    pixels = T.PIXELS[-1]
    for classes, dim, ldf in T.SHAPES:
        g = torch.Generator().manual_seed(1000 * classes + pixels % 997)
        feat = T._features(pixels, dim, ldf, g)
        for pattern in T.PATTERNS:
            lab = T._labels(pattern, pixels, classes, g)
            ref_sums, ref_sq, counts, abs_sums, abs_sq = R.accumulate_mirror(feat[:, :dim].numpy(), lab.numpy(), classes)
            bar_s, bar_q = R.sum_bars(counts, abs_sums, abs_sq)
            sums, sq, cnt = T._accumulators(classes, dim)
            K.proto_accumulate(feat.cuda(), ldf, dim, lab.cuda(), pixels, classes, sums, sq, cnt)
            live = bar_s > 0
            if not live.any():
                lines.append(f"{classes:>3}, {dim:>2}, {ldf:>2}        {pattern:<12} {'no class pixels':>15}")
                continue
            err = np.abs(sums.cpu().numpy().reshape(classes, dim) - ref_sums)
            errq = np.abs(sq.cpu().numpy() - ref_sq)
            keep = lab.long() < classes
            low = torch.zeros(classes, dim, device="cuda").index_add_(0, lab.long()[keep].cuda(), feat[:, :dim][keep].cuda())
            err32 = np.abs(low.double().cpu().numpy() - ref_sums)
            lines.append(f"{classes:>3}, {dim:>2}, {ldf:>2}        {pattern:<12} {float((err[live] / bar_s[live]).max()):>15.2e} "
                         f"{float((errq[bar_q > 0] / bar_q[bar_q > 0]).max()):>11.2e} "
                         f"{float((err32[live] / bar_s[live]).max()):>24.2e}")
    lines.append("")
    lines.append(f"{'rectify: C, D, scale, tau_scale, probs':<40} {'torch err':>10} {'bar':>10} {'kernel err':>11} {'excluded':>9} "
                 f"{'winner ok':>10} {'winner moved':>13}")
    for C, D, scale, tau_scale, probs in T.GRADE_CASES:
        ldc = 4 * ((C + 3) // 4)
        kernel = lambda f, s, p, it: T._kernel_rectify(f, D, s, ldc, C, probs, p, np.ones(C), it)[:, :C]      # noqa: E731
        fig = T.grade_case(C, D, scale, tau_scale, probs, rectify=kernel)
        lines.append(f"{str((C, D, scale, tau_scale, probs)):<40} {fig['torch_err']:>10.2e} {fig['bar']:>10.2e} "
                     f"{fig['kernel_err']:>11.2e} {fig['excluded']:>9.4f} {str(fig['winner_ok']):>10} {fig['moved_winner']:>13.4f}")
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
            fh.write("# python tools/grade_proto.py: the prototype kernels against their float64 mirrors (tests/_proto_ref.py) on "
                     f"1 x {torch.cuda.get_device_name(0)}.  One run.\n")
            fh.write(f"# sums at {pixels} pixels of randn + 2; rectify at {T.GRADE_PIXELS} pixels per case; errors are max abs\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
