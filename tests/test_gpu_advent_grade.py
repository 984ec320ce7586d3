"""The output-space adaptation kernels (csrc/advent.hip: udaseg_selfinfo_fwd, udaseg_selfinfo_bwd, udaseg_entropy_loss) against
the float64 restatement of tests/_entropy_ref.py (proven against torch's double-precision autograd by tests/test_advent_host.py),
called at kernel level through kernels.py.

The bar is the one of tests/test_gpu_loss_grade.py: with e = |kernel - f64| / magnitude and d = |fp32 leg - f64| / magnitude
element-wise, max(e) <= max(4 x max(d), 2^-22), scalars included, no element masked out; bf16 maps get half a bf16 ulp of the
reference value on top, bf16 gradients of the maps are rounded once on the host so both legs and the kernel see the same numbers.
Logits sit in padded NHWC buffers whose pad lanes hold 7.0 and one lane 1e30; every output buffer is pre-filled with NaN; the pad
lanes of the maps and of every gradient must come back exactly 0; the loss must be the same bits with and without its gradient.

Shapes: classes 2, 5, 12, 23, 32 (ldc 4, 8, 12, 24, 32; the bf16 maps' width 8 and 16 differs from ldc at 2 and 12) by pixels 1,
255, 257, and 1024 * 256 + 3 pixels at 23 classes, where one thread takes a second grid-stride pixel.  Rows: random at scale 3,
uniform (entropy 1), saturated (80 in one lane), one lane -inf -- mixed into every case, and each alone at one pixel.
tests/test_advent_host.py runs the same grading with the float32 leg (and six mutations of it) in the kernels' place.  Set
UDASEG_DEVIATION_LOG to a file name to collect the figures.
"""
import os

import numpy as np
import pytest
import torch

import _entropy_ref as E
from _entropy_ref import F32

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


class GpuBackend:
    """tests/_entropy_ref.py's operations on the HIP kernels, numpy in and out."""
    def __init__(self):
        from uda_aerial_semantic_segmentation_research_amd import kernels as K
        self.K = K

    def selfinfo_fwd(self, zbuf, classes, cpad, bf16, want_entropy):
        pixels, ldc = zbuf.shape
        maps = nans((pixels, cpad), torch.bfloat16 if bf16 else torch.float32)
        ent = nans((pixels,)) if want_entropy else None
        self.K.selfinfo_fwd(dev(zbuf), pixels, classes, ldc, maps, cpad, ent)
        return host(maps), None if ent is None else host(ent)

    def selfinfo_bwd(self, zbuf, dbuf, classes, bf16):
        pixels, ldc = zbuf.shape
        d = nans((pixels, ldc))
        dm = dev(dbuf, torch.bfloat16 if bf16 else None)          # exact: the bf16 cases hold bf16-rounded values (1e30 rounds, unread)
        self.K.selfinfo_bwd(dev(zbuf), dm, pixels, classes, ldc, dbuf.shape[1], d)
        return host(d)

    def entropy_loss(self, zbuf, classes, kind, want_grad, want_entropy):
        pixels, ldc = zbuf.shape
        parts = nans((self.K.seg_partials(),), torch.float64)
        loss = nans(())
        d = nans((pixels, ldc)) if want_grad else None
        ent = nans((pixels,)) if want_entropy else None
        self.K.entropy_loss(dev(zbuf), pixels, classes, ldc, kind, parts, loss, d, ent)
        return F32(host(loss)), None if d is None else host(d), None if ent is None else host(ent)


@pytest.fixture(scope="module")
def backend():
    return GpuBackend()


@pytest.mark.parametrize("classes", E.CLASSES)
@pytest.mark.parametrize("pixels", E.SMALL_PIXELS)
def test_kernels_meet_the_bar(backend, pixels, classes):
    E.grade_case(backend, pixels, classes, 100 * classes + pixels, _log).done()


@pytest.mark.parametrize("classes", E.CLASSES)
@pytest.mark.parametrize("row_kind", E.ROW_KINDS)
def test_kernels_meet_the_bar_on_single_rows(backend, row_kind, classes):
    E.grade_case(backend, 1, classes, 7 * classes, _log, row_kind=row_kind).done()


def test_kernels_meet_the_bar_past_the_grid(backend):
    """1024 * 256 + 3 pixels: three threads take a second grid-stride pixel (about 25 MB of logits at 23 classes)."""
    E.grade_case(backend, E.BIG_PIXELS, 23, 5, _log).done()
