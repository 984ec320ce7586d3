"""The prototype contrast kernels (csrc/proto_contrast.hip: udaseg_proto_assign, udaseg_proto_contrast_fwd_bwd) against the float64
restatement of tests/_contrast_ref.py (proven against torch's double-precision autograd by tests/test_contrast_host.py), called at
kernel level through kernels.py.

The bar is the project's, ``_norm_ref.bar``: with e = |kernel - f64| / magnitude and d = |fp32 leg - f64| / magnitude element-wise,
max(e) <= max(4 x max(d), 2^-22), the loss scalar included, no element masked out; the magnitudes are defined in
tests/_contrast_ref.py.  The features and the soft target sit in padded buffers whose pad lanes hold 7.0 and one lane 1e30; every
output buffer is pre-filled with NaN; pad lanes of the gradient and every lane of a void pixel must come back exactly 0; the loss
must be the same bits with and without dfeat and across two calls, the assignment the same bits across two calls; the four counters
must equal the mirror's exactly.

Shapes: dim 4, 16, 64 with ldf = dim and dim + 4; classes 2, 5, 23, 32; batch x pix_per_image 1 x 1, 3 x 85 (image boundaries inside
a wave), 1 x 257; ldt != ldc both ways; 1024 * 256 + 3 pixels at 16 x 23, where a lane takes a second grid-stride pixel.  Both
forms, every reduction, with both weights, each alone and none.  Rows (``make_case``): random features at the scale of the
prototypes' scatter, a feature on its prototype, a feature 1e3 away, label 255, the label of an unseen class, soft mass on unseen
classes only, a target of 1.5, NaN target rows, a NaN / inf feature, weight_px 0 / negative / NaN, an image with weight_img 0 --
mixed into every case and each alone at one pixel.  Whole calls with no class seen and with inv_tau == 0 return loss 0 and
gradient 0.  tests/test_contrast_host.py runs the same grading with the float32 leg (and six mutations of it) in the kernels' place.
Set UDASEG_DEVIATION_LOG to a file name to collect the figures.
"""
import os

import numpy as np
import pytest
import torch

import _contrast_ref as R
from _contrast_ref import F32

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


class GpuBackend:
    """tests/_contrast_ref.py's operations on the HIP kernels, numpy in and out."""
    def __init__(self):
        from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K
        _lib.require_gpu()
        self.K = K
        self._held = {}

    def dev(self, a):
        """The device copy of a host array, made once per array (a case calls with the same buffers many times)."""
        if a is None:
            return None
        hit = self._held.get(id(a))
        if hit is None or hit[0] is not a:
            if len(self._held) > 16:
                self._held.clear()
            hit = self._held[id(a)] = (a, torch.from_numpy(np.ascontiguousarray(a)).cuda())
        return hit[1]

    def bank(self, proto, seen, inv_tau):
        return (self.dev(proto), self.dev(seen), torch.tensor([inv_tau], dtype=torch.float32, device="cuda"))

    def contrast(self, fbuf, dim, labels, tbuf, classes, wpx, wimg, batch, ppi, proto, seen, inv_tau, reduction, want_grad):
        K = self.K
        pixels, ldf = fbuf.shape
        denom = None
        if reduction == "weighted_mean":
            denom = nans((1,), torch.float64)
            K.pixel_weight_sum(self.dev(wpx), self.dev(wimg), batch, ppi, nans((3 * K.seg_partials(),), torch.float64), denom,
                               torch.zeros(2, dtype=torch.int64, device="cuda"))
        loss = nans(())
        d = nans((pixels, ldf)) if want_grad else None
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        K.proto_contrast_fwd_bwd(self.dev(fbuf), ldf, dim, self.dev(labels), self.dev(tbuf), 0 if tbuf is None else tbuf.shape[1],
                                 self.dev(wpx), self.dev(wimg), batch, ppi, classes, *self.bank(proto, seen, inv_tau),
                                 reduction == "mean", denom, nans((K.seg_partials(),), torch.float64), loss, d, stats)
        host = lambda t: None if t is None else t.cpu().numpy()              # noqa: E731
        return F32(host(loss)), host(d), host(stats)

    def assign(self, fbuf, dim, classes, ldc, proto, seen, inv_tau):
        pixels, ldf = fbuf.shape
        out = nans((pixels, ldc))
        self.K.proto_assign(self.dev(fbuf), ldf, dim, classes, ldc, *self.bank(proto, seen, inv_tau), pixels, out)
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def backend():
    return GpuBackend()


@pytest.mark.parametrize("classes", R.CLASSES)
@pytest.mark.parametrize("dim", R.DIMS)
def test_kernels_meet_the_bar(backend, dim, classes):
    for batch, ppi in R.SHAPES:
        seed = 100 * classes + dim + ppi
        R.grade_case(backend, batch, ppi, classes, dim, seed, _log).done()
        R.grade_case(backend, batch, ppi, classes, dim, seed + 1, _log, ldf=dim + 4, combos=R.COVER, weight_variants=False).done()


@pytest.mark.parametrize("row_kind", R.ROW_KINDS)
def test_kernels_meet_the_bar_on_single_rows(backend, row_kind):
    for classes in R.CLASSES:
        R.grade_case(backend, 1, 1, classes, 16, 7 * classes, _log, row_kind=row_kind).done()
    R.grade_case(backend, 1, 1, 23, 64, 3, _log, row_kind=row_kind, ldf=68, combos=R.COVER, weight_variants=False).done()


@pytest.mark.parametrize("classes,ldt,ldc", [(5, 32, 8), (5, 8, 16), (23, 32, 24), (23, 24, 32)])
def test_kernels_meet_the_bar_with_unequal_strides(backend, classes, ldt, ldc):
    R.grade_case(backend, 3, 85, classes, 16, 41, _log, ldf=20, ldt=ldt, ldc=ldc, combos=R.COVER).done()


def test_kernels_meet_the_bar_past_the_grid(backend):
    """1024 * 256 + 3 pixels: three lanes take a second grid-stride pixel (about 17 MB of features at 16 channels)."""
    R.grade_case(backend, R.BIG[0], R.BIG[1], 23, 16, 5, _log, combos=R.COVER[:2], weight_variants=False).done()


@pytest.mark.parametrize("classes", [5, 23])
def test_a_call_without_seen_classes_or_temperature_is_zero(backend, classes):
    R.grade_case(backend, 3, 85, classes, 16, 9, _log, seen=np.zeros(classes, dtype=np.int32)).done()
    R.grade_case(backend, 3, 85, classes, 16, 9, _log, inv_tau=0.0).done()
