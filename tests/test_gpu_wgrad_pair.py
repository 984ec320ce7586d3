"""GPU parity of the pair-packed halo weight gradient for 16-channel tensors (csrc/conv_wgrad_halo2.hip, H2P; block algebra:
tests/test_wgrad_pair_host.py).

Reference = torch's CPU float64 weight gradient on the same fp32 operands.  The bars are those of tests/test_gpu_up.py's weight
gradients: relative l2 <= 1e-6, worst element <= 1e-5 of the tensor's scale.  On the same inputs conv3x3_small_wgrad_kernel (the
fp32-pipe kernel these layers ran on) is graded too and both errors are printed; the new kernel's l2 may exceed the old one's by
the factor tests/test_gpu_f32x3.py::test_wgrad_halo_f32x3_fp32_grade allows a split kernel against an fp32-pipe kernel: 1.6 x + 2^-24.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    kernels.set_option("WGRAD_PAIR", 7)          # every layer form on the pair-packed kernel, whatever the library's default routes
    yield kernels
    kernels.set_option("WGRAD_PAIR", -1)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to("cuda", f32)


def err(got, ref64):
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert torch.isfinite(got).all()
    return ((got.double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300)).item()


def err2(got, ref64):
    return ((got.double() - ref64).norm() / ref64.norm()).item()


def ref_wgrad(x64, dy64, co, ci):
    """[co][3][3][ci] float64 from NCHW float64 operands."""
    return torch.nn.grad.conv2d_weight(x64, (co, ci, 3, 3), dy64, padding=1).permute(0, 2, 3, 1).contiguous()


def grade(got, old, ref, what):
    e2, o2, em, om = err2(got, ref), err2(old, ref), err(got, ref), err(old, ref)
    print(f"{what}: l2 pair-packed {e2:.3e} small_wgrad {o2:.3e} (ratio {e2 / max(o2, 1e-30):.2f}) | worst element {em:.3e} / {om:.3e}")
    assert e2 <= 1e-6 and em <= 1e-5, f"{what}: l2 {e2:.3e}, worst element {em:.3e}"
    assert e2 <= 1.6 * o2 + 2.0 ** -24, f"{what}: pair-packed {e2:.3e} against conv3x3_small_wgrad_kernel {o2:.3e} (l2)"


PLAIN = [(2, 6, 32, 16), (1, 5, 34, 16), (2, 7, 34, 24), (1, 128, 128, 16), (2, 7, 34, 8), (1, 6, 66, 32)]


@pytest.mark.parametrize("n,h,w,co", PLAIN, ids=["16to16", "16to16_ragged", "16to24_23_classes", "16to16_long_sum", "16to8_half_block", "16to32_two_blocks"])
def test_pair_wgrad_fp32_grade(K, n, h, w, co):
    """16 -> 16 (whole and ragged tiles), the head's 16 -> 24 with 23 logical classes, and one long sum (128 x 128 pixels in one image:
    the + - - + tile signs against the truncating bf16-MFMA adder); from a zeroed gradient and onto an existing one.  Rows of dW behind
    the layer's physical channels stay untouched.

    Measured l2 (pair-packed / conv3x3_small_wgrad_kernel): 16to16 8.8e-8 / 1.3e-7, ragged 8.6e-8 / 1.3e-7, 16to24 9.9e-8 / 1.4e-7
    (ratios 0.65 - 0.72), 16to8 9.8e-8 / 1.4e-7, 16to32 9.4e-8 / 1.4e-7, long sum 2.6e-7 / 1.7e-7: ratio 1.48 - 1.51, inside the 1.6 x the split kernels are allowed (2.24 before the K
    shares of a block were summed in LDS ahead of the atomics)."""
    g = torch.Generator().manual_seed(n + h + w + co)
    x = torch.randn(n, 16, h, w, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)
    if co == 24:
        dy[:, 23] = 0.0
    ref = ref_wgrad(x.double(), dy.double(), co, 16)
    d = K.conv_desc(n, h, w, 16, co, 3, 1, 1)
    assert K.conv2d_wgrad_halo_ok(d, f32=True)
    xg, dyg = nhwc(x), nhwc(dy)
    buf = torch.full((co + 8, 3, 3, 16), 7.0, device="cuda")
    dw = buf[:co]
    dw.zero_()
    K.conv2d_wgrad_halo(d, xg, None, dyg, dw)
    old = torch.zeros(co, 3, 3, 16, device="cuda")
    K.conv2d_wgrad(d, xg, dyg, old, False)
    grade(dw.cpu(), old.cpu(), ref, "weight gradient")
    assert torch.equal(buf[co:], torch.full_like(buf[co:], 7.0)), "rows behind the layer's channels were written"
    if co == 24:
        assert not dw[23].any(), "the empty class's row"
    base = torch.randn(co, 3, 3, 16, generator=g).cuda()
    acc = base.clone()
    K.conv2d_wgrad_halo(d, xg, None, dyg, acc)
    assert err2((acc - base).cpu(), dw.cpu().double()) <= 1e-5, "accumulation onto an existing gradient"


@pytest.mark.parametrize("co,slope", [(16, 0.0), (16, 0.2), (24, 0.0)], ids=["relu", "leaky", "head_relu"])
def test_pair_wgrad_unwritten_activation(K, co, slope):
    """x = act(fma(y_prev, scale, shift)) applied while staging (engine.LazyAct), ReLU and a leaky slope; zero padding stays zero
    (shift != 0 would otherwise leak into the halo).  Measured l2 pair-packed / small_wgrad: relu 1.3e-7 / 1.4e-7, leaky 1.2e-7 / 1.6e-7,
    head 1.1e-7 / 1.3e-7 (ratios 0.74 - 0.93)."""
    from uda_aerial_semantic_segmentation_research_amd.engine import LazyAct
    n, h, w = 2, 9, 66
    g = torch.Generator().manual_seed(co + int(10 * slope))
    y_prev = (torch.randn(n, h, w, 16, generator=g) * 1.5 + 0.3).cuda()
    sc = (torch.rand(16, generator=g) + 0.5).cuda()
    sh = (torch.randn(16, generator=g) * 0.5).cuda()
    z = LazyAct(y_prev, sc, sh, 1, slope).materialize()
    dy = torch.randn(n, h, w, co, generator=g).cuda()
    ref = ref_wgrad(z.cpu().permute(0, 3, 1, 2).double(), dy.cpu().permute(0, 3, 1, 2).double(), co, 16)
    d = K.conv_desc(n, h, w, 16, co, 3, 1, 1)
    dw = torch.full((co, 3, 3, 16), float("nan"), device="cuda")
    K.conv2d_wgrad_bnin(d, y_prev, sc, sh, 1, slope, dy, dw, False)
    K.set_option("WGRAD_PAIR", 0)
    try:
        old = torch.full((co, 3, 3, 16), float("nan"), device="cuda")
        K.conv2d_wgrad_bnin(d, y_prev, sc, sh, 1, slope, dy, old, False)
    finally:
        K.set_option("WGRAD_PAIR", 7)
    grade(dw.cpu(), old.cpu(), ref, "weight gradient over an unwritten activation")


def test_pair_wgrad_slice_leaves_the_other_columns(K):
    """The slice form (rows of ldw channels, the launch fills [c_off, c_off + 16)): the columns outside the slice are untouched."""
    n, h, w, co, ldw, c_off = 1, 6, 32, 16, 48, 16
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 16, h, w, generator=g)
    dy = torch.randn(n, co, h, w, generator=g)
    ref = ref_wgrad(x.double(), dy.double(), co, 16)
    dw = torch.full((co, 3, 3, ldw), 7.0, device="cuda")
    dw[..., c_off:c_off + 16] = 0.0
    K.conv2d_wgrad_halo_slice(K.conv_desc(n, h, w, 16, co, 3, 1, 1), nhwc(x), nhwc(dy), dw, c_off)
    got = dw.cpu()
    assert err2(got[..., c_off:c_off + 16], ref) <= 1e-6 and err(got[..., c_off:c_off + 16], ref) <= 1e-5
    assert (got[..., :c_off] == 7.0).all() and (got[..., c_off + 16:] == 7.0).all()


def test_pair_wgrad_any_block_count_gives_the_same_sums(K):
    """The tile sequence split over 1, 7 or 600 blocks (more than there are tiles): the same gradient to atomics order."""
    n, h, w = 2, 10, 70
    g = torch.Generator().manual_seed(8)
    x, dy = torch.randn(n, 16, h, w, generator=g), torch.randn(n, 16, h, w, generator=g)
    ref = ref_wgrad(x.double(), dy.double(), 16, 16)
    d = K.conv_desc(n, h, w, 16, 16, 3, 1, 1)
    for blocks in (1, 7, 600):
        K.set_option("WGRAD_PAIR_BLOCKS", blocks)
        try:
            dw = torch.zeros(16, 3, 3, 16, device="cuda")
            K.conv2d_wgrad_halo(d, nhwc(x), None, nhwc(dy), dw)
        finally:
            K.set_option("WGRAD_PAIR_BLOCKS", -1)
        assert err2(dw.cpu(), ref) <= 1e-6 and err(dw.cpu(), ref) <= 1e-5, blocks


@pytest.mark.parametrize("n,ha,wa", [(2, 4, 16), (1, 5, 34)], ids=["a_2x4x16x32", "ragged_two_tiles"])
def test_pair_wgrad_upsampled_source(K, n, ha, wa):
    """32 -> 16 over nearest_x2(a), no skip half: dy paired, a's rows gathered at half resolution; onto an existing gradient too.
    Measured l2 pair-packed / small_wgrad: 8.8e-8 / 1.5e-7 and 1.1e-7 / 1.5e-7 (ratios 0.60, 0.74)."""
    g = torch.Generator().manual_seed(n + ha + wa)
    a = torch.randn(n, 32, ha, wa, generator=g)
    dy = torch.randn(n, 16, 2 * ha, 2 * wa, generator=g)
    up = F.interpolate(a, scale_factor=2, mode="nearest")
    ref = ref_wgrad(up.double(), dy.double(), 16, 32)
    d = K.conv_desc(n, 2 * ha, 2 * wa, 32, 16, 3, 1, 1)
    assert K.conv2d_wgrad_halo_ok(d, 32, f32=True)
    dw = torch.zeros(16, 3, 3, 32, device="cuda")
    K.conv2d_wgrad_halo(d, nhwc(a), None, nhwc(dy), dw, up=True)
    old = torch.zeros(16, 3, 3, 32, device="cuda")
    K.conv2d_wgrad_part(d, nhwc(a), 0, True, nhwc(dy), old, False)
    grade(dw.cpu(), old.cpu(), ref, "weight gradient over an up-sampled source")
    base = torch.randn(16, 3, 3, 32, generator=g).cuda()
    acc = base.clone()
    K.conv2d_wgrad_halo(d, nhwc(a), None, nhwc(dy), acc, up=True)
    assert err2((acc - base).cpu(), dw.cpu().double()) <= 1e-5, "accumulation onto an existing gradient"
