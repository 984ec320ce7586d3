"""The glue between the convolutions -- max pool forward / backward with its stored tap bytes, nearest and bilinear x2 up-sampling +
concat forward / backward, nchw_to_nhwc, the bf16 cast, fill / axpy / scale / add_i64 (csrc/pool_resize.hip in both storages,
csrc/bilinear.hip; the cast: csrc/elem_bf16.hip) -- element by element against the float64 restatement of tests/_pool_ref.py, which
tests/test_pool_ref_host.py proves against torch's float64 CPU results and shows to reject every mutant through the checks made here.

Two tiers.  EXACT: operands are integers in [-128, 128] (bf16-representable; the pools draw from five values so that maxima tie),
every bilinear weight is a multiple of 1/16, so every partial sum is exact in fp32 in any order and the kernel must equal float64,
rounded once to nearest even where the store is bf16, bit for bit.  ARBITRARY: operands are randn * 2 ** randint(-6, 6); selections
and copies (pool forward, nearest forward, dskip without accumulate, nchw_to_nhwc, cast) stay bit for bit, sums take the one bar of
tests/test_gpu_norm_grade.py: max(e) <= max(4 x max(d), 2^-22) with e = |kernel - f64| / magnitude and d = |fp32 leg - f64| /
magnitude, plus half a bf16 ulp at the float64 value for a bf16 output.

Every output is a slice of a larger allocation filled with NaN (with ``old`` where the call accumulates) between two 256-element
sentinel guards whose bits must survive; every input is a slice of a larger allocation with NaN on either side.  Nothing is masked.
The shapes are the smallest that reach each edge; the launch-path cases are the smallest that cross each threshold of the launch
arithmetic (tests/test_pool_ref_host.py has the arithmetic), one per kernel, exact tier.

Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _pool_ref as P
from _norm_ref import bf16_round

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
STORES = (P.FP32, P.BF16)
DT = {P.FP32: torch.float32, P.BF16: torch.bfloat16}
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    return kernels


class Buf:
    """A tensor that is a slice of a larger allocation.  role "out": NaN inside (``init`` where the call accumulates; all-ones
    bytes for integers), 256 sentinel elements on either side.  role "in": the values inside, NaN (all-ones bytes) on either side."""
    def __init__(self, shape, dtype=torch.float32, init=None, role="out"):
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.n, self.fl = int(np.prod(shape)), dtype.is_floating_point
        nan = P.NAN if self.fl else (0xFF if dtype == torch.uint8 else -1)
        guard = nan if role == "in" else (R.SENTINEL if self.fl else (0xA5 if dtype == torch.uint8 else -12345))
        self.whole = torch.full((self.n + 2 * R.GUARD,), guard, dtype=dtype, device="cuda")
        self.t = self.whole[R.GUARD:R.GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0
        if init is None:
            self.t.fill_(nan)
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype).view(shape))
        self.guards = self._guards().clone()

    def _guards(self):
        w = self.whole.view(BITS[self.whole.element_size()])
        return torch.cat([w[:R.GUARD], w[R.GUARD + self.n:]])

    def intact(self):
        return torch.equal(self._guards(), self.guards)

    def host(self):
        return (self.t.float() if self.fl else self.t).cpu().numpy()


def src(a, dtype=torch.float32):
    return Buf(np.shape(a), dtype, a, "in")


def guards(G, what, *bufs):
    ok = all(b.intact() for b in bufs if b is not None)
    G.note(what + " guards", ok, "intact" if ok else "OVERWRITTEN", quiet=True)


# ------------------------------------------------------------------------------------- launches into the test's own buffers
def pool_fwd(K, x, y, idx):
    n, h, w, c = x.shape
    if x.dtype == torch.bfloat16:
        K.check(K.ops.udaseg_maxpool3x3s2_fwd_bf16(x, y, idx, n, h, w, c, None), "maxpool_fwd_bf16")
    else:
        K.check(K.ops.udaseg_maxpool3x3s2_fwd(x, y, idx, n, h, w, c, None), "maxpool_fwd")


def nearest_fwd(K, a, skip, out, cb):
    n, h, w, ca = a.shape
    if a.dtype == torch.bfloat16:          # as kernels.upsample2x_concat_fwd: 16-byte vectors, 8 bf16 channels == 4 fp32 "channels"
        ca, cb = ca // 2, cb // 2
    K.check(K.ops.udaseg_upsample2x_concat_fwd(a, skip, out, n, h, w, ca, cb, None), "upsample2x_concat_fwd")


def bilinear_fwd(K, a, skip, out, cb):
    n, h, w, ca = a.shape
    K.check(K.ops.udaseg_upsample2x_bilinear_concat_fwd(a, skip, out, n, h, w, ca, cb, int(a.dtype == torch.bfloat16), None),
            "upsample2x_bilinear_concat_fwd")


def layout(K, x, y):
    n, c, h, w = x.shape
    if y.dtype == torch.bfloat16:
        K.check(K.ops.udaseg_nchw_to_nhwc_bf16(x, y, n, c, h, w, y.shape[-1], None), "nchw_to_nhwc_bf16")
    else:
        K.check(K.ops.udaseg_nchw_to_nhwc(x, y, n, c, h, w, y.shape[-1], None), "nchw_to_nhwc")


# ------------------------------------------------------------------------------------------------------------------- max pool
def run_pool_fwd(K, G, shape, kind, tier, store):
    x = P.pool_input(shape, kind, tier, store)
    y_ref, tap_ref = P.maxpool(x)
    xb, yb, ib = src(x, DT[store]), Buf(y_ref.shape, DT[store]), Buf(y_ref.shape, torch.uint8)
    pool_fwd(K, xb.t, yb.t, ib.t)
    what = f"{shape} {kind} {tier}"
    G.exact(what + " y", yb.host(), y_ref)
    G.equal(what + " idx", ib.host(), tap_ref)
    guards(G, what, yb, ib)


def run_pool_bwd(K, G, shape, kind, tier, store):
    tap, dy = P.pool_bwd_case(shape, kind, tier, store)
    r64, mag = P.maxpool_bwd(dy, tap, shape)
    r32, _ = P.maxpool_bwd(dy, tap, shape, F32)
    ib, dyb, dxb = src(tap, torch.uint8), src(dy, DT[store]), Buf(shape, DT[store])
    K.maxpool_bwd(dyb.t, ib.t, dxb.t)
    what = f"{shape} {kind} {tier}"
    G.tier(what + " dx", tier, dxb.host(), r64, r32, mag, store == P.BF16)
    guards(G, what, dxb)


@pytest.mark.parametrize("kind", P.POOL_KINDS)
@pytest.mark.parametrize("store", STORES)
def test_maxpool_forward(K, store, kind):
    """y by bits (NaN at the same positions) and the stored tap bytes exactly: the first valid tap starts, > or NaN replaces."""
    G = P.PoolGrader(f"maxpool_fwd {store}")
    for shape, k, tier in P.pool_cases(store):
        if k == kind:
            run_pool_fwd(K, G, shape, kind, tier, store)
    torch.cuda.synchronize()
    G.done()


@pytest.mark.parametrize("kind", P.POOL_KINDS)
@pytest.mark.parametrize("store", STORES)
def test_maxpool_backward(K, store, kind):
    """Every window's gradient lands on exactly the element the tap byte names, whatever made the forward choose it."""
    G = P.PoolGrader(f"maxpool_bwd {store}")
    for shape, k, tier in P.pool_cases(store):
        if k == kind:
            run_pool_bwd(K, G, shape, kind, tier, store)
    torch.cuda.synchronize()
    G.done()


@pytest.mark.parametrize("path", ["row-loop", "stride-f32", "stride-bf16"])
def test_maxpool_launch_paths(K, path):
    """row-loop: n * h = 65537 rows over gridDim.y = 65535 (fp32 backward).  stride: 257 x 257 x 16 output vectors over 4096 x 256
    threads (forward, fp32 and bf16; the bf16 shape also puts the bf16 backward past its 4096 x 256)."""
    G = P.PoolGrader(f"maxpool {path}")
    if path == "row-loop":
        run_pool_bwd(K, G, P.POOL_ROW_LOOP, "signed", "exact", P.FP32)
    else:
        store = P.FP32 if path == "stride-f32" else P.BF16
        run_pool_fwd(K, G, P.POOL_STRIDE[store], "signed", "exact", store)
        if store == P.BF16:
            run_pool_bwd(K, G, P.POOL_STRIDE[store], "signed", "exact", store)
    G.done()


# ----------------------------------------------------------------------------------------------- nearest up-sampling + concat
def run_nearest_fwd(K, G, a_shape, ca, cb, tier, store):
    d = P.up_case("nearest", a_shape, ca, cb, tier, store)
    want = P.upcat(d["a"], d["skip"])
    ab, sb, ob = src(d["a"], DT[store]), (src(d["skip"], DT[store]) if cb else None), Buf(want.shape, DT[store])
    nearest_fwd(K, ab.t, sb.t if cb else None, ob.t, cb)
    what = f"{a_shape} {ca}+{cb} {tier}"
    G.exact(what + " out", ob.host(), want)
    guards(G, what, ob)


def run_nearest_bwd(K, G, a_shape, ca, cb, tier, store, forms=("da", "dskip", "both")):
    d = P.up_case("nearest", a_shape, ca, cb, tier, store)
    n, h, w = a_shape
    r64, dskip, mag = P.upcat_bwd(d["dout"], ca)
    r32 = P.upcat_bwd(d["dout"], ca, F32)[0]
    db = src(d["dout"], DT[store])
    for form in forms:
        if form != "da" and not cb:
            continue
        what = f"{a_shape} {ca}+{cb} {tier} [{form}]"
        dab = Buf((n, h, w, ca), DT[store]) if form != "dskip" else None
        dsb = Buf((n, 2 * h, 2 * w, cb), DT[store]) if form != "da" else None
        K.upsample2x_concat_bwd(db.t, dab.t if dab else None, dsb.t if dsb else None, ca, cb)
        if dab:
            G.tier(what + " da", tier, dab.host(), r64, r32, mag, store == P.BF16)
        if dsb:
            G.exact(what + " dskip", dsb.host(), dskip)
        guards(G, what, dab, dsb)


@pytest.mark.parametrize("store", STORES)
def test_nearest_forward(K, store):
    G = P.PoolGrader(f"nearest_fwd {store}")
    for case in P.up_cases(P.NEAREST_A, store):
        run_nearest_fwd(K, G, *case, store)
    torch.cuda.synchronize()
    G.done()


@pytest.mark.parametrize("store", STORES)
def test_nearest_backward(K, store):
    """da alone, dskip alone and both in one call (the accumulate forms: tests/test_gpu_norm_grade.py)."""
    G = P.PoolGrader(f"nearest_bwd {store}")
    for case in P.up_cases(P.NEAREST_A, store):
        run_nearest_bwd(K, G, *case, store)
    torch.cuda.synchronize()
    G.done()


@pytest.mark.parametrize("path", ["row-loop", "forward-cap", "stride-bf16"])
def test_nearest_launch_paths(K, path):
    """row-loop: 65537 rows of da over gridDim.y = 65535 (fp32).  forward-cap: 4 x 182 x 182 x 16 vectors, more than the 4096 x 512
    of the 2-per-thread launch.  stride-bf16: 363 x 363 x 8 vectors of da over 4096 x 256 threads."""
    G = P.PoolGrader(f"nearest {path}")
    if path == "row-loop":
        a, ca, cb = P.NEAREST_ROW_LOOP
        run_nearest_bwd(K, G, a, ca, cb, "exact", P.FP32, forms=("both",))
    elif path == "forward-cap":
        a, ca, cb = P.NEAREST_FWD_CAP
        run_nearest_fwd(K, G, a, ca, cb, "exact", P.FP32)
    else:
        a, ca, cb = P.NEAREST_BF16_STRIDE
        run_nearest_bwd(K, G, a, ca, cb, "exact", P.BF16, forms=("da",))
    G.done()


# ---------------------------------------------------------------------------------------------- bilinear up-sampling + concat
@pytest.mark.parametrize("store", STORES)
def test_bilinear_forward(K, store):
    """Every element of cat(interpolate(a, 2, "bilinear"), skip): the clamps of the first and last row and column, 1-pixel extents,
    vector counts 1, 3 and 4 (+ skip), and the rounding of the bf16 store."""
    G = P.PoolGrader(f"bilinear_fwd {store}")
    for a_shape, ca, cb, tier in P.up_cases(P.BILINEAR_A, store):
        d = P.up_case("bilinear", a_shape, ca, cb, tier, store)
        r64, mag = P.bilinear_upcat(d["a"], d["skip"])
        r32, _ = P.bilinear_upcat(d["a"], d["skip"], F32)
        ab, sb, ob = src(d["a"], DT[store]), (src(d["skip"], DT[store]) if cb else None), Buf(r64.shape, DT[store])
        bilinear_fwd(K, ab.t, sb.t if cb else None, ob.t, cb)
        what = f"{a_shape} {ca}+{cb} {tier}"
        got = ob.host()
        G.tier(what + " out", tier, got, r64, r32, mag, store == P.BF16)
        if cb:
            G.exact(what + " skip channels", got[..., ca:], d["skip"])
        guards(G, what, ob)
    torch.cuda.synchronize()
    G.done()


FORMS = [(False, False), (True, False), (False, True), (True, True)]              # (accumulate_da, accumulate_dskip)


@pytest.mark.parametrize("store", STORES)
def test_bilinear_backward(K, store):
    """da and dskip plain, with each accumulate flag alone (the other output is overwritten: its buffer holds NaN) and with both."""
    G = P.PoolGrader(f"bilinear_bwd {store}")
    bf = store == P.BF16
    for a_shape, ca, cb, tier in P.up_cases(P.BILINEAR_A, store):
        d = P.up_case("bilinear", a_shape, ca, cb, tier, store)
        n, h, w = a_shape
        r64, dskip, mag = P.bilinear_upcat_bwd(d["dout"], ca)
        r32 = P.bilinear_upcat_bwd(d["dout"], ca, F32)[0]
        db = src(d["dout"], DT[store])
        for acc_a, acc_s in FORMS:
            if acc_s and not cb:
                continue
            what = f"{a_shape} {ca}+{cb} {tier} acc={int(acc_a)}{int(acc_s)}"
            dab = Buf((n, h, w, ca), DT[store], d["old_a"] if acc_a else None)
            dsb = Buf((n, 2 * h, 2 * w, cb), DT[store], d["old_s"] if acc_s else None) if cb else None
            K.upsample2x_bilinear_concat_bwd(db.t, dab.t, dsb.t if cb else None, ca, cb, accumulate_da=acc_a, accumulate_dskip=acc_s)
            if acc_a:
                a64, amag = P.accumulated(d["old_a"], r64, mag)
                G.tier(what + " da", tier, dab.host(), a64, P.accumulated(d["old_a"], r32, mag, F32)[0], amag, bf)
            else:
                G.tier(what + " da", tier, dab.host(), r64, r32, mag, bf)
            if cb and acc_s:
                s64, smag = P.accumulated(d["old_s"], dskip.astype(F64), np.abs(dskip.astype(F64)))
                G.tier(what + " dskip", tier, dsb.host(), s64, P.accumulated(d["old_s"], dskip, 0, F32)[0], smag, bf)
            elif cb:
                G.exact(what + " dskip", dsb.host(), dskip)
            guards(G, what, dab, dsb)
    torch.cuda.synchronize()
    G.done()


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("value", [P.INF, -P.INF, P.NAN], ids=["inf", "-inf", "nan"])
def test_bilinear_does_not_swallow_non_finite_values(K, store, value):
    """An Inf or NaN in one pixel of a (of dout) reaches every output (every element of da) that has a non-zero weight on it.
    Nothing is asserted about the zero-weight taps of the clamped edges."""
    G = P.PoolGrader(f"bilinear non-finite {store} {value}")
    ca = P.VEC[store] * 3
    reached = (lambda t: np.isnan(t)) if value != value else (lambda t: ~np.isfinite(t))
    for a_shape in ((1, 1, 1), (1, 3, 5), (1, 9, 1)):
        n, h, w = a_shape
        d = P.up_case("bilinear", a_shape, ca, 0, "exact", store)
        for py, px in {(0, 0), (h // 2, w // 2), (h - 1, w - 1)}:
            a = d["a"].copy()
            a[0, py, px] = value
            ab, ob = src(a, DT[store]), Buf((n, 2 * h, 2 * w, ca), DT[store])
            bilinear_fwd(K, ab.t, None, ob.t, 0)
            hit = P.bilinear_weights((h, w), py, px) > 0
            got = ob.host()[0]
            G.note(f"{a_shape} a[{py},{px}] forward", bool(reached(got[hit]).all()),
                   f"{int(reached(got[hit]).all(axis=-1).sum())} of {int(hit.sum())} weighted outputs reached")
        for Y, X in {(0, 0), (h, w), (2 * h - 1, 2 * w - 1)}:
            dout = d["dout"].copy()
            dout[0, Y, X] = value
            db, dab = src(dout, DT[store]), Buf((n, h, w, ca), DT[store])
            K.upsample2x_bilinear_concat_bwd(db.t, dab.t, None, ca, 0)
            hit = np.outer(P.bilinear_matrix(h)[Y], P.bilinear_matrix(w)[X]) > 0
            got = dab.host()[0]
            G.note(f"{a_shape} dout[{Y},{X}] backward", bool(reached(got[hit]).all()),
                   f"{int(reached(got[hit]).all(axis=-1).sum())} of {int(hit.sum())} weighted elements of da reached")
    G.done()


def torch_nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("path", ["forward", "backward"])
def test_bilinear_launch_paths(K, path):
    """4 x 363 x 363 x 4 output vectors (forward) and 363 x 363 x 16 vectors of da (backward), each more than 8192 x 256 threads.
    Exact tier, fp32; torch's fp32 CPU result stands in for float64: the operands are exact (tests/test_pool_ref_host.py)."""
    G = P.PoolGrader(f"bilinear {path} stride")
    (n, h, w), ca, cb = P.BILINEAR_FWD_STRIDE if path == "forward" else P.BILINEAR_BWD_STRIDE
    rng = P.rng_of("bilinear stride", path)
    if path == "forward":
        a = P.integers(rng, (n, h, w, ca))
        want = F.interpolate(torch_nchw(a), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
        ab, ob = src(a), Buf(want.shape)
        bilinear_fwd(K, ab.t, None, ob.t, 0)
        G.exact("out", ob.host(), want)
        guards(G, "out", ob)
    else:
        dout = P.integers(rng, (n, 2 * h, 2 * w, ca))
        at = torch.zeros(n, ca, h, w, requires_grad=True)
        F.interpolate(at, scale_factor=2, mode="bilinear", align_corners=False).backward(torch_nchw(dout))
        want = at.grad.permute(0, 2, 3, 1).numpy()
        db, dab = src(dout), Buf((n, h, w, ca))
        K.upsample2x_bilinear_concat_bwd(db.t, dab.t, None, ca, 0)
        G.exact("da", dab.host(), want)
        guards(G, "da", dab)
    G.done()


# ---------------------------------------------------------------------------------------------------------------------- layout
def run_layout(K, G, shape, cpad, store):
    x = P.layout_input(shape)
    want = P.nchw_to_nhwc(x, cpad)
    want = bf16_round(want) if store == P.BF16 else want
    xb, yb = src(x), Buf(want.shape, DT[store])
    layout(K, xb.t, yb.t)
    what = f"{shape} cpad={cpad}"
    got = yb.host()
    G.exact(what + " y", got, want)
    G.note(what + " padding", not P.bits(got[..., shape[1]:]).any(), "channels c .. cpad - 1 are +0.0 bit for bit")
    guards(G, what, yb)


@pytest.mark.parametrize("store", STORES)
def test_nchw_to_nhwc(K, store):
    """c below, across and above one vector, padding of less than, exactly and more than one vector; bf16: round to nearest even."""
    G = P.PoolGrader(f"nchw_to_nhwc {store}")
    for c, cpad in P.LAYOUT_C[store]:
        for n, h, w in P.LAYOUT_NHW:
            run_layout(K, G, (n, c, h, w), cpad, store)
    run_layout(K, G, P.LAYOUT_STRIDE, P.VEC[store], store)            # 1025 x 1024 pixels over 4096 x 256 threads
    G.done()


@pytest.mark.parametrize("count", P.CAST_COUNTS)
def test_cast_to_bf16(K, count):
    """Halfway cases to the even neighbour, the carry into the next binade, +-0, +-inf, FLT_MAX -> inf, subnormals: what
    tensor.bfloat16() gives, bit for bit; one vector, four vectors per thread, and more vectors than 4096 x 256 x 4."""
    G = P.PoolGrader(f"cast_to_bf16 count={count}")
    chunks = [P.cast_specials()[i:i + 8] for i in range(0, P.cast_specials().size, 8)] if count == 8 else [P.cast_input(count)]
    for i, x in enumerate(chunks):
        xb, yb = src(x), Buf(x.shape, torch.bfloat16)
        K.cast_to_bf16(xb.t, out=yb.t)
        G.exact(f"chunk {i}", yb.host(), torch.from_numpy(x).bfloat16().float().numpy())
        guards(G, f"chunk {i}", yb)
    G.done()


# ------------------------------------------------------------------------------------------------------------ flat element-wise
def bits16(rng, count, lo=0.5, hi=2.0):
    """fp32 values of 16 significant bits, +-[lo, hi)."""
    x = (rng.uniform(lo, hi, count) * rng.choice([-1.0, 1.0], count)).astype(F32)
    return (x.view(np.uint32) & np.uint32(0xFFFFFF00)).view(F32)


@pytest.mark.parametrize("count", P.FLAT_COUNTS)
def test_fill_axpy_scale_add_i64(K, count):
    """Counts 1, 5, 1027 and 4096 x 256 x 4 + 5 (every thread of the capped grid takes a fifth item)."""
    G = P.PoolGrader(f"flat count={count}")
    rng = P.rng_of("flat", count)
    # fill
    for value in (0.1, -0.0):
        b = Buf(count)
        K.fill(b.t, value)
        G.exact(f"fill {value}", b.host(), np.full(count, value, dtype=F32))
        guards(G, f"fill {value}", b)
    # axpy: operands of 16 significant bits and like magnitude, so alpha * x is exact in float64 and so is y + alpha * x: its one
    # rounding to fp32 is the fused result, fl(y + fl(alpha * x)) the unfused one; the kernel may give either, element by element
    x, y = bits16(rng, count), bits16(rng, count)
    alpha = float(bits16(rng, 1, 0.25, 0.5)[0])
    r64 = y.astype(F64) + alpha * x.astype(F64)
    fused, unfused = r64.astype(F32), (y + (F32(alpha) * x).astype(F32)).astype(F32)
    assert (fused != unfused).any() or count < 1000
    yb = Buf(count, init=y)
    K.axpy(yb.t, src(x).t, alpha)
    got = yb.host()
    either = (P.bits(got) == P.bits(fused)) | (P.bits(got) == P.bits(unfused))
    ulp = np.spacing(np.maximum.reduce([np.abs(y), np.abs(F32(alpha) * x), np.abs(fused)])).astype(F64)
    worst = float((np.abs(got.astype(F64) - r64) / ulp).max())
    G.note("axpy", bool(either.all()) and worst <= 1.0, f"{int((~either).sum())} of {count} are neither the fused nor the unfused rounding; "
           f"{int((P.bits(got) == P.bits(fused)).sum())} fused, {int((fused != unfused).sum())} where the two differ; worst {worst:.3f} ulp of float64")
    guards(G, "axpy", yb)
    # scale: one rounding
    x = P.arbitrary(rng, count)
    alpha = float(F32(-0.7))
    want = (alpha * x.astype(F64)).astype(F32)
    ob = Buf(count)
    K.scale(src(x).t, alpha, out=ob.t)
    G.exact("scale", ob.host(), want)
    ab = Buf(count, init=x)
    K.scale(ab.t, alpha, out=ab.t)
    G.exact("scale in place", ab.host(), want)
    guards(G, "scale", ob, ab)
    # add_i64
    p = (2 ** 40 + rng.integers(-2 ** 20, 2 ** 20, count)).astype(np.int64)
    for v in (2 ** 40 + 3, -(2 ** 41) - 1):
        pb = Buf(count, torch.int64, init=p)
        K.check(K.ops.udaseg_add_i64(pb.t, count, v, None), "add_i64")
        G.equal(f"add_i64 {v}", pb.host(), p + v)
        guards(G, f"add_i64 {v}", pb)
    G.done()
