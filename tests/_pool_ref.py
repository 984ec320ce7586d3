"""numpy restatement of the glue between the convolutions, NHWC: max_pool2d(3, 2, 1) with its stored tap bytes and its backward,
nearest and bilinear x2 up-sampling + concat with their backward, the NCHW -> NHWC layout pass (csrc/pool_resize.hip in both storages,
csrc/bilinear.hip; the bf16 cast: csrc/elem_bf16.hip), the launch arithmetic of those files, the cases tests/test_gpu_pool_grade.py runs and the
mutants tests/test_pool_ref_host.py shows those cases to reject.

Test infrastructure in the manner of ``_norm_ref``: sums are written once, generically over the float type ``elem`` -- ``np.float64``
is the reference, ``np.float32`` the same arithmetic in the kernels' precision (the leg the bar is measured from) -- and come with
the MAGNITUDE of every output element (the same operation on the absolute values).  Selections and copies have no ``elem``: they return
the operand's own values.  bf16 rounding is ``_norm_ref.bf16_round``.

A mutant is a keyword of the restatement that makes it wrong in one named way; the default of every keyword is the right thing.
"""
import numpy as np

from _grade import Grader, log
from _norm_ref import F32, F64, bf16_round

NAN, INF = float("nan"), float("inf")
FP32, BF16 = "f32", "bf16"
VEC = {FP32: 4, BF16: 8}                     # channels per 16-byte vector


def out_len(l):
    """Output extent of a 3-wide, stride-2, pad-1 window along an axis of length l."""
    return (l - 1) // 2 + 1


# ------------------------------------------------------------------------------------------------------------------ max pool
POOL_RULES = (None, "pad0", "ge", "nan_ignored", "init0")


def maxpool(x, rule=None):
    """(y, tap) of max_pool2d(kernel 3, stride 2, pad 1) on x [n, h, w, c]; tap = ky * 3 + kx (uint8) of the winner.

    The window is scanned row-major.  Padding never takes part; the first VALID tap is the initial winner whatever it holds, a
    later tap replaces it when it is greater or NaN -- so the first of equal maxima wins (+0 and -0 are equal), a window of -inf
    keeps its first valid tap, and once a NaN has won only another NaN replaces it (the last NaN wins).
    Mutants: "pad0" padding takes part as 0; "ge" >= instead of > (the last maximum wins); "nan_ignored" no NaN clause;
    "init0" the winner starts as (-inf, tap 0) instead of the first valid tap."""
    assert rule in POOL_RULES
    x = np.asarray(x)
    n, h, w, c = x.shape
    ho, wo = out_len(h), out_len(w)
    padded = np.zeros((n, 2 * ho + 1, 2 * wo + 1, c), dtype=x.dtype)
    valid = np.zeros((2 * ho + 1, 2 * wo + 1), dtype=bool)
    padded[:, 1:h + 1, 1:w + 1] = x
    valid[1:h + 1, 1:w + 1] = True
    if rule == "pad0":
        valid[:] = True
    best = np.full((n, ho, wo, c), -INF, dtype=x.dtype)
    tap = np.zeros((n, ho, wo, c), dtype=np.uint8)
    started = np.full((1, ho, wo, 1), rule == "init0")
    with np.errstate(invalid="ignore"):
        for t in range(9):
            ky, kx = divmod(t, 3)
            v = padded[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2]
            ok = valid[ky:ky + 2 * ho:2, kx:kx + 2 * wo:2][None, :, :, None]
            wins = (v >= best) if rule == "ge" else (v > best)
            if rule != "nan_ignored":
                wins = wins | np.isnan(v)
            upd = ok & (wins | ~started)
            best = np.where(upd, v, best)
            tap = np.where(upd, np.uint8(t), tap)
            started = started | ok
    return best, tap


def _tap_slices(t, h, w):
    """For tap t: the windows (oy, ox ranges) whose tap t is a real element, and the strided slices of those elements."""
    ky, kx = divmod(t, 3)
    out = []
    for k, l in ((ky, h), (kx, w)):
        o0, o1 = (1 if k == 0 else 0), min(out_len(l), (l - k) // 2 + 1)
        if o1 <= o0:
            return None
        i0 = 2 * o0 - 1 + k
        out.append((slice(o0, o1), slice(i0, 2 * (o1 - 1) + k, 2)))
    return out


def maxpool_bwd(dy, tap, shape, elem=F64, reverse=False, rows=None):
    """(dx, magnitude): every window's gradient lands on the element its tap names; the magnitude is the sum of |dy| over the
    windows that chose the element.  The <= 4 terms of an element are added in tap order (``reverse``: in the opposite order).
    Mutant: ``rows`` = number of image rows (of n * h) written, the rest left NaN."""
    n, h, w, c = shape
    dy, tap = np.asarray(dy), np.asarray(tap)
    dx, mag = np.zeros(shape, dtype=elem), np.zeros(shape, dtype=F64)
    for t in (range(8, -1, -1) if reverse else range(9)):
        s = _tap_slices(t, h, w)
        if s is None:
            continue
        (oy, iy), (ox, ix) = s
        sel = tap[:, oy, ox] == t
        g = dy[:, oy, ox]
        dx[:, iy, ix] = (dx[:, iy, ix] + np.where(sel, g.astype(elem), elem(0))).astype(elem)
        mag[:, iy, ix] += np.where(sel, np.abs(g.astype(F64)), 0.0)
    if rows is not None:
        dx.reshape(n * h, -1)[rows:] = NAN
    return dx, mag


# ------------------------------------------------------------------------------------------------- nearest up-sampling + concat
def upcat(a, skip):
    """cat(interpolate(a, scale_factor=2, mode="nearest"), skip) along the channels; skip None: no skip channels."""
    up = np.asarray(a).repeat(2, axis=1).repeat(2, axis=2)
    return up if skip is None else np.concatenate([up, np.asarray(skip)], axis=-1)


def upcat_bwd(dout, ca, elem=F64, reverse=False, dependants=4):
    """(da, dskip, magnitude of da): da sums the 2 x 2 outputs that copied the element (in row-major order, ``reverse``: the
    opposite), dskip is the skip channels of dout themselves.  Mutant: ``dependants`` < 4 leaves the last ones out."""
    dout = np.asarray(dout)
    d = dout[..., :ca]
    parts = [d[:, 0::2, 0::2], d[:, 0::2, 1::2], d[:, 1::2, 0::2], d[:, 1::2, 1::2]][:dependants]
    da, mag = np.zeros(parts[0].shape, dtype=elem), np.zeros(parts[0].shape, dtype=F64)
    for p in (parts[::-1] if reverse else parts):
        da = (da + p.astype(elem)).astype(elem)
        mag += np.abs(p.astype(F64))
    return da, dout[..., ca:].copy(), mag


# ------------------------------------------------------------------------------------------------ bilinear up-sampling + concat
BILINEAR_MUTANTS = (None, "swapped", "first_unclamped", "last_unclamped")


def bilinear_matrix(l, mutant=None):
    """The dense [2l, l] matrix of interpolate(scale_factor=2, mode="bilinear", align_corners=False) along one axis:
    out[2k] = 0.25 in[max(k - 1, 0)] + 0.75 in[k], out[2k + 1] = 0.75 in[k] + 0.25 in[min(k + 1, l - 1)]; l = 1: [[1], [1]].
    Mutants: "swapped" 0.25 and 0.75 exchanged; "first_unclamped" row 0 is 0.75 in[0] + 0.25 x (a zero outside);
    "last_unclamped" the same for the last row."""
    assert mutant in BILINEAR_MUTANTS
    near, far = (0.25, 0.75) if mutant == "swapped" else (0.75, 0.25)
    m = np.zeros((2 * l, l), dtype=F64)
    for k in range(l):
        m[2 * k, k] += near
        m[2 * k + 1, k] += near
        if k > 0 or mutant != "first_unclamped":
            m[2 * k, max(k - 1, 0)] += far
        if k < l - 1 or mutant != "last_unclamped":
            m[2 * k + 1, min(k + 1, l - 1)] += far
    return m


def _two_axes(t, mh, mw, dt, order):
    """t [n, h, w, c] -> [n, H, W, c] with mh [H, h] on axis 1 and mw [W, w] on axis 2, in ``dt``; order "hw": rows first."""
    t, mh, mw = np.asarray(t).astype(dt), mh.astype(dt), mw.astype(dt)
    for axis in order:
        if axis == "h":
            n, h, w, c = t.shape
            t = np.matmul(mh, t.reshape(n, h, w * c)).reshape(n, mh.shape[0], w, c)
        else:
            t = np.matmul(mw, t)
    return t.astype(dt)


def bilinear_upcat(a, skip, elem=F64, order="hw", mutant=None):
    """(out, magnitude) of cat(interpolate(a, scale_factor=2, mode="bilinear", align_corners=False), skip), built from
    bilinear_matrix; the magnitude is the same operation on the absolute values (|skip| for the copied channels)."""
    a = np.asarray(a)
    mh, mw = bilinear_matrix(a.shape[1], mutant), bilinear_matrix(a.shape[2], mutant)
    up, mag = _two_axes(a, mh, mw, elem, order), _two_axes(np.abs(a), np.abs(mh), np.abs(mw), F64, order)
    if skip is None:
        return up, mag
    skip = np.asarray(skip)
    return np.concatenate([up, skip.astype(elem)], axis=-1), np.concatenate([mag, np.abs(skip.astype(F64))], axis=-1)


def bilinear_upcat_bwd(dout, ca, elem=F64, order="hw", shift=0):
    """(da, dskip, magnitude of da): da is the transposed matrices applied to the first ca channels of dout, dskip the other
    channels themselves.  Mutant: ``shift`` columns off (the gradient rolled along the width before it is gathered)."""
    dout = np.asarray(dout)
    d = dout[..., :ca]
    if shift:
        d = np.roll(d, shift, axis=2)
    mh, mw = bilinear_matrix(d.shape[1] // 2).T, bilinear_matrix(d.shape[2] // 2).T
    return _two_axes(d, mh, mw, elem, order), dout[..., ca:].copy(), _two_axes(np.abs(d), mh, mw, F64, order)


def accumulated(old, value, mag, elem=F64):
    """(old + value, |old| + magnitude): what an accumulating backward leaves in a buffer that held ``old``."""
    return (np.asarray(old).astype(elem) + value).astype(elem), np.abs(np.asarray(old, dtype=F64)) + mag


def bilinear_weights(shape, py, px):
    """[2h, 2w] weights with which pixel (py, px) of an [h, w] image enters the up-sampled outputs -- and, read the other way,
    with which the gradient of up-sampled pixel (Y, X) enters da[py, px]."""
    return np.outer(bilinear_matrix(shape[0])[:, py], bilinear_matrix(shape[1])[:, px])


# ---------------------------------------------------------------------------------------------------------------------- layout
def nchw_to_nhwc(x, cpad, pad=0.0):
    """[n, c, h, w] -> [n, h, w, cpad], channels c .. cpad - 1 exactly +0.0.  Mutant: ``pad`` = NaN, what an unwritten channel of
    the graded buffer holds."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    out = np.full((n, h, w, cpad), pad, dtype=x.dtype)
    out[..., :c] = x.transpose(0, 2, 3, 1)
    return out


def bf16_trunc(x):
    """Mutant of ``bf16_round``: the low 16 bits dropped."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(F32).reshape(np.shape(x))


# ------------------------------------------------------------------------------------------------------------ launch arithmetic
CAP, CAP_ITEMS, ROWS_CAP, BLOCK = 4096, 8192, 65535, 256


def grid_for(items, per_thread=2):
    """Blocks of csrc/common.h grid_for, which both storages launch with (grid_for8: the name the bf16 cases use here)."""
    return max(min((items + BLOCK * per_thread - 1) // (BLOCK * per_thread), CAP), 1)


grid_for8 = grid_for


def grid_items(items):
    """Blocks of csrc/bilinear.hip grid_items."""
    return max(min((items + BLOCK - 1) // BLOCK, CAP_ITEMS), 1)


def grid_rows(n, h):
    """gridDim.y of maxpool_bwd_kernel and upcat_bwd_a_kernel: one image row per step of the row loop."""
    return min(n * h, ROWS_CAP)


def strides(items, blocks):
    """A thread of a grid-stride loop takes a second item: more items than threads."""
    return items > blocks * BLOCK


def launch_items(kernel, store, shape, ca=0, cb=0):
    """(items, blocks) of the flat launches graded below; shape: the pooled tensor x, or the low-resolution a of an up-sampling."""
    n, h, w = shape[:3]
    v = VEC[store]
    if kernel == "maxpool_fwd":
        items = n * out_len(h) * out_len(w) * (shape[3] // v)
        return items, grid_for(items, 1)
    if kernel == "maxpool_bwd_bf16":
        items = n * h * w * (shape[3] // v)
        return items, grid_for(items, 1)
    if kernel == "upcat_fwd":                        # bf16 moves as half as many fp32 channels: 16-byte vectors either way
        items = 4 * n * h * w * ((ca + cb) // v)
        return items, grid_for(items)
    if kernel == "upcat_bwd_a_bf16":
        items = n * h * w * (ca // v)
        return items, grid_for(items, 1)
    if kernel == "upcat_bwd_skip":
        items = 4 * n * h * w * (cb // v)
        return items, grid_for(items)
    if kernel == "bilinear_fwd":
        items = 4 * n * h * w * ((ca + cb) // v)
        return items, grid_items(items)
    if kernel == "bilinear_bwd_a":
        items = n * h * w * (ca // v)
        return items, grid_items(items)
    if kernel == "bilinear_bwd_skip":
        items = 4 * n * h * w * (cb // v)
        return items, grid_items(items)
    if kernel == "nchw_to_nhwc":
        items = n * h * w
        return items, grid_for(items, 1)
    raise KeyError(kernel)


# ------------------------------------------------------------------------------------------------------------------- the cases
POOL_HW = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 2, 2), (1, 3, 4), (1, 7, 9), (2, 6, 8)]           # (n, h, w)
POOL_C = {FP32: (4, 12, 64), BF16: (8, 24, 64)}
POOL_KINDS = ("signed", "ties", "neg_inf", "nan")
POOL_ROW_LOOP = (1, 65537, 3, 8)                                       # fp32 backward: n * h > 65535
POOL_STRIDE = {FP32: (1, 514, 514, 64), BF16: (1, 514, 514, 128)}      # forward (and the bf16 backward): > 4096 x 256 vectors
NEAREST_A = [(1, 1, 1), (2, 1, 7), (1, 9, 2), (2, 5, 6)]
BILINEAR_A = [(1, 1, 1), (2, 1, 7), (1, 9, 1), (1, 2, 2), (1, 3, 5), (2, 5, 6)]
CA_CB = {FP32: ((4, 0), (12, 4), (32, 16)), BF16: ((8, 0), (24, 8), (32, 16))}
NEAREST_ROW_LOOP = ((1, 65537, 1), 4, 4)                               # fp32 da: (a's n, h, w), ca, cb
NEAREST_FWD_CAP = ((1, 182, 182), 32, 32)                              # fp32 forward: > 4096 x 512 vectors
NEAREST_BF16_STRIDE = ((1, 363, 363), 64, 0)                           # bf16 da: > 4096 x 256 vectors
BILINEAR_FWD_STRIDE = ((1, 363, 363), 16, 0)                           # fp32 forward: > 8192 x 256 vectors
BILINEAR_BWD_STRIDE = ((1, 363, 363), 64, 0)                           # fp32 backward
LAYOUT_C = {FP32: ((3, 4), (3, 8), (1, 4), (5, 12), (23, 24)), BF16: ((3, 8), (3, 16), (9, 16), (23, 24))}      # (c, cpad)
LAYOUT_NHW = [(n, h, w) for n in (1, 3) for h, w in ((1, 1), (1, 7), (10, 14))]
LAYOUT_STRIDE = (1, 3, 1025, 1024)                                     # NCHW: n * h * w > 4096 x 256
FLAT_COUNTS = (1, 5, 1027, CAP * BLOCK * 4 + 5)                        # fill / axpy / scale / add_i64: 4 items per thread
CAST_COUNTS = (8, 8 * (3 * BLOCK * 4 + 1), 8 * (CAP * BLOCK * 4 + 3))  # one vector; every thread of 4 blocks strides; past the cap
POOL_ALPHABET = (-128.0, -3.0, -1.0, 2.0, 128.0)                       # five values over <= 9 taps: ties in every full window
TIES_ALPHABET = (-1.0, -0.0, 0.0, 1.0)


def _seed(*key):
    """A seed from the case's own description, the same in every process."""
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def rng_of(*key):
    return np.random.default_rng(_seed(*key))


def integers(rng, shape):
    """The exact tier's operands: integers in [-128, 128], bf16-representable."""
    return rng.integers(-128, 129, size=shape).astype(F32)


def arbitrary(rng, shape, store=FP32):
    """The arbitrary tier's operands: randn * 2 ** randint(-6, 6), rounded to the storage type."""
    x = (rng.standard_normal(shape) * np.exp2(rng.integers(-6, 6, size=shape))).astype(F32)
    return bf16_round(x) if store == BF16 else x


def operands(rng, shape, tier, store=FP32):
    return integers(rng, shape) if tier == "exact" else arbitrary(rng, shape, store)


def pool_input(shape, kind, tier="exact", store=FP32):
    """The pooled tensor of one case (fp32 array of the stored values).

    signed   exact: the five-value alphabet, no zero (padding counted as 0 would win over a negative window); arbitrary: randn.
    ties     {-1, -0.0, +0.0, 1}: the first of equal maxima, and -0 against +0.
    neg_inf  the corner windows (0, 0) and (last, last) and, where it exists, the interior window (1, 1) are -inf throughout,
             and a third of the lower half of the channels besides.
    nan      NaN in the corner element and in its neighbour (two NaNs in window (0, 0)), and a sixth of the upper half of the
             channels besides."""
    n, h, w, c = shape
    rng = rng_of("pool", shape, kind, tier, store)
    if kind == "signed" and tier == "arbitrary":
        return arbitrary(rng, shape, store)
    assert tier == "exact"
    if kind == "ties":
        return rng.choice(np.array(TIES_ALPHABET, dtype=F32), size=shape)
    x = rng.choice(np.array(POOL_ALPHABET, dtype=F32), size=shape)
    if kind == "neg_inf":
        x[..., :c // 2][rng.random((n, h, w, c // 2)) < 1 / 3] = -INF
        x[:, :2, :2] = -INF
        x[:, max(2 * out_len(h) - 3, 0):, max(2 * out_len(w) - 3, 0):] = -INF
        if h >= 4 and w >= 4:
            x[:, 1:4, 1:4] = -INF
    elif kind == "nan":
        x[..., c // 2:][rng.random((n, h, w, c - c // 2)) < 1 / 6] = NAN
        x[0, 0, 0] = NAN
        if w > 1:
            x[0, 0, 1] = NAN
        elif h > 1:
            x[0, 1, 0] = NAN
    return x


def pool_cases(store):
    """(shape, kind, tier) of every small max-pool case."""
    for n, h, w in POOL_HW:
        for c in POOL_C[store]:
            for kind in POOL_KINDS:
                yield (n, h, w, c), kind, "exact"
            yield (n, h, w, c), "signed", "arbitrary"


def pool_bwd_case(shape, kind, tier, store):
    """(tap, dy) of one max-pool backward case: the taps of the forward case of the same name, a gradient of the tier's kind."""
    _, tap = maxpool(pool_input(shape, kind, tier, store))
    return tap, operands(rng_of("pool dy", shape, kind, tier, store), tap.shape, tier, store)


def up_case(mode, a_shape, ca, cb, tier, store):
    """Operands of one up-sampling case (mode "nearest" / "bilinear"): a, skip (None when cb == 0), the gradient dout of the
    output, and what the accumulating backward finds in da and dskip."""
    n, h, w = a_shape
    rng = rng_of(mode, a_shape, ca, cb, tier, store)
    d = {"a": operands(rng, (n, h, w, ca), tier, store), "dout": operands(rng, (n, 2 * h, 2 * w, ca + cb), tier, store),
         "old_a": operands(rng, (n, h, w, ca), tier, store), "skip": None, "old_s": None}
    if cb:
        d["skip"], d["old_s"] = (operands(rng, (n, 2 * h, 2 * w, cb), tier, store) for _ in range(2))
    return d


def up_cases(shapes, store, tiers=("exact", "arbitrary")):
    for a_shape in shapes:
        for ca, cb in CA_CB[store]:
            for tier in tiers:
                yield a_shape, ca, cb, tier


def layout_input(shape):
    """A non-trivial fp32 pattern for nchw_to_nhwc [n, c, h, w]: hardly two elements alike, hardly one bf16-representable."""
    x = arbitrary(rng_of("layout", shape), shape)
    return (x + np.arange(x.size, dtype=F32).reshape(shape) * F32(2.0 ** -9)).astype(F32)


def cast_specials():
    """fp32 bit patterns the bf16 cast must round to nearest even: halfway cases with an even and an odd lower neighbour, the
    largest value below a power of two (rounds up into the next binade), +-0, +-inf, the largest finite fp32 (rounds to inf),
    subnormals (a halfway case, the smallest, the largest -- which rounds up to the smallest normal), each with both signs."""
    pos = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x3FFFFFFF, 0x00000000, 0x7F800000, 0x7F7FFFFF, 0x7F7F7FFF,
           0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x007F8000, 0x42FF8000, 0x477FE000, 0x3F800000]
    u = np.array(pos + [p | 0x80000000 for p in pos], dtype=np.uint32)
    return np.concatenate([u, u[:(-len(u)) % 8]]).view(F32)


def cast_input(count):
    """``count`` fp32 values: the specials first (count 8: their first vector), then random bit patterns of finite values."""
    s = cast_specials()
    if count <= len(s):
        return s[:count].copy()
    rng = rng_of("cast", count)
    u = rng.integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)          # no inf / NaN among the random ones
    u[:len(s)] = s.view(np.uint32)
    return u.view(F32)


# ------------------------------------------------------------------------------------------------------------------ the checks
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(got, want):
    """fp32 arrays equal bit for bit (so +0 and -0 differ), NaN at the same positions (a NaN's payload is not compared)."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    if got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(ng, nw) and np.array_equal(bits(got)[~ng], bits(want)[~nw]))


def exact_want(r64, bf16_out=False):
    """The exact tier's expectation: the float64 value, which fp32 must hold exactly, rounded once to bf16 where the store is."""
    r32 = np.asarray(r64).astype(F32)
    assert np.array_equal(r32.astype(F64), np.asarray(r64, dtype=F64), equal_nan=True), "exact tier: float64 value is not an fp32 number"
    return bf16_round(r32) if bf16_out else r32


class PoolGrader(Grader):
    """Grader with the bit-for-bit verdicts of selections, copies and the exact tier next to the bar of the sums."""
    PREFIX = "pool-grade"

    def exact(self, what, got, want):
        ok = same_bits(got, want)
        got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
        differ = -1 if got.shape != want.shape else int((~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))).sum())
        log(f"{self.PREFIX} {self.tag} {what}: {'bit for bit' if ok else f'DIFFERS in {differ} of {want.size}'}")
        if not ok:
            self.bad.append(f"{what}: {differ} of {want.size} elements differ in their bits")

    def equal(self, what, got, want):
        """Integer arrays (tap bytes, counters) equal."""
        got, want = np.asarray(got), np.asarray(want)
        differ = int((got != want).sum()) if got.shape == want.shape else -1
        log(f"{self.PREFIX} {self.tag} {what}: {'equal' if differ == 0 else f'DIFFERS in {differ} of {want.size}'}")
        if differ:
            self.bad.append(f"{what}: {differ} of {want.size} differ")

    def tier(self, what, tier, got, r64, r32, mag, bf16_out=False):
        """Exact tier: float64 rounded once, bit for bit.  Arbitrary tier: the bar."""
        if tier == "exact":
            self.exact(what, got, exact_want(r64, bf16_out))
        else:
            self.grade(what, got, r64, r32, mag, bf16_out)

    def note(self, what, ok, text, quiet=False):
        """A yes / no verdict; ``quiet``: logged only when it fails."""
        if not (ok and quiet):
            log(f"{self.PREFIX} {self.tag} {what}: {text}")
        if not ok:
            self.bad.append(f"{what}: {text}")
