"""tests/_pool_ref.py is right, and tests/test_gpu_pool_grade.py can tell: runs anywhere.

* every restatement equals torch's float64 CPU result (max_pool2d with its indices turned into taps, interpolate + cat, autograd)
  at every small shape and data kind the GPU file runs, NaN, -inf and signed zeros included;
* the operands of the exact tier are exact: the fp32 leg in two summation orders equals float64 bit for bit;
* every mutant of the restatement fails the very check the named GPU case makes (and the restatement itself passes it);
* the launch-path cases cross the thresholds of the launch arithmetic they are named after, the small cases stay below.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pool_ref as P
from _norm_ref import bf16_round, normalised

F32, F64 = np.float32, np.float64
STORES = (P.FP32, P.BF16)
RTOL = 1e-12


def nchw(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64)).permute(0, 3, 1, 2).contiguous().requires_grad_(grad)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def close(got, ref, mag, what):
    e = normalised(np.asarray(got, dtype=F64) - np.asarray(ref, dtype=F64), mag).max(initial=0.0)
    assert e <= RTOL, f"{what}: {e:.3e} of the magnitude"


def torch_taps(idx, h, w):
    """max_pool2d's flat indices into the [h, w] plane -> ky * 3 + kx of the window that reported them."""
    idx = nhwc(idx)
    oy = np.arange(idx.shape[1])[None, :, None, None]
    ox = np.arange(idx.shape[2])[None, None, :, None]
    ky, kx = idx // w - (2 * oy - 1), idx % w - (2 * ox - 1)
    assert ((ky >= 0) & (ky < 3) & (kx >= 0) & (kx < 3)).all()
    return (ky * 3 + kx).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ torch agreement
@pytest.mark.parametrize("store", STORES)
def test_maxpool_is_torch_float64(store):
    seen = set()
    for shape, kind, tier in P.pool_cases(store):
        x = P.pool_input(shape, kind, tier, store)
        n, h, w, c = shape
        xt = nchw(x, True)
        yt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
        y, tap = P.maxpool(x)
        what = f"{store} {shape} {kind} {tier}"
        assert P.same_bits(y, nhwc(yt)), f"y {what}"
        assert np.array_equal(tap, torch_taps(it, h, w)), f"tap {what}"
        tap2, dy = P.pool_bwd_case(shape, kind, tier, store)
        assert np.array_equal(tap, tap2)
        yt.backward(nchw(dy))
        dx, mag = P.maxpool_bwd(dy, tap, shape)
        close(dx, nhwc(xt.grad), mag, f"dx {what}")
        assert not dx[mag == 0].any(), "an element no window chose has a gradient"
        # the data kinds hold what they promise
        if kind == "ties":
            seen.update(np.unique(P.bits(x)).tolist())
        if kind == "neg_inf":
            assert np.isneginf(y[:, 0, 0]).all() and np.isneginf(y[:, -1, -1]).all(), f"{what}: corner windows of -inf"
            assert (tap[:, 0, 0] == 4).all(), "window (0, 0) of -inf keeps its first valid tap, the centre"
        if kind == "nan":
            assert np.isnan(y[0, 0, 0]).all(), f"{what}: the NaN in the corner"
            if h * w > 1:
                assert np.isnan(x[0, :2, :2]).sum(axis=(0, 1)).min() >= 2, f"{what}: two NaNs in window (0, 0)"
                assert (tap[0, 0, 0, :c // 2] == (5 if w > 1 else 7)).all(), "the last NaN wins (lower channels: no other NaN)"
    assert seen == set(P.bits(np.array(P.TIES_ALPHABET, dtype=F32)).tolist()), "ties: -0.0 and +0.0 both present"


@pytest.mark.parametrize("store", STORES)
def test_the_exact_pool_cases_are_full_of_ties(store):
    """Nine taps over an alphabet of at most five values: every full window repeats a value, and in most of them the maximum
    itself is shared, so the first-maximum rule decides the tap."""
    for shape, kind, tier in P.pool_cases(store):
        n, h, w, c = shape
        if tier != "exact" or kind == "nan" or h < 5 or w < 5:
            continue
        x = P.pool_input(shape, kind, tier, store)
        y, _ = P.maxpool(x)
        shared = []
        for oy in range(1, (h - 2) // 2 + 1):                  # windows with all nine taps inside
            for ox in range(1, (w - 2) // 2 + 1):
                win = x[:, 2 * oy - 1:2 * oy + 2, 2 * ox - 1:2 * ox + 2].reshape(n, 9, c)
                assert (np.sort(win, axis=1)[:, 1:] == np.sort(win, axis=1)[:, :-1]).any(axis=1).all(), (shape, kind, oy, ox)
                shared.append(((win == y[:, oy, ox][:, None]).sum(axis=1) >= 2).mean())
        assert shared and np.mean(shared) > 0.5, (shape, kind, np.mean(shared))


@pytest.mark.parametrize("store", STORES)
def test_nearest_is_torch_float64(store):
    for a_shape, ca, cb, tier in P.up_cases(P.NEAREST_A, store):
        d = P.up_case("nearest", a_shape, ca, cb, tier, store)
        at, st = nchw(d["a"], True), (nchw(d["skip"], True) if cb else None)
        up = F.interpolate(at, scale_factor=2, mode="nearest")
        out = torch.cat([up, st], 1) if cb else up
        what = f"nearest {store} {a_shape} {ca}+{cb} {tier}"
        assert P.same_bits(P.upcat(d["a"], d["skip"]), nhwc(out)), what
        out.backward(nchw(d["dout"]))
        da, dskip, mag = P.upcat_bwd(d["dout"], ca)
        close(da, nhwc(at.grad), mag, "da " + what)
        if cb:
            assert P.same_bits(dskip, nhwc(st.grad)), "dskip " + what


@pytest.mark.parametrize("store", STORES)
def test_bilinear_is_torch_float64(store):
    for a_shape, ca, cb, tier in P.up_cases(P.BILINEAR_A, store):
        d = P.up_case("bilinear", a_shape, ca, cb, tier, store)
        at, st = nchw(d["a"], True), (nchw(d["skip"], True) if cb else None)
        up = F.interpolate(at, scale_factor=2, mode="bilinear", align_corners=False)
        out = torch.cat([up, st], 1) if cb else up
        what = f"bilinear {store} {a_shape} {ca}+{cb} {tier}"
        r, mag = P.bilinear_upcat(d["a"], d["skip"])
        close(r, nhwc(out), mag, what)
        out.backward(nchw(d["dout"]))
        da, dskip, mag = P.bilinear_upcat_bwd(d["dout"], ca)
        close(da, nhwc(at.grad), mag, "da " + what)
        if cb:
            assert P.same_bits(dskip, nhwc(st.grad)), "dskip " + what


def test_bilinear_matrix():
    assert np.array_equal(P.bilinear_matrix(1), [[1.0], [1.0]])
    assert np.array_equal(P.bilinear_matrix(3), [[1, 0, 0], [.75, .25, 0], [.25, .75, 0], [0, .75, .25], [0, .25, .75], [0, 0, 1]])
    for l in (1, 2, 5, 9):
        m = P.bilinear_matrix(l)
        x = torch.eye(l, dtype=torch.float64)[None]                      # [1, l (channels), l]: column k is the response to e_k
        ref = F.interpolate(x, scale_factor=2, mode="linear", align_corners=False)[0].T.numpy()
        assert np.array_equal(m, ref), l
        assert np.array_equal(m.sum(1), np.ones(2 * l))
    w = P.bilinear_weights((3, 5), 1, 4)
    assert w.shape == (6, 10) and w[0].sum() == 0 and w[1, 9] == 0.25 and w[2, 9] == 0.75 and w[2, 8] == 0.75 * 0.75


def test_nchw_to_nhwc_is_a_permute_and_a_pad():
    for store in STORES:
        for c, cpad in P.LAYOUT_C[store]:
            for n, h, w in P.LAYOUT_NHW:
                x = P.layout_input((n, c, h, w))
                ref = F.pad(torch.from_numpy(x).permute(0, 2, 3, 1), (0, cpad - c)).numpy()
                assert P.same_bits(P.nchw_to_nhwc(x, cpad), ref)
                assert len(np.unique(x)) > 0.99 * x.size and (bf16_round(x) != x).mean() > 0.9, "the pattern is not trivial"


def test_cast_vector_is_what_torch_rounds():
    s = P.cast_specials()
    assert len(s) % 8 == 0 and P.cast_input(8).size == 8
    t = torch.from_numpy(s).bfloat16().float().numpy()
    assert P.same_bits(bf16_round(s), t), "bf16_round and torch disagree on the special values"
    u = lambda v: int(P.bits(np.array([v], dtype=F32))[0])
    by = dict(zip(P.bits(s).tolist(), P.bits(t).tolist()))
    assert by[0x3F808000] == 0x3F800000 and by[0x3F818000] == 0x3F820000, "halfway: to the even neighbour, down and up"
    assert by[0x3FFFFFFF] == u(2.0) and by[0x7F7FFFFF] == u(np.inf) and by[0xFF7FFFFF] == u(-np.inf)
    assert by[0x80000000] == 0x80000000 and by[0x00008000] == 0 and by[0x00018000] == 0x00020000 and by[0x007FFFFF] == 0x00800000
    for count in P.CAST_COUNTS[:2]:
        x = P.cast_input(count)
        assert x.size == count and count % 8 == 0 and np.isfinite(x[len(s):]).all()
        assert P.same_bits(bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())


# ------------------------------------------------------------------------------------------- the exact tier's operands are exact
def same64(leg, ref):
    return np.array_equal(np.asarray(leg).astype(F64), ref) and np.asarray(leg).dtype == F32


@pytest.mark.parametrize("store", STORES)
def test_exact_tier_fp32_leg_is_float64_in_any_order(store):
    for shape, kind, tier in P.pool_cases(store):
        if tier == "exact":
            tap, dy = P.pool_bwd_case(shape, kind, tier, store)
            r64, _ = P.maxpool_bwd(dy, tap, shape)
            assert all(same64(P.maxpool_bwd(dy, tap, shape, F32, reverse=rev)[0], r64) for rev in (False, True)), (shape, kind)
            P.exact_want(r64, store == P.BF16)
    for a_shape, ca, cb, _ in P.up_cases(P.NEAREST_A, store, ("exact",)):
        d = P.up_case("nearest", a_shape, ca, cb, "exact", store)
        r64 = P.upcat_bwd(d["dout"], ca)[0]
        assert all(same64(P.upcat_bwd(d["dout"], ca, F32, reverse=rev)[0], r64) for rev in (False, True)), (a_shape, ca, cb)
    for a_shape, ca, cb, _ in P.up_cases(P.BILINEAR_A, store, ("exact",)):
        d = P.up_case("bilinear", a_shape, ca, cb, "exact", store)
        r64, mag = P.bilinear_upcat(d["a"], d["skip"])
        assert all(same64(P.bilinear_upcat(d["a"], d["skip"], F32, order=o)[0], r64) for o in ("hw", "wh")), (a_shape, ca, cb)
        assert np.array_equal(r64 * 16, np.round(r64 * 16)) and np.abs(r64).max() <= 128, "multiples of 1/16 within +-128"
        b64, _, bmag = P.bilinear_upcat_bwd(d["dout"], ca)
        assert all(same64(P.bilinear_upcat_bwd(d["dout"], ca, F32, order=o)[0], b64) for o in ("hw", "wh")), (a_shape, ca, cb)
        acc64, _ = P.accumulated(d["old_a"], b64, bmag)
        assert all(same64(P.accumulated(d["old_a"], P.bilinear_upcat_bwd(d["dout"], ca, F32, order=o)[0], bmag, F32)[0], acc64)
                   for o in ("hw", "wh"))
        if cb:
            s64 = P.accumulated(d["old_s"], d["dout"][..., ca:].astype(F64), 0)[0]
            assert same64(P.accumulated(d["old_s"], d["dout"][..., ca:], 0, F32)[0], s64)
        if store == P.BF16 and min(a_shape[1:]) > 1:          # and the bf16 store has something to round, up and down
            r32 = r64.astype(F32)
            assert (bf16_round(r32) != r32).mean() > 0.1 and (bf16_round(r32) != P.bf16_trunc(r32)).mean() > 0.05, a_shape


# -------------------------------------------------------------------------------------------------------------------- mutants
def verdict(check):
    """Run one of the GPU file's checks on a PoolGrader; True when it passes."""
    g = P.PoolGrader("host")
    check(g)
    return not g.bad


def pool_fwd_check(shape, kind, store, rule):
    x = P.pool_input(shape, kind, "exact", store)
    y, tap = P.maxpool(x)
    got_y, got_tap = P.maxpool(x, rule)
    return verdict(lambda g: (g.exact("y", got_y, y), g.equal("idx", got_tap, tap)))


@pytest.mark.parametrize("rule,kind,shape", [("pad0", "signed", (2, 6, 8, 4)), ("ge", "ties", (1, 1, 5, 4)),
                                             ("nan_ignored", "nan", (1, 1, 5, 4)), ("init0", "neg_inf", (1, 1, 1, 4))])
def test_pool_forward_mutants_fail_the_named_case(rule, kind, shape):
    """pad0: test_maxpool_forward[f32-signed] (a window of negatives reports 0 and the padding's tap); ge: [f32-ties] (the last of
    equal maxima); nan_ignored: [f32-nan] (the NaN does not win); init0: [f32-neg_inf] (window (0, 0) of -inf reports tap 0)."""
    assert pool_fwd_check(shape, kind, P.FP32, None)
    assert not pool_fwd_check(shape, kind, P.FP32, rule)
    caught = [s for s, k, t in P.pool_cases(P.FP32) if k == kind and t == "exact" and not pool_fwd_check(s, kind, P.FP32, rule)]
    assert len(caught) >= 3, caught


def test_pool_backward_one_row_short_fails_the_row_loop_case():
    """test_maxpool_launch_paths[row-loop]: rows 65535 and 65536 of dx keep the NaN the buffer was filled with."""
    shape = P.POOL_ROW_LOOP
    tap, dy = P.pool_bwd_case(shape, "signed", "exact", P.FP32)
    r64, mag = P.maxpool_bwd(dy, tap, shape)
    r32, _ = P.maxpool_bwd(dy, tap, shape, F32)
    short, _ = P.maxpool_bwd(dy, tap, shape, F32, rows=P.grid_rows(shape[0], shape[1]))
    assert verdict(lambda g: g.tier("dx", "exact", r32, r64, r32, mag))
    assert not verdict(lambda g: g.tier("dx", "exact", short, r64, r32, mag))
    small = (2, 6, 8, 4)                                       # and no small case could have seen it
    assert P.grid_rows(small[0], small[1]) == small[0] * small[1]


BIL = ((1, 3, 5), 4, 0)


@pytest.mark.parametrize("mutant", ["swapped", "first_unclamped", "last_unclamped"])
def test_bilinear_forward_mutants_fail_the_exact_tier(mutant):
    """test_bilinear_forward[f32]: case (1, 3, 5) 4+0 of the exact tier."""
    a_shape, ca, cb = BIL
    d = P.up_case("bilinear", a_shape, ca, cb, "exact", P.FP32)
    r64, mag = P.bilinear_upcat(d["a"], d["skip"])
    r32, _ = P.bilinear_upcat(d["a"], d["skip"], F32)
    bad, _ = P.bilinear_upcat(d["a"], d["skip"], F32, mutant=mutant)
    assert verdict(lambda g: g.tier("out", "exact", r32, r64, r32, mag))
    assert not verdict(lambda g: g.tier("out", "exact", bad, r64, r32, mag))
    # the arbitrary tier's bar sees them too
    d = P.up_case("bilinear", a_shape, ca, cb, "arbitrary", P.FP32)
    r64, mag = P.bilinear_upcat(d["a"], d["skip"])
    r32, _ = P.bilinear_upcat(d["a"], d["skip"], F32)
    bad, _ = P.bilinear_upcat(d["a"], d["skip"], F32, mutant=mutant)
    assert not verdict(lambda g: g.tier("out", "arbitrary", bad, r64, r32, mag))


def test_bilinear_backward_one_column_off_fails_the_exact_tier():
    """test_bilinear_backward[f32]: case (1, 3, 5) 4+0, plain da."""
    a_shape, ca, cb = BIL
    d = P.up_case("bilinear", a_shape, ca, cb, "exact", P.FP32)
    r64, _, mag = P.bilinear_upcat_bwd(d["dout"], ca)
    r32 = P.bilinear_upcat_bwd(d["dout"], ca, F32)[0]
    bad = P.bilinear_upcat_bwd(d["dout"], ca, F32, shift=1)[0]
    assert verdict(lambda g: g.tier("da", "exact", r32, r64, r32, mag))
    assert not verdict(lambda g: g.tier("da", "exact", bad, r64, r32, mag))


def test_truncating_bf16_store_fails_the_exact_tier_and_passes_a_norm_wise_bar():
    """test_bilinear_forward[bf16]: case (1, 3, 5) 8+0 of the exact tier.  The norm-wise 2^-7 of the older bilinear test lets the
    same output through."""
    d = P.up_case("bilinear", (1, 3, 5), 8, 0, "exact", P.BF16)
    r64, mag = P.bilinear_upcat(d["a"], None)
    r32, _ = P.bilinear_upcat(d["a"], None, F32)
    bad = P.bf16_trunc(r32)
    assert verdict(lambda g: g.tier("out", "exact", bf16_round(r32), r64, r32, mag, True))
    assert not verdict(lambda g: g.tier("out", "exact", bad, r64, r32, mag, True))
    assert np.abs(bad - r64).max() / np.abs(r64).max() < 2.0 ** -7


def test_nearest_backward_three_of_four_fails_the_exact_tier():
    """test_nearest_backward[f32]: case (2, 5, 6) 4+0 of the exact tier."""
    d = P.up_case("nearest", (2, 5, 6), 4, 0, "exact", P.FP32)
    r64, _, mag = P.upcat_bwd(d["dout"], 4)
    r32 = P.upcat_bwd(d["dout"], 4, F32)[0]
    bad = P.upcat_bwd(d["dout"], 4, F32, dependants=3)[0]
    assert verdict(lambda g: g.tier("da", "exact", r32, r64, r32, mag))
    assert not verdict(lambda g: g.tier("da", "exact", bad, r64, r32, mag))


def test_unwritten_padding_fails_the_layout_case():
    """test_nchw_to_nhwc[f32]: (c, cpad) = (3, 8), whose channels 4 .. 7 are a whole vector of padding."""
    x = P.layout_input((1, 3, 10, 14))
    want = P.nchw_to_nhwc(x, 8)
    assert P.bits(want[..., 3:]).max() == 0, "padding is +0.0"
    assert verdict(lambda g: g.exact("y", P.nchw_to_nhwc(x, 8), want))
    assert not verdict(lambda g: g.exact("y", P.nchw_to_nhwc(x, 8, pad=P.NAN), want))
    assert not verdict(lambda g: g.exact("y", P.nchw_to_nhwc(x, 8, pad=-0.0), want))


# ------------------------------------------------------------------------------------------------------------ launch arithmetic
def test_launch_arithmetic():
    assert P.grid_for(1) == 1 and P.grid_for(513) == 2 and P.grid_for(257, 1) == 2 and P.grid_for(10 ** 9) == 4096
    assert P.grid_for(4096 * 256, 1) == 4096 and not P.strides(4096 * 256, P.grid_for(4096 * 256, 1))
    assert P.grid_items(257) == 2 and P.grid_items(10 ** 9) == 8192 and P.grid_items(8192 * 256) == 8192
    assert P.grid_rows(1, 65535) == 65535 and P.grid_rows(2, 40000) == 65535 and P.grid_rows(3, 7) == 21


def crosses(kernel, store, shape, ca=0, cb=0):
    items, blocks = P.launch_items(kernel, store, shape, ca, cb)
    return P.strides(items, blocks)


def test_launch_path_cases_cross_their_thresholds():
    n, h, w, c = P.POOL_ROW_LOOP
    assert n * h > P.grid_rows(n, h) == 65535 and w * (c // 4) <= 256
    (n, h, w), ca, cb = P.NEAREST_ROW_LOOP
    assert n * h > P.grid_rows(n, h) == 65535
    for store in STORES:
        assert crosses("maxpool_fwd", store, P.POOL_STRIDE[store]) and P.launch_items("maxpool_fwd", store, P.POOL_STRIDE[store])[1] == 4096
        assert crosses("nchw_to_nhwc", store, (P.LAYOUT_STRIDE[0],) + P.LAYOUT_STRIDE[2:])
    assert crosses("maxpool_bwd_bf16", P.BF16, P.POOL_STRIDE[P.BF16])
    a, ca, cb = P.NEAREST_FWD_CAP
    items, blocks = P.launch_items("upcat_fwd", P.FP32, a, ca, cb)
    assert blocks == 4096 and items > 4096 * 512, "past the cap of the 2-per-thread launch"
    a, ca, cb = P.NEAREST_BF16_STRIDE
    assert crosses("upcat_bwd_a_bf16", P.BF16, a, ca, cb)
    a, ca, cb = P.BILINEAR_FWD_STRIDE
    assert crosses("bilinear_fwd", P.FP32, a, ca, cb) and P.launch_items("bilinear_fwd", P.FP32, a, ca, cb)[1] == 8192
    a, ca, cb = P.BILINEAR_BWD_STRIDE
    assert crosses("bilinear_bwd_a", P.FP32, a, ca, cb) and P.launch_items("bilinear_bwd_a", P.FP32, a, ca, cb)[1] == 8192
    assert P.FLAT_COUNTS[-1] > 4096 * 256 * 4 and P.strides(-(-P.FLAT_COUNTS[-1] // 4), P.grid_for(P.FLAT_COUNTS[-1], 4))
    assert all(cnt % 8 == 0 for cnt in P.CAST_COUNTS) and P.CAST_COUNTS[0] == 8
    assert P.grid_for8(P.CAST_COUNTS[1] // 8, 4) == 4 and P.strides(P.CAST_COUNTS[1] // 8, 4)      # under the cap, 4 per thread
    assert P.grid_for8(P.CAST_COUNTS[2] // 8, 4) == 4096 and P.CAST_COUNTS[2] // 8 > 4096 * 256 * 4   # past the cap


def test_small_cases_stay_below_the_thresholds():
    for store in STORES:
        for shape, _, _ in P.pool_cases(store):
            assert not crosses("maxpool_fwd", store, shape) and P.grid_rows(shape[0], shape[1]) == shape[0] * shape[1]
            assert not crosses("maxpool_bwd_bf16", P.BF16, shape[:3] + (64,))
        for shapes, fwd, bwd_a, bwd_s in ((P.NEAREST_A, "upcat_fwd", "upcat_bwd_a_bf16", "upcat_bwd_skip"),
                                          (P.BILINEAR_A, "bilinear_fwd", "bilinear_bwd_a", "bilinear_bwd_skip")):
            for a_shape, ca, cb, _ in P.up_cases(shapes, store, ("exact",)):
                items, blocks = P.launch_items(fwd, store, a_shape, ca, cb)
                assert blocks < (4096 if fwd == "upcat_fwd" else 8192)
                assert not crosses(bwd_a, store, a_shape, ca, cb) and P.grid_rows(a_shape[0], a_shape[1]) < 65535
                assert P.launch_items(bwd_s, store, a_shape, ca, cb)[1] < 4096
        for n, h, w in P.LAYOUT_NHW:
            assert not crosses("nchw_to_nhwc", store, (n, h, w))
    assert all(P.grid_for(cnt, 4) < 4096 for cnt in P.FLAT_COUNTS[:-1])
