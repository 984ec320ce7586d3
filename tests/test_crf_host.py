"""CPU checks of the CRF refinement's numpy mirror (tests/_crf_ref.py) and of crf.py's host side: the mirror against an independent
dense formulation, the properties the rule promises, the parameter checks, and the condition under which tests/test_gpu_crf.py may
compare labels (few pixels of its inputs have a top-two margin below the bar)."""
import functools

import numpy as np
import pytest
import torch

import _crf_ref as M

FLOOR = 2.0 ** -22
P = dict(radius=2, dilation=1, w_app=4.0, w_smooth=1.5, theta_alpha=6.0, theta_beta=20.0, theta_gamma=2.0, strength=1.5)


def _small(seed=0, h=6, w=5, c=4, n=1):
    rng = np.random.default_rng(seed)
    return (2.0 * rng.standard_normal((n, h, w, c))).astype(np.float32), rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _step_args(p):
    return (p["radius"], p["dilation"], M.spatial_table(p["radius"], p["dilation"], p["theta_alpha"]),
            M.spatial_table(p["radius"], p["dilation"], p["theta_gamma"]), p["w_app"], p["w_smooth"], M.inv2b_of(p["theta_beta"]),
            p["strength"])


@pytest.mark.parametrize("radius,dilation", [(1, 1), (2, 1), (1, 2), (2, 2), (1, 3)])
@pytest.mark.parametrize("probs", [False, True])
def test_mirror_equals_the_dense_kernel_matrix(radius, dilation, probs):
    """A sweep as loops over the window equals the sweep through an explicit [HW, HW] kernel matrix, void pixels included."""
    s, f = _small(3)
    if probs:
        s = np.exp(s) / np.exp(s).sum(-1, keepdims=True)
        s[0, 1, 1, 2] = 0.0
    s[0, 2, 3] = np.nan
    s[0, 5, 4, 0] = np.inf if not probs else 1.5
    p = dict(P, radius=radius, dilation=dilation)
    logp, q, valid = M.prepare(s, probs)
    assert (~valid).sum() == 2
    for _ in range(2):
        got = M.step(logp, q, valid, f, *_step_args(p))
        want = M.dense_step(logp[0], q[0], valid[0], f[0], *_step_args(p))
        np.testing.assert_allclose(got[0], want, rtol=0, atol=1e-14, equal_nan=True)
        q = got


def test_rows_sum_to_one_and_zero_sweeps_is_the_softmax():
    s, f = _small(4, 9, 7, 5, 2)
    e = np.exp(s.astype(np.float64) - s.max(-1, keepdims=True))
    np.testing.assert_allclose(M.refine(s, f, **dict(P, iterations=0)), e / e.sum(-1, keepdims=True), rtol=0, atol=1e-15)
    q = M.refine(s, f, **dict(P, iterations=3))
    np.testing.assert_allclose(q.sum(-1), 1.0, rtol=0, atol=1e-14)
    assert (q >= 0).all()
    sp = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    sp[0, 0, 0] *= 0.5                                       # a row that must be renormalised
    q0 = M.refine(sp, f, probs=True, **dict(P, iterations=0))
    np.testing.assert_allclose(q0.sum(-1), 1.0, rtol=0, atol=1e-14)


def test_a_class_without_prior_mass_stays_at_zero():
    s, f = _small(5)
    p = np.exp(s) / np.exp(s).sum(-1, keepdims=True)
    p[0, :, :, 1] = 0.0
    q = M.refine(p.astype(np.float32), f, probs=True, **dict(P, iterations=3))
    assert (q[..., 1] == 0.0).all() and np.isfinite(q).all()


def test_constant_frame_makes_the_two_kernels_one():
    """On a constant frame col == 1: appearance alone equals smoothness alone when theta_alpha == theta_gamma."""
    s, _ = _small(6, 8, 9, 5)
    f = M.frames_of("constant", 1, 8, 9, 0)
    a = M.refine(s, f, **dict(P, w_app=3.0, w_smooth=0.0, theta_alpha=2.5, theta_gamma=7.0, iterations=3))
    b = M.refine(s, f, **dict(P, w_app=0.0, w_smooth=3.0, theta_alpha=9.0, theta_gamma=2.5, iterations=3))
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-14)


def test_message_is_bounded_by_strength_and_checkerboard_cuts_it():
    """With theta_beta = 1 the colour term of two different colours is exactly 0: at dilation 1 and radius 1 with the appearance
    kernel alone only the diagonal neighbours (same colour) send."""
    s, _ = _small(7, 6, 6, 3)
    f = M.frames_of("checker", 1, 6, 6, 0)
    p = dict(P, radius=1, theta_beta=1.0, w_smooth=0.0)
    logp, q, valid = M.prepare(s)
    got = M.step(logp, q, valid, f, *_step_args(p))
    sa = M.spatial_table(1, 1, p["theta_alpha"]).astype(np.float64)
    y, x = 2, 3
    diag = sum(sa[dy + 1, dx + 1] * q[0, y + dy, x + dx] for dy in (-1, 1) for dx in (-1, 1))
    z = sa.sum() - sa[1, 1]
    t = logp[0, y, x] + p["strength"] * diag / z
    want = np.exp(t - t.max()) / np.exp(t - t.max()).sum()
    np.testing.assert_allclose(got[0, y, x], want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("code", range(1, 8))
def test_mirror_is_d4_covariant(code):
    s, f = _small(8, 7, 9, 4, 2)
    s[1, 3, 4] = np.nan
    p = dict(P, dilation=2, iterations=2)
    np.testing.assert_allclose(M.refine(M.d4(s, code), M.d4(f, code), **p), M.d4(M.refine(s, f, **p), code), rtol=0, atol=1e-13,
                               equal_nan=True)


def test_void_rows_send_nothing_and_carry_no_mass():
    """What a void row holds does not matter, its output is NaN, everything else is finite; and with uniform scores every pixel
    keeps the uniform distribution whatever is void around it (the normaliser leaves the void mass out)."""
    s, f = _small(9, 7, 7, 3)
    a, b = s.copy(), s.copy()
    a[0, 3, 3] = np.nan
    b[0, 3, 3] = [np.inf, 7.0, -2.0]
    qa, qb = M.refine(a, f, **dict(P, iterations=2)), M.refine(b, f, **dict(P, iterations=2))
    np.testing.assert_array_equal(qa, qb)
    assert np.isnan(qa[0, 3, 3]).all() and np.isfinite(np.delete(qa.reshape(49, 3), 24, axis=0)).all()
    u = np.zeros_like(s)
    u[0, 2, :] = np.nan
    qu = M.refine(u, f, **dict(P, iterations=2))
    ok = np.isfinite(qu[..., 0])
    np.testing.assert_allclose(qu[ok], 1.0 / 3.0, rtol=0, atol=1e-15)


def test_float32_leg_stays_close_to_float64():
    s, f = _small(10, 12, 11, 23)
    d = np.abs(M.refine(s, f, dt=np.float32, **M.DEFAULTS).astype(np.float64) - M.refine(s, f, **M.DEFAULTS)).max()
    assert 0 < d < 1e-5


def test_module_tables_are_the_mirrors():
    from uda_aerial_semantic_segmentation_research_amd import crf
    for r, d, th in ((1, 1, 3.0), (3, 2, 80.0), (5, 2, 0.7), (2, 4, 13.0)):
        np.testing.assert_array_equal(crf.spatial_table(r, d, th), M.spatial_table(r, d, th).reshape(-1))
    assert crf.inv2b_of(13.0) == M.inv2b_of(13.0) and crf.inv2b_of(13.0).dtype == np.float32
    assert crf.DEFAULTS == M.DEFAULTS


@pytest.mark.parametrize("bad", [dict(radius=0), dict(radius=6), dict(radius=2.0), dict(radius=True), dict(dilation=0), dict(dilation=5),
                                 dict(radius=3, dilation=4), dict(iterations=-1), dict(iterations=17), dict(w_app=-1.0),
                                 dict(w_app=0.0, w_smooth=0.0), dict(w_smooth=float("nan")), dict(theta_alpha=0.0),
                                 dict(theta_beta=-2.0), dict(theta_beta=1e-30), dict(theta_gamma=float("inf")), dict(strength=-0.1),
                                 dict(strength="x")])
def test_bad_parameters_raise_before_anything_else(bad):
    from uda_aerial_semantic_segmentation_research_amd import crf
    with pytest.raises(ValueError):
        crf.check_params(**bad)
    with pytest.raises(ValueError):                          # CPU tensors would raise RuntimeError: the parameters come first
        crf.refine(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), **bad)
    with pytest.raises(ValueError):
        crf.CrfLabeler(torch.nn.Conv2d(3, 3, 1), 3, **bad)


def test_operand_checks():
    from uda_aerial_semantic_segmentation_research_amd import crf
    assert crf.check_params() == crf.DEFAULTS
    s, f = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        crf.refine(s, f)
    with pytest.raises(RuntimeError, match="GPU"):
        crf.refine_labels(s, f)
    for scores, frames in ((s[0], f), (s, f.float()), (s, f[:, :3]), (s.double(), f), (torch.zeros(1, 33, 4, 4), f), (s, "frames")):
        with pytest.raises(ValueError):
            crf.refine(scores, frames)
    with pytest.raises(TypeError):
        crf.refine(s, f, sigma=3)


@functools.lru_cache(maxsize=None)
def _tile(radius, dilation):
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    return K.crf_tile(radius, dilation)


def test_tile_query_needs_no_gpu():
    for r, d in ((1, 1), (5, 2), (3, 3), (2, 4)):
        th, tw = _tile(r, d)
        assert th >= 8 and tw >= 8 and th % 2 == 0
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    with pytest.raises(ValueError):
        K.crf_tile(5, 3)


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_gpu_inputs_keep_the_tie_share_under_the_cap(name):
    """tests/test_gpu_crf.py compares labels except where the float64 top-two margin is below the bar, and allows that at 0.5 % of
    a case's pixels at most: here the mirror's own two legs show that every case's inputs satisfy it."""
    case = M.BY_NAME[name]
    s, f = M.make_case(case, _tile(case["radius"], case["dilation"]))
    p = M.params_of(case)
    q64 = M.refine(s, f, probs=case["probs"], **p)
    q32 = M.refine(s, f, probs=case["probs"], dt=np.float32, **p).astype(np.float64)
    ok = np.isfinite(q64[..., 0])
    np.testing.assert_array_equal(np.isfinite(q32[..., 0]), ok)
    bar = max(4.0 * float(np.abs(q32[ok] - q64[ok]).max(initial=0.0)), FLOOR)
    assert bar < 1e-4, bar
    close = (M.margin(q64[ok]) < bar).sum()
    assert close <= 0.005 * ok.size, (close, ok.size)
    assert ok.sum() >= 0.5 * ok.size or case["shape"] == "3x2"
