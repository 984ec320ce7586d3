"""GPU checks of the CRF refinement (crf.py, csrc/crf.hip) against its numpy mirror tests/_crf_ref.py, on the inputs that
tests/test_crf_host.py vets on the CPU.  Every graded figure is held to tests/_grade.py's bar max(e) <= max(4 x max(d), 2^-22),
d the float32 evaluation's deviation from float64, errors relative to 1 (the outputs are probabilities); a single sweep is
graded from its own device inputs, so that no error is carried between sweeps.  Set UDASEG_DEVIATION_LOG to collect the figures."""
import functools

import numpy as np
import pytest
import torch

import _crf_ref as M
from _grade import Grader

pytestmark = pytest.mark.gpu


class CrfGrader(Grader):
    PREFIX = "crf-grade"


@pytest.fixture(scope="module")
def G():
    from uda_aerial_semantic_segmentation_research_amd import _lib, crf
    _lib.require_gpu()
    return crf


@functools.lru_cache(maxsize=None)
def _tile(radius, dilation):
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    return K.crf_tile(radius, dilation)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = M.BY_NAME[name]
    return M.make_case(case, _tile(case["radius"], case["dilation"]))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The mirror's float64 and float32 refinements of a case, computed once and shared (treated as read-only)."""
    case = M.BY_NAME[name]
    s, f = _inputs(name)
    p = M.params_of(case)
    return (M.refine(s, f, probs=case["probs"], **p), M.refine(s, f, probs=case["probs"], dt=np.float32, **p).astype(np.float64))


def _padded(s, pad, poison):
    """Device [N,H,W,ldc] fp32 buffer of NHWC scores, ldc = ceil4(C) + pad, the padding channels poisoned."""
    c = s.shape[-1]
    ldc = (c + 3) // 4 * 4 + pad
    buf = torch.full(s.shape[:-1] + (ldc,), poison, dtype=torch.float32, device="cuda")
    buf[..., :c] = torch.from_numpy(s).cuda()
    return buf, ldc


def _nchw(s):
    """The [N,C,H,W] view of a padded NHWC buffer that Unet.forward returns: crf.refine reads it in place."""
    buf, _ = _padded(s, 0, 0.0)
    return buf.permute(0, 3, 1, 2)[:, :s.shape[-1]]


def _masked(ok, *arrays):
    """The arrays with the void rows set to 0, once the void rows have been compared for themselves."""
    return [np.where(ok[..., None], np.nan_to_num(np.asarray(a, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0), 0.0) for a in arrays]


def _grade_probs(g, what, got, r64, r32):
    ok = np.isfinite(r64).all(axis=-1)
    nan_rows = np.isnan(got).all(axis=-1)
    if not np.array_equal(nan_rows, ~ok) or not np.isfinite(got[ok]).all():
        g.bad.append(f"{what}: NaN rows differ from the mirror's ({int(nan_rows.sum())} against {int((~ok).sum())})")
        return ok
    got0, a64, a32 = _masked(ok, got, r64, r32)
    ones = np.ones_like(a64)
    g.grade(what, got0, a64, a32, ones)
    rs = np.where(ok, 1.0, 0.0)
    g.grade(what + " row sums", got0.sum(-1), rs, a32.sum(-1), np.ones_like(rs))
    return ok


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_prepare_and_one_sweep_from_its_own_input(G, name):
    """udaseg_crf_prepare against the mirror's P0 and log P0, then ONE udaseg_crf_step on a Q that is not P0, graded against the
    float64 sweep of the very logp, Q and flags the device holds; padded rows with poison in the padding channels; NaN rows where
    the mirror has them; the padding channels of every output are 0; a second call gives the same bits."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    case = M.BY_NAME[name]
    s, f = _inputs(name)
    n, h, w, c = s.shape
    p = M.params_of(case)
    g = CrfGrader(name)
    sbuf, ldc = _padded(s, case["pad"], float("nan"))
    ldq = ldc
    frames = torch.from_numpy(f).cuda()
    logp, q0, out, out2 = (torch.full((n, h, w, ldq), 7.0, dtype=torch.float32, device="cuda") for _ in range(4))
    valid = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    K.crf_prepare(sbuf, ldc, c, case["probs"], n * h * w, logp, q0, ldq, valid)
    l64, p64, v64 = M.prepare(s, case["probs"])
    l32, p32, _ = M.prepare(s, case["probs"], np.float32)
    assert np.array_equal(valid.cpu().numpy().astype(bool), v64)
    ok = _grade_probs(g, "P0", q0[..., :c].cpu().numpy(), p64, p32.astype(np.float64))
    lg = logp[..., :c].cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isneginf(lg[ok]), np.isneginf(l64[ok])) and np.isnan(lg[~ok]).all()
    lg0, a64, a32 = _masked(ok, lg, l64, l32)
    g.grade("log P0", lg0, a64, a32, 1.0 + np.abs(a64))
    assert float(logp[..., c:].abs().max().item() if ldq > c else 0.0) == 0.0
    assert float(q0[..., c:].abs().max().item() if ldq > c else 0.0) == 0.0

    # a Q of its own: the prepared scores of another seed with the same void rows
    s2 = M.scores_of(n, h, w, c, case["probs"], case["void"], case["seed"] + 500)
    s2buf, _ = _padded(s2, case["pad"], float("nan"))
    qin, scratch = torch.empty_like(logp), torch.empty_like(logp)
    v2 = torch.empty_like(valid)
    K.crf_prepare(s2buf, ldc, c, case["probs"], n * h * w, scratch, qin, ldq, v2)
    assert torch.equal(v2, valid)
    sa, sg = M.spatial_table(p["radius"], p["dilation"], p["theta_alpha"]), M.spatial_table(p["radius"], p["dilation"], p["theta_gamma"])
    args = (c, ldq, p["radius"], p["dilation"], torch.from_numpy(sa.reshape(-1)).cuda(), torch.from_numpy(sg.reshape(-1)).cuda(),
            p["w_app"], p["w_smooth"], float(M.inv2b_of(p["theta_beta"])), p["strength"])
    K.crf_step(logp, qin, valid, frames, *args, out)
    K.crf_step(logp, qin, valid, frames, *args, out2)
    torch.cuda.synchronize()
    margs = (f, p["radius"], p["dilation"], sa, sg, p["w_app"], p["w_smooth"], M.inv2b_of(p["theta_beta"]), p["strength"])
    dl, dq = logp[..., :c].cpu().numpy(), qin[..., :c].cpu().numpy()
    r64 = M.step(dl, dq, v64, *margs)
    r32 = M.step(dl, dq, v64, *margs, dt=np.float32).astype(np.float64)
    _grade_probs(g, "sweep", out[..., :c].cpu().numpy(), r64, r32)
    if ldq > c:
        assert float(out[..., c:].abs().max().item()) == 0.0, "padding channels"
    assert torch.equal(_bits(out), _bits(out2)), "two sweeps of one input differ"
    g.done()


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_refine_and_labels(G, name):
    """The whole refine against the mirror run for the same number of sweeps (the bar then carries the recursion's own
    amplification; strength <= 2 in every case), its labels against the mirror's first maximum except where the float64 top-two
    margin is below the bar (at most 0.5 % of a case), and the same bits from a second call."""
    case = M.BY_NAME[name]
    assert case["strength"] <= 2.0
    s, f = _inputs(name)
    c = s.shape[-1]
    p = M.params_of(case)
    g = CrfGrader(name)
    q64, q32 = _reference(name)
    frames = torch.from_numpy(f).cuda()
    q = G.refine(_nchw(s), frames, probs=case["probs"], **p)
    assert tuple(q.shape) == (s.shape[0], c) + s.shape[1:3] and q.dtype == torch.float32 and q.stride(1) == 1
    got = q.permute(0, 2, 3, 1).cpu().numpy()
    ok = _grade_probs(g, f"refine T={p['iterations']}", got, q64, q32)
    labels, conf = G.refine_labels(_nchw(s), frames, probs=case["probs"], **p)
    bar = max(4.0 * float(np.abs(q32[ok] - q64[ok]).max(initial=0.0)), 2.0 ** -22)
    lab = labels.cpu().numpy()
    want = np.where(ok, np.argmax(np.nan_to_num(q64, nan=0.0), axis=-1), 255)
    differ = lab != want
    near = ok & (M.margin(np.nan_to_num(q64, nan=0.0)) < bar)
    if (differ & ~near).any():
        g.bad.append(f"labels: {int((differ & ~near).sum())} differ where the margin is above the bar")
    if near.sum() > 0.005 * ok.size:
        g.bad.append(f"labels: {int(near.sum())} of {ok.size} pixels have a margin below the bar")
    cf = conf.cpu().numpy().astype(np.float64)
    top = np.where(ok, np.nan_to_num(q64, nan=0.0).max(axis=-1), 0.0)
    if not (np.abs(cf - top) <= bar).all():
        g.bad.append(f"confidence: off by {float(np.abs(cf - top).max()):.3e}")
    again = G.refine(_nchw(s), frames, probs=case["probs"], **p)
    assert torch.equal(_bits(again), _bits(q)), "two calls differ"
    g.done()


def test_zero_sweeps_and_out_buffer(G):
    s, f = _inputs("sweeps-0")
    frames = torch.from_numpy(f).cuda()
    n, h, w, c = s.shape
    out = torch.full((n, h, w, 8), 3.0, dtype=torch.float32, device="cuda")
    q = G.refine(_nchw(s), frames, iterations=0, out=out)
    assert q.data_ptr() == out.data_ptr()
    p0 = M.prepare(s)[1]
    np.testing.assert_allclose(q.permute(0, 2, 3, 1).cpu().numpy(), p0, rtol=0, atol=2.0 ** -22, equal_nan=True)
    for t in (1, 2):                                         # the last sweep lands in out for an odd and an even count
        out.fill_(3.0)
        q = G.refine(_nchw(s), frames, iterations=t, out=out)
        assert torch.equal(_bits(q), _bits(G.refine(_nchw(s), frames, iterations=t))) and float(out[..., c:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        G.refine(_nchw(s), frames, out=out[..., :4])
    with pytest.raises(ValueError):
        G.refine(_nchw(s), frames[:, :-1])
    dense = torch.from_numpy(np.ascontiguousarray(np.moveaxis(s, -1, 1))).cuda()          # plain NCHW: one layout kernel first
    assert torch.equal(_bits(G.refine(dense, frames, iterations=2)), _bits(q))


@pytest.mark.parametrize("name", ["frame-random", "void-all", "window-3x3"])
@pytest.mark.parametrize("code", range(1, 8))
def test_d4_covariance(G, name, code):
    """refine of a flipped or transposed input is the flipped or transposed output, within the bar."""
    case = M.BY_NAME[name]
    s, f = _inputs(name)
    p = M.params_of(case)
    q64, q32 = _reference(name)
    ok = np.isfinite(q64[..., 0])
    bar = max(4.0 * float(np.abs(q32[ok] - q64[ok]).max()), 2.0 ** -22)
    base = G.refine(_nchw(s), torch.from_numpy(f).cuda(), probs=case["probs"], **p).permute(0, 2, 3, 1).cpu().numpy()
    turned = G.refine(_nchw(M.d4(s, code)), torch.from_numpy(M.d4(f, code)).cuda(), probs=case["probs"], **p)
    turned = turned.permute(0, 2, 3, 1).cpu().numpy()
    want = M.d4(base, code)
    assert np.array_equal(np.isnan(turned), np.isnan(want))
    e = float(np.abs(np.nan_to_num(turned) - np.nan_to_num(want)).max())
    print(f"crf-grade d4 {name} code {code}: {e:.3e} bar {bar:.3e}")
    assert e <= bar


@pytest.fixture(scope="module")
def r18():
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(0)
    return Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).to("cuda").eval()


def test_crf_labeler_labels_the_refined_forward(G, r18):
    """CrfLabeler.label: the masks equal pseudo_labels(refine(out, frames), probs=True) under the thresholds it took, and the
    table moved by exactly the pixel count."""
    from uda_aerial_semantic_segmentation_research_amd import pseudo
    from uda_aerial_semantic_segmentation_research_amd.data import prepare_batch
    frames = torch.from_numpy(M.frames_of("random", 2, 64, 96, 3)).cuda()
    lab = G.CrfLabeler(r18, 23, portion=0.5, cap=0.9, radius=2, dilation=2, iterations=3)
    masks = lab.label(frames)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (2, 64, 96) and lab.calls == 1
    assert int(lab.hist.table.sum().item()) + int(lab.hist.nonfinite.item()) == 2 * 64 * 96
    with torch.no_grad():
        out = r18(prepare_batch(frames, None, None, torch.float32)[0])
    q = G.refine(out, frames, radius=2, dilation=2, iterations=3)
    assert torch.equal(masks, pseudo.pseudo_labels(q, lab.thr_bins, 255, probs=True))
    raw = pseudo.pseudo_labels(out, lab.thr_bins, 255)
    assert not torch.equal(masks, raw)                       # the refinement changed something
    pairs = list(lab.loader([frames]))
    assert len(pairs) == 1 and pairs[0][1].dtype == torch.uint8 and lab.calls == 2
    assert int(lab.hist.table.sum().item()) + int(lab.hist.nonfinite.item()) == 2 * 2 * 64 * 96


def test_refine_large_refines_the_blended_frame(G, r18):
    from uda_aerial_semantic_segmentation_research_amd.predict import predict_large
    frame = M.frames_of("random", 1, 70, 90, 4)[0]
    kw = dict(radius=2, dilation=1, iterations=2)
    labels, q = G.refine_large(r18, frame, tile=32, overlap=0.25, return_probs=True, **kw)
    _, probs = predict_large(r18, frame, tile=32, overlap=0.25, return_probs=True)
    want = G.refine(probs, torch.from_numpy(frame).cuda()[None], probs=True, **kw)
    assert torch.equal(_bits(q), _bits(want))
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (70, 90) and torch.equal(labels, want.argmax(1)[0])
    assert torch.equal(G.refine_large(r18, frame, tile=32, overlap=0.25, **kw), labels)
