"""GPU checks of the calibration module: the reliability-table kernel against the float64 mirror (tests/_calib_ref.py) edge by
edge, the fixed-point confidence sums, every row width, the grid stride, the one definition shared with ``udaseg_conf_share``,
the finishing kernel against the host arithmetic, accumulation / determinism, the NLL sums graded against float64, the Newton
step bit for bit, the temperature fit, and the module level (``evaluate``, ``TemperatureScaler.fit``, ``state_dict``)."""
import numpy as np
import pytest
import torch

import _calib_ref as R
import _scores_ref as S
from _loss_ref import FLOOR, Grader

pytestmark = pytest.mark.gpu

DELTA = 1e-5         # 170 fp32 ulp of a confidence near 1: the mirror's fp32 leg stays within 4e-7 of its float64 leg on these inputs
HIST_SWEEP = 512 * 256       # pixels one sweep of calib_hist_kernel's grid covers (CH_BLOCKS x CH_THREADS, include/udaseg.h)


@pytest.fixture(scope="module")
def C():
    from uda_aerial_semantic_segmentation_research_amd import _lib, calibration
    _lib.require_gpu()
    return calibration


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import kernels
    return kernels


_CASES = {}


def _case(name):
    """(logits [N,C,H,W], target [N,H,W], flat logits [P,C], flat target [P]): made once, shared, never written."""
    if name not in _CASES:
        z, t = R.case(name)
        _CASES[name] = (z, t) + R.flat(z, t)
    return _CASES[name]


def _scaler(C, beta):
    if beta is None:
        return None
    sc = C.TemperatureScaler("cuda")._need_state()
    sc.inv_temp.fill_(beta)
    return sc


def _device_tables(C, z, t, bins, beta=None, probs=False):
    h = C.ReliabilityHistogram(z.shape[1], bins, "cuda")
    h.update(torch.from_numpy(np.ascontiguousarray(z)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda(), probs=probs,
             scaler=_scaler(C, beta))
    return h.tables() + (h,)


def _check_tables(name, ktab, kcnt, zf, tf, bins, beta=None, probs=False):
    """test_gpu_curves._check_tables's criterion: per predicted class the cumulative counts from the top bin down (count and
    correct each) may differ from the float64 mirror's by at most the number of mirror confidences within DELTA of that bin's lower
    edge; row totals and counters exact; the share of near-edge confidences below 2 %.  conf_q: per class row the sum over the
    bins within n_row * (0.5 + 2^24 e), e = max(4 x the fp32 leg's worst |p32 - p64|, 2^-22)."""
    b = np.float32(1.0 if beta is None else beta)
    c = zf.shape[1]
    r64, c64, i64 = R.tables(zf, tf, bins, b, R.F64, probs)
    _, _, i32 = R.tables(zf, tf, bins, b, R.F32, probs)
    assert kcnt.tolist() == c64.tolist(), (name, "counters", kcnt, c64)
    used = i64["used"]
    near = R.near_edge_counts(i64["p"][used], i64["cls"][used], c, bins, DELTA)
    worst = 0
    for k, what in ((0, "count"), (1, "correct")):
        assert np.array_equal(ktab[k].sum(axis=1), r64[k].sum(axis=1)), (name, what, "row totals differ")
        ck = np.cumsum(ktab[k][:, ::-1], axis=1)[:, ::-1]
        cr = np.cumsum(r64[k][:, ::-1], axis=1)[:, ::-1]
        diff = np.abs(ck - cr)
        worst = max(worst, int(diff.max()))
        bad = np.argwhere(diff > near)
        assert len(bad) == 0, (name, what, "class, edge:", bad[:5].tolist(), "diff", diff[tuple(bad[0])], "allowed", near[tuple(bad[0])])
    share = near.sum() / float(max(c64[0], 1))
    dp = float(np.abs(i32["p"][used].astype(np.float64) - i64["p"][used]).max(initial=0.0))
    e = max(4.0 * dp, FLOOR)
    n_row = r64[0].sum(axis=1).astype(np.float64)
    dq = np.abs(ktab[2].sum(axis=1) - r64[2].sum(axis=1)).astype(np.float64)
    allowed = n_row * (0.5 + R.Q_ONE * e)
    print(f"calib-grade {name} bins={bins} beta={float(b):g}: largest per-edge difference {worst}, near-edge share {100 * share:.3f} %, "
          f"fp32 leg max |p32 - p64| {dp:.2e}, worst conf_q row |got - want| / allowed {float((dq / np.maximum(allowed, 1)).max()):.3f}, "
          f"exact-equal count tables: {bool(np.array_equal(ktab[0], r64[0]))}")
    assert share < 0.02, (name, share)
    assert np.all(dq <= allowed), (name, "conf_q", dq, allowed)
    assert (ktab[2] > 0).sum() == (ktab[0] > 0).sum() and np.all(ktab[1] <= ktab[0]) and ktab.min() >= 0
    return near


@pytest.mark.parametrize("beta", [None, 0.5, 2.0])
@pytest.mark.parametrize("bins", [15, 64])
@pytest.mark.parametrize("name", list(R.CASES))
def test_tables_edge_by_edge(C, name, bins, beta):
    z, t, zf, tf = _case(name)
    ktab, kcnt, _ = _device_tables(C, z, t, bins, beta)
    _check_tables(name, ktab, kcnt, zf, tf, bins, beta)


@pytest.mark.parametrize("classes,ldc", [(ldc - 1, ldc) for ldc in range(4, 33, 4)] + [(4, 4), (32, 32)])
def test_every_row_width(K, classes, ldc):
    """All eight row widths of both kernels at kernel level: junk in the pad lanes, an exact tie of the maximum (the lower index
    wins), and a NaN above channel 0, whose pixel lands in counters[2], in no cell and in no sum."""
    rows = S.sweep_rows(classes, seed=300 + ldc)
    rng = np.random.default_rng(ldc)
    tgt = rng.integers(0, classes, S.PIXELS)
    tgt[[3, 290]] = -1, classes + 5
    lo, hi = S.tie_channels(classes)
    tgt[S.TIE_PIXEL], tgt[S.NAN_PIXEL] = lo, 0
    assert np.isnan(rows[S.NAN_PIXEL]).sum() == 1 and R.confidence(rows)[0][S.TIE_PIXEL] == lo
    buf, dt = torch.from_numpy(S.padded(rows, ldc)).cuda(), torch.from_numpy(tgt).cuda()
    for beta in (None, 0.7):
        inv = None if beta is None else torch.full((1,), beta, dtype=torch.float32, device="cuda")
        tables = torch.zeros(3 * classes * 15 + 3, dtype=torch.int64, device="cuda")
        K.calib_hist(buf, dt, S.PIXELS, classes, ldc, False, inv, 15, tables[:-3], tables[-3:])
        host = tables.cpu().numpy()
        ktab, kcnt = host[:-3].reshape(3, classes, 15), host[-3:]
        assert kcnt.tolist() == [S.PIXELS - 3, 2, 1]
        _check_tables(f"classes={classes} ldc={ldc}", ktab, kcnt, rows, tgt, 15, beta)
        # the tie pixel is counted as correct for the lower channel: without it class `lo` has one correct pixel fewer
        keep = np.arange(S.PIXELS) != S.TIE_PIXEL
        assert ktab[1, lo].sum() == R.tables(rows[keep], tgt[keep], 15, np.float32(beta or 1.0))[0][1, lo].sum() + 1
        # the NLL sums of the same rows
        sums = torch.zeros(4, dtype=torch.float64, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        K.calib_nll(buf, dt, S.PIXELS, classes, ldc, inv, torch.empty(4 * K.seg_partials(), dtype=torch.float64, device="cuda"), sums, cnt)
        _grade_sums(f"classes={classes} ldc={ldc} beta={beta}", sums.cpu().numpy(), cnt.cpu().numpy(), rows, tgt, beta)


def _grade_sums(tag, got, cnt, zf, tf, beta):
    b = np.float32(1.0 if beta is None else beta)
    s64, mag, c64 = R.nll_sums(zf, tf, b, R.F64)
    s32, _, _ = R.nll_sums(zf, tf, b, R.F32)
    assert cnt.tolist() == c64.tolist() and got[0] == s64[0], (tag, cnt, c64, got[0])
    g = Grader(f"calib {tag}")
    g.grade("nll, g1, g2 sums", got[1:], s64[1:], s32[1:], mag[1:])
    g.done()
    return s64


def test_grid_stride(C):
    """More pixels than one sweep of the histogram kernel's grid covers (512 blocks x 256 threads)."""
    z, t = R.seeded_input(2, 5, 384, 384, seed=7, invalid=200)
    assert t.size > 2 * HIST_SWEEP
    zf, tf = R.flat(z, t)
    ktab, kcnt, _ = _device_tables(C, z, t, 15)
    _check_tables("grid-stride", ktab, kcnt, zf, tf, 15)
    assert kcnt[0] == t.size - 200


def test_one_definition_with_conf_share(C, K):
    """bins = 16, beta = 1 (NULL), every target valid: p * 16 is exact in fp32, so ``p >= k / 16`` and ``floor(16 p) >= k`` are one
    statement and the cumulative counts equal udaseg_conf_share's ``above`` exactly.  Also on probabilities that hold exact 0.5
    and 1.0 values."""
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    z, t, _, _ = _case("c23")
    t = np.where((t >= 0) & (t < 23), t, 0)
    zt = torch.from_numpy(z).cuda()
    probs = torch.softmax(zt, dim=1)
    probs[0, :, 0, :8] = 0.0
    probs[0, 3, 0, :4] = 1.0                                              # exact 1.0: the top bin
    probs[0, 5, 0, 4:8] = 0.5                                             # exact 0.5 twice: the lower index wins, bin 8
    probs[0, 9, 0, 4:8] = 0.5
    for scores, is_probs in ((zt, False), (probs, True)):
        ktab, kcnt, _ = _device_tables(C, scores.cpu().numpy(), t, 16, probs=is_probs)
        assert kcnt.tolist() == [t.size, 0, 0]
        buf, ldc = padded_nhwc(scores)
        n, c, h, w = scores.shape
        counts = torch.zeros(2, n, dtype=torch.int64, device="cuda")
        share = torch.empty(n, dtype=torch.float32, device="cuda")
        from_top = np.cumsum(ktab[0].sum(axis=0)[::-1])[::-1]
        for k in (8, 12, 15):
            K.conf_share(buf, n, h * w, c, ldc, is_probs, k / 16.0, counts[0], counts[1], share)
            assert int(counts[0].sum()) == from_top[k] and int(counts[1].sum()) == 0, (is_probs, k)
    # the eight hand-made pixels alone: 1.0 in the top bin, the 0.5 tie at the lower index in bin 8, conf_q exact
    ktab, kcnt, _ = _device_tables(C, probs[:1, :, :1, :8].cpu().numpy(), t[:1, :1, :8], 16, probs=True)
    want = np.zeros((23, 16), dtype=np.int64)
    want[3, 15], want[5, 8] = 4, 4
    assert kcnt.tolist() == [8, 0, 0] and np.array_equal(ktab[0], want)
    assert ktab[2, 3, 15] == 4 * 2 ** 24 and ktab[2, 5, 8] == 4 * 2 ** 23 and ktab[2].sum() == 6 * 2 ** 24


def test_finish_kernel_against_host_arithmetic(C, K):
    for name, bins in (("c5", 64), ("c23", 15), ("c32", 10)):
        z, t, _, _ = _case(name)
        ktab, _, h = _device_tables(C, z, t, bins, 2.0 if name == "c23" else None)
        _compare_finish(C, name, h.compute(), ktab)
    # hand-made tables: an empty class, empty bins, and nothing at all
    tab = np.zeros((3, 3, 4), dtype=np.int64)
    tab[:, 0, 3] = 10, 7, 10 * 14680064
    tab[:, 1, 0] = 5, 0, 5 * 2097152
    for name, tb in (("hand-made", tab), ("empty", np.zeros_like(tab))):
        f = torch.empty(6 + 12, dtype=torch.float64, device="cuda")
        K.calib_finish(torch.from_numpy(tb).cuda().reshape(-1), 3, 4, f[:6], f[6:])
        _compare_finish(C, name, {"out": f[:6], "per_class": f[6:].view(4, 3)}, tb)


def _compare_finish(C, name, dev, ktab):
    host = C.reliability_from_tables(ktab)
    assert dev["out"].is_cuda and dev["out"].dtype == torch.float64
    pairs = [(k, dev["out"][i].item(), host[k]) for i, k in enumerate(C.OUT_KEYS)]
    pc = dev["per_class"].cpu().numpy()
    for i, k in enumerate(C.CLASS_KEYS):
        pairs += [(f"{k}[{c}]", pc[i, c], host["per_class"][k][c]) for c in range(pc.shape[1])]
    worst = 0.0
    for what, d, w in pairs:
        assert np.isnan(d) == np.isnan(w), (name, what, d, w)
        if not np.isnan(w):
            rel = abs(d - w) / max(abs(w), 1e-300) if w != 0 else abs(d)
            worst = max(worst, rel)
            assert rel <= 1e-12, (name, what, d, w)
    print(f"calib-grade finish {name}: max relative difference device / host {worst:.2e}")


def test_accumulation_and_determinism(C, K):
    """Tables: integers, so two updates on halves equal one on the whole exactly.  NLL sums: two identical call sequences give
    identical bits; two calls on halves against one call on the whole is NOT bit-exact by construction -- the halves' blocks hold
    other pixels than the whole's, so the float64 additions happen in another order -- and is held to 1e-13 of the magnitude
    (float64 rounding of at most 8192 terms; the terms themselves are the same fp32 numbers, and on an MI355X the difference
    measured 0: fp32 values of this range sum exactly in float64).  n is exact."""
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    z, t, zf, tf = _case("c23")
    zt, tt = torch.from_numpy(z).cuda(), torch.from_numpy(t).cuda()
    whole = C.ReliabilityHistogram(23, 15, "cuda").update(zt, tt)
    again = C.ReliabilityHistogram(23, 15, "cuda").update(zt, tt)
    halves = C.ReliabilityHistogram(23, 15, "cuda").update(zt[:1], tt[:1]).update(zt[1:], tt[1:, None])
    assert torch.equal(whole.buffer, again.buffer) and torch.equal(whole.buffer, halves.buffer)
    a, b = whole.compute(), again.compute()
    assert all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in ("out", "per_class"))
    twice = C.ReliabilityHistogram(23, 15, "cuda").update(zt, tt).update(zt, tt.int())
    assert torch.equal(twice.buffer, 2 * whole.buffer)
    assert int(twice.reset().buffer.abs().sum()) == 0

    inv = torch.full((1,), 0.36, dtype=torch.float32, device="cuda")

    def sums_of(parts):
        s, c = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
        for zz, ttt in parts:
            buf, ldc = padded_nhwc(zz)
            K.calib_nll(buf, ttt.reshape(-1).contiguous(), ttt.numel(), 23, ldc, inv,
                        torch.empty(4 * K.seg_partials(), dtype=torch.float64, device="cuda"), s, c)
        return s, c

    s1, c1 = sums_of([(zt, tt)])
    s2, c2 = sums_of([(zt, tt)])
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(c1, c2)
    sh, ch = sums_of([(zt[:1], tt[:1]), (zt[1:], tt[1:])])
    sh2, _ = sums_of([(zt[:1], tt[:1]), (zt[1:], tt[1:])])
    assert torch.equal(sh.view(torch.int64), sh2.view(torch.int64)) and torch.equal(ch, c1)
    _, mag, _ = R.nll_sums(zf, tf, np.float32(0.36))
    d = np.abs(sh.cpu().numpy() - s1.cpu().numpy()) / mag
    print(f"calib-grade accumulate: halves against whole, |difference| / magnitude {d}")
    assert d[0] == 0 and np.all(d <= 1e-13)


@pytest.mark.parametrize("beta", [None, 0.36])
@pytest.mark.parametrize("name", list(R.CASES))
def test_nll_sums_against_float64(K, name, beta):
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    z, t, zf, tf = _case(name)
    buf, ldc = padded_nhwc(torch.from_numpy(z).cuda())
    inv = None if beta is None else torch.full((1,), beta, dtype=torch.float32, device="cuda")
    sums = torch.zeros(4, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    K.calib_nll(buf, torch.from_numpy(t).cuda().reshape(-1), t.size, z.shape[1], ldc, inv,
                torch.empty(4 * K.seg_partials(), dtype=torch.float64, device="cuda"), sums, cnt)
    _grade_sums(f"{name} beta={beta}", sums.cpu().numpy(), cnt.cpu().numpy(), zf, tf, beta)


def test_step_bit_for_bit(K):
    """Given the DEVICE's own sums, the new beta equals the mirror's bit for bit: one IEEE double division, one subtraction,
    compares, one rounding to fp32 (no multiply feeds an add, so nothing can be contracted)."""
    from uda_aerial_semantic_segmentation_research_amd._args import padded_nhwc
    z, t, _, _ = _case("c23")
    tt = torch.from_numpy(t).cuda().reshape(-1)
    parts = torch.empty(4 * K.seg_partials(), dtype=torch.float64, device="cuda")
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    steps = 0
    for scale, beta0 in ((1.0, 1.0), (3.0, 1.0), (3.0, 0.25), (0.25, 2.0), (1.0, 0.7)):
        buf, ldc = padded_nhwc(torch.from_numpy(z * np.float32(scale)).cuda())
        inv = torch.full((1,), beta0, dtype=torch.float32, device="cuda")
        sums = torch.zeros(4, dtype=torch.float64, device="cuda")
        K.calib_nll(buf, tt, t.size, 23, ldc, inv, parts, sums, torch.zeros(3, dtype=torch.int64, device="cuda"))
        host = sums.cpu().numpy()
        K.calib_step(sums, inv, state)
        steps += 1
        want, wstate = R.step(host, np.float32(beta0))
        got, st = inv.cpu().numpy()[0], state.cpu().numpy()
        print(f"calib-grade step x{scale} from {beta0}: beta' {got!r} (mirror {want!r}), mean nll {st[0]:.6f}, mean g1 {st[1]:.6f}")
        assert got.tobytes() == np.float32(want).tobytes(), (scale, beta0, got, want)
        assert st[:3].tobytes() == wstate[:3].tobytes() and st[3] == steps and int(sums.abs().sum()) == 0
        if (scale, beta0) == (3.0, 1.0):
            assert got == 0.25                                               # the raw step is negative: clamped to beta / 4
    for hand in ([0.0, 0.0, 0.0, 0.0], [100.0, 50.0, 3.0, 0.0], [100.0, float("nan"), 3.0, 1.0], [100.0, 50.0, float("inf"), 1.0]):
        inv = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
        sums = torch.tensor(hand, dtype=torch.float64, device="cuda")
        K.calib_step(sums, inv, state)
        steps += 1
        st = state.cpu().numpy()
        assert inv.item() == float(np.float32(0.7)) and st[2] == 0 and st[3] == steps and float(sums.abs().sum()) == 0, hand


@pytest.mark.parametrize("scale", [1.0, 3.0, 0.25])
def test_fit(C, scale):
    """fit_logits(iters=8) against the float64 mirror's trajectory with the same guards: |beta_dev - beta_64| within 4 x the fp32
    leg's own final deviation, floored at 2^-22 relative.  The 15-bin ECE from the device tables at the fitted temperature agrees
    with the mirror's AT THE DEVICE'S beta to within the edge allowance -- a pixel that changes bins moves sum_b |a_b - q_b| by at
    most 2, and conf_q is within 0.5 + 2^24 e per pixel -- and on the x 3 input it falls from before the fit to after it."""
    z, t, zf, tf = _case("c23")
    zs = zf * np.float32(scale)
    zt, tt = torch.from_numpy(z * np.float32(scale)).cuda(), torch.from_numpy(t).cuda()
    sc = C.TemperatureScaler("cuda").fit_logits(zt, tt, iters=8)
    rep = sc.report()
    t64, t32 = R.fit(zs, tf, 8, R.F64), R.fit(zs, tf, 8, R.F32)
    bar = max(4.0 * abs(t32[-1] - t64[-1]), FLOOR * t64[-1])
    err = abs(rep["beta"] - t64[-1])
    print(f"calib-grade fit x{scale}: beta_dev {rep['beta']!r}  beta_64 {t64[-1]!r}  |diff| {err:.3e}  fp32 leg |diff| "
          f"{abs(t32[-1] - t64[-1]):.3e}  bar {bar:.3e}  steps {rep['steps']}  last move {rep['last_move']:.3e}")
    assert rep["steps"] == 8 and rep["counted"] == 8 * (t.size - 50) and rep["void"] == 8 * 50 and rep["nonfinite"] == 0
    assert abs(sc.temperature() - 1.0 / rep["beta"]) < 1e-12
    before = C.ReliabilityHistogram(23, 15, "cuda").update(zt, tt).reliability()
    after = C.ReliabilityHistogram(23, 15, "cuda").update(zt, tt, scaler=sc).reliability()
    beta_dev = np.float32(rep["beta"])
    r64, c64, i64 = R.tables(zs, tf, 15, beta_dev)
    _, _, i32 = R.tables(zs, tf, 15, beta_dev, R.F32)
    used = i64["used"]
    near = R.near_edge_counts(i64["p"][used], i64["cls"][used], 23, 15, DELTA).sum()
    e = max(4.0 * float(np.abs(i32["p"][used].astype(np.float64) - i64["p"][used]).max()), FLOOR)
    allowance = (2.0 * near + c64[0] * (0.5 / R.Q_ONE + e)) / c64[0]
    want = R.finish(r64)[0]
    print(f"calib-grade fit x{scale}: ece before {before['ece']:.6f} after {after['ece']:.6f} (mirror {want[3]:.6f}, allowance "
          f"{allowance:.2e}), gap before {before['gap']:.4f} after {after['gap']:.4f}")
    assert abs(after["ece"] - want[3]) <= allowance
    assert err <= bar
    if scale == 3.0:
        assert before["gap"] > 0 and after["ece"] < before["ece"]


def _tiny_model_and_loader():
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(4)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=5).cuda().eval()
    g = torch.Generator().manual_seed(8)
    images = [torch.randn(2, 3, 64, 64, generator=g) for _ in range(2)]
    loader = []
    with torch.no_grad():
        for x in images:                                                  # labels that follow the model on 2 pixels of 3
            pred = net(x.cuda()).argmax(1).cpu()
            noise = torch.randint(0, 5, pred.shape, generator=g)
            y = torch.where(torch.rand(pred.shape, generator=g) < 0.66, pred, noise)
            y[0, :4, :4] = 255
            loader.append((x, y))
    return net, loader


def test_evaluate_equals_the_histogram_of_the_models_own_logits(C):
    net, loader = _tiny_model_and_loader()
    net.train()
    res = C.evaluate(net, loader, 5, torch.device("cuda"))
    assert net.training
    net.eval()
    hist = C.ReliabilityHistogram(5, 15, "cuda")
    with torch.no_grad():
        for x, y in loader:
            hist.update(net(x.cuda()), y.cuda())
    tab, cnt = hist.tables()
    assert np.array_equal(res["tables"], tab) and [res["counted"], res["void"], res["nonfinite"]] == cnt.tolist()
    assert res["void"] == 2 * 16 and res["counted"] == 2 * 2 * 64 * 64 - 32
    want = C.reliability_from_tables(tab)
    for k in C.OUT_KEYS + ("bin_count", "bin_accuracy", "bin_confidence", "bin_lower"):
        assert np.array_equal(res[k], want[k], equal_nan=True), k
    dev = hist.compute()
    np.testing.assert_allclose([res[k] for k in C.OUT_KEYS], dev["out"].cpu().numpy(), rtol=1e-12)
    # at a fitted temperature
    sc = C.TemperatureScaler("cuda").fit(net, loader, "cuda", iters=2)
    scaled = C.evaluate(net, loader, 5, "cuda", scaler=sc)
    assert scaled["counted"] == res["counted"] and scaled["accuracy"] == res["accuracy"]   # a temperature moves no winner


def test_fit_over_a_loader_and_state_dict(C):
    """``fit`` over a two-batch loader against ``fit_logits`` on the concatenated logits: the per-pixel terms are the same fp32
    numbers, but a pass over two batches adds them in another order than one call on the concatenation (other blocks, and the
    second call adds onto the first call's sum), so the float64 sums agree to rounding, not bit for bit; after each step's
    rounding to fp32 the betas may differ in the last place.  Held to 2^-22 relative, the NLL bar's floor."""
    net, loader = _tiny_model_and_loader()
    with torch.no_grad():
        logits = torch.cat([net(x.cuda()) for x, _ in loader])
    masks = torch.cat([y for _, y in loader]).cuda()
    a = C.TemperatureScaler("cuda").fit(net, loader, "cuda", iters=8)
    b = C.TemperatureScaler("cuda").fit_logits(logits, masks, iters=8)
    ra, rb = a.report(), b.report()
    print(f"calib-grade fit loader {ra['beta']!r} / concatenated {rb['beta']!r}, mean nll {ra['mean_nll']:.6f}")
    assert abs(ra["beta"] - rb["beta"]) <= FLOOR * rb["beta"] and ra["steps"] == rb["steps"] == 8
    assert ra["counted"] == rb["counted"] and ra["void"] == rb["void"] == 8 * 32
    assert 1.0 / 64 < ra["beta"] < 64 and ra["beta"] != 1.0
    assert torch.equal(a.scale(logits), logits * a.inv_temp)
    state = a.state_dict()
    assert all(not v.is_cuda for v in state.values())
    c = C.TemperatureScaler("cuda").load_state_dict(state)
    for k in a._STATE:
        assert torch.equal(getattr(c, k), getattr(a, k)), k
    assert c.report() == ra
    with pytest.raises(ValueError):
        c.load_state_dict({**state, "inv_temp": state["inv_temp"].double()})
    assert c.reset().report()["beta"] == 1.0
