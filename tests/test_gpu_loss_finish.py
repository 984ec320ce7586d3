"""The reduction order of the scalar-loss kernels (csrc/loss_reduce.h, csrc/loss_reduce.hip), pinned without a second build.

Every entry point that takes a caller-owned ``partials`` buffer leaves the block partials in it, so the last stage of its
reduction can be restated on the host and compared BIT FOR BIT (``torch.equal``; the order is defined and IEEE addition is
commutative, so there is nothing to tolerate):

  loss     float32(S / D); S = the f64 sum of the n partials in the finish kernel's order: lane l of 64 adds partials[l],
           partials[l + 64], ... from 0.0, then six xor-butterfly steps with offsets 32 ... 1 (v = v + v[idx ^ o]); D = the
           entry point's divisor (pixels, 2 * batch, -2 * pixels, the device denominator, or 1).  D == 0 on the device: NaN.
  colsum   fp32, per column: thread t of 256 adds colsum_partials[t][c], [t + 256][c], ..., a butterfly per wave of 64, then
           (r0 + r1) + (r2 + r3).
  denom and counters of udaseg_ce_target_stats / udaseg_pixel_weight_sum: the loss tree over each row of their [k][n] partials;
           row 0 is the f64 denominator, the others whole numbers cast to int64.

Sizes: 1 x 23 x 136 x 136 (ldc 24): 18 496 pixels, 73 blocks -- more than one stride of the 64-lane loop, the last block ragged
at 64 pixels; 1 x 5 x 15 x 20 (ldc 8): 300 pixels, 2 blocks, fewer partials than lanes.  The partials buffers are pre-filled with
NaN: the entries past the n the test computes must still be NaN, so the test and the launch agree on n.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"136x136x23": (23, 24, 136 * 136), "15x20x5": (5, 8, 15 * 20)}     # classes, ldc, pixels (batch 1)
DIM, LDF = 8, 12                                                            # the prototype losses' feature rows
LANE = np.arange(64)


def butterfly(v):
    """wave_sum / wave_sum_d: lane 0 after v += shfl_xor(v, o) for o = 32 ... 1, in v's dtype."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[LANE ^ o]
    return v[0]


def strided(x, lanes):
    """Thread t of ``lanes`` adds x[t], x[t + lanes], ... in that order from 0 (a trailing +0.0 changes no bits), in x's dtype."""
    pad = (-len(x)) % lanes
    rows = np.concatenate([x, np.zeros(pad, x.dtype)]).reshape(-1, lanes)
    acc = np.zeros(lanes, x.dtype)
    for r in rows:
        acc = acc + r
    return acc


def finish_sum(partials):
    return butterfly(strided(np.asarray(partials, np.float64), 64))


def expect_loss(partials, n, divisor):
    """float32(S / D) from the first n partials; the rest of the buffer must be untouched."""
    p = partials.cpu().numpy()
    assert np.isnan(p[n:]).all() and not np.isnan(p[:n]).any(), "the launch wrote another number of partials than the test expects"
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(finish_sum(p[:n]) / np.float64(divisor))


def expect_colsum(colpart, n, ldc):
    p = colpart.cpu().numpy().reshape(-1, ldc)
    assert np.isnan(p[n:]).all() and not np.isnan(p[:n]).any()
    out = np.empty(ldc, np.float32)
    for c in range(ldc):
        r = [butterfly(w) for w in strided(np.ascontiguousarray(p[:n, c]), 256).reshape(4, 64)]
        out[c] = (r[0] + r[1]) + (r[2] + r[3])
    return out


def same_bits(got, want):
    want = torch.from_numpy(np.asarray(want).reshape(-1))
    got = got.detach().cpu().reshape(-1)
    assert got.dtype == want.dtype
    assert torch.equal(got, want), (got.tolist(), want.tolist())


def nans(n, dtype=torch.float32):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


class Case:
    """The inputs of one shape, made once and left unchanged."""
    def __init__(self, classes, ldc, pixels):
        from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K
        _lib.require_gpu()
        self.K, self.classes, self.ldc, self.pixels = K, classes, ldc, pixels
        self.n = min((pixels + 255) // 256, 1024)
        assert K.seg_partials() == 1024 and _lib.load().udaseg_ce_partials() == 1024
        g = torch.Generator().manual_seed(1000 * classes + pixels)
        rows = lambda w, scale=3.0: (scale * torch.randn(pixels, w, generator=g)).cuda()       # noqa: E731
        self.z, self.z2 = rows(ldc), rows(ldc)
        self.target = torch.randint(0, classes, (pixels,), generator=g).cuda()
        self.void_target = self.target.clone()
        self.void_target[::7] = 255
        self.cw = (0.5 + torch.rand(classes, generator=g)).cuda()
        self.wpx = torch.rand(pixels, generator=g).cuda()
        self.wpx[::11] = 0.0
        self.wpx[5::13] = -1.0
        self.wimg = torch.tensor([0.75]).cuda()
        self.teacher = torch.softmax(rows(ldc)[:, :classes], 1)
        self.teacher = torch.nn.functional.pad(self.teacher, (0, ldc - classes)).contiguous()
        self.feat = rows(LDF, 1.0)
        self.labels = self.target.to(torch.uint8)
        self.proto = torch.randn(classes * DIM, generator=g, dtype=torch.float64).cuda()
        self.seen = torch.ones(classes, dtype=torch.int32).cuda()
        self.seen[classes - 1] = 0
        self.inv_tau = torch.tensor([0.5]).cuda()

    def partials(self, rows=1):
        return nans(rows * 1024, torch.float64)

    def colbufs(self):
        return nans(1024 * self.ldc), nans(self.ldc)

    def target_stats(self, target, weight, ignore_index):
        parts, denom = self.partials(4), nans(1, torch.float64)
        stats = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        self.K.ce_target_stats(target, weight, self.pixels, self.classes, ignore_index, parts, denom, stats)
        return parts, denom, stats

    def weight_sum(self, wpx, wimg):
        parts, denom = self.partials(3), nans(1, torch.float64)
        counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        self.K.pixel_weight_sum(wpx, wimg, 1, self.pixels, parts, denom, counts)
        return parts, denom, counts


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request):
    return Case(*SHAPES[request.param])


def expect_rows(parts, n, rows):
    p = parts.cpu().numpy()
    assert np.isnan(p[rows * n:]).all() and not np.isnan(p[:rows * n]).any()
    s = [finish_sum(p[k * n:(k + 1) * n]) for k in range(rows)]
    return np.float64(s[0]), np.array(s[1:]).astype(np.int64)


def test_plain_cross_entropy(case):
    K, c = case.K, case
    lse, parts, loss = nans(c.pixels), c.partials(), nans(1)
    K.ce_fwd(c.z, c.target, c.pixels, c.classes, c.ldc, lse, parts, loss)
    same_bits(loss, expect_loss(parts, c.n, c.pixels))

    parts2, loss2, d = c.partials(), nans(1), nans(c.pixels * c.ldc)
    colpart, colsum = c.colbufs()
    K.ce_fwd_bwd(c.z, c.target, c.pixels, c.classes, c.ldc, parts2, loss2, d, colpart, colsum)
    same_bits(loss2, expect_loss(parts2, c.n, c.pixels))
    same_bits(colsum, expect_colsum(colpart, c.n, c.ldc))
    assert torch.equal(parts2[:c.n], parts[:c.n]) and torch.equal(loss2, loss)           # one pass and two passes: the same bits

    colpart, colsum = c.colbufs()
    K.ce_bwd(c.z, c.target, lse, None, c.pixels, c.classes, c.ldc, d, colpart, colsum)
    same_bits(colsum, expect_colsum(colpart, c.n, c.ldc))


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_optioned_cross_entropy(case, eps, mean):
    K, c = case.K, case
    sparts, denom, stats = c.target_stats(c.void_target, c.cw, 255)
    want_denom, want_stats = expect_rows(sparts, c.n, 4)
    same_bits(denom, want_denom)
    same_bits(stats, want_stats)
    assert int(stats.sum()) == c.pixels and int(stats[1]) == len(range(0, c.pixels, 7))
    divisor = denom.item() if mean else 1.0

    parts, loss, d = c.partials(), nans(1), nans(c.pixels * c.ldc)
    colpart, colsum = c.colbufs()
    K.ce_opt_fwd_bwd(c.z, c.void_target, c.cw, c.pixels, c.classes, c.ldc, 255, eps, mean, denom, parts, loss, d, colpart, colsum)
    same_bits(loss, expect_loss(parts, c.n, divisor))
    same_bits(colsum, expect_colsum(colpart, c.n, c.ldc))

    lse, parts2, loss2 = nans(c.pixels), c.partials(), nans(1)
    K.ce_opt_fwd(c.z, c.void_target, c.cw, c.pixels, c.classes, c.ldc, 255, eps, mean, denom, lse, parts2, loss2)
    same_bits(loss2, expect_loss(parts2, c.n, divisor))
    assert torch.equal(parts2[:c.n], parts[:c.n]) and torch.equal(loss2, loss)

    colpart, colsum = c.colbufs()
    K.ce_opt_bwd(c.z, c.void_target, c.cw, lse, None, None, c.pixels, c.classes, c.ldc, 255, eps, mean, denom, d, colpart, colsum)
    same_bits(colsum, expect_colsum(colpart, c.n, c.ldc))


def test_all_void_mean_is_nan(case):
    K, c = case.K, case
    target = torch.full_like(c.target, 255)
    sparts, denom, stats = c.target_stats(target, None, 255)
    assert denom.item() == 0.0 and stats.tolist() == [0, c.pixels, 0]
    parts, loss, d = c.partials(), nans(1), nans(c.pixels * c.ldc)
    K.ce_opt_fwd_bwd(c.z, target, None, c.pixels, c.classes, c.ldc, 255, 0.0, True, denom, parts, loss, d)
    want = expect_loss(parts, c.n, 0.0)
    assert np.isnan(want) and torch.isnan(loss).all()


@pytest.mark.parametrize("ignore_index", [None, 255])
@pytest.mark.parametrize("mean", [True, False])
def test_focal(case, mean, ignore_index):
    K, c = case.K, case
    target = c.target if ignore_index is None else c.void_target
    parts, loss = c.partials(), nans(1)
    K.focal_fwd(c.z, target, c.cw, 0.25, 2.0, c.pixels, c.classes, c.ldc, mean, parts, loss, ignore_index=ignore_index)
    want = expect_loss(parts, c.n, c.pixels if mean else 1.0)
    same_bits(loss, want)
    acc = torch.tensor([0.5], device="cuda")
    K.focal_fwd(c.z, target, c.cw, 0.25, 2.0, c.pixels, c.classes, c.ldc, mean, c.partials(), acc, accumulate=True,
                ignore_index=ignore_index)
    same_bits(acc, np.float32(0.5) + want)


def test_consistency(case):
    K, c = case.K, case
    parts, loss = c.partials(), nans(1)
    K.consistency_fwd(c.z, c.z2, 0.7, 3, c.pixels, c.classes, c.ldc, parts, loss)
    same_bits(loss, expect_loss(parts, c.n, 2.0 * 3))


@pytest.mark.parametrize("kind,sign", [("entropy", 1.0), ("max_squares", -2.0)])
def test_entropy_loss(case, kind, sign):
    K, c = case.K, case
    parts, loss = c.partials(), nans(1)
    K.entropy_loss(c.z, c.pixels, c.classes, c.ldc, kind, parts, loss, nans(c.pixels * c.ldc))
    same_bits(loss, expect_loss(parts, c.n, sign * c.pixels))


@pytest.mark.parametrize("reduction", ["mean", "denom", "sum"])
@pytest.mark.parametrize("kind,probs", [("ce", 0), ("kl", 1), ("symmetric", 1)])
def test_soft_cross_entropy(case, kind, probs, reduction):
    K, c = case.K, case
    wparts, denom, counts = c.weight_sum(c.wpx, c.wimg)
    want_denom, want_counts = expect_rows(wparts, c.n, 3)
    same_bits(denom, want_denom)
    same_bits(counts, want_counts)
    assert counts.tolist() == [int((c.wpx == 0).sum()), int((c.wpx < 0).sum())]
    parts, loss, d = c.partials(), nans(1), nans(c.pixels * c.ldc)
    colpart, colsum = c.colbufs()
    teacher = c.teacher if probs else c.z2
    K.soft_ce_fwd_bwd(c.z, teacher, c.wpx, c.wimg, 1, c.pixels, c.classes, c.ldc, c.ldc, probs, kind, 0.5, 1.0, 0.5, -4.0,
                      reduction == "mean", denom if reduction == "denom" else None, parts, loss, d, colpart, colsum)
    divisor = {"mean": c.pixels, "denom": denom.item(), "sum": 1.0}[reduction]
    same_bits(loss, expect_loss(parts, c.n, divisor))
    same_bits(colsum, expect_colsum(colpart, c.n, c.ldc))


@pytest.mark.parametrize("reduction", ["mean", "denom", "sum"])
@pytest.mark.parametrize("soft", [False, True])
def test_prototype_contrast(case, soft, reduction):
    K, c = case.K, case
    _, denom, _ = c.weight_sum(c.wpx, None)
    parts, loss = c.partials(), nans(1)
    K.proto_contrast_fwd_bwd(c.feat, LDF, DIM, None if soft else c.labels, c.teacher if soft else None, c.ldc if soft else 0, c.wpx,
                             None, 1, c.pixels, c.classes, c.proto, c.seen, c.inv_tau, reduction == "mean",
                             denom if reduction == "denom" else None, parts, loss, nans(c.pixels * LDF))
    divisor = {"mean": c.pixels, "denom": denom.item(), "sum": 1.0}[reduction]
    want = expect_loss(parts, c.n, divisor)
    assert np.isfinite(want) and want != 0
    same_bits(loss, want)
