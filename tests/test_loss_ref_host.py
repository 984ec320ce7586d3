"""tests/_loss_ref.py on the CPU: its float64 leg against torch's double-precision autograd of plainly written torch expressions
(and against oracle/losses_ref.py where a class exists) to 1e-12, then the grading of tests/test_gpu_loss_grade.py itself -- with
the float32 leg standing in for the kernels every case of the GPU file passes, and with each of the nine mutations of that leg at
least one case fails."""
import numpy as np
import pytest
import torch

import _loss_cases as C
import _loss_ref as R
from _loss_ref import F32, F64
from oracle import losses_ref as O

TOL = 1e-12


def close(got, want, what):
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max(initial=0.0))
    ref = float(np.abs(want).max(initial=0.0))
    assert err <= TOL * max(ref, 1e-300) or err == 0.0, f"{what}: {err:.3e} against {ref:.3e}"


def data(seed, batch=2, classes=5, ppi=12, scale=3.0):
    g = np.random.default_rng(seed)
    z = g.standard_normal((batch * ppi, classes)) * scale
    t = g.integers(0, classes, batch * ppi).astype(np.int64)
    return g, z, t


def leaf(z):
    return torch.from_numpy(np.array(z, dtype=F64)).requires_grad_(True)


def nchw(zt, batch):
    """[P, C] -> [B, C, P / B, 1] for the oracle classes."""
    p, c = zt.shape
    return zt.reshape(batch, p // batch, 1, c).permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------------------- float64 leg against torch autograd
@pytest.mark.parametrize("smooth", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("ignore_index", [None, 255, 0])
def test_dice_per_image(smooth, ignore_index):
    batch = 3
    g, z, t = data(1, batch, 5, 14)
    if ignore_index is not None:
        t[g.random(t.size) < 0.3] = ignore_index
        t[3] = 9                                                   # outside [0, C): void too
    t[:14][t[:14] == 4] = 1                                        # class 4 absent from image 0
    r = R.dice(z, t, batch, smooth, 1e-7, False, ignore_index, 0.37)
    zt = leaf(z)
    p = torch.softmax(zt, 1)
    tt = torch.from_numpy(t)
    live = (tt >= 0) & (tt < 5) & (tt != ignore_index) if ignore_index is not None else torch.ones_like(tt, dtype=torch.bool)
    oh = torch.zeros_like(p)
    oh[live, tt[live]] = 1.0
    pl = p * live[:, None]
    inter, union = (pl * oh).reshape(batch, 14, 5).sum(1), pl.reshape(batch, 14, 5).sum(1) + oh.reshape(batch, 14, 5).sum(1)
    loss = 1.0 - ((2 * inter + smooth) / (union + smooth)).mean()
    (loss * 0.37).backward()
    close(r["loss"][0], loss.item(), "dice value")
    close(r["grad"][0], zt.grad.numpy(), "dice gradient")
    assert not r["grad"][0][~live.numpy()].any()
    # coef: dLoss/dp_c = a [c == t] + b
    pp = leaf(torch.softmax(zt.detach(), 1).numpy())
    pl = pp * live[:, None]
    inter, union = (pl * oh).reshape(batch, 14, 5).sum(1), pl.reshape(batch, 14, 5).sum(1) + oh.reshape(batch, 14, 5).sum(1)
    (1.0 - ((2 * inter + smooth) / (union + smooth)).mean()).backward()
    coef = r["coef"][0]
    bi = np.arange(t.size) // 14
    want = (coef[bi, 1] + oh.numpy() * coef[bi, 0]) * live.numpy()[:, None]
    close(want, pp.grad.numpy(), "dice coef")
    if ignore_index is None:
        zo = leaf(z)
        lo = O.DiceLossRef(smooth)(nchw(zo, batch), torch.from_numpy(t).reshape(batch, 14, 1))
        (lo * 0.37).backward()
        close(r["loss"][0], lo.item(), "dice value against the oracle")
        close(r["grad"][0], zo.grad.numpy(), "dice gradient against the oracle")


@pytest.mark.parametrize("smooth,eps", [(0.0, 1e-7), (0.1, 1e-7), (1.0, 50.0), (0.0, 50.0)])
@pytest.mark.parametrize("ignore_index", [None, 255])
def test_dice_pooled(smooth, eps, ignore_index):
    """The formula quoted in csrc/losses_seg.hip: sums pooled over the batch, score_c = (2 I_c + s) / max(U_c + s, eps),
    loss = mean_c (1 - score_c) [class c present]."""
    batch = 2
    g, z, t = data(2, batch, 6, 11)
    t[t == 4] = 0                                                  # absent from the batch
    if ignore_index is not None:
        t[g.random(t.size) < 0.3] = ignore_index
    r = R.dice(z, t, batch, smooth, eps, True, ignore_index, 1.7)
    zt = leaf(z)
    p = torch.softmax(zt, 1)
    tt = torch.from_numpy(t)
    live = (tt >= 0) & (tt < 6) & (tt != ignore_index) if ignore_index is not None else torch.ones_like(tt, dtype=torch.bool)
    oh = torch.zeros_like(p)
    oh[live, tt[live]] = 1.0
    pl = p * live[:, None]
    inter, union, count = (pl * oh).sum(0), pl.sum(0) + oh.sum(0), oh.sum(0)
    score = (2 * inter + smooth) / (union + smooth).clamp_min(eps)
    loss = ((1.0 - score) * (count > 0)).sum() / 6
    (loss * 1.7).backward()
    assert (count == 0).any()
    close(r["loss"][0], loss.item(), "pooled dice value")
    close(r["grad"][0], zt.grad.numpy(), "pooled dice gradient")


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 3.0])
@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("ignore_index", [None, -100])
def test_focal(gamma, mean, ignore_index):
    g, z, t = data(3, 2, 7, 9)
    w = g.random(7) + 0.5
    w[3] = 0.0
    if ignore_index is not None:
        t[g.random(t.size) < 0.3] = ignore_index
    r = R.focal(z, t, w, 0.25, gamma, mean, ignore_index, 0.37)
    zt = leaf(z)
    tt = torch.from_numpy(t)
    live = tt != ignore_index if ignore_index is not None else torch.ones_like(tt, dtype=torch.bool)
    ts = torch.where(live, tt, torch.zeros_like(tt))
    ce = torch.nn.functional.cross_entropy(zt, ts, torch.from_numpy(w), reduction="none") * live
    f = 0.25 * (1 - torch.exp(-ce)) ** gamma * ce
    loss = f.mean() if mean else f.sum()
    # R.focal's scale is everything the gradient is multiplied by: the caller's 1 / pixels is part of it for 'mean'
    (loss * 0.37 * (t.size if mean else 1.0)).backward()
    close(r["loss"][0], loss.item(), "focal value")
    keep = (ce.detach().numpy() > 0) | (gamma >= 1.0) | (gamma == 0.0)    # ce = 0 (w_t = 0, void) and 0 < gamma < 1: 0 x inf in autograd
    close(r["grad"][0][keep], zt.grad.numpy()[keep], "focal gradient")
    assert np.isfinite(r["grad"][0]).all() and not r["grad"][0][~live.numpy()].any()
    if ignore_index is None:
        zo = leaf(z)
        lo = O.WeightedSegmentationLossRef(7, torch.from_numpy(w), 0.25, gamma, "mean" if mean else "sum").focal_loss(
            nchw(zo, 2), torch.from_numpy(t).reshape(2, 9, 1))
        (lo * 0.37 * (t.size if mean else 1.0)).backward()
        close(r["loss"][0], lo.item(), "focal value against the oracle")
        close(r["grad"][0][keep], zo.grad.numpy()[keep], "focal gradient against the oracle")


def test_focal_plus_dice_against_the_oracle():
    """WeightedSegmentationLossRef: domain_weight x (focal + Dice with smooth 1), the sum losses.py forms from the two kernels."""
    g, z, t = data(8, 2, 7, 9)
    w = g.random(7) + 0.5
    f = R.focal(z, t, w, 0.25, 2.0, True, None, 0.7 / t.size)
    d = R.dice(z, t, 2, 1.0, 1e-7, False, None, 0.7)
    zo = leaf(z)
    lo = O.WeightedSegmentationLossRef(7, torch.from_numpy(w))(nchw(zo, 2), torch.from_numpy(t).reshape(2, 9, 1), 0.7)
    lo.backward()
    close(0.7 * (f["loss"][0] + d["loss"][0]), lo.item(), "focal + dice value")
    close(f["grad"][0] + d["grad"][0], zo.grad.numpy(), "focal + dice gradient")


def test_focal_rule_where_one_minus_pt_is_zero():
    """om == 0: the derivative is alpha for gamma == 0 and 0 otherwise."""
    z = np.array([[0.0, 40.0, 0.0]])                               # 1 + 2 exp(-40) rounds to 1 in float64: ce = 0, pt = 1
    t = np.array([1])
    for gamma, want in ((0.0, 0.25), (0.5, 0.0), (2.0, 0.0)):
        g = R.focal(z, t, None, 0.25, gamma, False, None, 1.0)["grad"][0][0]
        assert g[0] == want * np.exp(-40.0) and g[0] == g[2] and g[1] == 0.0
    assert R.focal(np.array([[0.0, 3.0, 0.0]]), t, None, 0.25, 0.0, False, None, 1.0)["grad"][0][0, 1] < 0


@pytest.mark.parametrize("temperature", [0.5, 0.7, 1.0, 2.0])
def test_consistency(temperature):
    g, z1, _ = data(4, 2, 6, 10)
    z2 = z1 + g.standard_normal(z1.shape)
    r = R.consistency(z1, z2, 1.0 / temperature, 2, 0.37)
    a, b = leaf(z1), leaf(z2)
    loss = O.ConsistencyLossRef(temperature)(nchw(a, 2), nchw(b, 2))
    (loss * 0.37).backward()
    close(r["loss"][0], loss.item(), "consistency value against the oracle")
    close(r["d1"][0], a.grad.numpy(), "consistency d1")
    close(r["d2"][0], b.grad.numpy(), "consistency d2")
    a, b = leaf(z1), leaf(z2)
    l1, l2 = torch.log_softmax(a / temperature, 1), torch.log_softmax(b / temperature, 1)
    kl = torch.nn.functional.kl_div
    loss = (kl(l1.reshape(2, -1), l2.exp().reshape(2, -1), reduction="batchmean")
            + kl(l2.reshape(2, -1), l1.exp().reshape(2, -1), reduction="batchmean")) / 2
    close(r["loss"][0], loss.item(), "consistency value")
    same = R.consistency(z1, z1, 1.0 / temperature, 2, 0.37)
    assert same["loss"][0] == 0 and not same["d1"][0].any() and not same["d2"][0].any()


def test_cross_entropy():
    g, z, t = data(5, 1, 11, 300)
    r = R.cross_entropy(z, t, 0.37)
    zt = leaf(z)
    loss = torch.nn.functional.cross_entropy(zt, torch.from_numpy(t))
    (loss * 0.37).backward()
    close(r["loss"][0], loss.item(), "ce value")
    close(r["lse"][0], torch.logsumexp(zt.detach(), 1).numpy(), "ce lse")
    close(r["grad"][0], zt.grad.numpy(), "ce gradient")
    assert np.abs(r["colsum"][0] - zt.grad.numpy().sum(0)).max() <= 1e-12 * r["colsum"][1].max()


@pytest.mark.parametrize("sigmoid", [True, False])
def test_discriminator_tail(sigmoid):
    g = np.random.default_rng(6)
    n, hw, c = 3, 33, 8
    z, w, b, dp = g.standard_normal((n, hw, c)), g.standard_normal(c), g.standard_normal(1), g.standard_normal(n)
    f = R.tail_forward(z, w, b, sigmoid)
    zt, wt, bt = leaf(z), leaf(w), leaf(b)
    pooled = zt.mean(1)
    out = pooled @ wt + bt
    out = torch.sigmoid(out) if sigmoid else out
    out.backward(torch.from_numpy(dp))
    close(f["pooled"][0], pooled.detach().numpy(), "pooled")
    close(f["out"][0], out.detach().numpy(), "tail output")
    bw = R.tail_backward(dp, f["out"][0], f["pooled"][0], w, hw, sigmoid)
    close(np.repeat(bw["dz"][0][:, None], hw, 1), zt.grad.numpy(), "tail dz")
    close(bw["dw"][0], wt.grad.numpy(), "tail dw")
    close(bw["db"][0], bt.grad.numpy()[0], "tail db")


@pytest.mark.parametrize("vector", [False, True])
def test_bce(vector):
    g = np.random.default_rng(7)
    x = g.standard_normal(13) * 4
    y = g.random(13) if vector else 1.0
    r = R.bce(x, y, 0.6, 0.37)
    xt = leaf(x)
    yt = torch.from_numpy(np.broadcast_to(np.asarray(y, dtype=F64), x.shape).copy())
    loss = 0.6 * torch.nn.functional.binary_cross_entropy_with_logits(xt, yt)
    (loss * 0.37).backward()
    close(r["loss"][0], loss.item(), "bce value")
    close(r["dx"][0], xt.grad.numpy(), "bce gradient")


# ---------------------------------------------------------------------------------------------------------- the grading itself
def test_grader_verdicts():
    log = []
    r64 = np.array([1.0, -2.0, 1e-3])
    mag = np.array([1.0, 2.0, 4.0])
    r32 = r64 + np.array([1e-7, 0.0, 0.0]) * mag                    # d = 1e-7: below the floor / 4, the bar is 2^-22
    G = R.Grader("t", log.append)
    G.grade("at the bar", r64 + 2.0 ** -22 * mag, r64, r32, mag)
    assert not G.bad
    G.grade("small element", r64 + np.array([0, 0, 1e-6]) * mag, r64, r32, mag)    # small next to its neighbours, judged by its own magnitude
    assert len(G.bad) == 1
    G.grade("nan", np.array([1.0, np.nan, 1e-3]), r64, r32, mag)
    G.grade("leg sets the bar", r64 + 3e-6 * mag, r64, r64 + 1e-6 * mag, mag)
    assert len(G.bad) == 2
    G.zero("zeros", np.array([0.0, -0.0]))
    G.zero("not zeros", np.array([0.0, 1e-45]))
    G.exact("nan is not exact", np.array([np.nan]), np.array([np.nan]))
    G.within_ulp("fused add", np.float32(1.0) + np.spacing(np.float32(1.0)), np.float32(0.5), np.float32(0.5))
    G.within_ulp("two ulp", np.float32(1.0) + 2 * np.spacing(np.float32(1.0)), np.float32(0.5), np.float32(0.5))
    assert len(G.bad) == 5 and len(log) == 9
    with pytest.raises(AssertionError):
        G.done()


def test_the_shapes_reach_every_launch_regime():
    """The cases name the smallest size at which each path exists; this pins that they do."""
    assert [C.grid_pix(p) for p in (1, 255, 256, 257)] == [1, 1, 1, 2]                       # tail block
    assert C.grid_pix(262_656) == 1024 and C.passes(262_656) == 2 and 262_656 == 513 * 512 == 1026 * 256
    assert C.grid_pix(65_792, 256) == 256 and C.passes(65_792, 256) == 2 and 65_792 == 257 * 256   # dice_stats: gridDim.x <= 256
    assert C.straddling_blocks(3, 35) == [0] and C.straddling_blocks(2, 272) == [1] and C.straddling_blocks(2, 65_792) == []
    assert [c["ldc"] for c in C.TEMPLATE_SHAPES[:8]] == [4, 8, 12, 16, 20, 24, 28, 32]
    assert all(c["classes"] == c["ldc"] - 1 and (c["batch"], c["ppi"]) == (3, 35) for c in C.TEMPLATE_SHAPES[:8])
    assert [(c["classes"], c["ldc"]) for c in C.TEMPLATE_SHAPES[8:]] == [(4, 4), (32, 32), (1, 4)]
    assert C.ce_row_groups(24) == (10, 240) and C.ce_row_groups(12) == (21, 252)
    assert sorted({c["ldc"] for c in C.CE_CASES}) == [12, 24, 40, 64] and {c["pixels"] for c in C.CE_CASES} == {257, 262_656}
    assert C.grid_pix(262_656, 4096) == 1026                                                # ce_bwd_simple: one pass
    assert R.gap_slices(1) == (1, 1, 1) and R.gap_slices(24) == (24, 1, 24) and R.gap_slices(32) == (32, 1, 32)
    assert R.gap_slices(33) == (32, 2, 17) and R.gap_slices(4096) == (32, 128, 32)          # at 33 the last 15 slices are empty
    tails = {(c["n"], c["hw"], c["c"]) for c in C.TAIL_CASES}
    assert {hw for _, hw, _ in tails} == {1, 24, 32, 33, 4096} and {c for _, _, c in tails} == {4, 512, 1028}
    assert {n for n, _, _ in tails} == {1, 3} and 1028 // 4 > 256
    assert [c["n"] for c in C.BCE_CASES] == [1, 4, 64, 65, 300]


ALL_CASES = [(name, c) for name, (cases, _, _) in C.FAMILIES.items() for c in cases]
ALL_IDS = [f"{name}-{C.FAMILIES[name][1](c)}" for name, c in ALL_CASES]
LOG = []


@pytest.mark.parametrize("name,case", ALL_CASES, ids=ALL_IDS)
def test_float32_leg_passes_every_case(name, case):
    """Also the assertion the GPU file makes before any launch: across focal's om > 0 branch the float32 leg meets the bar."""
    G = C.FAMILIES[name][2](C.LegBackend(), case, LOG.append)
    assert G.worst <= 0.25 + 1e-12                    # e == d and bar >= 4 d


MUTATION_FAMILIES = {"dice_divisor": ["dice_edge"], "absent_counted": ["dice_edge"], "focal_no_pt": ["focal_edge"],
                     "consistency_no_inv_t": ["consistency_edge"], "pad_lane": ["launch"], "colsum_tail": ["ce"],
                     "straddle": ["launch", "seg_accumulate"], "bce_wrong_n": ["bce"], "dw_overwrite": ["tail"]}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutation_fails_some_case(mut):
    assert set(MUTATION_FAMILIES) == set(R.MUTATIONS)
    failed = []
    for name in MUTATION_FAMILIES[mut]:
        cases, ident, run = C.FAMILIES[name]
        for c in cases:
            if c.get("size") == C.BIG:
                continue
            try:
                run(C.LegBackend(mut), c, LOG.append)
            except AssertionError as e:
                failed.append((ident(c), str(e)))
    assert failed, f"no case notices the mutation {mut}"
    print(f"{mut}: {len(failed)} cases fail, first: {failed[0][0]}: {failed[0][1][:200]}")
