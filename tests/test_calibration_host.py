"""CPU checks of the calibration module: the float64 leg of the mirror (tests/_calib_ref.py) against torch's double-precision
autograd, the guarded Newton step on hand-made sums, the fit trajectories, ``reliability_from_tables`` on a hand-made table, the
error convention of the four entry points and the "no CPU path" errors.  No GPU."""
import numpy as np
import pytest
import torch

import _calib_ref as R


def test_derivatives_of_the_float64_leg_equal_double_precision_autograd():
    z, t = R.flat(*R.case("c23"))
    for beta0 in (1.0, 0.36, 2.5):
        sums, mags, counters = R.nll_sums(z, t, beta0)
        valid = (t >= 0) & (t < z.shape[1])
        assert counters.tolist() == [int(valid.sum()), int((~valid).sum()), 0] and counters[1] == 50
        zt, tt = torch.from_numpy(z[valid]).double(), torch.from_numpy(t[valid])
        beta = torch.tensor(beta0, dtype=torch.float64, requires_grad=True)
        nll = torch.nn.functional.cross_entropy(zt * beta, tt, reduction="sum")
        g1, = torch.autograd.grad(nll, beta, create_graph=True)
        g2, = torch.autograd.grad(g1, beta)
        for got, want, mag in ((sums[1], nll.item(), mags[1]), (sums[2], g1.item(), mags[2]), (sums[3], g2.item(), mags[3])):
            assert abs(got - want) <= 1e-12 * mag, (beta0, got, want)
        assert sums[3] > 0 and np.all(mags[1:] >= np.abs(sums[1:]))
        # the float32 leg is the same arithmetic: close to the float64 leg relative to the magnitudes, never equal by contract
        s32, _, c32 = R.nll_sums(z, t, beta0, R.F32)
        assert np.array_equal(c32, counters)
        dev = np.abs(s32[1:] - sums[1:]) / mags[1:]
        print(f"beta {beta0}: fp32 leg deviation / magnitude {dev}")
        assert np.all(dev < 1e-6)


def test_step_rule_on_hand_made_sums():
    # the raw Newton step 1 - 3.74 / 1 = -2.74 is clamped to beta / 4
    b, state = R.step([100.0, 50.0, 3.74, 1.0], 1.0)
    assert b == 0.25 and state.tolist() == [0.5, 3.74 / 100.0, -0.75, 1.0]
    assert R.step([100.0, 50.0, -90.0, 1.0], 1.0)[0] == 4.0                  # and to 4 beta on the other side
    assert R.step([100.0, 50.0, 1.0, 1e-3], 1.0 / 32.0)[0] == 1.0 / 64.0     # then to [1 / 64, 64]
    assert R.step([100.0, 50.0, -1.0, 1e-3], 32.0)[0] == 64.0
    b, _ = R.step([100.0, 50.0, 0.5, 4.0], 1.0)                              # an ordinary step, rounded to fp32 once
    assert b == float(np.float32(1.0 - 0.5 / 4.0))
    b, _ = R.step([10.0, 5.0, 1.0, 3.0], 0.7)
    beta = float(np.float32(0.7))
    assert b == float(np.float32(beta - 1.0 / 3.0)) and R.step([10.0, 5.0, 1.0, 3.0], 0.7, R.F64)[0] == 0.7 - 1.0 / 3.0
    for sums in ([0.0, 0.0, 0.0, 0.0], [100.0, 50.0, 3.0, 0.0], [100.0, 50.0, 3.0, -1.0], [100.0, float("nan"), 3.0, 1.0],
                 [100.0, 50.0, float("nan"), 1.0], [100.0, 50.0, 3.0, float("inf")], [float("nan"), 50.0, 3.0, 1.0]):
        b, state = R.step(sums, 0.7)
        assert b == beta and state[2] == 0.0, sums
    assert np.isnan(R.step([0.0, 0.0, 0.0, 0.0], 1.0)[1][:2]).all()
    assert np.isnan(R.step([100.0, 50.0, 1.0, 1.0], float("nan"))[0])        # a beta that is no positive number stays as it is
    assert R.step([100.0, 50.0, 1.0, 1.0], 0.0)[0] == 0.0 and R.step([100.0, 50.0, 1.0, 1.0], -1.0)[0] == -1.0


def test_fit_trajectories_and_ece_before_and_after():
    """Found on the CPU with this seed: beta converges to 1.067259 (plain), 0.355753 (logits x 3), 4.269036 (x 0.25) within 7 steps,
    the first step of the x 3 input clamped: its raw Newton step from beta = 1 is negative; its 15-bin ECE falls 0.145 -> 0.042."""
    z, t = R.flat(*R.case("c23"))
    want = {1.0: 1.067259, 3.0: 1.067259 / 3.0, 0.25: 1.067259 * 4.0}
    for s, beta_star in want.items():
        zs = z * np.float32(s)
        t64, t32 = R.fit(zs, t, 8), R.fit(zs, t, 8, R.F32)
        print(f"x {s}: float64 trajectory {t64}, float32 leg ends at {t32[-1]!r}")
        assert abs(t64[-1] - beta_star) <= 2e-6 * beta_star and abs(t64[-1] - t64[-2]) <= 1e-9 * beta_star
        assert abs(t32[-1] - t64[-1]) <= 1e-5 * t64[-1]
        if s == 3.0:
            sums, _, _ = R.nll_sums(zs, t, 1.0)
            assert 1.0 - sums[2] / sums[3] < 0 and t64[1] == 0.25                  # the relative clamp is needed
            before, after = (R.finish(R.tables(zs, t, 15, b)[0])[0] for b in (1.0, t64[-1]))
            print(f"x 3: ece {before[3]:.4f} -> {after[3]:.4f}, gap {before[5]:.4f} -> {after[5]:.4f}")
            assert before[5] > 0 and after[3] < 0.5 * before[3]
        if s == 0.25:
            assert all(b > a for a, b in zip(t64[:7], t64[1:8]))                    # unclamped here, and rising step by step


def test_mirror_tables_and_the_edge_allowance():
    """The fp32 leg against the float64 leg on the three GPU cases: few confidences lie within 1e-5 of an edge, so the per-edge
    allowance of the GPU test cannot swallow a wrong kernel."""
    for name in R.CASES:
        z, t = R.flat(*R.case(name))
        c = z.shape[1]
        for bins in (15, 64):
            for beta in (0.5, 1.0, 2.0):
                t64, c64, i64 = R.tables(z, t, bins, beta)
                t32, c32, i32 = R.tables(z, t, bins, beta, R.F32)
                assert np.array_equal(c64, c32) and c64[0] + c64[1] == len(t) and c64[2] == 0
                assert np.array_equal(t64[0].sum(1), t32[0].sum(1)) and np.array_equal(t64[1].sum(1), t32[1].sum(1))
                near = R.near_edge_counts(i64["p"][i64["used"]], i64["cls"][i64["used"]], c, bins, 1e-5)
                assert near.sum() < 0.02 * c64[0]
                cum = lambda x: np.cumsum(x[:, ::-1], axis=1)[:, ::-1]
                assert np.all(np.abs(cum(t64[0]) - cum(t32[0])) <= near)
                assert np.abs(i64["p"] - i32["p"].astype(np.float64)).max() < 2e-6
                out, pc = R.finish(t64)
                assert out[0] == c64[0] and abs(out[5] - (out[2] - out[1])) == 0 and 0 <= out[3] <= out[4] <= 1
                assert np.nansum(pc[0] * pc[3]) / out[0] >= out[3] - 1e-12           # the class-wise ECE is no smaller
    # at beta = 1 the confidence of the winner is the softmax's
    z, t = R.flat(*R.case("c5"))
    cls, p, fin = R.confidence(z)
    sm = torch.softmax(torch.from_numpy(z).double(), 1).numpy()
    assert fin.all() and np.array_equal(cls, sm.argmax(1)) and np.abs(p - sm.max(1)).max() < 1e-14


def test_reliability_from_tables_on_a_hand_made_table():
    from uda_aerial_semantic_segmentation_research_amd.calibration import reliability_from_tables
    q = lambda v: int(round(v * 2 ** 24))
    tab = np.zeros((3, 3, 4), dtype=np.int64)                              # 3 classes, 4 bins; bin 1 and class 2 stay empty
    tab[:, 0, 3] = 10, 7, 10 * q(0.875)                                    # class 0: ten pixels at 0.875, seven right
    tab[:, 0, 2] = 4, 1, 4 * q(0.625)
    tab[:, 1, 3] = 6, 6, 6 * q(1.0)
    tab[:, 1, 0] = 5, 0, 5 * q(0.125)
    r = reliability_from_tables(tab)
    assert r["n"] == 25.0 and r["accuracy"] == 14 / 25 and r["mean_conf"] == (8.75 + 2.5 + 6 + 0.625) / 25
    ece = (abs(0 - 0.625) + abs(1 - 2.5) + abs(13 - 14.75)) / 25
    assert abs(r["ece"] - ece) < 1e-15 and abs(r["gap"] - (r["mean_conf"] - r["accuracy"])) < 1e-15
    assert abs(r["mce"] - max(0.125, 0.625 - 0.25, 14.75 / 16 - 13 / 16)) < 1e-15
    assert r["bin_lower"].tolist() == [0.0, 0.25, 0.5, 0.75] and r["bin_count"].tolist() == [5, 0, 4, 16]
    assert np.isnan(r["bin_accuracy"][1]) and np.isnan(r["bin_confidence"][1]) and r["bin_accuracy"][3] == 13 / 16
    pc = r["per_class"]
    assert pc["n"].tolist() == [14.0, 11.0, 0.0] and pc["accuracy"][0] == 8 / 14 and pc["accuracy"][1] == 6 / 11
    assert all(np.isnan(pc[k][2]) for k in ("accuracy", "mean_conf", "ece"))
    assert abs(pc["ece"][0] - (abs(7 - 8.75) + abs(1 - 2.5)) / 14) < 1e-15 and abs(pc["ece"][1] - 0.625 / 11) < 1e-15
    out, mpc = R.finish(tab)                                               # the mirror's finish agrees
    assert np.allclose(out, [r[k] for k in ("n", "accuracy", "mean_conf", "ece", "mce", "gap")], rtol=1e-15, atol=0)
    assert np.allclose(mpc, [pc[k] for k in ("n", "accuracy", "mean_conf", "ece")], rtol=1e-15, atol=0, equal_nan=True)
    empty = reliability_from_tables(torch.zeros(3, 2, 5, dtype=torch.int64))
    assert empty["n"] == 0.0 and all(np.isnan(empty[k]) for k in ("accuracy", "mean_conf", "ece", "mce", "gap"))
    with pytest.raises(ValueError):
        reliability_from_tables(np.zeros((2, 3, 4)))


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    P = 4096                                                              # a non-NULL, aligned address; nothing is launched
    good = dict(scores=P, target=P, pixels=100, classes=23, ldc=24, probs=0, inv_temp=None, bins=15, tables=P, counters=P)

    def hist(**kw):
        a = {**good, **kw}
        return lib.udaseg_calib_hist(a["scores"], a["target"], a["pixels"], a["classes"], a["ldc"], a["probs"], a["inv_temp"],
                                     a["bins"], a["tables"], a["counters"], None)

    for bad in (dict(scores=None), dict(target=None), dict(tables=None), dict(counters=None), dict(bins=1), dict(bins=65),
                dict(ldc=23), dict(ldc=26), dict(classes=33, ldc=36), dict(classes=0), dict(classes=23, ldc=20),
                dict(probs=1, inv_temp=P), dict(probs=2), dict(pixels=0), dict(pixels=2 ** 31), dict(scores=P + 4)):
        assert hist(**bad) == -1, bad
        assert lib.udaseg_last_error()
    assert b"bins" in (hist(bins=65), lib.udaseg_last_error())[1]
    assert b"inv_temp" in (hist(probs=1, inv_temp=P), lib.udaseg_last_error())[1]
    assert b"2^31" in (hist(pixels=2 ** 31), lib.udaseg_last_error())[1]

    fin = lambda tables=P, classes=23, bins=15, out=P, per_class=P: lib.udaseg_calib_finish(tables, classes, bins, out, per_class, None)
    for bad in (dict(tables=None), dict(out=None), dict(per_class=None), dict(classes=33), dict(classes=0), dict(bins=1), dict(bins=65)):
        assert fin(**bad) == -1, bad

    goodn = dict(logits=P, target=P, pixels=100, classes=23, ldc=24, inv_temp=P, partials=P, sums=P, counters=P)

    def nll(**kw):
        a = {**goodn, **kw}
        return lib.udaseg_calib_nll(a["logits"], a["target"], a["pixels"], a["classes"], a["ldc"], a["inv_temp"], a["partials"],
                                    a["sums"], a["counters"], None)

    for bad in (dict(logits=None), dict(target=None), dict(partials=None), dict(sums=None), dict(counters=None), dict(ldc=23),
                dict(classes=33, ldc=36), dict(classes=0), dict(classes=23, ldc=20), dict(pixels=0), dict(pixels=2 ** 31),
                dict(logits=P + 8)):
        assert nll(**bad) == -1, bad
        assert lib.udaseg_last_error()
    for bad in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.udaseg_calib_step(*bad, None) == -1, bad
        assert b"calib_step" in lib.udaseg_last_error()


def test_operand_table_guards_the_new_entry_points():
    from uda_aerial_semantic_segmentation_research_amd import _operands as O
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    req = {nm: (dt, cnt, opt) for nm, dt, cnt, opt in O.requirements("udaseg_calib_hist", None, None, 100, 23, 24, 0, None, 15, None, None, 0)}
    assert req == {"scores": (torch.float32, 2400, False), "target": (torch.int64, 100, False), "inv_temp": (torch.float32, 1, True),
                   "tables": (torch.int64, 3 * 23 * 15, False), "counters": (torch.int64, 3, False)}
    req = {nm: (dt, cnt) for nm, dt, cnt, _ in O.requirements("udaseg_calib_finish", None, 23, 15, None, None, 0)}
    assert req == {"tables": (torch.int64, 1035), "out": (torch.float64, 6), "per_class": (torch.float64, 92)}
    req = {nm: (dt, cnt) for nm, dt, cnt, _ in O.requirements("udaseg_calib_nll", None, None, 100, 23, 24, None, None, None, None, 0)}
    assert req["partials"] == (torch.float64, 4 * K.seg_partials()) and req["sums"] == (torch.float64, 4)
    req = {nm: (dt, cnt) for nm, dt, cnt, _ in O.requirements("udaseg_calib_step", None, None, None, 0)}
    assert req == {"sums": (torch.float64, 4), "inv_temp": (torch.float32, 1), "state": (torch.float64, 4)}


def test_cpu_tensors_raise():
    from uda_aerial_semantic_segmentation_research_amd import calibration as C
    z, t = torch.zeros(1, 23, 8, 8), torch.zeros(1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.ReliabilityHistogram(23).update(z, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.ReliabilityHistogram(23, device="cpu").compute()
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.TemperatureScaler().fit_logits(z, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.TemperatureScaler().scale(z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.TemperatureScaler(device="cpu").temperature()
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.TemperatureScaler().fit(torch.nn.Identity(), [(z, t)], "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        C.evaluate(torch.nn.Identity(), [(z, t)], 23, "cpu")
    for bad in (dict(num_classes=33), dict(num_classes=0), dict(num_classes=23, bins=1), dict(num_classes=23, bins=65)):
        with pytest.raises(ValueError):
            C.ReliabilityHistogram(**bad)
