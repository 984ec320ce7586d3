"""CPU checks of the prototype module: the two host mirrors against hand-computed cases, argument validation, "no CPU path",
and the three bindings' error convention (bad shapes come back as error codes before any launch)."""
import numpy as np
import pytest
import torch

from _proto_ref import accumulate_mirror, rectify_mirror, sum_bars, update_mirror


def _state(C, D):
    return np.zeros((C, D)), np.zeros(C), np.zeros(C, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------ update_mirror
def test_first_sight_copies_the_mean_and_the_spread():
    sums = np.array([[2.0, 4.0, 6.0, 8.0], [0.0, 0.0, 0.0, 0.0]])
    sq = np.array([2.0 * (1 + 4 + 9 + 16) + 8.0, 0.0])              # two pixels around (1, 2, 3, 4), spread 4
    counts = np.array([2, 0, 3, 1])
    proto, spread, seen = _state(2, 4)
    p, s, sn, last, inv = update_mirror(sums, sq, counts, proto, spread, seen, momentum=0.9, min_pixels=1, tau_scale=2.0)
    assert p[0].tolist() == [1.0, 2.0, 3.0, 4.0] and s[0] == 4.0 and sn.tolist() == [1, 0]
    assert p[1].tolist() == [0.0] * 4 and s[1] == 0.0               # an unseen class is left alone
    assert last.tolist() == [2, 0, 3, 1] and last.dtype == np.int64
    assert inv.dtype == np.float32 and inv == np.float32(1.0 / 8.0)  # tau = 2 * mean spread of the seen classes


def test_ema_is_two_products_and_one_sum_each_rounded():
    mom = 0.999
    old, new = 0.1, 0.7
    proto = np.array([[old, 0.0, 0.0, 0.0]])
    sums = np.array([[3 * new, 0.0, 0.0, 0.0]])
    sq = np.array([3 * new * new + 3.0])
    p, s, sn, _, _ = update_mirror(sums, sq, np.array([3, 0, 0]), proto, np.array([0.5]), np.array([1]), momentum=mom, min_pixels=1)
    mean = np.float64(3 * new) / np.float64(3.0)
    want = np.float64(mom) * np.float64(old) + (np.float64(1.0) - np.float64(mom)) * mean
    assert p[0, 0] == want and sn[0] == 1
    batch_s = np.float64(sq[0]) / 3.0 - mean * mean
    assert s[0] == np.float64(mom) * 0.5 + (np.float64(1.0) - np.float64(mom)) * batch_s
    # the inputs are not modified
    assert proto[0, 0] == old


def test_min_pixels_gate():
    sums, sq = np.ones((2, 4)) * 5.0, np.array([30.0, 30.0])
    proto, spread, seen = _state(2, 4)
    p, s, sn, last, inv = update_mirror(sums, sq, np.array([5, 4, 0, 0]), proto, spread, seen, min_pixels=5)
    assert sn.tolist() == [1, 0] and p[0].tolist() == [1.0] * 4 and p[1].tolist() == [0.0] * 4
    assert last.tolist() == [5, 4, 0, 0]
    with pytest.raises(ValueError):
        update_mirror(sums, sq, np.array([5, 4, 0, 0]), proto, spread, seen, min_pixels=0)


def test_spread_clamps_at_zero_for_a_one_pixel_class():
    f = np.array([[0.1, 0.2, 0.3, 0.7]], dtype=np.float32).astype(np.float64)
    sums, sq = f.copy(), np.array([(f * f).sum() * (1 - 2.0 ** -50)])   # a hair below |mean|^2: the difference is negative
    proto, spread, seen = _state(1, 4)
    p, s, sn, _, inv = update_mirror(sums, sq, np.array([1, 0, 0]), proto, spread, seen, min_pixels=1)
    assert s[0] == 0.0 and sn[0] == 1 and np.array_equal(p, f)
    assert inv == 0.0                                               # tau = 0 is not positive


def test_auto_tau_with_no_class_seen_is_zero_and_fixed_tau_is_left_alone():
    proto, spread, seen = _state(3, 4)
    z = np.zeros
    _, _, sn, _, inv = update_mirror(z((3, 4)), z(3), z(5, dtype=np.int64), proto, spread, seen, tau_scale=1.0, inv_tau=7.0)
    assert not sn.any() and inv == 0.0 and inv.dtype == np.float32
    _, _, _, _, inv = update_mirror(z((3, 4)), z(3), z(5, dtype=np.int64), proto, spread, seen, tau_scale=0.0, inv_tau=7.0)
    assert inv == np.float32(7.0)


# ----------------------------------------------------------------------------------------------------------- rectify_mirror
def _case(seed=0, P=50, C=5, D=8):
    g = np.random.default_rng(seed)
    proto = g.standard_normal((C, D))
    cls = g.integers(0, C, P)
    feat = (proto[cls] + 0.3 * g.standard_normal((P, D))).astype(np.float32)
    logits = (3.0 * g.standard_normal((P, C))).astype(np.float32)
    return feat, logits, proto, cls


def test_rectify_with_zero_inv_tau_is_p_renormalised_over_the_seen_classes():
    feat, logits, proto, _ = _case()
    seen = np.array([1, 0, 1, 1, 0])
    out = rectify_mirror(feat, logits, proto, seen, 0.0)
    z = logits.astype(np.float64)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    want = p * seen / (p * seen).sum(1, keepdims=True)
    assert np.allclose(out, want, rtol=1e-14, atol=0) and (out[:, [1, 4]] == 0.0).all()
    assert np.allclose(out.sum(1), 1.0, atol=1e-14)
    none = rectify_mirror(feat, logits, proto, np.zeros(5), 123.0)   # nothing seen: u = 1, the softmax itself
    assert np.allclose(none, p, rtol=1e-14, atol=0)


def test_rectify_with_a_huge_inv_tau_is_the_nearest_seen_prototype():
    feat, logits, proto, cls = _case(1)
    seen = np.array([1, 1, 0, 1, 1])
    out = rectify_mirror(feat, logits, proto, seen, 1e30)
    pr = proto.astype(np.float32).astype(np.float64)
    d = ((feat.astype(np.float64)[:, None] - pr[None]) ** 2).sum(2)
    d[:, 2] = np.inf
    near = d.argmin(1)
    assert (out.argmax(1) == near).all() and np.array_equal(out[np.arange(len(near)), near], np.ones(len(near)))
    assert (near[cls != 2] == cls[cls != 2]).all()                  # the noise is small against the prototypes' distances
    probs = rectify_mirror(feat, np.full_like(logits, 0.2), proto, seen, 1e30, probs=True)
    assert (probs.argmax(1) == near).all()


def test_rectify_nan_rows():
    feat, logits, proto, _ = _case(2, P=6)
    seen = np.ones(5)
    feat[0, 3], logits[1, 2], logits[2, 0] = np.nan, np.inf, -np.inf
    out = rectify_mirror(feat, logits, proto, seen, 0.5)
    assert np.isnan(out[:3]).all() and np.isfinite(out[3:]).all()
    probs = np.full((6, 5), 0.2, dtype=np.float32)
    probs[0, 0], probs[1, 1], probs[2] = 1.5, -0.1, 0.0
    out = rectify_mirror(feat[3:].repeat(2, 0), probs, proto, seen, 0.5, probs=True)
    assert np.isnan(out[:3]).all() and np.isfinite(out[3:]).all()   # outside [0, 1]; R == 0
    with pytest.raises(ValueError):
        rectify_mirror(feat, logits[:, :4], proto, seen, 0.5)


def test_accumulate_mirror_rules():
    f = np.arange(24, dtype=np.float32).reshape(6, 4)
    f[5, 1] = np.inf
    lab = np.array([0, 1, 0, 9, 255, 0], dtype=np.uint8)
    sums, sq, counts, abs_sums, abs_sq = accumulate_mirror(f, lab, 3)
    assert counts.tolist() == [2, 1, 0, 2, 1]
    assert sums[0].tolist() == (f[0] + f[2]).tolist() and sq[1] == float((f[1] ** 2).sum()) and not sums[2].any()
    bs, bq = sum_bars(counts, abs_sums, abs_sq)
    assert bs[0, 1] == 2 * 2.0 ** -52 * (1 + 9) and bq[2] == 0.0


# --------------------------------------------------------------------------------------------------------------- validation
def test_bank_validation():
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    for bad in (dict(num_classes=0), dict(num_classes=33), dict(num_classes=2.5), dict(dim=6), dict(dim=0), dict(dim=68),
                dict(momentum=-0.1), dict(momentum=1.5), dict(min_pixels=0), dict(min_pixels=1.5), dict(tau="fixed"),
                dict(tau=0.0), dict(tau=float("nan")), dict(tau_scale=0.0), dict(tau_scale=float("inf"))):
        with pytest.raises(ValueError):
            PR.PrototypeBank(**{"num_classes": 5, **bad})
    bank = PR.PrototypeBank(5, dim=8, tau=2.0)
    assert bank.tau == 2.0 and PR.PrototypeBank(5).tau is None and PR.PrototypeBank(5).dim == 16
    with pytest.raises(ValueError):
        bank.accumulate(torch.zeros(1, 16, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))          # 16 channels, the bank has 8
    with pytest.raises(ValueError):
        bank.accumulate(torch.zeros(8, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        bank.accumulate(torch.zeros(1, 8, 4, 4, dtype=torch.float64), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        PR.rectify(torch.zeros(1, 8, 4, 4), torch.zeros(1, 5, 4, 4), "bank")
    with pytest.raises(ValueError):
        PR.domain_gap(bank, PR.PrototypeBank(5, dim=16))
    with pytest.raises(ValueError):
        PR.domain_gap(bank, None)


def test_no_cpu_path():
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    bank = PR.PrototypeBank(5, dim=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bank.accumulate(torch.zeros(1, 8, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PR.rectify(torch.zeros(1, 8, 4, 4), torch.zeros(1, 5, 4, 4), bank)
    with pytest.raises(RuntimeError, match="no CPU path"):
        PR.PrototypeBank(5, device="cpu").update()
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=5)
    lab = PR.PrototypeLabeler(net, 5)
    assert lab.bank.dim == 16 and lab.bank.num_classes == 5 and lab.rectify_after == 0 and lab.update_bank
    with pytest.raises(RuntimeError, match="no CPU path"):
        lab.label(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lab.init_from([(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), torch.zeros(1, 32, 32, dtype=torch.uint8))])


def test_labeler_validation():
    from uda_aerial_semantic_segmentation_research_amd import proto as PR
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=5)
    for bad in (dict(bank=PR.PrototypeBank(6)), dict(bank="bank"), dict(rectify_after=-1), dict(rectify_after=1.5),
                dict(portion=0.0), dict(halve_every=0), dict(void=3)):
        with pytest.raises(ValueError):
            PR.PrototypeLabeler(net, 5, **bad)
    with pytest.raises(ValueError):
        PR.PrototypeLabeler(torch.nn.Conv2d(3, 5, 1), 5)            # no forward_parts
    bank = PR.PrototypeBank(5, dim=16, momentum=0.9)
    assert PR.PrototypeLabeler(net, 5, bank=bank, rectify_after=3, update_bank=False).bank is bank


# ------------------------------------------------------------------------------------------------- the bindings' error codes
def test_bindings_refuse_bad_shapes_before_any_launch():
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    N = None
    acc = lambda ldf, dim, pixels, classes: lib.udaseg_proto_accumulate(N, ldf, dim, N, pixels, classes, N, N, N, N)
    upd = lambda classes, dim, mom=0.9, mp=1, ts=1.0: lib.udaseg_proto_update(N, N, N, classes, dim, mom, mp, ts, 1, N, N, N, N, N, N)
    rec = lambda ldf, dim, ldc, classes, probs=0, pixels=64: lib.udaseg_proto_rectify(N, ldf, dim, N, ldc, classes, probs, N, N, N,
                                                                                     pixels, N, N)
    cases = [(acc, (16, 6, 64, 5), b"dim"), (acc, (16, 0, 64, 5), b"dim"), (acc, (16, 68, 64, 5), b"dim"),
             (acc, (12, 16, 64, 5), b"ldf"), (acc, (18, 16, 64, 5), b"ldf"), (acc, (16, 16, 64, 0), b"classes"),
             (acc, (16, 16, 64, 33), b"classes"), (acc, (16, 16, 0, 5), b"pixels"),
             (upd, (0, 16), b"classes"), (upd, (33, 16), b"classes"), (upd, (5, 10), b"dim"), (upd, (5, 16, 1.5), b"momentum"),
             (upd, (5, 16, 0.9, 0), b"min_pixels"), (upd, (5, 16, 0.9, 1, float("nan")), b"tau_scale"),
             (rec, (16, 6, 8, 5), b"dim"), (rec, (8, 16, 8, 5), b"ldf"), (rec, (16, 16, 8, 33), b"classes"),
             (rec, (16, 16, 6, 5), b"ldc"), (rec, (16, 16, 4, 5), b"ldc"), (rec, (16, 16, 8, 5, 2), b"probs"),
             (rec, (16, 16, 8, 5, 0, 0), b"pixels")]
    for fn, args, word in cases:                                    # the message is the last call's: one call at a time
        rc = fn(*args)
        assert rc == -1 and word in lib.udaseg_last_error(), (args, rc, word, lib.udaseg_last_error())
    # well-shaped calls with NULL pointers are refused too, as NULL pointers
    for fn, args in ((acc, (16, 16, 64, 5)), (upd, (5, 16)), (rec, (16, 16, 8, 5))):
        assert fn(*args) == -1 and b"NULL" in lib.udaseg_last_error()
