"""CPU checks of the pseudo-label module: the threshold arithmetic against a brute-force definition, the argument checks of the
three entry points (error code and message, no launch), their rows in the operand table, and the Python-side argument errors."""
import numpy as np
import pytest
import torch

from uda_aerial_semantic_segmentation_research_amd import _lib, _operands as O, pseudo as P

B = 256
FAKE = 4096          # any non-null, 16-byte aligned "device pointer": nothing is dereferenced before the checks


def _brute(hist, portion, floor=0.0, cap=1.0):
    """Definition by expansion: every pixel of class c as its bin index, sorted from the top; the threshold bin is the bin of the
    need-th one (need = ceil(portion * n)), B - 1 for an empty class, then clamped into [bin(floor), bin(cap)]."""
    C, bins = hist.shape
    por = np.full(C, portion, dtype=np.float64) if np.isscalar(portion) else np.asarray(portion, dtype=np.float64)
    kf = int(min(np.floor(floor * bins), bins - 1))
    kc = int(min(np.floor(cap * bins), bins - 1))
    thr, sup = [], []
    for c in range(C):
        idx = np.repeat(np.arange(bins), hist[c])[::-1]              # descending bin indices
        n = len(idx)
        need = int(np.ceil(por[c] * np.float64(n)))
        k = bins - 1 if n == 0 else int(idx[need - 1])
        thr.append(min(max(k, kf), kc))
        sup.append(n)
    return np.array(thr, dtype=np.int32), np.array(sup, dtype=np.int64)


def _table():
    h = np.zeros((6, B), dtype=np.int64)
    # class 0: empty
    h[1, 137] = 1000                                                 # a class living in one bin
    h[2, [3, 40, 41, 200, 255]] = [7, 1, 12, 5, 2]                   # spread, with a populated top bin
    g = np.random.default_rng(0)
    h[3] = g.integers(0, 50, B)                                      # dense
    h[4, 0] = 9                                                      # everything in the bottom bin
    h[5, 250:] = [1, 0, 3, 0, 0, 1]                                  # a few pixels near the top, an empty top-but-one bin
    return h


@pytest.mark.parametrize("portion, floor, cap", [
    (0.2, 0.0, 1.0),
    (1.0, 0.0, 1.0),                                                 # portion = 1: the lowest non-empty bin of every class
    (1e-9, 0.0, 1.0),                                                # need = 1: the highest non-empty bin
    (0.5, 0.9, 1.0),                                                 # floor above the quantile of most classes
    (0.05, 0.0, 0.3),                                                # cap below it
    (0.3, 0.5, 0.5),                                                 # k_floor == k_cap: every class gets that bin
    ([0.1, 0.9, 0.5, 0.01, 1.0, 0.34], 0.0, 1.0),                    # per-class portions
    ([0.1, 0.9, 0.5, 0.01, 1.0, 0.34], 0.1, 0.9),
])
def test_thresholds_from_hist_against_brute_force(portion, floor, cap):
    h = _table()
    thr, sup = P.thresholds_from_hist(h, portion, floor, cap)
    bt, bs = _brute(h, portion, floor, cap)
    assert thr.dtype == np.int32 and sup.dtype == np.int64
    np.testing.assert_array_equal(thr, bt)
    np.testing.assert_array_equal(sup, bs)


def test_thresholds_from_hist_named_cases():
    h = _table()
    thr, sup = P.thresholds_from_hist(h, 0.2)
    assert sup[0] == 0 and thr[0] == B - 1                           # empty class
    assert thr[1] == 137                                             # one bin
    assert thr[2] == 200                                             # n = 27, need = 6: 2 + 5 = 7 >= 6 at bin 200
    thr1, _ = P.thresholds_from_hist(h, 1.0)
    assert list(thr1[1:]) == [137, 3, int(np.nonzero(h[3])[0][0]), 0, 250]
    thr0, _ = P.thresholds_from_hist(h, 1e-9)
    assert list(thr0[1:]) == [137, 255, int(np.nonzero(h[3])[0][-1]), 0, 255]
    eq, _ = P.thresholds_from_hist(h, 0.3, 0.5, 0.5)
    assert list(eq) == [128] * 6
    # tensors are taken as well, and the kept count is a tail sum >= portion * n
    thr_t, sup_t = P.thresholds_from_hist(torch.from_numpy(h), 0.2)
    np.testing.assert_array_equal(thr_t, thr)
    for c in range(1, 6):
        assert h[c, thr[c]:].sum() >= 0.2 * sup[c]
        assert h[c, thr[c] + 1:].sum() < np.ceil(0.2 * sup[c])
    np.testing.assert_array_equal(P.bin_edges(B), np.arange(B) / B)
    assert P.bin_of(1.0, B) == B - 1 and P.bin_of(0.0, B) == 0 and P.bin_of(0.5, B) == 128 and P.bin_of(0.9, 1024) == 921


def test_thresholds_from_hist_argument_errors():
    h = _table()
    for bad in (0.0, -0.1, 1.5, [0.2] * 5, float("nan")):
        with pytest.raises(ValueError, match="portion"):
            P.thresholds_from_hist(h, bad)
    with pytest.raises(ValueError, match="floor"):
        P.thresholds_from_hist(h, 0.2, floor=0.8, cap=0.5)
    with pytest.raises(ValueError, match="cap"):
        P.thresholds_from_hist(h, 0.2, cap=1.5)
    with pytest.raises(ValueError, match="bins"):
        P.thresholds_from_hist(np.zeros((3, 100), dtype=np.int64), 0.2)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.udaseg_last_error().decode()        # noqa: E731

    def hist(scores=FAKE, pixels=100, classes=5, ldc=8, probs=0, bins=1024, h=FAKE, nf=FAKE):
        return lib.udaseg_conf_hist(scores, pixels, classes, ldc, probs, bins, h, nf, None)

    def labels(scores=FAKE, pixels=100, classes=5, ldc=8, probs=0, bins=1024, thr=FAKE, void=255, lab=FAKE, conf=None, cnt=FAKE):
        return lib.udaseg_pseudo_labels(scores, pixels, classes, ldc, probs, bins, thr, void, lab, conf, cnt, None)

    def thresholds(h=FAKE, classes=5, bins=1024, portion=FAKE, kf=0, kc=1023, thr=FAKE, sup=FAKE):
        return lib.udaseg_pseudo_thresholds(h, classes, bins, portion, kf, kc, thr, sup, None)

    for fn, ptrs in ((hist, ("scores", "h", "nf")), (labels, ("scores", "thr", "lab", "cnt")),
                     (thresholds, ("h", "portion", "thr", "sup"))):
        for name in ptrs:
            assert fn(**{name: None}) == -1 and "NULL" in err(), (fn.__name__, name)
    for fn in (hist, labels):
        assert fn(ldc=6) == -1 and "ldc" in err()                    # ldc % 4 != 0
        assert fn(classes=33, ldc=36) == -1 and "classes" in err()
        assert fn(classes=9, ldc=8) == -1 and "classes" in err()     # classes > ldc
        assert fn(classes=0) == -1
        assert fn(bins=1000) == -1 and "bins" in err()
        assert fn(bins=128) == -1 and "bins" in err()
        assert fn(pixels=1 << 31) == -1 and "pixels" in err()
        assert fn(pixels=0) == -1 and "pixels" in err()
        assert fn(probs=2) == -1 and "probs" in err()
        assert fn(scores=FAKE + 4) == -1 and "aligned" in err()
    assert labels(void=4) == -1 and "void_label" in err()            # void_label < classes
    assert labels(void=256) == -1 and "void_label" in err()
    assert labels(void=-1) == -1
    assert thresholds(classes=33) == -1 and "classes" in err()
    assert thresholds(classes=0) == -1
    assert thresholds(bins=300) == -1 and "bins" in err()
    assert thresholds(kf=10, kc=9) == -1 and "k_floor" in err()
    assert thresholds(kf=-1) == -1 and "k_floor" in err()
    assert thresholds(kc=1024) == -1 and "k_cap" in err()


def test_operand_rows_give_the_documented_extents():
    pixels, classes, ldc, bins = 1000, 23, 24, 1024
    req = {n: (dt, cnt, opt) for n, dt, cnt, opt in
           O.requirements("udaseg_conf_hist", None, pixels, classes, ldc, 0, bins, None, None, 0)}
    assert req == {"scores": (torch.float32, pixels * ldc, False), "hist": (torch.int64, classes * bins, False),
                   "nonfinite": (torch.int64, 1, False)}
    req = {n: (dt, cnt, opt) for n, dt, cnt, opt in
           O.requirements("udaseg_pseudo_thresholds", None, classes, bins, None, 0, bins - 1, None, None, 0)}
    assert req == {"hist": (torch.int64, classes * bins, False), "portion": (torch.float64, classes, False),
                   "thr_bins": (torch.int32, classes, False), "support": (torch.int64, classes, False)}
    req = {n: (dt, cnt, opt) for n, dt, cnt, opt in
           O.requirements("udaseg_pseudo_labels", None, pixels, classes, ldc, 0, bins, None, 255, None, None, None, 0)}
    assert req == {"scores": (torch.float32, pixels * ldc, False), "thr_bins": (torch.int32, classes, False),
                   "labels": (torch.uint8, pixels, False), "conf": (torch.float32, pixels, True),
                   "counts": (torch.int64, classes + 2, False)}


def test_python_argument_errors_and_no_cpu_path():
    model = torch.nn.Conv2d(3, 5, 1)
    ok = dict(model=model, num_classes=5)
    for bad, word in ((dict(portion=0.0), "portion"), (dict(portion=1.2), "portion"), (dict(portion=[0.2, 0.3]), "portion"),
                      (dict(floor=-0.1), "floor"), (dict(cap=1.1), "cap"), (dict(floor=0.95, cap=0.9), "floor"),
                      (dict(bins=1000), "bins"), (dict(void=4), "void"), (dict(void=256), "void"),
                      (dict(num_classes=0), "num_classes"), (dict(num_classes=33), "num_classes"),
                      (dict(dtype=torch.float16), "dtype")):
        with pytest.raises(ValueError, match=word):
            P.PseudoLabeler(**{**ok, **bad})
    lab = P.PseudoLabeler(model, 5, portion=[0.1, 0.2, 0.3, 0.4, 0.5], floor=0.5, cap=0.5, bins=256, void=5)
    assert lab.void == 5 and lab.thr_bins is None
    with pytest.raises(RuntimeError, match="fit"):
        lab.report()
    with pytest.raises(RuntimeError, match="fit"):
        lab.label(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="bins"):
        P.ConfidenceHistogram(5, bins=100)
    with pytest.raises(ValueError, match="num_classes"):
        P.ConfidenceHistogram(40)
    thr = torch.zeros(5, dtype=torch.int32)
    z = torch.zeros(1, 5, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.pseudo_labels(z, thr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.ConfidenceHistogram(5).update(z)
    with pytest.raises(ValueError, match="thr_bins"):
        P.pseudo_labels(z, thr.long())
    with pytest.raises(ValueError, match="thr_bins"):
        P.pseudo_labels(z, thr[:4])
    with pytest.raises(ValueError, match="void"):
        P.pseudo_labels(z, thr, void=3)
    with pytest.raises(ValueError, match="bins"):
        P.pseudo_labels(z, thr, bins=300)
    with pytest.raises(ValueError, match="counts"):
        P.pseudo_labels(z, thr, counts=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        P.pseudo_labels(torch.zeros(5, 4, 4), thr)
