"""CPU checks of the regions module: the numpy mirror (tests/_regions_ref.py) against scipy.ndimage.label, the properties that make
the shared case maps worth running on the GPU, the host-side tables and measures of regions.py, and the argument rules of the
entry points, which refuse bad arguments with rc < 0 and a message before any launch (no GPU needed)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _regions_ref as R

TH, TW = R.TILE
STRUCT_SHAPE = (3 * TH + 5, 3 * TW + 7)
DEEP_SHAPE = (5 * TH + 3, 5 * TW + 1)
MIN_AREA = 12                                                                  # the scalar threshold of the sieve tests
PER_CLASS = [0, 30, 3, 1, 500]                                                 # and the per-class one (beyond its length: kept)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Every map the GPU tests run, by name: 'map:n,h,w' or 'struct:name' / 'deep:name'."""
    kind, arg = name.split(":")
    if kind == "map":
        n, h, w = (int(v) for v in arg.split(","))
        return R.make_map(n, h, w)
    h, w = STRUCT_SHAPE if kind == "struct" else DEEP_SHAPE
    return R.structure(arg, h, w)


CASES = [f"map:{n},{h},{w}" for n, h, w in R.shapes()] + [f"struct:{s}" for s in R.STRUCTURES] + ["deep:u", "deep:serpentine"]


def _scipy_ids(L, void, connectivity):
    """First-raster-pixel ids from scipy's labelling of every class mask of one image."""
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = L.shape
    out = np.full((h, w), -1, dtype=np.int32)
    idx = np.arange(h * w).reshape(h, w)
    st = np.ones((3, 3), dtype=int) if connectivity == 8 else None
    for c in np.unique(L[~void]):
        lab, k = ndi.label((L == c) & ~void, structure=st)
        if k:
            first = ndi.minimum(idx, lab, index=np.arange(1, k + 1)).astype(np.int32)
            sel = lab > 0
            out[sel] = first[lab[sel] - 1]
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("case", CASES)
def test_mirror_partition_equals_scipy(case, ignore, connectivity):
    pytest.importorskip("scipy")
    m = _case(case)
    if m.shape[0] > 3:
        m = m[:3]
    got = R.ids(m, connectivity, ignore)
    L = R.read(m)
    V = R.void_of(L, ignore)
    for i in range(m.shape[0]):
        assert np.array_equal(got[i], _scipy_ids(L[i], V[i], connectivity)), (case, i)
    a = R.areas(got)
    assert ((a == 0) == (got < 0)).all() and int(a[R.roots(got)].sum()) == int((got >= 0).sum())
    m64 = R.as_int64(m)
    assert np.array_equal(R.ids(m64, connectivity, ignore), got)                # out-of-range values read as 255


def test_mirror_on_a_hand_made_map():
    m = np.array([[[1, 1, 0, 2],
                   [0, 1, 0, 2],
                   [1, 0, 255, 2]]], dtype=np.uint8)
    i4, i8 = R.ids(m, 4, 255), R.ids(m, 8, 255)
    assert i4[0].tolist() == [[0, 0, 2, 3], [4, 0, 2, 3], [8, 9, -1, 3]]
    assert i8[0].tolist() == [[0, 0, 2, 3], [2, 0, 2, 3], [0, 2, -1, 3]]
    assert R.areas(i4)[0].tolist() == [[3, 3, 2, 3], [1, 3, 2, 3], [1, 1, 0, 3]]
    assert R.ids(m, 4, None)[0, 2, 2] == 10 and R.areas(R.ids(m, 4, None))[0, 2, 2] == 1
    out, counts = R.sieve(m, 2, 4, void=9, ignore_index=255)
    assert out[0].tolist() == [[1, 1, 0, 2], [9, 1, 0, 2], [9, 9, 255, 2]] and counts.tolist() == [[3, 3, 3]]
    out, counts = R.sieve(m, [0, 4], 8, void=9, ignore_index=255)              # class 1: one region of 4 pixels under 8
    assert np.array_equal(out, m) and counts.tolist() == [[0, 0, 3]]
    s = R.stats(m, 2, 4, 255)
    assert s[0, :4].tolist() == [3, 4, 2, 1] and s[1, :4].tolist() == [2, 4, 1, 1] and s[:, 4:].sum() == 0


@pytest.mark.parametrize("case", CASES)
def test_case_maps_can_tell_a_broken_kernel(case):
    """A component spans at least two tile seams wherever the map has two; the sieve thresholds remove and keep something on every
    map the sieve tests use; 4- and 8-connectivity differ wherever the case is meant to tell them apart."""
    m = _case(case)
    n, h, w = m.shape
    i4, i8 = R.ids(m, 4, 255), R.ids(m, 8, 255)
    seams = (h - 1) // TH + (w - 1) // TW
    kind, arg = case.split(":")
    if seams >= 2 and arg not in ("checker", "diagonals"):                      # those two are about one-pixel regions
        assert R.seams_spanned(i4) >= 2 and R.seams_spanned(i8) >= 2, case
    if kind != "map" and arg == "u":
        assert R.seams_spanned(i4) >= (h - 1) // TH + 1
    if (kind == "map" and h * w >= 45) or arg == "random":                      # the maps the sieve tests run
        for thr in (MIN_AREA, PER_CLASS):
            for conn in (4, 8):
                c = R.sieve(m, thr, conn)[1].sum(axis=0)
                assert c[0] > 0 and c[1] > 0 and c[2] > 0, (case, thr, conn, c)
    if arg in R.TELLS_4_FROM_8 or (kind == "map" and h * w >= 45):
        assert not np.array_equal(i4, i8), case
    if arg == "checker":
        assert np.array_equal(i4[0].reshape(-1), np.arange(h * w)) and sorted(np.unique(i8).tolist()) == [0, 1]
    if arg == "constant":
        assert (i4 == 0).all() and (R.areas(i4) == h * w).all()
    if arg == "fenced":
        assert (i4[m == 255] == -1).all() and len(np.unique(i4)) == 4 and len(np.unique(R.ids(m, 8, None))) == 4
    if arg == "diagonals":
        assert (R.areas(i4)[m == 5] == 1).all() and (R.areas(i8)[m == 5] == 14).all() and (R.areas(i8)[m == 6] == 14).all()
    if arg == "serpentine":
        assert (i4[m == 8] == 0).all()
    if case == "map:65,9,13":
        assert (m[:-1, -1] == m[1:, 0]).all() and (i4[:, 0, 0] == 0).all()


def test_min_area_table_and_summary():
    from uda_aerial_semantic_segmentation_research_amd import regions as G
    t = G.min_area_table(7)
    assert t.dtype == np.int32 and t.shape == (256,) and (t == 7).all()
    t = G.min_area_table([0, 5, 2])
    assert t[:4].tolist() == [0, 5, 2, 0] and (t[3:] == 0).all()
    assert np.array_equal(G.min_area_table(torch.tensor([1, 2])), G.min_area_table(np.array([1, 2])))
    for bad in (-1, [3, -2], [1.5], True, np.zeros(257, dtype=np.int64), np.zeros((2, 2), dtype=np.int64), 1 << 31):
        with pytest.raises(ValueError):
            G.min_area_table(bad)
    s = np.zeros((3, 34), dtype=np.int64)
    s[0, :2] = [4, 10]
    s[0, 2], s[0, 3] = 3, 1
    s[2, :2] = [1, 1 << 33]
    r = G.summarize(s)
    assert r["components"].tolist() == [4, 0, 1] and r["pixels"].tolist() == [10, 0, 1 << 33]
    assert r["mean_area"][0] == 2.5 and np.isnan(r["mean_area"][1]) and r["mean_area"][2] == float(1 << 33)
    assert r["hist"].shape == (3, 32) and r["hist"][0, :2].tolist() == [3, 1] and np.array_equal(r["stats"], s)
    t2 = G.summarize(np.array([[2, 10] + [0] * 32, [0, 0] + [0] * 32, [4, 4] + [0] * 32]))
    ratio = G.fragmentation(r, t2)
    assert ratio[0] == 2.0 and np.isnan(ratio[1]) and ratio[2] == 0.25


def test_cpu_tensors_and_bad_arguments_raise():
    from uda_aerial_semantic_segmentation_research_amd import regions as G
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    for call in (lambda: G.label(m), lambda: G.sieve(m, 2), lambda: G.RegionStats(3).update(m),
                 lambda: G.RegionStats(3).update(torch.zeros(1, 3, 4, 4)), lambda: G.evaluate(torch.nn.Identity(), [], 3, "cpu")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for call in (lambda: G.label(m, connectivity=6), lambda: G.label(m, ignore_index=256), lambda: G.label([[0]]),
                 lambda: G.sieve(m, 2, connectivity=True), lambda: G.sieve(m, 2, void=None), lambda: G.sieve(m, 2, void=-1),
                 lambda: G.RegionStats(256), lambda: G.RegionStats(0), lambda: G.RegionStats(3, connectivity=5),
                 lambda: G.RegionStats(3, ignore_index=-1), lambda: G.RegionStats(3).update("x"),
                 lambda: G.SievedLoader([], -1), lambda: G.SievedLoader([], 2, connectivity=3),
                 lambda: G.SievedLoader([], 2, void=256)):
        with pytest.raises(ValueError):
            call()
    assert len(G.SievedLoader([1, 2, 3], 4)) == 3


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """rc < 0 and a message that names the argument, from the library itself: the pointers are host buffers nothing reads."""
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K
    lib = _lib.load()
    assert K.regions_tile() == R.TILE and lib.udaseg_regions_tile() == (TH << 16) | TW
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(n=2, h=4, w=4, connectivity=4, classes=5, ignore_index=255, void_label=255, i64=0, has=1)

    def call(entry, **kw):
        a = {**good, **kw}
        if entry == "label":
            return lib.udaseg_regions_label(p, a["i64"], a["n"], a["h"], a["w"], a["connectivity"], a["has"], a["ignore_index"], p, p, None)
        if entry == "sieve":
            return lib.udaseg_regions_sieve(p, a["i64"], p, p, a["n"], a["h"], a["w"], a["has"], a["ignore_index"], p, a["void_label"],
                                            p, p, None)
        return lib.udaseg_regions_stats(p, a["i64"], p, p, a["n"], a["h"], a["w"], a["classes"], a["has"], a["ignore_index"], p, None)

    for entry in ("label", "sieve", "stats"):
        cases = [(dict(n=0), b"n"), (dict(n=65536), b"n"), (dict(h=0), b"h"), (dict(w=0), b"w"), (dict(h=1 << 16, w=1 << 15), b"2^31"),
                 (dict(ignore_index=256), b"ignore_index"), (dict(ignore_index=-1), b"ignore_index"), (dict(i64=2), b"labels_i64"),
                 (dict(has=2), b"has_ignore")]
        if entry == "label":
            cases += [(dict(connectivity=c), b"connectivity") for c in (0, 6, -4, 1)]
        if entry == "sieve":
            cases += [(dict(void_label=256), b"void_label"), (dict(void_label=-1), b"void_label")]
        if entry == "stats":
            cases += [(dict(classes=256), b"classes"), (dict(classes=0), b"classes")]
        for kw, word in cases:
            rc = call(entry, **kw)
            msg = lib.udaseg_last_error()
            assert rc < 0 and word in msg and b"regions_" + entry.encode() in msg, (entry, kw, rc, msg)
    assert lib.udaseg_regions_label(None, 0, 2, 4, 4, 4, 0, 0, p, p, None) < 0     # a missing operand
    assert lib.udaseg_regions_label(p, 0, 2, 4, 4, 4, 0, 0, None, p, None) < 0
    assert lib.udaseg_regions_sieve(p, 0, p, None, 2, 4, 4, 0, 0, p, 255, p, None, None) < 0
    assert lib.udaseg_regions_stats(p, 0, p, p, 2, 4, 4, 5, 0, 0, None, None) < 0
