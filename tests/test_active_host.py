"""CPU checks of the active-labelling module: the numpy mirror (tests/_active_ref.py, integral images) against brute-force loops
over the window and closed forms, the inputs of the GPU tests (so that those are not vacuous), the argument rules of active.py and
of the entry points (no launch is reached), and ActivePool's bookkeeping on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import _active_ref as R

TINY = [(1, 1, 1, 1), (2, 1, 7, 3), (2, 7, 1, 3), (3, 5, 9, 16), (2, 12, 17, 0), (2, 12, 17, 1), (1, 23, 31, 4)]


@pytest.mark.parametrize("classes", [2, 5, 32])
@pytest.mark.parametrize("shape", TINY)
def test_mirror_counts_match_brute_force(shape, classes):
    n, h, w, r = shape
    m = R.make_map(n, h, w, r, classes, seed=3)
    for ign in (None, 255):
        nc, L, v = R.counts(m, r, classes, ign)
        assert np.array_equal(nc, R.counts_brute(m, r, classes, ign))
    m64 = R.as_int64(m)
    assert np.array_equal(R.counts(m64, r, classes, 255)[0], nc)               # out-of-range values read as 255: void
    assert (v == (m >= classes)).all()                                         # a label >= classes is void with or without ignore


def test_mirror_counts_match_scipy_on_the_interior():
    ndi = pytest.importorskip("scipy.ndimage")
    r, classes = 3, 5
    m = R.make_map(1, 40, 50, r, classes, seed=1)
    nc, L, v = R.counts(m, r, classes, 255)
    for c in range(classes):
        f = ndi.uniform_filter(((L[0] == c) & ~v[0]).astype(np.float64), size=2 * r + 1, mode="constant") * (2 * r + 1) ** 2
        assert np.array_equal(np.rint(f[r:-r, r:-r]).astype(np.int64), nc[0, c, r:-r, r:-r])


def test_window_sum32_is_the_box_sum():
    rng = np.random.RandomState(0)
    e = rng.rand(2, 9, 13).astype(np.float32)
    for r in (0, 1, 4, 16):
        assert np.allclose(R.window_sum32(e, r), R.box(e.astype(np.float64), r), rtol=1e-5, atol=0)


def test_radius_zero_constant_map_and_bound():
    classes = 5
    m = R.make_map(2, 12, 17, 1, classes, seed=2)
    out, agr, cnt = R.mode(m, 0, classes, 255, False, 255)
    live = m < classes
    assert np.array_equal(out[live], m[live]) and (out[~live] == 255).all() and (agr[live] == 1).all() and (agr[~live] == 0).all()
    assert cnt[:, 0].tolist() == [0, 0] and cnt[:, 2].tolist() == (~live).reshape(2, -1).sum(1).tolist()
    i64, i32 = R.impurity(m, 0, classes, 255)
    assert (i64 == 0).all() and (i32 == 0).all()
    const = np.full((1, 9, 11), 3, dtype=np.uint8)
    for r in (1, 4, 16):
        i64, i32 = R.impurity(const, r, classes, None)
        assert (i64 == 0).all() and (i32 == 0).all()
    for c in (2, 5, 32):
        mm = R.make_map(1, 23, 31, 2, c, seed=5)
        nc = R.counts(mm, 2, c, 255)[0]
        i64, i32 = R.impurity_of_counts(nc, c, 2)
        n = nc.sum(1)
        bound = np.log(np.minimum(c, np.maximum(n, 1))) / np.log(c)
        assert (i64 <= bound + 1e-12).all() and (i32 <= bound + 1e-6).all() and (i64 >= 0).all() and i64.max() > 0.5
        assert np.abs(i32 - i64).max() < 1e-6


@pytest.mark.parametrize("r", [1, 3, 16])
def test_straight_edge_has_the_closed_form_impurity(r):
    h, w, c = 2 * r + 3, 6 * r + 8, 3 * r + 4
    m = np.zeros((1, h, w), dtype=np.uint8)
    m[0, :, c:] = 1
    i64, i32 = R.impurity(m, r, 2, None)
    x = np.arange(r, w - r)                                                    # whole windows (columns); rows are clipped alike
    k = np.clip(np.where(x < c, x + r - c + 1, c - (x - r)), 0, 2 * r + 1)     # columns of the window on the far side of the edge
    q = k / (2 * r + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = -(np.where(q > 0, q * np.log(q), 0) + np.where(q < 1, (1 - q) * np.log(1 - q), 0)) / np.log(2)
    # the fp32 form subtracts two sums of the size of T[n]: four roundings of that size over the smallest n log 2 of these windows
    tol32 = 4 * float(np.spacing(R.table(r).max())) / ((r + 1) * (2 * r + 1) * np.log(2))
    assert np.abs(i64[0, :, r:w - r] - want[None, :]).max() < 1e-12 and np.abs(i32[0, :, r:w - r] - want[None, :]).max() < tol32
    assert i64[0, r + 1, c] == i64[0, r + 1, c - 1] and i64[0, r + 1, c + r] == 0 and i64[0, r + 1, c + r - 1] > 0
    if r == 1:
        assert abs(i64[0, 2, c] - (np.log(3) - (2 / 3) * np.log(2)) / np.log(2)) < 1e-12


def test_tie_rule_three_ways():
    a = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]]], dtype=np.uint8)          # 3 : 3 : 3, the centre is one of them
    assert R.mode(a, 1, 5, 255, False, 255)[0][0, 1, 1] == 1
    b = np.array([[[0, 0, 0], [0, 1, 2], [2, 2, 2]]], dtype=np.uint8)          # 4 : 1 : 4, the centre is not
    out, agr, _ = R.mode(b, 1, 5, 255, False, 255)
    assert out[0, 1, 1] == 0 and agr[0, 1, 1] == np.float32(4) / np.float32(9)
    c = np.array([[[3, 3, 3], [3, 255, 1], [1, 1, 1]]], dtype=np.uint8)        # 4 : 4 around a void centre
    out, agr, cnt = R.mode(c, 1, 5, 255, True, 255)
    assert out[0, 1, 1] == 1 and agr[0, 1, 1] == np.float32(0.5) and cnt.tolist() == [[0, 1, 0]]
    out, _, cnt = R.mode(c, 1, 5, 255, False, 254)
    assert out[0, 1, 1] == 254 and cnt[0, 1:].tolist() == [0, 1]
    d = np.full((1, 5, 5), 255, dtype=np.uint8)                                # nothing to vote with
    out, agr, cnt = R.mode(d, 1, 5, 255, True, 255)
    assert (out == 255).all() and (agr == 0).all() and cnt.tolist() == [[0, 0, 25]]


# ------------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("case", R.CASES)
def test_gpu_label_cases_are_not_vacuous(case):
    """Every case with more than one pixel and a radius >= 1 has pixels with impurity 0 and with impurity > 0 and a pixel the vote
    leaves; every such case but the 7 x 1 column (where, with 2 and 23 classes, the texture happens to move no vote) has a pixel the
    vote changes.  What cannot hold is not asked: at 1 x 1 and at radius 0 the window is the pixel, the vote is the identity and the
    impurity is 0.  Where the map holds whole blocks (R.roomy) there is also an empty window and a label beyond the classes that is
    not 255; the small shapes are there for the frame and the n-in-grid limit."""
    n, h, w, r, classes = case
    m = R.make_map(n, h, w, r, classes)
    nc, L, v = R.counts(m, r, classes, 255)
    i64, _ = R.impurity_of_counts(nc, classes, r)
    out, agr, cnt = R.mode(m, r, classes, 255, False, 255)
    assert (L >= classes).any() or h * w < 8
    assert (i64 == 0).any() and (~v & (out == m)).any()
    if h * w == 1 or r == 0:
        assert (i64 == 0).all() and cnt[:, 0].sum() == 0
        return
    assert (i64 > 0).any()
    if (h, w) != (7, 1):
        assert cnt[:, 0].sum() > 0
    if R.roomy(h, w, r):
        assert (nc.sum(1) == 0).any()
        assert ((L >= classes) & (L != 255)).any()                             # labels beyond the classes that are not 255


def test_some_gpu_case_has_a_window_that_covers_the_image():
    assert any(r >= max(h, w) - 1 and h * w > 1 for n, h, w, r, c in R.CASES)
    assert any(R.roomy(h, w, r) for n, h, w, r, c in R.CASES)


@pytest.mark.parametrize("probs", [False, True])
@pytest.mark.parametrize("case", R.CASES)
def test_gpu_score_cases_have_a_clear_winner(case, probs):
    n, h, w, r, classes = case
    z = R.make_scores(n, h, w, r, classes, probs=probs)
    gap = R.top_two_gap(z, classes)
    assert gap.min() >= R.GAP, gap.min()
    lab, h64, h32, cnt = R.prepare(z, classes, probs)
    assert cnt.sum() == n * h * w and (cnt[1] > 0 or n * h * w < 200) and (lab == 255).sum() == cnt[1]
    assert np.abs(h32 - h64).max() < 1e-5 and h64.max() <= 1 + 1e-12 and h64.max() > (0.2 if h * w > 1 else 0.1)      # (one pixel of two classes: 0.157)


def test_gpu_selection_cases_select_some_but_not_all_and_one_has_ties():
    tie_groups = []
    for n, h, w, r, classes, kind, budget, cell in R.SELECT_CASES:
        z = R.make_scores(n, h, w, r, classes)
        lab, _, h32, _ = R.prepare(z, classes)
        _, _, _, key32, cand = R.score(lab, h32, r, classes, kind)
        if cell is not None:
            key32 = R.cells(key32, *cell)[1]
        items = key32[0].size
        k = budget if isinstance(budget, int) else max(1, int(np.floor(budget * items)))
        mask, cnt, ties = R.select(key32, k)
        assert (cnt[:, 0] > 0).all() and (cnt[:, 0] < cnt[:, 1]).all(), (cnt, k)
        assert (cnt[:, 0] >= k).all() and (cnt[:, 0] <= k + ties - 1).all()        # the budget, and at most the last key's ties
        tie_groups.append(int(ties.max()))
    assert max(tie_groups) > 1, tie_groups


def test_select_mirror_keeps_ties_and_counts_only_new():
    key = np.array([[[0.5, 0.25, -1.0, 0.25], [0.75, 0.25, 0.9, -1.0]]], dtype=np.float32)
    mask, cnt, ties = R.select(key, 2)
    assert mask.tolist() == [[[0, 1, 0, 1], [0, 1, 0, 0]]] and cnt.tolist() == [[3, 6]] and ties.tolist() == [3]
    mask2, cnt2, _ = R.select(key, 4, into=mask)
    assert mask2.tolist() == [[[1, 1, 0, 1], [0, 1, 0, 0]]] and cnt2.tolist() == [[1, 6]]
    everything, cnt3, _ = R.select(key, 100)
    assert np.array_equal(everything, (key >= 0).astype(np.uint8)) and cnt3.tolist() == [[6, 6]]
    cm = np.array([[[1, 0], [0, 1]]], dtype=np.uint8)
    assert R.expand(cm, 3, 3, 2, 2).tolist() == [[[1, 1, 0], [1, 1, 0], [0, 0, 1]]]


# ------------------------------------------------------------------------------------------------------- argument rules
def test_public_functions_refuse_bad_arguments_before_the_library_is_called(monkeypatch):
    from uda_aerial_semantic_segmentation_research_amd import _operands as O, active as A
    calls = []
    for name in O.OPERANDS:
        if name.startswith(("udaseg_window_", "udaseg_acquire_", "udaseg_kth_")):
            monkeypatch.setitem(O._FN, name, lambda *a, _n=name: calls.append(_n) or 0)
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    z = torch.zeros(1, 5, 4, 4)
    key = torch.zeros(1, 4, 4)
    bad = [lambda: A.mode_filter(m, 17, 5), lambda: A.mode_filter(m, -1, 5), lambda: A.mode_filter(m, 1, 1),
           lambda: A.mode_filter(m, 1, 33), lambda: A.mode_filter(m, 1, 5, ignore_index=4), lambda: A.mode_filter(m, 1, 5, void=256),
           lambda: A.mode_filter(m.float(), 1, 5), lambda: A.mode_filter(m[0, 0], 1, 5), lambda: A.mode_filter("m", 1, 5),
           lambda: A.agreement(m, 17, 5), lambda: A.agreement(m.int(), 1, 5), lambda: A.impurity(m, 17, 5),
           lambda: A.impurity(m, 1, 33), lambda: A.impurity(m, 1, 5, ignore_index=3), lambda: A.impurity(m.float(), 1, 5),
           lambda: A.acquisition(z, radius=17), lambda: A.acquisition(z, kind="entropy"), lambda: A.acquisition(z[0]),
           lambda: A.acquisition(z.double()), lambda: A.acquisition(torch.zeros(1, 1, 4, 4)),
           lambda: A.acquisition(torch.zeros(1, 33, 4, 4)), lambda: A.acquisition(z, exclude=torch.zeros(1, 4, 4)),
           lambda: A.select(key, 0), lambda: A.select(key, 1.0), lambda: A.select(key, 0.0), lambda: A.select(key, -3),
           lambda: A.select(key, True), lambda: A.select(key, 2, cell=0), lambda: A.select(key, 2, cell=(4, 4, 4)),
           lambda: A.select(key.double(), 2), lambda: A.select(key[0], 2), lambda: A.select(key, 2, into=torch.zeros(1, 4, 4)),
           lambda: A.ActivePool(1), lambda: A.ActivePool(5, radius=17), lambda: A.ActivePool(5, kind="x"),
           lambda: A.ActivePool(5, budget=1.0), lambda: A.ActivePool(5, void=4), lambda: A.table_of(17)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    cpu = [lambda: A.mode_filter(m, 1, 5), lambda: A.agreement(m, 1, 5), lambda: A.impurity(m, 1, 5), lambda: A.acquisition(z),
           lambda: A.prepare(z), lambda: A.score_maps(m, key, 5), lambda: A.select(key, 2),
           lambda: A.ActivePool(5).query(torch.nn.Identity(), [0], torch.zeros(1, 4, 4, 3, dtype=torch.uint8))]
    for call in cpu:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert not calls


def test_table_and_budget_arithmetic():
    from uda_aerial_semantic_segmentation_research_amd import active as A
    for r in (0, 1, 16):
        t = A.table_of(r)
        assert t.dtype == np.float32 and t.shape == ((2 * r + 1) ** 2 + 1,) and np.array_equal(t, R.table(r)) and t[0] == 0 and t[1] == 0
    assert A.table_of(1)[9] == np.float32(9 * np.log(9.0))
    assert A.items_of(7, 100) == 7 and A.items_of(0.05, 100) == 5 and A.items_of(0.001, 100) == 1 and A.items_of(0.5, 7) == 3


def test_entry_points_refuse_bad_extents_before_any_launch():
    """rc < 0 and a message that names the argument, from the library itself: the pointers are host buffers nothing reads."""
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(n=2, h=4, w=4, radius=2, classes=5, ignore_index=255, kind=0, cell=2)

    def call(entry, **kw):
        a = {**good, **kw}
        head = (p, 0, a["n"], a["h"], a["w"], a["radius"], a["classes"], 1, a["ignore_index"])
        if entry == "window_mode":
            return lib.udaseg_window_mode(*head, 0, 255, p, p, p, None)
        if entry == "window_impurity":
            return lib.udaseg_window_impurity(*head, p, p, None)
        if entry == "acquire_score":
            return lib.udaseg_acquire_score(p, p, p, a["n"], a["h"], a["w"], a["radius"], a["classes"], a["kind"], p, p, p, None)
        if entry == "acquire_cells":
            return lib.udaseg_acquire_cells(p, a["n"], a["h"], a["w"], a["cell"], a["cell"], p, None)
        return lib.udaseg_acquire_expand(p, a["n"], a["h"], a["w"], a["cell"], a["cell"], p, None)

    grid = [(dict(n=0), b"n"), (dict(n=65536), b"n"), (dict(h=0), b"h"), (dict(h=1 << 16, w=1 << 15), b"2^31")]
    window = grid + [(dict(radius=17), b"radius"), (dict(radius=-1), b"radius"), (dict(classes=1), b"classes"),
                     (dict(classes=33), b"classes")]
    for entry, cases in (("window_mode", window + [(dict(ignore_index=256), b"ignore_index")]),
                         ("window_impurity", window + [(dict(ignore_index=-1), b"ignore_index")]),
                         ("acquire_score", window + [(dict(kind=3), b"kind")]),
                         ("acquire_cells", grid + [(dict(cell=0), b"cell")]), ("acquire_expand", grid + [(dict(cell=0), b"cell")])):
        for kw, word in cases:
            rc = call(entry, **kw)
            msg = lib.udaseg_last_error()
            assert rc < 0 and word in msg and entry.encode() in msg, (entry, kw, rc, msg)
    assert lib.udaseg_window_mode(None, 0, 2, 4, 4, 2, 5, 0, 0, 0, 255, p, None, None, None) < 0          # a missing operand
    assert lib.udaseg_window_mode(p, 0, 2, 4, 4, 2, 5, 0, 0, 2, 255, p, None, None, None) < 0             # fill_void
    assert lib.udaseg_acquire_prepare(p, 6, 5, 0, 16, p, p, p, None) < 0 and b"ldc" in lib.udaseg_last_error()
    assert lib.udaseg_acquire_prepare(p, 8, 1, 0, 16, p, p, p, None) < 0 and b"classes" in lib.udaseg_last_error()
    assert lib.udaseg_acquire_prepare(p, 36, 33, 0, 16, p, p, p, None) < 0
    assert lib.udaseg_acquire_prepare(p, 8, 5, 2, 16, p, p, p, None) < 0 and b"probs" in lib.udaseg_last_error()
    assert lib.udaseg_acquire_select(p, p, 2, 0, p, p, None) < 0 and b"items_per_image" in lib.udaseg_last_error()
    assert lib.udaseg_acquire_select(p, p, 0, 16, p, p, None) < 0
    assert lib.udaseg_window_tile(17) < 0 and lib.udaseg_window_tile(-1) < 0
    for r in (0, 1, 8, 9, 16):
        v = lib.udaseg_window_tile(r)
        assert v > 0 and (v & 0xffff) == 64 and (v >> 16) in (16, 32)


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def test_active_pool_bookkeeping_on_cpu_tensors():
    from uda_aerial_semantic_segmentation_research_amd import active as A
    n, h, w, r, classes = 2, 12, 17, 1, 5
    pool = A.ActivePool(classes, radius=r, budget=10)
    truth = torch.from_numpy(R.make_map(n, h, w, r, classes, seed=4))
    idx = [7, 3]
    assert pool.coverage() == {"per_frame": {}, "total": 0, "pixels": 0}
    assert (pool.sparse_masks(idx, truth) == 255).all() and not pool.requested_maps(idx, (h, w), "cpu").any()
    # round one, as query does it: score under the requested maps, select into them
    z = R.make_scores(n, h, w, r, classes, seed=2)
    lab, _, h32, _ = R.prepare(z, classes)
    before = pool.requested_maps(idx, (h, w), "cpu").numpy()
    key = R.score(lab, h32, r, classes, 0, exclude=before)[3]
    after, cnt1, _ = R.select(key, 10, into=before)
    for j, i in enumerate(idx):
        pool.requested[i] = torch.from_numpy(after[j])
    cov = pool.coverage()
    assert cov["per_frame"] == {3: int(after[1].sum()), 7: int(after[0].sum())} and cov["total"] == int(cnt1[:, 0].sum())
    assert cov["pixels"] == 2 * h * w and (cnt1[:, 0] >= 10).all()
    sparse = pool.sparse_masks(torch.tensor(idx), truth)
    assert sparse.dtype == torch.uint8 and np.array_equal(sparse.numpy(), np.where(after != 0, truth.numpy(), 255))
    assert np.array_equal(pool.sparse_masks(idx, truth.long()).numpy(), sparse.numpy())
    # round two: what was requested is excluded, and is not counted again
    before2 = pool.requested_maps(idx, (h, w), "cpu").numpy()
    assert np.array_equal(before2, after)
    key2 = R.score(lab, h32, r, classes, 0, exclude=before2)[3]
    assert (key2[before2 != 0] == -1).all()
    after2, cnt2, _ = R.select(key2, 10, into=before2)
    assert not ((after2 != 0) & (before2 != 0) & (key2 >= 0)).any() and int((after2 != 0).sum()) == cov["total"] + int(cnt2[:, 0].sum())
    assert (cnt2[:, 1] == cnt1[:, 1] - cnt1[:, 0]).all()
    # a frame the pool has not seen is all void; a loader yields (frames, sparse masks)
    assert (pool.sparse_masks([99], truth[:1]) == 255).all()
    frames = torch.zeros(n, h, w, 3, dtype=torch.uint8)
    batches = list(pool.loader([(idx, frames, truth)]))
    assert len(pool.loader([1, 2])) == 2 and batches[0][0] is frames and np.array_equal(batches[0][1].numpy(), sparse.numpy())
    # the checkpoint
    state = pool.state_dict()
    other = A.ActivePool(classes, radius=r, budget=10)
    other.load_state_dict(state)
    assert sorted(other.requested) == [3, 7] and all(other.requested[i].dtype == torch.uint8 for i in (3, 7))
    assert all(np.array_equal(other.requested[i].numpy(), pool.requested[i].numpy()) for i in (3, 7))
    assert other.coverage() == pool.coverage() and other.rounds == pool.rounds
    with pytest.raises(ValueError):
        A.ActivePool(6).load_state_dict(state)
    with pytest.raises(ValueError):
        pool.sparse_masks([7, 7], truth)
    with pytest.raises(ValueError):
        pool.requested_maps([7], (h + 1, w), "cpu")
