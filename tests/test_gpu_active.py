"""GPU checks of the active-labelling module (active.py, csrc/window.hip) against its numpy mirror tests/_active_ref.py.  Integer
products (votes, agreement through an int32 view, counters, winners, masks) bit for bit; float products graded with
tests/_grade.py's bar max(4 x the fp32 mirror's worst deviation from float64, 2^-22), errors relative to 1 because every output
lies in [0, 1].  tests/test_active_host.py vets the inputs."""
import functools

import numpy as np
import pytest
import torch

import _active_ref as R
from _grade import Grader

pytestmark = pytest.mark.gpu


class ActiveGrader(Grader):
    PREFIX = "active-grade"


@pytest.fixture(scope="module")
def A():
    from uda_aerial_semantic_segmentation_research_amd import _lib, active
    _lib.require_gpu()
    return active


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import kernels
    return kernels


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _label_reference(case, ignore):
    """The map of a case and the mirror's products of it, computed once and shared (treated as read-only)."""
    n, h, w, r, classes = case
    m = R.make_map(n, h, w, r, classes)
    nc = R.counts(m, r, classes, ignore)[0]
    return {"map": m, "mode": R.mode(m, r, classes, ignore, False, 254), "fill": R.mode(m, r, classes, ignore, True, 254),
            "impurity": R.impurity_of_counts(nc, classes, r)}


@functools.lru_cache(maxsize=None)
def _score_reference(case, probs):
    n, h, w, r, classes = case
    z = R.make_scores(n, h, w, r, classes, probs=probs)
    return {"scores": z, "prepare": R.prepare(z, classes, probs)}


# ------------------------------------------------------------------------------------------------------- integer products
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("case", R.CASES)
def test_votes_match_the_mirror(A, case, i64, ignore):
    n, h, w, r, classes = case
    ref = _label_reference(case, ignore)
    m = torch.from_numpy(R.as_int64(ref["map"]) if i64 else ref["map"]).cuda()
    for fill, name in ((False, "mode"), (True, "fill")):
        want, agr, cnt = ref[name]
        counts = torch.full((n, 3), 7, dtype=torch.int64, device="cuda")
        out = torch.full((n, h, w), 99, dtype=torch.uint8, device="cuda")          # a sentinel no product holds
        got, got_agr = A.mode_filter(m, r, classes, ignore_index=ignore, fill_void=fill, counts=counts, return_agreement=True,
                                     void=254, out=out)
        assert got is out and got.dtype == torch.uint8 and np.array_equal(_np(got), want)
        assert got_agr.dtype == torch.float32 and np.array_equal(_bits(got_agr), _bits(agr))
        assert np.array_equal(_np(counts), 7 + cnt)
    assert np.array_equal(_bits(A.agreement(m, r, classes, ignore)), _bits(ref["mode"][1]))


@pytest.mark.parametrize("probs", [False, True])
@pytest.mark.parametrize("case", R.CASES)
def test_winners_and_entropy(A, case, probs):
    n, h, w, r, classes = case
    ref = _score_reference(case, probs)
    lab, h64, h32, cnt = ref["prepare"]
    counters = torch.full((2,), 3, dtype=torch.int64, device="cuda")
    got_lab, got_h = A.prepare(torch.from_numpy(ref["scores"]).cuda(), probs, counters)
    assert got_lab.dtype == torch.uint8 and np.array_equal(_np(got_lab), lab) and np.array_equal(_np(counters), 3 + cnt)
    g = ActiveGrader(f"{case} probs={int(probs)}")
    g.grade("entropy", _np(got_h), h64, h32, np.ones_like(h64))
    g.done()
    assert (_np(got_h)[lab == 255] == 0).all()


# --------------------------------------------------------------------------------------------------------- float products
@pytest.mark.parametrize("case", R.CASES)
def test_float_products_meet_the_bar(A, K, case):
    n, h, w, r, classes = case
    g = ActiveGrader(str(case))
    one = np.ones((n, h, w))
    ref = _label_reference(case, 255)
    i64, i32 = ref["impurity"]
    for dt in (False, True):
        m = torch.from_numpy(R.as_int64(ref["map"]) if dt else ref["map"]).cuda()
        out = torch.full((n, h, w), -7.0, device="cuda")
        assert A.impurity(m, r, classes, out=out) is out
        g.grade(f"impurity i64={int(dt)}", _np(out), i64, i32, one)
    z = torch.from_numpy(_score_reference(case, False)["scores"]).cuda()
    exclude = torch.from_numpy((np.random.RandomState(5).rand(n, h, w) < 0.1).astype(np.uint8)).cuda()
    for kind, name in enumerate(("ripu", "impurity", "uncertainty")):
        score, key, lab = A.acquisition(z, radius=r, kind=name, exclude=exclude)
        lab_np, ent_np = _np(lab), _np(A.prepare(z)[1])                        # graded from what the device itself produced
        s64, k64, s32, k32, cand = R.score(lab_np, ent_np, r, classes, kind, exclude=_np(exclude))
        key_np = _np(key)
        assert np.array_equal(key_np >= 0, cand) and (key_np[~cand] == -1).all() and (_np(score)[~cand] == 0).all()
        g.grade(f"score {name}", _np(score), s64, s32, one)
        g.grade(f"key {name}", key_np, k64, k32, one)
        if kind == 0 and h * w > 1:
            ch, cw = (8, 8) if min(h, w) >= 8 else (2, 3)
            gh, gw = -(-h // ch), -(-w // cw)
            cell_key = torch.full((n, gh, gw), -7.0, device="cuda")
            K.acquire_cells(key, ch, cw, cell_key)
            c64, c32, has = R.cells(key_np, ch, cw)
            ck = _np(cell_key)
            assert np.array_equal(ck >= 0, has) and (ck[~has] == -1).all()
            g.grade("cells", ck, c64, c32, np.ones_like(c64))
    g.done()


@pytest.mark.parametrize("r", [1, 16])
def test_straight_edges_on_each_side_of_every_tile_seam(A, K, r):
    """One vertical and one horizontal two-class edge per image, at the column / row before, on and after every seam of the
    launch's tile, in a map of 2 th + 5 by 2 tw + 7 pixels."""
    th, tw = K.window_tile(r)
    h, w = 2 * th + 5, 2 * tw + 7
    cols = [s + o for s in (tw, 2 * tw) for o in (-1, 0, 1)]
    rows = [s + o for s in range(th, h, th) for o in (-1, 0, 1) if s + o < h]
    m = np.zeros((len(cols) + len(rows), h, w), dtype=np.uint8)
    for i, c in enumerate(cols):
        m[i, :, c:] = 1
    for j, c in enumerate(rows):
        m[len(cols) + j, c:, :] = 2
    want, agr, cnt = R.mode(m, r, 3, 255, False, 255)
    i64, i32 = R.impurity(m, r, 3, 255)
    assert (i64 > 0).any() and (i64 == 0).any() and (cnt[:, 1:] == 0).all()    # (a strip thinner than the radius is outvoted)
    for dev in (torch.from_numpy(m).cuda(), torch.from_numpy(m).cuda().long()):
        counts = torch.zeros((len(m), 3), dtype=torch.int64, device="cuda")
        got, got_agr = A.mode_filter(dev, r, 3, return_agreement=True, counts=counts)
        assert np.array_equal(_np(got), want) and np.array_equal(_bits(got_agr), _bits(agr)) and np.array_equal(_np(counts), cnt)
        g = ActiveGrader(f"seams r={r} {dev.dtype}")
        g.grade("impurity", _np(A.impurity(dev, r, 3)), i64, i32, np.ones_like(i64))
        g.done()
    x = np.arange(r, w - r)                                                    # and the closed form across a vertical edge
    c = cols[1]
    q = np.clip(np.where(x < c, x + r - c + 1, c - (x - r)), 0, 2 * r + 1) / (2 * r + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        closed = -(np.where(q > 0, q * np.log(q), 0) + np.where(q < 1, (1 - q) * np.log(1 - q), 0)) / np.log(3)
    assert np.abs(i64[1, :, r:w - r] - closed[None, :]).max() < 1e-12


# -------------------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("case", R.SELECT_CASES)
def test_selection_matches_the_mirror(A, K, case):
    n, h, w, r, classes, kind, budget, cell = case
    z = torch.from_numpy(R.make_scores(n, h, w, r, classes)).cuda()
    exclude = (np.random.RandomState(3).rand(n, h, w) < 0.1).astype(np.uint8)
    _, key, _ = A.acquisition(z, radius=r, kind=("ripu", "impurity", "uncertainty")[kind], exclude=torch.from_numpy(exclude).cuda())
    key_np = _np(key)
    assert (key_np[exclude != 0] == -1).all() and (key_np >= 0).any()
    if cell is None:
        items_key, items = key_np, h * w
    else:
        gh, gw = -(-h // cell[0]), -(-w // cell[1])
        assert h % cell[0] and w % cell[1]                                     # ragged edge cells
        cell_key = torch.empty((n, gh, gw), device="cuda")
        K.acquire_cells(key, cell[0], cell[1], cell_key)
        items_key, items = _np(cell_key), gh * gw
    k = A.items_of(budget, items)
    sel, cnt, ties = R.select(items_key, k)
    want = sel if cell is None else R.expand(sel, h, w, *cell)
    mask, counts = A.select(key, budget, cell=cell)
    assert mask.dtype == torch.uint8 and np.array_equal(_np(mask), want) and np.array_equal(_np(counts), cnt)
    assert (cnt[:, 0] > 0).all() and (cnt[:, 0] < cnt[:, 1]).all() and (cnt[:, 0] >= k).all() and (cnt[:, 0] <= k + ties - 1).all()
    # into= carries earlier selections (the first row among them, whatever its keys): the mask is OR-ed into, only new items count
    earlier = _np(mask).copy()
    earlier[:, 0, :] = 1
    into = torch.from_numpy(earlier).cuda()
    k2 = 3 * k
    sel2, cnt2, _ = R.select(items_key, k2, into=None if cell is not None else earlier)
    mask2, counts2 = A.select(key, k2, cell=cell, into=into)
    assert mask2 is into
    want2 = (sel2 if cell is None else R.expand(sel2, h, w, *cell)) | earlier
    assert np.array_equal(_np(mask2), want2) and np.array_equal(_np(counts2), cnt2) and (_np(mask2)[:, 0, :] == 1).all()
    # a budget above the number of candidates selects exactly the candidates
    everything, counts3 = A.select(key, 10 ** 6, cell=cell)
    all_items = (items_key >= 0).astype(np.uint8)
    assert np.array_equal(_np(everything), all_items if cell is None else R.expand(all_items, h, w, *cell))
    assert np.array_equal(_np(counts3)[:, 0], _np(counts3)[:, 1]) and np.array_equal(_np(counts3)[:, 1], all_items.reshape(n, -1).sum(1))


# ------------------------------------------------------------------------------------------------ determinism and hygiene
def test_second_calls_give_the_same_bits_and_padding_is_never_read(A, K):
    n, h, w, r, classes = 2, 33, 65, 2, 23
    z = torch.from_numpy(R.make_scores(n, h, w, r, classes)).cuda()
    m = torch.from_numpy(R.make_map(n, h, w, r, classes)).cuda()
    twice = []
    for _ in range(2):
        mode, agr = A.mode_filter(m, r, classes, fill_void=True, return_agreement=True)
        score, key, lab = A.acquisition(z, radius=r)
        mask, counts = A.select(key, 0.05)
        cmask, ccounts = A.select(key, 0.2, cell=(8, 8))
        twice.append([_np(mode), _bits(agr), _bits(A.impurity(m, r, classes)), _bits(score), _bits(key), _np(lab), _np(mask),
                      _np(counts), _np(cmask), _np(ccounts)])
    assert all(np.array_equal(a, b) for a, b in zip(*twice))
    # padded score rows with NaN in the padding channels: the same labels, entropy and counters as the tight rows
    pixels, ld_tight, ld_wide = n * h * w, 24, 28
    rows = z.permute(0, 2, 3, 1).reshape(pixels, classes)
    outs = []
    for ld in (ld_tight, ld_wide):
        buf = torch.full((pixels, ld), float("nan"), device="cuda")
        buf[:, :classes] = rows
        lab = torch.full((pixels,), 77, dtype=torch.uint8, device="cuda")
        ent = torch.full((pixels,), -7.0, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        K.acquire_prepare(buf, ld, classes, False, pixels, lab, ent, cnt)
        outs.append((_np(lab), _bits(ent), _np(cnt)))
    assert all(np.array_equal(a, b) for a, b in zip(*outs)) and outs[0][2].sum() == pixels and outs[0][2][1] > 0
    assert np.array_equal(outs[0][0].reshape(n, h, w), twice[0][5]) and not (outs[0][0] == 77).any()
    # a [H,W] map comes back as [H,W]
    assert tuple(A.mode_filter(m[0], r, classes).shape) == (h, w) and tuple(A.impurity(m[0], r, classes).shape) == (h, w)


def test_score_key_and_agreement_overwrite_every_element(A, K):
    """The entry points called directly on sentinel-filled buffers (active.py allocates these three itself, and a recycled block
    could hold an earlier call's correct result), at a shape with ragged tiles in both directions."""
    n, h, w, r, classes = 2, 37, 70, 2, 23
    m = R.make_map(n, h, w, r, classes)
    z = R.make_scores(n, h, w, r, classes)
    lab, _, h32, _ = R.prepare(z, classes)
    tab = torch.from_numpy(A.table_of(r)).cuda()
    score = torch.full((n, h, w), -7.0, device="cuda")
    key = torch.full((n, h, w), -7.0, device="cuda")
    K.acquire_score(torch.from_numpy(lab).cuda(), torch.from_numpy(h32).cuda(), None, r, classes, 0, tab, score, key)
    s64, k64, s32, k32, cand = R.score(lab, h32, r, classes, 0)
    assert not (_np(score) == -7.0).any() and not (_np(key) == -7.0).any() and np.array_equal(_np(key) >= 0, cand)
    g = ActiveGrader("sentinel (2, 37, 70, 2, 23)")
    g.grade("score", _np(score), s64, s32, np.ones_like(s64))
    g.grade("key", _np(key), k64, k32, np.ones_like(k64))
    g.done()
    out = torch.full((n, h, w), 99, dtype=torch.uint8, device="cuda")
    agr = torch.full((n, h, w), -7.0, device="cuda")
    K.window_mode(torch.from_numpy(m).cuda(), r, classes, 255, False, 254, out, agr, None)
    want, want_agr, _ = R.mode(m, r, classes, 255, False, 254)
    assert np.array_equal(_np(out), want) and np.array_equal(_bits(agr), _bits(want_agr))


def test_an_entropy_above_one_keeps_its_pixel_a_candidate(A, K):
    """The fp32 entropy of a uniform row may be 1 + 1 ulp; A is capped at 1, so the key is 0 and not below, and the most uncertain
    pixel stays in the selection.  Once from uniform logits, once from an entropy map that is above 1 by construction."""
    n, h, w, classes = 1, 9, 13, 23
    for probs, z in ((False, torch.zeros(n, classes, h, w)), (True, torch.full((n, classes, h, w), 1.0 / classes))):
        for kind in ("uncertainty", "ripu"):
            score, key, lab = A.acquisition(z.cuda(), radius=1, kind=kind, probs=probs)
            k, sc = _np(key), _np(score)
            if kind == "uncertainty":
                assert (k >= 0).all() and (k <= 2.0 ** -18).all() and (sc <= 1).all() and (sc >= 1 - 2.0 ** -18).all()
            else:
                assert (k == -1).all() and (sc == 0).all() and (_np(lab) == 0).all()      # one label everywhere: impurity 0
    lab = torch.from_numpy((np.indices((h, w)).sum(0) % 2).astype(np.uint8)[None]).cuda()
    above = torch.full((n, h, w), float(np.nextafter(np.float32(1), np.float32(2))), device="cuda")
    tab = torch.from_numpy(A.table_of(1)).cuda()
    for kind in (2, 0):
        score, key = torch.empty((n, h, w), device="cuda"), torch.empty((n, h, w), device="cuda")
        K.acquire_score(lab, above, None, 1, 2, kind, tab, score, key)
        s64, k64, s32, k32, cand = R.score(_np(lab), _np(above), 1, 2, kind)
        g = ActiveGrader(f"entropy above one, kind {kind}")
        g.grade("score", _np(score), s64, s32, np.ones_like(s64))
        g.grade("key", _np(key), k64, k32, np.ones_like(k64))
        g.done()
        assert cand.all() and (_np(key) >= 0).all() and (_np(score) <= 1).all()
        if kind == 2:
            assert (_np(key) == 0).all() and (_np(score) == 1).all()
        mask, counts = A.select(key, 5)
        assert _np(counts)[0, 1] == h * w and _np(counts)[0, 0] >= 5


def test_agreement_is_a_pixel_weight_of_the_soft_cross_entropy(A):
    from uda_aerial_semantic_segmentation_research_amd.losses import SoftCrossEntropyLoss
    g = torch.Generator().manual_seed(4)
    n, c, h, w, r = 2, 5, 16, 16, 1
    m = R.make_map(n, h, w, r, c, seed=2)
    logits = torch.randn(n, c, h, w, generator=g).cuda()
    teacher = torch.randn(n, c, h, w, generator=g).cuda()
    wm = A.agreement(torch.from_numpy(m).cuda(), r, c)
    ref_w = R.mode(m, r, c, 255, False, 255)[1]
    assert np.array_equal(_bits(wm), _bits(ref_w)) and (ref_w < 1).any() and (ref_w == 1).any()
    loss_fn = SoftCrossEntropyLoss(reduction="weighted_mean")
    a = loss_fn(logits, teacher, pixel_weight=wm)
    assert torch.isfinite(a) and not np.array_equal(_bits(a), _bits(loss_fn(logits, teacher)))


# -------------------------------------------------------------------------------------------------------------- end to end
def test_pool_queries_twice_and_trains_on_the_sparse_masks(A):
    from uda_aerial_semantic_segmentation_research_amd import data as D
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(21)
    g = torch.Generator().manual_seed(6)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=5)
    crit = CrossEntropyLoss(ignore_index=255)
    tr = SegmentationTrainer(net, torch.device("cuda", 0), criterion=crit)
    net.train()
    frames = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8).cuda()
    truth = torch.randint(0, 5, (2, 64, 64), generator=g, dtype=torch.uint8).cuda()
    budget = 50
    pool = A.ActivePool(5, radius=1, kind="ripu", budget=budget)
    idx = [4, 9]
    first = pool.query(net, idx, frames)
    c1 = _np(pool.last_counts)
    second = pool.query(net, idx, frames)
    c2 = _np(pool.last_counts)
    assert net.training and first.dtype == torch.uint8 and tuple(first.shape) == (2, 64, 64)
    f, s = _np(first), _np(second)
    assert not (f & s).any() and (f.reshape(2, -1).sum(1) == c1[:, 0]).all() and (s.reshape(2, -1).sum(1) == c2[:, 0]).all()
    assert (c1[:, 0] >= budget).all() and (c2[:, 0] >= budget).all() and (c2[:, 1] == c1[:, 1] - c1[:, 0]).all()
    # within budget + ties: the tie group of the device's own keys at the threshold
    net.eval()
    with torch.no_grad():
        out = net(D.prepare_batch(frames)[0])
    net.train()
    _, key, _ = A.acquisition(out, radius=1)
    _, cnt, ties = R.select(_np(key), budget)
    assert np.array_equal(cnt, c1) and (c1[:, 0] <= budget + ties - 1).all()
    # ... and the second round's, whose key was made under the first round's requests
    _, key2, _ = A.acquisition(out, radius=1, exclude=first)
    sel2, cnt2, ties2 = R.select(_np(key2), budget)
    assert (_np(key2)[f != 0] == -1).all() and np.array_equal(cnt2, c2) and (c2[:, 0] <= budget + ties2 - 1).all()
    assert np.array_equal(sel2, s)
    cov = pool.coverage()
    requested = int(c1[:, 0].sum() + c2[:, 0].sum())
    assert cov["total"] == requested and cov["per_frame"] == {4: int(c1[0, 0] + c2[0, 0]), 9: int(c1[1, 0] + c2[1, 0])}
    sparse = pool.sparse_masks(idx, truth)
    assert int((sparse != 255).sum()) == requested and torch.equal(sparse[sparse != 255], truth[sparse != 255])
    images, masks = D.prepare_batch(frames, sparse)
    loss, _ = tr.train_step(images, masks, FusedAdam(net.parameters(), lr=1e-4))
    n_valid, n_void, n_invalid = crit.last_target_stats.tolist()
    assert np.isfinite(float(loss.detach())) and n_valid == requested and n_invalid == 0 and n_valid + n_void == 2 * 64 * 64
    # a frame that is requested in full selects nothing and does not raise
    pool.requested[4] = torch.ones(64, 64, dtype=torch.uint8, device="cuda")
    third = pool.query(net, idx, frames)
    assert not _np(third)[0].any() and _np(pool.last_counts)[0].tolist() == [0, 0] and _np(third)[1].any()
    state = pool.state_dict()
    other = A.ActivePool(5, budget=budget)
    other.load_state_dict(state, device="cuda")
    assert all(torch.equal(other.requested[i], pool.requested[i]) for i in idx) and other.coverage() == pool.coverage()


def test_select_counts_accumulate_per_image_and_an_image_without_candidates_adds_nothing(K):
    """acquire_select's counters at 2 x 1500 items (two blocks an image, a ragged last wave), into a buffer that holds 5 already: image
    0 selects by the mirror's threshold, image 1 has no candidate and keeps its 5 (no atomic is issued for it)."""
    rs = np.random.RandomState(21)
    key = rs.rand(2, 1500).astype(np.float32)
    key[0, ::5] = -1.0
    key[1] = -1.0
    k = 300
    sel, cnt, _ = R.select(key, k)
    assert cnt[0, 0] >= k and cnt[0, 1] == 1200 and cnt[1].tolist() == [0, 0]
    thr = np.array([np.sort(key[0][key[0] >= 0])[k - 1], 0.5], dtype=np.float32)
    mask = torch.zeros((2, 1500), dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 2), 5, dtype=torch.int64, device="cuda")
    K.acquire_select(torch.from_numpy(key).cuda(), torch.from_numpy(thr).cuda(), mask, counts)
    assert np.array_equal(_np(mask), sel) and np.array_equal(_np(counts), 5 + cnt)
    K.acquire_select(torch.from_numpy(key).cuda(), torch.from_numpy(thr).cuda(), mask, counts)     # nothing is new the second time
    assert np.array_equal(_np(mask), sel) and np.array_equal(_np(counts), 5 + cnt + np.array([[0, 1200], [0, 0]]))
