"""GPU checks of the regions module (regions.py, csrc/regions.hip) against its numpy mirror tests/_regions_ref.py.  Integers only:
every comparison is np.array_equal.  The maps are the ones tests/test_regions_host.py vets on the mirror (a component across two
seams, something removed and something kept by the sieve, 4- and 8-connectivity apart)."""
import functools

import numpy as np
import pytest
import torch

import _boundary_ref as BR
import _regions_ref as R

pytestmark = pytest.mark.gpu

C = R.CLASSES
MIN_AREA = 12
PER_CLASS = [0, 30, 3, 1, 500]


@pytest.fixture(scope="module")
def G():
    from uda_aerial_semantic_segmentation_research_amd import _lib, regions
    _lib.require_gpu()
    return regions


@functools.lru_cache(maxsize=None)
def _tile():
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    return K.regions_tile()


@functools.lru_cache(maxsize=None)
def _map(case):
    """uint8 [n,h,w] by name, made once: 'map:i' (shape i of R.shapes), 'struct:name' (three tiles and a bit), 'deep:name' (five)."""
    th, tw = _tile()
    kind, arg = case.split(":")
    if kind == "map":
        return R.make_map(*R.shapes((th, tw))[int(arg)])
    h, w = (3 * th + 5, 3 * tw + 7) if kind == "struct" else (5 * th + 3, 5 * tw + 1)
    return R.structure(arg, h, w, (th, tw))


@functools.lru_cache(maxsize=None)
def _reference(case, connectivity, ignore):
    """The mirror's ids and areas of a map, computed once and shared (treated as read-only)."""
    ids = R.ids(_map(case), connectivity, ignore)
    return ids, R.areas(ids)


def _dev(a, i64, seed=0):
    return torch.from_numpy(R.as_int64(a, seed) if i64 else a).cuda()


LABEL_CASES = [f"map:{i}" for i in range(8)] + [f"struct:{s}" for s in R.STRUCTURES] + ["deep:u", "deep:serpentine"]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("case", LABEL_CASES)
def test_ids_and_areas_match_the_mirror(G, case, i64, ignore, connectivity):
    m = _map(case)
    want_ids, want_area = _reference(case, connectivity, ignore)
    lab = _dev(m, i64)
    if i64 and (m == 255).any():
        assert bool(((lab < 0) | (lab > 255)).any())                           # the int64 variant holds out-of-range values
    ids, area = G.label(lab, connectivity, ignore, return_area=True)
    assert ids.dtype == torch.int32 and area.dtype == torch.int32 and tuple(ids.shape) == m.shape == tuple(area.shape)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(area.cpu().numpy(), want_area)
    if ignore is not None and (m == ignore).any():
        assert bool((ids[lab == ignore] == -1).all()) and bool((area[lab == ignore] == 0).all())
    only = G.label(lab, connectivity, ignore)
    assert torch.equal(only, ids)


def test_the_shapes_use_the_library_tile_and_every_merge_depth():
    th, tw = _tile()
    assert th >= 8 and tw >= 8
    sh = R.shapes((th, tw))
    assert sh[4] == (2, th + 1, tw + 1) and sh[5] == (1, 3 * th + 5, 3 * tw + 7) and sh[6] == (1, 5 * th + 3, 5 * tw + 1)
    assert _map("map:7").shape == (65, 9, 13) and (_map("map:7")[:-1, -1] == _map("map:7")[1:, 0]).all()
    ids4, _ = _reference("struct:u", 4, None)                                  # the U: one id, rooted at the top of its left arm
    u = _map("struct:u") == 7
    assert (ids4[u] == 2 * u.shape[2] + 5).all()


def test_label_without_an_area_buffer_and_twice(G):
    """The C entry point with area == NULL takes its own scratch; two runs on the random map return equal tensors."""
    from uda_aerial_semantic_segmentation_research_amd import kernels as K
    m = _map("struct:random")
    want, _ = _reference("struct:random", 8, None)
    lab = torch.from_numpy(m).cuda()
    ids = torch.full(m.shape, -7, dtype=torch.int32, device="cuda")
    K.regions_label(lab, 8, None, ids, None)
    assert np.array_equal(ids.cpu().numpy(), want)
    a, b = G.label(lab, 8, None, return_area=True), G.label(lab, 8, None, return_area=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], ids)


SIEVE_CASES = ["map:3", "map:4", "map:5", "map:7", "struct:random"]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("case", SIEVE_CASES)
def test_sieve_and_counts_match_the_mirror(G, case, i64, connectivity):
    m = _map(case)
    n = m.shape[0]
    lab = _dev(m, i64)
    counts = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    total = np.zeros((n, 3), dtype=np.int64)
    for thr, kw in ((MIN_AREA, dict(void=254, ignore_index=255)), (PER_CLASS, dict(void=254, ignore_index=None)),
                    (PER_CLASS, dict())):                                       # the last: a tensor of thresholds, void = ignore = 255
        want, wc = R.sieve(m, thr, connectivity, kw.get("void", 255), kw.get("ignore_index", kw.get("void", 255)))
        assert wc[:, 1].sum() > 0 and wc[:, 2].sum() > 0
        out = G.sieve(lab, thr if kw else torch.tensor(thr), connectivity, counts=counts, **kw)
        total += wc
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(counts.cpu().numpy(), total)                      # accumulates over the calls
    for thr in (0, 1):                                                          # nothing is smaller than one pixel
        out = G.sieve(lab, thr, connectivity, void=254, ignore_index=None)
        assert np.array_equal(out.cpu().numpy(), R.read(m).astype(np.uint8))


def test_sieve_of_a_single_map_and_into_a_buffer(G):
    m = _map("struct:diagonals")[0]
    lab = torch.from_numpy(m).cuda()
    out = G.sieve(lab, 2, connectivity=4, void=9)                               # an [H,W] map comes back as [H,W]
    assert tuple(out.shape) == m.shape and np.array_equal(out.cpu().numpy(), np.where(m >= 5, 9, m))
    assert np.array_equal(G.sieve(lab, 2, connectivity=8, void=9).cpu().numpy(), m)
    buf = torch.empty((1,) + m.shape, dtype=torch.uint8, device="cuda")
    assert G.sieve(lab[None], 15, connectivity=8, void=9, out=buf) is buf and np.array_equal(buf.cpu().numpy()[0], np.where(m >= 5, 9, m))
    ids = G.label(lab, 8)
    assert tuple(ids.shape) == m.shape
    with pytest.raises(ValueError):
        G.sieve(lab, 2, counts=torch.zeros((1, 2), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        G.sieve(lab, -2)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("ignore", [None, 255])
def test_region_stats_on_label_maps_and_on_scores(G, connectivity, ignore):
    maps = [_map("map:5"), _map("struct:random"), _map("map:7")]
    want = sum(R.stats(m, C, connectivity, ignore) for m in maps)
    st = G.RegionStats(C, connectivity, ignore)
    st.update(torch.from_numpy(maps[0]).cuda()).update(_dev(maps[1], True)).update(torch.from_numpy(maps[2]).cuda())
    got = st.compute()
    assert np.array_equal(got["stats"], want) and want[:, 0].min() >= 0 and want[:4, 0].min() > 0
    assert np.array_equal(got["components"], want[:, 0]) and np.array_equal(got["hist"], want[:, 2:])
    st.reset()
    assert st.compute()["stats"].sum() == 0
    # scores: the arg-max path.  Labels below the class count only (a score map cannot say 255); the first maximum wins a tie.
    m = np.minimum(_map("map:4"), C - 1)
    scores = np.zeros((m.shape[0], C) + m.shape[1:], dtype=np.float32)
    np.put_along_axis(scores, m[:, None].astype(np.int64), 1.0, axis=1)
    scores[:, C - 1] = np.maximum(scores[:, C - 1], (m == 2) * 1.0)             # a tie of classes 2 and C - 1: 2 is first
    sc = G.RegionStats(C, connectivity, ignore).update(torch.from_numpy(scores).cuda()).compute()
    assert np.array_equal(sc["stats"], R.stats(m, C, connectivity, ignore))


def test_sieved_loader_and_its_composition_with_the_eroded_loader(G):
    from uda_aerial_semantic_segmentation_research_amd import boundary as B
    maps = [_map("map:4"), _map("map:5")]
    frames = [torch.full((m.shape[0], 3) + m.shape[1:], 7 + i, dtype=torch.uint8, device="cuda") for i, m in enumerate(maps)]
    batches = [(f, torch.from_numpy(m) if i else torch.from_numpy(m).cuda()) for i, (f, m) in enumerate(zip(frames, maps))]
    ld = G.SievedLoader(batches, PER_CLASS, connectivity=8, void=255)
    assert len(ld) == 2
    for i, (f, out) in enumerate(ld):
        want, wc = R.sieve(maps[i], PER_CLASS, 8, 255, 255)
        assert f is frames[i] and bool((f == 7 + i).all())
        assert out.is_cuda and np.array_equal(out.cpu().numpy(), want)
        assert ld.last_counts.is_cuda and np.array_equal(ld.last_counts.cpu().numpy(), wc)
    for f, out in G.SievedLoader(B.ErodedLoader(batches, 1), MIN_AREA):
        i = int(f[0, 0, 0, 0]) - 7
        assert np.array_equal(out.cpu().numpy(), R.sieve(BR.erode(maps[i], 1, 255, 255)[0], MIN_AREA, 4, 255, 255)[0])
    for f, out in B.ErodedLoader(G.SievedLoader(batches, MIN_AREA), 1):
        i = int(f[0, 0, 0, 0]) - 7
        assert np.array_equal(out.cpu().numpy(), BR.erode(R.sieve(maps[i], MIN_AREA, 4, 255, 255)[0], 1, 255, 255)[0])
    with pytest.raises(ValueError):
        next(iter(G.SievedLoader([torch.zeros(2)], 2)))


def test_evaluate_counts_predictions_and_truth_in_one_pass(G):
    m = np.minimum(_map("map:4"), C - 1)
    truth = torch.from_numpy(m)
    scores = torch.zeros((m.shape[0], C) + m.shape[1:])
    scores.scatter_(1, truth[:, None].long(), 1.0)
    shifted = torch.roll(scores, 1, dims=3)

    class Fixed(torch.nn.Module):
        def forward(self, x):
            return x

    res = G.evaluate(Fixed(), [(shifted, truth), (scores, truth.long())], C, "cuda", connectivity=8, ignore_index=None)
    pm = np.roll(m, 1, axis=2)
    assert np.array_equal(res["pred"]["stats"], R.stats(pm, C, 8) + R.stats(m, C, 8))
    assert np.array_equal(res["truth"]["stats"], 2 * R.stats(m, C, 8))
    t = res["truth"]["components"].astype(np.float64)
    assert np.array_equal(np.isnan(res["ratio"]), t == 0) and np.array_equal(res["ratio"][t > 0], (res["pred"]["components"] / t)[t > 0])
