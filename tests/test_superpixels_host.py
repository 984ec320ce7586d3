"""CPU checks of the superpixel module: the numpy mirror (tests/_superpixels_ref.py) against brute-force restatements on tiny
shapes, the overflow bounds of the rule at its extreme arguments, the properties that keep tests/test_gpu_superpixels.py from being
vacuous (every superpixel 4-connected, the fragment-heavy cases really absorbing over long chains, the clean frames voting their
regions back), the host-side argument rules of superpixels.py and regions.label_ids, and the argument rules of the new entry
points, which refuse bad arguments with rc < 0 and a message before any launch (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

import _superpixels_ref as R


# ------------------------------------------------------------------------------------------------- mirror against brute force
@pytest.mark.parametrize("shape,S,m", [((7, 9), 2, 10), ((9, 9), 16, 10), ((5, 24), 8, 1), ((13, 11), 4, 1024), ((12, 12), 3, 40)])
def test_mirror_equals_brute_force(shape, S, m):
    h, w = shape
    for kind in ("voronoi", "random", "constant"):
        if kind == "voronoi":
            frame = R.voronoi(1, h, w, 3, noise=6, seed=S)[0][0]
        elif kind == "random":
            frame = R.random_frame(1, h, w, seed=S)[0]
        else:
            frame = R.constant(1, h, w)[0]
        c = R.start_centres(frame, S)
        gh, gw = R.grid_of(h, w, S)
        assert c.shape == (gh * gw, 6) and (c[:, 5] == 0).all()
        assert c[0, 0] == 16 * min(S // 2, h - 1) and c[-1, 1] == 16 * min((gw - 1) * S + S // 2, w - 1)
        for _ in range(3):
            lab = R.assign(frame, c, S, m)
            assert np.array_equal(lab, R.assign_brute(frame, c, S, m)), (kind, shape, S)
            gy, gx = np.divmod(lab, gw)                      # a pixel's cluster lies in the 3 x 3 cells around its own
            y, x = np.mgrid[0:h, 0:w]
            assert (np.abs(gy - y // S) <= 1).all() and (np.abs(gx - x // S) <= 1).all()
            c = R.update(frame, lab, c)
            assert c[:, 5].sum() == h * w and c[:, 5].max() <= 9 * S * S
        for min_area in (0, 3, S * S):
            ids, counts, _ = R.connect(lab, min_area)
            assert np.array_equal(ids, R.connect_brute(lab, min_area)), (kind, shape, S, min_area)
            assert counts[3] == counts[0] - counts[1] == len(np.unique(ids))
        if kind == "constant":                               # every colour ties: the distance alone decides, then the smallest k
            assert np.array_equal(R.assign(frame, R.start_centres(frame, S), S, m),
                                  R.assign_brute(frame, R.start_centres(frame, S), S, m))


def test_update_rounds_to_nearest_and_keeps_an_empty_centre():
    frame = np.zeros((4, 4, 3), dtype=np.uint8)
    frame[..., 0] = np.arange(16).reshape(4, 4)
    c = R.start_centres(frame, 2)
    lab = np.zeros((4, 4), dtype=np.int64)
    lab[0, :3] = 1                                           # cluster 1: pixels (0,0), (0,1), (0,2); clusters 2, 3 empty
    out = R.update(frame, lab, c)
    assert out[1].tolist() == [0, (16 * 3 + 1) // 3, (16 * 3 + 1) // 3, 0, 0, 3]
    assert out[2, :5].tolist() == c[2, :5].tolist() and out[2, 5] == 0 and out[0, 5] == 13


def test_overflow_bounds_at_the_extreme_arguments():
    S, m, side = 64, 1024, 32768
    # a pixel and the centre of a candidate cluster: the cluster's pixels lie within its 3 x 3 cells and the pixel within one cell
    # of the cluster's, so they are less than 3 S apart on either axis; colours differ by at most 255
    d_space, d_colour = 16 * 3 * S, 16 * 255
    D = S * S * 3 * d_colour ** 2 + m * m * 2 * d_space ** 2
    assert D < 2.1e13 and D < 2 ** 63
    assert 3 * d_colour ** 2 < 2 ** 31                       # the colour part is summed in 32 bits on the device
    assert 9 * S * S == 36864 and 36864 * (side - 1) < 2 ** 31 and 36864 * 255 < 2 ** 31      # the int32 sums
    assert 16 * 36864 * (side - 1) + 36864 // 2 < 2 ** 63    # the update's numerator, formed in 64 bits
    assert 16 * (side - 1) < 2 ** 31 and (side // 2) ** 2 == 2 ** 28                          # centres; K at step 2
    assert 64 * (side - 1) < 2 ** 21 and 64 * 255 < 2 ** 14  # the packed per-wave sums of the assign pass
    assert 2 ** 31 * (2 ** 24 + 1) < 2 ** 63                 # the mean's int64 sum over a whole image
    # the extreme colours really reach the colour bound in the mirror, at the largest step and compactness
    frame = np.zeros((3, 130, 3), dtype=np.uint8)
    frame[:, 64:] = 255
    c = R.start_centres(frame, S)
    lab = R.assign(frame, c, S, m)
    assert np.array_equal(lab, R.assign_brute(frame, c, S, m)) and lab.max() == 2


# ------------------------------------------------------------------------------------------- properties of the shared cases
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_superpixel_of_every_case_is_connected(name):
    n, h, w, S = R.CASES[name][:4]
    ids, cen, counts, info = R.reference(name)
    gh, gw = R.grid_of(h, w, S)
    assert ids.min() >= 0 and ids.max() < gh * gw and cen.shape == (n, gh * gw, 6)
    for i in range(n):
        assert R.n_components(ids[i]) == len(np.unique(ids[i])) == counts[i, 3], name
        assert len(np.unique(info["labels"][i])) == counts[i, 3]                # min_area = 0: every non-empty cluster survives
    ids_a, _, counts_a, _ = R.reference(name, S * S // 4)
    for i in range(n):
        assert R.n_components(ids_a[i]) == len(np.unique(ids_a[i])) == counts_a[i, 3], name
    if n > 1:
        frames = R.case(name)[0]
        assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(ids[0], ids[1])


def test_the_cases_cover_what_their_names_say():
    assert R.reference("one_cluster")[0].max() == 0
    assert R.grid_of(5, 40, 8)[0] == 1
    for name in R.FRAGMENT_HEAVY:
        counts, chains = R.reference(name)[2], R.reference(name)[3]["chains"]
        assert counts[0, 1] > 1000 and counts[0, 2] > 1000 and max(chains) >= 8, (name, counts, chains)
    assert R.reference("random", 16)[2][0, 3] < 48                              # with min_area whole clusters vanish on noise
    n, h, w, S = R.CASES["constant"][:4]
    c = R.start_centres(R.case("constant")[0][0], S)                            # a constant frame: pixels with two nearest centres
    tie = 0
    for yy in range(h):
        for xx in range(w):
            d = sorted(((16 * yy - Y) ** 2 + (16 * xx - X) ** 2) for Y, X in c[:, :2].tolist())
            tie += d[0] == d[1]
    assert tie > 0
    h, w = R.CASES["fragments"][1:3]
    assert -(-h // 64) >= 3 and -(-w // 64) >= 4                                # 3 x 4 tiles of the labelling: two merge levels


@pytest.mark.parametrize("name", sorted(R.ROUND_TRIP))
def test_clean_frames_vote_their_regions_back(name):
    n, h, w, S, seeds = R.ROUND_TRIP[name]
    frames, regions = R.voronoi(n, h, w, seeds)
    ids = R.slic(frames, S, R.COMPACTNESS, R.ITERATIONS)[0]
    gh, gw = R.grid_of(h, w, S)
    out, counts = R.vote(ids, regions, seeds, K=gh * gw)
    assert np.array_equal(out, regions) and counts.sum() == 0
    assert len(np.unique(regions)) == seeds


def test_vote_and_mean_mirrors_on_a_hand_made_map():
    ids = np.array([[[0, 0, 1, 1], [0, 0, 1, 2]]])
    m = np.array([[[1, 1, 0, 2], [0, 255, 1, 9]]], dtype=np.uint8)
    out, c = R.vote(ids, m, 3, K=3)
    assert out[0].tolist() == [[1, 1, 0, 0], [1, 1, 0, 255]] and c.tolist() == [[3, 1, 0]]      # cluster 1 ties three ways: class 0
    out, c = R.vote(ids, m, 3, min_share=0.7, K=3)
    assert out[0].tolist() == [[255] * 4, [255] * 4] and c.tolist() == [[0, 0, 6]]
    out, c = R.vote(ids, m, 3, min_cover=1.0, void=7, K=3)
    assert out[0].tolist() == [[7, 7, 0, 0], [7, 7, 0, 7]] and c.tolist() == [[2, 0, 3]]
    v = np.array([[[0.5, 0.25, 1.0, np.nan], [-1.0, 0.0, 1.0, 2.0]]], dtype=np.float32)
    assert R.mean(v, ids, 4).tolist() == [[0.25, 1.0, -1.0, -1.0]]
    mask, counts = R.select(v, ids, 3, 1)
    assert mask[0].tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]] and counts.tolist() == [[1, 2]]
    assert R.outline(ids)[0].tolist() == [[0, 1, 0, 1], [0, 1, 1, 0]]


# ------------------------------------------------------------------------------------------------------- argument rules
def test_module_argument_rules():
    from uda_aerial_semantic_segmentation_research_amd import regions as G, superpixels as SP
    f = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    ids = torch.zeros(1, 8, 8, dtype=torch.int32)
    m = torch.zeros(1, 8, 8, dtype=torch.uint8)
    v = torch.zeros(1, 8, 8)
    seg = SP.Segments(ids, (1, 1), 8, None)
    for call in (lambda: SP.slic(f), lambda: SP.slic(f[0]), lambda: SP.vote(seg, m, 3), lambda: SP.vote(ids, m, 3),
                 lambda: SP.mean(v, seg), lambda: SP.select(v, seg, 1), lambda: SP.outline(seg), lambda: G.label_ids(ids)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for call in (lambda: SP.slic(f, step=1), lambda: SP.slic(f, step=65), lambda: SP.slic(f, step=True), lambda: SP.slic(f, compactness=0),
                 lambda: SP.slic(f, compactness=1025), lambda: SP.slic(f, iterations=0), lambda: SP.slic(f, iterations=65),
                 lambda: SP.slic(f, min_area=-1), lambda: SP.slic(f.float()), lambda: SP.slic(f[..., :2]), lambda: SP.slic("x"),
                 lambda: SP.vote(seg, m, 0), lambda: SP.vote(seg, m, 256), lambda: SP.vote(seg, m, 3, ignore_index=256),
                 lambda: SP.vote(seg, m, 3, min_share=1.5), lambda: SP.vote(seg, m, 3, min_cover=-0.1),
                 lambda: SP.vote(seg, m, 3, min_share=float("nan")), lambda: SP.vote(seg, m, 3, void=256),
                 lambda: SP.vote(seg, m[:, :4], 3), lambda: SP.vote(seg, m.float(), 3), lambda: SP.vote(ids.long(), m, 3),
                 lambda: SP.vote(ids, m, 3, clusters=0), lambda: SP.vote("x", m, 3),
                 lambda: SP.mean(v.double(), seg), lambda: SP.mean(v[:, :4], seg), lambda: SP.mean(v, ids.long()),
                 lambda: SP.select(v, ids, 1), lambda: SP.select(v, seg, 0), lambda: SP.select(v, seg, 1.5), lambda: SP.select(m, seg, 1),
                 lambda: SP.outline(ids.long()), lambda: SP.SnappedLoader([], 0), lambda: SP.SnappedLoader([], 3, step=1),
                 lambda: SP.SnappedLoader([], 3, min_share=2.0), lambda: SP.SnappedLoader([], 3, ignore_index=-1),
                 lambda: G.label_ids(ids.long()), lambda: G.label_ids(ids, connectivity=6), lambda: G.label_ids([[0]]),
                 lambda: G.label_ids(torch.zeros(0, 4, 4, dtype=torch.int32))):
        with pytest.raises(ValueError):
            call()
    assert len(SP.SnappedLoader([1, 2, 3], 4)) == 3 and SP.snap is SP.vote
    assert SP.grid_of(37, 53, 8) == (5, 7) == R.grid_of(37, 53, 8)


def test_label_maps_still_refuses_int32():
    from uda_aerial_semantic_segmentation_research_amd import _args as A
    with pytest.raises(ValueError):
        A.label_maps("x", torch.zeros(1, 4, 4, dtype=torch.int32))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """rc < 0 and a message that names the argument, from the library itself: the pointers are host buffers nothing reads."""
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    good = dict(n=2, h=4, w=4, step=2, m=10, T=3, min_area=0, clusters=4, classes=5, ign=255, has=1, share=0.5, cover=0.5, void=255,
                i64=0, conn=4)
    entries = {
        "superpixel_slic": lambda a: lib.udaseg_superpixel_slic(a.get("frames", p), a["n"], a["h"], a["w"], a["step"], a["m"], a["T"],
                                                                a["min_area"], a.get("ids", p), a.get("centres", p),
                                                                a.get("counts", p), None),
        "superpixel_assign": lambda a: lib.udaseg_superpixel_assign(a.get("frames", p), a["n"], a["h"], a["w"], a["step"], a["m"],
                                                                    a.get("centres", p), a.get("labels", p), None),
        "superpixel_connect": lambda a: lib.udaseg_superpixel_connect(a.get("labels", p), a["n"], a["h"], a["w"], a["step"],
                                                                      a["min_area"], a.get("ids", p), a.get("counts", p), None),
        "superpixel_vote": lambda a: lib.udaseg_superpixel_vote(a.get("ids", p), a.get("masks", p), a["i64"], a["n"], a["h"], a["w"],
                                                                a["clusters"], a["classes"], a["has"], a["ign"], a["share"],
                                                                a["cover"], a["void"], a.get("out", p), a.get("counts", p), None),
        "superpixel_mean": lambda a: lib.udaseg_superpixel_mean(a.get("values", p), a.get("ids", p), a["n"], a["h"], a["w"],
                                                                a["clusters"], a.get("mean", p), None),
        "superpixel_gather": lambda a: lib.udaseg_superpixel_gather(a.get("ids", p), a.get("table", p), a["n"], a["h"], a["w"],
                                                                    a["clusters"], a.get("mask", p), None),
        "regions_label_i32": lambda a: lib.udaseg_regions_label_i32(a.get("labels", p), a["n"], a["h"], a["w"], a["conn"],
                                                                    a.get("ids", ctypes.c_void_p(p.value + 64)), a.get("area", p), None),
    }
    shape = [(dict(n=0), b"n"), (dict(n=65536), b"n"), (dict(h=0), b"h"), (dict(w=0), b"w")]
    big = [(dict(h=32769), b"h"), (dict(w=32769), b"w")]
    step = [(dict(step=1), b"step"), (dict(step=65), b"step")]
    clusters = [(dict(clusters=0), b"clusters"), (dict(clusters=(1 << 28) + 1), b"clusters")]
    cases = {
        "superpixel_slic": shape + big + step + [(dict(m=0), b"compactness"), (dict(m=1025), b"compactness"), (dict(T=0), b"iterations"),
                                                 (dict(T=65), b"iterations"), (dict(min_area=-1), b"min_area"),
                                                 (dict(frames=None), b"frames"), (dict(ids=None), b"ids"), (dict(centres=None), b"centres"),
                                                 (dict(ids=odd), b"ids"), (dict(centres=odd), b"centres"), (dict(counts=odd), b"counts")],
        "superpixel_assign": shape + big + step + [(dict(m=0), b"compactness"), (dict(frames=None), b"frames"),
                                                   (dict(centres=None), b"centres"), (dict(centres=odd), b"centres"),
                                                   (dict(labels=odd), b"labels")],
        "superpixel_connect": shape + big + step + [(dict(min_area=-1), b"min_area"), (dict(labels=None), b"labels"),
                                                    (dict(ids=None), b"ids"), (dict(labels=odd), b"labels"), (dict(counts=odd), b"counts")],
        "superpixel_vote": shape + big + clusters + [(dict(i64=2), b"masks_i64"), (dict(classes=0), b"classes"), (dict(classes=256), b"classes"),
                                                     (dict(has=2), b"has_ignore"), (dict(ign=256), b"ignore_index"),
                                                     (dict(ign=-1), b"ignore_index"), (dict(share=1.5), b"min_share"),
                                                     (dict(share=float("nan")), b"min_share"), (dict(cover=-0.5), b"min_cover"),
                                                     (dict(void=256), b"void_label"), (dict(ids=None), b"ids"), (dict(masks=None), b"masks"),
                                                     (dict(out=None), b"out"), (dict(ids=odd), b"ids"), (dict(counts=odd), b"counts"),
                                                     (dict(i64=1, masks=odd), b"masks")],
        "superpixel_mean": shape + big + clusters + [(dict(values=None), b"values"), (dict(ids=None), b"ids"), (dict(mean=None), b"mean"),
                                                     (dict(values=odd), b"values"), (dict(mean=odd), b"mean")],
        "superpixel_gather": shape + big + clusters + [(dict(ids=None), b"ids"), (dict(table=None), b"table"), (dict(mask=None), b"mask"),
                                                       (dict(ids=odd), b"ids")],
        "regions_label_i32": shape + [(dict(h=1 << 16, w=1 << 15), b"2^31"), (dict(conn=6), b"connectivity"), (dict(conn=0), b"connectivity"),
                                      (dict(labels=None), b"labels"), (dict(ids=None), b"ids"), (dict(ids=p), b"ids"),
                                      (dict(labels=odd), b"labels"), (dict(area=odd), b"area")],
    }
    assert sorted(cases) == sorted(entries)
    for entry, call in entries.items():
        for kw, word in cases[entry]:
            rc = call({**good, **kw})
            msg = lib.udaseg_last_error()
            assert rc < 0 and word in msg and entry.encode() in msg, (entry, kw, rc, msg)
