"""CPU checks of the prediction module's host side (uda_aerial_semantic_segmentation_research_amd/predict.py): the tile planner,
the blend windows, the inverse-view table, and the argument checks of the new C entry points (rc -1 + message, no launch)."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from uda_aerial_semantic_segmentation_research_amd import predict as P


@pytest.mark.parametrize("length,tile,overlap", list(itertools.product(
    (1, 17, 31, 32, 100, 128, 129, 300, 452, 511, 512, 513, 1000, 4000, 6000), (32, 128, 512), (0.0, 0.25, 0.4, 0.5))))
def test_planner_covers_the_axis_with_the_fewest_tiles(length, tile, overlap):
    t, s, origins = P.plan_axis(length, tile, overlap)
    ceil32 = (length + 31) // 32 * 32
    assert t == min(tile, ceil32) and t % 32 == 0
    assert s == t - round(overlap * t) and 1 <= s <= t
    assert origins[0] == 0
    if length <= t:
        assert origins == [0]
    else:
        assert origins[-1] == length - t
        assert len(origins) == math.ceil((length - t) / s) + 1          # the fewest tiles of stride <= s that reach the end
        assert all(b > a for a, b in zip(origins, origins[1:]))
        assert all(b - a <= s for a, b in zip(origins, origins[1:]))
        assert all(0 <= o <= length - t for o in origins)
    covered = np.zeros(length, dtype=bool)
    for o in origins:
        covered[o:o + t] = True
    assert covered.all()


def test_planner_grid_and_rejections():
    g = P.plan_grid(300, 452, 128, 0.25)
    assert (g.th, g.tw, g.rows, g.cols) == (128, 128, 3, 5) and g.oy == [0, 96, 172] and g.ox[-1] == 452 - 128
    g = P.plan_grid(100, 330, (64, 96), 0.5)
    assert (g.th, g.tw, g.sy, g.sx) == (64, 96, 32, 48)
    for bad in (dict(tile=48), dict(tile=0), dict(tile=(128, 100)), dict(overlap=-0.1), dict(overlap=0.6)):
        with pytest.raises(ValueError):
            P.plan_grid(300, 452, **{"tile": 128, "overlap": 0.25, **bad})
    with pytest.raises(ValueError):
        P.plan_axis(0, 128, 0.25)


def test_predict_large_rejects_bad_requests_before_any_gpu_work():
    """tta='d4' on a non-square tile, a bad tile / overlap / window / tta and a non-uint8 frame: ValueError before the model or the
    device is touched (the model argument is never looked at here)."""
    img = np.zeros((300, 452, 3), dtype=np.uint8)
    for kw in (dict(tile=(128, 256), tta="d4"), dict(tile=100), dict(overlap=0.75), dict(window="hann"), dict(tta="rot90")):
        with pytest.raises(ValueError):
            P.predict_large(None, img, **kw)
    with pytest.raises(ValueError, match="square"):
        P.predict_large(None, np.zeros((40, 330, 3), dtype=np.uint8), tile=128, tta="d4")     # 40 rows: tile clamped to 64x128
    with pytest.raises(ValueError, match="uint8"):
        P.predict_large(None, img.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        P.predict_large(None, img[..., :2])


@pytest.mark.parametrize("t", [32, 64, 128, 256, 512, 96])
def test_window_vectors(t):
    g = P.window_vector(t, "gaussian")
    assert g.dtype == np.float32 and g.shape == (t,)
    assert np.array_equal(g, g[::-1])
    assert g.max() == 1.0 and g.min() >= np.float32(1e-3)
    i = np.arange(t, dtype=np.float64)
    ref = np.exp(-0.5 * ((i - (t - 1) / 2) / (t / 8)) ** 2)
    assert np.array_equal(g, np.maximum(ref / ref.max(), 1e-3).astype(np.float32))
    u = P.window_vector(t, "uniform")
    assert u.dtype == np.float32 and (u == 1).all()
    with pytest.raises(ValueError):
        P.window_vector(t, "hann")


@pytest.mark.parametrize("code", range(8))
def test_inverse_view_undoes_every_code(code):
    shapes = [(5, 5)] + ([(4, 6), (6, 4)] if not code & 1 else [])
    for th, tw in shapes:
        seen = set()
        for y in range(th):
            for x in range(tw):
                ty, tx = P.apply_view(code, y, x, th, tw)
                assert 0 <= ty < th and 0 <= tx < tw
                assert P.inverse_view(code, ty, tx, th, tw) == (y, x)
                assert P.apply_view(code, *P.inverse_view(code, y, x, th, tw), th, tw) == (y, x)
                seen.add((ty, tx))
        assert len(seen) == th * tw
    # square tiles: the same map as data._apply_code, which prepare_batch's kernel implements
    from uda_aerial_semantic_segmentation_research_amd.data import _apply_code
    assert all(P.apply_view(code, y, x, 5, 5) == _apply_code(code, y, x, 5) for y in range(5) for x in range(5))


def test_view_sets():
    assert P.VIEWS[None] == (0,) and P.VIEWS["flips"] == (0, 2, 4, 6) and P.VIEWS["d4"] == tuple(range(8))
    assert all(not c & 1 for c in P.VIEWS["flips"])
    assert P.accumulator_bytes(4000, 6000, 23) == 4000 * 6000 * 25 * 4


def test_entry_points_refuse_bad_arguments_without_gpu():
    """Every new entry point checks its scalars before any launch: rc -1 and a message through udaseg_last_error."""
    from uda_aerial_semantic_segmentation_research_amd import _lib
    lib = _lib.load()
    f3 = ctypes.c_float * 3
    m, r = f3(1, 2, 3), f3(1, 1, 1)
    p = 4096                                                           # never dereferenced: the checks fail first
    # grid of a 300 x 452 frame, tile 128, overlap 0.25: rows 3, cols 5, strides 96
    grid = (300, 452, 128, 128, 3, 5, 96, 96)

    def blend(ldc=24, classes=23, ldp=24, views=1, grid=grid):
        return lib.udaseg_predict_blend(p, ldc, *grid, 0, 2, views, classes, p, p, p, ldp, p, None)

    def err():
        return lib.udaseg_last_error().decode()

    assert blend(ldc=22) == -1 and "ldc" in err()
    assert blend(ldp=22) == -1 and "ldp" in err()
    assert blend(classes=33, ldc=36, ldp=36) == -1 and "classes" in err()
    assert blend(classes=25, ldc=24) == -1 and "classes" in err()
    rect = (300, 452, 128, 256, 3, 3, 96, 192)
    assert blend(views=0xFF, grid=rect) == -1 and "square" in err()
    assert blend(views=0x02, grid=rect) == -1 and "square" in err()
    assert blend(views=0x55, grid=(300, 452, 128, 256, 3, 2, 96, 192)) == -1 and "grid" in err()   # 452 wide: 3 columns
    assert blend(grid=(300, 452, 100, 100, 3, 5, 75, 75)) == -1 and "32" in err()
    assert blend(grid=(300, 452, 128, 128, 4, 5, 96, 96)) == -1 and "grid" in err()

    def gather(views=1, grid=grid, cpad=4, bf16=0):
        return lib.udaseg_predict_gather_u8(p, *grid, 0, 2, views, m, r, p, cpad, bf16, None)

    assert gather(views=0x02, grid=(300, 452, 128, 256, 3, 3, 96, 192)) == -1 and "square" in err()
    assert gather(cpad=4, bf16=1) == -1 and "cpad" in err()
    assert gather(views=0) == -1 and "views" in err()
    assert lib.udaseg_predict_gather_u8(p, *grid, 14, 2, 1, m, r, p, 4, 0, None) == -1 and "grid" in err()   # tiles 14, 15 of 15

    assert lib.udaseg_predict_finish(p, p, 100, 23, 22, p, None) == -1 and "ldc" in err()
    assert lib.udaseg_predict_finish(p, None, 100, 33, 36, p, None) == -1 and "classes" in err()
    assert lib.udaseg_predict_threshold(p, 1, 100, 23, 21, p, None) == -1 and "ldc" in err()
    assert lib.udaseg_predict_threshold(p, 1, 100, 40, 40, p, None) == -1 and "classes" in err()
