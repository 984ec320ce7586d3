"""Host side of CLAHE in the augmentation pipelines (no GPU): the opt-in draws of ``data.draw_strong_params`` /
``data.draw_training_params``, ``set_clahe`` and the refusals of ``check``, and the numpy restatement (tests/_clahe_ref.py)
against hand-computed cases."""
import math
import os

import numpy as np
import pytest
import torch

import _clahe_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000


@pytest.fixture(scope="module")
def D():
    from uda_aerial_semantic_segmentation_research_amd import data
    return data


def _draws(D):
    return ((D.draw_strong_params, 0.5, 4.0), (D.draw_training_params, 0.3, 2.0))


def test_default_draw_is_todays_table(D):
    for draw, _, _ in _draws(D):
        a = draw(512, 64, 64, torch.Generator().manual_seed(7))
        b = draw(512, 64, 64, torch.Generator().manual_seed(7), clahe=False)
        assert np.array_equal(a.ints, b.ints)
        assert a.ints[:, 21].any() and not a.clahe.any()               # drawn, recorded, no stage
        assert not (((a.ints[:, 0] & D.SA_STAGE5) != 0) & (a.ints[:, 21] != 0)).any()


def test_opt_in_changes_four_words_of_the_drawn_samples_only(D):
    for draw, p, limit in _draws(D):
        off = draw(N, 64, 64, torch.Generator().manual_seed(3))
        on = draw(N, 64, 64, torch.Generator().manual_seed(3), clahe=True)
        was = off.ints[:, 21] != 0
        diff = off.ints != on.ints
        assert set(np.nonzero(diff.any(axis=0))[0]) == {0, 5, 15, 21}
        assert np.array_equal(diff.any(axis=1), was)                   # every drawn sample changes, no other does
        assert not on.ints[:, 21].any()
        assert np.array_equal(on.clahe, was)
        assert np.array_equal(on.ints[was, 0], off.ints[was, 0] | D.SA_STAGE5)
        assert (on.ints[was, 5] == D.STAGE5_CLAHE).all() and (on.floats[was, 16] == 0).all()
        rate, want = was.mean(), p / 4
        assert abs(rate - want) <= 3 * math.sqrt(want * (1 - want) / N), (rate, want)
        clip = on.floats[was, 15]
        assert clip.min() >= 1.0 and clip.max() <= limit and clip.max() - clip.min() > 0.9 * (limit - 1)
        on.check(N, 64, 64)


def test_set_clahe_and_check_refusals(D):
    for cls in (D.StrongAugParams, D.TrainAugParams):
        P = cls(2, 64, 64)
        with pytest.raises(ValueError):
            P.set_stage5(0, D.STAGE5_CLAHE, 2.0, 0.0)                  # kind 3 has its own setter
        for bad in (0.99, 0.0, -1.0, float("nan")):
            with pytest.raises(ValueError):
                P.set_clahe(0, bad)
        assert not P.flags.any()                                        # a refused call leaves the record alone
        P.set_clahe(1, 2.5)
        assert P.flags[1] == D.SA_STAGE5 and P.ints[1, 5] == 3 and P.floats[1, 15] == 2.5 and list(P.clahe) == [False, True]
        P.check(2, 64, 64)
        P.floats[1, 15] = 0.5                                           # written past the setter
        with pytest.raises(ValueError):
            P.check(2, 64, 64)
        for h, w in ((60, 64), (64, 60), (65, 65)):
            Q = cls(2, h, w)
            Q.check(2, h, w)                                            # no CLAHE record: any frame
            Q.set_clahe(0, 1.0)
            with pytest.raises(ValueError):
                Q.check(2, h, w)
    for draw, _, _ in _draws(D):
        draw(4, 60, 60, torch.Generator().manual_seed(0))               # the default draws on any frame
        with pytest.raises(ValueError):
            draw(4, 60, 64, torch.Generator().manual_seed(0), clahe=True)


# ------------------------------------------------------------------------------------------------------ the restatement
def test_header_states_the_matrices_the_restatement_forms():
    fwd, inv = C.matrices(np.float32)
    assert [np.float32(float(s)) for s in C.FORWARD_F32] == list(fwd.ravel())
    assert [np.float32(float(s)) for s in C.INVERSE_F32] == list(inv.ravel())
    hdr = open(os.path.join(ROOT, "uda_aerial_semantic_segmentation_research_amd", "csrc", "aug_common.h")).read()
    for s in C.FORWARD_F32 + C.INVERSE_F32:
        assert s + "f" in hdr, s


def test_lab_round_trip_in_float64():
    rgb = np.random.default_rng(5).uniform(0.0, 255.0, (4096, 3))
    rgb[:64] = np.random.default_rng(6).integers(0, 12, (64, 3))          # the linear toe of the transfer function
    l8, a, b = C.rgb_to_lab(rgb, np.float64)
    assert l8.min() >= 0 and l8.max() <= 255.0
    back = C.lab_to_rgb(l8, a, b, np.float64)
    assert np.abs(back - rgb).max() <= 1e-9
    white = C.rgb_to_lab(np.array([[255.0, 255.0, 255.0]]), np.float64)
    assert abs(white[0][0] - 255.0) < 1e-3 and abs(white[1][0]) < 1e-3 and abs(white[2][0]) < 1e-3


def test_flat_histogram_is_the_identity_ramp():
    for area in (256, 1024):
        lut, info = C.tile_table(np.full(256, area // 256), 4.0, area)
        assert info["excess"] == 0 and info["limit"] == 4 * area // 256
        assert list(lut) == [round((k + 1) * 255 / 256) for k in range(256)]      # Python's round: half to even


def test_one_bin_tile_by_hand():
    hist = np.zeros(256, dtype=np.int64)
    hist[100] = 64
    lut, info = C.tile_table(hist, 1.0, 64)
    assert info == dict(limit=1, excess=63, share=0, rest=63, step=4)
    # after the clip: bin 100 holds 1; bins 0, 4, ..., 248 get one more each (63 of them; 100 is one of them)
    want = np.zeros(256, dtype=np.int64)
    want[100] = 1
    want[0:249:4] += 1
    assert want.sum() == 64
    cum = np.cumsum(want)
    assert list(lut) == [min(255, round(int(c) * 255 / 64)) for c in cum]
    assert lut[0] == 4 and lut[99] == round(25 * 255 / 64) and lut[100] == round(27 * 255 / 64) and lut[255] == 255


def test_even_share_and_half_even_rounding():
    hist = np.zeros(256, dtype=np.int64)
    hist[7] = 1024
    lut, info = C.tile_table(hist, 4.0, 1024)                            # limit 16, excess 1008 = 3 * 256 + 240, step 1
    assert info == dict(limit=16, excess=1008, share=3, rest=240, step=1)
    # area 510: cumsum * 255 / 510 = cumsum / 2 -- every odd count is a tie
    h2 = np.zeros(256, dtype=np.int64)
    h2[:255] = 2
    lut2, _ = C.tile_table(h2, 40.0, 510)
    assert list(lut2[:4]) == [1, 2, 3, 4]
    h3 = np.zeros(256, dtype=np.int64)
    h3[0], h3[1], h3[2], h3[3] = 1, 2, 2, 505
    lut3, _ = C.tile_table(h3, 400.0, 510)                               # cumsum 1, 3, 5: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert list(lut3[:3]) == [0, 2, 2]


def test_blend_weights_and_constant_frame():
    k = np.full((64, 64), 9, dtype=np.int64)
    lut = np.zeros((8, 8, 256), dtype=np.uint8)
    lut[:, :, 9] = np.arange(64, dtype=np.uint8).reshape(8, 8) * 3
    out = C.blend(k, lut, np.float64)
    assert out[4, 4] == lut[0, 0, 9] and out[0, 0] == lut[0, 0, 9]       # a tile centre; the corner clamps to its tile
    assert out[63, 63] == lut[7, 7, 9]
    assert out[4, 8] == 0.5 * lut[0, 0, 9] + 0.5 * lut[0, 1, 9]           # half way between two centres
    v = np.full((64, 64, 3), 77.0)
    res, own, l8, info = C.clahe(v, 1.0, np.float64)
    assert (own == own[0, 0]).all() and info[0]["excess"] == 63 and np.ptp(res) == 0.0
