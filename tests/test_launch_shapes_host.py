"""tests/_launch_shapes.py and tests/_grid_stride_cases.py on the CPU.

1. Every cap of _launch_shapes.py is read out of the ``.hip`` text with a regular expression: a cap changed in csrc/ fails here
   and does not silently move a case of tests/test_gpu_grid_stride.py back to one trip.
2. Every new case makes its kernel go round the grid-stride loop at least twice, and the largest shape any OTHER test of the
   suite gives each of these kernels makes exactly one trip -- the record of the gap the new cases close.
3. The checks can fail: for every new case a first-trip-only mutant of the reference stands in for the kernel (an element-wise
   output left at its pre-fill beyond trip one, a histogram, count or sum made of trip one's pixels only), and the case's own
   comparator has to refuse it.  Where the reference is cheap it also stands in unmutated and has to pass.
"""
import os
import re

import numpy as np
import pytest
import torch

import _grid_stride_cases as G
import _launch_shapes as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uda_aerial_semantic_segmentation_research_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{what}: {len(found)} matches of {pattern!r}"
    return found[0]


def _constant(text, name):
    return int(_one(rf"constexpr int {name} = (\d+);", text, name))


def _entry(text, name):
    """The body of one extern "C" entry point (up to the next one)."""
    start = text.index(f'extern "C" int {name}(')
    end = text.find('extern "C"', start + 1)
    return text[start:end if end > 0 else len(text)]


# ------------------------------------------------------------------------------------------------------------------- 1. caps
def test_caps_agree_with_csrc():
    inline = r"gx = \(h \* w \+ 255\) / 256 > (\d+) \? (\d+) : \(h \* w \+ 255\) / 256;"
    assert _one(inline, _text("data_prep.hip"), "prepare_batch") == (str(L.PREPARE_BATCH_CAP),) * 2
    assert _one(inline, _text("augment.hip"), "aug_output") == (str(L.AUG_OUTPUT_CAP),) * 2
    predict = _text("predict.hip")
    assert int(_one(r"capped_grid\(tp, 256, (\d+)\)", _entry(predict, "udaseg_predict_gather_u8"), "gather")) == L.PREDICT_GATHER_CAP
    assert int(_one(r"capped_grid\(pixels, 256, (\d+)\)", _entry(predict, "udaseg_predict_finish"), "finish")) == L.PREDICT_FINISH_CAP
    assert int(_one(r"capped_grid\(hw, 256, (\d+)\)", _entry(predict, "udaseg_predict_threshold"), "threshold")) == L.PREDICT_THRESHOLD_CAP
    confusion = _entry(_text("losses.hip"), "udaseg_argmax_confusion")
    assert int(_one(r"capped_grid\(pixels, 256, (\d+)\)", confusion, "argmax_confusion")) == L.ARGMAX_CONFUSION_CAP
    pseudo = _text("pseudo.hip")
    for name in ("CH_CELLS", "CH_THREADS", "CH_BLOCKS", "PL_THREADS", "PL_MAX_BLOCKS"):
        assert _constant(pseudo, name) == getattr(L, name), name
    assert "int gx = CH_BLOCKS / groups;" in pseudo and "min(classes, CH_CELLS / bins)" in pseudo
    _one(r"capped_grid\(cdiv64\(pixels, 256\), PL_THREADS / 64, PL_MAX_BLOCKS\)", pseudo, "pseudo_labels")
    proto = _text("proto.hip")
    for name in ("PA_CU", "PR_THREADS", "PR_MAX_BLOCKS"):
        assert _constant(proto, name) == getattr(L, name), name
    _one(r"threads = DV <= 4 \? 1024 : DV <= 8 \? 512 : 256;", proto, "PaShape::threads")
    _one(r"max_blocks = PA_CU \* \(1024 / threads\);", proto, "PaShape::max_blocks")
    _one(r"capped_grid\(chunks, PaShape<DV>::threads / 64, PaShape<DV>::max_blocks\)", proto, "proto_accumulate")
    _one(r"capped_grid\(pixels, PR_THREADS, PR_MAX_BLOCKS\)", proto, "proto_rectify")
    contrast = _text("proto_contrast.hip")
    for name in ("PC_THREADS", "PC_MAX_BLOCKS"):
        assert _constant(contrast, name) == getattr(L, name), name
    _one(r"capped_grid\(pixels, PC_THREADS, PC_MAX_BLOCKS\)", _entry(contrast, "udaseg_proto_assign"), "proto_assign")
    nearest = _entry(_text("resize.hip"), "udaseg_resize_nearest_u8")
    assert _one(r"cdiv64\(groups, 256\) > (\d+) \? (\d+) : cdiv64\(groups, 256\)", nearest, "resize_nearest") == (str(L.RESIZE_NEAREST_CAP),) * 2


def test_helpers_restate_capped_grid():
    assert L.prepare_batch(512, 512) == L.Launch(1024, 256, 1, 262144)
    assert L.prepare_batch(1, 1) == L.Launch(1, 256, 1, 256)
    assert L.predict_finish(4000 * 6000).trips == 12 and L.predict_gather(512, 512).trips == 4
    assert [L.conf_hist(10 ** 7, 23, b).per_trip for b in (1024, 2048, 4096)] == [262144, 131072, 87040]
    assert L.conf_hist(10 ** 7, 32, 4096).per_trip == 65536 and L.conf_hist_groups(32, 4096) == 4 and L.conf_hist_groups(16, 2048) == 1
    assert L.pseudo_labels(10 ** 7).per_trip == 2097152 and L.pseudo_labels(257) == L.Launch(1, 256, 1, 1024)
    assert {L.proto_accumulate(10 ** 7, d).per_trip for d in range(4, 65, 4)} == {262144}
    assert [L.proto_accumulate(10 ** 7, d).threads for d in (4, 16, 20, 32, 36, 64)] == [1024, 1024, 512, 512, 256, 256]
    assert L.resize_nearest(1025, 1030) == L.Launch(1024, 256, 2, 262144)
    assert L.first_trip_nearest(1025, 1030).sum() == 262144 * 4 - 2 * (1024 * 256 // 258)        # a row's last group holds two pixels


# ------------------------------------------------------------------------------------------------------------------ 2. trips
def _new_cases():
    out = []
    for name, (n, h, w, _) in G.PREPARE_CASES.items():
        out.append((f"prepare_batch {name}", L.prepare_batch(h, w)))
    out.append(("aug_output", L.aug_output(G.AUG_H, G.AUG_W)))
    out.append(("predict_gather clamped", L.predict_gather(288, 288)))
    out.append(("predict_gather default", L.predict_gather(512, 512)))
    out.append(("predict_finish", L.predict_finish(G.FINISH_PIXELS)))
    out.append(("predict_threshold", L.predict_threshold(G.THRESHOLD_HW)))
    out.append(("argmax_confusion", L.argmax_confusion(G.CONFUSION_PIXELS)))
    for name, (c, bins, pixels) in G.PSEUDO_CASES.items():
        out.append((f"conf_hist {name}", L.conf_hist(pixels, c, bins)))
    out.append(("pseudo_labels", L.pseudo_labels(G.PSEUDO_CASES["labels_second_trip"][2])))
    for _, dim, _ in G.ACCUMULATE_SHAPES:
        out.append((f"proto_accumulate dim {dim}", L.proto_accumulate(G.ACCUMULATE_PIXELS, dim)))
    out.append(("proto_rectify", L.proto_rectify(G.RECTIFY_PIXELS)))
    out.append(("proto_assign", L.proto_assign(G.ASSIGN_CASE["batch"] * G.ASSIGN_CASE["ppi"])))
    for name, (_, _, _, h, w) in G.NEAREST_CASES.items():
        out.append((f"resize_nearest {name}", L.resize_nearest(h, w)))
    return out


def test_every_new_case_reaches_the_second_trip():
    for name, launch in _new_cases():
        assert launch.trips >= 2, (name, launch)
    assert [L.conf_hist_groups(c, b) for c, b, _ in G.PSEUDO_CASES.values()] == [1, 2, 3, 1]
    assert sorted({L.proto_accumulate_threads(d) for _, d, _ in G.ACCUMULATE_SHAPES}) == [256, 512, 1024]
    # the flat convention: on the second trip block 0 is full and block 1 holds three threads
    for pixels, launch in ((G.FINISH_PIXELS, L.predict_finish(G.FINISH_PIXELS)), (G.THRESHOLD_HW, L.predict_threshold(G.THRESHOLD_HW)),
                           (G.CONFUSION_PIXELS, L.argmax_confusion(G.CONFUSION_PIXELS)), (G.RECTIFY_PIXELS, L.proto_rectify(G.RECTIFY_PIXELS))):
        assert pixels - launch.per_trip == 259
    # pseudo_labels: the second trip has one whole chunk (the packed store) and one of three pixels (the byte stores)
    pixels = G.PSEUDO_CASES["labels_second_trip"][2]
    assert pixels - L.pseudo_labels(pixels).per_trip == L.PL_CHUNK + 3
    # proto_accumulate: one whole chunk and one of a single pixel, for every block size
    assert all(G.ACCUMULATE_PIXELS - L.proto_accumulate(G.ACCUMULATE_PIXELS, d).per_trip == L.PA_CHUNK + 1 for _, d, _ in G.ACCUMULATE_SHAPES)


def test_the_largest_shapes_of_the_other_tests_make_one_trip():
    """What the suite gave these kernels before tests/test_gpu_grid_stride.py, read from the other test files."""
    largest = [
        ("prepare_batch 512x512 (test_gpu_data)", L.prepare_batch(512, 512)),
        ("aug_output strong 512x512 (test_gpu_finetune)", L.aug_output(512, 512)),
        ("aug_output train 256x256 (test_gpu_train_aug)", L.aug_output(256, 256)),
        ("predict_gather 128x128 (test_gpu_predict)", L.predict_gather(128, 128)),
        ("predict_gather 96x160 (test_gpu_predict)", L.predict_gather(96, 160)),
        ("predict_finish 300x452 (test_gpu_predict)", L.predict_finish(300 * 452)),
        ("predict_threshold 256x256 (test_gpu_predict)", L.predict_threshold(256 * 256)),
        ("argmax_confusion 3x17x19 (test_gpu_kernels)", L.argmax_confusion(3 * 17 * 19)),
        ("argmax_confusion 130x170 (test_gpu_predict)", L.argmax_confusion(130 * 170)),
        ("conf_hist 23 x 1024 at 65537 (test_gpu_pseudo)", L.conf_hist(65537, 23, 1024)),
        ("conf_hist 23 x 2048 at 65537 (test_gpu_pseudo)", L.conf_hist(65537, 23, 2048)),
        ("conf_hist 23 x 4096 at 63 (test_gpu_pseudo)", L.conf_hist(63, 23, 4096)),
        ("pseudo_labels 65537 (test_gpu_pseudo)", L.pseudo_labels(65537)),
        ("proto_rectify 65537 (test_gpu_proto)", L.proto_rectify(65537)),
        ("proto_assign 262147 (test_gpu_contrast)", L.proto_assign(262147)),
        ("resize_nearest 512x768 (test_gpu_ingest)", L.resize_nearest(512, 768)),
    ] + [(f"proto_accumulate dim {d} at 65537 (test_gpu_proto)", L.proto_accumulate(65537, d)) for d in (4, 8, 16, 64)]
    for name, launch in largest:
        assert launch.trips == 1, (name, launch)
    assert L.conf_hist(65537, 32, 4096).trips == 2          # the one second trip the suite had: the four-group route


# ---------------------------------------------------------------------------------------------------------------- 3. mutants
def refused(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


@pytest.fixture(scope="module")
def D():
    from uda_aerial_semantic_segmentation_research_amd import data
    return data


@pytest.mark.parametrize("name", list(G.PREPARE_CASES))
@pytest.mark.parametrize("bf16", [False, True])
def test_prepare_batch_mutants(name, bf16):
    imgs, masks = G.prepare_inputs(name)
    codes = G.PREPARE_CASES[name][3][-1]
    want_x, want_m = G.prepare_reference(imgs[:len(codes)], masks[:len(codes)], codes)
    cpad = 8 if bf16 else 4
    full = np.zeros(want_x.shape[:3] + (cpad,), dtype=np.float32)
    full[..., :3] = G.bf16_round(want_x) if bf16 else want_x
    G.check_prepare(full, want_m, want_x, want_m, bf16)
    for what, out, out_m in G.prepare_mutants(want_x, want_m, cpad, bf16):
        refused(G.check_prepare, out, out_m, want_x, want_m, bf16)


def test_d4_combos_cover_the_group():
    from uda_aerial_semantic_segmentation_research_amd.data import compose_d4
    assert all(compose_d4(*G.d4_combo(c)) == c for c in range(8))


def test_strong_views_mutant(D):
    ref = G.strong_reference(D, "hsv")
    G.check_strong(ref["img32"], ref, "hsv")
    refused(G.check_strong, G.image_mutant(ref["img32"]), ref, "hsv")


def test_train_batch_mutants(D):
    ref = G.train_reference(D, "grid")
    G.check_train(ref["img32"], ref["m64"], ref, "grid")
    refused(G.check_train, G.image_mutant(ref["img32"]), ref["m64"], ref, "grid")
    refused(G.check_train, ref["img32"], np.where(G.aug_first_trip(), ref["m64"], -7), ref, "grid")


@pytest.mark.parametrize("pipe", ("strong", "train"))
def test_clahe_mutant(D, pipe):
    ref = G.clahe_reference(D, pipe, "clahe")
    img32, lut = G.clahe_leg32(ref, pipe)
    G.check_clahe(img32, lut, ref, pipe, "clahe")
    refused(G.check_clahe, G.image_mutant(img32), lut, ref, pipe, "clahe")


def test_the_clahe_cases_keep_their_caps(D):
    """Computed here before any GPU run: the share of pixels next to a bin boundary and the hue-ill share of every CLAHE case."""
    from test_gpu_clahe import ILL_CAP, LEFT_CAP
    for pipe, label in G.CLAHE_CASES:
        ref = G.clahe_reference(D, pipe, label)
        print(f"clahe {pipe} {label}: left {ref['left'].mean():.6f} (cap {LEFT_CAP})  ill {ref['ill'].mean():.6f} (cap {ILL_CAP})")
        assert ref["left"].mean() <= LEFT_CAP and ref["ill"].mean() <= ILL_CAP


@pytest.mark.parametrize("name", list(G.GATHER_CASES))
def test_predict_gather_mutant(name):
    from uda_aerial_semantic_segmentation_research_amd import predict as P
    _, g, codes, want = G.gather_reference(P, name)
    assert (g.th, g.tw) == ((288, 288) if name.startswith("clamped") else (512, 512))
    for bf16 in (False, True):
        cpad = 8 if bf16 else 4
        full = np.zeros(want.shape[:3] + (cpad,), dtype=np.float32)
        full[..., :3] = G.bf16_round(want) if bf16 else want
        G.check_gather(full, want, bf16)
        refused(G.check_gather, G.gather_mutant(want, cpad, bf16), want, bf16)


def test_predict_large_mutants():
    """The comparator of the end-to-end case on synthetic logits of three classes (the model needs a GPU; the comparator does not)."""
    from test_gpu_predict import _blend_oracle
    from uda_aerial_semantic_segmentation_research_amd import predict as P
    g = P.plan_grid(*G.E2E_FRAME)
    assert (g.rows, g.cols, g.th, g.tw) == (2, 2, 512, 512)
    logits = (3.0 * np.random.default_rng(5).standard_normal((4, 512, 512, 4))).astype(np.float32)
    want = _blend_oracle(P, g, logits, (0,), 3, P.window_vector(512), P.window_vector(512))
    G.check_predict_large(want.astype(np.float32), want.argmax(-1), want)
    for what, probs, labels in G.predict_large_mutants(P, want):
        refused(G.check_predict_large, probs, labels, want)


def test_predict_finish_mutants():
    ref = G.finish_case()
    done = np.zeros_like(ref["acc"])
    done[:, :G.FINISH_CLASSES] = ref["q"].astype(np.float32)
    err, excluded = G.check_finish(done, ref["am"], ref)
    print(f"predict_finish reference alone: fp32 quotient error {err:.3e}, excluded share {excluded:.6f}")
    for what, probs, labels in G.finish_mutants(ref):
        refused(G.check_finish, probs, labels, ref)
    G.check_finish_labels_only(ref["acc"], ref["am_rows"], ref)
    refused(G.check_finish_labels_only, ref["acc"], G.finish_labels_only_mutant(ref), ref)


def test_predict_threshold_mutant():
    _, want = G.threshold_case()
    G.check_threshold(want.copy(), want)
    refused(G.check_threshold, G.threshold_mutant(want), want)


def test_argmax_confusion_mutants():
    _, tgt, am, cm = G.confusion_case()
    G.check_confusion(cm, am, cm, am)
    G.check_confusion(2 * cm, am, cm, am, calls=2)
    for what, m_cm, m_pred in G.confusion_mutants(tgt, am, cm):
        refused(G.check_confusion, m_cm, m_pred, cm, am)


@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("name", list(G.PSEUDO_CASES))
def test_pseudo_mutants(name, probs):
    from uda_aerial_semantic_segmentation_research_amd import pseudo as P
    ref = G.pseudo_case(name, probs)
    C, B, pixels = ref["classes"], ref["bins"], ref["pixels"]
    assert ref["nbad"] == len(ref["planted"]) >= 3 and min(ref["planted"]) >= L.conf_hist(pixels, C, B).per_trip
    bar = G.pseudo_bar(ref, G.torch_confidence(ref))
    table, nonfinite, _, _, _ = G.pseudo_leg(ref, np.zeros(C, dtype=np.int64))
    thr, _ = P.thresholds_from_hist(table, np.linspace(0.1, 1.0, C), floor=0.05, cap=0.9)
    table, nonfinite, labels, conf, counts = G.pseudo_leg(ref, thr)
    G.check_conf_hist(table, nonfinite, ref, bar)
    G.check_pseudo_labels(labels, conf, counts, table, thr, ref, bar)
    # conf_hist on its first trip only: the table and the non-finite count
    m_table, m_bad, _, _, _ = G.pseudo_leg(ref, thr, L.first_trip(L.conf_hist(pixels, C, B), pixels))
    refused(G.check_conf_hist, m_table, nonfinite, ref, bar)
    refused(G.check_conf_hist, table, m_bad, ref, bar)
    launch = L.pseudo_labels(pixels)
    if launch.trips > 1:                          # pseudo_labels on its first trip only: labels, confidence, counts -- one at a time
        _, _, m_labels, m_conf, m_counts = G.pseudo_leg(ref, thr, L.first_trip(launch, pixels))
        refused(G.check_pseudo_labels, m_labels, conf, counts, table, thr, ref, bar)
        refused(G.check_pseudo_labels, labels, m_conf, counts, table, thr, ref, bar)
        refused(G.check_pseudo_labels, labels, conf, m_counts, table, thr, ref, bar)


@pytest.mark.parametrize("classes,dim,ldf", G.ACCUMULATE_SHAPES)
def test_proto_accumulate_mutant(classes, dim, ldf):
    from _proto_ref import accumulate_mirror
    for pattern in G.ACCUMULATE_PATTERNS:
        feat, lab = G.accumulate_case(classes, dim, ldf, pattern)
        mirror = accumulate_mirror(feat[:, :dim].numpy(), lab.numpy(), classes)
        G.check_accumulate(*mirror[:3], mirror)
        sums, sq, counts = G.accumulate_mutant(feat, lab, classes, dim)
        refused(G.check_accumulate, sums, sq, counts, mirror)
        refused(G.check_accumulate, sums, mirror[1], mirror[2], mirror)           # the sums alone: the bar is no blanket
        refused(G.check_accumulate, mirror[0], sq, mirror[2], mirror)


def test_proto_rectify_mutant_and_excluded_share():
    """torch's fp32 error and the excluded share of the case on the CPU first (as tests/test_gpu_proto.py records having done),
    then the mutant."""
    from test_gpu_proto import EXCLUDED_CAP, grade_case
    fig = grade_case(*G.RECTIFY_CASE, device="cpu", pixels=G.RECTIFY_PIXELS)
    print("proto_rectify past the grid, torch fp32 on the CPU:", fig)
    assert fig["excluded"] <= EXCLUDED_CAP and fig["moved_winner"] > 0.01
    refused(G.check_rectify, grade_case(*G.RECTIFY_CASE, device="cpu", rectify=G.rectify_mutant, pixels=G.RECTIFY_PIXELS))


def test_proto_assign_mutant():
    import _contrast_ref as R
    quiet = lambda line: None                                                     # noqa: E731
    G.grade_assign(R.LegBackend(), quiet).done()
    with pytest.raises(AssertionError):
        G.grade_assign(G.assign_mutant_backend(), quiet).done()


@pytest.mark.parametrize("name", list(G.NEAREST_CASES))
def test_resize_nearest_mutant(name):
    _, want = G.nearest_case(name)
    G.check_nearest(want.copy(), want)
    mutant = G.nearest_mutant(want)
    assert (mutant != want).any(axis=(1, 2)).all()
    refused(G.check_nearest, mutant, want)
