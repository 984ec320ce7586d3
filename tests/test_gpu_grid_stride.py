"""The capped-grid pixel kernels outside the convolutions on their SECOND grid-stride trip: data preparation, the two augmentation
pipelines' output pass (all eight instantiations), the prediction kernels (gather, finish, threshold, the default tile end to
end), argmax + confusion, the pseudo-label kernels, the prototype kernels and the nearest mask resize -- each at the smallest
size at which a thread (or wave) comes round its loop again, element by element or count by count against the oracles the suite
already has.  What a second trip can get wrong: the stride itself, state carried from one trip to the next (LDS tables and
counters, a wave's short last chunk) and the last, partial trip overrunning an output; so every output buffer allocated here sits
between two runs of 256 sentinel elements, or is pre-filled, and that is checked afterwards.  The augmentation entry points
(``strong_views``, ``train_batch``) allocate their outputs themselves: there every element of the padded buffer is compared, pad
lanes included, and the buffer's surroundings are out of this file's reach.

Cases, references and comparators live in tests/_grid_stride_cases.py, the launch shapes in tests/_launch_shapes.py;
tests/test_launch_shapes_host.py holds the caps against csrc/, asserts ``trips >= 2`` for every case here and shows that every
comparator refuses a kernel that stops after its first trip.  Figures of one MI355X run: profiles/grid_stride_grade.txt.
Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import os

import numpy as np
import pytest
import torch

import _grid_stride_cases as G
import _launch_shapes as L
import _scores_ref as S
from _grid_stride_cases import Guarded

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def D():
    from uda_aerial_semantic_segmentation_research_amd import _lib, data
    _lib.require_gpu()
    return data


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    return kernels


@pytest.fixture(scope="module")
def P():
    from uda_aerial_semantic_segmentation_research_amd import _lib, predict
    _lib.require_gpu()
    return predict


def _log(line):
    line = "grid-stride " + line
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _dev(a):
    return torch.tensor(a).cuda()                                   # a copy: the shared references stay read-only


def _nhwc(t):
    return t.permute(0, 2, 3, 1).float().cpu().numpy()


def _pad_lanes_are_zero(view):
    """``view``: the [N,3,H,W]-shaped view the data entry points hand out of their padded NHWC buffer [N,H,W,cpad]."""
    n, _, h, w = view.shape
    cpad = view.stride(3)
    full = view.as_strided((n, h, w, cpad), (h * w * cpad, w * cpad, cpad, 1), view.storage_offset())
    return bool((full[..., 3:] == 0).all())


def _worst(worst):
    err, dev, bar = worst
    return f"kernel-vs-f64 {err:.3e}  f32-vs-f64 {dev:.3e}  bar {bar:.3e}"


# ------------------------------------------------------------------------------------------------------------ prepare_batch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(G.PREPARE_CASES))
def test_prepare_batch(D, name, dtype):
    from uda_aerial_semantic_segmentation_research_amd._lib import check
    from uda_aerial_semantic_segmentation_research_amd._operands import ops
    n, h, w, calls = G.PREPARE_CASES[name]
    imgs, masks = G.prepare_inputs(name)
    dev_i, dev_m = torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda()
    bf16 = dtype == BF16
    cpad = 8 if bf16 else 4
    m255, r255 = D.normalize_constants()
    for codes in calls:
        k = len(codes)
        out, out_m = Guarded(k * h * w * cpad, dtype, G.PREPARE_FILL), Guarded(k * h * w, torch.int64, -7)
        check(ops.udaseg_prepare_batch_u8(dev_i[:k], dev_m[:k], torch.tensor(codes, dtype=torch.int32).cuda(), k, h, w, m255, r255,
                                          out.body, cpad, int(bf16), out_m.body, int(h != w), None), "prepare_batch_u8")
        want_x, want_m = G.prepare_reference(imgs[:k], masks[:k], codes)
        G.check_prepare(out.body.float().cpu().numpy().reshape(k, h, w, cpad), out_m.body.cpu().numpy().reshape(k, h, w), want_x, want_m,
                        bf16)
        assert out.intact() and out_m.intact()
    _log(f"prepare_batch {name} {'bf16' if bf16 else 'fp32'}: {h * w} px per image, trips {L.prepare_batch(h, w).trips}, codes {calls}: "
         f"image and mask bit-exact, pad lanes 0, sentinels intact")


# ------------------------------------------------------------------------------------------------------------- strong views
@pytest.mark.parametrize("label", G.STRONG_LABELS)
def test_strong_views_one_view(D, label):
    ref = G.strong_reference(D, label)
    dev = _dev(ref["imgs"])
    got32 = D.strong_views(dev, ref["P"])
    worst, share = G.check_strong(_nhwc(got32), ref, label)
    got16 = D.strong_views(dev, ref["P"], dtype=BF16)
    assert got16.dtype == BF16 and torch.equal(got16, got32.to(BF16))
    assert _pad_lanes_are_zero(got32) and _pad_lanes_are_zero(got16)
    _log(f"strong_views {label} {G.AUG_N}x{G.AUG_H}x{G.AUG_W}: trips {L.aug_output(G.AUG_H, G.AUG_W).trips}  {_worst(worst)}  "
         f"ill share {share:.6f} (cap 0.002)  bf16 = fp32 rounded once")


@pytest.mark.parametrize("a,b", G.STRONG_TWO_VIEWS)
def test_strong_views_two_views(D, a, b):
    ra, rb = G.strong_reference(D, a), G.strong_reference(D, b)
    dev = _dev(ra["imgs"])
    va, vb = D.strong_views(dev, ra["P"], rb["P"])
    wa, _ = G.check_strong(_nhwc(va), ra, a)
    wb, _ = G.check_strong(_nhwc(vb), rb, b)
    ha, hb = D.strong_views(dev, ra["P"], rb["P"], dtype=BF16)
    assert torch.equal(ha, va.to(BF16)) and torch.equal(hb, vb.to(BF16))
    assert all(_pad_lanes_are_zero(v) for v in (va, vb, ha, hb))
    _log(f"strong_views two views ({a}, {b}): {a} {_worst(wa)}; {b} {_worst(wb)}; bf16 = fp32 rounded once")


# -------------------------------------------------------------------------------------------------------------- train batch
@pytest.mark.parametrize("label", G.TRAIN_LABELS)
def test_train_batch(D, label):
    ref = G.train_reference(D, label)
    dev_img, dev_msk = _dev(ref["imgs"]), _dev(ref["masks"])
    got32, gm = D.train_batch(dev_img, dev_msk, ref["P"])
    assert gm.dtype == torch.int64
    worst, ill, band = G.check_train(_nhwc(got32), gm.cpu().numpy(), ref, label)
    got16, gm16 = D.train_batch(dev_img, dev_msk, ref["P"], dtype=BF16)
    assert got16.dtype == BF16 and torch.equal(got16, got32.to(BF16)) and torch.equal(gm16, gm)
    assert _pad_lanes_are_zero(got32) and _pad_lanes_are_zero(got16)
    _log(f"train_batch {label} {G.AUG_N}x{G.AUG_H}x{G.AUG_W}: trips {L.aug_output(G.AUG_H, G.AUG_W).trips}  {_worst(worst)}  "
         f"ill share {ill:.6f} (cap 0.002)  band share {band:.6f} (cap 0.01)  bf16 = fp32 rounded once, masks equal")


# -------------------------------------------------------------------------------------------------------------------- CLAHE
@pytest.mark.parametrize("pipe,label", G.CLAHE_CASES)
def test_clahe(D, pipe, label):
    from test_gpu_clahe import _device
    ref = G.clahe_reference(D, pipe, label)
    dev = _dev(ref["imgs"])
    got32, _, lut = _device(D, pipe, dev, ref["P"])
    lut = lut.cpu().numpy()
    worst, left, ill, (touched, tworst) = G.check_clahe(_nhwc(got32), lut, ref, pipe, label)
    got16, _, lut16 = _device(D, pipe, dev, ref["P"], dtype=BF16)
    assert got16.dtype == BF16 and torch.equal(got16, got32.to(BF16)) and np.array_equal(lut16.cpu().numpy(), lut)
    assert _pad_lanes_are_zero(got32) and _pad_lanes_are_zero(got16)
    _log(f"clahe {pipe} {label} {G.AUG_N}x{G.AUG_H}x{G.AUG_W}: trips {L.aug_output(G.AUG_H, G.AUG_W).trips}  {_worst(worst)}  "
         f"bin-boundary share {left:.6f} (cap 0.002)  ill share {ill:.6f} (cap 0.002)  tiles with a left-out pixel {touched} "
         f"(table off by up to {tworst})  bf16 = fp32 rounded once")


# ----------------------------------------------------------------------------------------------------------- predict gather
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(G.GATHER_CASES))
def test_predict_gather(P, K, D, name, dtype):
    img, g, codes, want = G.gather_reference(P, name)
    bf16 = dtype == BF16
    cpad = 8 if bf16 else 4
    tiles = g.rows * g.cols
    b = tiles * len(codes)
    out = Guarded(b * g.th * g.tw * cpad, dtype, G.GATHER_FILL)
    m, r = D.normalize_constants()
    K.predict_gather_u8(torch.from_numpy(img).cuda(), P._grid_args(g), 0, tiles, P.view_mask(codes), m, r, out.body.view(b, g.th, g.tw, cpad))
    G.check_gather(out.body.float().cpu().numpy().reshape(b, g.th, g.tw, cpad), want, bf16)
    assert out.intact()
    _log(f"predict_gather {name} {'bf16' if bf16 else 'fp32'}: {tiles} tile(s) of {g.th}x{g.tw}, codes {codes}, trips "
         f"{L.predict_gather(g.th, g.tw).trips}: bit-exact, pad lanes 0, sentinels intact")


@pytest.fixture(scope="module")
def r18():
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(0)
    return Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).to("cuda").eval()


def test_predict_large_with_every_default(P, r18):
    """tile 512, overlap 0.25, one view, the gaussian window: a 2 x 2 grid of full tiles over a 600 x 520 frame, against the
    oracle tiles through the same device model and the float64 blend."""
    from test_gpu_predict import _blend_oracle, _tile_oracle
    h, w = G.E2E_FRAME
    img = G.gather_frame(h, w)
    labels, probs = P.predict_large(r18, img, return_probs=True)
    g = P.plan_grid(h, w)
    assert (g.rows, g.cols, g.th, g.tw) == (2, 2, 512, 512)
    tiles = np.stack([_tile_oracle(P, img, g, k, 0) for k in range(g.rows * g.cols)])
    with torch.no_grad():
        lg = r18(torch.from_numpy(tiles).permute(0, 3, 1, 2).contiguous().cuda()).permute(0, 2, 3, 1).cpu().numpy()
    want = _blend_oracle(P, g, lg, (0,), 23, P.window_vector(g.th), P.window_vector(g.tw))
    err, kept = G.check_predict_large(probs[0].permute(1, 2, 0).cpu().numpy(), labels.cpu().numpy(), want)
    _log(f"predict_large defaults {h}x{w}: gather trips {L.predict_gather(g.th, g.tw).trips}  probs error {err:.3e} (bar {G.E2E_PROB_TOL:.0e})  "
         f"labels equal on the {kept:.4%} of pixels with a float64 top-two margin above {G.E2E_MARGIN:.0e} (at least {G.E2E_MIN_KEPT:.0%})")


# ----------------------------------------------------------------------------------------------------------- predict finish
def test_predict_finish(K):
    ref = G.finish_case()
    pixels, C, ldc = G.FINISH_PIXELS, G.FINISH_CLASSES, G.FINISH_LDC
    probs, labels = Guarded(pixels * ldc, torch.float32, 0.0), Guarded(pixels, torch.int64, -7)
    probs.body.copy_(_dev(ref["acc"]).reshape(-1))
    K.predict_finish(probs.body, _dev(ref["ws"]), pixels, C, ldc, labels.body)
    err, excluded = G.check_finish(probs.body.cpu().numpy().reshape(pixels, ldc), labels.body.cpu().numpy(), ref)
    assert probs.intact() and labels.intact()
    probs.body.copy_(_dev(ref["acc"]).reshape(-1))
    labels.body.fill_(-7)
    K.predict_finish(probs.body, None, pixels, C, ldc, labels.body)
    G.check_finish_labels_only(probs.body.cpu().numpy().reshape(pixels, ldc), labels.body.cpu().numpy(), ref)
    assert probs.intact() and labels.intact()
    _log(f"predict_finish {pixels} px, {C} classes, ldc {ldc}: trips {L.predict_finish(pixels).trips}  probs error {err:.3e} (bar "
         f"{G.FINISH_PROB_TOL:.0e})  margin-excluded share {excluded:.6f} (cap {G.FINISH_EXCLUDED_CAP})  without wsum: labels "
         f"bit-exact, buffer untouched")


# -------------------------------------------------------------------------------------------------------- predict threshold
def test_predict_threshold(K):
    z, want = G.threshold_case()
    n, hw, C, ldc = G.THRESHOLD_N, G.THRESHOLD_HW, G.THRESHOLD_CLASSES, G.THRESHOLD_LDC
    out = Guarded(n * C * hw, torch.float32, float("nan"))
    K.predict_threshold(torch.from_numpy(z).cuda(), n, hw, C, ldc, out.body.view(n, C, hw))
    G.check_threshold(out.body.cpu().numpy().reshape(n, C, hw), want)
    assert out.intact()
    _log(f"predict_threshold {n} x {hw} px, {C} classes: trips {L.predict_threshold(hw).trips}: equal to (sigmoid(z) > 0.5), sentinels intact")


# --------------------------------------------------------------------------------------------------------- argmax confusion
def test_argmax_confusion(K):
    buf, tgt, am, cm = G.confusion_case()
    pixels, C, ldc = G.CONFUSION_PIXELS, G.CONFUSION_CLASSES, G.CONFUSION_LDC
    logits, target = torch.from_numpy(buf).cuda(), torch.from_numpy(tgt).cuda()
    got, pred = Guarded(C * C, torch.int64, 0), Guarded(pixels, torch.int64, -7)
    for calls in (1, 2):                                            # the second call accumulates
        K.argmax_confusion(logits, target, pixels, C, ldc, got.body, pred.body)
        G.check_confusion(got.body.cpu().numpy(), pred.body.cpu().numpy(), cm, am, calls)
        assert got.intact() and pred.intact()
    _log(f"argmax_confusion {pixels} px, {C} classes, ldc {ldc}: trips {L.argmax_confusion(pixels).trips}: matrix = np.bincount "
         f"({int(cm.sum())} valid targets), pred = first_max (ties on the second trip), a second call doubles the matrix")


# ----------------------------------------------------------------------------------------------- conf_hist / pseudo_labels
@pytest.mark.parametrize("probs", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("name", list(G.PSEUDO_CASES))
def test_conf_hist_and_pseudo_labels(K, name, probs):
    """tests/test_gpu_pseudo.py::test_exact_invariants' method at kernel level (junk pad lanes, NaN pixels on the second trip),
    with the table and the confidence map also held to the float64 statement."""
    from uda_aerial_semantic_segmentation_research_amd import pseudo as PS
    ref = G.pseudo_case(name, probs)
    C, B, pixels = ref["classes"], ref["bins"], ref["pixels"]
    ldc = (C + 3) // 4 * 4
    buf = torch.from_numpy(S.padded(ref["rows"], ldc)).cuda()
    bar = G.pseudo_bar(ref, G.torch_confidence(ref, "cuda"))
    h = PS.ConfidenceHistogram(C, B)
    h._ensure(torch.device("cuda", torch.cuda.current_device()))
    K.conf_hist(buf, pixels, C, ldc, probs, B, h.table, h.nonfinite)
    table = h.table.cpu().numpy()
    near = G.check_conf_hist(table, int(h.nonfinite), ref, bar)
    portion = np.linspace(0.1, 1.0, C)
    thr = h.thresholds(portion, floor=0.05, cap=0.9)
    host_thr, host_sup = PS.thresholds_from_hist(table, portion, floor=0.05, cap=0.9)
    assert thr.dtype == torch.int32 and np.array_equal(thr.cpu().numpy(), host_thr) and np.array_equal(h.support.cpu().numpy(), host_sup)
    thr_open = h.thresholds(0.3, floor=0.0, cap=1.0)
    assert np.array_equal(thr_open.cpu().numpy(), PS.thresholds_from_hist(table, 0.3)[0])
    worst = 0.0
    routes = [(t, 0) for t in (thr, thr_open)]
    if name == "labels_second_trip":
        routes.append((thr, 1))                                     # a labels buffer one byte into its allocation: the byte stores
    for t, offset in routes:
        labels = Guarded(pixels, torch.uint8, 77, sentinel=177, offset=offset)
        conf, counts = Guarded(pixels, torch.float32, float("nan")), Guarded(C + 2, torch.int64, 0)
        assert labels.body.data_ptr() % 4 == offset
        K.pseudo_labels(buf, pixels, C, ldc, probs, B, t, G.PSEUDO_VOID, labels.body, conf.body, counts.body)
        err = G.check_pseudo_labels(labels.body.cpu().numpy(), conf.body.cpu().numpy(), counts.body.cpu().numpy(), table,
                                    t.cpu().numpy(), ref, bar)
        worst = max(worst, err)
        assert labels.intact() and conf.intact() and counts.intact()
        again = Guarded(pixels, torch.uint8, 77, sentinel=177, offset=offset)
        K.pseudo_labels(buf, pixels, C, ldc, probs, B, t, G.PSEUDO_VOID, again.body, None, torch.zeros(C + 2, dtype=torch.int64, device="cuda"))
        assert torch.equal(again.body, labels.body) and again.intact()          # bit-identical across calls
    K.conf_hist(buf, pixels, C, ldc, probs, B, h.table, h.nonfinite)
    G.check_conf_hist(h.table.cpu().numpy(), int(h.nonfinite), ref, bar, calls=2)   # accumulates
    _log(f"conf_hist / pseudo_labels {name} {'probs' if probs else 'logits'}: {C} classes, {B} bins, {pixels} px, groups "
         f"{L.conf_hist_groups(C, B)}, trips {L.conf_hist(pixels, C, B).trips} / {L.pseudo_labels(pixels).trips}  confidence error "
         f"{worst:.3e} (bar {bar:.3e})  bin-edge share {near:.6f}  non-finite {ref['nbad']}  table, thresholds, labels, counts exact"
         f"{', byte route too' if len(routes) == 3 else ''}")


# ---------------------------------------------------------------------------------------------------------------- prototypes
@pytest.mark.parametrize("pattern", G.ACCUMULATE_PATTERNS)
@pytest.mark.parametrize("classes,dim,ldf", G.ACCUMULATE_SHAPES)
def test_proto_accumulate(K, classes, dim, ldf, pattern):
    from _proto_ref import accumulate_mirror
    pixels = G.ACCUMULATE_PIXELS
    feat, lab = G.accumulate_case(classes, dim, ldf, pattern)
    mirror = accumulate_mirror(feat[:, :dim].numpy(), lab.numpy(), classes)
    sums, sq = Guarded(classes * dim, torch.float64, 0.0), Guarded(classes, torch.float64, 0.0)
    counts = Guarded(classes + 2, torch.int64, 0)
    fd, ld = feat.cuda(), lab.cuda()
    figures = []
    for calls in (1, 2):                                            # the second call accumulates
        K.proto_accumulate(fd, ldf, dim, ld, pixels, classes, sums.body, sq.body, counts.body)
        figures.append(G.check_accumulate(sums.body.cpu().numpy().reshape(classes, dim), sq.body.cpu().numpy(), counts.body.cpu().numpy(),
                                          mirror, calls))
        assert sums.intact() and sq.intact() and counts.intact()
    launch = L.proto_accumulate(pixels, dim)
    _log(f"proto_accumulate {classes} classes, dim {dim}, {pattern}: {pixels} px, {launch.threads} threads, trips {launch.trips}  counts exact  "
         f"sums err/bar {figures[0][0]:.3e}  sq err/bar {figures[0][1]:.3e}  (second call {figures[1][0]:.3e} / {figures[1][1]:.3e})")


def test_proto_rectify():
    from test_gpu_proto import _kernel_rectify, grade_case
    from uda_aerial_semantic_segmentation_research_amd import _lib
    _lib.require_gpu()
    C, dim, _, _, probs = G.RECTIFY_CASE
    ldc = 4 * ((C + 3) // 4)

    def kernel(feat, scores, proto, inv_tau):
        full = _kernel_rectify(feat, dim, scores, ldc, C, probs, proto, np.ones(C), inv_tau)      # -7 pre-filled, run twice: same bits
        assert (full[:, C:] == 0).all()
        return full[:, :C]

    fig = grade_case(*G.RECTIFY_CASE, rectify=kernel, pixels=G.RECTIFY_PIXELS)
    G.check_rectify(fig)
    _log(f"proto_rectify {G.RECTIFY_PIXELS} px, trips {L.proto_rectify(G.RECTIFY_PIXELS).trips}: {fig}")


def test_proto_assign():
    from test_gpu_contrast import GpuBackend
    c = G.ASSIGN_CASE
    G.grade_assign(GpuBackend(), _log).done()
    _log(f"proto_assign {c['batch']} x {c['ppi']} px, {c['classes']} classes, dim {c['dim']}: trips {L.proto_assign(c['batch'] * c['ppi']).trips}")


# ------------------------------------------------------------------------------------------------------------ nearest resize
@pytest.mark.parametrize("name", list(G.NEAREST_CASES))
def test_resize_nearest(K, name):
    n, H, W, h, w = G.NEAREST_CASES[name]
    src, want = G.nearest_case(name)
    dst = Guarded(n * h * w, torch.uint8, G.NEAREST_FILL, sentinel=177)
    K.resize_nearest_u8(torch.from_numpy(src).cuda(), dst.body.view(n, h, w))
    G.check_nearest(dst.body.cpu().numpy().reshape(n, h, w), want)
    assert dst.intact()
    _log(f"resize_nearest {name}: {h * ((w + 3) // 4)} groups per image, trips {L.resize_nearest(h, w).trips}: equal, sentinels intact")
