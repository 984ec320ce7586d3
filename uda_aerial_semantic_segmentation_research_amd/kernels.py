"""Thin tensor-level wrappers over the C-ABI (one Python function per entry point of include/udaseg.h).

No autograd here and no arithmetic: these marshal ``torch.Tensor`` storage pointers, sizes and the current HIP
stream into libudaseg_hip.so.  All activations are NHWC fp32 contiguous tensors ``[N, H, W, C]`` with C % 4 == 0.
"""
import torch

from . import _lib
from ._lib import ACT_LEAKY, ACT_NONE, ConvDesc, check
from ._operands import OPERANDS, ops          # the table every pointer-passing call goes through (checks before data_ptr())

_byref = _lib.C.byref


def stream():
    """hipStream_t of torch's current stream (kernels are enqueued there, asynchronously)."""
    return torch.cuda.current_stream().cuda_stream


def zeros(shape, dtype, device, st=None):
    """torch.zeros at a sixth of its host cost: torch.empty + one hipMemsetAsync on the plan's stream (a torch fill costs ~30 us of
    host time on this stack, and BASELINE cfg 3 is bound by the host's launch rate: profiles/r04_host_bound.txt)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    check(ops.udaseg_memset_async(t, 0, t.numel() * t.element_size(), st), "memset_async")
    return t


def zeros_like(x, st=None):
    return zeros(x.shape, x.dtype, x.device, st)


def stream_wait(waiter, signal):
    """Stream ``waiter`` (a hipStream_t handle) waits for everything enqueued on ``signal`` so far -- torch's
    ``Event().record(signal); waiter.wait_event(ev)`` at a third of its host cost (a pooled event inside the library)."""
    check(ops.udaseg_stream_wait(waiter, signal), "stream_wait")


_WORKSPACE = {}


def ensure_workspace(device, nbytes=16 << 20):
    """Hand the library its scratch buffer (once per device; PyTorch owns the memory)."""
    key = str(device)
    if key not in _WORKSPACE:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        scr = torch.zeros(256 << 10, dtype=torch.uint8, device=device)     # zeroed once; the library keeps it zeroed
        with torch.cuda.device(device):          # the library binds the buffers to the CURRENT device
            check(ops.udaseg_set_workspace(buf, nbytes), "set_workspace")
            check(ops.udaseg_set_stats_scratch(scr, scr.numel()), "set_stats_scratch")
        _WORKSPACE[key] = buf
        _WORKSPACE[key + "/stats"] = scr
    return _WORKSPACE[key]


def conv_desc(n, hi, wi, ci, co, k, stride, pad):
    ho = (hi + 2 * pad - k) // stride + 1
    wo = (wi + 2 * pad - k) // stride + 1
    return ConvDesc(n, hi, wi, ci, ho, wo, co, k, k, stride, pad)


def conv2d_fwd(d, x, w, bias, y, act=ACT_NONE, slope=0.0, accumulate=False, st=None):
    if x.dtype == torch.bfloat16:
        assert not accumulate
        return conv2d_fwd_bf16(d, x, w, bias, None, y, act, slope, None, st)
    check(ops.udaseg_conv2d_fwd(d, x, w, bias, y, act, slope,
                                         int(accumulate), st), "conv2d_fwd")


def conv2d_fwd_bnstats(d, x, w, bias, y, stats, st=None):
    if x.dtype == torch.bfloat16:
        return conv2d_fwd_bf16(d, x, w, bias, None, y, ACT_NONE, 0.0, stats, st)
    check(ops.udaseg_conv2d_fwd_bnstats(d, x, w, bias, y,
                                                 stats, st), "conv2d_fwd_bnstats")


def conv2d_fwd_fused(d, x, w, bias, residual, y, act=ACT_NONE, slope=0.0, st=None):
    if x.dtype == torch.bfloat16:
        return conv2d_fwd_bf16(d, x, w, bias, residual, y, act, slope, None, st)
    check(ops.udaseg_conv2d_fwd_fused(d, x, w, bias, residual, y,
                                               act, slope, st), "conv2d_fwd_fused")


def bn_fold(w, bias, gamma, beta, running_mean, running_var, eps, w_folded, bias_folded, st=None):
    co = w.shape[0]
    check(ops.udaseg_bn_fold(w, bias, gamma, beta, running_mean,
                                      running_var, eps, co, w.numel() // co, w_folded,
                                      bias_folded, st), "bn_fold")


def argmax_confusion(logits_base, target, pixels, classes, ldc, confusion, pred=None, st=None):
    check(ops.udaseg_argmax_confusion(logits_base, target, pixels, classes, ldc,
                                               confusion, pred, st),
          "argmax_confusion")


def score_hist(logits_base, target, pixels, classes, ldc, bins, score_range, pos, neg, st=None):
    """pos / neg [classes * bins] int64 += per-class histograms of the log-odds score (they accumulate)."""
    check(ops.udaseg_score_hist(logits_base, target, pixels, classes, ldc, bins, score_range, pos, neg, st), "score_hist")


def curve_finish(pos, neg, classes, bins, auc, ap, auc_slack, support, st=None):
    check(ops.udaseg_curve_finish(pos, neg, classes, bins, auc, ap, auc_slack, support, st), "curve_finish")


def calib_hist(scores_base, target, pixels, classes, ldc, probs, inv_temp, bins, tables, counters, st=None):
    """tables [3 * classes * bins] int64 += count / correct / conf_q by predicted class and confidence bin, counters [3] += in the
    tables / void / non-finite (they accumulate).  inv_temp: device fp32 [1] or None (beta = 1)."""
    check(ops.udaseg_calib_hist(scores_base, target, pixels, classes, ldc, int(bool(probs)), inv_temp, bins, tables, counters, st),
          "calib_hist")


def calib_finish(tables, classes, bins, out, per_class, st=None):
    check(ops.udaseg_calib_finish(tables, classes, bins, out, per_class, st), "calib_finish")


def calib_nll(logits_base, target, pixels, classes, ldc, inv_temp, partials, sums, counters, st=None):
    """sums [4] f64 += n, sum nll, sum d nll / d beta, sum d2 nll / d beta2 (fixed-order sums; they accumulate).
    partials: 4 * seg_partials() doubles of scratch."""
    check(ops.udaseg_calib_nll(logits_base, target, pixels, classes, ldc, inv_temp, partials, sums, counters, st), "calib_nll")


def calib_step(sums, inv_temp, state, st=None):
    """One guarded Newton step on inv_temp [1] from sums [4]; sums is zeroed, state [4] f64 written."""
    check(ops.udaseg_calib_step(sums, inv_temp, state, st), "calib_step")


def conf_hist(scores_base, pixels, classes, ldc, probs, bins, hist, nonfinite, st=None):
    """hist [classes * bins] int64 += the histogram of the winning class's confidence, nonfinite [1] += the pixels without one
    (they accumulate)."""
    check(ops.udaseg_conf_hist(scores_base, pixels, classes, ldc, int(bool(probs)), bins, hist, nonfinite, st), "conf_hist")


def pseudo_thresholds(hist, classes, bins, portion, k_floor, k_cap, thr_bins, support, st=None):
    """thr_bins [classes] int32, support [classes] int64 from the table; portion: float64 [classes] on the device."""
    check(ops.udaseg_pseudo_thresholds(hist, classes, bins, portion, k_floor, k_cap, thr_bins, support, st), "pseudo_thresholds")


def pseudo_labels(scores_base, pixels, classes, ldc, probs, bins, thr_bins, void_label, labels, conf, counts, st=None):
    """labels [pixels] uint8 (void_label below the class's threshold bin), conf [pixels] fp32 or None, counts [classes + 2] int64 +=
    kept per class, void, non-finite."""
    check(ops.udaseg_pseudo_labels(scores_base, pixels, classes, ldc, int(bool(probs)), bins, thr_bins, void_label, labels, conf,
                                   counts, st), "pseudo_labels")


def proto_accumulate(feat_base, ldf, dim, labels, pixels, classes, sums, sq, counts, st=None):
    """sums [classes * dim] / sq [classes] float64, counts [classes + 2] int64 += the per-class feature sums, squared norms and pixel
    counts of feat [pixels * ldf] fp32 under labels [pixels] uint8 (then the labels beyond the classes, then the non-finite pixels)."""
    check(ops.udaseg_proto_accumulate(feat_base, ldf, dim, labels, pixels, classes, sums, sq, counts, st), "proto_accumulate")


def proto_update(sums, sq, counts, classes, dim, momentum, min_pixels, tau_scale, clear, proto, spread, seen, last_counts, inv_tau,
                 st=None):
    """proto / spread / seen from the accumulated batch (first sight or EMA), last_counts = counts, the accumulators zeroed with
    ``clear``, inv_tau [1] fp32 from the spreads with ``tau_scale > 0``; include/udaseg.h has the arithmetic."""
    check(ops.udaseg_proto_update(sums, sq, counts, classes, dim, float(momentum), int(min_pixels), float(tau_scale),
                                  int(bool(clear)), proto, spread, seen, last_counts, inv_tau, st), "proto_update")


def proto_rectify(feat_base, ldf, dim, scores_base, ldc, classes, probs, proto, seen, inv_tau, pixels, out, st=None):
    """out [pixels * ldc] fp32 = the class probabilities of scores [pixels * ldc] re-weighted by the distance of feat [pixels * ldf]
    to the seen prototypes and renormalised; NaN rows for non-finite pixels."""
    check(ops.udaseg_proto_rectify(feat_base, ldf, dim, scores_base, ldc, classes, int(bool(probs)), proto, seen, inv_tau, pixels,
                                   out, st), "proto_rectify")


def proto_assign(feat_base, ldf, dim, classes, ldc, proto, seen, inv_tau, pixels, out, st=None):
    """out [pixels * ldc] fp32 = the soft assignment of feat [pixels * ldf] to the seen prototypes (softmax of -d / tau over them);
    NaN rows for non-finite pixels, 1 / classes everywhere while no class is seen."""
    check(ops.udaseg_proto_assign(feat_base, ldf, dim, classes, ldc, proto, seen, inv_tau, pixels, out, st), "proto_assign")


def proto_contrast_fwd_bwd(feat_base, ldf, dim, labels, target_base, ldt, weight_px, weight_img, batch, pix_per_image, classes, proto,
                           seen, inv_tau, mean, denom, partials, loss, dfeat=None, stats=None, st=None):
    """loss = the weighted cross entropy of the pixels' prototype assignment against uint8 labels [pixels] or a target distribution
    [pixels * ldt] (exactly one of them); dfeat (optional) [pixels * ldf] its gradient with respect to the FEATURES for an upstream
    gradient of 1, made in the same pass; stats (optional) int64 [4], accumulated.  include/udaseg.h has the arithmetic and the
    void rule."""
    check(ops.udaseg_proto_contrast_fwd_bwd(feat_base, ldf, dim, labels, target_base, ldt, weight_px, weight_img, batch,
                                            pix_per_image, classes, proto, seen, inv_tau, int(bool(mean)), denom, partials, loss,
                                            dfeat, stats, st), "proto_contrast_fwd_bwd")


def classmix_select(hist, n, classes, min_pixels, keys, sel, st=None):
    """sel [n] int32 = the class selection of every source mask from its row of the [n,256] int64 mask histogram and its Philox
    key (keys [n,2] int32 bit patterns): half of the present classes, rounded up (mix.py's module docstring has the rule)."""
    check(ops.udaseg_classmix_select(hist, n, classes, min_pixels, keys, sel, st), "classmix_select")


def classmix_u8(src, src_masks, tgt, tgt_masks, sel, boxes, n, h, w, classes, void_label, out, out_masks, counts, st=None):
    """out [n,h,w,3] / out_masks [n,h,w] uint8 = the source where its class is selected (or inside the sample's box), the target
    (tgt_masks None: void_label) elsewhere; counts [n,3] int64 or None += pasted, kept target labels, void."""
    check(ops.udaseg_classmix_u8(src, src_masks, tgt, tgt_masks, sel, boxes, n, h, w, classes, void_label, out, out_masks, counts, st),
          "classmix_u8")


def fda_spectrum_u8(frames, tw_h, tw_w, n, h, w, bmax, rows_ws, coeffs, st=None):
    """coeffs [n,3,K,K,2] float64 = the K x K lowest frequencies (K = 2 bmax + 1) of every channel of uint8 frames [n,h,w,3], through
    rows_ws [n,3,h,K,2] float64; tw_h [h,2] / tw_w [w,2]: the float64 (cos, sin) tables (fda.py's module docstring)."""
    check(ops.udaseg_fda_spectrum_u8(frames, tw_h, tw_w, n, h, w, bmax, rows_ws, coeffs, st), "fda_spectrum_u8")


def fda_amplitude(coeffs, count, amps, st=None):
    """amps [count] float64 = the moduli of count (re, im) float64 coefficients."""
    check(ops.udaseg_fda_amplitude(coeffs, count, amps, st), "fda_amplitude")


def fda_delta(coeffs, amps, pick, b, lam, n, m, h, w, bmax, delta, st=None):
    """delta [n,3,K,K,2] float32 = lam (|F_t| - |F_s|) F_s / |F_s| / (h w) inside every sample's band b [n] int32, 0 outside; amps
    [m,3,K,K] float64, pick [n] int32 the row of amps per sample, lam [n] float32."""
    check(ops.udaseg_fda_delta(coeffs, amps, pick, b, lam, n, m, h, w, bmax, delta, st), "fda_delta")


def fda_apply_u8(src, delta, b, tw_h, tw_w, n, h, w, bmax, cols_ws, out, field, counts, st=None):
    """out [n,h,w,3] uint8 and / or field [n,h,w,3] float32 = src + the real inverse transform of delta; counts [n,2] int64 or None
    += values below 0, above 255; cols_ws [n,3,K,w,2] float32; tw_h / tw_w: the float32 tables."""
    check(ops.udaseg_fda_apply_u8(src, delta, b, tw_h, tw_w, n, h, w, bmax, cols_ws, out, field, counts, st), "fda_apply_u8")


def _ignore_args(ignore_index):
    """ignore_index (None or any int64) -> (has_ignore, ignore_index) as the C ABI takes them."""
    return (0, 0) if ignore_index is None else (1, int(ignore_index))


def _label_args(labels):
    """A label map [n,h,w] (uint8 or int64) -> (labels_i64, n, h, w) as the C ABI takes them."""
    return (int(getattr(labels, "dtype", None) == torch.int64),) + tuple(getattr(labels, "shape", ()))


RENDER_BASE_NONE, RENDER_BASE_U8, RENDER_BASE_F32, RENDER_BASE_BF16 = 0, 1, 2, 3
_RENDER_HOST = {}


def render_u8(labels, truth, base, table, n, h, w, classes, ignore_index, alpha, denorm, outline, out, counts, agreement, st=None):
    """out [n,h,w,3] uint8 = the rendering of labels [n,h,w] (uint8 or int64; truth None or alike) over base (None, a uint8
    [n,h,w,3] frame or the padded fp32 [n,h,w,4] / bf16 [n,h,w,8] model input: the kind follows its dtype).  table: uint8 [256,3]
    on the device; alpha: four integers in [0, 256]; denorm: six floats (std * 255, mean * 255) or None; ignore_index: an int or
    None; outline: r | g << 8 | b << 16 or -1; counts [n,256] / agreement [n,3] int64 or None (they accumulate)."""
    kind = RENDER_BASE_NONE if base is None else {torch.uint8: RENDER_BASE_U8, torch.float32: RENDER_BASE_F32,
                                                   torch.bfloat16: RENDER_BASE_BF16}.get(getattr(base, "dtype", None), RENDER_BASE_F32)
    key = (tuple(alpha), None if denorm is None else tuple(denorm))
    host = _RENDER_HOST.get(key)
    if host is None:                         # the two small host arrays of a call are kept: callers render with the same few tables
        if len(_RENDER_HOST) > 256:
            _RENDER_HOST.clear()
        host = _RENDER_HOST[key] = ((_lib.C.c_int32 * 4)(*[int(v) for v in key[0]]),
                                    None if denorm is None else (_lib.C.c_float * 6)(*[float(v) for v in key[1]]))
    a4, d6 = host
    check(ops.udaseg_render_u8(labels, truth, _label_args(labels)[0], base, kind, table, n, h, w, classes, *_ignore_args(ignore_index),
                               a4, d6, outline, out, counts, agreement, st), "render_u8")


# ---- label boundary distances (boundary.py; csrc/boundary.hip).  labels: uint8 or int64 [n,h,w]; ignore_index: an int or None
def _boundary_head(labels, radius, ignore_index):
    return _label_args(labels) + (int(radius),) + _ignore_args(ignore_index)


def boundary_tile(radius, stats=False):
    """(tile height, tile width) of the launch at this radius."""
    v = _lib.load().udaseg_boundary_tile(int(radius), int(bool(stats)))
    if v < 0:
        check(v, "boundary_tile")
    return v >> 16, v & 0xffff


def boundary_d2(labels, radius, ignore_index, d2, st=None):
    """d2 [n,h,w] int32 = the capped squared distance to the nearest label boundary (radius * radius + 1: further than radius)."""
    check(ops.udaseg_boundary_d2(labels, *_boundary_head(labels, radius, ignore_index), d2, st), "boundary_d2")


def boundary_lookup(labels, radius, ignore_index, table, out, st=None):
    """out [n,h,w] fp32 = table[d2] (table [radius * radius + 3] fp32 on the device; the last slot is the void pixels')."""
    check(ops.udaseg_boundary_lookup(labels, *_boundary_head(labels, radius, ignore_index), table, out, st), "boundary_lookup")


def boundary_erode(labels, radius, ignore_index, void_label, out, counts, st=None):
    """out [n,h,w] uint8 = labels with void_label within radius of a boundary; counts [n,2] int64 or None += voided, void before."""
    check(ops.udaseg_boundary_erode(labels, *_boundary_head(labels, radius, ignore_index), int(void_label), out, counts, st),
          "boundary_erode")


def boundary_stats(pred, truth, radius, classes, ignore_index, stats, trimap, st=None):
    """stats [classes,3] / trimap [2] int64 += the band counters of pred against truth (one dtype, one shape)."""
    i64, n, h, w, r, has, ign = _boundary_head(truth, radius, ignore_index)
    check(ops.udaseg_boundary_stats(pred, truth, i64, n, h, w, r, int(classes), has, ign, stats, trimap, st), "boundary_stats")


# ---- connected components (regions.py; csrc/regions.hip).  labels: uint8 or int64 [n,h,w]; ignore_index: an int or None
def regions_tile():
    """(tile height, tile width) of the labelling: regions are labelled per tile, then joined across the seams."""
    v = _lib.load().udaseg_regions_tile()
    return v >> 16, v & 0xffff


def regions_label(labels, connectivity, ignore_index, ids, area, st=None):
    """ids [n,h,w] int32 = the first raster index of every pixel's component (-1: void); area [n,h,w] int32 or None = its size."""
    check(ops.udaseg_regions_label(labels, *_label_args(labels), int(connectivity), *_ignore_args(ignore_index), ids, area, st),
          "regions_label")


def regions_sieve(labels, ids, area, ignore_index, min_area, void_label, out, counts, st=None):
    """out [n,h,w] uint8 = labels with void_label on the components smaller than min_area[label] (int32 [256] on the device);
    counts [n,3] int64 or None += pixels voided, components removed, components kept."""
    i64, n, h, w = _label_args(labels)
    check(ops.udaseg_regions_sieve(labels, i64, ids, area, n, h, w, *_ignore_args(ignore_index), min_area, int(void_label), out,
                                   counts, st), "regions_sieve")


def regions_stats(labels, ids, area, classes, ignore_index, stats, st=None):
    """stats [classes,34] int64 += components, pixels and the log2 area histogram [32] of every class."""
    i64, n, h, w = _label_args(labels)
    check(ops.udaseg_regions_stats(labels, i64, ids, area, n, h, w, int(classes), *_ignore_args(ignore_index), stats, st),
          "regions_stats")


def regions_label_i32(labels, connectivity, ids, area, st=None):
    """``regions_label`` of an int32 map [n,h,w]: every value >= 0 a label of its own, a negative one void."""
    n, h, w = getattr(labels, "shape", (0, 0, 0))
    check(ops.udaseg_regions_label_i32(labels, n, h, w, int(connectivity), ids, area, st), "regions_label_i32")


# ---- superpixels (superpixels.py; csrc/superpixels.hip).  ids / labels: int32 [n,h,w]; centres: int32 [n,K,6]
def superpixel_slic(frames, step, compactness, iterations, min_area, ids, centres, counts=None, st=None):
    """ids [n,h,w] int32 = the 4-connected integer SLIC superpixels of uint8 frames [n,h,w,3]; centres [n,K,6] int32 = the last
    update's; counts [n,4] int64 or None += components found, absorbed, pixels relabelled, clusters left."""
    n, h, w, _ = frames.shape
    check(ops.udaseg_superpixel_slic(frames, n, h, w, int(step), int(compactness), int(iterations), int(min_area), ids, centres,
                                     counts, st), "superpixel_slic")


def superpixel_assign(frames, step, compactness, centres, labels=None, st=None):
    """One iteration from ``centres`` (updated in place); labels [n,h,w] int32 or None = the assignment it was made from."""
    n, h, w, _ = frames.shape
    check(ops.udaseg_superpixel_assign(frames, n, h, w, int(step), int(compactness), centres, labels, st), "superpixel_assign")


def superpixel_connect(labels, step, min_area, ids, counts=None, st=None):
    """ids = the connect step of ``superpixel_slic`` alone on cluster indices of the grid of ``step`` (ids may be labels)."""
    n, h, w = labels.shape
    check(ops.udaseg_superpixel_connect(labels, n, h, w, int(step), int(min_area), ids, counts, st), "superpixel_connect")


def superpixel_vote(ids, masks, clusters, classes, ignore_index, min_share, min_cover, void_label, out, counts=None, st=None):
    """out [n,h,w] uint8 = the winning class of every pixel's superpixel, or void_label; counts [n,3] int64 or None += changed,
    filled, voided."""
    i64, n, h, w = _label_args(masks)
    check(ops.udaseg_superpixel_vote(ids, masks, i64, n, h, w, int(clusters), int(classes), *_ignore_args(ignore_index),
                                     float(min_share), float(min_cover), int(void_label), out, counts, st), "superpixel_vote")


def superpixel_mean(values, ids, clusters, mean, st=None):
    """mean [n,clusters] fp32 = the mean of the values in [0, 1] of every superpixel, -1 where it has none."""
    n, h, w = ids.shape
    check(ops.udaseg_superpixel_mean(values, ids, n, h, w, int(clusters), mean, st), "superpixel_mean")


def superpixel_gather(ids, table, clusters, mask, st=None):
    """mask [n,h,w] uint8 |= table[n,clusters][ids]."""
    n, h, w = ids.shape
    check(ops.udaseg_superpixel_gather(ids, table, n, h, w, int(clusters), mask, st), "superpixel_gather")


# ---- CRF refinement (crf.py; csrc/crf.hip).  Score rows are padded NHWC: [pixels][ld] fp32
def crf_tile(radius, dilation):
    """(tile height, tile width) of ``crf_step``'s blocks at this window."""
    v = _lib.load().udaseg_crf_tile(int(radius), int(dilation))
    if v == 0:
        raise ValueError(f"crf_tile: need 1 <= radius <= 5, 1 <= dilation <= 4, radius * dilation <= 10, got {radius}, {dilation}")
    return v >> 16, v & 0xffff


def crf_prepare(scores, ldc, classes, probs, pixels, logp, q0, ldq, valid, st=None):
    """logp, q0 [pixels * ldq] fp32 = log P0 and P0 of scores [pixels * ldc]; valid [pixels] uint8; NaN rows at invalid pixels."""
    check(ops.udaseg_crf_prepare(scores, ldc, classes, int(bool(probs)), pixels, logp, q0, ldq, valid, st), "crf_prepare")


def crf_step(logp, q, valid, frames, classes, ldq, radius, dilation, s_alpha, s_gamma, w_app, w_smooth, inv2b, strength, q_out,
             st=None):
    """q_out = one mean-field sweep of q under uint8 frames [n,h,w,3]; the spatial tables are fp32 [(2 radius + 1)^2] on the device."""
    n, h, w, _ = frames.shape
    check(ops.udaseg_crf_step(logp, q, valid, frames, n, h, w, classes, ldq, int(radius), int(dilation), s_alpha, s_gamma,
                              float(w_app), float(w_smooth), float(inv2b), float(strength), q_out, st), "crf_step")


# ---- window votes and active label acquisition (active.py; csrc/window.hip).  labels: uint8 or int64 [n,h,w]
def _window_head(labels, radius, classes, ignore_index):
    return _label_args(labels) + (int(radius), int(classes)) + _ignore_args(ignore_index)


def window_tile(radius):
    """(tile height, tile width) of the window kernels' launch at this radius."""
    v = _lib.load().udaseg_window_tile(int(radius))
    if v < 0:
        check(v, "window_tile")
    return v >> 16, v & 0xffff


def window_mode(labels, radius, classes, ignore_index, fill_void, void_label, out, agreement=None, counts=None, st=None):
    """out [n,h,w] uint8 = the mode of the window's labels; agreement [n,h,w] fp32 or None = its share of the window; counts [n,3]
    int64 or None += changed, void filled, void left."""
    check(ops.udaseg_window_mode(labels, *_window_head(labels, radius, classes, ignore_index), int(bool(fill_void)), int(void_label),
                                 out, agreement, counts, st), "window_mode")


def window_impurity(labels, radius, classes, ignore_index, table, out, st=None):
    """out [n,h,w] fp32 = the normalised entropy of the window's label histogram (table: fp32 [(2 radius + 1)^2 + 1] of m log m)."""
    check(ops.udaseg_window_impurity(labels, *_window_head(labels, radius, classes, ignore_index), table, out, st), "window_impurity")


def acquire_prepare(scores, ldc, classes, probs, pixels, labels, entropy, counters, st=None):
    """labels [pixels] uint8 = the first maximal class (255: a non-finite row), entropy [pixels] fp32; counters [2] int64 += finite,
    non-finite rows."""
    check(ops.udaseg_acquire_prepare(scores, ldc, classes, int(bool(probs)), pixels, labels, entropy, counters, st), "acquire_prepare")


def acquire_score(labels, entropy, exclude, radius, classes, kind, table, score, key, st=None):
    """score, key [n,h,w] fp32 of uint8 labels and their entropy map; exclude: uint8 [n,h,w] or None; kind 0 / 1 / 2."""
    n, h, w = labels.shape
    check(ops.udaseg_acquire_score(labels, entropy, exclude, n, h, w, int(radius), int(classes), int(kind), table, score, key, st),
          "acquire_score")


def acquire_cells(key, cell_h, cell_w, cell_key, st=None):
    """cell_key [n, ceil(h / cell_h), ceil(w / cell_w)] fp32 = 1 - the mean score of the cell, -1 without a candidate."""
    n, h, w = key.shape
    check(ops.udaseg_acquire_cells(key, n, h, w, int(cell_h), int(cell_w), cell_key, st), "acquire_cells")


def acquire_select(key, thresholds, mask, counts=None, st=None):
    """mask [n, ...] uint8 |= (0 <= key <= thresholds[i]); counts [n,2] int64 or None += newly selected, candidates."""
    n = key.shape[0]
    check(ops.udaseg_acquire_select(key, thresholds, n, key.numel() // n, mask, counts, st), "acquire_select")


def acquire_expand(cell_mask, cell_h, cell_w, mask, st=None):
    """mask [n,h,w] uint8 |= the rectangles of the selected cells."""
    n, h, w = mask.shape
    check(ops.udaseg_acquire_expand(cell_mask, n, h, w, int(cell_h), int(cell_w), mask, st), "acquire_expand")


def conv2d_fwd_bf16(d, x, w, bias, residual, y, act=ACT_NONE, slope=0.0, stats=None, st=None):
    """bf16 x / w / residual; y bf16, or fp32 when its dtype says so (logits)."""
    check(ops.udaseg_conv2d_fwd_bf16(d, x, w, bias, residual, y,
                                              int(y.dtype == torch.float32), act, slope, stats,
                                              st), "conv2d_fwd_bf16")


def conv2d_dgrad_bf16(d, dy, w_t, dx, accumulate=False, st=None):
    check(ops.udaseg_conv2d_dgrad_bf16(d, dy, w_t, dx, int(accumulate),
                                                st), "conv2d_dgrad_bf16")


def conv2d_wgrad_bf16(d, x, dy, dw, accumulate=False, st=None):
    check(ops.udaseg_conv2d_wgrad_bf16(d, x, dy, dw, int(accumulate),
                                                st), "conv2d_wgrad_bf16")


def conv2d_dgrad(d, dy, w_t, dx, accumulate=False, st=None):
    if dy.dtype == torch.bfloat16:
        return conv2d_dgrad_bf16(d, dy, w_t, dx, accumulate, st)
    check(ops.udaseg_conv2d_dgrad(d, dy, w_t, dx, int(accumulate),
                                           st), "conv2d_dgrad")


def conv2d_dgrad_bnreduce_ok(d, dtype=torch.float32):
    if dtype == torch.bfloat16:
        return bool(ops.udaseg_conv2d_dgrad_bnreduce_bf16_ok(d))
    return dtype == torch.float32 and bool(ops.udaseg_conv2d_dgrad_bnreduce_ok(d))


def conv2d_dgrad_bnreduce(d, dy, w_t, dx, prev_y, save_mean, save_rstd, gamma, beta, act, slope, bsums, st=None):
    """dx = dgrad AND the BatchNorm-backward reductions (sum g, sum g*xhat) of the layer whose output prev_y feeds this conv."""
    fn = ops.udaseg_conv2d_dgrad_bnreduce_bf16 if dy.dtype == torch.bfloat16 else ops.udaseg_conv2d_dgrad_bnreduce
    check(fn(d, dy, w_t, dx, prev_y, save_mean,
             save_rstd, gamma, beta, act, slope, bsums,
             st), "conv2d_dgrad_bnreduce")


def conv2d_wgrad(d, x, dy, dw, accumulate=False, st=None):
    if x.dtype == torch.bfloat16:
        return conv2d_wgrad_bf16(d, x, dy, dw, accumulate, st)
    check(ops.udaseg_conv2d_wgrad(d, x, dy, dw, int(accumulate),
                                           st), "conv2d_wgrad")


def conv2d_fwd_upcat(d, a, skip, w, bias, y, act=ACT_NONE, slope=0.0, stats=None, st=None):
    """y = act(conv(cat([nearest_x2(a), skip], C), w) + bias) without materialising the concatenation (+ BN statistics of y)."""
    fn = ops.udaseg_conv2d_fwd_upcat_bf16 if a.dtype == torch.bfloat16 else ops.udaseg_conv2d_fwd_upcat
    check(fn(d, a, skip, a.shape[-1], w, bias, y, act, slope, stats,
             st), "conv2d_fwd_upcat")


def conv2d_dgrad_split(d, dy, w_t, dx_a, dx_b, st=None):
    fn = ops.udaseg_conv2d_dgrad_split_bf16 if dy.dtype == torch.bfloat16 else ops.udaseg_conv2d_dgrad_split
    check(fn(d, dy, w_t, dx_a, dx_b, dx_a.shape[-1],
             st), "conv2d_dgrad_split")


def conv2d_wgrad_part(d, src, c_off, up, dy, dw, accumulate=True, st=None):
    fn = ops.udaseg_conv2d_wgrad_part_bf16 if src.dtype == torch.bfloat16 else ops.udaseg_conv2d_wgrad_part
    check(fn(d, src, src.shape[-1], c_off, int(up), dy, dw, int(accumulate),
             st), "conv2d_wgrad_part")


def upcat_fusable(ca, cb, co, dtype):
    """Can the convolution over cat([up(a), skip]) take the fused gather?  Channel counts that are multiples of the K-tile
    for the implicit-GEMM kernels (32 fp32 / 64 bf16) plus a 64-channel boundary for the data gradient's two outputs, or the
    fp32 small-channel kernel (<= 32 channels in all, no skip)."""
    if dtype == torch.bfloat16:
        return ca % 64 == 0 and cb % 64 == 0
    g_in, g_out = (ca + cb + 15) // 16, (co + 15) // 16
    if cb == 0 and g_in * g_out <= 2:
        return True
    return ca % 32 == 0 and cb % 32 == 0 and (cb == 0 or ca % 64 == 0)


def bn_finalize(sums, gamma, beta, pixels, eps, momentum, running_mean, running_var, save_mean, save_rstd, scale, shift, st=None):
    """Statistics -> saved mean / rstd, running statistics and the per-channel scale / shift a consumer applies while staging."""
    c = scale.numel()
    check(ops.udaseg_bn_finalize(sums, gamma, beta, pixels, c, eps, momentum,
                                          running_mean, running_var, save_mean, save_rstd, scale,
                                          shift, st), "bn_finalize")


def bn_bwd_apply_recompute(dz, y, fwd_scale, fwd_shift, save_mean, save_rstd, gamma, bsums, dy, dgamma, dbeta, act, slope, st=None):
    """BatchNorm backward of a layer whose activation was never written: the mask is re-evaluated from y, fwd_scale, fwd_shift."""
    c = y.shape[-1]
    if y.dtype != torch.bfloat16:
        raise ValueError("bn_bwd_apply_recompute: bf16 storage only")
    check(ops.udaseg_bn_bwd_apply_recompute_bf16(dz, y, fwd_scale, fwd_shift,
                                                          save_mean, save_rstd, gamma,
                                                          bsums, dy, dgamma, dbeta, y.numel() // c,
                                                          c, act, slope, st),
          "bn_bwd_apply_recompute_bf16")


def conv2d_wgrad_halo_ok(d, up_ca=0, f32=False):
    if f32:
        return bool(ops.udaseg_conv2d_wgrad_halo_f32x3_ok(d, up_ca))
    return bool(ops.udaseg_conv2d_wgrad_halo_bf16_ok(d, up_ca))


def conv2d_wgrad_halo(d, x, skip, dy, dw, up=False, st=None):
    """dW += weight gradient of a stride-1 3x3 layer (channel counts multiples of 64) on the halo-resident kernel: bf16 tensors,
    or fp32 tensors with the exact three-term split.  up: x is the half-resolution source of a fused decoder input, skip the
    other one."""
    fn, name = ((ops.udaseg_conv2d_wgrad_halo_f32x3, "conv2d_wgrad_halo_f32x3") if x.dtype == torch.float32
                else (ops.udaseg_conv2d_wgrad_halo_bf16, "conv2d_wgrad_halo_bf16"))
    check(fn(d, x, skip, x.shape[-1] if up else 0, dy, dw,
             st), name)


def conv_bnin_ok(d, up=False):
    """fp32: can BOTH consumers of an unwritten BatchNorm activation in front of this convolution apply it while staging?
    (forward on the split kernels, weight gradient on the small-channel direct kernel or the halo-resident split kernel)
    up: the activation reaches the convolution through a nearest x2 up-sampling (d describes the up-sampled geometry)."""
    return bool(ops.udaseg_conv2d_fwd_f32x3_bnin_ok(d, int(up))) and bool(ops.udaseg_conv2d_wgrad_bnin_ok(d, int(up)))


def conv_bnin_writes(d):
    """fp32: the forward of this convolution can write the transformed activation out while it stages it (wave-specialised kernel)"""
    return bool(ops.udaseg_conv2d_fwd_f32x3_bnin_writes(d)) and bool(ops.udaseg_conv2d_fwd_f32x3_bnin_ok(d, 0))


def conv2d_wgrad_bnin(d, y_prev, in_scale, in_shift, in_act, in_slope, dy, dw, accumulate=False, st=None, up=False):
    """Weight gradient whose gathered operand is act(fma(y_prev, in_scale, in_shift)) (never written), bf16 or fp32."""
    if y_prev.dtype == torch.float32:
        check(ops.udaseg_conv2d_wgrad_bnin(d, y_prev, int(up), in_scale, in_shift, in_act, in_slope, dy, dw, int(accumulate),
                                           st), "conv2d_wgrad_bnin")
        return
    check(ops.udaseg_conv2d_wgrad_bnin_bf16(d, y_prev, in_scale, in_shift, in_act,
                                                     in_slope, dy, dw, int(accumulate),
                                                     st), "conv2d_wgrad_bnin_bf16")


def frag_elems(n_out, k_in, ks):
    """bf16 elements of the MFMA-fragment packing of a convolution with n_out produced / k_in gathered channels, ks x ks window."""
    return int(ops.udaseg_frag_elems(n_out, k_in, ks))


def pack_frag_batched(w, wt, packed, table, st=None):
    """Fragment-pack every listed convolution in one launch (table rows: mode, src offset, dst offset, N, K, ks; int32 x 6).
    bf16 sources: one plane (csrc/conv_halo_bf16.hip); fp32 sources: the three split planes (csrc/conv_halo_f32x3.hip)."""
    src = w if w is not None else wt
    if src.dtype == torch.float32:
        check(ops.udaseg_pack_frag_batched_f32x3(w, wt, packed, table, table.shape[0],
                                                          st), "pack_frag_batched_f32x3")
        return
    check(ops.udaseg_pack_frag_batched_bf16(w, wt, packed, table, table.shape[0],
                                                     st), "pack_frag_batched_bf16")


def pack_up_batched(w, wt, packed, table, st=None):
    """Fragment packings of the decoder conv1 layers whose up-sampled half runs as four 2x2 phase convolutions
    (csrc/conv_up_f32x3.hip): table rows of 8 int32 {mode, src offset, dst offset, N, K, ldk, 0, 0}."""
    check(ops.udaseg_pack_up_batched_f32x3(w, wt, packed, table, table.shape[0], st), "pack_up_batched_f32x3")


def conv_up_ok(d, up_ca):
    return bool(ops.udaseg_conv_up_f32x3_ok(d, up_ca))


def conv2d_fwd_up(d, a, wfrag_up, y, accumulate=False, stats=None, st=None):
    """y (+)= conv3x3(nearest_x2(a)) as four 2x2 phase convolutions of a (fp32, three-term split); d: the whole decoder conv1."""
    check(ops.udaseg_conv2d_fwd_up_f32x3(d, a, a.shape[-1], wfrag_up, y, int(accumulate), stats, st), "conv2d_fwd_up_f32x3")


# the ``bn=`` operand of the data-gradient launches when no BatchNorm-backward reduction rides in the epilogue:
# (prev_y, save_mean, save_rstd, gamma, beta, act, slope, bsums), built by engine.ConvRecord.bn_reduce_args
NO_BN = (None, None, None, None, None, ACT_NONE, 0.0, None)


def conv2d_dgrad_up(d, dy, up_ca, wfrag_up_t, da, accumulate=False, bn=None, st=None):
    """da (+)= gradient of a through conv3x3(nearest_x2(a)), at a's resolution.
    bn = (prev_y, save_mean, save_rstd, gamma, beta, act, slope, bsums): BatchNorm-backward reductions of the layer that produced a."""
    py, mu, rs, ga, be, act, slope, bs = bn or NO_BN
    check(ops.udaseg_conv2d_dgrad_up_f32x3(d, dy, up_ca, wfrag_up_t, da, py, mu, rs, ga, be, act, slope, bs, int(accumulate), st),
          "conv2d_dgrad_up_f32x3")


def conv2d_wgrad_up_ok(d, up_ca):
    return bool(ops.udaseg_conv2d_wgrad_up_f32x3_ok(d, up_ca))


def conv2d_wgrad_up(d, a, dy, dw, st=None):
    """dW[..., :ca] += weight gradient of conv3x3(nearest_x2(a)) in the phase form (16 phase taps at a's resolution); d: the whole
    decoder conv1, dW its [co][3][3][ci] gradient."""
    check(ops.udaseg_conv2d_wgrad_up_f32x3(d, a, a.shape[-1], dy, dw, st), "conv2d_wgrad_up_f32x3")


def conv2d_wgrad_halo_slice(d_slice, x, dy, dw, c_off, st=None):
    """dW[..., c_off:c_off + x channels] += halo-resident weight gradient of the slice (d_slice: the slice as its own convolution)."""
    check(ops.udaseg_conv2d_wgrad_halo_slice_f32x3(d_slice, x, dy, dw, dw.shape[-1], c_off, st), "conv2d_wgrad_halo_slice_f32x3")


STEM_FRAG_ELEMS = 3 * 28 * 512


def conv_stem_ok(d):
    return bool(ops.udaseg_conv_stem_f32x3_ok(d))


def conv2d_fwd_stem(d, x, wfrag, y, stats=None, st=None):
    """The encoder's 7x7 / stride 2 stem on its own kernel (csrc/conv_stem_f32x3.hip, mode-8 packing)."""
    check(ops.udaseg_conv2d_fwd_stem_f32x3(d, x, wfrag, y, stats, st), "conv2d_fwd_stem_f32x3")


def conv_stem_wgrad_bn_ok(d):
    """May the stem's weight gradient form dy = bn_bwd_apply(dz, y) in its staging (csrc/conv_stem_wgrad.hip)?  Geometry, the
    device's LDS and the STEM_WGRAD_BN switch; the caller knows whether the layer has a residual input or an unwritten activation."""
    return bool(ops.udaseg_conv_stem_wgrad_bn_ok(d))


def conv2d_wgrad_stem_bn(d, x, dz, y, save_mean, save_rstd, gamma, beta, bsums, act, slope, dw, dgamma, dbeta, accumulate=True,
                         accumulate_param=False, st=None):
    """dW (+)= the 7x7 / stride 2 stem's weight gradient from x and the never-stored dy = bn_bwd_apply(dz, y); dgamma / dbeta as
    bn_bwd_apply writes them.  bsums: bn_bwd_reduce's."""
    check(ops.udaseg_conv2d_wgrad_stem_bn(d, x, dz, y, save_mean, save_rstd, gamma, beta, bsums, act, slope, dw, dgamma, dbeta,
                                          int(accumulate), int(accumulate_param), st), "conv2d_wgrad_stem_bn")


def stem_wgrad_set_blocks(blocks):
    """tests / tuning: cap on the blocks of a conv2d_wgrad_stem_bn launch (0: one per CU)."""
    check(ops.udaseg_stem_wgrad_set_blocks(int(blocks)), "stem_wgrad_set_blocks")


def conv_n16_ok(d, dgrad=False):
    return bool(ops.udaseg_conv_n16_f32x3_ok(d, int(dgrad)))


def n16_frag_elems(k_in):
    """bf16 elements of the three-plane sixteen-wide-tile packing of a convolution gathering k_in channels."""
    return 3 * ((k_in + 15) // 16) * 5 * 512


def conv2d_fwd_n16(d, x, wfrag, y, stats=None, in_scale=None, in_shift=None, in_act=ACT_NONE, in_slope=0.0, st=None):
    """Forward 3x3 convolution producing 16 channels on the sixteen-wide matrix tile (csrc/conv_n16_f32x3.hip)."""
    check(ops.udaseg_conv2d_fwd_n16_f32x3(d, x, in_scale, in_shift, in_act, in_slope, wfrag, y, stats, st), "conv2d_fwd_n16_f32x3")


def conv2d_dgrad_n16(d, dy, wfrag_t, dx, bn=None, st=None):
    """Data gradient of a 3x3 convolution with 16 input channels on the sixteen-wide tile; bn as conv2d_dgrad_frag."""
    py, mu, rs, ga, be, act, slope, bs = bn or NO_BN
    check(ops.udaseg_conv2d_dgrad_n16_f32x3(d, dy, wfrag_t, dx, py, mu, rs, ga, be, act, slope, bs, st), "conv2d_dgrad_n16_f32x3")


def conv_frag_ok(d, dgrad=False, up_ca=0, f32=False):
    if f32:
        return bool(ops.udaseg_conv_f32x3_ok(d, int(dgrad), up_ca))
    return bool(ops.udaseg_conv_frag_ok(d, int(dgrad), up_ca))


def conv_frag_preferred(d, dgrad=False, up_ca=0, f32=False):
    """Supported AND expected to beat the shared implicit-GEMM kernel for this shape (the library's measured heuristic)."""
    if f32:
        return bool(ops.udaseg_conv_f32x3_preferred(d, int(dgrad), up_ca))
    return bool(ops.udaseg_conv_frag_preferred(d, int(dgrad), up_ca))


def conv2d_fwd_frag(d, x, skip, wfrag, bias, y, act=ACT_NONE, slope=0.0, stats=None, in_scale=None, in_shift=None, in_act=ACT_NONE,
                    in_slope=0.0, up=False, st=None, z_out=None):
    """Halo-resident forward convolution on the bf16 matrix pipe: bf16 tensors (csrc/conv_halo_bf16.hip) or fp32 tensors with
    the three-term split (csrc/conv_halo_f32x3.hip).  up: x is the half-resolution tensor of a fused decoder input."""
    if x.dtype == torch.float32 and in_scale is not None:
        assert y.dtype == torch.float32 and skip is None
        check(ops.udaseg_conv2d_fwd_f32x3_bnin(d, x, int(up), in_scale, in_shift, in_act, in_slope, z_out, wfrag, bias, y, act, slope,
                                               stats, st), "conv2d_fwd_f32x3_bnin")
        return
    assert z_out is None
    if x.dtype == torch.float32:
        assert y.dtype == torch.float32
        check(ops.udaseg_conv2d_fwd_f32x3(d, x, skip, x.shape[-1] if up else 0, wfrag,
                                                   bias, y, act, slope, stats,
                                                   st), "conv2d_fwd_f32x3")
        return
    check(ops.udaseg_conv2d_fwd_frag_bf16(d, x, skip, x.shape[-1] if up else 0, wfrag,
                                                   bias, in_scale, in_shift, in_act, in_slope, y,
                                                   int(y.dtype == torch.float32), act, slope, stats,
                                                   st), "conv2d_fwd_frag_bf16")


def conv2d_dgrad_frag(d, dy, wfrag_t, dx, dx2=None, bn=None, accumulate=False, st=None):
    """Halo-resident data gradient (bf16 tensors, or fp32 tensors with the three-term split).  dx2: second destination of a
    split gradient (channels [dx.shape[-1], ci)).
    bn = (prev_y, save_mean, save_rstd, gamma, beta, act, slope, bsums): BatchNorm-backward reductions of the layer behind."""
    py, mu, rs, ga, be, act, slope, bs = bn or NO_BN
    fn, name = ((ops.udaseg_conv2d_dgrad_f32x3, "conv2d_dgrad_f32x3") if dy.dtype == torch.float32
                else (ops.udaseg_conv2d_dgrad_frag_bf16, "conv2d_dgrad_frag_bf16"))
    check(fn(d, dy, wfrag_t, dx, dx2, dx.shape[-1] if dx2 is not None else 0,
             py, mu, rs, ga, be, act, slope, bs, int(accumulate),
             st), name)


def pack_dgrad_weights(d, w, w_t, st=None):
    check(ops.udaseg_pack_dgrad_weights(d, w, w_t,
                                                 st), "pack_dgrad_weights")


def cast_to_bf16(x, out=None, st=None):
    """fp32 -> bf16 (round to nearest even), flat; numel must be a multiple of 8."""
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(ops.udaseg_cast_f32_to_bf16(x, out, x.numel(), st),
          "cast_f32_to_bf16")
    return out


def pack_dgrad_batched(arena, packed, table, st=None):
    if packed.dtype == torch.bfloat16:
        check(ops.udaseg_pack_dgrad_batched_bf16(arena, packed, table, table.shape[0],
                                                          st), "pack_dgrad_batched_bf16")
        return
    check(ops.udaseg_pack_dgrad_batched(arena, packed, table, table.shape[0],
                                                 st), "pack_dgrad_batched")


def conv_flops(d):
    return ops.udaseg_conv_flops(d)


def nchw_to_nhwc(x, cpad=None, st=None, dtype=torch.float32):
    """[N,C,H,W] contiguous fp32 -> [N,H,W,cpad] (zero-padded channels), fp32 or bf16."""
    n, c, h, w = x.shape
    if not x.is_contiguous():
        x = x.contiguous()
    if dtype == torch.bfloat16:
        cpad = cpad or ((c + 7) // 8) * 8
        y = torch.empty((n, h, w, cpad), device=x.device, dtype=torch.bfloat16)
        check(ops.udaseg_nchw_to_nhwc_bf16(x, y, n, c, h, w, cpad,
                                                    st), "nchw_to_nhwc_bf16")
        return y
    cpad = cpad or ((c + 3) // 4) * 4
    y = torch.empty((n, h, w, cpad), device=x.device, dtype=torch.float32)
    check(ops.udaseg_nchw_to_nhwc(x, y, n, c, h, w, cpad,
                                           st), "nchw_to_nhwc")
    return y


_BN_R = None


def bn_replicas():
    global _BN_R
    if _BN_R is None:
        _BN_R = ops.udaseg_bn_replicas()
    return _BN_R


def bn_stats(y, sums, st=None):
    c = y.shape[-1]
    if y.dtype not in (torch.float32, torch.bfloat16) or not y.is_contiguous():
        raise ValueError(f"bn_stats: contiguous fp32 or bf16 tensor expected, got {y.dtype}")
    fn = ops.udaseg_bn_stats_bf16 if y.dtype == torch.bfloat16 else ops.udaseg_bn_stats
    check(fn(y, y.numel() // c, c, sums, st), "bn_stats")


def bn_apply(y, sums, gamma, beta, residual, z, eps, momentum, running_mean, running_var, save_mean, save_rstd, act, slope,
             st=None):
    c = y.shape[-1]
    if y.dtype == torch.bfloat16:
        check(ops.udaseg_bn_apply_bf16(y, sums, gamma, beta, residual,
                                                z, y.numel() // c, c, eps, momentum, running_mean,
                                                running_var, save_mean, save_rstd, act, slope,
                                                st), "bn_apply_bf16")
        return
    check(ops.udaseg_bn_apply(y, sums, gamma, beta, residual,
                                       z, y.numel() // c, c, eps, momentum, running_mean, running_var,
                                       save_mean, save_rstd, act, slope,
                                       st), "bn_apply")


def bn_apply_eval(y, gamma, beta, running_mean, running_var, residual, z, eps, act, slope, st=None):
    c = y.shape[-1]
    check(ops.udaseg_bn_apply_eval(y, gamma, beta, running_mean,
                                            running_var, residual, z, y.numel() // c, c, eps, act,
                                            slope, st), "bn_apply_eval")


def bn_bwd_reduce(dz, z, y, save_mean, save_rstd, bsums, act, slope, st=None, gamma=None, beta=None):
    """z=None (fp32 only, layers without a residual input): the activation's argument is re-evaluated from y, gamma, beta."""
    c = y.shape[-1]
    if y.dtype == torch.bfloat16:
        check(ops.udaseg_bn_bwd_reduce_bf16(dz, z, y, save_mean,
                                                     save_rstd, y.numel() // c, c, bsums, act, slope,
                                                     st), "bn_bwd_reduce_bf16")
        return
    check(ops.udaseg_bn_bwd_reduce(dz, z, y, save_mean, save_rstd,
                                            gamma, beta, y.numel() // c, c, bsums, act, slope,
                                            st), "bn_bwd_reduce")


def bn_bwd_apply(dz, z, y, save_mean, save_rstd, gamma, bsums, dy, dres, dgamma, dbeta, act, slope, accumulate_dy=False,
                 accumulate_dres=False, accumulate_param=False, st=None, beta=None):
    c = y.shape[-1]
    if y.dtype == torch.bfloat16:
        check(ops.udaseg_bn_bwd_apply_bf16(dz, z, y, save_mean,
                                                    save_rstd, gamma, bsums, dy,
                                                    dres, dgamma, dbeta, y.numel() // c, c, act, slope,
                                                    int(accumulate_dy), int(accumulate_dres), int(accumulate_param),
                                                    st), "bn_bwd_apply_bf16")
        return
    check(ops.udaseg_bn_bwd_apply(dz, z, y, save_mean, save_rstd,
                                           gamma, beta, bsums, dy, dres, dgamma,
                                           dbeta, y.numel() // c, c, act, slope, int(accumulate_dy),
                                           int(accumulate_dres), int(accumulate_param),
                                           st), "bn_bwd_apply")


def act_bwd(dz, z, dy, act, slope, st=None):
    if dz.dtype == torch.bfloat16:
        check(ops.udaseg_act_bwd_bf16(dz, z, dy, dz.numel(), act, slope,
                                               st), "act_bwd_bf16")
        return
    check(ops.udaseg_act_bwd(dz, z, dy, dz.numel(), act, slope,
                                      st), "act_bwd")


_CHSUM_SCRATCH = {}          # (device index, stream handle) -> persistent fp32 scratch for channel_sum's partial sums


def channel_sum(x, out, accumulate=False, st=None):
    """out[c] (+)= sum over pixels.  Large inputs reduce through 16 replicas of ``out`` in a scratch that belongs to the
    stream the call runs on (kept per stream: calls on one stream are ordered, calls on different streams never share it)."""
    c = x.shape[-1]
    st = st
    key = (x.device.index, st)
    ws = _CHSUM_SCRATCH.get(key)
    need = 16 * c
    if ws is None or ws.numel() < need:
        ws = _CHSUM_SCRATCH[key] = torch.empty(max(need, 16 * 2048), dtype=torch.float32, device=x.device)
    fn = ops.udaseg_channel_sum_bf16_ws if x.dtype == torch.bfloat16 else ops.udaseg_channel_sum_ws
    check(fn(x, x.numel() // c, c, out, int(accumulate), ws, ws.numel() * 4, st), "channel_sum")


def maxpool_fwd(x, st=None):
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, ho, wo, c), device=x.device, dtype=x.dtype)
    idx = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.uint8)
    if x.dtype == torch.bfloat16:
        check(ops.udaseg_maxpool3x3s2_fwd_bf16(x, y, idx, n, h, w, c,
                                                        st), "maxpool_fwd_bf16")
        return y, idx
    check(ops.udaseg_maxpool3x3s2_fwd(x, y, idx, n, h, w, c,
                                               st), "maxpool_fwd")
    return y, idx


def maxpool_bwd(dy, idx, dx, accumulate=False, st=None):
    n, h, w, c = dx.shape
    if dx.dtype == torch.bfloat16:
        check(ops.udaseg_maxpool3x3s2_bwd_bf16(dy, idx, dx, n, h, w, c, int(accumulate),
                                                        st), "maxpool_bwd_bf16")
        return
    check(ops.udaseg_maxpool3x3s2_bwd(dy, idx, dx, n, h, w, c, int(accumulate),
                                               st), "maxpool_bwd")


def upsample2x_concat_fwd(a, skip, st=None):
    n, h, w, ca = a.shape
    cb = 0 if skip is None else skip.shape[-1]
    out = torch.empty((n, 2 * h, 2 * w, ca + cb), device=a.device, dtype=a.dtype)
    if a.dtype == torch.bfloat16:      # pure data movement in 16-byte vectors: 8 bf16 channels == 4 fp32 "channels"
        ca, cb = ca // 2, cb // 2
    check(ops.udaseg_upsample2x_concat_fwd(a, skip, out, n, h, w, ca, cb,
                                                    st), "upsample2x_concat_fwd")
    return out


def upsample2x_concat_bwd(dout, da, dskip, ca, cb, accumulate_da=False, accumulate_dskip=False, st=None):
    n, h2, w2, _ = dout.shape
    if dout.dtype == torch.bfloat16:
        check(ops.udaseg_upsample2x_concat_bwd_bf16(dout, da, dskip, n, h2 // 2, w2 // 2, ca, cb,
                                                             int(accumulate_da), int(accumulate_dskip),
                                                             st), "upsample2x_concat_bwd_bf16")
        return
    check(ops.udaseg_upsample2x_concat_bwd(dout, da, dskip, n, h2 // 2, w2 // 2, ca, cb,
                                                    int(accumulate_da), int(accumulate_dskip),
                                                    st), "upsample2x_concat_bwd")


def upsample2x_bilinear_concat_fwd(a, skip, st=None):
    """cat(interpolate(a, scale_factor=2, mode='bilinear', align_corners=False), skip) on NHWC tensors (fp32 or bf16)."""
    n, h, w, ca = a.shape
    cb = 0 if skip is None else skip.shape[-1]
    out = torch.empty((n, 2 * h, 2 * w, ca + cb), device=a.device, dtype=a.dtype)
    check(ops.udaseg_upsample2x_bilinear_concat_fwd(a, skip, out, n, h, w, ca, cb,
                                                             int(a.dtype == torch.bfloat16), st),
          "upsample2x_bilinear_concat_fwd")
    return out


def upsample2x_bilinear_concat_bwd(dout, da, dskip, ca, cb, accumulate_da=False, accumulate_dskip=False, st=None):
    n, h2, w2, _ = dout.shape
    check(ops.udaseg_upsample2x_bilinear_concat_bwd(dout, da, dskip, n, h2 // 2, w2 // 2, ca, cb,
                                                             int(accumulate_da), int(accumulate_dskip),
                                                             int(dout.dtype == torch.bfloat16), st),
          "upsample2x_bilinear_concat_bwd")


def ce_fwd(logits_base, target, pixels, classes, ldc, lse, partials, loss, st=None):
    check(ops.udaseg_ce_fwd(logits_base, target, pixels, classes, ldc, lse,
                                     partials, loss, st), "ce_fwd")


def ce_bwd(logits_base, target, lse, grad_out, pixels, classes, ldc, dlogits, colsum_partials=None, colsum=None, st=None):
    check(ops.udaseg_ce_bwd(logits_base, target, lse, grad_out, pixels, classes,
                                     ldc, dlogits, colsum_partials, colsum,
                                     st), "ce_bwd")


def ce_fwd_bwd(logits_base, target, pixels, classes, ldc, partials, loss, dlogits, colsum_partials=None, colsum=None, st=None):
    """Loss and its gradient for an upstream gradient of 1 in ONE pass over the logits (ldc <= 32); both bit-identical to
    ``ce_fwd`` / ``ce_bwd``."""
    check(ops.udaseg_ce_fwd_bwd(logits_base, target, pixels, classes, ldc, partials, loss, dlogits, colsum_partials, colsum, st),
          "ce_fwd_bwd")


def scale_unless_one(x, g, x2=None, st=None):
    """x *= g (and x2 *= g) unless the device scalar ``g`` is exactly 1: then the launch returns at once."""
    check(ops.udaseg_scale_unless_one(x, x.numel(), x2, 0 if x2 is None else x2.numel(), g, st), "scale_unless_one")


def ce_target_stats(target, weight, pixels, classes, ignore_index, partials, denom, stats, st=None):
    """From the targets alone: denom = sum of weight[t] over valid pixels (f64), stats = [n_valid, n_void, n_invalid] (int64)."""
    check(ops.udaseg_ce_target_stats(target, weight, pixels, classes, *_ignore_args(ignore_index), partials, denom, stats, st),
          "ce_target_stats")


def ce_opt_fwd_bwd(logits_base, target, weight, pixels, classes, ldc, ignore_index, eps, mean, denom, partials, loss, dlogits,
                   colsum_partials=None, colsum=None, st=None):
    """Cross entropy with options, loss and (already scaled) gradient in ONE pass over the logits (ldc <= 32)."""
    check(ops.udaseg_ce_opt_fwd_bwd(logits_base, target, weight, pixels, classes, ldc, *_ignore_args(ignore_index), float(eps),
                                    int(mean), denom, partials, loss, dlogits, colsum_partials, colsum, st), "ce_opt_fwd_bwd")


def ce_opt_fwd(logits_base, target, weight, pixels, classes, ldc, ignore_index, eps, mean, denom, lse, partials, loss=None,
               loss_px=None, st=None):
    check(ops.udaseg_ce_opt_fwd(logits_base, target, weight, pixels, classes, ldc, *_ignore_args(ignore_index), float(eps), int(mean),
                                denom, lse, partials, loss, loss_px, st), "ce_opt_fwd")


def ce_opt_bwd(logits_base, target, weight, lse, grad_out, grad_px, pixels, classes, ldc, ignore_index, eps, mean, denom, dlogits,
               colsum_partials=None, colsum=None, st=None):
    check(ops.udaseg_ce_opt_bwd(logits_base, target, weight, lse, grad_out, grad_px, pixels, classes, ldc,
                                *_ignore_args(ignore_index), float(eps), int(mean), denom, dlogits, colsum_partials, colsum, st),
          "ce_opt_bwd")


KTH_BINS, KTH_STATE = 1024, 8            # bins per radix level, int64 words of the select's state (include/udaseg.h)


def ohem_conf(logits_base, target, pixels, classes, ldc, ignore_index, conf, hist0, counters, st=None):
    """conf = the target class's confidence per pixel (-1 at void / out-of-range / non-finite pixels), hist0 += its level-0 histogram,
    counters += [void, invalid, non-finite]."""
    check(ops.udaseg_ohem_conf(logits_base, target, pixels, classes, ldc, *_ignore_args(ignore_index), conf, hist0, counters, st),
          "ohem_conf")


def kth_hist(values, level, state, hist, st=None):
    check(ops.udaseg_kth_hist(values, values.numel(), level, state, hist, st), "kth_hist")


def kth_select(hist, level, state, min_kept=0, fraction=-1.0, st=None):
    check(ops.udaseg_kth_select(hist, level, int(min_kept), float(fraction), state, st), "kth_select")


def kth_value(state, thresh, out, st=None):
    """out = [q, max(q, thresh)] of a state after level 2."""
    check(ops.udaseg_kth_value(state, float(thresh), out, st), "kth_value")


def kth_refine(values, hist, state, st=None):
    """Levels 1 and 2 of the radix select, after level 0's select: ``hist`` int64 [3, 1024] (zeroed), ``state`` int64 [8]."""
    for level in (1, 2):
        kth_hist(values, level, state, hist[level], st)
        kth_select(hist[level], level, state, st=st)


def kth_smallest(values, k):
    """The exact k-th smallest (1-indexed) of a contiguous fp32 device buffer of values in [0, 2), as a device fp32 scalar: a
    three-level radix select (csrc/ohem.hip), no sort, nothing read back, the same bits on every call.  Values with the sign bit
    set or >= 2 (-1.0, inf, NaN) are skipped; with n values left, k == 0 gives -inf and k > n gives +inf (so that ``v <= result``
    selects exactly the ``min(k, n)`` smallest and every tie of the last one)."""
    if values.dtype != torch.float32 or values.numel() == 0:
        raise ValueError(f"kth_smallest: need a non-empty fp32 tensor, got {values.dtype} with {values.numel()} elements")
    if int(k) < 0:
        raise ValueError(f"kth_smallest: k must be >= 0, got {k}")
    flat = values.reshape(-1)
    ws = torch.zeros(3 * KTH_BINS + KTH_STATE, device=values.device, dtype=torch.int64)
    hist, state = ws[:3 * KTH_BINS].view(3, KTH_BINS), ws[3 * KTH_BINS:]
    kth_hist(flat, 0, None, hist[0])
    kth_select(hist[0], 0, state, min_kept=k)
    kth_refine(flat, hist, state)
    out = torch.empty(2, device=values.device, dtype=torch.float32)
    kth_value(state, 0.0, out)
    return out[0]


def ohem_denom(conf, target, weight, pixels, classes, thresh, state, partials, denom, counts, keep=None, st=None):
    """denom = sum of weight[t] over the kept pixels (f64), counts = [valid finite, kept], keep = the optional uint8 map."""
    check(ops.udaseg_ohem_denom(conf, target, weight, pixels, classes, float(thresh), state, partials, denom, counts, keep, st),
          "ohem_denom")


def ce_ohem_fwd_bwd(logits_base, target, weight, conf, state, thresh, pixels, classes, ldc, mean, denom, partials, loss, dlogits=None,
                    colsum_partials=None, colsum=None, st=None):
    """Cross entropy over the kept pixels, loss and (already scaled) gradient in ONE pass over the logits; dlogits None: loss only."""
    check(ops.udaseg_ce_ohem_fwd_bwd(logits_base, target, weight, conf, state, float(thresh), pixels, classes, ldc, int(mean), denom,
                                     partials, loss, dlogits, colsum_partials, colsum, st), "ce_ohem_fwd_bwd")


def lovasz_hist(logits_base, target, pixels, classes, ldc, ignore_index, images, bins, tables, counters, st=None):
    """tables (int32 [images, classes, 2, bins], zeroed) += the fg / bg error histograms of the Lovasz-softmax loss,
    counters (int64 [4], zeroed) += [valid finite, void, invalid, non-finite] pixels."""
    check(ops.udaseg_lovasz_hist(logits_base, target, pixels, classes, ldc, *_ignore_args(ignore_index), images, bins, tables,
                                 counters, st), "lovasz_hist")


def lovasz_table(tables, images, classes, bins, all_classes, coef, present, slack_parts, slack, st=None):
    """tables -> coef (fp32, the tables' shape; the reduction factor folded in), present (int32 [images, classes]) and
    slack (f64 [classes], the bound on what the grid costs); slack_parts: f64 [images * classes] scratch."""
    check(ops.udaseg_lovasz_table(tables, images, classes, bins, int(all_classes), coef, present, slack_parts, slack, st),
          "lovasz_table")


def lovasz_fwd_bwd(logits_base, target, coef, counters, pixels, classes, ldc, ignore_index, images, bins, ce_weight, partials, loss,
                   dlogits=None, colsum_partials=None, colsum=None, st=None):
    """Lovasz-softmax loss (+ ce_weight * cross entropy) and its gradient in ONE pass over the logits; dlogits None: loss only."""
    check(ops.udaseg_lovasz_fwd_bwd(logits_base, target, coef, counters, pixels, classes, ldc, *_ignore_args(ignore_index), images,
                                    bins, float(ce_weight), partials, loss, dlogits, colsum_partials, colsum, st), "lovasz_fwd_bwd")


def seg_partials():
    return ops.udaseg_seg_partials()


def dice_fwd(logits_base, target, batch, pix_per_image, classes, ldc, smooth, sums, coef, loss, eps=1e-7, pooled=False, st=None,
             ignore_index=None):
    if ignore_index is not None:
        check(ops.udaseg_dice_fwd_ignore(logits_base, target, batch, pix_per_image, classes, ldc, float(smooth), float(eps),
                                         int(pooled), sums, coef, loss, int(ignore_index), st), "dice_fwd_ignore")
        return
    check(ops.udaseg_dice_fwd(logits_base, target, batch, pix_per_image, classes, ldc,
                                       float(smooth), float(eps), int(pooled), sums, coef,
                                       loss, st), "dice_fwd")


def dice_bwd(logits_base, target, coef, grad_out, weight, batch, pix_per_image, classes, ldc, dlogits, accumulate=False,
             st=None, ignore_index=None):
    if ignore_index is not None:
        check(ops.udaseg_dice_bwd_ignore(logits_base, target, coef, grad_out, float(weight), batch, pix_per_image, classes, ldc,
                                         dlogits, int(accumulate), int(ignore_index), st), "dice_bwd_ignore")
        return
    check(ops.udaseg_dice_bwd(logits_base, target, coef, grad_out,
                                       float(weight), batch, pix_per_image, classes, ldc, dlogits,
                                       int(accumulate), st), "dice_bwd")


def focal_fwd(logits_base, target, class_weights, alpha, gamma, pixels, classes, ldc, mean, partials, loss, accumulate=False,
              st=None, ignore_index=None):
    if ignore_index is not None:
        check(ops.udaseg_focal_fwd_ignore(logits_base, target, class_weights, float(alpha), float(gamma), pixels, classes, ldc,
                                          int(mean), partials, loss, int(accumulate), int(ignore_index), st), "focal_fwd_ignore")
        return
    check(ops.udaseg_focal_fwd(logits_base, target, class_weights, float(alpha),
                                        float(gamma), pixels, classes, ldc, int(mean), partials, loss,
                                        int(accumulate), st), "focal_fwd")


def focal_bwd(logits_base, target, class_weights, alpha, gamma, grad_out, weight, pixels, classes, ldc, dlogits,
              accumulate=False, st=None, ignore_index=None):
    if ignore_index is not None:
        check(ops.udaseg_focal_bwd_ignore(logits_base, target, class_weights, float(alpha), float(gamma), grad_out, float(weight),
                                          pixels, classes, ldc, dlogits, int(accumulate), int(ignore_index), st), "focal_bwd_ignore")
        return
    check(ops.udaseg_focal_bwd(logits_base, target, class_weights, float(alpha),
                                        float(gamma), grad_out, float(weight), pixels, classes, ldc,
                                        dlogits, int(accumulate), st), "focal_bwd")


def consistency_fwd(z1, z2, temperature, batch, pixels, classes, ldc, partials, loss, st=None):
    check(ops.udaseg_consistency_fwd(z1, z2, float(temperature), batch, pixels, classes, ldc,
                                              partials, loss, st),
          "consistency_fwd")


def consistency_bwd(z1, z2, temperature, grad_out, weight, batch, pixels, classes, ldc, d1, d2, accumulate=False, st=None):
    check(ops.udaseg_consistency_bwd(z1, z2, float(temperature), grad_out, float(weight),
                                              batch, pixels, classes, ldc, d1, d2, int(accumulate),
                                              st), "consistency_bwd")


def selfinfo_fwd(logits_base, pixels, classes, ldc, maps, cpad, entropy=None, st=None):
    """maps [pixels * cpad] fp32 or bf16 = the weighted self-information -p log p / log C of softmax(logits), zeros in the pad
    lanes; entropy [pixels] fp32 or None = its sum over the classes."""
    check(ops.udaseg_selfinfo_fwd(logits_base, pixels, classes, ldc, maps, cpad, int(maps.dtype == torch.bfloat16), entropy, st),
          "selfinfo_fwd")


def selfinfo_bwd(logits_base, dmaps, pixels, classes, ldc, cpad, dlogits, st=None):
    """dlogits [pixels * ldc] fp32 = the gradient of the logits from dmaps [pixels * cpad] (fp32 or bf16), the maps' gradient."""
    check(ops.udaseg_selfinfo_bwd(logits_base, dmaps, pixels, classes, ldc, cpad, int(dmaps.dtype == torch.bfloat16), dlogits, st),
          "selfinfo_bwd")


ENTROPY_KINDS = {"entropy": 0, "max_squares": 1}


def entropy_loss(logits_base, pixels, classes, ldc, kind, partials, loss, dlogits=None, entropy=None, st=None):
    """loss = mean normalised entropy (kind 'entropy') or -mean sum p^2 / 2 ('max_squares') of softmax(logits); dlogits (optional) its
    gradient for an upstream gradient of 1, made in the same pass; entropy (optional) [pixels] the per-pixel normalised entropy."""
    check(ops.udaseg_entropy_loss(logits_base, pixels, classes, ldc, ENTROPY_KINDS[kind], partials, loss, dlogits, entropy, st),
          "entropy_loss")


SOFT_CE_KINDS = {"ce": 0, "kl": 1, "symmetric": 2}


def soft_ce_fwd_bwd(logits_base, teacher_base, weight_px, weight_img, batch, pix_per_image, classes, ldc, ldt, probs, kind,
                    teacher_inv_temp, alpha, beta, log_floor, mean, denom, partials, loss, dlogits=None, colsum_partials=None,
                    colsum=None, stats=None, st=None):
    """loss = the weighted soft cross entropy ('ce'), KL(teacher || student) ('kl') or symmetric cross entropy ('symmetric') of the
    student logits [pixels * ldc] against the teacher's logits or probabilities [pixels * ldt]; dlogits / colsum (optional) the
    gradient for an upstream gradient of 1 and its per-class sums, made in the same pass; stats (optional) int64 [3], accumulated.
    include/udaseg.h has the arithmetic and the void rule."""
    check(ops.udaseg_soft_ce_fwd_bwd(logits_base, teacher_base, weight_px, weight_img, batch, pix_per_image, classes, ldc, ldt,
                                     int(bool(probs)), SOFT_CE_KINDS[kind], float(teacher_inv_temp), float(alpha), float(beta),
                                     float(log_floor), int(bool(mean)), denom, partials, loss, dlogits, colsum_partials, colsum,
                                     stats, st), "soft_ce_fwd_bwd")


def pixel_weight_sum(weight_px, weight_img, batch, pix_per_image, partials, denom, counts, st=None):
    """denom [1] f64 = the sum of weight_px[p] * weight_img[image of p] over the pixels whose weight is positive and finite;
    counts int64 [2] = zero weights, negative or non-finite weights."""
    check(ops.udaseg_pixel_weight_sum(weight_px, weight_img, batch, pix_per_image, partials, denom, counts, st), "pixel_weight_sum")


def conf_share(scores_base, batch, pix_per_image, classes, ldc, probs, tau, above, nonfinite, share, st=None):
    """Per image: above = pixels whose winner confidence (conf_hist's) is >= tau, nonfinite = its non-finite pixels,
    share = above / pix_per_image (fp32)."""
    check(ops.udaseg_conf_share(scores_base, batch, pix_per_image, classes, ldc, int(bool(probs)), float(tau), above, nonfinite,
                                share, st), "conf_share")


def gap_linear_sigmoid_fwd(z, w, b, st=None):
    n, h, wd, c = z.shape
    hw = h * wd
    splits = ops.udaseg_gap_splits(hw)
    partial = torch.empty((n, splits, c), device=z.device, dtype=torch.float32)
    pooled = torch.empty((n, c), device=z.device, dtype=torch.float32)
    p = torch.empty((n, 1), device=z.device, dtype=torch.float32)
    if z.dtype == torch.bfloat16:
        sv = st
        check(ops.udaseg_gap_partial_bf16(z, partial, n, hw, c, sv), "gap_partial_bf16")
        check(ops.udaseg_gap_finish(partial, w, b, pooled, p, n, hw,
                                             c, sv), "gap_finish")
        return p, pooled
    check(ops.udaseg_gap_linear_sigmoid_fwd(z, w, b, partial,
                                                     pooled, p, n, hw, c,
                                                     st), "gap_linear_sigmoid_fwd")
    return p, pooled


def gap_linear_sigmoid_bwd(dp, p, pooled, w, dz, dw, db, accumulate_param=False, st=None):
    n, h, wd, c = dz.shape
    if dz.dtype == torch.bfloat16:
        sv = st
        check(ops.udaseg_gap_bwd_broadcast_bf16(dp, p, w, dz, n, h * wd, c, sv),
              "gap_bwd_broadcast_bf16")
        check(ops.udaseg_gap_bwd_param(dp, p, pooled, dw, db, n, c,
                                                int(accumulate_param), sv), "gap_bwd_param")
        return
    check(ops.udaseg_gap_linear_sigmoid_bwd(dp, p, pooled, w, dz,
                                                     dw, db, n, h * wd, c, int(accumulate_param),
                                                     st), "gap_linear_sigmoid_bwd")


def bce_logits_fwd(x, label, weight, loss, accumulate=False, st=None):
    check(ops.udaseg_bce_logits_fwd(x, x.numel(), label, weight, loss, int(accumulate),
                                             st), "bce_logits_fwd")


def bce_logits_bwd(x, label, weight, grad_out, dx, accumulate=False, st=None):
    check(ops.udaseg_bce_logits_bwd(x, x.numel(), label, weight, grad_out, dx,
                                             int(accumulate), st), "bce_logits_bwd")


def gap_linear_fwd(z, w, b, st=None):
    """logit[n] = dot(mean over pixels of z[n], w) + b for NHWC z; returns (logit [n], pooled [n, c])."""
    n, h, wd, c = z.shape
    hw = h * wd
    splits = ops.udaseg_gap_splits(hw)
    partial = torch.empty((n, splits, c), device=z.device, dtype=torch.float32)
    pooled = torch.empty((n, c), device=z.device, dtype=torch.float32)
    logit = torch.empty(n, device=z.device, dtype=torch.float32)
    check(ops.udaseg_gap_linear_fwd(z, w, b, partial, pooled,
                                             logit, n, hw, c, st), "gap_linear_fwd")
    return logit, pooled


def gap_linear_bwd(dlogit, pooled, w, dz, dw, db, accumulate_param=False, st=None):
    n, h, wd, c = dz.shape
    check(ops.udaseg_gap_linear_bwd(dlogit, pooled, w, dz, dw,
                                             db, n, h * wd, c, int(accumulate_param),
                                             st), "gap_linear_bwd")


def bce_logits_target_fwd(x, target, weight, loss, accumulate=False, st=None):
    check(ops.udaseg_bce_logits_target_fwd(x, target, x.numel(), float(weight), loss,
                                                    int(accumulate), st), "bce_logits_target_fwd")


def bce_logits_target_bwd(x, target, weight, grad_out, dx, accumulate=False, st=None):
    check(ops.udaseg_bce_logits_target_bwd(x, target, x.numel(), float(weight), grad_out,
                                                    dx, int(accumulate), st),
          "bce_logits_target_bwd")


def _storage_order(t, who):
    """A flat view of ``t`` in the order of its storage: ``t`` itself when contiguous, the underlying run of elements when ``t`` is a
    dense permutation (an [N,C,H,W]-shaped view of an NHWC buffer) -- an element-wise kernel does not care about the order."""
    if t.is_contiguous():
        return t
    st = sorted(zip(t.stride(), t.shape), reverse=True)
    run = 1
    for stride, size in reversed(st):
        if size != 1 and stride != run:
            raise ValueError(f"{who}: tensor must be dense (contiguous or a permutation of a contiguous tensor), strides {t.stride()}")
        run *= size
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


def scale(x, alpha, out=None, st=None):
    """out = alpha * x (fp32; x dense in any dimension order, out with the same strides)."""
    out = torch.empty_like(x) if out is None else out
    if out.stride() != x.stride() or out.shape != x.shape:
        raise ValueError("scale: out must have x's shape and strides")
    check(ops.udaseg_scale_f32(_storage_order(x, "scale"), _storage_order(out, "scale"), x.numel(), float(alpha), st), "scale_f32")
    return out


def adam_flat(p, g, m, v, count, lr, beta1, beta2, eps, bc1, bc2, st=None):
    check(ops.udaseg_adam_flat(p, g, m, v, count, lr, beta1, beta2, eps,
                                        bc1, bc2, st), "adam_flat")


def ema_flat(t, s, count, decay, partials=None, dist2=None, accumulate=False, st=None):
    """t <- t + (1 - decay) * (s - t) over ``count`` fp32 elements (include/udaseg.h: decay 0 copies, 1 keeps; fused multiply-add);
    with ``dist2`` (0-dim fp64, and the 257-double ``partials`` scratch of ``sumsq_f32``) also the squared distance |s - t_new|^2."""
    check(ops.udaseg_ema_flat(t, s, count, float(decay), partials, dist2, int(accumulate), st), "ema_flat")


def fill(t, value, st=None):
    check(ops.udaseg_fill_f32(t, t.numel(), value, st), "fill_f32")


def axpy(y, x, alpha=1.0, st=None):
    check(ops.udaseg_axpy_f32(y, x, y.numel(), alpha, st),
          "axpy_f32")


def set_option(name, value):
    """Override one switch of the library's switchboard (``_lib.OPTIONS``: name -> UDASEG_OPT_* key; the environment variable of the
    same name is only its default); value -1 restores the default.  Every override bumps ``option_epoch()``."""
    key = _lib.OPTIONS[name] if isinstance(name, str) else int(name)
    check(ops.udaseg_set_option(key, int(value)), f"set_option({name})")


def get_option(name):
    key = _lib.OPTIONS[name] if isinstance(name, str) else int(name)
    return int(ops.udaseg_get_option(key))


def option_epoch():
    """Number of overrides made so far: the plans key their cached routing answers with it (engine.Plan)."""
    return int(ops.udaseg_option_epoch())


def set_generic_gather(value):
    """1: convolution kernels keep their generic gather loops; 0: uniform-tap / row-uniform loops allowed; -1: environment."""
    set_option("GENERIC_GATHER", value)


def set_f32_split(value):
    """0: the shared-source fp32 kernels stay on the fp32 matrix pipe; 1: three-term bf16 split allowed; -1: environment."""
    set_option("F32_SPLIT", value)


def prof_enable(on):
    check(ops.udaseg_prof_enable(int(on)))


def prof_reset():
    check(ops.udaseg_prof_reset())


def prof_read(family):
    ms, fl, n = _lib.C.c_double(), _lib.C.c_double(), _lib.C.c_int64()
    check(ops.udaseg_prof_read(family, _byref(ms), _byref(fl), _byref(n)), "prof_read")
    return ms.value, fl.value, n.value


def prof_records(family, max_records=4096):
    """[(ms, flops, kind, (n,hi,wi,ci,ho,wo,co,kh,kw,stride,pad))] of the recorded launches of one kernel family."""
    C = _lib.C
    ms, fl = (C.c_double * max_records)(), (C.c_double * max_records)()
    kind, desc = (C.c_int * max_records)(), (C.c_int * (11 * max_records))()
    n = ops.udaseg_prof_records(family, max_records, ms, fl, kind, desc)
    if n < 0:
        check(n, "prof_records")
    return [(ms[i], fl[i], kind[i], tuple(desc[11 * i:11 * i + 11])) for i in range(n)]


def prof_kernels():
    """[(kernel symbol, total ms, total flops, launches)] for every conv kernel instantiation."""
    lib = _lib.load()
    out = []
    for kid in range(lib.udaseg_prof_kernel_count()):
        ms, fl, n = _lib.C.c_double(), _lib.C.c_double(), _lib.C.c_int64()
        check(lib.udaseg_prof_kernel_read(kid, _byref(ms), _byref(fl), _byref(n)), "prof_kernel_read")
        out.append((lib.udaseg_prof_kernel_name(kid).decode(), ms.value, fl.value, n.value))
    return out


# ---- prediction (predict.py; csrc/predict.hip).  grid = (h, w, th, tw, rows, cols, sy, sx) of predict.plan_grid
def predict_gather_u8(image, grid, first, tiles, views, mean255, inv_std255, out, st=None):
    """uint8 [h,w,3] frame -> out [tiles*V, th, tw, cpad] model input (fp32 or bf16 by out's dtype)."""
    check(ops.udaseg_predict_gather_u8(image, *grid, first, tiles, views, mean255, inv_std255, out, out.shape[-1],
                                       int(out.dtype == torch.bfloat16), st), "predict_gather_u8")


def predict_blend(logits, ldc, grid, first, tiles, views, classes, win_y, win_x, acc, ldp, wsum, st=None):
    check(ops.udaseg_predict_blend(logits, ldc, *grid, first, tiles, views, classes, win_y, win_x, acc, ldp, wsum, st),
          "predict_blend")


def predict_finish(probs, wsum, pixels, classes, ldc, labels, st=None):
    check(ops.udaseg_predict_finish(probs, wsum, pixels, classes, ldc, labels, st), "predict_finish")


def predict_threshold(logits, n, hw, classes, ldc, out, st=None):
    check(ops.udaseg_predict_threshold(logits, n, hw, classes, ldc, out, st), "predict_threshold")


# ---- frame ingest (ingest.py; csrc/resize.hip).  Sizes are (height, width)
def resize_area_u8(src, dst, st=None):
    """uint8 [n,H,W,3] -> uint8 [n,h,w,3] (dst's size), exact area filter; shrinking only."""
    n, H, W, _ = src.shape
    check(ops.udaseg_resize_area_u8(src, n, H, W, dst.shape[1], dst.shape[2], dst, st), "resize_area_u8")


def resize_nearest_u8(src, dst, st=None):
    """uint8 [n,H,W] -> uint8 [n,h,w] (dst's size), dst[i][j] = src[(i*H)//h][(j*W)//w]."""
    n, H, W = src.shape
    check(ops.udaseg_resize_nearest_u8(src, n, H, W, dst.shape[1], dst.shape[2], dst, st), "resize_nearest_u8")


def mask_hist_u8(masks, hist, st=None):
    """uint8 [n, ...] masks -> hist int64 [n,256] += per-mask counts of every byte value (accumulates)."""
    n = masks.shape[0]
    check(ops.udaseg_mask_hist_u8(masks, n, masks.numel() // n, hist, st), "mask_hist_u8")


def resize_aa_u8(src, y_table, x_table, mean255, inv_std255, out, st=None):
    """uint8 [n,H,W,3] -> out [n,h,w,cpad] (fp32 or bf16 by out's dtype): antialiased bilinear + A.Normalize.  A table is
    (start int32 [l], weights fp32 [l,taps]) on the device."""
    n, H, W, _ = src.shape
    (ys, yw), (xs, xw) = y_table, x_table
    check(ops.udaseg_resize_aa_u8(src, n, H, W, out.shape[1], out.shape[2], ys, yw, yw.shape[1], xs, xw, xw.shape[1], mean255,
                                  inv_std255, out, out.shape[-1], int(out.dtype == torch.bfloat16), st), "resize_aa_u8")
