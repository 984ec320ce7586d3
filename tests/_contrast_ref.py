"""numpy restatement of the prototype contrast kernels (csrc/proto_contrast.hip: udaseg_proto_assign,
udaseg_proto_contrast_fwd_bwd), in the manner of ``_distill_ref``, whose weights, ``embed`` and ``Grader`` it reuses.

Per pixel, with P the prototypes rounded to fp32 (what the kernel stages; BOTH legs start from them), over the SEEN classes:

    d_c = sum_j (f_j - P_cj)^2,  d* = min d_c,  a_c = -(d_c - d*) inv_tau,  L = log sum exp(a_c),  s_c = exp(a_c - L)   (assign)
    hard: t_c = [c == label];   soft: t_c = target_c for a seen class, 0 for an unseen one;   T = sum_c t_c
    l = sum_c t_c (-a_c) + T L                       dl/df_j = 2 inv_tau sum_c (T s_c - t_c) P_cj

An unseen class is in no sum and gets s_c = 0.  w_p = weight_px[p] * weight_img[p // pix_per_image] is the fp32 product in both
legs.  A pixel is void -- loss 0, gradient 0, magnitude 0, so only 0 passes -- for the FIRST of: its weight is 0, negative or not
finite (stats[1]); its label is beyond the classes or names an unseen class / a target lane is not finite or outside [0, 1] or
T == 0 (stats[2]); a feature is not finite (stats[3]).  While no class is seen every pixel is void by 1 or 2; while inv_tau is
not positive the pixels are counted as usual and loss and gradient are 0.  loss = sum_p w_p l_p / D, D = pixels ('mean'), 1
('sum') or the sum of the w_p that do not void their pixel ('weighted_mean'; D == 0 gives NaN); the gradient carries w_p / D.

``elem`` = ``np.float64`` is the reference (tests/test_contrast_host.py proves it against torch's double-precision autograd),
``np.float32`` follows the kernel's order of operations -- the distances in four chains of fused multiply-adds (a product of two
fp32 numbers is exact in float64, so rounding product + sum once from float64 IS the fused operation up to a double rounding),
S and T in four chains, the gradient one chain of fused multiply-adds over ascending c -- and is the leg the bar is measured from.

MAGNITUDES, made of the inputs only (the float64 distances are a function of the inputs, not of the code under test):
    loss of a pixel       w T ((dmax - d*) inv_tau + log C)      dmax: the largest seen distance, C: the number of classes
    gradient, channel j   2 inv_tau (w / D) T max_seen |P_cj|
    loss scalar           the sum of the pixels' magnitudes / D
    assignment s_c        s_c (1 + (d_c - d*) inv_tau + |L|) + UNDERFLOW    (``_distill_ref``'s rule for a probability exp(lp): it
                          inherits the absolute error of its exponent a_c - L as a relative error)
The rounding of the distances themselves (relative to d, which for a feature far from every prototype is much larger than
dmax - d*) is in no magnitude: the float32 leg carries it, and the bar is 4 x that leg's worst deviation.

``mut`` names one deliberate mistake (MUTATIONS); tests/test_contrast_host.py shows that the grading catches each.
"""
import numpy as np

from _distill_ref import REDUCTIONS, ceil_to, embed, pixel_weights  # noqa: F401
from _loss_ref import F32, F64, PAD_JUNK, UNDERFLOW, Grader, bar, f32, normalised  # noqa: F401

FORMS = ("hard", "soft")
MUTATIONS = ("f_terms_kept", "T_is_1", "unseen_in_sum", "grad_not_divided", "pad_lanes", "void_grad")
BLOCKS, THREADS = 1024, 256                # udaseg_seg_partials() blocks of 256 pixels: beyond them a lane takes a second pixel
CHUNK = 1 << 14                            # rows per [rows, C, D] broadcast of the restatement


def _fma(a, b, c, elem):
    if elem is F64:
        return a * b + c
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _chains4(x, elem):
    """Sum over axis 1: column c into chain c % 4, folded as (s0 + s1) + (s2 + s3)."""
    if elem is F64:
        return x.sum(1)
    ch = [np.zeros(x.shape[0], dtype=elem) for _ in range(4)]
    for c in range(x.shape[1]):
        ch[c % 4] = (ch[c % 4] + x[:, c]).astype(elem)
    return ((ch[0] + ch[1]).astype(elem) + (ch[2] + ch[3]).astype(elem)).astype(elem)


def _seq(x, elem):
    return np.cumsum(x, axis=1, dtype=elem)[:, -1]


def distances(f, pr, elem):
    """d [rows, C]: float64 plainly; float32 as the kernel: channel j into chain j % 4 by fused multiply-adds, (s0 + s1) + (s2 + s3)."""
    t = (f[:, None, :] - pr[None, :, :]).astype(elem)
    if elem is F64:
        return (t * t).sum(2)
    ch = np.zeros(t.shape[:2] + (4,), dtype=F32)
    for q in range(t.shape[2] // 4):
        tq = t[:, :, 4 * q:4 * q + 4]
        ch = _fma(tq, tq, ch, elem)
    return ((ch[..., 0] + ch[..., 1]).astype(F32) + (ch[..., 2] + ch[..., 3]).astype(F32)).astype(F32)


def _assignment(f, pr, sum_over, it, elem):
    """(d, dmin, a, L, s) over the classes of ``sum_over`` (a bool [C], not empty); a = 0 and s = 0 in the other columns."""
    d = distances(f.astype(elem), pr.astype(elem), elem)
    dmin = d[:, sum_over].min(1, keepdims=True)
    a = np.where(sum_over[None, :], (-(d - dmin).astype(elem) * elem(it)).astype(elem), elem(0))
    e = np.where(sum_over[None, :], np.exp(a).astype(elem), elem(0))
    L = np.log(_chains4(e, elem)).astype(elem)
    s = np.where(sum_over[None, :], np.exp((a - L[:, None]).astype(elem)).astype(elem), elem(0))
    return d, dmin, a, L, s


def _rounded(proto):
    return np.asarray(proto, dtype=F64).astype(F32)


def assign(f, proto, seen, inv_tau, elem=F64):
    """(s [pixels, C], magnitude): NaN rows where a feature is not finite; 1 / C everywhere while no class is seen."""
    f = np.asarray(f, dtype=F32)
    pr, seen = _rounded(proto), np.asarray(seen).astype(bool)
    pixels, C = f.shape[0], pr.shape[0]
    out, mag = np.zeros((pixels, C), dtype=elem), np.zeros((pixels, C), dtype=F64)
    fin = np.isfinite(f).all(1)
    if not seen.any():
        out[:] = elem(1) / elem(C)
        mag[:] = 1.0 / C
    else:
        live = np.nonzero(fin)[0]
        for lo in range(0, len(live), CHUNK):
            rows = live[lo:lo + CHUNK]
            with np.errstate(under="ignore"):
                d, dmin, a, L, s = _assignment(f[rows], pr, seen, inv_tau, elem)
            out[rows] = s
            if elem is F64:
                mag[rows] = s * (1.0 + np.where(seen[None, :], (d - dmin) * float(inv_tau), 0.0) + np.abs(L)[:, None]) + UNDERFLOW * seen[None, :]
    out[~fin] = np.nan
    return out, mag


def classify(f, labels, target, wpx, wimg, batch, ppi, seen, mut=None):
    """(w fp32, why, t fp32 [pixels, C]): decided on the fp32 numbers the kernel tests, for both legs.  t is the target with the
    mass on unseen classes dropped (0 rows where the pixel is void)."""
    seen = np.asarray(seen).astype(bool)
    C = len(seen)
    w, why_w = pixel_weights(wpx, wimg, batch, ppi)
    pixels = len(w)
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64)
        inr = lab < C
        t = np.zeros((pixels, C), dtype=F32)
        t[np.nonzero(inr)[0], lab[inr]] = 1
        bad = ~(inr & seen[np.where(inr, lab, 0)])
    else:
        t = np.asarray(target, dtype=F32)
        with np.errstate(invalid="ignore"):
            bad = ~((t >= 0) & (t <= 1)).all(1)
        t = np.where(seen[None, :] & ~bad[:, None], t, F32(0))
        bad |= _chains4(t, F32) == 0
    t = np.where(bad[:, None], F32(0), t)
    fin = np.isfinite(np.asarray(f, dtype=F32)).all(1)
    why = np.where(why_w != 0, 1, np.where(bad, 2, np.where(~fin, 3, 0)))
    return w, why, t


def contrast(f, labels, target, proto, seen, inv_tau, wpx, wimg, batch, ppi, reduction, elem=F64, mut=None):
    """name -> (value, magnitude) for loss and grad [pixels, dim]; plus "stats" (int64 [4]) and "why" [pixels].  Exactly one of
    ``labels`` (uint8 [pixels]) and ``target`` (fp32 [pixels, C])."""
    assert (labels is None) != (target is None)
    f = np.asarray(f, dtype=F32)
    pr, seen = _rounded(proto), np.asarray(seen).astype(bool)
    pixels, dim = f.shape
    C = pr.shape[0]
    assert pixels == batch * ppi
    w, why, t_all = classify(f, labels, target, wpx, wimg, batch, ppi, seen, mut)
    stats = np.array([(why == k).sum() for k in range(4)], dtype=np.int64)
    it = F32(inv_tau)
    if reduction == "mean":
        div, scale = float(pixels), elem(1) / elem(pixels)
    elif reduction == "sum":
        div, scale = 1.0, elem(1)
    else:
        w_only, why_w = pixel_weights(wpx, wimg, batch, ppi)
        div = float(w_only[why_w == 0].astype(F64).sum())
        with np.errstate(divide="ignore"):
            scale = elem(F64(1.0) / F64(div))
    grad = np.zeros((pixels, dim), dtype=elem)
    mag_grad = np.zeros((pixels, dim), dtype=F64)
    total, mag_total = 0.0, 0.0
    live = np.nonzero(why == 0)[0] if (it > 0 and seen.any()) else np.zeros(0, dtype=np.int64)
    sum_over = np.ones(C, dtype=bool) if mut == "unseen_in_sum" else seen
    pe = pr.astype(elem)
    pmax = np.abs(pr[seen].astype(F64)).max(0) if seen.any() else np.zeros(dim)
    for lo in range(0, len(live), CHUNK):
        rows = live[lo:lo + CHUNK]
        with np.errstate(under="ignore"):
            d, dmin, a, L, s = _assignment(f[rows], pr, sum_over, it, elem)
        t = t_all[rows].astype(elem)
        wl = w[rows].astype(elem)
        T = _chains4(t, elem)
        if labels is not None:
            l = (np.where(t > 0, -a, elem(0)).sum(1).astype(elem) + L).astype(elem)            # one term: (d_y - d*) inv_tau
        else:
            fwd = _seq(np.where(t > 0, (t * -a).astype(elem), elem(0)).astype(elem), elem)
            l = (fwd + (T * L).astype(elem)).astype(elem)
        Tk = np.ones_like(T) if (mut == "T_is_1" and labels is None) else T
        k = ((Tk[:, None] * s).astype(elem) - t).astype(elem)
        g = np.zeros((len(rows), dim), dtype=elem)
        for c in range(C):
            if mut == "f_terms_kept":
                g = _fma(k[:, c:c + 1], (pe[c][None, :] - f[rows].astype(elem)).astype(elem), g, elem)
            else:
                g = _fma(k[:, c:c + 1], np.broadcast_to(pe[c][None, :], g.shape), g, elem)
        cw = (scale * wl).astype(elem) if mut != "grad_not_divided" else wl
        coef = ((elem(2) * elem(it)) * cw).astype(elem)
        grad[rows] = (coef[:, None] * g).astype(elem)
        total += float((wl * l).astype(elem).astype(F64).sum())
        if elem is F64:
            mag_l = wl * T * ((d[:, seen].max(1) - dmin[:, 0]) * float(it) + np.log(C))
            mag_total += float(mag_l.sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                mag_grad[rows] = (2.0 * float(it) * wl * T / div)[:, None] * pmax[None, :] if div else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = elem(F64(total) / F64(div))
        mag_loss = mag_total / div if div else 0.0
    if mut == "void_grad":
        grad[why == 2] = elem(scale) * elem(0.25)
    return {"loss": (loss, mag_loss), "grad": (grad, mag_grad), "stats": stats, "why": why}


# ------------------------------------------------------------------------------------------------------------ cases and grading
CLASSES = (2, 5, 23, 32)
DIMS = (4, 16, 64)
SHAPES = ((1, 1), (3, 85), (1, 257))       # batch x pix_per_image: one pixel; image boundaries inside a wave; a second block
BIG = (1, BLOCKS * THREADS + 3)            # three lanes take a second grid-stride pixel
ROW_KINDS = ("random", "on_proto", "far", "label_255", "label_unseen", "soft_unseen_only", "target_1p5", "nan_target", "nan_feature",
             "w_zero", "w_negative", "w_nan", "img_zero")
COMBOS = tuple((form, r) for form in FORMS for r in REDUCTIONS)
COVER = (("hard", "mean"), ("soft", "weighted_mean"), ("soft", "sum"))        # both forms, every reduction
INV_TAU = f32(1.0 / 2.5)


def unseen_class(classes):
    """The class the graded banks have not seen: the last one; none at two classes (a softmax over one class is constant)."""
    return classes - 1 if classes >= 3 else None


def make_case(batch, ppi, classes, dim, seed, row_kind=None):
    """features [pixels, dim] fp32, labels uint8 [pixels], target fp32 [pixels, classes], weight_px [pixels], weight_img [batch],
    proto float64 [classes, dim], seen int32 [classes].  Prototypes: normal at scale 2 (not fp32 numbers: the rounding is part of
    the contract); features: the label's prototype plus unit normal noise, the prototypes' own scatter (inv_tau = 1 / 2.5).
    Rows i mod 14 = 1.. are the special kinds of ROW_KINDS[1:] in order; ``row_kind`` makes every row of that kind.
    on_proto: the feature IS the fp32 prototype of its label (d = 0).  far: 1e3 along a unit direction from it (every distance
    about 1e6, the assignment saturated).  label_255 / label_unseen: void in the hard form (at two classes, where every class is
    seen, label_unseen is the label 2).  soft_unseen_only: all the mass on the unseen class (all-zero at two classes): T == 0.
    target_1p5: one lane 1.5.  nan_target: the whole row NaN (what rectify and assign write) on even rows, one lane on odd.
    nan_feature: one channel NaN on even rows, +inf on odd.  w_zero / w_negative / w_nan: weight_px 0, -0.5, NaN.  img_zero:
    image 1's weight_img is 0 (all of them for the single-row case).  In the mixed case every other w_zero, label_255 and
    target_1p5 row also has a NaN feature: the first cause must decide."""
    rng = np.random.default_rng(seed)
    pixels = batch * ppi
    proto = 2.0 * rng.standard_normal((classes, dim))
    seen = np.ones(classes, dtype=np.int32)
    un = unseen_class(classes)
    nseen = classes
    if un is not None:
        seen[un] = 0
        nseen = classes - 1
    p32 = proto.astype(F32)
    labels = rng.integers(0, nseen, pixels).astype(np.uint8)
    f = (p32[labels] + rng.standard_normal((pixels, dim))).astype(F32)
    e = np.exp(2.0 * rng.standard_normal((pixels, classes)))
    target = np.minimum((e / e.sum(1, keepdims=True)).astype(F32), F32(1))
    r = np.arange(pixels)
    lane = rng.integers(0, classes, pixels)
    pick = {k: ((r % 14 == i + 1) if row_kind is None else np.full(pixels, row_kind == k)) for i, k in enumerate(ROW_KINDS[1:])}
    f[pick["on_proto"]] = p32[labels[pick["on_proto"]]]
    rows = pick["far"]
    u = rng.standard_normal((pixels, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    f[rows] = (p32[labels[rows]] + 1e3 * u[rows]).astype(F32)
    labels[pick["label_255"]] = 255
    labels[pick["label_unseen"]] = un if un is not None else 2
    rows = pick["soft_unseen_only"]
    target[rows] = 0
    if un is not None:
        target[rows, un] = 1
    target[pick["target_1p5"], lane[pick["target_1p5"]]] = 1.5
    rows = pick["nan_target"]
    target[rows & (r % 2 == 0)] = np.nan
    part = rows & (r % 2 == 1)
    target[part, lane[part]] = np.nan
    rows = pick["nan_feature"]
    ch = rng.integers(0, dim, pixels)
    f[rows & (r % 2 == 0), ch[rows & (r % 2 == 0)]] = np.nan
    f[rows & (r % 2 == 1), ch[rows & (r % 2 == 1)]] = np.inf
    wpx = rng.uniform(0.25, 1.75, pixels).astype(F32)
    wpx[pick["w_zero"]], wpx[pick["w_negative"]], wpx[pick["w_nan"]] = 0.0, -0.5, np.nan
    wimg = rng.uniform(0.5, 1.5, batch).astype(F32)
    if row_kind == "img_zero":
        wimg[:] = 0
    elif row_kind is None:
        if batch >= 2:
            wimg[1] = 0
        both = (pick["w_zero"] | pick["label_255"] | pick["target_1p5"]) & ((r // 14) % 2 == 1)
        f[both, 0] = np.nan
    return f, labels, target, wpx, wimg, proto, seen


class LegBackend:
    """The float32 leg in the kernels' place (optionally with one mutation), on the same padded buffers, NaN-prefilled outputs."""

    def __init__(self, mut=None):
        self.mut = mut

    def contrast(self, fbuf, dim, labels, tbuf, classes, wpx, wimg, batch, ppi, proto, seen, inv_tau, reduction, want_grad):
        pixels, ldf = fbuf.shape
        out = contrast(fbuf[:, :dim], labels, None if tbuf is None else tbuf[:, :classes], proto, seen, inv_tau, wpx, wimg, batch, ppi,
                       reduction, F32, self.mut)
        d = None
        if want_grad:
            d = np.full((pixels, ldf), 0.5 if self.mut == "pad_lanes" else 0.0, dtype=F32)
            d[:, :dim] = out["grad"][0]
        return F32(out["loss"][0]), d, out["stats"]

    def assign(self, fbuf, dim, classes, ldc, proto, seen, inv_tau):
        out = np.zeros((fbuf.shape[0], ldc), dtype=F32)
        out[:, :classes] = assign(fbuf[:, :dim], proto, seen, inv_tau, F32)[0]
        return out


def _bits(v):
    return np.asarray(v, dtype=F32).view(np.uint32)            # NaN compares by its bits


def grade_case(backend, batch, ppi, classes, dim, seed, log=print, row_kind=None, ldf=None, ldt=None, ldc=None, combos=COMBOS,
               weight_variants=True, inv_tau=INV_TAU, seen=None):
    """One (batch, pix_per_image, classes, dim) case through ``backend``: every (form, reduction) of ``combos`` with both weights,
    graded on loss and feature gradient with the counters exact, pad lanes and void pixels exactly 0, the loss-only call the same
    bits; the first combination is run twice over and (``weight_variants``) with each weight alone and with none; then the
    assignment, graded, its pad lanes 0, its NaN rows where the contract puts them, the same bits on a second call.
    ``seen`` / ``inv_tau`` override the case's (the whole-call cases: nothing seen, no temperature).  Returns the Grader."""
    ldf = ldf or dim
    ldt = ldt or ceil_to(classes, 4)
    ldc = ldc or ceil_to(classes, 4)
    f, labels, target, wpx, wimg, proto, seen_case = make_case(batch, ppi, classes, dim, seed, row_kind)
    seen = seen_case if seen is None else np.asarray(seen, dtype=np.int32)
    fbuf, tbuf = embed(f, ldf), embed(target, ldt)
    tag = (f"contrast {batch}x{ppi} C={classes} D={dim} ldf={ldf} ldt={ldt} ldc={ldc}{'' if row_kind is None else ' ' + row_kind}"
           f"{'' if seen.any() else ' none-seen'}{'' if inv_tau > 0 else ' inv_tau=0'}")
    g = Grader(tag, log)
    dead_call = not (seen.any() and inv_tau > 0)

    def one(form, reduction, a, b, extra=False):
        what = f"{form} {reduction}{'' if a is not None else ' no-wpx'}{'' if b is not None else ' no-wimg'}"
        lab, tg, tb = (labels, None, None) if form == "hard" else (None, target, tbuf)
        r64 = contrast(f, lab, tg, proto, seen, inv_tau, a, b, batch, ppi, reduction, F64)
        r32 = contrast(f, lab, tg, proto, seen, inv_tau, a, b, batch, ppi, reduction, F32)
        args = (fbuf, dim, lab, tb, classes, a, b, batch, ppi, proto, seen, inv_tau, reduction)
        loss, d, stats = backend.contrast(*args, True)
        loss0, d0, stats0 = backend.contrast(*args, False)
        assert d0 is None
        if np.isnan(r64["loss"][0]):
            ok = bool(np.isnan(loss)) and bool(np.isnan(r32["loss"][0]))
            log(f"loss-grade {tag} {what} loss: D == 0, {'NaN' if ok else 'NOT NaN'}")
            if not ok:
                g.bad.append(f"{what} loss: expected NaN for D == 0, got {loss}")
        elif dead_call:
            g.exact(f"{what} loss of a call without seen classes or temperature is +0", _bits(loss), _bits(0.0))
        else:
            g.grade(f"{what} loss", loss, r64["loss"][0], r32["loss"][0], r64["loss"][1])
        g.exact(f"{what} loss, loss-only call", _bits(loss0), _bits(loss))
        g.grade(f"{what} dfeat", d[:, :dim], r64["grad"][0], r32["grad"][0], r64["grad"][1])
        g.zero(f"{what} dfeat pad lanes", d[:, dim:])
        g.zero(f"{what} dfeat void pixels", d[r64["why"] != 0])
        if dead_call:
            g.zero(f"{what} dfeat of a call without seen classes or temperature", d)
        g.exact(f"{what} stats", stats, r64["stats"])
        g.exact(f"{what} stats, loss-only call", stats0, r64["stats"])
        if extra:
            again = backend.contrast(*args, True)
            g.exact(f"{what} loss, second call", _bits(again[0]), _bits(loss))
            g.exact(f"{what} dfeat, second call", again[1].view(np.uint32), d.view(np.uint32))

    for i, (form, reduction) in enumerate(combos):
        one(form, reduction, wpx, wimg, extra=i == 0)
    for a, b in ((wpx, None), (None, wimg), (None, None)) if weight_variants else ():
        one(combos[0][0], "weighted_mean", a, b)

    s = backend.assign(fbuf, dim, classes, ldc, proto, seen, inv_tau)
    s64, mag = assign(f, proto, seen, inv_tau, F64)
    s32, _ = assign(f, proto, seen, inv_tau, F32)
    bad = np.isnan(s64).any(1)
    g.exact("assign NaN rows", np.isnan(s[:, :classes]), np.isnan(s64))
    if seen.any():
        g.grade("assign", s[~bad, :classes], s64[~bad], s32[~bad], mag[~bad])
    else:
        g.exact("assign without seen classes is 1 / classes", _bits(s[~bad, :classes]), _bits(s32[~bad]))
    g.zero("assign pad lanes", s[:, classes:])
    g.exact("assign, second call", backend.assign(fbuf, dim, classes, ldc, proto, seen, inv_tau).view(np.uint32), s.view(np.uint32))
    return g


# ------------------------------------------------------------------------------------------------------ torch composition
def torch_contrast_loss(feat, target, proto32, seen, inv_tau, reduction, pixel_weight, image_weight):
    """The textbook composition on [N,D,H,W] features of any float type: ``cross_entropy(-(dist - dist.min) * inv_tau, t)`` over the
    seen classes with the [pixels, C, D] broadcast; void pixels by hand.  target: an integer [N,H,W] mask or a float [N,C,H,W]
    distribution.  Returns (loss, dead [N,H,W])."""
    import torch
    import torch.nn.functional as F
    n, dch, h, w = feat.shape
    seen_t = torch.as_tensor(np.asarray(seen).astype(bool), device=feat.device)
    pr = proto32.to(feat.dtype)
    C = pr.shape[0]
    wt = torch.ones((n, h, w), dtype=feat.dtype, device=feat.device)
    if pixel_weight is not None:
        wt = wt * pixel_weight.to(feat.dtype)
    if image_weight is not None:
        wt = wt * image_weight.to(feat.dtype)[:, None, None]
    dead = ~(wt > 0) | ~torch.isfinite(wt) | ~torch.isfinite(feat).all(1)
    if target.is_floating_point():
        t = target.to(feat.dtype)
        dead = dead | ~((t >= 0) & (t <= 1)).all(1)
        t = torch.where(seen_t[None, :, None, None], torch.nan_to_num(t), torch.zeros_like(t))
        dead = dead | (t.sum(1) == 0)
    else:
        lab = target.long()
        ok = (lab >= 0) & (lab < C)
        ok = ok & seen_t[torch.where(ok, lab, torch.zeros_like(lab))]
        dead = dead | ~ok
        t = F.one_hot(torch.where(ok, lab, torch.zeros_like(lab)), C).permute(0, 3, 1, 2).to(feat.dtype)
    x = torch.where(dead[:, None], torch.zeros_like(feat), feat).permute(0, 2, 3, 1).reshape(-1, dch)
    dist = ((x[:, None, :] - pr[None, :, :]) ** 2).sum(2)[:, seen_t]
    z = -(dist - dist.min(1, keepdim=True).values) * inv_tau
    l = F.cross_entropy(z, t.permute(0, 2, 3, 1).reshape(-1, C)[:, seen_t], reduction="none").view(n, h, w)
    wt = torch.where(dead, torch.zeros_like(wt), wt)
    div = {"mean": float(n * h * w), "sum": 1.0}.get(reduction)
    if div is None:
        wv = torch.ones((n, h, w), dtype=feat.dtype, device=feat.device)
        if pixel_weight is not None:
            wv = wv * pixel_weight.to(feat.dtype)
        if image_weight is not None:
            wv = wv * image_weight.to(feat.dtype)[:, None, None]
        div = wv[(wv > 0) & torch.isfinite(wv)].sum()
    return (wt * l).sum() / div, dead
