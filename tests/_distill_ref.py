"""numpy restatement of the distillation kernels (csrc/distill.hip: udaseg_soft_ce_fwd_bwd, udaseg_pixel_weight_sum,
udaseg_conf_share), in the manner of ``_entropy_ref`` and ``_loss_ref``, whose ``_seqsum``, ``UNDERFLOW``, ``PAD_JUNK``, ``Grader`` and bar
it reuses.

Per pixel, with lp = log_softmax(z), p = exp(lp) of the student, q the teacher's distribution (``probs``: given, lq = log q; otherwise
q = softmax(t / T), lq = log_softmax(t / T)) and Q = sum_c q_c:

    ce:         l = -sum_c q_c lp_c                                   dl/dz_k = Q p_k - q_k
    kl:         l =  sum_c q_c (lq_c - lp_c)                          the same gradient
    symmetric:  l = alpha ce + beta sum_c p_c g_c,  g_c = -max(lq_c, log_floor), -log_floor where q_c == 0
                dl/dz_k = alpha (Q p_k - q_k) + beta p_k (g_k - sum_c p_c g_c)

A lane with q_c == 0 contributes exactly 0 to ce and kl, a lane with p_c == 0 exactly 0 to the reverse term.  w_p = weight_px[p] *
weight_img[p // pix_per_image] is the fp32 product in BOTH legs (a number the kernel is handed, like a C float argument).  A pixel is
void -- loss 0, gradient 0, magnitude 0, so only 0 passes -- when w_p == 0 (stats[1]), when w_p is negative or not finite, a
teacher lane is not finite, a probability lies outside [0, 1] or Q == 0 (stats[2]).  loss = sum_p w_p l_p / D with D = pixels
('mean'), 1 ('sum') or the sum of the w_p that do not void their pixel ('weighted_mean'; D == 0 gives NaN); the gradient carries
w_p / D; colsum is its per-class sum over the pixels.

The arithmetic is generic over ``elem``: ``np.float64`` is the reference (tests/test_distill_host.py proves it against torch's
double-precision autograd), ``np.float32`` follows the kernel's order of operations and is the leg the bar is measured from.

MAGNITUDES.  Every value comes with the sum of the absolute values of the terms that formed it, and errors are judged relative to
that.  A log probability (x - mx) - log s counts |x| + |mx| + |log s| (``_loss_ref``).  A probability exp(lp) inherits the ABSOLUTE
error of its exponent as a RELATIVE error, so its magnitude is p (1 + mag_lp) + UNDERFLOW (one rounding of the exp, the exponent's
terms, and fp32's lack of relative precision below the normal range); a given probability (``probs``) is exact: magnitude q.
Products propagate to first order: mag(a b) = mag_a |b| + |a| mag_b, sums add.  This is written down here rather than taken from
``_entropy_ref`` (which gives a probability the magnitude p + UNDERFLOW) because q_c lp_c with q = exp(lq) has two log
probabilities behind it, and a bar that forgets the teacher's would rest on the fp32 leg's luck in the single-row cases.

The second half is the grading, written against a *backend* (the kernels: tests/test_gpu_distill.py; the float32 leg, alone or with
one of MUTATIONS: tests/test_distill_host.py): padded NHWC buffers whose pad lanes hold 7.0 and one 1e30, outputs pre-filled with NaN,
pad lanes and void pixels of the gradient exactly 0, the loss the same bits with and without its gradient, the counters exact.
"""
import numpy as np

from _loss_ref import F32, F64, FLOOR, PAD_JUNK, UNDERFLOW, Grader, _a, _seqsum, f32  # noqa: F401

KINDS = ("ce", "kl", "symmetric")
REDUCTIONS = ("mean", "sum", "weighted_mean")
MUTATIONS = ("no_Q", "floor_after_negation", "void_grad", "wimg_by_pixel", "double_divisor", "no_rowsum")
BLOCKS, THREADS = 1024, 256                # udaseg_seg_partials() blocks of 256 pixels: beyond them a thread takes a second pixel
HP = dict(inv_temp=f32(1.0 / 1.5), alpha=0.75, beta=1.25, log_floor=-4.0)      # what the graded calls pass, exact in fp32


def ceil_to(c, a):
    return (c + a - 1) // a * a


# ------------------------------------------------------------------------------------------------------------------ weights
def pixel_weights(wpx, wimg, batch, ppi, mut=None):
    """(w fp32 [pixels], why [pixels]): why 0 = the pixel counts, 1 = void by a zero weight, 2 = void by a negative or non-finite one."""
    pixels = batch * ppi
    w = np.ones(pixels, dtype=F32) if wpx is None else np.asarray(wpx, dtype=F32).copy()
    if wimg is not None:
        p = np.arange(pixels)
        idx = np.minimum(p, batch - 1) if mut == "wimg_by_pixel" else p // ppi
        with np.errstate(invalid="ignore", over="ignore"):
            w = (w * np.asarray(wimg, dtype=F32)[idx]).astype(F32)
    with np.errstate(invalid="ignore"):
        why = np.where(w == 0, 1, np.where((w > 0) & np.isfinite(w), 0, 2))
    return w, why


def pixel_weight_sum(wpx, wimg, batch, ppi):
    """(D float64, [n_zero, n_invalid] int64): udaseg_pixel_weight_sum's outputs."""
    w, why = pixel_weights(wpx, wimg, batch, ppi)
    return F64(w[why == 0].astype(F64).sum()), np.array([(why == 1).sum(), (why == 2).sum()], dtype=np.int64)


# --------------------------------------------------------------------------------------------------------------------- rows
def _log_softmax(x, elem):
    """The kernel's row: d = x - mx, s = sum exp(d) left to right, lp = d - log s, p = exp(lp); (lp, p, mag_lp)."""
    mx = x.max(1, keepdims=True)
    d = (x - mx).astype(elem)
    s = _seqsum(np.exp(d).astype(elem), elem)[:, None]
    lg = np.log(s).astype(elem)
    lp = (d - lg).astype(elem)
    return lp, np.exp(lp).astype(elem), _a(x) + _a(mx) + _a(lg)


def classify(t, wpx, wimg, batch, ppi, probs, hp, mut=None):
    """(w, why) with the teacher's part of the void rule added: decided on the fp32 numbers the kernel tests, for both legs."""
    w, why = pixel_weights(wpx, wimg, batch, ppi, mut)
    with np.errstate(invalid="ignore", over="ignore"):
        tt = np.asarray(t, dtype=F32) if probs else (np.asarray(t, dtype=F32) * F32(hp["inv_temp"])).astype(F32)
        bad = ~np.isfinite(tt).all(1)
        if probs:
            bad |= ((tt < 0) | (tt > 1)).any(1) | (tt == 0).all(1)
    return w, np.where((why == 0) & bad, 2, why)


def soft_ce(z, t, wpx, wimg, batch, ppi, probs, kind, hp, reduction, elem=F64, mut=None):
    """name -> (value, magnitude) for loss, grad [pixels, classes], colsum [classes]; plus "stats" (int64 [3]) and "why" [pixels]."""
    z, t = np.asarray(z), np.asarray(t)
    pixels, classes = z.shape
    assert pixels == batch * ppi and t.shape == z.shape
    w, why = classify(t, wpx, wimg, batch, ppi, probs, hp, mut)
    live = np.nonzero(why == 0)[0]
    alpha, beta, floor = elem(hp["alpha"]), elem(hp["beta"]), elem(hp["log_floor"])

    lp, p, mag_lp = _log_softmax(z[live].astype(elem), elem)
    p64 = p.astype(F64)
    mp = p64 * (1.0 + mag_lp) + UNDERFLOW
    if probs:
        q = t[live].astype(elem)
        with np.errstate(divide="ignore"):
            lq = np.where(q > 0, np.log(np.where(q > 0, q, 1)), 0).astype(elem)
        mag_lq = _a(lq)
        mq = q.astype(F64)
    else:
        x = (t[live].astype(elem) * elem(hp["inv_temp"])).astype(elem)
        lq, q, mag_lq = _log_softmax(x, elem)
        mq = q.astype(F64) * (1.0 + mag_lq) + UNDERFLOW
    q64 = q.astype(F64)
    pos, pp = q > 0, p > 0
    big_q = _seqsum(q, elem)[:, None]
    m_big_q = mq.sum(1, keepdims=True)

    if kind == "kl":
        diff = (lq - lp).astype(elem)
        terms = np.where(pos, (q * diff).astype(elem), elem(0))
        mag_terms = np.where(pos, mq * _a(diff) + q64 * (mag_lq + mag_lp), 0.0)
    else:
        terms = np.where(pos, -(q * lp).astype(elem), elem(0))
        mag_terms = np.where(pos, mq * _a(lp) + q64 * mag_lp, 0.0)
    fwd = _seqsum(terms.astype(elem), elem)
    mag_fwd = mag_terms.sum(1)
    d01 = ((big_q * p).astype(elem) - q).astype(elem) if mut != "no_Q" else (p - q).astype(elem)
    mag_d01 = m_big_q * p64 + _a(big_q) * mp + mq
    if kind == "symmetric":
        if mut == "floor_after_negation":
            g = np.where(pos, np.maximum(-lq, floor), -floor).astype(elem)
        else:
            g = np.where(pos, -np.maximum(lq, floor), -floor).astype(elem)
        mag_g = np.where(pos & (lq > floor), mag_lq, abs(float(floor)))
        rev = _seqsum(np.where(pp, (p * g).astype(elem), elem(0)).astype(elem), elem)[:, None]
        mag_rev = np.where(pp, mp * _a(g) + p64 * mag_g, 0.0).sum(1, keepdims=True)
        l = ((alpha * fwd).astype(elem) + (beta * rev[:, 0]).astype(elem)).astype(elem)
        mag_l = abs(float(alpha)) * mag_fwd + abs(float(beta)) * mag_rev[:, 0]
        centre = rev if mut != "no_rowsum" else rev * elem(0)
        back = np.where(pp, (beta * (p * (g - centre).astype(elem)).astype(elem)).astype(elem), elem(0))
        d = ((alpha * d01).astype(elem) + back).astype(elem)
        mag_d = abs(float(alpha)) * mag_d01 + abs(float(beta)) * (mp * _a(g - rev) + p64 * (mag_g + mag_rev))
    else:
        l, mag_l, d, mag_d = fwd, mag_fwd, d01, mag_d01

    wl = w[live].astype(elem)
    total = (wl * l).astype(elem).astype(F64).sum()
    if reduction == "mean":
        div, scale = float(pixels), elem(1) / elem(pixels)
    elif reduction == "sum":
        div, scale = 1.0, elem(1)
    else:
        w_only, why_w = pixel_weights(wpx, wimg, batch, ppi, mut)
        div = float(w_only[why_w == 0].astype(F64).sum())
        with np.errstate(divide="ignore"):
            scale = elem(F64(1.0) / F64(div))
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = elem(F64(total) / F64(div))
        mag_loss = float((wl.astype(F64) * mag_l).sum() / div) if div else 0.0
    cw = (scale * wl).astype(elem)
    if mut == "double_divisor":
        cw = (scale * cw).astype(elem)
    grad = np.zeros((pixels, classes), dtype=elem)
    mag_grad = np.zeros((pixels, classes), dtype=F64)
    grad[live] = (cw[:, None] * d).astype(elem)
    mag_grad[live] = _a(scale * wl)[:, None] * mag_d
    if mut == "void_grad":
        grad[why == 2] = elem(scale) * elem(0.25)
    if elem is F64:
        colsum = grad.sum(0)
    else:
        pad = (-pixels) % 256
        gp = np.concatenate([grad, np.zeros((pad, classes), dtype=elem)]) if pad else grad
        colsum = gp.reshape(-1, 256, classes).sum(1, dtype=F32).sum(0, dtype=F32)
    stats = np.array([(why == k).sum() for k in range(3)], dtype=np.int64)
    return {"loss": (loss, mag_loss), "grad": (grad, mag_grad), "colsum": (colsum, mag_grad.sum(0)), "stats": stats, "why": why}


# ------------------------------------------------------------------------------------------------------------ confidence share
def conf_share(scores, batch, ppi, probs, tau):
    """(above int64 [batch], nonfinite int64 [batch], share fp32 [batch]): the winner confidence of pseudo.py's module docstring
    (1 / S with S in four fp32 chains for logits, q[c^] for probabilities), counted per image against tau (a C float)."""
    s = np.asarray(scores, dtype=F32)
    pixels, classes = s.shape
    tau = F32(tau)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # channel 0 seeds the maximum whatever it holds; a NaN beyond it never compares greater and is stepped over
        m = np.where(np.isnan(s[:, 0]), s[:, 0], np.where(np.isnan(s), -np.inf, s).max(1)).astype(F32)
        if probs:
            conf = m
            finite = ~np.isnan(s).any(1) & (m >= 0) & (m <= 1)
        else:
            e = np.exp((s - m[:, None]).astype(F32)).astype(F32)
            chains = [np.zeros(pixels, dtype=F32) for _ in range(4)]
            for c in range(classes):
                chains[c % 4] = (chains[c % 4] + e[:, c]).astype(F32)
            big_s = ((chains[0] + chains[1]).astype(F32) + (chains[2] + chains[3]).astype(F32)).astype(F32)
            conf = (F32(1) / big_s).astype(F32)
            finite = np.isfinite(conf)
        hit = finite & (conf >= tau)
    img = np.arange(pixels) // ppi
    above = np.bincount(img[hit], minlength=batch).astype(np.int64)
    nonfinite = np.bincount(img[~finite], minlength=batch).astype(np.int64)
    return above, nonfinite, (above.astype(F64) / F64(ppi)).astype(F32)


def conf64(scores, probs):
    """The winner confidence in float64 (NaN where the fp32 rule calls the pixel non-finite is not decided here)."""
    s = np.asarray(scores, dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = s.max(1)
        return m if probs else 1.0 / np.exp(s - m[:, None]).sum(1)


# ------------------------------------------------------------------------------------------------------------ cases and grading
CLASSES = (2, 5, 12, 23, 32)
SHAPES = ((1, 1), (3, 85), (1, 257))       # batch x pix_per_image: one pixel; image boundaries inside a wave; a second block
BIG = (1, BLOCKS * THREADS + 3)            # three threads take a second grid-stride pixel
ROW_KINDS = ("random", "one_hot", "saturated", "nan_teacher", "prob_1p5", "subnormal", "zero_probs", "w_zero", "w_negative", "w_nan",
             "img_zero")
COMBOS = tuple((k, pr, r) for k in KINDS for pr in (0, 1) for r in REDUCTIONS)
COVER = (("ce", 0, "mean"), ("kl", 1, "weighted_mean"), ("symmetric", 1, "sum"), ("symmetric", 0, "mean"))   # every kind, mode, reduction


def make_case(batch, ppi, classes, seed, row_kind=None):
    """Student logits, teacher logits, teacher probabilities ([pixels, classes] fp32), weight_px [pixels], weight_img [batch].
    Rows i mod 13 = 1.. are the special kinds of ROW_KINDS[1:] in order; ``row_kind`` makes every row of that kind.
    random: scale 3.  one_hot: one probability 1, the rest 0 (logits: 400 in one lane, whose softmax is one-hot in fp32).
    saturated: 80 in one student lane (200 on every other such row: the other probabilities are 0 in fp32).  nan_teacher: the whole row NaN (what proto.rectify writes) on even rows, one lane on odd.
    prob_1p5 / zero_probs: a probability of 1.5 / all probabilities 0 (void with ``probs``).  subnormal: probabilities that sum to 0.7.
    w_zero / w_negative / w_nan: weight_px 0, -0.5, NaN.  img_zero: image 1's weight_img is 0 (all of them for the single-row case)."""
    rng = np.random.default_rng(seed)
    pixels = batch * ppi
    z = (3.0 * rng.standard_normal((pixels, classes))).astype(F32)
    tl = (3.0 * rng.standard_normal((pixels, classes))).astype(F32)
    e = np.exp(3.0 * rng.standard_normal((pixels, classes)))
    tp = np.minimum((e / e.sum(1, keepdims=True)).astype(F32), F32(1))
    r = np.arange(pixels)
    lane = rng.integers(0, classes, pixels)
    pick = {k: ((r % 13 == i + 1) if row_kind is None else np.full(pixels, row_kind == k)) for i, k in enumerate(ROW_KINDS[1:])}
    rows = pick["one_hot"]
    tp[rows] = 0
    tp[rows, lane[rows]] = 1
    tl[rows, lane[rows]] = 400.0
    rows = pick["saturated"]
    z[rows, lane[rows]] = np.where((r[rows] // 13) % 2 == 0, 80.0, 200.0)
    rows = pick["nan_teacher"]
    whole = rows & (r % 2 == 0)
    tl[whole], tp[whole] = np.nan, np.nan
    part = rows & (r % 2 == 1)
    tl[part, lane[part]], tp[part, lane[part]] = np.nan, np.nan
    tp[pick["prob_1p5"], lane[pick["prob_1p5"]]] = 1.5
    tp[pick["subnormal"]] = (tp[pick["subnormal"]] * F32(0.7)).astype(F32)
    tp[pick["zero_probs"]] = 0
    wpx = rng.uniform(0.25, 1.75, pixels).astype(F32)
    wpx[pick["w_zero"]], wpx[pick["w_negative"]], wpx[pick["w_nan"]] = 0.0, -0.5, np.nan
    wimg = rng.uniform(0.5, 1.5, batch).astype(F32)
    if row_kind == "img_zero":
        wimg[:] = 0
    elif row_kind is None and batch >= 2:
        wimg[1] = 0
    return z, tl, tp, wpx, wimg


def embed(x, ld):
    """The padded buffer [pixels, ld]: pad lanes hold PAD_JUNK, one of them 1e30."""
    pixels, classes = x.shape
    buf = np.full((pixels, ld), PAD_JUNK, dtype=F32)
    buf[:, :classes] = x
    if ld > classes:
        buf[pixels // 2, ld - 1] = 1e30
    return buf


class LegBackend:
    """The float32 leg in the kernels' place (optionally with one mutation), on the same padded buffers, NaN-prefilled outputs."""

    def __init__(self, mut=None):
        self.mut = mut

    def soft_ce(self, zbuf, tbuf, wpx, wimg, batch, ppi, classes, probs, kind, hp, reduction, want_grad, want_colsum):
        pixels, ldc = zbuf.shape
        out = soft_ce(zbuf[:, :classes], tbuf[:, :classes], wpx, wimg, batch, ppi, probs, kind, hp, reduction, F32, self.mut)
        d = np.zeros((pixels, ldc), dtype=F32)
        d[:, :classes] = out["grad"][0]
        cs = np.zeros(ldc, dtype=F32)
        cs[:classes] = out["colsum"][0]
        return F32(out["loss"][0]), (d if want_grad else None), (cs if want_colsum else None), out["stats"]

    def pixel_weight_sum(self, wpx, wimg, batch, ppi):
        return pixel_weight_sum(wpx, wimg, batch, ppi)

    def conf_share(self, sbuf, batch, ppi, classes, probs, tau):
        return conf_share(sbuf[:, :classes], batch, ppi, probs, tau)


def grade_case(backend, batch, ppi, classes, seed, log=print, row_kind=None, ldc=None, ldt=None, combos=COMBOS, hp=HP,
               weight_variants=True):
    """One (batch, pix_per_image, classes) case through ``backend``: every (kind, probs, reduction) of ``combos`` with both weights,
    each graded on loss, gradient and column sums with the counters exact; the loss-only call and the call without column sums
    must return the same bits; the first combination is run twice over and (``weight_variants``) with each weight alone and with
    none, where udaseg_pixel_weight_sum is checked too.
    Returns the Grader (``.done()`` asserts)."""
    ldc = ldc or ceil_to(classes, 4)
    ldt = ldt or ceil_to(classes, 4)
    z, tl, tp, wpx, wimg = make_case(batch, ppi, classes, seed, row_kind)
    zbuf, tbuf = embed(z, ldc), {0: embed(tl, ldt), 1: embed(tp, ldt)}
    tag = f"distill {batch}x{ppi} C={classes} ldc={ldc} ldt={ldt}{'' if row_kind is None else ' ' + row_kind}"
    g = Grader(tag, log)

    def one(kind, probs, reduction, a, b, extra=False):
        what = f"{kind} probs={probs} {reduction}{'' if a is not None else ' no-wpx'}{'' if b is not None else ' no-wimg'}"
        t = tp if probs else tl
        r64 = soft_ce(z, t, a, b, batch, ppi, probs, kind, hp, reduction, F64)
        r32 = soft_ce(z, t, a, b, batch, ppi, probs, kind, hp, reduction, F32)
        loss, d, cs, stats = backend.soft_ce(zbuf, tbuf[probs], a, b, batch, ppi, classes, probs, kind, hp, reduction, True, True)
        loss0, d0, cs0, stats0 = backend.soft_ce(zbuf, tbuf[probs], a, b, batch, ppi, classes, probs, kind, hp, reduction, False, False)
        loss1, d1, cs1, _ = backend.soft_ce(zbuf, tbuf[probs], a, b, batch, ppi, classes, probs, kind, hp, reduction, True, False)
        assert d0 is None and cs0 is None and cs1 is None
        bits = lambda v: np.asarray(v, dtype=F32).view(np.uint32)              # noqa: E731  (NaN compares by its bits)
        if np.isnan(r64["loss"][0]):
            ok = bool(np.isnan(loss)) and bool(np.isnan(r32["loss"][0]))
            log(f"loss-grade {tag} {what} loss: D == 0, {'NaN' if ok else 'NOT NaN'}")
            if not ok:
                g.bad.append(f"{what} loss: expected NaN for D == 0, got {loss}")
        else:
            g.grade(f"{what} loss", loss, r64["loss"][0], r32["loss"][0], r64["loss"][1])
        g.exact(f"{what} loss, loss-only call", bits(loss0), bits(loss))
        g.exact(f"{what} loss, call without colsum", bits(loss1), bits(loss))
        g.exact(f"{what} dlogits, call without colsum", d1.view(np.uint32), d.view(np.uint32))
        g.grade(f"{what} dlogits", d[:, :classes], r64["grad"][0], r32["grad"][0], r64["grad"][1])
        g.zero(f"{what} dlogits pad lanes", d[:, classes:])
        g.zero(f"{what} dlogits void pixels", d[r64["why"] != 0])
        g.grade(f"{what} colsum", cs[:classes], r64["colsum"][0], r32["colsum"][0], r64["colsum"][1])
        g.zero(f"{what} colsum pad lanes", cs[classes:])
        g.exact(f"{what} stats", stats, r64["stats"])
        g.exact(f"{what} stats, loss-only call", stats0, r64["stats"])
        if extra:
            again = backend.soft_ce(zbuf, tbuf[probs], a, b, batch, ppi, classes, probs, kind, hp, reduction, True, True)
            g.exact(f"{what} loss, second call", bits(again[0]), bits(loss))
            g.exact(f"{what} dlogits, second call", again[1].view(np.uint32), d.view(np.uint32))
            g.exact(f"{what} colsum, second call", again[2].view(np.uint32), cs.view(np.uint32))

    for i, (kind, probs, reduction) in enumerate(combos):
        one(kind, probs, reduction, wpx, wimg, extra=i == 0)
    kind, probs, _ = combos[0]
    for a, b in ((wpx, None), (None, wimg), (None, None)) if weight_variants else ():
        one(kind, probs, "weighted_mean", a, b)
        denom, counts = backend.pixel_weight_sum(a, b, batch, ppi)
        want, want_counts = pixel_weight_sum(a, b, batch, ppi)
        # a float64 sum of n fp32 numbers in any order is within (n - 1) 2^-53 sum |w| of the exact sum; two such sums are compared
        tol = 2.0 * batch * ppi * 2.0 ** -53 * float(want)
        ok = abs(float(denom) - float(want)) <= tol
        log(f"loss-grade {tag} weight sum{'' if a is not None else ' no-wpx'}{'' if b is not None else ' no-wimg'}: "
            f"|D - mirror| {abs(float(denom) - float(want)):.3e}  bar {tol:.3e}")
        if not ok:
            g.bad.append(f"weight sum {denom!r} != {want!r}")
        g.exact("weight counts", counts, want_counts)
    return g


def make_scores(batch, ppi, classes, seed, probs, tau):
    """[pixels, classes] fp32 scores for udaseg_conf_share with their pitfalls: NaN and +inf rows, probabilities above 1, exact
    ties of the maximum, a confidence of exactly tau (probabilities: tau in one lane; logits: a row of -400 beside one 0, confidence
    exactly 1, and for two classes a uniform row, confidence exactly 0.5).  The kernel's expf and numpy's may differ in the last
    place, so a logits row whose float64 confidence lies within 2^-18 of tau -- a hundred times the fp32 error of 1 / S -- is
    replaced by a confident one: the counts of the mirror are then the kernel's whatever the last bit of an exponential."""
    rng = np.random.default_rng(seed)
    pixels = batch * ppi
    r = np.arange(pixels)
    lane = rng.integers(0, classes, pixels)
    if probs:
        e = np.exp(3.0 * rng.standard_normal((pixels, classes)))
        s = np.minimum((e / e.sum(1, keepdims=True)).astype(F32), F32(1))
        s[r % 11 == 3, 0] = F32(tau)
        s[r % 11 == 3, 1:] = 0
        s[r % 11 == 4, lane[r % 11 == 4]] = 1.5
    else:
        s = (3.0 * rng.standard_normal((pixels, classes))).astype(F32)
        s[r % 11 == 3] = -400.0
        s[r % 11 == 3, lane[r % 11 == 3]] = 0.0
        s[r % 11 == 4, lane[r % 11 == 4]] = np.inf
        if classes == 2:
            s[r % 11 == 6] = 1.25
    s[r % 11 == 5, lane[r % 11 == 5]] = np.nan
    s[r % 11 == 7] = s[r % 11 == 7, :1]                       # every lane equal: the first wins
    if not probs:
        c = conf64(s, 0)
        with np.errstate(invalid="ignore"):
            near = np.isfinite(c) & (np.abs(c - float(F32(tau))) < 2.0 ** -18) & ~((c == 1.0) | (c == 0.5))
        s[near] = -400.0
        s[near, 0] = 0.0
    return s


def grade_share(backend, batch, ppi, classes, seed, log=print, ldc=None):
    ldc = ldc or ceil_to(classes, 4)
    g = Grader(f"conf_share {batch}x{ppi} C={classes} ldc={ldc}", log)
    for probs, tau in ((0, 0.968), (1, 0.968), (0, 0.5), (1, 0.25), (0, 1.0)):
        s = make_scores(batch, ppi, classes, seed, probs, tau)
        above, nonfinite, share = backend.conf_share(embed(s, ldc), batch, ppi, classes, probs, f32(tau))
        want = conf_share(s, batch, ppi, probs, f32(tau))
        g.exact(f"probs={probs} tau={tau} above", above, want[0])
        g.exact(f"probs={probs} tau={tau} nonfinite", nonfinite, want[1])
        g.exact(f"probs={probs} tau={tau} share", np.asarray(share, dtype=F32).view(np.uint32), want[2].view(np.uint32))
    return g


# ------------------------------------------------------------------------------------------------------ torch composition
def torch_soft_loss(x, t, probs, kind, T, alpha, beta, floor, reduction, pixel_weight, image_weight):
    """The textbook composition: the loss as torch ops on [N,C,H,W] tensors of any float type; void pixels (NaN teacher rows, weights <= 0) by hand."""
    import torch
    import torch.nn.functional as F
    n, c, h, w = x.shape
    wt = torch.ones((n, h, w), dtype=x.dtype, device=x.device)
    if pixel_weight is not None:
        wt = wt * pixel_weight.to(x.dtype)
    if image_weight is not None:
        wt = wt * image_weight.to(x.dtype)[:, None, None]
    dead = ~torch.isfinite(t).all(1) | ~(wt > 0)
    if probs:
        dead = dead | ((t < 0) | (t > 1)).any(1) | (t == 0).all(1)
    t = torch.where(dead[:, None], torch.full_like(t, 1.0 / c), t).to(x.dtype)
    q = t if probs else torch.softmax(t / T, 1)
    ce = F.cross_entropy(x, q, reduction="none")
    if kind == "ce":
        l = ce
    elif kind == "kl":
        l = F.kl_div(torch.log_softmax(x, 1), q, reduction="none").sum(1)
    else:
        l = alpha * ce + beta * (torch.softmax(x, 1) * -torch.clamp(torch.log(q), min=floor)).sum(1)
    wt = torch.where(dead, torch.zeros_like(wt), wt)
    div = {"mean": float(n * h * w), "sum": 1.0}.get(reduction)
    if div is None:
        wv = torch.ones((n, h, w), dtype=x.dtype, device=x.device)
        if pixel_weight is not None:
            wv = wv * pixel_weight.to(x.dtype)
        if image_weight is not None:
            wv = wv * image_weight.to(x.dtype)[:, None, None]
        div = wv[wv > 0].sum()
    return (wt * l).sum() / div, dead
