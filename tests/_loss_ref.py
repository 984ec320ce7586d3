"""numpy restatement of the loss kernels every training step ends in (csrc/losses_seg.hip: Dice per image and pooled, focal-weighted
cross entropy, consistency; csrc/losses.hip: plain cross entropy with its column sums, the discriminator tail global average pool
-> linear -> optional sigmoid, BCE with logits).

Test infrastructure, in the manner of ``_norm_ref``: the arithmetic is written once, generically over the float type ``elem`` --
``np.float64`` is the reference the kernels are held to (tests/test_loss_ref_host.py proves it against torch's double-precision
autograd), ``np.float32`` the same arithmetic in the kernels' precision and ORDER of operations (max-shifted log-sum-exp, then
``lp - lse``, then ``exp``; focal through ``ce``, ``pt = exp(-ce)``, ``max(1 - pt, 0)``): the leg the bar is measured from, never
compared for equality.  Logits are ``[pixels, classes]`` (the valid lanes only), targets int64 ``[pixels]``.  Scalars that the
kernels receive as C floats (alpha, gamma, smooth, 1 / T, weights, upstream gradients) are taken as given: callers that grade a
kernel pass values already rounded to fp32, so both legs use the number the kernel sees.

Every function also returns the MAGNITUDE of each output element: the sum of the absolute values of the terms that formed it
(|k0| (p_c + [c == t]) for a softmax gradient, 1 + pt for 1 - pt, sum |per-pixel terms| / divisor for a reduced scalar; a log
probability x - (mx + log s) counts |x| + |mx| + |log s|).  Errors are judged relative to it.  A probability's magnitude carries
UNDERFLOW = 2^-126 / 2^-22 on top: fp32 has no relative precision below its normal range (exp(-100) is 0 or a denormal, in
float64 it is 3.7e-44), so an absolute error of the smallest normal number, scaled by whatever multiplies the probability, is
within 2 ulp's worth of any bar.

``mut`` names one deliberate mistake (MUTATIONS); tests/test_loss_ref_host.py runs the float32 leg with each to show that the
grading would catch it.
"""
import numpy as np

from _norm_ref import F32, F64, FLOOR, bar, bf16_half_ulp, bf16_round, normalised  # noqa: F401  (re-exported for the graders)

UNDERFLOW = 2.0 ** -126 / FLOOR
MUTATIONS = ("dice_divisor", "absent_counted", "focal_no_pt", "consistency_no_inv_t", "pad_lane", "colsum_tail", "straddle",
             "bce_wrong_n", "dw_overwrite")
PAD_JUNK = 7.0                            # what the graded buffers hold in most pad lanes (one lane holds 1e30)


def f32(v):
    """The value a C float argument receives."""
    return float(np.float32(v))


def _a(x):
    return np.abs(np.asarray(x, dtype=F64))


def _seqsum(x, elem):
    """Left-to-right sum over the class axis in ``elem``, as the kernels' unrolled class loops."""
    return np.cumsum(x, axis=1, dtype=elem)[:, -1]


def _chunksum(x, elem, chunk=256):
    """Sum over axis 0.  float64: plain.  float32: fp32 within each run of ``chunk`` rows (a block's share), float64 across."""
    if elem is F64:
        return np.asarray(x, dtype=F64).sum(0)
    rows = x.shape[0]
    pad = (-rows) % chunk
    x = np.concatenate([x, np.zeros((pad,) + x.shape[1:], dtype=x.dtype)]) if pad else x
    return x.reshape((-1, chunk) + x.shape[1:]).astype(F32).sum(1, dtype=F32).astype(F64).sum(0)


def log_softmax(z, elem, inv_t=1.0, mut=None):
    """(lp, lse, mag_lp): x = z * inv_t, mx = max x, s = sum exp(x - mx), lse = mx + log s, lp = x - lse."""
    x = (np.asarray(z).astype(elem) * elem(inv_t)).astype(elem)
    mx = x.max(1, keepdims=True)
    s = _seqsum(np.exp(x - mx), elem)[:, None]
    if mut == "pad_lane":
        with np.errstate(over="ignore"):
            s = (s + np.exp(elem(PAD_JUNK) * elem(inv_t) - mx)).astype(elem)
    logs = np.log(s)
    lse = (mx + logs).astype(elem)
    return (x - lse).astype(elem), lse[:, 0], _a(x) + _a(mx) + _a(logs)


def live_mask(t, classes, ignore_index):
    """(live, hot): live pixels take part at all; hot pixels have a class.  ignore_index None: the entry points without void
    handling, where every pixel is live and a label outside [0, C) merely has no class."""
    t = np.asarray(t)
    inr = (t >= 0) & (t < classes)
    if ignore_index is None:
        return np.ones_like(inr), inr
    live = inr & (t != ignore_index)
    return live, live


def _one_hot(t, hot, classes):
    oh = np.zeros((len(t), classes), dtype=bool)
    rows = np.nonzero(hot)[0]
    oh[rows, np.asarray(t)[rows]] = True
    return oh


# ---------------------------------------------------------------------------------------------------------------------- Dice
def dice(z, t, batch, smooth, eps, pooled, ignore_index, scale, elem=F64, mut=None):
    """Soft Dice of softmax(z) against the labels, per image or pooled over the batch (csrc/losses_seg.hip dice_finish_kernel).

    per image: loss = 1 - mean_{b,c} (2I + s) / (U + s).   pooled: score_c = (2I_c + s) / max(U_c + s, eps),
    loss = mean_c (1 - score_c) [class c present].   coef[b] = (a, b) with dLoss/dp_c = a [c == t] + b, and
    grad_k = scale p_k (g_k - sum_c p_c g_c), g = b + a [c == t]; exactly 0 at void pixels.
    Returns a dict name -> (value, magnitude) for loss, coef [batch, 2, classes], grad [pixels, classes]."""
    z = np.asarray(z)
    pixels, classes = z.shape
    ppi = pixels // batch
    lp, _, _ = log_softmax(z, elem, 1.0, mut)
    p = np.exp(lp).astype(elem)
    live, hot = live_mask(t, classes, ignore_index)
    oh = _one_hot(t, hot, classes)
    pl = np.where(live[:, None], p, elem(0))
    inter = np.stack([_chunksum(np.where(oh[b * ppi:(b + 1) * ppi], pl[b * ppi:(b + 1) * ppi], elem(0)), elem) for b in range(batch)])
    psum = np.stack([_chunksum(pl[b * ppi:(b + 1) * ppi], elem) for b in range(batch)])
    count = oh.reshape(batch, ppi, classes).sum(1).astype(F64)
    s, e = float(smooth), float(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        if not pooled:
            n = classes if mut == "dice_divisor" else batch * classes
            den = psum + count + s
            num = 2.0 * inter + s
            score = num / den
            loss, mag_loss = 1.0 - score.sum() / (batch * classes), 1.0 + _a(score).sum() / (batch * classes)
            ca, cb = -(2.0 / den) / n, (num / (den * den)) / n
        else:
            i_, u_, t_ = inter.sum(0), (psum + count).sum(0), count.sum(0)
            den = u_ + s
            num = 2.0 * i_ + s
            present = np.ones_like(t_, dtype=bool) if mut == "absent_counted" else t_ > 0
            clamped = den < e
            dd = np.where(clamped, e, den)
            score = num / dd
            loss, mag_loss = np.where(present, 1.0 - score, 0.0).sum() / classes, np.where(present, 1.0 + _a(score), 0.0).sum() / classes
            ca = np.where(present, -(2.0 / dd) / classes, 0.0)
            cb = np.where(present & ~clamped, (num / (den * den)) / classes, 0.0)
            ca, cb = np.broadcast_to(ca, (batch, classes)), np.broadcast_to(cb, (batch, classes))
    coef = np.stack([ca, cb], axis=1).astype(elem)
    idx = np.arange(pixels)
    bi = (idx // 256 * 256 // ppi if mut == "straddle" else idx // ppi)
    a_p, b_p = coef[bi, 0], coef[bi, 1]
    g = (b_p + np.where(oh, a_p, elem(0))).astype(elem)
    big_s = _seqsum(p * g, elem)[:, None]
    scale = elem(scale)
    grad = (scale * p * (g - big_s)).astype(elem)
    grad[~live] = 0
    pm = p.astype(F64) + UNDERFLOW
    mag_g = _a(b_p) + np.where(oh, _a(a_p), 0.0)
    mag_grad = abs(float(scale)) * pm * (mag_g + (pm * mag_g).sum(1, keepdims=True))
    mag_grad[~live] = 0
    return {"loss": (elem(loss), mag_loss), "coef": (coef, _a(coef)), "grad": (grad, mag_grad)}


# --------------------------------------------------------------------------------------------- focal-weighted cross entropy
def focal(z, t, class_w, alpha, gamma, mean, ignore_index, scale, elem=F64, mut=None):
    """ce = w_t (lse - z_t), pt = exp(-ce), om = max(1 - pt, 0), f = alpha om^gamma ce; value = sum f / (pixels | 1) -- void pixels
    count in the divisor.  grad_k = scale df/dce w_t (p_k - [k == t]) with
    df/dce = alpha (om^gamma + ce gamma om^(gamma-1) pt) where om > 0, else alpha for gamma == 0 and 0 otherwise (the kernel's rule).
    ``scale`` is everything the gradient is multiplied by (upstream x weight, the caller's 1 / pixels for 'mean' included).
    1 - pt has the magnitude 1 + pt, so om^gamma counts (1 + pt)^gamma: that absorbs the om > 0 branch.
    Returns a dict name -> (value, magnitude) for loss and grad."""
    z = np.asarray(z)
    pixels, classes = z.shape
    lp, _, mag_lp = log_softmax(z, elem, 1.0, mut)
    live, hot = live_mask(t, classes, ignore_index)
    hot = hot & live
    oh = _one_hot(t, hot, classes)
    rows, idx = np.arange(pixels), np.where(hot, np.asarray(t), 0)
    lpt = np.where(hot, lp[rows, idx], elem(0)).astype(elem)
    mag_lpt = np.where(hot, mag_lp[rows, idx], 0.0)
    w = (np.ones(pixels, dtype=elem) if class_w is None else np.asarray(class_w).astype(elem)[idx])
    alpha, gamma, scale = elem(alpha), elem(gamma), elem(scale)
    ce = (-w * lpt).astype(elem)
    pt = np.exp(-ce).astype(elem)
    om = np.maximum(elem(1) - pt, elem(0))
    f = (alpha * np.power(om, gamma) * ce).astype(elem)
    f[~live] = 0
    m = 1.0 + pt.astype(F64)
    wa = _a(w) * abs(float(alpha))
    mag_f = np.where(live, wa * m ** float(gamma) * mag_lpt, 0.0)
    div = float(pixels) if mean else 1.0
    loss = elem(f.astype(F64).sum() / div)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        second = ce * gamma * np.power(om, gamma - elem(1))
        if mut != "focal_no_pt":
            second = second * pt
        dfdce = np.where(om > 0, alpha * (np.power(om, gamma) + second), alpha if float(gamma) == 0.0 else elem(0)).astype(elem)
    k0 = (scale * dfdce * w).astype(elem)
    p = np.exp(lp).astype(elem)
    grad = (k0[:, None] * (p - oh.astype(elem))).astype(elem)
    grad[~live] = 0
    mag_k = abs(float(scale)) * wa * (m ** float(gamma) + _a(ce) * float(gamma) * m ** (float(gamma) - 1.0) * pt.astype(F64))
    mag_grad = mag_k[:, None] * (p.astype(F64) + UNDERFLOW + oh)
    mag_grad[~live] = 0
    return {"loss": (loss, mag_f.sum() / div), "grad": (grad, mag_grad), "f": (f, mag_f)}


# --------------------------------------------------------------------------------------------------------------- consistency
def consistency(z1, z2, inv_t, batch, scale, elem=F64, mut=None):
    """Symmetric KL of softmax(z1 inv_t) and softmax(z2 inv_t), each 'batchmean', halved:
    value = sum_pix sum_c (p1 - p2)(l1 - l2) / (2 batch);  d1 = s [(p1 - p2) + p1 ((l1 - l2) - kl12)], d2 symmetric,
    s = scale inv_t / (2 batch).  Returns a dict name -> (value, magnitude) for loss, d1, d2."""
    l1, _, m1 = log_softmax(z1, elem, inv_t, mut)
    l2, _, m2 = log_softmax(z2, elem, inv_t, mut)
    p1, p2 = np.exp(l1).astype(elem), np.exp(l2).astype(elem)
    dl = (l1 - l2).astype(elem)
    acc = _seqsum((p1 - p2) * dl, elem)
    q1, q2, mdl = p1.astype(F64) + UNDERFLOW, p2.astype(F64) + UNDERFLOW, m1 + m2
    loss = elem(acc.astype(F64).sum() / (2.0 * batch))
    mag_loss = ((q1 + q2) * mdl).sum() / (2.0 * batch)
    s = elem(scale) / (elem(2) * elem(batch)) if mut == "consistency_no_inv_t" else elem(scale) * elem(inv_t) / (elem(2) * elem(batch))
    kl12, kl21 = _seqsum(p1 * dl, elem)[:, None], -_seqsum(p2 * dl, elem)[:, None]
    d1 = (s * ((p1 - p2) + p1 * (dl - kl12))).astype(elem)
    d2 = (s * ((p2 - p1) + p2 * (-dl - kl21))).astype(elem)
    sa = abs(float(s))
    mag1 = sa * ((q1 + q2) + q1 * (mdl + (q1 * mdl).sum(1, keepdims=True)))
    mag2 = sa * ((q1 + q2) + q2 * (mdl + (q2 * mdl).sum(1, keepdims=True)))
    return {"loss": (loss, mag_loss), "d1": (d1, mag1), "d2": (d2, mag2)}


# ------------------------------------------------------------------------------------------------------- plain cross entropy
def cross_entropy(z, t, grad_out, elem=F64, mut=None):
    """Mean cross entropy: lse = mx + log sum exp(z - mx), value = mean (lse - z_t), grad = (exp(z - lse) - [c == t]) grad_out / pixels,
    colsum = per-class sum of grad over the pixels.  Returns a dict name -> (value, magnitude) for loss, lse, grad, colsum."""
    x = np.asarray(z).astype(elem)
    pixels, classes = x.shape
    t = np.asarray(t)
    mx = x.max(1, keepdims=True)
    s = _seqsum(np.exp(x - mx), elem)[:, None]
    if mut == "pad_lane":
        with np.errstate(over="ignore"):
            s = (s + np.exp(elem(PAD_JUNK) - mx)).astype(elem)
    lse = (mx + np.log(s)).astype(elem)
    mag_lse = (_a(mx) + _a(np.log(s)))[:, 0]
    xt = x[np.arange(pixels), t]
    loss = elem((lse[:, 0] - xt).astype(elem).astype(F64).sum() / pixels)
    mag_loss = (mag_lse + _a(xt)).sum() / pixels
    oh = _one_hot(t, np.ones(pixels, dtype=bool), classes)
    scale = elem(grad_out) / elem(pixels)
    e = np.exp(x - lse).astype(elem)
    grad = ((e - oh.astype(elem)) * scale).astype(elem)
    mag_grad = (e.astype(F64) + UNDERFLOW + oh) * abs(float(scale))
    if elem is F64:
        colsum = grad.sum(0)
    else:
        rows = pixels - pixels % 256 if (mut == "colsum_tail" and pixels % 256) else pixels
        pad = (-rows) % 256
        g = np.concatenate([grad[:rows], np.zeros((pad, classes), dtype=elem)]) if pad else grad[:rows]
        colsum = g.reshape(-1, 256, classes).sum(1, dtype=F32).sum(0, dtype=F32)
    return {"loss": (loss, mag_loss), "lse": (lse[:, 0], mag_lse), "grad": (grad, mag_grad), "colsum": (colsum, mag_grad.sum(0))}


# ------------------------------------------------------------------------------------------------------ discriminator tail
def gap_slices(hw, splits_max=32):
    """(splits, pixels per slice, number of non-empty slices) of the pooling pass: splits = min(32, hw), per = ceil(hw / splits)."""
    splits = max(1, min(splits_max, hw))
    per = -(-hw // splits)
    return splits, per, -(-hw // per)


def tail_forward(z, w, b, sigmoid, elem=F64):
    """pooled[n, c] = mean over the pixels of z[n, :, c]; t[n] = pooled[n] . w + b; out = sigmoid(t) or t.
    float32: slice partials, their sum, x (1 / hw) as the kernels; the dot product left to right.
    Returns a dict name -> (value, magnitude) for pooled [n, c] and out [n]."""
    z = np.asarray(z)
    n, hw, c = z.shape
    w, b = np.asarray(w).astype(elem), elem(np.asarray(b).reshape(-1)[0])
    mag_pooled = _a(z).sum(1) / hw
    if elem is F64:
        pooled = z.astype(F64).sum(1) / hw
    else:
        splits, per, _ = gap_slices(hw)
        tot = np.zeros((n, c), dtype=F32)
        for s in range(splits):
            p0, p1 = s * per, min(hw, (s + 1) * per)
            part = np.zeros((n, c), dtype=F32)
            for p in range(p0, p1):
                part = part + z[:, p].astype(F32)
            tot = tot + part
        pooled = (tot * (F32(1) / F32(hw))).astype(F32)
    t = (np.cumsum(pooled * w, axis=1, dtype=elem)[:, -1] + b).astype(elem)
    mag_t = (mag_pooled * _a(w)).sum(1) + abs(float(b))
    if not sigmoid:
        return {"pooled": (pooled, mag_pooled), "out": (t, mag_t)}
    with np.errstate(over="ignore"):
        out = (elem(1) / (elem(1) + np.exp(-t))).astype(elem)
    o = out.astype(F64)
    return {"pooled": (pooled, mag_pooled), "out": (out, o * (1.0 + (1.0 - o) * mag_t) + UNDERFLOW)}


def tail_backward(dp, p, pooled, w, hw, sigmoid, elem=F64):
    """From the forward's own outputs p and pooled: dl = dp (p (1 - p) | 1);  dz[n, :, c] = w[c] dl[n] / hw (one row per image: the
    value every pixel receives);  dw[c] = sum_n dl[n] pooled[n, c];  db = sum_n dl[n].
    Returns a dict name -> (value, magnitude) for dz [n, c], dw [c], db []."""
    dp, w, pooled = np.asarray(dp).astype(elem), np.asarray(w).astype(elem), np.asarray(pooled).astype(elem)
    if sigmoid:
        p = np.asarray(p).astype(elem).reshape(-1)
        dl = (dp * (p * (elem(1) - p))).astype(elem)
        mag_dl = _a(dp) * _a(p) * (1.0 + _a(p))
        dli = (dp * p * (elem(1) - p) * (elem(1) / elem(hw))).astype(elem)           # the broadcast kernel's order
    else:
        dl, mag_dl = dp, _a(dp)
        dli = (dp * elem(1) * (elem(1) / elem(hw))).astype(elem)
    dz = (w[None, :] * dli[:, None]).astype(elem)
    dw = np.cumsum(dl[:, None] * pooled, axis=0, dtype=elem)[-1]
    db = elem(np.cumsum(dl, dtype=elem)[-1])
    return {"dz": (dz, _a(w)[None, :] * mag_dl[:, None] / hw), "dw": (dw, (mag_dl[:, None] * _a(pooled)).sum(0)), "db": (db, mag_dl.sum())}


# --------------------------------------------------------------------------------------------------------- BCE with logits
def bce(x, y, weight, grad_out, elem=F64, n_div=None):
    """weight mean((1 - y) x + softplus(-x)), softplus(v) = max(v, 0) + log1p(exp(-|v|)); y a scalar label or a per-sample vector.
    dx = (sigmoid(x) - y) grad_out weight / n.  Returns a dict name -> (value, magnitude) for loss and dx."""
    x = np.asarray(x).astype(elem).reshape(-1)
    n = x.size if n_div is None else n_div
    y = np.broadcast_to(np.asarray(y).astype(elem), x.shape)
    sp = np.maximum(-x, elem(0)) + np.log1p(np.exp(-np.abs(x)))
    terms = ((elem(1) - y) * x + sp).astype(elem)
    s = np.cumsum(terms, dtype=elem)[-1]
    loss = elem(elem(weight) * (s / elem(n)))
    mag_loss = abs(float(weight)) * (_a((1.0 - y.astype(F64)) * x) + _a(sp)).sum() / n
    g = elem(grad_out) * elem(weight) / elem(n)
    with np.errstate(over="ignore"):
        sg = (elem(1) / (elem(1) + np.exp(-x))).astype(elem)
    dx = ((sg - y) * g).astype(elem)
    return {"loss": (loss, mag_loss), "dx": (dx, (sg.astype(F64) + UNDERFLOW + _a(y)) * abs(float(g)))}


# ------------------------------------------------------------------------------------------------------------------- grading
class Grader:
    """Collects the verdicts of one case so that every figure is logged before the first assertion fires.
    bar = max(4 x the fp32 leg's worst normalised deviation from the float64 leg over the whole output, floor), floor 2^-22."""
    def __init__(self, tag, log=print):
        self.tag, self.bad, self.log, self.worst = tag, [], log, 0.0

    def grade(self, what, got, r64, r32, mag, bf16_out=False, floor=FLOOR):
        r64, mag = np.asarray(r64, dtype=F64), np.asarray(mag, dtype=F64)
        b, dmax = bar(r32, r64, mag)
        b = max(b, floor)
        got = np.asarray(got, dtype=F64)
        err = np.abs(got - r64)
        if bf16_out:
            err = np.maximum(err - bf16_half_ulp(r64, b * mag), 0.0)
        ok = got.shape == r64.shape and np.isfinite(got).all() and np.isfinite(dmax)
        e = float(normalised(err, mag).max(initial=0.0)) if ok else float("inf")
        self.worst = max(self.worst, e / b)
        self.log(f"loss-grade {self.tag} {what}: kernel-vs-f64 {e:.3e}  f32-vs-f64 {dmax:.3e}  bar {b:.3e}  e/bar {e / b:.3f}")
        if not e <= b:
            self.bad.append(f"{what}: {e:.3e} > bar {b:.3e}")

    def exact(self, what, got, want):
        """Bit for bit (NaN never equal)."""
        same = np.array_equal(np.asarray(got), np.asarray(want))
        self.log(f"loss-grade {self.tag} {what}: {'exact' if same else 'DIFFERS'}")
        if not same:
            self.bad.append(f"{what}: not bit for bit")

    def zero(self, what, got):
        got = np.asarray(got)
        bad = int(np.count_nonzero(got) + np.isnan(got).sum())
        self.log(f"loss-grade {self.tag} {what}: {bad} entries are not exactly 0")
        if bad:
            self.bad.append(f"{what}: {bad} entries are not exactly 0")

    def within_ulp(self, what, acc, old, plain):
        """An accumulating call against old + plain where a product may fuse into the add: one fp32 ulp at the largest operand."""
        acc, old, plain = (np.asarray(v, dtype=F32) for v in (acc, old, plain))
        want = old + plain
        m = np.maximum.reduce([np.abs(old), np.abs(plain), np.abs(want)]).astype(F32)
        tol = np.spacing(m).astype(F64)
        diff = np.abs(acc.astype(F64) - (old.astype(F64) + plain.astype(F64)))
        worst = float((diff / tol).max(initial=0.0)) if np.isfinite(acc).all() else float("inf")
        self.log(f"loss-grade {self.tag} {what}: worst |acc - (old + plain)| {worst:.3f} ulp  bar 1 ulp")
        if not worst <= 1.0:
            self.bad.append(f"{what}: {worst:.3f} ulp off old + plain")

    def done(self):
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)
