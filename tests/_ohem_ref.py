"""numpy mirror of hard-pixel mining for the cross entropy (csrc/ohem.hip; the definition stands in include/udaseg.h).

Test infrastructure, in the manner of ``_loss_ref``: the arithmetic is written once over the float type ``elem`` -- ``np.float64``
is the reference the kernels are held to, ``np.float32`` the same arithmetic in the kernels' precision and order (the leg the
bar is measured from, never compared for equality).  Logits are ``[pixels, classes]`` (the valid lanes only), targets int64.

The SELECTION is exact integer work and is compared for equality: ``select`` sorts the confidences it is handed (``np.sort``)
-- the tests hand it the confidences the kernel wrote, so that a last-bit difference between two exponentials cannot move a
pixel across the threshold.
"""
import math

import numpy as np

from _loss_ref import F32, F64, UNDERFLOW, _a, _one_hot, _seqsum


def pixel_classes(t, classes, ignore_index, z=None):
    """(valid, void, invalid, nonfinite): void == ignore_index; invalid out of range; nonfinite valid with a non-finite row."""
    t = np.asarray(t)
    void = np.zeros(t.shape, dtype=bool) if ignore_index is None else t == ignore_index
    inr = (t >= 0) & (t < classes)
    invalid = ~void & ~inr
    valid = inr & ~void
    nonfinite = valid & ~np.isfinite(np.asarray(z)).all(1) if z is not None else np.zeros(t.shape, dtype=bool)
    return valid & ~nonfinite, void, invalid, nonfinite


def confidence(z, t, ignore_index, elem=F64):
    """(conf, mag): conf = exp(z_t - m) / S at the valid finite pixels, -1 elsewhere; m the row maximum, S = sum exp(z_c - m) with
    channel c in partial sum c % 4, folded (s0 + s1) + (s2 + s3).  mag: the probability itself plus UNDERFLOW."""
    z = np.asarray(z)
    pixels, classes = z.shape
    live, _, _, _ = pixel_classes(t, classes, ignore_index, z)
    conf = np.full(pixels, -1.0, dtype=elem)
    rows = np.nonzero(live)[0]
    x = z[rows].astype(elem)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m).astype(elem)
    part = [e[:, r::4].cumsum(1, dtype=elem)[:, -1] if e[:, r::4].shape[1] else np.zeros(len(rows), dtype=elem) for r in range(4)]
    s = ((part[0] + part[1]).astype(elem) + (part[2] + part[3]).astype(elem)).astype(elem)
    conf[rows] = (e[np.arange(len(rows)), np.asarray(t)[rows]] / s).astype(elem)
    mag = np.where(live, np.abs(conf.astype(F64)) + UNDERFLOW, 0.0)
    return conf, mag


def rank_k(n, min_kept=None, fraction=None):
    """k of the definition: min_kept, or ceil(fraction * n) in float64."""
    return int(min_kept) if fraction is None else int(math.ceil(float(fraction) * float(n)))


def kth_smallest(values, k):
    """The k-th smallest (1-indexed) of the values in [0, 2) as fp32; -inf for k == 0, +inf for k > n.  Also returns n."""
    v = np.asarray(values, dtype=F32).reshape(-1)
    bits = v.view(np.uint32)
    v = np.sort(v[bits < (1 << 30)])
    n = len(v)
    if k <= 0:
        return F32(-np.inf), n
    if k > n:
        return F32(np.inf), n
    return v[k - 1], n


def select(conf, thresh, min_kept=None, fraction=None):
    """The kept set of fp32 confidences (-1: not a candidate): keep iff conf >= 0 and (conf < thresh or conf <= q)."""
    conf = np.asarray(conf, dtype=F32)
    n = int((conf >= 0).sum())
    k = rank_k(n, min_kept, fraction)
    q, n2 = kth_smallest(conf, k)
    assert n2 == n
    keep = (conf >= 0) & ((conf < F32(thresh)) | (conf <= q))
    return {"keep": keep, "q": q, "n": n, "k": k}


def select_brute(conf, thresh, k):
    """The definition as a loop, for tests/test_ohem_host.py: q by counting, not sorting."""
    conf = [float(c) for c in np.asarray(conf, dtype=F32)]
    cand = [c for c in conf if c >= 0]
    q = -math.inf if k <= 0 else math.inf
    if 0 < k <= len(cand):
        for c in cand:                      # the smallest value with at least k candidates <= it
            if sum(1 for d in cand if d <= c) >= k and c < q:
                q = c
    return [c >= 0 and (c < float(F32(thresh)) or c <= q) for c in conf], q


def loss_and_grad(z, t, weight, keep, mean, elem=F64):
    """Cross entropy over the kept pixels: dict name -> (value, magnitude) for loss, grad [pixels, classes], colsum; and "denom".
    lse = mx + log(sum exp(z - mx)) summed left to right, l = w_t (lse - z_t), grad = a (exp(z - lse) - [c == t]), a = w_t / D."""
    z = np.asarray(z)
    pixels, classes = z.shape
    keep = np.asarray(keep, dtype=bool)
    t = np.where(keep, np.asarray(t), 0)
    w = np.ones(classes, dtype=F32) if weight is None else np.asarray(weight, dtype=F32)
    wt = np.where(keep, w[t], 0).astype(elem)
    denom = float(wt.astype(F64).sum())
    x = np.where(keep[:, None], z, 0).astype(elem)
    mx = x.max(1, keepdims=True)
    s = _seqsum(np.exp(x - mx), elem)[:, None]
    lse = (mx + np.log(s)).astype(elem)
    xt = x[np.arange(pixels), t]
    lp = (wt * (lse[:, 0] - xt).astype(elem)).astype(elem)
    mag_lp = _a(wt) * ((_a(mx) + _a(np.log(s)))[:, 0] + _a(xt))
    div = denom if mean else 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = elem(lp.astype(F64).sum() / div) if div != 0 else elem(np.nan)
        scale = elem(1.0 / div) if mean else elem(1.0)
    a = (scale * wt).astype(elem) if div != 0 else np.zeros(pixels, dtype=elem)
    e = np.exp(x - lse).astype(elem)
    oh = _one_hot(t, keep, classes)
    grad = (e * a[:, None] - oh.astype(elem) * a[:, None]).astype(elem)
    grad[~keep] = 0
    mag_grad = (e.astype(F64) + UNDERFLOW + oh) * _a(a)[:, None] * keep[:, None]
    if elem is F64:
        colsum = grad.sum(0)
    else:
        pad = (-pixels) % 256
        g = np.concatenate([grad, np.zeros((pad, classes), dtype=elem)]) if pad else grad
        colsum = g.reshape(-1, 256, classes).sum(1, dtype=F32).sum(0, dtype=F32)
    return {"loss": (loss, mag_lp.sum() / div if div != 0 else 0.0), "grad": (grad, mag_grad), "colsum": (colsum, mag_grad.sum(0)),
            "denom": denom}
