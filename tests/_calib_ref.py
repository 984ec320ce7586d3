"""numpy restatement of the calibration kernels (csrc/calib.hip): the winner's confidence at a reciprocal temperature ``beta``, its
bin, the reliability tables and their finishing arithmetic, the NLL sums with their derivatives in ``beta``, the guarded Newton
step and the fit trajectory.

Test infrastructure in the manner of ``_loss_ref``: the arithmetic is written once, generically over the float type ``elem`` --
``np.float64`` is the reference the kernels are held to (tests/test_calibration_host.py proves its derivatives against torch's
double-precision autograd), ``np.float32`` the same arithmetic in the kernels' precision and ORDER of operations (shift by the
winner's score, scale by beta, exp, four partial sums by channel % 4, ``(s0 + s1) + (s2 + s3)``): the leg the bars are measured
from, never compared for equality.  Scores are ``[pixels, classes]`` (the valid lanes only), targets int64 ``[pixels]``.

Sums come with their MAGNITUDE, the sum of the absolute values of the terms that formed them; errors are judged relative to it.
"""
import numpy as np

from _loss_ref import F32, F64
from _scores_ref import first_max

Q_ONE = 16777216.0                         # conf_q: the confidence in 2^-24 fixed point
BETA_MIN, BETA_MAX, REL_STEP = 1.0 / 64.0, 64.0, 4.0


def _sum4(x, elem):
    """Sum over the class axis as the kernels': channel c adds into partial sum c % 4 in channel order, then (s0 + s1) + (s2 + s3)."""
    p, c = x.shape
    s = np.zeros((p, 4), dtype=elem)
    for k in range(c):
        s[:, k % 4] = (s[:, k % 4] + x[:, k]).astype(elem)
    return ((s[:, 0] + s[:, 1]).astype(elem) + (s[:, 2] + s[:, 3]).astype(elem)).astype(elem)


def _shifted(z, elem):
    """(c^, d): the winner by the one tie rule and d_j = z_j - z[c^] in ``elem``."""
    z = np.asarray(z)
    cls = first_max(z)
    x = z.astype(elem)
    with np.errstate(invalid="ignore"):
        d = (x - x[np.arange(len(x)), cls][:, None]).astype(elem)
    return cls, d


def confidence(z, beta=1.0, elem=F64, probs=False):
    """(c^, p, finite).  Logits: p = 1 / sum_j exp((z_j - m) * beta).  ``probs``: p = the winner's value, finite only without a NaN
    in the row and with p in [0, 1].  A pixel whose p is not a finite number in [0, 1] is not finite."""
    z = np.asarray(z)
    if probs:
        cls = first_max(z)
        p = z[np.arange(len(z)), cls].astype(elem)
        with np.errstate(invalid="ignore"):
            fin = ~np.isnan(z).any(axis=1) & (p >= 0) & (p <= 1)
        return cls, p, fin
    cls, d = _shifted(z, elem)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = _sum4(np.exp((d * elem(beta)).astype(elem)).astype(elem), elem)
        p = (elem(1) / s).astype(elem)
        fin = np.isfinite(p) & (p >= 0) & (p <= 1)
    return cls, p, fin


def bin_index(p, bins, elem=F64):
    """min(floor(p * bins), bins - 1) with the product in ``elem``."""
    return np.minimum(np.floor((np.asarray(p).astype(elem) * elem(bins)).astype(elem)).astype(np.int64), bins - 1)


def tables(z, t, bins, beta=1.0, elem=F64, probs=False):
    """(tables int64 [3, C, B], counters int64 [3], info): count / correct / conf_q by predicted class and bin over the pixels with a
    target in [0, C) and a finite confidence; counters = in the tables, void, non-finite.  info: dict with ``cls``, ``p`` and ``used``
    (the mask of the pixels in the tables)."""
    z, t = np.asarray(z), np.asarray(t).reshape(-1)
    c = z.shape[1]
    cls, p, fin = confidence(z, beta, elem, probs)
    valid = (t >= 0) & (t < c)
    used = valid & fin
    tab = np.zeros((3, c, bins), dtype=np.int64)
    b = bin_index(np.where(used, p, 0), bins, elem)
    q = np.rint(np.where(used, p, 0).astype(elem) * elem(Q_ONE)).astype(np.int64)       # exact product: a power of two
    np.add.at(tab[0], (cls[used], b[used]), 1)
    np.add.at(tab[1], (cls[used], b[used]), (cls[used] == t[used]).astype(np.int64))
    np.add.at(tab[2], (cls[used], b[used]), q[used])
    counters = np.array([used.sum(), (~valid).sum(), (valid & ~fin).sum()], dtype=np.int64)
    return tab, counters, {"cls": cls, "p": p, "used": used}


def near_edge_counts(p, cls, classes, bins, delta):
    """[C, B] int64: per predicted class, the number of confidences within ``delta`` of bin b's lower edge b / bins."""
    p = np.asarray(p, dtype=F64)
    out = np.zeros((classes, bins), dtype=np.int64)
    k = np.rint(p * bins).astype(np.int64)                       # the nearest edge
    near = (np.abs(p - k / float(bins)) <= delta) & (k >= 0) & (k < bins)
    np.add.at(out, (np.asarray(cls)[near], k[near]), 1)
    return out


def finish(tab):
    """(out [6], per_class [4, C]) in float64 from integer tables, the order of udaseg_calib_finish: N, accuracy, mean confidence,
    ECE, MCE, gap; n_c, acc_c, conf_c, ece_c.  NaN where the denominator is 0."""
    tab = np.asarray(tab).astype(np.int64)
    nan = float("nan")
    n_b, a_b, q_b = (tab[k].sum(axis=0) for k in range(3))
    N, A, Q = int(n_b.sum()), int(a_b.sum()), int(q_b.sum())
    e, mce = 0.0, nan
    for b in range(tab.shape[2]):
        ab, qb = float(a_b[b]), float(q_b[b]) / Q_ONE
        e += abs(ab - qb)
        if n_b[b]:
            g = abs(ab / float(n_b[b]) - qb / float(n_b[b]))
            if not mce >= g:
                mce = g
    acc = A / float(N) if N else nan
    conf = float(Q) / Q_ONE / float(N) if N else nan
    out = np.array([float(N), acc, conf, e / float(N) if N else nan, mce, conf - acc])
    pc = np.full((4, tab.shape[1]), nan)
    for c in range(tab.shape[1]):
        n = int(tab[0, c].sum())
        pc[0, c] = float(n)
        if n:
            pc[1, c] = float(tab[1, c].sum()) / n
            pc[2, c] = float(tab[2, c].sum()) / Q_ONE / n
            ec = 0.0
            for b in range(tab.shape[2]):
                ec += abs(float(tab[1, c, b]) - float(tab[2, c, b]) / Q_ONE)
            pc[3, c] = ec / n
    return out, pc


def nll_terms(z, t, beta=1.0, elem=F64):
    """Per pixel in ``elem``: (terms [P, 3] = nll, g1, g2; magnitudes [P, 3] float64; counted [P] bool; valid [P] bool).
    d_j = z_j - m, e_j = exp(beta d_j), S = sum e_j:  nll = log S - beta d_t,  mu = sum e_j d_j / S,  g1 = mu - d_t,
    g2 = sum e_j d_j^2 / S - mu^2.  A pixel is counted when its target is in [0, C) and its three terms are finite."""
    z, t = np.asarray(z), np.asarray(t).reshape(-1)
    c = z.shape[1]
    valid = (t >= 0) & (t < c)
    _, d = _shifted(z, elem)
    beta = elem(beta)
    with np.errstate(all="ignore"):
        e = np.exp((beta * d).astype(elem)).astype(elem)
        ed = (e * d).astype(elem)
        s, a, b = _sum4(e, elem), _sum4(ed, elem), _sum4((ed * d).astype(elem), elem)
        dt = d[np.arange(len(d)), np.where(valid, t, 0)]
        logs = np.log(s).astype(elem)
        nll = (logs - (beta * dt).astype(elem)).astype(elem)
        mu = (a / s).astype(elem)
        g1 = (mu - dt).astype(elem)
        bs, mm = (b / s).astype(elem), (mu * mu).astype(elem)
        g2 = (bs - mm).astype(elem)
        terms = np.stack([nll, g1, g2], axis=1)
        mag = np.stack([np.abs(logs.astype(F64)) + float(beta) * np.abs(dt.astype(F64)),
                        np.abs(mu.astype(F64)) + np.abs(dt.astype(F64)),
                        np.abs(bs.astype(F64)) + np.abs(mm.astype(F64))], axis=1)
        counted = valid & np.isfinite(terms).all(axis=1)
    return terms, mag, counted, valid


def nll_sums(z, t, beta=1.0, elem=F64):
    """(sums [4] float64 = n, sum nll, sum g1, sum g2; magnitudes [4]; counters [3] = counted, void, non-finite).  The per-pixel
    terms are ``elem``, every sum over the pixels is float64 (as the kernel's)."""
    terms, mag, counted, valid = nll_terms(z, t, beta, elem)
    n = float(counted.sum())
    sums = np.concatenate([[n], terms[counted].astype(F64).sum(axis=0)])
    mags = np.concatenate([[n], mag[counted].sum(axis=0)])
    counters = np.array([counted.sum(), (~valid).sum(), (valid & ~counted).sum()], dtype=np.int64)
    return sums, mags, counters


def step(sums, beta, store=F32):
    """udaseg_calib_step in IEEE float64, operation by operation.  ``beta``: the value before (``store`` = np.float32: what the
    device holds; np.float64 for the unrounded reference trajectory).  Returns (beta', state [4] without the step counter's
    history: mean nll, mean g1, beta' - beta, 1)."""
    n, l, g1, g2 = (float(v) for v in sums)
    beta = float(store(beta))
    out = beta
    ok = (n > 0.0 and all(np.isfinite(v) for v in (n, l, g1, g2)) and g2 > 0.0 and beta > 0.0 and np.isfinite(beta))
    if ok:
        with np.errstate(all="ignore"):
            bn = float(np.float64(beta) - np.float64(g1) / np.float64(g2))
        bn = min(max(bn, beta / REL_STEP), REL_STEP * beta)
        bn = min(max(bn, BETA_MIN), BETA_MAX)
        out = float(store(bn))
    nan = float("nan")
    return out, np.array([l / n if n > 0.0 else nan, g1 / n if n > 0.0 else nan, out - beta, 1.0])


def fit(z, t, iters=8, elem=F64, beta0=1.0):
    """The trajectory [beta_0, ..., beta_iters] of ``iters`` x (nll_sums, step).  The float32 leg holds beta as fp32 (the device's),
    the float64 leg unrounded."""
    store = F32 if elem is F32 else F64
    traj = [float(store(beta0))]
    for _ in range(iters):
        sums, _, _ = nll_sums(z, t, traj[-1], elem)
        traj.append(step(sums, traj[-1], store)[0])
    return traj


def seeded_input(n, c, h, w, seed, block=8, invalid=0):
    """The recipe of tests/test_gpu_curves.py's seeded inputs: targets constant on block x block squares, logits 1.5 * randn plus
    12 * rand on the target's channel; ``invalid`` pixels get targets of -1 and c + 200.  Returns numpy ([N,C,H,W] fp32, [N,H,W])."""
    import torch
    g = torch.Generator().manual_seed(seed)
    tb = torch.randint(0, c, (n, h // block, w // block), generator=g)
    target = tb.repeat_interleave(block, 1).repeat_interleave(block, 2).contiguous()
    z = 1.5 * torch.randn(n, c, h, w, generator=g)
    z.scatter_add_(1, target[:, None], 12.0 * torch.rand(n, 1, h, w, generator=g))
    if invalid:
        idx = torch.randperm(target.numel(), generator=g)[:invalid]
        target.view(-1)[idx[::2]] = -1
        target.view(-1)[idx[1::2]] = c + 200
    return z.numpy(), target.numpy()


CASES = {"c5": (2, 5, 48, 40, 5, 60), "c23": (2, 23, 64, 64, 23, 50), "c32": (2, 32, 32, 48, 32, 40)}   # n, c, h, w, seed, invalid


def case(name):
    n, c, h, w, seed, invalid = CASES[name]
    return seeded_input(n, c, h, w, seed, invalid=invalid)


def flat(logits, target):
    """[N, C, H, W] logits and [N, H, W] targets -> ([pixels, C], [pixels]) in the kernels' pixel order."""
    logits, target = np.asarray(logits), np.asarray(target)
    return np.ascontiguousarray(np.moveaxis(logits, 1, -1)).reshape(-1, logits.shape[1]), target.reshape(-1)
