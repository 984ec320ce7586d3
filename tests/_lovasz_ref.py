"""numpy mirror of the Lovasz-softmax loss on a grid of error bins (csrc/lovasz.hip; the definition stands in include/udaseg.h).

Test infrastructure, in the manner of ``_ohem_ref``: the arithmetic is written once over the float type ``elem`` -- ``np.float64``
is the reference the kernels are held to, ``np.float32`` the same arithmetic in the kernels' precision and order (the leg the bar
is measured from, never compared for equality).  Logits are ``[pixels, classes]`` (the valid lanes only), targets int64.

The TABLES are integer work and are compared for equality.  That needs the fp32 bin of every error to equal the float64 bin:
``make_inputs`` resamples every row with an error within MARGIN of a bin edge, and tests/test_lovasz_host.py asserts that none is
left.  ``exact_lovasz`` is the sort-based loss of the paper (Berman, Rannen Triki, Blaschko 2018, Algorithm 1 / eq. 9), written
from the paper in float64.

The second half of the file holds the GPU cases (shapes, bins, the input maker), so that the host file can state their
preconditions without a GPU.
"""
import numpy as np
import torch

from _loss_ref import F32, F64, UNDERFLOW, _a
from _ohem_ref import pixel_classes

MARGIN = 2.0 ** -16                      # several times the worst fp32 error of a 32-class softmax probability


# ------------------------------------------------------------------------------------------------------------------- errors
def softmax_rows(z, live, elem=F64):
    """(p, m, S) of the live rows (zeros / ones elsewhere): m the row maximum, S = sum exp(z_c - m) with channel c in partial sum
    c % 4, folded (s0 + s1) + (s2 + s3), p = exp(z - m) / S."""
    z = np.asarray(z)
    x = np.where(np.asarray(live)[:, None], z, 0).astype(elem)
    m = x.max(1, keepdims=True)
    ex = np.exp((x - m).astype(elem)).astype(elem)
    part = [ex[:, r::4].cumsum(1, dtype=elem)[:, -1] if ex[:, r::4].shape[1] else np.zeros(len(x), dtype=elem) for r in range(4)]
    s = ((part[0] + part[1]).astype(elem) + (part[2] + part[3]).astype(elem)).astype(elem)[:, None]
    return (ex / s).astype(elem), m[:, 0], s[:, 0]


def errors(rows, targets, ignore_index=None, elem=F64):
    """(e, fg, live, p): e[i, c] = 1 - p_c where targets[i] == c and p_c elsewhere, in ``elem``; fg the one-hot map; live the valid
    finite pixels (every other row of e, fg and p is 0)."""
    rows = np.asarray(rows)
    pixels, classes = rows.shape
    t = np.asarray(targets)
    live, _, _, _ = pixel_classes(t, classes, ignore_index, rows)
    p, _, _ = softmax_rows(rows, live, elem)
    fg = np.zeros((pixels, classes), dtype=bool)
    fg[np.nonzero(live)[0], t[live]] = True
    e = np.where(fg, (elem(1) - p).astype(elem), p).astype(elem)
    e[~live] = 0
    p = np.where(live[:, None], p, 0).astype(elem)
    return e, fg, live, p


def bin_of(e, B):
    """min(B - 1, floor(e * B)); e * B is exact in either precision (B is a power of two)."""
    return np.minimum(B - 1, np.floor(np.asarray(e) * B).astype(np.int64))


def groups_of(pixels, images):
    """The group of every pixel: image i holds pixels [i * pixels / images, (i + 1) * pixels / images)."""
    assert pixels % images == 0
    return np.arange(pixels) // (pixels // images)


def tables(e, fg, B, live=None, images=1):
    """int64 [images, classes, 2, B]: row 0 the fg pixels of every bin, row 1 the bg pixels, over the live pixels."""
    e = np.asarray(e)
    pixels, classes = e.shape
    live = np.ones(pixels, dtype=bool) if live is None else np.asarray(live)
    g = groups_of(pixels, images)
    b = bin_of(e, B)
    out = np.zeros((images, classes, 2, B), dtype=np.int64)
    for c in range(classes):
        np.add.at(out, (g[live], c, np.where(fg[live, c], 0, 1), b[live, c]), 1)
    return out


# ------------------------------------------------------------------------------------------------------------- coefficients
def bin_weights(pos, neg):
    """(wf, wb) [B] in float64 of one (group, class) by the closed forms; bins walked from the top."""
    pos, neg = np.asarray(pos, dtype=F64), np.asarray(neg, dtype=F64)
    G = pos.sum()
    a0 = np.concatenate([[0.0], np.cumsum(pos[::-1])[:-1]])[::-1]       # fg strictly above the bin
    b0 = np.concatenate([[0.0], np.cumsum(neg[::-1])[:-1]])[::-1]
    if G > 0:
        d0, d1 = G + b0, G + b0 + neg
        return 0.5 * (1.0 / d0 + 1.0 / d1), (G - a0 - 0.5 * pos) / (d0 * d1)
    wb = np.zeros_like(neg)
    top = np.nonzero(neg)[0]
    if len(top):
        wb[top[-1]] = 1.0 / neg[top[-1]]
    return np.zeros_like(pos), wb


def jaccard(G, a, b):
    """J(a, b) = 1 - (G - a) / (G + b) after a fg and b bg pixels; J(0, 0) := 0."""
    return 0.0 if a == 0 and b == 0 else 1.0 - (G - a) / (G + b)


def bin_weights_naive(pos, neg):
    """The same weights from the definition: inside a bin the increments of J are added up pixel by pixel in the order "fg
    first" and in the order "bg first"; an fg (bg) pixel's weight is the average over the two orders of the fg (bg) total / count."""
    B = len(pos)
    G = int(np.sum(pos))
    wf, wb = np.zeros(B), np.zeros(B)
    a0 = b0 = 0
    for b in range(B - 1, -1, -1):
        p, n = int(pos[b]), int(neg[b])
        tot = {"f": 0.0, "b": 0.0}
        for order in ("fb", "bf"):
            a, bb = a0, b0
            for kind in order:
                for _ in range(p if kind == "f" else n):
                    j0 = jaccard(G, a, bb)
                    a, bb = (a + 1, bb) if kind == "f" else (a, bb + 1)
                    tot[kind] += jaccard(G, a, bb) - j0
        if p:
            wf[b] = tot["f"] / (2 * p)
        if n:
            wb[b] = tot["b"] / (2 * n)
        a0, b0 = a0 + p, b0 + n
    return wf, wb


def coefficients(tab, classes_mode="present"):
    """From integer tables [images, classes, 2, B]: dict with coef (float64, the tables' shape, the reduction factor folded in),
    present [images, classes], slack [classes] (float64, summed over the groups) and factor [images, classes]."""
    tab = np.asarray(tab)
    images, classes, _, B = tab.shape
    present = tab[:, :, 0, :].sum(-1) > 0
    coef = np.zeros(tab.shape, dtype=F64)
    factor = np.zeros((images, classes))
    slack = np.zeros(classes)
    for g in range(images):
        npres = int(present[g].sum())
        for c in range(classes):
            if classes_mode == "all":
                f = 1.0 / (images * classes)
            else:
                f = 1.0 / (images * npres) if present[g, c] else 0.0
            wf, wb = bin_weights(tab[g, c, 0], tab[g, c, 1])
            coef[g, c, 0], coef[g, c, 1] = f * wf, f * wb
            factor[g, c] = f
            p, n = tab[g, c, 0].astype(F64), tab[g, c, 1].astype(F64)
            tied = p + n >= 2
            slack[c] += f * float((p * wf + n * wb)[tied].sum()) / B
    return {"coef": coef, "present": present, "slack": slack, "factor": factor}


# ---------------------------------------------------------------------------------------------------------- loss and gradient
def loss_and_grad(rows, targets, ignore_index, coef, ce_weight=0.0, elem=F64, lovasz=True):
    """The grid loss and its gradient given coefficient tables [images, classes, 2, B] (float64; the float32 leg rounds them):
    dict name -> (value, magnitude) for loss, grad [pixels, classes], colsum.  ``lovasz=False`` leaves the Lovasz term out (the
    cross-entropy term alone), ``ce_weight`` adds ce_weight * mean over the live pixels of (log S - (z_t - m))."""
    rows = np.asarray(rows)
    pixels, classes = rows.shape
    coef = np.asarray(coef)
    images, _, _, B = coef.shape
    t = np.asarray(targets)
    e, fg, live, p = errors(rows, t, ignore_index, elem)
    _, m, S = softmax_rows(rows, live, elem)
    g = groups_of(pixels, images)
    cidx = np.arange(classes)[None, :]
    w = coef.astype(elem)[g[:, None], cidx, np.where(fg, 0, 1), bin_of(e, B)]
    w = np.where(live[:, None], w, 0).astype(elem) * elem(1 if lovasz else 0)
    ew = (e * w).astype(elem)
    lpx = np.cumsum(ew, axis=1, dtype=elem)[:, -1]
    d = np.where(fg, -w, w).astype(elem)
    pd = (p * d).astype(elem)
    dot = np.cumsum(pd, axis=1, dtype=elem)[:, -1:]
    grad = (p * (d - dot).astype(elem)).astype(elem)
    pm = p.astype(F64) + UNDERFLOW * live[:, None]
    mag_grad = pm * (_a(d) + _a(pd).sum(1, keepdims=True))
    loss, mag_loss = float(lpx.astype(F64).sum()), float(_a(ew).sum())
    if ce_weight != 0.0:
        n = int(live.sum())
        if n == 0:
            loss, s = float("nan"), elem(0)
        else:
            s = elem(F64(F32(ce_weight)) / n)
            tt = np.where(live, t, 0)
            zt = np.where(live, rows[np.arange(pixels), tt], 0).astype(elem)
            logs = np.log(S).astype(elem)
            nll = (s * (logs - (zt - m).astype(elem)).astype(elem)).astype(elem) * live
            loss += float(nll.astype(F64).sum())
            mag_loss += float((_a(s) * (_a(logs) + _a(zt) + _a(m)) * live).sum())
            grad = (grad + (s * (p - fg.astype(elem)).astype(elem)).astype(elem)).astype(elem)
            mag_grad = mag_grad + _a(s) * (pm + fg) * live[:, None]
    grad[~live] = 0
    if elem is F64:
        colsum = grad.sum(0)
    else:
        pad = (-pixels) % 256
        gg = np.concatenate([grad, np.zeros((pad, classes), dtype=elem)]) if pad else grad
        colsum = gg.reshape(-1, 256, classes).sum(1, dtype=F32).sum(0, dtype=F32)
    return {"loss": (elem(loss), mag_loss), "grad": (grad, mag_grad), "colsum": (colsum, mag_grad.sum(0))}


def grid_loss(e, fg, B, live=None, images=1, classes_mode="present"):
    """(L_B, sum of slack, coefficient dict) straight from errors: tables, coefficients, sum e * w."""
    e = np.asarray(e, dtype=F64)
    pixels, classes = e.shape
    live = np.ones(pixels, dtype=bool) if live is None else np.asarray(live)
    co = coefficients(tables(e, fg, B, live, images), classes_mode)
    g = groups_of(pixels, images)
    w = co["coef"][g[:, None], np.arange(classes)[None, :], np.where(fg, 0, 1), bin_of(e, B)]
    return float((e * w)[live].sum()), float(co["slack"].sum()), co


# ------------------------------------------------------------------------------------------------------- the paper's loss
def lovasz_1d(e, fg):
    """The Lovasz extension of the Jaccard loss of one class over one group: errors sorted in descending order, the k-th weighted
    with J_k - J_{k-1}, J_k = 1 - (G - fg seen) / (G + bg seen).  0 for an empty group."""
    e, fg = np.asarray(e, dtype=F64), np.asarray(fg, dtype=bool)
    if len(e) == 0:
        return 0.0
    order = np.argsort(-e, kind="stable")
    es, fs = e[order], fg[order]
    G = float(fs.sum())
    a, b = np.cumsum(fs), np.cumsum(~fs)
    J = 1.0 - (G - a) / (G + b)
    return float((es * np.diff(np.concatenate([[0.0], J]))).sum())


def exact_lovasz(rows, targets, ignore_index=None, images=1, classes_mode="present"):
    """The sort-based Lovasz-softmax loss in float64 with this project's reductions: per group the mean over the present (or
    all) classes, 0 for a group with none; then the mean over the groups."""
    e, fg, live, _ = errors(rows, targets, ignore_index, F64)
    pixels, classes = e.shape
    g = groups_of(pixels, images)
    total = 0.0
    for i in range(images):
        sel = live & (g == i)
        vals = [lovasz_1d(e[sel, c], fg[sel, c]) for c in range(classes) if classes_mode == "all" or fg[sel, c].any()]
        total += sum(vals) / len(vals) if vals else 0.0
    return total / images


# ---------------------------------------------------------------------------------------------------------- the GPU cases
IGN = 255
# shape -> bins
CASES = {(1, 3, 8, 8): 4096,             # "distinct": no bin holds two pixels
         (2, 5, 9, 7): 64,               # "tied": under one chunk, ldc 8, class 1 absent from image 1 only
         (2, 23, 37, 41): 1024,          # ldc 24, three class groups of the histogram pass
         (1, 32, 16, 16): 256,           # no pad lane
         (1, 5, 513, 512): 256}          # the grid-stride loops of both passes run twice
DISTINCT, TIED = (1, 3, 8, 8), (2, 5, 9, 7)
_INPUTS = {}


def nhwc_rows(z):
    n, c, h, w = z.shape
    return z.permute(0, 2, 3, 1).reshape(-1, c).numpy()


def violations(rows, t, B, images, distinct):
    """Rows (live ones only) with a float64 error within MARGIN of a bin edge k / B, 0 < k < B; for the distinct case also every
    later occupant of a bin that already holds a pixel of the same (group, class)."""
    e, fg, live, _ = errors(rows, t, IGN, F64)
    x = e * B
    k = np.rint(x)
    near = (np.abs(x - k) < MARGIN * B) & (k > 0) & (k < B)
    bad = live & near.any(1)
    if distinct:
        b = bin_of(e, B)
        g = groups_of(len(rows), images)
        for c in range(rows.shape[1]):
            seen = set()
            for i in np.nonzero(live & ~bad)[0]:
                key = (g[i], b[i, c])
                if key in seen:
                    bad[i] = True
                seen.add(key)
    return bad


def make_inputs(shape):
    """(z [N,C,H,W] fp32, t [N,H,W] int64): logits 3 * randn; the target is the argmax at 70 % of the pixels and random elsewhere;
    10 % void (255), a few targets out of range, one row with an inf.  Class C - 1 occurs in no target (an absent class), in TIED
    class 1 is also taken out of image 1.  Rows that violate a precondition of the integer comparison are drawn again."""
    if shape in _INPUTS:
        return _INPUTS[shape]
    n, c, h, w = shape
    B = CASES[shape]
    gen = torch.Generator().manual_seed(90 + list(CASES).index(shape))
    z = torch.randn(n, c, h, w, generator=gen) * 3.0
    t = z.argmax(1)
    r = torch.rand(n, h, w, generator=gen)
    t = torch.where(r < 0.3, torch.randint(0, c, (n, h, w), generator=gen), t)
    t[t == c - 1] = 0
    if shape == TIED:
        t[1][t[1] == 1] = 2
    r = torch.rand(n, h, w, generator=gen)
    t[r < 0.10] = IGN
    t[(r >= 0.10) & (r < 0.12)] = c
    t[(r >= 0.12) & (r < 0.13)] = -3
    zf = z.permute(0, 2, 3, 1).reshape(-1, c).contiguous()
    tf = t.reshape(-1).numpy()
    for _ in range(200):
        bad = violations(zf.numpy(), tf, B, 1, shape == DISTINCT)
        if not bad.any():
            break
        zf[torch.from_numpy(bad)] = torch.randn(int(bad.sum()), c, generator=gen) * 3.0
    live = ((t.view(-1) >= 0) & (t.view(-1) < c)).nonzero()[:, 0]
    px = int(live[len(live) // 2])                           # a pixel with a valid target gets an inf: non-finite
    zf[px, (int(tf[px]) + 1) % c] = float("inf")
    z = zf.reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    _INPUTS[shape] = (z, t)
    return _INPUTS[shape]


def modes(shape):
    """(images, classes mode) combinations of a shape: per_image off and on where N > 1, 'present' and 'all'."""
    return [(i, m) for i in sorted({1, shape[0]}) for m in ("present", "all")]
