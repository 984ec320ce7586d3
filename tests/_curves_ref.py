"""Float64 numpy restatement of the score, the grid and the tables of the curves module (the definition in
``uda_aerial_semantic_segmentation_research_amd/curves.py``): what the HIP kernel is held to.  No torch, no GPU."""
import numpy as np

SCORE_BINS = 2048
SCORE_RANGE = 16.0


def scores(logits):
    """[N,C,H,W] logits -> [N*H*W, C] float64 log-odds s_c = z_c - log(sum_{j != c} exp(z_j)), without cancellation."""
    z = np.asarray(logits, dtype=np.float64)
    n, c, h, w = z.shape
    z = z.transpose(0, 2, 3, 1).reshape(-1, c)
    am = z.argmax(axis=1)
    zm = z - z[np.arange(len(z)), am][:, None]
    e = np.exp(zm)
    S = e.sum(axis=1)
    e_wo = e.copy()
    e_wo[np.arange(len(z)), am] = 0.0
    Sp = e_wo.sum(axis=1)
    others = S[:, None] - e
    others[np.arange(len(z)), am] = Sp
    with np.errstate(divide="ignore"):
        return zm - np.log(others)


def bin_index(s, bins=SCORE_BINS, score_range=SCORE_RANGE):
    x = np.floor((s + score_range) * (bins / (2.0 * score_range)))
    return np.clip(x, 0, bins - 1).astype(np.int64)


def tables(logits, target, bins=SCORE_BINS, score_range=SCORE_RANGE):
    """(pos, neg): [C, bins] int64; targets outside [0, C) are left out."""
    s = scores(logits)
    c = s.shape[1]
    t = np.asarray(target).reshape(-1)
    valid = (t >= 0) & (t < c)
    b = bin_index(s, bins, score_range)
    pos = np.zeros((c, bins), dtype=np.int64)
    neg = np.zeros((c, bins), dtype=np.int64)
    for k in range(c):
        pos[k] = np.bincount(b[valid & (t == k), k], minlength=bins)
        neg[k] = np.bincount(b[valid & (t != k), k], minlength=bins)
    return pos, neg


def edges(bins=SCORE_BINS, score_range=SCORE_RANGE):
    """Lower edge of every bin as a score."""
    return -score_range + np.arange(bins, dtype=np.float64) * (2.0 * score_range / bins)


def near_edge_counts(s_class, delta, bins=SCORE_BINS, score_range=SCORE_RANGE):
    """For one class's scores: number of scores within delta of each bin's lower edge (0 for edge 0, which nothing crosses)."""
    e = edges(bins, score_range)
    srt = np.sort(s_class)
    out = np.searchsorted(srt, e + delta, side="right") - np.searchsorted(srt, e - delta, side="left")
    out[0] = 0
    return out.astype(np.int64)


def sharp_case(seed=7, n=2, c=23, h=64, w=64):
    """The seeded sharper case of the fixture's recipe: targets constant on 8 x 8 blocks, logits 1.5 * randn plus 12 * rand on the
    target's channel, one logit raised by 40 on a handful of pixels (the upper end bin), rounded to multiples of 1/256 and
    returned as int16 (exact in fp32) with the int64 targets."""
    rng = np.random.default_rng(seed)
    tb = rng.integers(0, c, size=(n, h // 8, w // 8))
    target = np.repeat(np.repeat(tb, 8, axis=1), 8, axis=2).astype(np.int64)
    z = 1.5 * rng.standard_normal((n, c, h, w))
    boost = 12.0 * rng.random((n, h, w))
    nn, hh, ww = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    z[nn, target, hh, ww] += boost
    for i in range(12):
        z[i % n, int(target[i % n, 5 * i % h, 3 * i % w]), 5 * i % h, 3 * i % w] += 40.0
    q = np.clip(np.round(z * 256.0), -32768, 32767).astype(np.int16)
    return q, target
