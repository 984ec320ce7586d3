"""numpy restatement of the output-space adaptation kernels (csrc/advent.hip: weighted self-information maps forward and backward,
entropy / maximum-squares loss with its gradient), in the manner of ``_loss_ref``, whose ``_seqsum``, ``UNDERFLOW``, ``PAD_JUNK``, ``f32``,
``Grader`` and the magnitude of ``log_softmax`` it reuses (the log probability itself is formed as the kernels form it, ``_rows_uncached``).

With s = 1 / log C, lp = log_softmax(z), p = exp(lp):

    I_c = p_c > 0 ? -s p_c lp_c : 0          H = sum_c I_c
    maps backward:   g_c = -s (lp_c + 1) dmaps_c,   dlogits_k = p_k (g_k - sum_c p_c g_c)
    entropy:         loss = sum_p H_p / P,          dlogits_k = -(s / P) p_k (lp_k + H_nat),  H_nat = -sum_c p_c lp_c
    max squares:     loss = -sum_p sum_c p_c^2 / (2 P),   dlogits_k = -(1 / P) p_k (p_k - sum_c p_c^2)

A lane whose probability is 0 (a -inf logit) contributes exactly 0 everywhere and has magnitude 0: nothing but 0 passes there.

The arithmetic is generic over ``elem``: ``np.float64`` is the reference (tests/test_advent_host.py proves it against torch's
double-precision autograd), ``np.float32`` follows the kernels' order of operations and is the leg the bar is measured from.  Every
function returns name -> (value, magnitude), the magnitude being the sum of the absolute values of the terms that formed the element:
s p (|x| + |mx| + |log s|) plus the underflow term for I_c; p_k (|g_k| + sum_c p_c |g_c|) with |g_c| = s (mag_lp_c + 1) |dmaps_c| for
the maps' gradient; sum |terms| / P for the losses.

The second half is the grading itself, written against a *backend* (the kernels on the GPU: tests/test_gpu_advent_grade.py; the
float32 leg, alone or with one of MUTATIONS: tests/test_advent_host.py): padded NHWC buffers whose pad lanes hold junk, outputs
pre-filled with NaN, pad lanes of every output exactly 0, the bar of tests/test_gpu_loss_grade.py.
"""
import numpy as np

from _loss_ref import F32, F64, PAD_JUNK, UNDERFLOW, Grader, _a, _chunksum, _seqsum, bf16_round, f32, log_softmax  # noqa: F401

MUTATIONS = ("pad_lane", "lp_plus_one", "log_ldc", "no_rowsum", "map_pad_unwritten", "tail_pixel")
KINDS = ("entropy", "max_squares")
BLOCKS, THREADS = 1024, 256                # udaseg_seg_partials() blocks of 256 pixels: beyond them a thread takes a second pixel


_ROWS = []                                 # the last few (z, key, result): one case asks for the same rows several times


def _rows(z, elem, mut, ldc):
    """(lp, p, s, mag_lp, live): mag_lp is 0 and live False in the lanes whose logit is -inf.  Read-only results."""
    key = (elem, mut if mut in ("pad_lane", "log_ldc") else None, ldc if mut == "log_ldc" else None)
    for z0, k0, out in _ROWS:
        if z0 is z and k0 == key:
            return out
    out = _rows_uncached(z, elem, mut, ldc)
    _ROWS.append((z, key, out))
    del _ROWS[:-4]
    return out


def _rows_uncached(z, elem, mut, ldc):
    """The kernels' row: d = x - mx, sm = sum exp(d) left to right, lp = d - log(sm), p = exp(lp).  The sum mx + log(sm) is never
    formed (``_loss_ref.log_softmax`` rounds it, which puts half an ulp of |lse| on every probability of the row); the magnitude of
    a log probability is ``log_softmax``'s: |x| + |mx| + |log sm|."""
    x = np.asarray(z).astype(elem)
    mx = x.max(1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - mx).astype(elem)
        sm = _seqsum(np.exp(d), elem)[:, None]
        if mut == "pad_lane":
            sm = (sm + np.exp(elem(PAD_JUNK) - mx)).astype(elem)
        lg = np.log(sm).astype(elem)
        lp = (d - lg).astype(elem)
    mag_lp = _a(x) + _a(mx) + _a(lg)
    p = np.exp(lp).astype(elem)
    s = (elem(1) / np.log(elem(ldc if mut == "log_ldc" else x.shape[1]))).astype(elem)
    live = np.isfinite(mag_lp)
    return lp, p, s, np.where(live, mag_lp, 0.0), live


def _info(lp, p, s, elem):
    with np.errstate(invalid="ignore"):
        t = (p * lp).astype(elem)
        return np.where(p > 0, -(s * t), elem(0)).astype(elem)


def self_information(z, elem=F64, mut=None, ldc=None):
    """maps [pixels, classes] = I_c, entropy [pixels] = H."""
    lp, p, s, mag_lp, live = _rows(z, elem, mut, ldc)
    info = _info(lp, p, s, elem)
    mag = np.where(live, float(s) * (p.astype(F64) + UNDERFLOW) * mag_lp, 0.0)
    return {"maps": (info, mag), "entropy": (_seqsum(info, elem), mag.sum(1))}


def self_information_bwd(z, dmaps, elem=F64, mut=None, ldc=None):
    """grad [pixels, classes] of the logits from dmaps [pixels, classes], the maps' gradient."""
    lp, p, s, mag_lp, live = _rows(z, elem, mut, ldc)
    dm = np.asarray(dmaps).astype(elem)
    one = elem(0) if mut == "lp_plus_one" else elem(1)
    with np.errstate(invalid="ignore"):
        g = np.where(p > 0, -(s * (lp + one)) * dm, elem(0)).astype(elem)
    big_s = _seqsum(p * g, elem)[:, None]
    if mut == "no_rowsum":
        big_s = big_s * elem(0)
    grad = np.where(p > 0, p * (g - big_s), elem(0)).astype(elem)
    pm = np.where(live, p.astype(F64) + UNDERFLOW, 0.0)
    mag_g = float(s) * (mag_lp + 1.0) * _a(dm) * live
    return {"grad": (grad, pm * (mag_g + (pm * mag_g).sum(1, keepdims=True)))}


def entropy_loss(z, kind, elem=F64, mut=None, ldc=None, counted=None):
    """loss, grad [pixels, classes] for an upstream gradient of 1, entropy [pixels].  ``counted``: the rows that reach the sum
    (None: all)."""
    lp, p, s, mag_lp, live = _rows(z, elem, mut, ldc)
    pixels = p.shape[0]
    info = _info(lp, p, s, elem)
    mag_i = np.where(live, float(s) * (p.astype(F64) + UNDERFLOW) * mag_lp, 0.0)
    h = _seqsum(info, elem)
    pm = np.where(live, p.astype(F64) + UNDERFLOW, 0.0)
    sel = slice(None) if counted is None else counted
    if kind == "entropy":
        loss = elem(h[sel].astype(F64).sum() / pixels)
        mag_loss = mag_i.sum() / pixels
        with np.errstate(invalid="ignore"):
            centre = _seqsum(np.where(p > 0, p * lp, elem(0)).astype(elem), elem)[:, None]
            coef = -(s / elem(pixels))
            grad = np.where(p > 0, coef * (p * (lp - centre)), elem(0)).astype(elem)
        mag_grad = abs(float(coef)) * pm * (mag_lp + (pm * mag_lp).sum(1, keepdims=True))
    else:
        q = _seqsum((p * p).astype(elem), elem)
        loss = elem(q[sel].astype(F64).sum() / (-2.0 * pixels))
        mag_loss = (p.astype(F64) ** 2).sum() / (2.0 * pixels)
        coef = -(elem(1) / elem(pixels))
        grad = np.where(p > 0, coef * (p * (p - q[:, None])), elem(0)).astype(elem)
        mag_grad = abs(float(coef)) * pm * (pm + (pm * pm).sum(1, keepdims=True))
    return {"loss": (loss, mag_loss), "grad": (grad, mag_grad), "entropy": (h, mag_i.sum(1))}


# ------------------------------------------------------------------------------------------------------------ cases and grading
CLASSES = (2, 5, 12, 23, 32)
SMALL_PIXELS = (1, 255, 257)
BIG_PIXELS = BLOCKS * THREADS + 3          # one thread takes a second grid-stride pixel
ROW_KINDS = ("random", "uniform", "saturated", "neg_inf")


def ceil_to(c, a):
    return (c + a - 1) // a * a


def make_logits(pixels, classes, seed, kind=None):
    """[pixels, classes] fp32: random at scale 3, with uniform / saturated (80 in one lane) / one-lane -inf rows mixed in (rows
    1, 2, 3 mod 7); ``kind`` makes every row of that kind."""
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((pixels, classes))).astype(F32)
    r = np.arange(pixels)
    lane = rng.integers(0, classes, pixels)
    pick = {k: (r % 7 == i + 1) if kind is None else np.full(pixels, kind == k) for i, k in enumerate(ROW_KINDS[1:])}
    z[pick["uniform"]] = z[pick["uniform"], :1]
    z[pick["saturated"], lane[pick["saturated"]]] = 80.0
    z[pick["neg_inf"], lane[pick["neg_inf"]]] = -np.inf
    return z


def embed(z, ldc):
    """The padded buffer [pixels, ldc]: pad lanes hold PAD_JUNK, one of them 1e30."""
    pixels, classes = z.shape
    buf = np.full((pixels, ldc), PAD_JUNK, dtype=F32)
    buf[:, :classes] = z
    if ldc > classes:
        buf[pixels // 2, ldc - 1] = 1e30
    return buf


class LegBackend:
    """The float32 leg in the kernels' place (optionally with one mutation), on the same padded buffers, NaN-prefilled outputs."""

    def __init__(self, mut=None):
        self.mut = mut

    def _covered(self, pixels):
        return min(pixels, BLOCKS * THREADS) if self.mut == "tail_pixel" else pixels

    def selfinfo_fwd(self, zbuf, classes, cpad, bf16, want_entropy):
        pixels, ldc = zbuf.shape
        out = self_information(zbuf[:, :classes], F32, self.mut, ldc)
        maps = np.full((pixels, cpad), np.nan, dtype=F32)
        n = self._covered(pixels)
        maps[:n] = 0
        maps[:n, :classes] = out["maps"][0][:n]
        if self.mut == "map_pad_unwritten" and cpad > classes:
            maps[:, cpad - 1] = np.nan
        ent = np.full(pixels, np.nan, dtype=F32)
        ent[:n] = out["entropy"][0][:n]
        return (bf16_round(maps) if bf16 else maps), (ent if want_entropy else None)

    def selfinfo_bwd(self, zbuf, dbuf, classes, bf16):
        pixels, ldc = zbuf.shape
        out = self_information_bwd(zbuf[:, :classes], dbuf[:, :classes], F32, self.mut, ldc)
        d = np.full((pixels, ldc), np.nan, dtype=F32)
        n = self._covered(pixels)
        d[:n] = 0
        d[:n, :classes] = out["grad"][0][:n]
        return d

    def entropy_loss(self, zbuf, classes, kind, want_grad, want_entropy):
        pixels, ldc = zbuf.shape
        n = self._covered(pixels)
        out = entropy_loss(zbuf[:, :classes], kind, F32, self.mut, ldc, counted=slice(0, n))
        d = np.full((pixels, ldc), np.nan, dtype=F32)
        d[:n] = 0
        d[:n, :classes] = out["grad"][0][:n]
        ent = np.full(pixels, np.nan, dtype=F32)
        ent[:n] = out["entropy"][0][:n]
        return F32(out["loss"][0]), (d if want_grad else None), (ent if want_entropy else None)


def grade_case(backend, pixels, classes, seed, log=print, row_kind=None, parts=("fwd", "bwd", "loss")):
    """One (pixels, classes) case through ``backend``: all three entry points, fp32 and bf16 maps, both loss kinds in both modes.
    Returns the Grader (``.done()`` asserts)."""
    ldc = ceil_to(classes, 4)
    z = make_logits(pixels, classes, seed, row_kind)
    zbuf = embed(z, ldc)
    g = Grader(f"advent px={pixels} C={classes}{'' if row_kind is None else ' ' + row_kind}", log)
    rng = np.random.default_rng(seed + 1)
    if "fwd" in parts:
        r64, r32 = self_information(z, F64), self_information(z, F32)
        for bf16 in (False, True):
            cpad, tag = ceil_to(classes, 8 if bf16 else 4), "bf16" if bf16 else "fp32"
            maps, ent = backend.selfinfo_fwd(zbuf, classes, cpad, bf16, True)
            g.grade(f"maps {tag}", maps[:, :classes], r64["maps"][0], r32["maps"][0], r64["maps"][1], bf16_out=bf16)
            g.zero(f"maps {tag} pad lanes", maps[:, classes:])
            g.grade(f"entropy ({tag} call)", ent, r64["entropy"][0], r32["entropy"][0], r64["entropy"][1])
            maps2, none = backend.selfinfo_fwd(zbuf, classes, cpad, bf16, False)
            g.exact(f"maps {tag} without entropy", maps2, maps)
            assert none is None
    if "bwd" in parts:
        for bf16 in (False, True):
            cpad, tag = ceil_to(classes, 8 if bf16 else 4), "bf16" if bf16 else "fp32"
            dm = rng.standard_normal((pixels, classes)).astype(F32)
            dm = bf16_round(dm) if bf16 else dm            # rounded once on the host: both legs and the kernel see the same numbers
            dbuf = embed(dm, cpad)
            r64, r32 = self_information_bwd(z, dm, F64), self_information_bwd(z, dm, F32)
            d = backend.selfinfo_bwd(zbuf, dbuf, classes, bf16)
            g.grade(f"dlogits from {tag} dmaps", d[:, :classes], r64["grad"][0], r32["grad"][0], r64["grad"][1])
            g.zero(f"dlogits from {tag} dmaps pad lanes", d[:, classes:])
    if "loss" in parts:
        for kind in KINDS:
            r64, r32 = entropy_loss(z, kind, F64), entropy_loss(z, kind, F32)
            loss, d, ent = backend.entropy_loss(zbuf, classes, kind, True, True)
            loss0, d0, ent0 = backend.entropy_loss(zbuf, classes, kind, False, False)
            assert d0 is None and ent0 is None
            g.grade(f"{kind} loss", loss, r64["loss"][0], r32["loss"][0], r64["loss"][1])
            g.exact(f"{kind} loss, loss-only call", np.asarray(loss0), np.asarray(loss))
            g.grade(f"{kind} dlogits", d[:, :classes], r64["grad"][0], r32["grad"][0], r64["grad"][1])
            g.zero(f"{kind} dlogits pad lanes", d[:, classes:])
            g.grade(f"{kind} entropy", ent, r64["entropy"][0], r32["entropy"][0], r64["entropy"][1])
    return g
