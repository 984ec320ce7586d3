"""Layer-local grading of one training step: every conv+BN+activation layer, the max pool and the head are graded element-wise
against float64 FROM THE ENGINE'S OWN INPUTS, forward and backward (tests/test_gpu_step_tape.py, tests/test_step_tape_host.py).

Host-only test infrastructure (numpy and torch on the CPU), in the manner of ``_conv_ref`` / ``_norm_ref``, whose references and bars
it uses: a check builds a ``_conv_ref.Ref`` (r64, magnitude, two fp32 legs) and is judged by the grader of the arithmetic its route
runs -- ``X3Grader`` for the fp32 split routes, ``F32Grader`` for the fp32 matrix pipe, ``Grader`` (truncating leg) for bf16 storage
-- with the one bar max(4 x the worse leg, 2^-22) of the magnitude.  The second leg takes the default step order (16 consecutive K
terms, no sign pattern).  The package is imported lazily and only for ``engine`` names.

What is graded are the values ``engine.Plan`` hands to and receives from its kernels in a REAL step: the route, the packed operand of
that route, an unwritten activation's scale / shift, the accumulate flags, the BatchNorm-backward sums made in another layer's
epilogue, the offsets into the gradient arena.  No ReLU mask and no pool winner is forced: both sides of a comparison start from the
same recorded input, so a flipped bit upstream moves them alike.

The Recorder wraps ``Plan.bn_bwd`` and ``Plan.conv_bwd`` for one ``loss.backward()`` and synchronises the device before and after
every wrapped call: IT SERIALISES THE TWO STREAMS (the weight gradients run on a side stream).  This grades values, not overlap.

Two places compare a quantity the kernels form from values BEFORE a bf16 store with the same quantity of the STORED values (the
only ones a recorder can see): the BatchNorm statistics made in a convolution's epilogue, and the BatchNorm-backward sums / the head's
bias gradient made in a producer's epilogue.  There (bf16 storage only) the deviation is first reduced by the rigorous bound of
that difference, sum_i half_ulp_bf16(v_i) |coefficient_i| -- the precision of the number format, not a measured figure.

The activation band: where the backward re-evaluates the activation's argument in fp32 instead of reading a written z (the z-less
fp32 forms and the LazyAct form), an element may take either branch only where the float64 argument lies within
max(4 x max|arg32 - arg64| over the layer, 2 ulp of fp32 at the layer's scale) of zero; at most BAND_CAP of a layer's elements may.
"""
import time

import numpy as np
import torch

import _conv_ref as R
import _norm_ref as N
from _grade import log as _log

F32, F64 = np.float32, np.float64
BAND_CAP = 1e-3
PREFIX = "step-tape"

# routes of the fp32 split pipe whatever the geometry; the shared launches (igemm, upcat, split, bnreduce, generic, part, bnin) take
# the split only above 32 channels on both sides
X3_FWD = ("stem", "frag", "frag_bnin", "frag_up_bnin", "phase", "n16")
X3_DGRAD = ("phase", "n16", "frag")
X3_WGRAD = ("halo",)


def arith(storage, direction, route, gathered, produced):
    """'bf16' | 'x3' | 'f32': the arithmetic a route runs.  gathered / produced: the channel counts of THIS direction's product."""
    if storage == "bf16":
        return "bf16"
    if route in {"fwd": X3_FWD, "dgrad": X3_DGRAD, "wgrad": X3_WGRAD}[direction]:
        return "x3"
    return "x3" if R.x3_shared_applicable(gathered, produced) else "f32"


def _mm(ar):
    return {"x3": R.x3_matmul, "f32": lambda A, B: R.rne_matmul(A, B, R.MFMA_32), "bf16": R.trunc_matmul}[ar]


def _less(got, ref, slack):
    """``got`` with its deviation from r64 reduced element-wise by ``slack`` (see the module docstring); None: as it is."""
    if slack is None or np.shape(got) != ref.r64.shape:
        return got
    dev = np.asarray(got, dtype=F64) - ref.r64
    return ref.r64 + np.sign(dev) * np.maximum(np.abs(dev) - slack, 0.0)


class _Tape:
    PREFIX = PREFIX


class _X3(_Tape, R.X3Grader):
    pass


class _F32(_Tape, R.F32Grader):
    pass


class _BF16(_Tape, R.Grader):
    pass


class _Norm(_Tape, R.Grader):
    """The BatchNorm / channel-sum checks: ONE fp32 leg, the same arithmetic in the kernels' precision (both legs of the Ref)."""
    LEG = "d_f32"


GRADERS = {"x3": _X3, "f32": _F32, "bf16": _BF16, "norm": _Norm}


class Report:
    """The verdicts of one case: every figure is logged (UDASEG_DEVIATION_LOG) before done() asserts; ``worst`` keeps the largest e/bar
    per check kind, ``failed`` the (layer, kind) pairs that missed."""

    def __init__(self, tag):
        self.tag, self.bad, self.failed, self.worst, self.band, self.t0 = tag, [], [], {}, {}, time.time()

    def _note(self, layer, kind, ratio, ok, text):
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)
        if not ok:
            self.failed.append((layer, kind))
            self.bad.append(text)

    def grade(self, ar, layer, kind, route, got, ref, bf16_out=False, slack=None):
        g, got = GRADERS[ar](self.tag, log=_log), _less(got, ref, slack)
        g.grade(f"{layer}:{kind}:{route}", got, ref, bf16_out)
        _, e, A, _, _, _ = R.verdict(got, ref, bf16_out)
        self._note(layer, kind, e / A, not g.bad, "; ".join(g.bad))

    def bound(self, layer, kind, err, allowed):
        """|err| <= allowed element-wise, the bound worked out by the caller from Refs' bars."""
        err, allowed = np.abs(np.asarray(err, dtype=F64)), np.asarray(allowed, dtype=F64)
        ratio = float(np.max(err / allowed)) if np.isfinite(err).all() and (allowed > 0).all() else float("inf")
        _log(f"{PREFIX} {self.tag} | {layer}:{kind} | e {float(err.max()):.3e} e/bar {ratio:.3f}")
        self._note(layer, kind, ratio, ratio <= 1.0, f"{layer}:{kind}: e/bar {ratio:.3f}")

    def exact(self, layer, kind, got, want):
        same = np.array_equal(np.asarray(got), np.asarray(want))
        _log(f"{PREFIX} {self.tag} | {layer}:{kind} | {'exact' if same else 'DIFFERS'}")
        self._note(layer, kind, 0.0 if same else float("inf"), same, f"{layer}:{kind}: not bit for bit")

    def share(self, layer, count, size):
        s = count / max(size, 1)
        self.band[layer] = s
        _log(f"{PREFIX} {self.tag} | {layer}:band | {count} of {size} elements ({s:.3e}), cap {BAND_CAP:g}")
        self._note(layer, "band", s / BAND_CAP, s <= BAND_CAP, f"{layer}:band: share {s:.3e} > {BAND_CAP:g}")

    def done(self):
        _log(f"{PREFIX} {self.tag} | time {time.time() - self.t0:.2f} s | worst e/bar " +
             " ".join(f"{k} {v:.3f}" for k, v in sorted(self.worst.items())))
        assert not self.bad, f"{self.tag}: " + "; ".join(b for b in self.bad if b)


# ------------------------------------------------------------------------------------------------------------------- the records
class Inp:
    """A convolution's input as the engine holds it: kind 'plain' (t), 'lazy' (y, scale, shift, act, slope: never written) or 'upcat'
    (a: a plain or lazy Inp at half resolution, skip: array or None)."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)


class Layer:
    """One convolution (+ BatchNorm + activation) of the forward.  Arrays are NHWC fp32 numpy with the PHYSICAL (padded) channel
    counts; w is the LOGICAL OHWI weight.  z None with ``lazy`` = (scale, shift): the activation was never written."""

    def __init__(self, **kw):
        self.bias = self.gamma = self.beta = self.z = self.lazy = self.mean = self.rstd = self.residual = None
        self.act, self.slope, self.eps, self.storage = N.NONE, 0.0, 1e-5, "fp32"
        self.__dict__.update(kw)

    @property
    def bf16(self):
        return self.storage == "bf16"


def act64(t, act, slope):
    return np.where(t < 0, t * slope, t) if act == N.LEAKY else t


def materialise(inp, bf16=False):
    """(x64, x32) of an input: an unwritten activation is re-evaluated in float64 for the reference and with ONE fp32 rounding of the
    fused multiply-add for the legs (rounded to the storage type under bf16 storage, as its consumer stages it)."""
    if inp.kind == "plain":
        return inp.t.astype(F64), inp.t.astype(F32)
    if inp.kind == "lazy":
        x64 = act64(inp.y.astype(F64) * inp.scale.astype(F64) + inp.shift.astype(F64), inp.act, inp.slope)
        x32 = R.bn_apply_f32(inp.y, inp.scale, inp.shift, inp.slope if inp.act == N.LEAKY else None)
        return x64, (N.bf16_round(x32) if bf16 else x32)
    a64, a32 = materialise(inp.a, bf16)
    return R.upcat(a64, None if inp.skip is None else inp.skip.astype(F64)), R.upcat(a32, inp.skip)


def phys_weight(L, cin_p, cout_p):
    """The logical weights laid into the physical [cout_p][k][k][cin_p] shape, pad lanes zero; bf16 storage: rounded to bf16."""
    w = np.zeros((cout_p, L.k, L.k, cin_p), dtype=F32)
    w[:L.w.shape[0], :, :, :L.w.shape[3]] = N.bf16_round(L.w) if L.bf16 else L.w
    return w


def _ref(op, ar, a64, a32, b, *geom):
    """A Ref of one of the three products; the float64 reference takes a64, the legs a32 (they differ for an unwritten input)."""
    t, i = {"fwd": (R.torch_fwd, R.im2col_fwd), "dgrad": (R.torch_dgrad, R.im2col_dgrad), "wgrad": (R.torch_wgrad, R.im2col_wgrad)}[op]
    return R.Ref(t(a64, b, *geom, torch.float64), t(np.abs(a64), np.abs(b), *geom, torch.float64), t(a32, b, *geom, torch.float32),
                 i(a32, b, *geom, _mm(ar)))


def _triple(r64, mag, r32):
    return R.Ref(r64, mag, r32, r32)


# ------------------------------------------------------------------------------------------------------------------- forward checks
def seq_sums(y2d):
    """Per channel (sum, sum of squares) of the stored values as two Refs, the legs sequential fp32 sums (``_conv_ref.stats_ref``)."""
    return R.stats_ref(R.Ref(y2d, np.abs(y2d), y2d, y2d))


def check_stats(rep, L):
    """mean / rstd against the float64 statistics of the engine's own y.  The bound is that of the two sums (their Refs' bars, the
    legs sequential fp32 sums) carried through var = s2 / P - mean^2 and rstd = (var + eps)^-1/2, plus 2 ulp of the fp32 store."""
    c = L.y.shape[-1]
    y = L.y.reshape(-1, c).astype(F64)
    p = y.shape[0]
    mean, var, rstd = N.stats(y, L.eps)
    s1, s2 = seq_sums(y)
    a1, a2 = R.bar(s1)[0] * s1.mag / p, R.bar(s2)[0] * s2.mag / p
    if L.bf16:       # the epilogue summed the values before their bf16 store
        h = N.bf16_half_ulp(y)
        a1 = a1 + h.sum(0) / p
        a2 = a2 + ((2.0 * np.abs(y) + h) * h).sum(0) / p
    dv = a2 + (2.0 * np.abs(mean) + a1) * a1
    rep.bound(L.name, "mean", L.mean.astype(F64) - mean, a1 + 2.0 * np.spacing(np.abs(mean).astype(F32)).astype(F64))
    lo = 1.0 / np.sqrt(np.maximum(var - dv, 0.0) + L.eps)
    rep.bound(L.name, "rstd", L.rstd.astype(F64) - rstd, (lo - rstd) + 2.0 * np.spacing(rstd.astype(F32)).astype(F64))


def coeffs(L, elem):
    return N._coeffs(L.gamma, L.beta, L.mean, L.rstd, elem, F32)


def check_forward(rep, L):
    """y, pad channels, statistics, scale / shift of an unwritten activation, z."""
    x64, x32 = materialise(L.x, L.bf16)
    cin_p, cout_p = x64.shape[-1], L.y.shape[-1]
    w = phys_weight(L, cin_p, cout_p)
    ar = arith(L.storage, "fwd", L.route, cin_p, cout_p)
    ref = _ref("fwd", ar, x64, x32, w, L.stride, L.pad)
    if L.bias is not None:
        ref = R.epilogue(ref, bias=np.pad(L.bias, (0, cout_p - L.bias.shape[0])))
    rep.grade(ar, L.name, "y", L.route, L.y, ref, L.bf16 and not getattr(L, "y_fp32", False))
    if cout_p > L.w.shape[0]:
        rep.exact(L.name, "y-pad", L.y[..., L.w.shape[0]:], np.zeros_like(L.y[..., L.w.shape[0]:]))
    if L.gamma is None:
        return
    check_stats(rep, L)
    if L.lazy is not None:
        (_, _, sc64, sh64), (m32, _, sc32, sh32) = coeffs(L, F64), coeffs(L, F32)
        rep.grade("norm", L.name, "scale", "-", L.lazy[0], _triple(sc64, np.abs(sc64), sc32))
        rep.grade("norm", L.name, "shift", "-", L.lazy[1], _triple(sh64, np.abs(L.beta.astype(F64)) + np.abs(m32.astype(F64) * sc64), sh32))
    if L.z is not None:
        y2, res = L.y.reshape(-1, cout_p), None if L.residual is None else L.residual.reshape(-1, cout_p)
        (z64, _, mag), (z32, _, _) = (N._apply(y2, *coeffs(L, e)[2:], res, L.act, L.slope, e) for e in (F64, F32))
        rep.grade("norm", L.name, "z", "-", L.z.reshape(-1, cout_p), _triple(z64, mag, z32), L.bf16)


def check_pool(rep, f1, pooled, pidx):
    """pooled is the 3x3 / stride 2 / pad 1 maximum of f1 bit for bit; every index (tap = ky * 3 + kx) points at an element that attains it."""
    n, h, w, c = f1.shape
    ho, wo = pooled.shape[1:3]
    xp = np.pad(f1, ((0, 0), (1, 2), (1, 2), (0, 0)), constant_values=-np.inf)
    taps = np.stack([xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] for ky in range(3) for kx in range(3)], axis=0)
    rep.exact("maxpool", "pooled", pooled, taps.max(0))
    idx = np.asarray(pidx).astype(np.int64)
    ok = (idx >= 0) & (idx < 9)
    at = np.take_along_axis(taps, np.clip(idx, 0, 8)[None], axis=0)[0]
    rep.exact("maxpool", "pidx", ok & (at == taps.max(0)), np.ones(idx.shape, dtype=bool))


# ------------------------------------------------------------------------------------------------------------------ backward checks
def bn_backward_from(dz, factor, y, mean, rstd, gamma, elem):
    """``_norm_ref.bn_backward`` with the saved statistics and the activation's derivative factor given (None: no activation)."""
    mean, rstd, scale, _ = N._coeffs(gamma, gamma, mean, rstd, elem, F32)
    y, g = np.asarray(y).astype(elem), np.asarray(dz).astype(elem)
    if factor is not None:
        g = (g * factor.astype(elem)).astype(elem)
    p = y.shape[0]
    xhat = ((y - mean) * rstd).astype(elem)
    dbeta, dgamma = g.sum(0, dtype=elem), (g * xhat).sum(0, dtype=elem)
    mg, mgx = (dbeta / elem(p)).astype(elem), (dgamma / elem(p)).astype(elem)
    dy = (scale * (g - mg - xhat * mgx)).astype(elem)
    a = lambda t: np.abs(np.asarray(t, dtype=F64))  # noqa: E731
    return {"dy": (dy, a(scale) * (a(g) + a(mg) + a(xhat.astype(F64) * mgx.astype(F64)))), "dres": (g, a(g)),
            "dgamma": (dgamma, (a(g) * (a(xhat) + a(rstd) * a(mean))).sum(0)), "dbeta": (dbeta, a(g).sum(0)),
            "xhat": xhat.astype(F64), "scale": np.asarray(scale, dtype=F64)}


def band_of(L):
    """(arg64, in-band mask) of a layer whose backward re-evaluates the activation's argument from y: with the unwritten activation's
    scale / shift, else with gamma rstd and beta - mean gamma rstd formed in fp32."""
    c = L.y.shape[-1]
    y = L.y.reshape(-1, c)
    sc, sh = L.lazy if L.lazy is not None else coeffs(L, F32)[2:]
    arg64 = y.astype(F64) * sc.astype(F64) + sh.astype(F64)
    arg32 = R.bn_apply_f32(y, sc, sh, None).astype(F64)
    tol = max(4.0 * float(np.abs(arg32 - arg64).max()), 2.0 ** -22 * float(np.abs(arg64).max()))
    return arg64, arg32, np.abs(arg64) <= tol


def check_bn_bwd(rep, L, call):
    """dy, dgamma, dbeta, dres (+ old contents) of one Plan.bn_bwd call."""
    c = L.y.shape[-1]
    y, dz, got_dy = L.y.reshape(-1, c), call["dz"].reshape(-1, c), call["dy"].reshape(-1, c)
    slope = F64(F32(L.slope))
    factor = None
    if L.act == N.LEAKY and call["mask"] == "z":
        assert L.z is not None, f"{L.name}: the call read a z the forward never wrote"
        factor = np.where(L.z.reshape(-1, c) > 0, 1.0, slope)
    elif L.act == N.LEAKY:
        arg64, arg32, band = band_of(L)
        rep.share(L.name, int(band.sum()), band.size)
        factor = np.where(arg64 > 0, 1.0, slope)
        if band.any():                  # inside the band either branch: the one that explains the element's own dy
            factor[band] = np.where(arg32 > 0, 1.0, slope)[band]
            first = bn_backward_from(dz, factor, y, L.mean, L.rstd, L.gamma, F64)
            sc, xh, g0 = first["scale"], first["xhat"], dz.astype(F64)
            mg, mgx = first["dbeta"][0] / y.shape[0], first["dgamma"][0] / y.shape[0]
            cand = [np.abs(got_dy - sc * (g0 * m - mg - xh * mgx)) for m in (1.0, slope)]
            factor[band] = np.where(cand[0] <= cand[1], 1.0, slope)[band]
    r64, r32 = (bn_backward_from(dz, factor, y, L.mean, L.rstd, L.gamma, e) for e in (F64, F32))
    sb = sg = None
    if L.bf16 and call["fused"]:        # the sums were made from the gradient before its bf16 store
        h = N.bf16_half_ulp(dz) * (1.0 if factor is None else np.abs(factor))
        sb, sg = h.sum(0), (h * np.abs(r64["xhat"])).sum(0)
    p = y.shape[0]
    s_dy = None if sb is None else np.abs(r64["scale"]) * (sb + np.abs(r64["xhat"]) * sg) / p
    rep.grade("norm", L.name, "dy", call["mask"], got_dy, _triple(r64["dy"][0], r64["dy"][1], r32["dy"][0]), L.bf16, s_dy)
    rep.grade("norm", L.name, "dgamma", call["mask"], call["dgamma"][:c], _triple(*r64["dgamma"], r32["dgamma"][0]), False, sg)
    rep.grade("norm", L.name, "dbeta", call["mask"], call["dbeta"][:c], _triple(*r64["dbeta"], r32["dbeta"][0]), False, sb)
    if call["dres"] is not None:
        ref = _triple(*r64["dres"], r32["dres"][0])
        if call["dres_old"] is not None:
            ref = R.epilogue(ref, old=call["dres_old"].reshape(-1, c))
        rep.grade("norm", L.name, "dres", call["mask"], call["dres"].reshape(-1, c), ref, L.bf16)


def _pool_ref(ref):
    """The 2x2 sum-pool of a Ref (the gradient of nearest_x2): float64 sums, magnitudes summed, the legs summed in fp32."""
    p32 = lambda v: (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]).astype(F32) + v[:, 1::2, 0::2]).astype(F32) + v[:, 1::2, 1::2]).astype(F32)  # noqa: E731
    return R.Ref(R.pool2(ref.r64), R.pool2(ref.mag), p32(ref.leg_rne), p32(ref.leg_trunc))


def _cut(ref, lo, hi):
    return R.Ref(ref.r64[..., lo:hi], ref.mag[..., lo:hi], ref.leg_rne[..., lo:hi], ref.leg_trunc[..., lo:hi])


def check_conv_bwd(rep, L, call):
    """Weight gradient (logical region, pad lanes, old arena contents), dbias, and the data gradient in the form the call wrote it."""
    x64, x32 = materialise(L.x, L.bf16)
    dy = call["dy"]
    cin_p, cout_p = x64.shape[-1], dy.shape[-1]
    w = phys_weight(L, cin_p, cout_p)
    co, ci = L.w.shape[0], L.w.shape[3]
    ar = arith(L.storage, "wgrad", call["wgrad_route"], cin_p, cout_p)
    if call["wgrad_route"] == "bnin" and not L.bf16:
        ar = "f32" if max(cin_p, cout_p) <= 32 else "x3"           # the small-channel direct kernel / the halo-resident split kernel
    ref = _ref("wgrad", ar, x64, x32, dy, L.k, L.stride, L.pad)
    rep.exact(L.name, "gw-old", call["gw_old"], np.zeros_like(call["gw_old"]))
    rep.grade(ar, L.name, "wgrad", call["wgrad_route"], call["gw"], ref)
    lanes = np.ones(call["gw"].shape, dtype=bool)
    lanes[:co, :, :, :ci] = False
    rep.exact(L.name, "gw-pad", call["gw"][lanes], np.zeros(int(lanes.sum()), dtype=call["gw"].dtype))
    if L.bias is not None:
        d2 = dy.reshape(-1, cout_p)
        (b64, mag), (b32, _) = N.channel_sum(d2, F64), N.channel_sum(d2, F32)
        rep.exact(L.name, "gb-old", call["gb_old"], np.zeros_like(call["gb_old"]))
        rep.grade("norm", L.name, "dbias", "-", call["gb"][:cout_p], _triple(b64, mag, b32), False,
                  N.bf16_half_ulp(d2).sum(0) if L.bf16 else None)
    if call["dx_kind"] is None:
        return
    n, hi, wi, _ = x64.shape
    route = call["dgrad_route"]
    ar = arith(L.storage, "dgrad", route, cout_p, cin_p)
    ref = _ref("dgrad", ar, dy.astype(F64), dy, w, L.stride, L.pad, hi, wi)
    if call["dx_kind"] == "plain":
        if call["dx_old"] is not None:
            ref = R.epilogue(ref, old=call["dx_old"])
        rep.grade(ar, L.name, "dx", route, call["dx"], ref, L.bf16)
        return
    ca = L.x.a.y.shape[-1] if L.x.a.kind == "lazy" else L.x.a.t.shape[-1]
    if call["dx_kind"] == "pair":
        rep.grade(ar, L.name, "d_up", route, call["d_up"], _cut(ref, 0, ca), L.bf16)
    else:
        da = _pool_ref(_cut(ref, 0, ca))
        if call["da_old"] is not None:
            da = R.epilogue(da, old=call["da_old"])
        rep.grade(ar, L.name, "da", route, call["da"], da, L.bf16)
    if call["d_skip"] is not None:
        rep.grade(ar, L.name, "d_skip", route, call["d_skip"], _cut(ref, ca, cin_p), L.bf16)


def check_step(rep, tape, only=None):
    """Every forward and backward check of a recorded step {"layers": {name: Layer}, "pool": (f1, pooled, pidx) or None, "calls": [...]}
    (``only``: a predicate on layer names, the section of a parametrised case)."""
    keep = only or (lambda name: True)
    for L in tape["layers"].values():
        if keep(L.name):
            check_forward(rep, L)
    if tape.get("pool") is not None and keep("maxpool"):
        check_pool(rep, *tape["pool"])
    seen = {}
    for call in tape["calls"]:
        if keep(call["layer"]):
            L = tape["layers"][call["layer"]]
            seen[(call["layer"], call["kind"])] = seen.get((call["layer"], call["kind"]), 0) + 1
            (check_bn_bwd if call["kind"] == "bn" else check_conv_bwd)(rep, L, call)
    for L in tape["layers"].values():            # every conv is visited once, every BatchNorm once
        if keep(L.name):
            want = {"conv": 1, "bn": 0 if L.gamma is None else 1}
            got = {k: seen.get((L.name, k), 0) for k in want}
            rep._note(L.name, "visits", 0.0, got == want, f"{L.name}: backward calls {got}, expected {want}")


def census(tape):
    """{layer: (forward route, data-gradient route taken, weight-gradient route)}"""
    out = {}
    for call in tape["calls"]:
        if call["kind"] == "conv":
            dg = (call["dgrad_route"] or "-") + ("+bn" if call.get("bn_fused") else "")       # +bn: BatchNorm-backward sums ride along
            out[call["layer"]] = (tape["layers"][call["layer"]].route, dg, call["wgrad_route"])
    return out


def routes_visited(tape):
    c = census(tape).values()
    return {"fwd": sorted({r[0] for r in c}), "dgrad": sorted({r[1] for r in c}), "wgrad": sorted({r[2] for r in c})}


# ----------------------------------------------------------------------------------------------------- the recorder (GPU side)
def to_host(t):
    return None if t is None else t.detach().float().cpu().numpy().copy()


class Recorder:
    """Wraps Plan.bn_bwd / Plan.conv_bwd (and, to learn the data-gradient route ACTUALLY taken and whether the BatchNorm backward read
    a z, the engine's kernel entry points of those two families) through ``monkeypatch`` for one backward pass."""
    DGRAD = {"conv2d_dgrad_up": "phase", "conv2d_dgrad_n16": "n16", "conv2d_dgrad_frag": "frag", "conv2d_dgrad_bnreduce": "bnreduce",
             "conv2d_dgrad_split": "split", "conv2d_dgrad": "igemm"}

    def __init__(self, engine, monkeypatch, values=True):
        """values False: routes only, nothing is copied and nothing synchronised (the census of a full-size step)."""
        self.E, self.calls, self._dg, self._mask = engine, [], [], None
        E, rec = engine, self
        sync = torch.cuda.synchronize if values else (lambda: None)
        host = self._h = to_host if values else (lambda t: None)
        bn_orig, conv_orig = E.Plan.bn_bwd, E.Plan.conv_bwd

        def bn_bwd(P, bn, y, z, ms, dz, act, slope, dres=None, dres_acc=False, has_res=True):
            sync()
            call = {"kind": "bn", "key": y, "dz": host(dz), "dres_old": host(dres) if dres is not None and dres_acc else None,
                    "fused": id(y) in P._bnb}
            rec._mask = None
            out = bn_orig(P, bn, y, z, ms, dz, act, slope, dres, dres_acc, has_res)
            sync()
            call.update(dy=host(dz), dres=host(dres), dgamma=host(P.gvec(bn, "weight")), dbeta=host(P.gvec(bn, "bias")), mask=rec._mask)
            rec.calls.append(call)
            return out

        def conv_bwd(P, conv, d, x, dy, dx=None, dx_acc=False, dbias=None, prev=None):
            sync()
            up = isinstance(dx, E.UpGrad)
            call = {"kind": "conv", "key": conv, "dy": host(dy), "gw_old": host(P.gw(conv)),
                    "gb_old": host(P.gvec(conv, "bias")) if conv.bias is not None else None,
                    "dx_kind": None if dx is None else "upgrad" if up else "pair" if isinstance(dx, tuple) else "plain",
                    "dx_old": host(dx) if dx_acc and torch.is_tensor(dx) else None, "da_old": host(dx.da) if up and dx.acc else None}
            rec._dg = []
            conv_orig(P, conv, d, x, dy, dx, dx_acc, dbias, prev)
            sync()
            call.update(gw=host(P.gw(conv)), gb=host(P.gvec(conv, "bias")) if conv.bias is not None else None,
                        wgrad_route=P.wgrad_route(d, x), dgrad_route=rec._dg[0][0] if rec._dg else None,
                        bn_fused=any(f for _, f in rec._dg), d_skip=None)
            if up:
                call.update(da=host(dx.da), d_skip=host(dx.d_skip))
            elif isinstance(dx, tuple):
                call.update(d_up=host(dx[0]), d_skip=host(dx[1]) if isinstance(x, E.UpCat) and x.skip is not None else None)
            elif dx is not None:
                call["dx"] = host(dx)
            rec.calls.append(call)

        monkeypatch.setattr(E.Plan, "bn_bwd", bn_bwd)
        monkeypatch.setattr(E.Plan, "conv_bwd", conv_bwd)
        for name, route in self.DGRAD.items():
            monkeypatch.setattr(E.K, name, self._noting(getattr(E.K, name), route))
        apply_orig, rec_orig = E.K.bn_bwd_apply, E.K.bn_bwd_apply_recompute

        def bn_bwd_apply(dz, z, y, *a, **kw):
            act = a[8] if len(a) > 8 else kw.get("act")
            rec._mask = "none" if act == N.NONE else "recompute" if z is None else "z"
            return apply_orig(dz, z, y, *a, **kw)

        def bn_bwd_apply_recompute(*a, **kw):
            rec._mask = "recompute"
            return rec_orig(*a, **kw)

        monkeypatch.setattr(E.K, "bn_bwd_apply", bn_bwd_apply)
        monkeypatch.setattr(E.K, "bn_bwd_apply_recompute", bn_bwd_apply_recompute)

    def _noting(self, fn, route):
        def wrapped(*a, **kw):
            bn = kw.get("bn")
            self._dg.append((route, route == "bnreduce" or bn is not None))
            return fn(*a, **kw)
        return wrapped

    def tape(self, net, logits):
        """The recorded step: the layers from ``net._last_tape`` (debug_keep_tape) and ``net.state_dict()``, the calls named by layer.
        logits: what the forward returned (the [N, classes, H, W] view of the padded NHWC buffer)."""
        E, host = self.E, self._h
        P, blocks, (r_stem, f1, pooled, pidx), (head, d_head, h_last), _ = net._last_tape
        sd = {k: host(v) for k, v in net.state_dict().items()}
        names = {id(m): n for n, m in net.named_modules()}
        storage = "bf16" if P.bf16 else "fp32"

        def inp(x):
            if isinstance(x, E.UpCat):
                return Inp("upcat", a=inp(x.a), skip=host(x.skip))
            if isinstance(x, E.LazyAct):
                return Inp("lazy", y=host(x.y), scale=host(x.scale), shift=host(x.shift), act=x.act, slope=x.slope)
            return Inp("plain", t=host(x))

        def conv_fields(conv):
            nm = names[id(conv)]
            return dict(name=nm, k=conv.k, stride=conv.stride, pad=conv.pad, w=None if sd[nm + ".weight"] is None else np.ascontiguousarray(sd[nm + ".weight"].transpose(0, 2, 3, 1)),
                        bias=sd[nm + ".bias"] if conv.bias is not None else None, storage=storage)

        layers, by_y, by_conv = {}, {}, {}
        recs = [(r_stem, None)]
        for blk, rec, _ in blocks:
            first = next(i for i, e in enumerate(rec) if isinstance(e, E.ConvRecord))
            recs += [(r, rec[first - 1] if r.has_res else None) for r in rec if isinstance(r, E.ConvRecord)]
        for r, res in recs:
            bn = names[id(r.bn)]
            lazy = isinstance(r.z, E.LazyAct)
            L = Layer(x=inp(r.x), y=host(r.y), z=None if lazy else host(r.z), lazy=(host(r.z.scale), host(r.z.shift)) if lazy else None,
                      mean=host(r.mean), rstd=host(r.rstd), gamma=sd[bn + ".weight"], beta=sd[bn + ".bias"], eps=r.bn.eps, act=r.act,
                      slope=r.slope, residual=host(res), route=r.route, **conv_fields(r.conv))
            layers[L.name] = L
            by_y[id(r.y)], by_conv[id(r.conv)] = L.name, L.name
        calls = []
        for call in self.calls:
            call = dict(call)
            key = call.pop("key")
            if call["kind"] == "conv" and key is head:
                hx = inp(h_last)
                d = d_head
                route, _ = P.fwd_route(head, d, h_last, (E.FRAG_BNIN, E.FRAG, E.IGEMM))
                n, _, hh, ww = logits.shape
                y = host(logits.detach().as_strided((n, hh, ww, head.cout_p), (hh * ww * head.cout_p, ww * head.cout_p, head.cout_p, 1),
                                                    logits.storage_offset()))
                L = Layer(x=hx, y=y, route=route, y_fp32=True, **conv_fields(head))
                layers[L.name] = L
                call["layer"] = L.name
            else:
                call["layer"] = (by_conv if call["kind"] == "conv" else by_y)[id(key)]
            calls.append(call)
        return {"layers": layers, "pool": (host(f1), host(pooled), host(pidx)), "calls": calls}
