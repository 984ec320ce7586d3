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

The discriminators (tests/test_gpu_disc_tape.py, tests/test_disc_tape_host.py) run on the same Plan and add what the segmenter's step
never does.  Their checks: a convolution's fused activation (Layer.fused_act), check_act_bwd, check_tail (both pooled tails, judged
as tests/test_gpu_loss_grade.py judges the kernels), the pad lanes of an input gradient, check_eval_layer (the folded eval plan,
bn_fold judged as tests/test_gpu_conv_f32_grade.py judges it), check_grad_sum (k delivered arenas) and check_running (judged as
tests/test_gpu_norm_grade.py judges the two outputs).  Recorder.watch wraps a discriminator's ``_forward_plan``; every recorded call
carries the Plan it ran under, so two forwards followed by one backward come apart again (image_tape / feature_tape / eval_tape).
"""
import time

import numpy as np
import torch

import _conv_ref as R
import _loss_ref as LR
import _norm_ref as N
from _grade import Grader as _NormGrader, log as _log

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

    def tail(self, layer, kind, got, r64, r32, mag, bf16_out=False):
        """tests/_loss_ref.py's Grader as tests/test_gpu_loss_grade.py uses it: its margin, its floor."""
        g = LR.Grader(self.tag, lambda line: _log(f"{PREFIX} {line}"))
        g.grade(f"{layer}:{kind}", got, r64, r32, mag, bf16_out)
        self._note(layer, kind, g.worst, not g.bad, "; ".join(g.bad))

    def fold(self, layer, what, got, r64, leg, mag):
        """tests/test_gpu_conv_f32_grade.py::test_bn_fold's verdict: the norm bar of the fp32 restatement of the same formula."""
        A, dleg = N.bar(leg, r64, mag)
        got = np.asarray(got, dtype=F64)
        e = float(N.normalised(got - r64, mag).max(initial=0.0)) if got.shape == np.shape(r64) and np.isfinite(got).all() else float("inf")
        _log(f"{PREFIX} {self.tag} | {layer}:fold:{what} | fp32 | e {e:.3e} d_rne {dleg:.3e} bar {A:.3e} e/bar {e / A:.3f}")
        self._note(layer, "fold", e / A, e <= A, f"{layer}:fold:{what}: e {e:.3e} > bar {A:.3e}")

    def ulp2(self, layer, kind, got, r64, operand, slack=None):
        """tests/_grade.py's Grader.ulp2 as tests/test_gpu_norm_grade.py applies it to running_mean / running_var; ``slack`` as in _less."""
        if slack is not None:
            dev = np.asarray(got, dtype=F64) - r64
            got = r64 + np.sign(dev) * np.maximum(np.abs(dev) - slack, 0.0)
        g = _NormGrader(self.tag)
        g.PREFIX = PREFIX
        g.ulp2(f"{layer}:{kind}", got, r64, operand)
        ulp = np.spacing(np.maximum(np.abs(r64), operand).astype(F32)).astype(F64)
        err = np.abs(np.asarray(got, dtype=F64) - r64) / ulp
        self._note(layer, kind, float(err.max(initial=0.0)) / 2.0 if np.isfinite(err).all() else float("inf"), not g.bad, "; ".join(g.bad))

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
    counts; w is the LOGICAL OHWI weight.  z None with ``lazy`` = (scale, shift): the activation was never written.  ``fused_act`` /
    ``fused_slope``: a convolution without BatchNorm whose stored y is act(conv + bias), the pre-activation never written."""

    def __init__(self, **kw):
        self.bias = self.gamma = self.beta = self.z = self.lazy = self.mean = self.rstd = self.residual = self.fused_act = None
        self.fused_slope = 0.0
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


def stats_bound(y, eps, bf16):
    """(mean, var, rstd, a1, dv) of y [pixels, channels]: the float64 statistics and how far the kernels' mean / variance may lie from
    them -- the bars of the two sums' Refs (the legs sequential fp32 sums) over P, carried through var = s2 / P - mean^2; bf16 storage:
    plus what the values lost in their bf16 store, since the epilogue summed them before it."""
    y = np.asarray(y, dtype=F64)
    p = y.shape[0]
    mean, var, rstd = N.stats(y, eps)
    s1, s2 = seq_sums(y)
    a1, a2 = R.bar(s1)[0] * s1.mag / p, R.bar(s2)[0] * s2.mag / p
    if bf16:
        h = N.bf16_half_ulp(y)
        a1 = a1 + h.sum(0) / p
        a2 = a2 + ((2.0 * np.abs(y) + h) * h).sum(0) / p
    return mean, var, rstd, a1, a2 + (2.0 * np.abs(mean) + a1) * a1


def check_stats(rep, L):
    """mean / rstd against the float64 statistics of the engine's own y.  The bound is that of the two sums (stats_bound) carried through
    rstd = (var + eps)^-1/2, plus 2 ulp of the fp32 store."""
    c = L.y.shape[-1]
    mean, var, rstd, a1, dv = stats_bound(L.y.reshape(-1, c), L.eps, L.bf16)
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
    bias = None if L.bias is None else np.pad(L.bias, (0, cout_p - L.bias.shape[0]))
    if L.fused_act == N.LEAKY:           # the stored output is act(conv + bias); LeakyReLU is 1-Lipschitz: the same bar, no band
        ref = R.epilogue(ref, bias=bias, slope=float(F32(L.fused_slope)))
    elif bias is not None:
        ref = R.epilogue(ref, bias=bias)
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
        if ci < cin_p:                  # the input's pad lanes meet zero weights: no gradient may appear in them
            rep.exact(L.name, "dx-pad", call["dx"][..., ci:], np.zeros_like(call["dx"][..., ci:]))
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


def check_act_bwd(rep, L, call):
    """The in-place act_bwd through a convolution's fused activation: dz * act'(stored output), one fp32 product per element, bit for
    bit (rounded once to bf16 under bf16 storage)."""
    want = N.act_bwd(call["dz"], L.y, L.fused_act, L.fused_slope, F32)[0]
    rep.exact(L.name, "act-bwd", call["dy"], N.bf16_round(want) if L.bf16 else want)


def check_tail(rep, t):
    """A pooled tail (global average pool -> dot product (-> sigmoid)) as the plan wired it, judged as tests/test_gpu_loss_grade.py
    judges the same kernels.  t: layer, sigmoid, bf16, z [n, h, w, c], w [c], b, pooled [n, c], out [n]; with a backward also dp [n],
    dz [n, h, w, c], gw [c], gb, gw_old, gb_old; the feature-level tail also block / block_old: the [rows][c] gradient block of the 1x1
    convolution whose row 0 is gw."""
    name, sig = t["layer"], t["sigmoid"]
    n, c = t["pooled"].shape
    z = t["z"].reshape(n, -1, c)
    hw = z.shape[1]
    f64, f32 = (LR.tail_forward(z, t["w"], t["b"], sig, e) for e in (F64, F32))
    for key, got in (("pooled", t["pooled"]), ("out", np.reshape(t["out"], -1))):
        rep.tail(name, key, got, f64[key][0], f32[key][0], f64[key][1])
    if t.get("dp") is None:
        return
    b64, b32 = (LR.tail_backward(t["dp"], np.reshape(t["out"], -1), t["pooled"], t["w"], hw, sig, e) for e in (F64, F32))
    spread = lambda a: np.repeat(np.asarray(a)[:, None, :], hw, axis=1)  # noqa: E731
    rep.tail(name, "dz", t["dz"].reshape(n, hw, c), spread(b64["dz"][0]), spread(b32["dz"][0]), spread(b64["dz"][1]), t["bf16"])
    rep.exact(name, "dw-old", t["gw_old"], np.zeros_like(t["gw_old"]))
    rep.exact(name, "db-old", t["gb_old"], np.zeros_like(t["gb_old"]))
    rep.tail(name, "dw", t["gw"], b64["dw"][0], b32["dw"][0], b64["dw"][1])
    rep.tail(name, "db", t["gb"], b64["db"][0], b32["db"][0], b64["db"][1])
    if t.get("block") is not None:
        block = t["block"].reshape(t["block"].shape[0], -1)
        rep.exact(name, "block-old", t["block_old"], np.zeros_like(t["block_old"]))
        rep.exact(name, "dw-rows", block[1:], np.zeros_like(block[1:]))
        rep.exact(name, "dw-row0", block[0], t["gw"])


def check_eval_layer(rep, ev):
    """One Plan._conv_bn_act_eval call from the operands the engine itself used.  ev: layer, storage, x (Inp), k, stride, pad, w32 (the
    physical fp32 weights), bias, gamma, beta, rm, rv, eps, wf / bf (the folded slices the call wrote), wf16 (their cast, bf16 storage),
    z, act, slope, residual."""
    name, bf16 = ev["layer"], ev["storage"] == "bf16"
    c = ev["gamma"].shape[0]
    bias = None if ev["bias"] is None else ev["bias"][:c]
    args = (ev["w32"][:c], bias, ev["gamma"], ev["beta"], ev["rm"], ev["rv"], ev["eps"])
    (w64, b64, bmag), (w32, b32, _) = R.bn_fold_ref(*args, F64), R.bn_fold_ref(*args, F32)
    rep.fold(name, "weights", ev["wf"][:c], w64, w32, np.abs(w64))
    rep.fold(name, "bias", ev["bf"][:c], b64, b32, bmag)
    stored = ev["wf"]
    if bf16:
        rep.exact(name, "fold-bf16", ev["wf16"], N.bf16_round(ev["wf"]))
        stored = ev["wf16"]
    x64, x32 = materialise(ev["x"], bf16)
    cin_p, cout_p = x64.shape[-1], ev["z"].shape[-1]
    ar = arith(ev["storage"], "fwd", "igemm", cin_p, cout_p)
    ref = _ref("fwd", ar, x64, x32, stored, ev["stride"], ev["pad"])
    ref = R.epilogue(ref, bias=np.pad(ev["bf"][:c], (0, cout_p - c)), residual=ev["residual"],
                     slope=float(F32(ev["slope"])) if ev["act"] == N.LEAKY else None)
    rep.grade(ar, name, "z-eval", "igemm", ev["z"], ref, bf16)


def check_grad_sum(rep, name, delivered, arena):
    """After a backward that delivered k arenas the module's gradient arena is their fp32 sum in delivery order, bit for bit."""
    want = np.asarray(delivered[0], dtype=F32)
    for d in delivered[1:]:
        want = (want + np.asarray(d, dtype=F32)).astype(F32)
    rep.exact(name, "grad-sum", arena, want)


def check_running(rep, r):
    """running_mean / running_var of one BatchNorm after its training forwards: ``_norm_ref.running`` applied in forward order to the
    float64 statistics of each forward's recorded y, judged as tests/test_gpu_norm_grade.py judges the two (2 ulp of fp32 at the larger
    operand); num_batches_tracked counts the forwards.  r: layer, ys, eps, momentum, bf16, rm0 / rv0 / nbt0 (before), rm / rv / nbt.
    That grade feeds the kernel float64 sums of the stored values.  The plan's statistics are made in the convolution's epilogue: what
    check_stats allows the saved mean and the variance for it (stats_bound: the sums' own bars, under bf16 storage also the values'
    bf16 store), carried through the same recurrence, is taken off the deviation first, as _less does."""
    name, mom = r["layer"], float(F32(r["momentum"]))
    rm, rv = r["rm0"].astype(F64), r["rv0"].astype(F64)
    sm = sv = op_m = op_v = np.zeros_like(rm)
    for y in r["ys"]:
        y2 = y.reshape(-1, y.shape[-1])[:, :rm.shape[0]]
        p = y2.shape[0]
        mean, var, _, a1, dv = stats_bound(y2, r["eps"], r["bf16"])
        rm, rv, op_m, op_v = N.running(mean, var, p, mom, rm, rv)
        sm, sv = (1.0 - mom) * sm + mom * a1, (1.0 - mom) * sv + mom * dv * (p / (p - 1.0) if p > 1 else 1.0)
    rep.ulp2(name, "running_mean", r["rm"], rm, op_m, sm)
    rep.ulp2(name, "running_var", r["rv"], rv, op_v, sv)
    want = int(r["nbt0"]) + len(r["ys"])
    rep._note(name, "batches", 0.0, int(r["nbt"]) == want, f"{name}: num_batches_tracked {int(r['nbt'])}, expected {want}")


def check_step(rep, tape, only=None):
    """Every forward and backward check of a recorded step {"layers": {name: Layer}, "pool": (f1, pooled, pidx) or None, "calls": [...],
    "tail": a pooled tail or None} (``only``: a predicate on layer names, the section of a parametrised case)."""
    keep = only or (lambda name: True)
    for L in tape["layers"].values():
        if keep(L.name):
            check_forward(rep, L)
    if tape.get("pool") is not None and keep("maxpool"):
        check_pool(rep, *tape["pool"])
    if tape.get("tail") is not None and keep(tape["tail"]["layer"]):
        check_tail(rep, tape["tail"])
    seen = {}
    checks = {"bn": check_bn_bwd, "conv": check_conv_bwd, "act": check_act_bwd}
    for call in tape["calls"]:
        if keep(call["layer"]):
            L = tape["layers"][call["layer"]]
            seen[(call["layer"], call["kind"])] = seen.get((call["layer"], call["kind"]), 0) + 1
            checks[call["kind"]](rep, L, call)
    for L in tape["layers"].values():            # every conv is visited once, every BatchNorm once, every fused activation once
        if keep(L.name):
            want = {"conv": 1, "bn": 0 if L.gamma is None else 1, "act": 0 if L.fused_act is None else 1}
            got = {k: seen.get((L.name, k), 0) for k in want}
            rep._note(L.name, "visits", 0.0, got == want, f"{L.name}: backward calls {got}, expected {want}")


def check_eval(rep, tape, only=None):
    """Every check of a recorded eval forward {"evals": [...], "tail": a pooled tail without a backward}."""
    keep = only or (lambda name: True)
    for ev in tape["evals"]:
        if keep(ev["layer"]):
            check_eval_layer(rep, ev)
    if tape.get("tail") is not None and keep(tape["tail"]["layer"]):
        check_tail(rep, tape["tail"])


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
    a z, the engine's kernel entry points of those two families) through ``monkeypatch`` for one backward pass.  With values it also
    wraps what the discriminators run around them (_wrap_tails); ``watch`` a discriminator to get its forwards."""
    DGRAD = {"conv2d_dgrad_up": "phase", "conv2d_dgrad_n16": "n16", "conv2d_dgrad_frag": "frag", "conv2d_dgrad_bnreduce": "bnreduce",
             "conv2d_dgrad_split": "split", "conv2d_dgrad": "igemm"}

    def __init__(self, engine, monkeypatch, values=True):
        """values False: routes only, nothing is copied and nothing synchronised (the census of a full-size step)."""
        self.E, self.calls, self._dg, self._mask = engine, [], [], None
        # the discriminators' records: forwards (watch), delivered gradient arenas, the plan whose backward is running, what the forward
        # in progress noted (eval layers, tail forwards), the last bf16 cast, the feature-level tail's gradient block (a function of the plan)
        self.forwards, self.delivered, self._plan, self._now, self._cast, self.tail_block = [], [], None, [], None, None
        self._mp = monkeypatch
        E, rec = engine, self
        sync = torch.cuda.synchronize if values else (lambda: None)
        host = self._h = to_host if values else (lambda t: None)
        bn_orig, conv_orig = E.Plan.bn_bwd, E.Plan.conv_bwd

        def bn_bwd(P, bn, y, z, ms, dz, act, slope, dres=None, dres_acc=False, has_res=True):
            sync()
            call = {"kind": "bn", "plan": P, "key": y, "dz": host(dz), "dres_old": host(dres) if dres is not None and dres_acc else None,
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
            call = {"kind": "conv", "plan": P, "key": conv, "dy": host(dy), "gw_old": host(P.gw(conv)),
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
        if values:
            self._wrap_tails(monkeypatch, sync, host)

    def _wrap_tails(self, monkeypatch, sync, host):
        """What the discriminators run around Plan.conv_bwd / Plan.bn_bwd: the in-place act_bwd, the two pooled tails, the eval layers,
        the delivery of a gradient arena.  A kernel entry point does not know its plan: Plan.begin_backward names the one whose
        backward is running, the forward in progress (watch) collects what its own calls note."""
        E, rec = self.E, self
        begin_orig, act_orig, eval_orig, deliver_orig = E.Plan.begin_backward, E.K.act_bwd, E.Plan._conv_bn_act_eval, E.ArenaModule.deliver_grads
        cast_orig = E.K.cast_to_bf16

        def begin_backward(P):
            rec._plan = P
            return begin_orig(P)

        def act_bwd(dz, z, dy, act, slope, st=None):
            sync()
            call = {"kind": "act", "plan": rec._plan, "key": z, "dz": host(dz), "act": act, "slope": slope}
            act_orig(dz, z, dy, act, slope, st)
            sync()
            call["dy"] = host(dy)
            rec.calls.append(call)

        def tail_bwd(orig, sigmoid):
            def wrapped(dp, *a):
                p, (pooled, w, dz, dw, db) = (a[0], a[1:6]) if sigmoid else (None, a[0:5])
                sync()
                P = rec._plan
                block = rec.tail_block(P) if rec.tail_block is not None else None
                call = {"kind": "tail", "plan": P, "key": pooled, "sigmoid": sigmoid, "dp": host(dp).reshape(-1), "gw_old": host(dw), "gb_old": host(db)[:1],
                        "block_old": host(block)}
                orig(dp, *a)
                sync()
                call.update(dz=host(dz), gw=host(dw), gb=host(db)[0], block=host(block))
                rec.calls.append(call)
            return wrapped

        def tail_fwd(orig, sigmoid):
            def wrapped(z, w, b, st=None):
                out, pooled = orig(z, w, b, st)
                sync()
                rec._now.append({"kind": "tail_fwd", "key": pooled, "sigmoid": sigmoid, "bf16": z.dtype == torch.bfloat16, "z": host(z),
                                 "w": host(w), "b": host(b)[:1], "pooled": host(pooled), "out": host(out).reshape(-1)})
                return out, pooled
            return wrapped

        def cast_to_bf16(x, out=None, st=None):
            rec._cast = cast_orig(x, out, st)
            return rec._cast

        def conv_bn_act_eval(P, conv, bn, d, x, bias, act, slope, residual):
            sync()
            off, c = P._fold_off, bn.c
            o, nel, shp = P.idx[(id(conv), "weight")]
            ev = {"kind": "eval", "plan": P, "key": conv, "bn": bn, "x": rec._inp(x), "k": conv.k, "stride": conv.stride, "pad": conv.pad,
                  "w32": host(P.net._arena[o:o + nel].view(shp)), "bias": host(bias), "gamma": host(P.pvec(bn, "weight"))[:c],
                  "beta": host(P.pvec(bn, "bias"))[:c], "rm": host(bn.running_mean), "rv": host(bn.running_var), "eps": bn.eps, "act": act,
                  "slope": slope, "residual": host(residual), "storage": "bf16" if P.bf16 else "fp32"}
            rec._cast = None
            z = eval_orig(P, conv, bn, d, x, bias, act, slope, residual)
            sync()
            ev.update(wf=host(P.fold_w[o:o + nel].view(shp)), bf=host(P.fold_b[off:off + E.ceil4(c)]), z=host(z),
                      wf16=host(rec._cast.view(shp)) if P.bf16 and rec._cast is not None else None)
            rec._now.append(ev)
            return z

        def deliver_grads(net, garena):
            sync()
            rec.delivered.append((net, host(garena)))          # before the original adds it onto an earlier one
            return deliver_orig(net, garena)

        monkeypatch.setattr(E.Plan, "begin_backward", begin_backward)
        monkeypatch.setattr(E.K, "act_bwd", act_bwd)
        monkeypatch.setattr(E.K, "gap_linear_sigmoid_bwd", tail_bwd(E.K.gap_linear_sigmoid_bwd, True))
        monkeypatch.setattr(E.K, "gap_linear_bwd", tail_bwd(E.K.gap_linear_bwd, False))
        monkeypatch.setattr(E.K, "gap_linear_sigmoid_fwd", tail_fwd(E.K.gap_linear_sigmoid_fwd, True))
        monkeypatch.setattr(E.K, "gap_linear_fwd", tail_fwd(E.K.gap_linear_fwd, False))
        monkeypatch.setattr(E.K, "cast_to_bf16", cast_to_bf16)
        monkeypatch.setattr(E.Plan, "_conv_bn_act_eval", conv_bn_act_eval)
        monkeypatch.setattr(E.ArenaModule, "deliver_grads", deliver_grads)

    def _inp(self, x):
        E, host = self.E, self._h
        if isinstance(x, E.UpCat):
            return Inp("upcat", a=self._inp(x.a), skip=host(x.skip))
        if isinstance(x, E.LazyAct):
            return Inp("lazy", y=host(x.y), scale=host(x.scale), shift=host(x.shift), act=x.act, slope=x.slope)
        return Inp("plain", t=host(x))

    def watch(self, net):
        """Wrap ``_forward_plan`` on this discriminator (through monkeypatch): every forward leaves {"net", "tape", "out", "events" (its
        eval layers and its tail's forward), "bn": the BatchNorm buffers before and after} in ``self.forwards``; debug_keep_tape makes
        Plan.keep_grads hold."""
        rec, host, orig = self, self._h, net._forward_plan
        self._mp.setattr(net, "debug_keep_tape", True, raising=False)
        names = {n: m for n, m in net.named_modules() if isinstance(m, self.E.BNP)}
        state = lambda: {n: (host(m.running_mean), host(m.running_var), int(m.num_batches_tracked)) for n, m in names.items()}  # noqa: E731

        def forward_plan(x, save):
            torch.cuda.synchronize()
            before, rec._now = state(), []
            out, tape = orig(x, save)
            torch.cuda.synchronize()
            rec.forwards.append({"net": net, "tape": tape, "out": host(out), "events": rec._now, "training": net.training,
                                 "bn": (before, state())})
            rec._now = []
            return out, tape

        self._mp.setattr(net, "_forward_plan", forward_plan, raising=False)
        return net

    # -- the discriminators' tapes, in the form of ``tape`` below
    def _of(self, f, records, tail_layer, first=None):
        """Layers, calls, tail of one training forward ``f`` of a watched discriminator.  records: [(ConvRecord, name)]; first: (Layer of
        the BatchNorm-less first convolution, its module, its stored output)."""
        host, net, P = self._h, f["net"], f["tape"][0]
        sd = {k: host(v) for k, v in net.state_dict().items()}
        names = {id(m): n for n, m in net.named_modules()}
        storage = "bf16" if P.bf16 else "fp32"

        def conv_fields(conv):
            nm = names[id(conv)]
            return dict(name=nm, k=conv.k, stride=conv.stride, pad=conv.pad, w=np.ascontiguousarray(sd[nm + ".weight"].transpose(0, 2, 3, 1)),
                        bias=sd[nm + ".bias"] if conv.bias is not None else None, storage=storage)

        layers, by = {}, {}
        if first is not None:
            conv0, d0, x4, a0 = first
            route, _ = P.fwd_route(conv0, d0, x4, (self.E.FRAG_BNIN, self.E.FRAG, self.E.IGEMM))
            L = Layer(x=self._inp(x4), y=host(a0), route=route, fused_act=N.LEAKY, fused_slope=float(self.act_slope), **conv_fields(conv0))
            layers[L.name] = L
            by[id(conv0)], by[id(a0)] = L.name, L.name
        for r in records:
            bn = names[id(r.bn)]
            L = Layer(x=self._inp(r.x), y=host(r.y), z=host(r.z), mean=host(r.mean), rstd=host(r.rstd), gamma=sd[bn + ".weight"],
                      beta=sd[bn + ".bias"], eps=r.bn.eps, act=r.act, slope=r.slope, route=r.route, bn_name=bn, **conv_fields(r.conv))
            layers[L.name] = L
            by[id(r.y)], by[id(r.conv)] = L.name, L.name
        calls, tail = [], next(dict(e) for e in f["events"] if e["kind"] == "tail_fwd")
        pooled = tail.pop("key")
        tail.update(layer=tail_layer, dp=None)
        for call in self.calls:
            if call.get("plan") is not P:
                continue
            call = dict(call)
            key = call.pop("key")
            call.pop("plan")
            if call["kind"] == "tail":
                assert key is pooled, "a tail backward on another forward's pooled vector"
                tail.update({k: v for k, v in call.items() if k not in ("kind", "sigmoid")})
                continue
            call["layer"] = by[id(key)]
            calls.append(call)
        return {"layers": layers, "pool": None, "calls": calls, "tail": tail, "out": f["out"], "bf16": P.bf16}

    act_slope = 0.2          # discriminator.SLOPE, the slope of the image-level network's LeakyReLUs

    def image_tape(self, f):
        """The step of one training forward of the image-level discriminator: tape (P, (conv0, d0, x4, a0), recs, (lin, h, pooled, p))."""
        P, first, recs, (lin, h, pooled, p) = f["tape"]
        return self._of(f, recs, {id(m): n for n, m in f["net"].named_modules()}[id(lin)], first)

    def feature_tape(self, f):
        """The step of one training forward of the feature-level discriminator: tape (P, recs, (last, h, pooled))."""
        P, recs, (last, h, pooled) = f["tape"]
        return self._of(f, recs, {id(m): n for n, m in f["net"].named_modules()}[id(last)])

    def eval_tape(self, f):
        """An eval forward of a watched discriminator: its folded layers and its tail's forward."""
        names = {id(m): n for n, m in f["net"].named_modules()}
        evals = []
        for e in f["events"]:
            if e["kind"] == "eval":
                e = dict(e)
                e["layer"] = names[id(e.pop("key"))]
                e.pop("plan"), e.pop("bn")
                evals.append(e)
        tail = next(dict(e) for e in f["events"] if e["kind"] == "tail_fwd")
        tail.pop("key")
        tail.update(layer=names[id(f["net"]._layers()[-1])], dp=None)
        return {"evals": evals, "tail": tail, "out": f["out"]}

    def running(self, net, forwards):
        """check_running's records of a watched network after its training ``forwards`` (in forward order), one per BatchNorm."""
        names = {id(m): n for n, m in net.named_modules()}
        out = []
        for i, r in enumerate(forwards[0]["tape"][2] if len(forwards[0]["tape"]) == 4 else forwards[0]["tape"][1]):
            bn = names[id(r.bn)]
            ys = [self._h((f["tape"][2] if len(f["tape"]) == 4 else f["tape"][1])[i].y) for f in forwards]
            rm0, rv0, nbt0 = forwards[0]["bn"][0][bn]
            rm, rv, nbt = forwards[-1]["bn"][1][bn]
            out.append({"layer": bn, "ys": ys, "eps": r.bn.eps, "momentum": r.bn.momentum, "bf16": forwards[0]["tape"][0].bf16,
                        "rm0": rm0, "rv0": rv0, "nbt0": nbt0, "rm": rm, "rv": rv, "nbt": nbt})
        return out

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
            if call["kind"] not in ("bn", "conv"):
                continue
            call = dict(call)
            key = call.pop("key")
            call.pop("plan")
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
