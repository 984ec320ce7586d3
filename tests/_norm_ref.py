"""numpy restatement of the streaming kernels every training step runs: training- and eval-mode BatchNorm with its fused
activation / residual add and their backward (csrc/norm_act.hip, both storages from one body per kernel), ``act_bwd``,
``channel_sum``, ``bn_finalize`` and Adam (csrc/optim.hip).

Test infrastructure, in the manner of ``_resize_ref`` / ``_clahe_ref``: the per-element arithmetic is written once, generically
over the float type ``elem`` -- ``np.float64`` is the reference the kernels are held to, ``np.float32`` the same arithmetic in the
kernels' precision (the leg the bar of tests/test_gpu_norm_grade.py is measured from).  Tensors are ``[pixels, channels]`` (NHWC
with the pixel axes flattened).

Statistics are always float64 sums over the STORED input values, as in the kernels.  What the kernels document about them is the
cast of mean and rstd to fp32 before any per-element use; ``stat=np.float32`` (the default) applies that cast in BOTH legs, so the
float64 leg differs from the kernels only by the rounding of the per-element arithmetic.  ``stat=np.float64`` leaves the cast out:
that is the textbook definition, the one tests/test_norm_ref_host.py holds to torch's double-precision autograd.

Every function also returns the MAGNITUDE of each output element (or channel): the sum of the absolute values of the terms that
formed it.  Errors are judged relative to it, so cancellation cannot hide behind a small output and a small channel cannot hide
behind a large one.
"""
import numpy as np

NONE, LEAKY = 0, 1                       # UDASEG_ACT_*; ReLU is LEAKY with slope 0
F64, F32 = np.float64, np.float32


def bf16_round(x):
    """Round-to-nearest-even of fp32 values to bf16, returned as fp32 (finite values)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def bf16_half_ulp(v, slack=0.0):
    """Half the bf16 spacing (8 significant bits) at |v| + slack: with ``slack`` the distance a pre-rounding value may lie from
    v, this is the larger neighbouring spacing at a binade edge.  0 where |v| + slack == 0."""
    a = np.abs(np.asarray(v, dtype=F64)) + slack
    out = np.zeros_like(a)
    nz = a > 0
    out[nz] = np.exp2(np.floor(np.log2(a[nz])) - 8.0)
    return out


# ---------------------------------------------------------------------------------------------------------------- statistics
def stats(y, eps):
    """(mean, var, rstd) per channel in float64: mean = sum y / P, var = max(sum y^2 / P - mean^2, 0), rstd = 1 / sqrt(var + eps)."""
    y = np.asarray(y, dtype=F64)
    p = y.shape[0]
    mean = y.sum(0) / p
    var = np.maximum((y * y).sum(0) / p - mean * mean, 0.0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def running(mean, var, pixels, momentum, running_mean, running_var):
    """(running_mean, running_var, their magnitudes) in float64; the variance enters with the unbiased factor P / (P - 1), 1 when P == 1."""
    unb = var * (pixels / (pixels - 1.0) if pixels > 1 else 1.0)
    rm0, rv0 = np.asarray(running_mean, dtype=F64), np.asarray(running_var, dtype=F64)
    a, b = (1.0 - momentum) * rm0, momentum * mean
    c, d = (1.0 - momentum) * rv0, momentum * unb
    return a + b, c + d, np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d))


def _act(t, act, slope, dt):
    return np.where(t < 0, t * dt(slope), t).astype(dt) if act == LEAKY else t


def _act_factor(z, act, slope, dt):
    """Derivative factor from the OUTPUT's sign: ``slope`` where not (z > 0) -- so 0.0 and -0.0 both take ``slope``."""
    return np.where(z > 0, dt(1), dt(slope)).astype(dt) if act == LEAKY else None


def _coeffs(gamma, beta, mean, rstd, elem, stat):
    mean, rstd = np.asarray(mean).astype(stat).astype(elem), np.asarray(rstd).astype(stat).astype(elem)
    scale = (np.asarray(gamma).astype(elem) * rstd).astype(elem)
    shift = (np.asarray(beta).astype(elem) - mean * scale).astype(elem)
    return mean, rstd, scale, shift


def _apply(y, scale, shift, residual, act, slope, elem):
    y = np.asarray(y).astype(elem)
    t = (y * scale + shift).astype(elem)
    mag = np.abs(y.astype(F64) * scale.astype(F64)) + np.abs(shift.astype(F64))
    if residual is not None:
        t = (t + np.asarray(residual).astype(elem)).astype(elem)
        mag = mag + np.abs(np.asarray(residual, dtype=F64))
    return _act(t, act, slope, elem), t, mag


# ------------------------------------------------------------------------------------------------------------------- forward
def bn_finalize(y, gamma, beta, eps, elem=F64, stat=F32):
    """(scale, shift) = (gamma * rstd, beta - mean * scale) and their magnitudes (|scale|, |beta| + |mean * scale|)."""
    mean, _, rstd = stats(y, eps)
    mean, _, scale, shift = _coeffs(gamma, beta, mean, rstd, elem, stat)
    return scale, shift, np.abs(scale.astype(F64)), np.abs(np.asarray(beta, dtype=F64)) + np.abs(mean.astype(F64) * scale.astype(F64))


def bn_forward(y, gamma, beta, residual, eps, act, slope, elem=F64, stat=F32):
    """Training-mode forward: z = act(y * scale + shift (+ residual)).  Returns (z, pre-activation t, magnitude)."""
    mean, _, rstd = stats(y, eps)
    _, _, scale, shift = _coeffs(gamma, beta, mean, rstd, elem, stat)
    return _apply(y, scale, shift, residual, act, slope, elem)


def bn_eval(y, gamma, beta, running_mean, running_var, residual, eps, act, slope, elem=F64):
    """Eval-mode apply: the running statistics (fp32 values) take the place of the batch's; rstd is formed in ``elem``."""
    rstd = (elem(1) / np.sqrt(np.asarray(running_var).astype(elem) + elem(eps))).astype(elem)
    scale = (np.asarray(gamma).astype(elem) * rstd).astype(elem)
    shift = (np.asarray(beta).astype(elem) - np.asarray(running_mean).astype(elem) * scale).astype(elem)
    return _apply(y, scale, shift, residual, act, slope, elem)


# ------------------------------------------------------------------------------------------------------------------ backward
def bn_backward(dz, z, y, gamma, eps, act, slope, elem=F64, stat=F32):
    """Backward of the training-mode layer from its output z (None without an activation).

    g = dz * factor(z);  xhat = (y - mean) * rstd;  dbeta = sum g;  dgamma = sum g * xhat;
    dy = scale * (g - mean(g) - xhat * mean(g * xhat));  dres = g.  The sums are taken in ``elem``.
    Returns a dict name -> (value, magnitude) for dy, dres, dgamma, dbeta."""
    mean, _, rstd = stats(y, eps)
    mean, rstd, scale, _ = _coeffs(gamma, gamma, mean, rstd, elem, stat)
    y, g = np.asarray(y).astype(elem), np.asarray(dz).astype(elem)
    if act == LEAKY:
        g = (g * _act_factor(np.asarray(z), act, slope, elem)).astype(elem)
    p = y.shape[0]
    xhat = ((y - mean) * rstd).astype(elem)
    dbeta = g.sum(0, dtype=elem)
    dgamma = (g * xhat).sum(0, dtype=elem)
    mg, mgx = (dbeta / elem(p)).astype(elem), (dgamma / elem(p)).astype(elem)
    dy = (scale * (g - mg - xhat * mgx)).astype(elem)
    a = lambda t: np.abs(np.asarray(t, dtype=F64))
    mag_dy = a(scale) * (a(g) + a(mg) + a(xhat.astype(F64) * mgx.astype(F64)))
    mag_dgamma = (a(g) * (a(xhat) + a(rstd) * a(mean))).sum(0)
    mag_dbeta = a(g).sum(0)
    return {"dy": (dy, mag_dy), "dres": (g, a(g)), "dgamma": (dgamma, mag_dgamma), "dbeta": (dbeta, mag_dbeta)}


def act_bwd(dz, z, act, slope, elem=F64):
    """dy = dz * factor(z) and its magnitude |dy|."""
    g = np.asarray(dz).astype(elem)
    if act == LEAKY:
        g = (g * _act_factor(np.asarray(z), act, slope, elem)).astype(elem)
    return g, np.abs(g.astype(F64))


def channel_sum(x, elem=F64):
    """Per-channel sum over the pixels and its magnitude sum |x|."""
    x = np.asarray(x)
    return x.astype(elem).sum(0, dtype=elem), np.abs(x.astype(F64)).sum(0)


# ---------------------------------------------------------------------------------------------------------------------- Adam
def adam_step(p, g, m, v, lr, beta1, beta2, eps, t, elem=F64):
    """One step of torch's single-tensor Adam (no weight decay, no amsgrad), t counted from 1:
    m += (g - m) * (1 - b1);  v = v * b2 + (1 - b2) * g * g;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
    with bc = 1 - beta ** t.  The hyper-parameters are python floats, each rounded once to ``elem`` where it meets a tensor.
    Returns (p, m, v) and their magnitudes (|p| + lr, |m| + (1 - b1) (|g| + |m|), b2 v + (1 - b2) g^2)."""
    p, g, m, v = (np.asarray(x).astype(elem) for x in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    a = lambda x: np.abs(np.asarray(x, dtype=F64))
    mag_m = a(m) + (1.0 - beta1) * (a(g) + a(m))
    mag_v = beta2 * a(v) + (1.0 - beta2) * a(g) ** 2
    m = (m + (g - m) * elem(1.0 - beta1)).astype(elem)
    v = (v * elem(beta2) + elem(1.0 - beta2) * g * g).astype(elem)
    denom = (np.sqrt(v) / elem(bc2 ** 0.5) + elem(eps)).astype(elem)
    p_new = (p - elem(lr / bc1) * (m / denom)).astype(elem)
    return (p_new, m, v), (a(p) + lr, mag_m, mag_v)


# ----------------------------------------------------------------------------------------------------------------------- bar
def normalised(err, mag):
    """|err| / mag element-wise; where the magnitude is 0 every term of the output is 0 and any error at all is infinite."""
    err, mag = np.abs(np.asarray(err, dtype=F64)), np.asarray(mag, dtype=F64)
    out = np.zeros_like(err)
    nz = mag > 0
    out[nz] = err[nz] / mag[nz]
    out[~nz & (err > 0)] = np.inf
    return out


FLOOR = 2.0 ** -22                         # 2 ulp of fp32, relative to the magnitude


def bar(leg, ref, mag, margin=4.0):
    """max(margin x the fp32 leg's worst normalised deviation from the float64 leg over the WHOLE output, 2 ulp)."""
    d = normalised(np.asarray(leg, dtype=F64) - np.asarray(ref, dtype=F64), mag)
    return max(margin * float(d.max(initial=0.0)), FLOOR), float(d.max(initial=0.0))
