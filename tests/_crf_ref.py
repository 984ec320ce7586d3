"""numpy mirror of the CRF refinement (crf.py, csrc/crf.hip; include/udaseg.h states the rule): the definition as plain loops over
the neighbours of the window, made obviously right rather than fast.  Every function takes the float type ``dt``: ``np.float64`` is
the reference the kernels are held to, ``np.float32`` the same formulas evaluated in the kernels' precision (the leg the bar
``max(4 x max(d), 2^-22)`` of tests/_grade.py is measured from).  Scores are NHWC here: ``[N, H, W, C]``.

Also the inputs of tests/test_gpu_crf.py (``CASES``, ``make_case``), so that tests/test_crf_host.py can vet them on the CPU.
"""
import numpy as np

F64, F32 = np.float64, np.float32

DEFAULTS = dict(radius=3, dilation=2, iterations=5, w_app=10.0, w_smooth=3.0, theta_alpha=80.0, theta_beta=13.0, theta_gamma=3.0,
                strength=1.0)


# ------------------------------------------------------------------------------------------------------------------ the rule
def spatial_table(radius, dilation, theta):
    """fp32 [K, K]: exp(-(dy^2 + dx^2) d^2 / (2 theta^2)) made in float64 and rounded, as the host hands it to the kernel."""
    k = 2 * radius + 1
    t = np.empty((k, k), dtype=F64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            t[dy + radius, dx + radius] = np.exp(-(dy * dy + dx * dx) * float(dilation) ** 2 / (2.0 * float(theta) ** 2))
    return t.astype(F32)


def inv2b_of(theta_beta):
    return F32(1.0 / (2.0 * float(theta_beta) ** 2))


def prepare(scores, probs=False, dt=F64):
    """(log P0, P0, valid) of scores [N, H, W, C]; invalid rows are NaN in both.  log 0 = -inf is kept."""
    s = np.asarray(scores).astype(dt)
    with np.errstate(all="ignore"):
        if probs:
            valid = ((s >= 0) & (s <= 1)).all(axis=-1)
            tot = s.sum(axis=-1, keepdims=True, dtype=dt)
            valid &= np.isfinite(tot[..., 0]) & (tot[..., 0] > 0)
            p0 = (s / tot).astype(dt)
            logp = np.log(p0).astype(dt)
        else:
            valid = np.isfinite(s).all(axis=-1)
            z = (s - s.max(axis=-1, keepdims=True)).astype(dt)
            lse = np.log(np.exp(z).sum(axis=-1, keepdims=True, dtype=dt)).astype(dt)
            logp = (z - lse).astype(dt)
            p0 = (np.exp(z) / np.exp(z).sum(axis=-1, keepdims=True, dtype=dt)).astype(dt)
    logp[~valid] = np.nan
    p0[~valid] = np.nan
    return logp, p0, valid


def _shifted(a, oy, ox):
    """out[n, y, x] = a[n, y + oy, x + ox] inside the image, 0 outside (images never see each other)."""
    out = np.zeros_like(a)
    h, w = a.shape[1], a.shape[2]
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = a[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def step(logp, q, valid, frames, radius, dilation, s_alpha, s_gamma, w_app, w_smooth, inv2b, strength, dt=F64):
    """One Jacobi sweep: Q' = softmax(log P0 + m), m = strength * sum_j k_ij Q_j / Z_i, a loop over the window's neighbours."""
    logp, q = np.asarray(logp).astype(dt), np.asarray(q).astype(dt)
    valid = np.asarray(valid).astype(bool)
    rgb = np.asarray(frames).astype(np.int64)
    qz = np.where(valid[..., None], q, dt(0))                # a void pixel sends nothing
    wa, ws, ib, st = dt(w_app), dt(w_smooth), dt(inv2b), dt(strength)
    acc = np.zeros(q.shape, dtype=dt)
    zsum = np.zeros(valid.shape, dtype=dt)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            oy, ox = dy * dilation, dx * dilation
            nb = _shifted(valid, oy, ox)                     # the neighbour lies inside the image and is valid
            c2 = ((rgb - _shifted(rgb, oy, ox)) ** 2).sum(axis=-1)
            col = np.exp(-(c2.astype(dt) * ib)).astype(dt)
            sa, sg = dt(s_alpha[dy + radius, dx + radius]), dt(s_gamma[dy + radius, dx + radius])
            k = ((wa * sa) * col + ws * sg).astype(dt)
            k = np.where(nb, k, dt(0))
            acc = (acc + k[..., None] * _shifted(qz, oy, ox)).astype(dt)
            zsum = (zsum + np.where(nb, wa * sa + ws * sg, dt(0))).astype(dt)
    with np.errstate(all="ignore"):
        m = np.where(zsum[..., None] > 0, st * acc / zsum[..., None], dt(0)).astype(dt)
        t = (logp + m).astype(dt)
        e = np.exp(t - t.max(axis=-1, keepdims=True)).astype(dt)
        out = (e / e.sum(axis=-1, keepdims=True, dtype=dt)).astype(dt)
    out[~valid] = np.nan
    return out


def refine(scores, frames, radius=3, dilation=2, iterations=5, w_app=10.0, w_smooth=3.0, theta_alpha=80.0, theta_beta=13.0,
           theta_gamma=3.0, strength=1.0, probs=False, dt=F64):
    """Q^T of scores [N, H, W, C] under uint8 frames [N, H, W, 3]; NaN rows at the void pixels."""
    logp, q, valid = prepare(scores, probs, dt)
    sa, sg = spatial_table(radius, dilation, theta_alpha), spatial_table(radius, dilation, theta_gamma)
    for _ in range(iterations):
        q = step(logp, q, valid, frames, radius, dilation, sa, sg, w_app, w_smooth, inv2b_of(theta_beta), strength, dt)
    return q


def dense_step(logp, q, valid, frame, radius, dilation, s_alpha, s_gamma, w_app, w_smooth, inv2b, strength):
    """The same sweep of ONE image [H, W, C] through an explicit [HW, HW] kernel matrix (float64): the independent formulation."""
    h, w, c = q.shape
    npix = h * w
    kern, mass = np.zeros((npix, npix)), np.zeros((npix, npix))
    val = np.asarray(valid).reshape(npix)
    rgb = np.asarray(frame).astype(np.int64).reshape(npix, 3)
    for i in range(npix):
        for j in range(npix):
            oy, ox = j // w - i // w, j % w - i % w
            if i == j or oy % dilation or ox % dilation or not val[j]:
                continue
            dy, dx = oy // dilation, ox // dilation
            if abs(dy) > radius or abs(dx) > radius:
                continue
            c2 = float(((rgb[i] - rgb[j]) ** 2).sum())
            sa, sg = float(s_alpha[dy + radius, dx + radius]), float(s_gamma[dy + radius, dx + radius])
            kern[i, j] = w_app * sa * np.exp(-c2 * float(inv2b)) + w_smooth * sg
            mass[i, j] = w_app * sa + w_smooth * sg
    qz = np.where(val[:, None], np.asarray(q, dtype=F64).reshape(npix, c), 0.0)
    z = mass.sum(axis=1)
    m = np.zeros((npix, c))
    nz = z > 0
    m[nz] = strength * (kern @ qz)[nz] / z[nz, None]
    with np.errstate(all="ignore"):
        t = np.asarray(logp, dtype=F64).reshape(npix, c) + m
        e = np.exp(t - t.max(axis=1, keepdims=True))
        out = e / e.sum(axis=1, keepdims=True)
    out[~val] = np.nan
    return out.reshape(h, w, c)


def d4(a, code):
    """View ``code`` (bit 0: transpose, bit 1: flip rows, bit 2: flip columns) of the two image axes of [N, H, W, ...]."""
    if code & 2:
        a = a[:, ::-1]
    if code & 4:
        a = a[:, :, ::-1]
    if code & 1:
        a = np.swapaxes(a, 1, 2)
    return np.ascontiguousarray(a)


def margin(q):
    """The top-two margin of every row of [..., C] (inf for one class, NaN for a NaN row)."""
    if q.shape[-1] == 1:
        return np.full(q.shape[:-1], np.inf)
    s = np.sort(q, axis=-1)
    return s[..., -1] - s[..., -2]


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def shape_of(name, tile):
    th, tw = tile
    return {"1x1": (1, 1, 1), "3x2": (1, 3, 2), "tile": (1, th, tw), "seam": (1, th + 1, tw + 1),
            "two": (2, 2 * th + 3, 2 * tw + 5)}[name]


def frames_of(kind, n, h, w, seed):
    rng = np.random.default_rng(1000 + seed)
    if kind == "constant":
        return np.full((n, h, w, 3), 97, dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        f = np.stack([(3 * x + y) % 256, (2 * y + 40) % 256, (x + 2 * y) % 256], axis=-1).astype(np.uint8)
        return np.broadcast_to(f, (n, h, w, 3)).copy()
    if kind == "checker":
        y, x = np.mgrid[0:h, 0:w]
        on = ((y + x) & 1).astype(bool)
        f = np.where(on[..., None], np.array([255, 255, 255]), np.array([0, 0, 0])).astype(np.uint8)
        return np.broadcast_to(f, (n, h, w, 3)).copy()
    assert kind == "random", kind
    return rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def scores_of(n, h, w, c, probs, void, seed):
    """fp32 [N, H, W, C]: logits of spread 2 (the images differ), or their softmax with ``probs``; then the void rows."""
    rng = np.random.default_rng(seed)
    s = (2.0 * rng.standard_normal((n, h, w, c))).astype(F32)
    if probs:
        e = np.exp(s.astype(F64) - s.max(axis=-1, keepdims=True))
        s = (e / e.sum(axis=-1, keepdims=True)).astype(F32)
        s = np.minimum(s, F32(1.0))
        s[:, h // 2, w // 3, 0] = 0.0                        # a class with P0 = 0 stays at 0
    bad = np.float32("nan")
    if void in ("interior", "all"):
        s[0, h // 2, w // 2] = bad
    if void in ("corner", "all"):
        s[-1, h - 1, w - 1, c - 1] = np.float32("inf") if not probs else bad
    if void in ("column", "all"):
        s[0, :, min(w - 1, 2)] = bad
    if void == "above1":
        assert probs
        s[0, h // 3, w // 2, 0] = 1.5
    if void == "zerorow":
        assert probs
        s[0, h // 3, w // 2] = 0.0
    return s


def _case(name, **kw):
    base = dict(name=name, shape="seam", C=5, probs=False, void="none", frame="random", pad=0, seed=len(CASES), **DEFAULTS)
    base.update(radius=3, dilation=1, iterations=1, strength=1.5)
    base.update(kw)
    CASES.append(base)


CASES = []
for _s in ("1x1", "3x2", "tile", "seam", "two"):                                        # shapes, at the defaults and 23 classes
    _case(f"shape-{_s}", shape=_s, C=23, dilation=2, iterations=5, void="interior" if _s == "two" else "none")
for _c in (1, 2, 5, 23, 32):                                                            # row widths 4, 4, 8, 24, 32
    _case(f"classes-{_c}", C=_c, radius=1, iterations=5, pad=4 if _c in (2, 23) else 0)
for _r, _d in ((1, 1), (3, 1), (5, 1), (1, 2), (3, 2), (5, 2), (3, 3), (2, 4)):         # windows; (5, 2) reaches 10; every dilation
    _case(f"window-{_r}x{_d}", shape="two", radius=_r, dilation=_d)
_case("chunks-23-reach10", shape="seam", C=23, radius=5, dilation=2, iterations=1)       # class chunks of 2 vectors
_case("chunks-32-reach10", shape="seam", C=32, radius=5, dilation=2, iterations=5, strength=2.0)
_case("chunks-12-reach10", shape="seam", C=12, radius=5, dilation=2)
_case("chunks-23-r3", shape="two", C=23, radius=3, dilation=1, iterations=5)             # chunks of 3
_case("sweeps-0", iterations=0, void="interior")
_case("sweeps-5-probs", iterations=5, probs=True, C=23)
_case("probs", probs=True, shape="two", dilation=2)
_case("app-only", w_smooth=0.0, frame="ramp")
_case("smooth-only", w_app=0.0)
for _f in ("constant", "ramp", "random"):
    _case(f"frame-{_f}", frame=_f, iterations=5, dilation=2, shape="two", C=23 if _f == "ramp" else 5)
_case("frame-checker", frame="checker", theta_beta=1.0, iterations=5, shape="two")
_case("frame-checker-d2", frame="checker", theta_beta=1.0, dilation=2, w_smooth=0.0)     # every neighbour of one colour
for _v in ("interior", "corner", "column", "all"):
    _case(f"void-{_v}", void=_v, iterations=5, shape="two", dilation=2 if _v == "all" else 1)
_case("void-above1", void="above1", probs=True, iterations=5)
_case("void-zerorow", void="zerorow", probs=True, iterations=5)
_case("void-column-3x2", void="column", shape="3x2", radius=1)
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def params_of(case):
    return {k: case[k] for k in DEFAULTS}


def make_case(case, tile):
    """(scores fp32 [N, H, W, C], frames uint8 [N, H, W, 3]) of one case at the kernel's tile for its window."""
    n, h, w = shape_of(case["shape"], tile)
    return (scores_of(n, h, w, case["C"], case["probs"], case["void"], case["seed"]),
            frames_of(case["frame"], n, h, w, case["seed"]))
