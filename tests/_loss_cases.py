"""The cases of tests/test_gpu_loss_grade.py and the code that grades one of them, written against a BACKEND: an object that runs
the loss operations on padded NHWC buffers given as numpy arrays.  The GPU file's backend launches the HIP kernels;
tests/test_loss_ref_host.py passes ``LegBackend``, the float32 leg of tests/_loss_ref.py standing in for the kernels -- plain to
show that every case can pass, with one of ``_loss_ref.MUTATIONS`` to show that a mistake of that kind cannot.

Every graded figure obeys one bar, that of tests/test_gpu_norm_grade.py: e = |kernel - f64| / magnitude,
d = |fp32 leg - f64| / magnitude element-wise, max(e) <= max(4 max(d), 2^-22); pad lanes and void rows of every gradient exactly 0.
"""
import numpy as np

import _loss_ref as R
from _loss_ref import F32, F64, f32

BIG = "big"                                   # marks the cases of 65 792 pixels per image and more


# ----------------------------------------------------------------------------------------------------------- launch shapes
def grid_pix(pixels, cap=1024):
    """Blocks of 256 threads that the segmentation-loss and cross-entropy kernels launch over ``pixels``."""
    return min(-(-pixels // 256), cap)


def passes(pixels, cap=1024):
    """Grid-stride passes the busiest thread makes."""
    return -(-pixels // (grid_pix(pixels, cap) * 256))


def ce_row_groups(ldc):
    """(NG, threads that reduce) of the tiled cross-entropy backward's column sums."""
    ng = 256 // ldc
    return ng, ng * ldc


def straddling_blocks(batch, ppi):
    """Blocks of 256 consecutive pixels that hold pixels of more than one image."""
    total = batch * ppi
    return [b for b in range(-(-total // 256)) if (b * 256) // ppi != (min(total, (b + 1) * 256) - 1) // ppi]


# -------------------------------------------------------------------------------------------------------------------- data
def pad_buf(z, ldc):
    """[P, C] -> [P, ldc] fp32 whose pad lanes hold finite junk: 7.0, and one lane 1e30."""
    p, c = z.shape
    buf = np.full((p, ldc), R.PAD_JUNK, dtype=F32)
    buf[:, :c] = z
    if ldc > c:
        buf[p // 2, ldc - 1] = 1e30
    return buf


def make_target(rng, batch, ppi, classes, absent=False, void=None, ignore_index=None, out_of_range=False):
    t = rng.integers(0, classes, batch * ppi).astype(np.int64)
    if absent and classes > 2:
        t[t == classes - 2] = 0                           # absent from the whole batch
        t[:ppi][t[:ppi] == classes - 1] = 1               # absent from image 0 only
        t[-1] = classes - 1
    n = t.size
    if void == "random_void":
        t[rng.random(n) < 0.25] = ignore_index
    elif void == "void_run":                              # from 6 pixels before an aligned 256-chunk to 8 pixels after its end
        lo, hi = (250, 520) if n > 520 else (n // 3, 2 * n // 3)
        t[lo:hi] = ignore_index
    elif void == "all_void":
        t[:] = ignore_index
    if out_of_range:
        t[1 % n], t[(n // 2 + 1) % n], t[n - 1] = classes + 3, -7, classes
    return t


def make_logits(rng, pixels, classes, kind, t):
    """randn3: randn x 3.  marginM: the target class M above the largest other logit (8: confident; 20: 1 - pt rounds to 0 in fp32;
    60: the other probabilities near 1e-26).  wrong50: the target 50 below the smallest.  shift1e4: randn x 3 plus 1e4 or -1e4 per
    pixel.  Void and out-of-range labels take class 0 for this purpose."""
    z = rng.standard_normal((pixels, classes)) * (3.0 if kind in ("randn3", "shift1e4") else 1.0)
    tt = np.where((t >= 0) & (t < classes), t, 0)
    rows = np.arange(pixels)
    if kind.startswith("margin"):
        z[rows, tt] = -np.inf
        z[rows, tt] = (z.max(1) if classes > 1 else 0.0) + float(kind[6:])
    elif kind == "wrong50":
        z[rows, tt] = np.inf
        z[rows, tt] = (z.min(1) if classes > 1 else 0.0) - 50.0
    elif kind == "shift1e4":
        z += np.where(rows % 2 == 0, 1e4, -1e4)[:, None]
    return z.astype(F32)


def scales(go, weight):
    """Upstream gradient (None: the null pointer, 1) x weight: the float64 product and the fp32 one the kernel forms."""
    g = 1.0 if go is None else f32(go)
    return g * f32(weight), float(F32(g) * F32(weight))


def _trip(r64, r32, key):
    return r64[key][0], r32[key][0], r64[key][1]


def _seed(tag):
    return np.random.default_rng(int.from_bytes(tag.encode(), "little") % (2 ** 63))


UPSTREAM = [(None, 1.0), (1.0, 0.6), (0.37, 1.7)]         # (upstream gradient, weight)


# ----------------------------------------------------------------------------------------------------------- the float32 leg
class LegBackend:
    """The float32 leg of _loss_ref standing in for the kernels; ``mut``: one of _loss_ref.MUTATIONS."""
    def __init__(self, mut=None):
        self.mut = mut

    @staticmethod
    def _padded(d, ldc, old):
        out = np.zeros((d.shape[0], ldc), dtype=F32)
        out[:, :d.shape[1]] = d
        return out if old is None else (old + out).astype(F32)

    def dice(self, zbuf, t, batch, classes, smooth, eps, pooled, ignore_index, go, weight, old=None):
        r = R.dice(zbuf[:, :classes], t, batch, smooth, eps, pooled, ignore_index, scales(go, weight)[1], F32, self.mut)
        return r["loss"][0], r["coef"][0], self._padded(r["grad"][0], zbuf.shape[1], old)

    def focal_fwd(self, zbuf, t, class_w, alpha, gamma, mean, classes, ignore_index, old=None):
        v = R.focal(zbuf[:, :classes], t, class_w, alpha, gamma, mean, ignore_index, 1.0, F32, self.mut)["loss"][0]
        return v if old is None else F32(old) + v

    def focal_bwd(self, zbuf, t, class_w, alpha, gamma, classes, ignore_index, go, weight, old=None):
        r = R.focal(zbuf[:, :classes], t, class_w, alpha, gamma, False, ignore_index, scales(go, weight)[1], F32, self.mut)
        return self._padded(r["grad"][0], zbuf.shape[1], old)

    def consistency(self, z1buf, z2buf, temperature, batch, classes, go, weight, which="both", old=None):
        inv_t = float(F32(1) / F32(temperature))
        r = R.consistency(z1buf[:, :classes], z2buf[:, :classes], inv_t, batch, scales(go, weight)[1], F32, self.mut)
        ldc = z1buf.shape[1]
        d1 = self._padded(r["d1"][0], ldc, None if old is None else old[0]) if which in ("both", "d1") else None
        d2 = self._padded(r["d2"][0], ldc, None if old is None else old[1]) if which in ("both", "d2") else None
        return r["loss"][0], d1, d2

    def ce(self, zbuf, t, classes, go, fused=False):
        r = R.cross_entropy(zbuf[:, :classes], t, 1.0 if go is None else go, F32, self.mut)
        ldc = zbuf.shape[1]
        colsum = None
        if ldc <= 32:
            colsum = np.zeros(ldc, dtype=F32)
            colsum[:classes] = r["colsum"][0]
        return r["loss"][0], r["lse"][0], self._padded(r["grad"][0], ldc, None), colsum

    def tail_fwd(self, z, w, b, sigmoid, bf16=False):
        r = R.tail_forward(z, w, b, sigmoid, F32)
        return r["out"][0], r["pooled"][0]

    def tail_bwd(self, dp, p, pooled, w, hw, sigmoid, old=None, bf16=False):
        r = R.tail_backward(dp, p, pooled, w, hw, sigmoid, F32)
        dz = np.repeat(r["dz"][0][:, None, :], hw, axis=1)
        dz = R.bf16_round(dz) if bf16 else dz
        dw, db = r["dw"][0], r["db"][0]
        if old is not None:
            dw, db = (dw if self.mut == "dw_overwrite" else (old[0] + dw).astype(F32)), F32(old[1] + db)
        return dz, dw, db

    def bce_fwd(self, x, y, weight, old=None):
        wrong = self.mut == "bce_wrong_n" and old is not None
        v = R.bce(x, y, weight, 1.0, F32, n_div=2 * np.size(x) if wrong else None)["loss"][0]
        return v if old is None else F32(old) + v

    def bce_bwd(self, x, y, weight, go, old=None):
        wrong = self.mut == "bce_wrong_n" and old is not None
        d = R.bce(x, y, weight, 1.0 if go is None else go, F32, n_div=2 * np.size(x) if wrong else None)["dx"][0]
        return d if old is None else (old + d).astype(F32)


# ------------------------------------------------------------------------------------------------- segmentation-loss cases
def seg_case(batch, classes, h, w, ldc=None, kind="randn3", seed=0, **kw):
    ldc = ldc or (classes + 3) // 4 * 4
    return dict(batch=batch, classes=classes, ppi=h * w, ldc=ldc, kind=kind, seed=seed, **kw)


def seg_id(c):
    extra = "-".join(f"{k}={v}" for k, v in c.items() if k not in ("batch", "classes", "ppi", "ldc", "kind", "seed"))
    return f"{c['batch']}x{c['classes']}x{c['ppi']}-ldc{c['ldc']}-{c['kind']}" + (f"-{extra}" if extra else "")


TEMPLATE_SHAPES = [seg_case(3, ldc - 1, 5, 7, ldc) for ldc in range(4, 33, 4)] + [seg_case(3, 4, 5, 7), seg_case(3, 32, 5, 7), seg_case(3, 1, 5, 7)]
TAIL_SHAPES = [seg_case(1, 3, 1, p) for p in (1, 255, 256, 257)]
STRIDE_SHAPES = [seg_case(1, 3, 513, 512, size=BIG), seg_case(2, 3, 257, 256, size=BIG)]
LAUNCH_SHAPES = TEMPLATE_SHAPES + TAIL_SHAPES + STRIDE_SHAPES
EDGE_SHAPES = [(3, 23, 5, 7), (2, 5, 16, 17)]
KINDS = ["randn3", "margin8", "margin20", "margin60", "wrong50", "shift1e4"]
GAMMAS = [0.0, 0.5, 1.0, 2.0, 3.0]
VOIDS = [(v, i) for v in ("random_void", "void_run", "all_void") for i in (255, -100, 0)]

FOCAL_EDGE = [seg_case(*s, kind=k, gamma=g) for s in EDGE_SHAPES for k in KINDS for g in GAMMAS]
FOCAL_VOID = [seg_case(*s, kind=k, void=v, ignore_index=i) for s in EDGE_SHAPES for v, i in VOIDS for k in ("randn3", "margin20")]
DICE_EDGE = [seg_case(*s, kind=k, smooth=sm) for s in EDGE_SHAPES for k in KINDS for sm in (0.0, 0.1, 1.0)]
DICE_VOID = [seg_case(*s, void=v, ignore_index=i, smooth=sm) for s in EDGE_SHAPES for v, i in VOIDS for sm in (0.1, 1.0)]
CONS_EDGE = [seg_case(*s, kind=k, temperature=t) for s in EDGE_SHAPES for t in (0.5, 0.7, 1.0, 2.0)
             for k in ("randn3", "same", "margin200", "shift1e4")]


def seg_data(c, absent=False):
    rng = _seed(seg_id(c))
    t = make_target(rng, c["batch"], c["ppi"], c["classes"], absent=absent, void=c.get("void"), ignore_index=c.get("ignore_index"),
                    out_of_range=c.get("out_of_range", False))
    kind = c["kind"] if c["kind"] not in ("same", "margin200") else "randn3"
    z = make_logits(rng, t.size, c["classes"], kind, t)
    return rng, z, t


def grade_dice(B, G, c, z, t, smooth, eps, pooled, ignore_index, go, weight, tag):
    classes, ldc, batch = c["classes"], c["ldc"], c["batch"]
    s64, s32 = scales(go, weight)
    r64 = R.dice(z, t, batch, smooth, eps, pooled, ignore_index, s64, F64)
    r32 = R.dice(z, t, batch, smooth, eps, pooled, ignore_index, s32, F32)
    loss, coef, d = B.dice(pad_buf(z, ldc), t, batch, classes, smooth, eps, pooled, ignore_index, go, weight)
    G.grade(f"{tag} loss", loss, *_trip(r64, r32, "loss"))
    G.grade(f"{tag} coef", coef, *_trip(r64, r32, "coef"))
    G.grade(f"{tag} grad", d[:, :classes], *_trip(r64, r32, "grad"))
    G.zero(f"{tag} grad pad lanes", d[:, classes:])
    G.zero(f"{tag} grad void rows", d[~R.live_mask(t, classes, ignore_index)[0]])
    return d, r64, r32


def grade_focal(B, G, c, z, t, class_w, alpha, gamma, mean, ignore_index, go, weight, tag):
    classes, ldc = c["classes"], c["ldc"]
    s64, s32 = scales(go, weight)
    r64 = R.focal(z, t, class_w, alpha, gamma, mean, ignore_index, s64, F64)
    r32 = R.focal(z, t, class_w, alpha, gamma, mean, ignore_index, s32, F32)
    # the one discontinuity, om > 0: the float32 leg must meet the bar across it before anything is launched
    b, dmax = R.bar(r32["grad"][0], *r64["grad"])
    assert np.isfinite(dmax) and dmax <= b, f"{tag}: the float32 leg misses its own bar across the om > 0 branch"
    zbuf = pad_buf(z, ldc)
    loss = B.focal_fwd(zbuf, t, class_w, alpha, gamma, mean, classes, ignore_index)
    d = B.focal_bwd(zbuf, t, class_w, alpha, gamma, classes, ignore_index, go, weight)
    G.grade(f"{tag} loss", loss, *_trip(r64, r32, "loss"))
    G.grade(f"{tag} grad", d[:, :classes], *_trip(r64, r32, "grad"))
    G.zero(f"{tag} grad pad lanes", d[:, classes:])
    G.zero(f"{tag} grad void rows", d[~R.live_mask(t, classes, ignore_index)[0]])
    return d, r64, r32


def grade_consistency(B, G, c, z1, z2, temperature, go, weight, tag, which="both"):
    classes, ldc, batch = c["classes"], c["ldc"], c["batch"]
    inv_t = float(F32(1) / F32(temperature))
    s64, s32 = scales(go, weight)
    r64 = R.consistency(z1, z2, inv_t, batch, s64, F64)
    r32 = R.consistency(z1, z2, inv_t, batch, s32, F32)
    loss, d1, d2 = B.consistency(pad_buf(z1, ldc), pad_buf(z2, ldc), temperature, batch, classes, go, weight, which)
    G.grade(f"{tag} loss", loss, *_trip(r64, r32, "loss"))
    for name, d in (("d1", d1), ("d2", d2)):
        if name == which or which == "both":
            G.grade(f"{tag} {name}", d[:, :classes], *_trip(r64, r32, name))
            G.zero(f"{tag} {name} pad lanes", d[:, classes:])
        else:
            assert d is None
    return loss, d1, d2


def cons_pair(c):
    rng, z1, t = seg_data(c)
    if c["kind"] == "same":
        return z1, z1.copy()
    if c["kind"] == "margin200":                       # z2 certain of the label by 200: most lanes of p2 underflow to 0
        return z1, make_logits(rng, t.size, c["classes"], "margin200", t)
    return z1, (z1 + rng.standard_normal(z1.shape) * 2).astype(F32)


def run_launch_shape(B, c, log=print):
    """Every segmentation-loss kernel at one launch shape: Dice per image and pooled, focal, consistency."""
    G = R.Grader(seg_id(c), log)
    rng, z, t = seg_data(c)
    z2 = (z + rng.standard_normal(z.shape)).astype(F32)
    cw = (rng.random(c["classes"]) + 0.5).astype(F32)
    grade_dice(B, G, c, z, t, 1.0, 1e-7, False, None, 0.37, 1.7, "dice")
    grade_dice(B, G, c, z, t, 0.0, 1e-7, True, None, None, 0.6, "dice pooled")
    grade_dice(B, G, c, z, t, 1.0, 1e-7, False, 255, 0.37, 1.7, "dice ignore")
    grade_focal(B, G, c, z, t, cw, 0.25, 2.0, True, None, 0.37, f32(1.7 / t.size), "focal")
    grade_focal(B, G, c, z, t, cw, 0.25, 2.0, False, -100, None, 0.6, "focal ignore")
    grade_consistency(B, G, c, z, z2, 0.5, 0.37, 1.7, "consistency")
    G.done()
    return G


def run_focal_edge(B, c, log=print):
    G = R.Grader("focal " + seg_id(c), log)
    rng, z, t = seg_data(c)
    classes, gamma = c["classes"], c["gamma"]
    cw = (rng.random(classes) + 0.5).astype(F32)
    cw[classes // 2] = 0.0
    n = t.size
    for (go, weight), (w_, mean, alpha) in zip(UPSTREAM, [(cw, True, 0.25), (None, False, 0.5), (cw, False, 1.0)]):
        weight = f32(weight / n) if mean else weight
        grade_focal(B, G, c, z, t, w_, alpha, gamma, mean, None, go, weight, f"{'mean' if mean else 'sum'} w={'y' if w_ is not None else 'n'}")
    G.done()
    return G


def run_focal_void(B, c, log=print):
    """Void labels through the _ignore entry points, with class weights (never read at a void pixel); a label outside [0, C) there
    too, and through the plain entry points only without class weights."""
    G = R.Grader("focal " + seg_id(c), log)
    cc = dict(c, out_of_range=True)
    rng, z, t = seg_data(cc)
    cw = (rng.random(c["classes"]) + 0.5).astype(F32)
    grade_focal(B, G, c, z, t, cw, 0.25, 2.0, True, c["ignore_index"], 0.37, f32(1.7 / t.size), "ignore mean")
    grade_focal(B, G, c, z, t, None, 0.5, 0.0, False, c["ignore_index"], None, 0.6, "ignore sum gamma0")
    if c["ignore_index"] != 0:
        grade_focal(B, G, c, z, t, None, 0.5, 1.0, False, None, 1.0, 0.6, "plain entry, no weights")
    G.done()
    return G


def run_dice_edge(B, c, log=print):
    G = R.Grader("dice " + seg_id(c), log)
    rng, z, t = seg_data(c, absent=True)
    go, weight = UPSTREAM[(0.0, 0.1, 1.0).index(c["smooth"])]
    grade_dice(B, G, c, z, t, c["smooth"], 1e-7, False, None, go, weight, "per image")
    grade_dice(B, G, c, z, t, c["smooth"], 1e-7, True, None, go, weight, "pooled eps=1e-7")
    grade_dice(B, G, c, z, t, c["smooth"], 50.0, True, None, go, weight, "pooled eps=50")
    G.done()
    return G


def run_dice_void(B, c, log=print):
    G = R.Grader("dice " + seg_id(c), log)
    cc = dict(c, out_of_range=True)
    rng, z, t = seg_data(cc, absent=True)
    grade_dice(B, G, c, z, t, c["smooth"], 1e-7, False, c["ignore_index"], 0.37, 1.7, "ignore per image")
    grade_dice(B, G, c, z, t, 0.0, 1e-7, True, c["ignore_index"], None, 0.6, "ignore pooled smooth=0")
    grade_dice(B, G, c, z, t, c["smooth"], 50.0, True, c["ignore_index"], 1.0, 0.6, "ignore pooled eps=50")
    if c["ignore_index"] != 0:
        grade_dice(B, G, c, z, t, c["smooth"], 1e-7, False, None, 1.0, 0.6, "plain entry")
    G.done()
    return G


def run_consistency_edge(B, c, log=print):
    G = R.Grader("consistency " + seg_id(c), log)
    z1, z2 = cons_pair(c)
    for (go, weight), which in zip(UPSTREAM, ("both", "d1", "d2")):
        loss, d1, d2 = grade_consistency(B, G, c, z1, z2, c["temperature"], go, weight, which, which)
        if c["kind"] == "same":
            G.zero(f"{which} loss of identical inputs", loss)
            for d in (d1, d2):
                if d is not None:
                    G.zero(f"{which} gradient of identical inputs", d)
    G.done()
    return G


ACC_SHAPES = [seg_case(3, 23, 5, 7), seg_case(2, 5, 16, 17)]


def run_seg_accumulate(B, c, log=print):
    """The accumulate flags on buffers that hold seeded values, against old + plain, and the chain losses.py runs."""
    G = R.Grader("accumulate " + seg_id(c), log)
    cc = dict(c, void="random_void", ignore_index=255)
    rng, z, t = seg_data(cc)
    classes, ldc, batch, n = c["classes"], c["ldc"], c["batch"], t.size
    zbuf = pad_buf(z, ldc)
    cw = (rng.random(classes) + 0.5).astype(F32)
    old = rng.standard_normal((n, ldc)).astype(F32)
    old1 = rng.standard_normal((n, ldc)).astype(F32)
    live = R.live_mask(t, classes, 255)[0]
    for ign in (None, 255):
        tt = t if ign is not None else np.where(live, t, 0)
        wf = f32(1.7 / n)
        # dice_bwd, focal_bwd, consistency_bwd: d = product; d += old -- the product may fuse into the add
        _, _, plain = B.dice(zbuf, tt, batch, classes, 1.0, 1e-7, False, ign, 0.37, 1.7)
        _, _, acc = B.dice(zbuf, tt, batch, classes, 1.0, 1e-7, False, ign, 0.37, 1.7, old=old)
        G.within_ulp(f"dice_bwd ignore={ign}", acc, old, plain)
        fplain = B.focal_bwd(zbuf, tt, cw, 0.25, 2.0, classes, ign, 0.37, wf)
        G.within_ulp(f"focal_bwd ignore={ign}", B.focal_bwd(zbuf, tt, cw, 0.25, 2.0, classes, ign, 0.37, wf, old=old), old, fplain)
        if ign is not None:                               # a void row of an accumulating call keeps what it held, bit for bit
            G.exact("dice_bwd void rows keep old", acc[~live], old[~live])
        # focal_fwd: the loss scalar, a cast then a plain add
        v = B.focal_fwd(zbuf, tt, cw, 0.25, 2.0, True, classes, ign)
        G.exact(f"focal_fwd ignore={ign}", B.focal_fwd(zbuf, tt, cw, 0.25, 2.0, True, classes, ign, old=F32(0.8125)), F32(0.8125) + F32(v))
        # the chain of losses.py: focal_bwd(accumulate=False) then dice_bwd(accumulate=True), against the float64 sum
        _, _, chain = B.dice(zbuf, tt, batch, classes, 1.0, 1e-7, False, ign, 0.37, 1.7, old=fplain)
        legs = []
        for elem, k in ((F64, 0), (F32, 1)):
            f = R.focal(z, tt, cw, 0.25, 2.0, True, ign, scales(0.37, wf)[k], elem)["grad"]
            d = R.dice(z, tt, batch, 1.0, 1e-7, False, ign, scales(0.37, 1.7)[k], elem)["grad"]
            legs.append((f[0] + d[0], f[1] + d[1]))
        G.grade(f"focal_bwd then dice_bwd ignore={ign}", chain[:, :classes], legs[0][0], legs[1][0], legs[0][1])
        G.zero(f"chain pad lanes ignore={ign}", chain[:, classes:])
    z2 = (z + rng.standard_normal(z.shape)).astype(F32)
    z2buf = pad_buf(z2, ldc)
    _, p1, p2 = B.consistency(zbuf, z2buf, 0.7, batch, classes, 0.37, 1.7)
    _, a1, a2 = B.consistency(zbuf, z2buf, 0.7, batch, classes, 0.37, 1.7, old=(old, old1))
    G.within_ulp("consistency_bwd d1", a1, old, p1)
    G.within_ulp("consistency_bwd d2", a2, old1, p2)
    _, a1, a2 = B.consistency(zbuf, z2buf, 0.7, batch, classes, 0.37, 1.7, which="d2", old=(None, old1))
    assert a1 is None
    G.within_ulp("consistency_bwd d2 alone", a2, old1, p2)
    G.done()
    return G


# -------------------------------------------------------------------------------------------------------- cross entropy
CE_CASES = [dict(ldc=ldc, classes=cl, pixels=p, **({"size": BIG} if p > 257 else {}))
            for ldc, cl in ((24, 23), (12, 11), (40, 37), (64, 64)) for p in (257, 262_656)]


# every width of the ce_fwd / ce_bwd / ce_fwd_bwd launch ladders (ldc 4 ... 64; the tiled backward and the fused pass end at 32):
# one full 256-pixel chunk plus a ragged tail
CE_WIDTH_CASES = [dict(ldc=ldc, classes=ldc - 1, pixels=300) for ldc in range(4, 65, 4)]


def ce_id(c):
    return f"ldc{c['ldc']}-c{c['classes']}-p{c['pixels']}"


def run_ce(B, c, log=print):
    """ce_fwd + ce_bwd against float64 (upstream gradient: the null pointer, then 0.37), column sums where ldc <= 32, and the
    fused ce_fwd_bwd bit for bit against the two-pass result."""
    G = R.Grader("ce " + ce_id(c), log)
    rng = _seed(ce_id(c))
    classes, ldc, pixels = c["classes"], c["ldc"], c["pixels"]
    t = rng.integers(0, classes, pixels).astype(np.int64)
    z = make_logits(rng, pixels, classes, "randn3", t)
    z[::5] = make_logits(rng, pixels, classes, "margin20", t)[::5]
    zbuf = pad_buf(z, ldc)
    # the largest cases take one pair of references: the null-pointer gradient is then held to the fused pass bit for bit only
    for go in ((0.37,) if c.get("size") == BIG else (None, 0.37)):
        g = 1.0 if go is None else f32(go)
        r64, r32 = R.cross_entropy(z, t, g, F64), R.cross_entropy(z, t, g, F32)
        loss, lse, d, colsum = B.ce(zbuf, t, classes, go)
        G.grade(f"go={go} loss", loss, *_trip(r64, r32, "loss"))
        G.grade(f"go={go} lse", lse, *_trip(r64, r32, "lse"))
        G.grade(f"go={go} grad", d[:, :classes], *_trip(r64, r32, "grad"))
        G.zero(f"go={go} grad pad lanes", d[:, classes:])
        if ldc <= 32:
            G.grade(f"go={go} colsum", colsum[:classes], *_trip(r64, r32, "colsum"))
            G.zero(f"go={go} colsum pad lanes", colsum[classes:])
        else:
            assert colsum is None
    if ldc <= 32:
        loss, _, d, colsum = B.ce(zbuf, t, classes, None)
        loss2, _, d2, colsum2 = B.ce(zbuf, t, classes, None, fused=True)
        G.exact("ce_fwd_bwd loss", loss2, loss)
        G.exact("ce_fwd_bwd grad", d2, d)
        G.exact("ce_fwd_bwd colsum", colsum2, colsum)
    G.done()
    return G


# ------------------------------------------------------------------------------------------------------ discriminator tail
TAIL_CASES = [dict(n=n, hw=hw, c=c, **({"size": BIG} if n * hw * c > 2_000_000 else {}))
              for n, hw, c in ((1, 1, 4), (3, 1, 512), (3, 24, 4), (1, 24, 1028), (3, 32, 512), (1, 33, 1028), (3, 33, 4), (3, 4096, 4),
                               (1, 4096, 512), (3, 32, 1028))]


def tail_id(c):
    return f"n{c['n']}-hw{c['hw']}-c{c['c']}" + ("-bf16" if c.get("bf16") else "")


def run_tail(B, c, log=print):
    G = R.Grader("tail " + tail_id(c), log)
    rng = _seed(tail_id(c))
    n, hw, ch, bf = c["n"], c["hw"], c["c"], bool(c.get("bf16"))
    z = (rng.standard_normal((n, hw, ch)) + 0.25).astype(F32)
    z = R.bf16_round(z) if bf else z
    w = (rng.standard_normal(ch) * (4.0 / np.sqrt(ch))).astype(F32)
    b = np.array([0.3], dtype=F32)
    dp = (rng.standard_normal(n) + 0.1).astype(F32)
    old = (rng.standard_normal(ch).astype(F32), F32(rng.standard_normal()))
    for sigmoid in ((True,) if bf else (True, False)):
        tag = "sigmoid" if sigmoid else "linear"
        f64, f32_ = R.tail_forward(z, w, b, sigmoid, F64), R.tail_forward(z, w, b, sigmoid, F32)
        out, pooled = B.tail_fwd(z, w, b, sigmoid, bf16=bf)
        G.grade(f"{tag} pooled", pooled, *_trip(f64, f32_, "pooled"))
        G.grade(f"{tag} out", np.reshape(out, -1), *_trip(f64, f32_, "out"))
        # the backward from the forward's own outputs, as discriminator.py calls it
        b64, b32 = (R.tail_backward(dp, np.reshape(out, -1), pooled, w, hw, sigmoid, e) for e in (F64, F32))
        dz, dw, db = B.tail_bwd(dp, out, pooled, w, hw, sigmoid, bf16=bf)
        rep = lambda a: np.repeat(np.asarray(a)[:, None, :], hw, axis=1)
        G.grade(f"{tag} dz", dz, rep(b64["dz"][0]), rep(b32["dz"][0]), rep(b64["dz"][1]), bf16_out=bf)
        G.grade(f"{tag} dw", dw, *_trip(b64, b32, "dw"))
        G.grade(f"{tag} db", db, *_trip(b64, b32, "db"))
        dz2, dw2, db2 = B.tail_bwd(dp, out, pooled, w, hw, sigmoid, old=old, bf16=bf)
        G.exact(f"{tag} dz with accumulate_param", dz2, dz)
        G.exact(f"{tag} dw accumulate", dw2, old[0] + np.asarray(dw, dtype=F32))       # a finished sum, then a plain add
        G.exact(f"{tag} db accumulate", db2, F32(old[1] + F32(db)))
    G.done()
    return G


# ----------------------------------------------------------------------------------------------------------------- BCE
BCE_CASES = [dict(n=n) for n in (1, 4, 64, 65, 300)]


def run_bce(B, c, log=print):
    n = c["n"]
    G = R.Grader(f"bce n={n}", log)
    rng = _seed(f"bce{n}")
    x = (rng.standard_normal(n) * 3).astype(F32)
    x[:min(n, 4)] = np.array([-100, 30, -30, 100], dtype=F32)[:min(n, 4)]
    if n > 8:                                              # and in the last lanes of the last pass over the wavefront
        x[-2:] = (100, -100)
    y = rng.random(n).astype(F32)
    y[::3], y[1::5] = 0.0, 1.0
    old_l, old_d = F32(0.8125), rng.standard_normal(n).astype(F32)
    for (go, weight), label in zip(UPSTREAM + UPSTREAM[1:], (0.0, 1.0, 1.0, y, y)):
        tag = f"label={'vector' if np.ndim(label) else label} go={go} w={weight}"
        weight, g = f32(weight), 1.0 if go is None else f32(go)
        r64, r32 = R.bce(x, label, weight, g, F64), R.bce(x, label, weight, g, F32)
        loss, dx = B.bce_fwd(x, label, weight), B.bce_bwd(x, label, weight, go)
        G.grade(f"{tag} loss", loss, *_trip(r64, r32, "loss"))
        G.grade(f"{tag} dx", dx, *_trip(r64, r32, "dx"))
        # weight * (s / n) and (sg - y) * g are products that may fuse into the accumulating add
        G.within_ulp(f"{tag} loss accumulate", B.bce_fwd(x, label, weight, old=old_l), old_l, loss)
        G.within_ulp(f"{tag} dx accumulate", B.bce_bwd(x, label, weight, go, old=old_d), old_d, dx)
    G.done()
    return G


FAMILIES = {                               # name -> (cases, id function, runner)
    "launch": (LAUNCH_SHAPES, seg_id, run_launch_shape),
    "focal_edge": (FOCAL_EDGE, seg_id, run_focal_edge),
    "focal_void": (FOCAL_VOID, seg_id, run_focal_void),
    "dice_edge": (DICE_EDGE, seg_id, run_dice_edge),
    "dice_void": (DICE_VOID, seg_id, run_dice_void),
    "consistency_edge": (CONS_EDGE, seg_id, run_consistency_edge),
    "seg_accumulate": (ACC_SHAPES, seg_id, run_seg_accumulate),
    "ce": (CE_CASES, ce_id, run_ce),
    "ce_width": (CE_WIDTH_CASES, ce_id, run_ce),
    "tail": (TAIL_CASES + [dict(n=3, hw=24, c=512, bf16=True)], tail_id, run_tail),
    "bce": (BCE_CASES, lambda c: f"n{c['n']}", run_bce),
}
