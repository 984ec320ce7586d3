"""Float64 mirror of ``udaseg_ema_flat`` (include/udaseg.h, INTEGRATION.md "Mean teacher") in numpy: no torch op on the checked path.

``ema_ref(t, s, decay)`` -> ``(e, B)``: ``w64 = float64(float32(1 - decay))`` (the weight the kernel uses, exactly),
``e = t64 + w64 * (s64 - t64)`` and the bound per element

    B = 2^-24 * (|e| + |w64 * (s64 - t64)|) * 1.0001 + 2^-149

The kernel rounds twice: ``d = fl(s - t)`` is off by at most ``2^-24 |s - t|``, which the multiplication by ``w`` scales to
``2^-24 |w (s - t)|``; ``fmaf(w, d, t)`` rounds once more, by at most ``2^-24`` of its result, which is ``e`` up to the first error.
1.0001 covers the second-order terms, ``2^-149`` a result in the subnormal range.  Derived, not measured.
"""
import numpy as np

MAGNITUDES = (1e-6, 1e3)


def ema_weight(decay):
    return np.float64(np.float32(1.0 - np.float64(decay)))


def ema_ref(t, s, decay):
    t64, s64 = np.asarray(t, dtype=np.float64), np.asarray(s, dtype=np.float64)
    step = ema_weight(decay) * (s64 - t64)
    e = t64 + step
    return e, 2.0 ** -24 * (np.abs(e) + np.abs(step)) * 1.0001 + 2.0 ** -149


def operands(count, seed, same_share=0.0):
    """Seeded fp32 ``(t, s)``: independent signs, magnitudes log-uniform over ``MAGNITUDES`` (normal range, no zeros);
    ``same_share`` of the elements have ``s == t``."""
    rng = np.random.default_rng(seed)
    lo, hi = np.log(MAGNITUDES[0]), np.log(MAGNITUDES[1])

    def draw():
        mag = np.exp(rng.uniform(lo, hi, count))
        return np.clip(mag, *MAGNITUDES).astype(np.float32) * rng.choice(np.float32([-1, 1]), count)

    t, s = draw(), draw()
    if same_share:
        same = rng.random(count) < same_share
        s[same] = t[same]
    return t, s


def dist2_ref(s, t_new):
    d = np.asarray(s, dtype=np.float64) - np.asarray(t_new, dtype=np.float64)
    return float(np.sum(d * d))
