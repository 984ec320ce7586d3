"""Host side of the width sweeps of the class-score kernels (csrc/scores_common.h): the winner rule restated in numpy and the
seeded rows every sweep uses.  No torch, no GPU.

A kernel over a padded [pixels][ldc] score buffer is a template on its row width in 4-float vectors, ldc / 4 for the loss, confusion
and curve kernels and ceil(classes / 4) for the pseudo-label and prediction kernels, chosen at run time from eight (cross entropy:
sixteen) instantiations.  A sweep reaches every width with a graded result: 300 pixels (one full 256-pixel chunk plus a tail that is
no multiple of 4 or 64), an exact tie of the maximum between two channels at one pixel and a NaN in a channel above 0 at another.
"""
import numpy as np

PIXELS = 300
TIE_PIXEL, NAN_PIXEL = 7, 261                                    # one in the full chunk, one in the tail
SWEEP_LDC = list(range(4, 33, 4))
SWEEP_CLASSES = [c for k in range(1, 9) for c in (4 * k - 3, 4 * k)]   # both ends of every ceil(classes / 4) = 1 ... 8
PAD_JUNK = 1e4                                                   # larger than any score: a pad lane that is read wins


def first_max(rows):
    """[P, C] -> [P] int64: channel 0 seeds the maximum, a later channel takes over only if it is strictly greater -- the first
    maximal index of torch.argmax, with a NaN beyond channel 0 stepped over (no comparison with a NaN is true)."""
    rows = np.asarray(rows)
    m = rows[:, 0].copy()
    am = np.zeros(len(rows), dtype=np.int64)
    for c in range(1, rows.shape[1]):
        with np.errstate(invalid="ignore"):
            g = rows[:, c] > m
        m[g] = rows[g, c]
        am[g] = c
    return am


def tie_channels(classes):
    return (classes - 1) // 2, classes - 1


def sweep_rows(classes, seed, scale=3.0, nan=True):
    """[PIXELS, classes] fp32 randn x scale.  From two classes on: at TIE_PIXEL two channels share the maximum (the lower index must
    win), and with ``nan`` the last channel of NAN_PIXEL is NaN."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((PIXELS, classes)) * scale).astype(np.float32)
    if classes >= 2:
        lo, hi = tie_channels(classes)
        z[TIE_PIXEL, lo] = z[TIE_PIXEL, hi] = z[TIE_PIXEL].max() + np.float32(1.0)
        if nan:
            z[NAN_PIXEL, classes - 1] = np.nan
    return z


def padded(rows, ldc, junk=PAD_JUNK):
    """[P, C] -> [P, ldc] fp32 with ``junk`` in the pad lanes."""
    p, c = rows.shape
    buf = np.full((p, ldc), junk, dtype=np.float32)
    buf[:, :c] = rows
    return buf
