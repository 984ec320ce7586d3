"""numpy mirror of the Fourier style transfer (fda.py, csrc/fda.hip): the SPECIFICATION the GPU tests hold the kernels to.  It is
the original algorithm (Yang & Soatto 2020) in float64 -- full ``np.fft.fft2``, the band mask from ``np.fft.fftfreq``, the
amplitude rule ``(1-lam) |F_s| + lam |F_t|`` with the source's phase, ``ifft2(...).real`` -- plus the one defined deviation of the
contract: where ``|F_s| <= 1e-9 * 255 * H * W`` the unit phasor is 1.  Also here: the frame recipe and the cases of the tests, and
an independent partial-DFT evaluation (dense float64 matrices, no FFT) that tests/test_fda_host.py compares the mirror with."""
import functools

import numpy as np

DEGENERATE = 1e-9

# (n, h, w, b): the smallest shapes at which each mechanism can break; lam = (1.0, 0.5, 1.0)[:n]
CASES = [
    (1, 1, 1, (0,)),              # single pixel
    (2, 3, 5, (1, 0)),            # tiny, mixed bands
    (1, 16, 16, (7,)),            # K = 15 at a width of 16
    (2, 17, 31, (8, 3)),          # odd sizes; K = H exactly
    (3, 64, 48, (0, 2, 5)),       # per-sample bands; wide-store path
    (1, 257, 129, (3,)),          # scalar path; rows not a multiple of anything
    (2, 128, 128, (11, -1)),      # a copied sample
    (1, 512, 512, (46,)),         # the largest K = 93 of practical use
]
LAM = (1.0, 0.5, 1.0)
SOURCE_CAST, TARGET_CAST = (150, 90, 40), (30, 120, 230)


def case_id(case):
    n, h, w, b = case
    return f"{n}x{h}x{w}-b{'_'.join(str(v) for v in b)}"


def recipe(rng, n, h, w, cast):
    """uint8 [n,h,w,3]: noise with a colour cast that grows along the diagonal and a low-frequency wave, so that the frames have
    low-frequency content and the transfer clips on both sides (plain uniform noise has neither)."""
    noise = rng.integers(0, 96, size=(n, h, w, 3))
    yy = (np.arange(h, dtype=np.float64) / max(h - 1, 1))[None, :, None, None]
    xx = (np.arange(w, dtype=np.float64) / max(w - 1, 1))[None, None, :, None]
    c = np.asarray(cast, dtype=np.float64)[None, None, None, :]
    f = noise + c * (0.25 + 0.75 * yy * xx) + 40.0 * np.sin(2.0 * np.pi * (yy + 2.0 * xx))
    return np.clip(f, 0, 255).astype(np.uint8)


def frames(n, h, w):
    """(source, target) of a case: one generator seeded 1000 n + 10 h + w, the source drawn first."""
    rng = np.random.default_rng(1000 * n + 10 * h + w)
    return recipe(rng, n, h, w, SOURCE_CAST), recipe(rng, n, h, w, TARGET_CAST)


def band_mask(h, w, b):
    fu = np.abs(np.rint(np.fft.fftfreq(h) * h))
    fv = np.abs(np.rint(np.fft.fftfreq(w) * w))
    return (fu[:, None] <= b) & (fv[None, :] <= b)


def transfer(src, tgt, b, lam, pick=None):
    """(field float64 [n,h,w,3], the minimum of |F_s| / (255 h w) over the bands).  src, tgt: uint8 [n|m,h,w,3]; b: integers [n];
    lam: [n]; pick: the target of every sample (default i)."""
    n, h, w, _ = src.shape
    pick = np.arange(n) if pick is None else np.asarray(pick)
    out = np.empty(src.shape, dtype=np.float64)
    smallest = np.inf
    for i in range(n):
        if b[i] < 0:
            out[i] = src[i]
            continue
        mask = band_mask(h, w, int(b[i]))
        li = float(lam[i])
        for c in range(3):
            fs = np.fft.fft2(src[i, :, :, c].astype(np.float64))
            ft = np.fft.fft2(tgt[pick[i], :, :, c].astype(np.float64))
            a_s, a_t = np.abs(fs), np.abs(ft)
            degenerate = a_s <= DEGENERATE * 255.0 * h * w
            phasor = np.where(degenerate, 1.0, fs / np.where(degenerate, 1.0, a_s))
            new = np.where(mask, ((1.0 - li) * a_s + li * a_t) * phasor, fs)
            out[i, :, :, c] = np.fft.ifft2(new).real
            smallest = min(smallest, float(a_s[mask].min()) / (255.0 * h * w))
    return out, smallest


def to_u8(field):
    return np.clip(np.rint(field), 0, 255).astype(np.uint8)


def counts(field):
    """int64 [n,2]: values below 0, values above 255."""
    return np.stack([(field < 0).sum(axis=(1, 2, 3)), (field > 255).sum(axis=(1, 2, 3))], axis=1).astype(np.int64)


def near_half(field, tau):
    """Values within tau of a rounding boundary (a half-integer)."""
    return np.abs(field - np.floor(field) - 0.5) <= tau


def low_spectrum(fr, bmax):
    """complex128 [n,3,K,K]: the coefficients of u, v in [-bmax, bmax] from the full FFT."""
    f = np.fft.fft2(fr.astype(np.float64), axes=(1, 2))
    idx = np.arange(-bmax, bmax + 1)
    h, w = fr.shape[1:3]
    return np.transpose(f[:, idx % h][:, :, idx % w], (0, 3, 1, 2))


# ------------------------------------------------------------------------------ the independent evaluation: partial DFT, no FFT
def _twiddles(length, bmax):
    k = np.arange(-bmax, bmax + 1)[:, None] * np.arange(length)[None, :]
    return np.exp(-2j * np.pi * (k % length) / length)                       # [K, L], the index reduced in integers


def partial_spectrum(fr, bmax):
    h, w = fr.shape[1:3]
    return np.einsum("uy,nyxc,vx->ncuv", _twiddles(h, bmax), fr.astype(np.float64), _twiddles(w, bmax), optimize=True)


def partial_transfer(src, tgt, b, lam, pick=None):
    """The contract's own form: out = src + Re(IDFT(D)) on the bmax block, dense float64 matrices."""
    n, h, w, _ = src.shape
    pick = np.arange(n) if pick is None else np.asarray(pick)
    bmax = max(max(int(v) for v in b), 0)
    fs, ft = partial_spectrum(src, bmax), partial_spectrum(tgt, bmax)
    a_s, a_t = np.abs(fs), np.abs(ft)[pick]
    degenerate = a_s <= DEGENERATE * 255.0 * h * w
    phasor = np.where(degenerate, 1.0, fs / np.where(degenerate, 1.0, a_s))
    f = np.abs(np.arange(-bmax, bmax + 1))
    band = np.asarray(b)[:, None, None, None]
    inside = (f[None, None, :, None] <= band) & (f[None, None, None, :] <= band)
    lam = np.asarray(lam, dtype=np.float64)[:, None, None, None]
    d = np.where(inside, lam * (a_t - a_s) * phasor, 0.0) / (h * w)
    add = np.einsum("uy,ncuv,vx->nyxc", np.conj(_twiddles(h, bmax)), d, np.conj(_twiddles(w, bmax)), optimize=True).real
    return src.astype(np.float64) + add


@functools.lru_cache(maxsize=None)
def reference(case):
    """{src, tgt, b, lam, field, smallest} of a case, computed once and shared (treat the arrays as read-only)."""
    n, h, w, b = case
    src, tgt = frames(n, h, w)
    b = np.asarray(b, dtype=np.int32)
    lam = np.asarray(LAM[:n], dtype=np.float32)
    field, smallest = transfer(src, tgt, b, lam)
    for a in (src, tgt, b, lam, field):
        a.setflags(write=False)
    return {"src": src, "tgt": tgt, "b": b, "lam": lam, "field": field, "smallest": smallest}
