"""Fourier-domain style transfer of labelled source frames to the style of target frames, on the device: input-space adaptation,
the step before "augment and train" (``data.DeviceAugmentedLoader``) or before mixing (``mix.MixedLoader``).  An EXTENSION: the
reference has no counterpart.  The method is Fourier Domain Adaptation (Yang & Soatto 2020): replace the low-frequency
amplitude of a source frame's spectrum by a target frame's, keep the source's phase, transform back; with ``lam < 1`` the
amplitudes are mixed (Xu et al. 2021).  Labels are untouched.

The usual implementation is two ``fft2`` and an ``ifft2`` per frame and channel plus ``abs``, ``angle``, ``fftshift`` and a slice
assignment.  This library links no FFT and needs none, because only the ``(2b+1) x (2b+1)`` lowest frequencies change::

    out = src + Re(IDFT(D)),   D[u][v] = lam * (|F_t[u][v]| - |F_s[u][v]|) * F_s[u][v] / |F_s[u][v]|  for |u|, |v| <= b, else 0

and ``F_s``, ``F_t`` are needed on that block alone: a separable partial DFT ``W_r (K x H) . X (H x W) . W_c^T (W x K)`` with
``K = 2b+1``, exact for any ``H, W``.  Three kernels (``csrc/fda.hip``): ``udaseg_fda_spectrum_u8`` (frames -> coefficients),
``udaseg_fda_delta`` (-> ``D``; its companion ``udaseg_fda_amplitude`` makes the target side's table) and ``udaseg_fda_apply_u8``
(the streaming pass that writes the frames).  Nothing is read back from the device.

The contract

Frames are uint8 ``[N,H,W,3]``.  Sample ``i`` has a band half-width ``b[i]`` (int32) and a strength ``lam[i]`` (float32 in [0,1]).
    Band: ``-1 <= b[i] <= (min(H,W)-1)//2``.  ``b[i] = -1`` copies the source sample unchanged; ``b[i] = 0`` transfers the channel
    means only.  The band is the frequencies ``u in [-b, b]``, ``v in [-b, b]``: the ``fftshift``-centred square of the original
    code at centre ``(H//2, W//2)``.  From a band fraction: ``b = floor(min(H,W) * beta)`` as in the original (``band_of``, which
    also caps it at ``(min(H,W)-1)//2``).
    New amplitude inside the band: ``(1-lam) * |F_s| + lam * |F_t|``.  ``lam = 1`` is FDA, ``lam < 1`` the amplitude mix.
    Phase: the source's.
    Degenerate coefficient -- a DEFINED DEVIATION from the original, which leaves it to ``atan2`` of rounding noise: where
    ``|F_s[u][v]| <= 1e-9 * 255 * H * W`` the phase is taken as 0, the unit phasor as 1.
    Float output (``dtype=torch.float32``): the real field itself, float32 ``[N,H,W,3]``.
    uint8 output: the field rounded half to even, then clamped to ``[0, 255]``.
    ``counts``: int64 ``[N,2]``, ACCUMULATES across calls like every counter table of this library; ``[0]`` the values of the
    field below 0, ``[1]`` the values above 255 (before the rounding and the clamp), each counted per channel value.

Numerics.  The analysis (both forward stages and everything up to ``D``) accumulates in float64 from the exact integer pixels and
float64 twiddles; the synthesis (``D`` to pixels) is float32.  Twiddles come from tables ``(cos, sin)(2 pi k / L)``, ``k in [0, L)``
for ``L = H`` and ``L = W``, built on the host in float64 (the synthesis takes their float32 roundings), indexed by ``(u * y) mod L``
in integers: there is no device ``sincos`` of a large argument.

Draws (host, from the caller's CPU ``torch.Generator``):
    ``draw_bands``: ``u = torch.rand(n, 2, generator=g, dtype=torch.float64)``; ``beta = lo + u[:,0] * (hi - lo)``;
    ``b = band_of(beta, h, w)``; the sample gets ``-1`` where ``u[:,1] >= p``.
    ``draw_strengths``: ``u = torch.rand(n, generator=g, dtype=torch.float64)``; ``lam = float32(lo + u * (hi - lo))``.
    ``AmplitudeBank.draw``: ``torch.randint(0, len(bank), (n,), generator=g, dtype=torch.int64)`` as int32.

Use::

    bank = fda.AmplitudeBank(bmax=fda.band_of(0.05, 512, 512), capacity=4096).fit(target_loader_u8)
    styled = fda.StyledLoader(source_loader_u8, bank, beta=(0.01, 0.05), generator=g)       # (frames u8, masks u8)
    loader = data.DeviceAugmentedLoader(styled, generator=g)
    SegmentationTrainer(model, dev).train_epoch(loader, opt, epoch)
"""
import math

import numpy as np
import torch

from . import _args as A
from . import kernels as K


def _check_pair(name, pair, lo_min, hi_max):
    return A.pair("fda", name, pair, lo_min, hi_max)


def _check_size(name, v, least=1):
    return A.int_in("fda", name, v, least)


def _check_p(p):
    if not isinstance(p, (int, float)):
        raise ValueError(f"fda: p must be a probability, got {p!r}")
    return A.number("fda", "p", p, 0.0, 1.0)


def max_band(h, w):
    """The largest band half-width of an ``h x w`` frame: ``(min(h, w) - 1) // 2``."""
    return (min(_check_size("h", h), _check_size("w", w)) - 1) // 2


def band_of(beta, h, w):
    """``floor(min(h, w) * beta)`` (the original's rule) capped at ``max_band(h, w)``; ``0 <= beta <= 0.5``.  Needs no GPU."""
    cap = max_band(h, w)
    return min(int(math.floor(min(h, w) * A.number("band_of", "beta", beta, 0.0, 0.5))), cap)


def draw_bands(n, h, w, generator=None, beta=(0.01, 0.05), p=1.0):
    """int32 ``[n]`` host tensor of band half-widths for ``h x w`` frames: the band fraction uniform in ``beta``, ``-1`` (copy the
    sample) with probability ``1 - p`` (the module docstring has the draw).  Needs no GPU."""
    n = _check_size("n", n)
    cap = max_band(h, w)
    lo, hi = _check_pair("beta", beta, 0.0, 0.5)
    p = _check_p(p)
    u = torch.rand(n, 2, generator=generator, dtype=torch.float64).numpy()
    b = np.minimum(np.floor(min(h, w) * (lo + u[:, 0] * (hi - lo))), cap).astype(np.int32)
    b[u[:, 1] >= p] = -1
    return torch.from_numpy(b)


def draw_strengths(n, generator=None, lam=(1.0, 1.0)):
    """float32 ``[n]`` host tensor of strengths uniform in ``lam`` (the module docstring has the draw).  Needs no GPU."""
    n = _check_size("n", n)
    lo, hi = _check_pair("lam", lam, 0.0, 1.0)
    u = torch.rand(n, generator=generator, dtype=torch.float64).numpy()
    return torch.from_numpy((lo + u * (hi - lo)).astype(np.float32))


def _tables(length, dev):
    """(float64 [L,2], float32 [L,2]) device tables of (cos, sin)(2 pi k / L), made once per length and device on the host."""
    def make():
        ang = 2.0 * np.pi * np.arange(length, dtype=np.float64) / length
        t64 = np.stack([np.cos(ang), np.sin(ang)], axis=1)
        return t64, t64.astype(np.float32)
    return A.const_table("fda", length, make, dev)


def _frames_shape(who, name, t):
    return A.frames_u8(who, t, name=name, below_2_31=True)


def _check_bmax(who, bmax, h, w):
    return A.int_in(who, f"bmax (for {h} x {w} frames)", bmax, 0, max_band(h, w))


def _vector(who, name, t, dtype, n, lo, hi):
    """A ``[n]`` tensor of ``dtype``; a host tensor's values are checked against ``[lo, hi]``, a device tensor is the caller's word
    (no read-back: the kernels clamp what could index out of bounds)."""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (n,):
        raise ValueError(f"{who}: {name} must be a {dtype} [{n}] tensor, got {getattr(t, 'dtype', type(t).__name__)} "
                         f"{list(getattr(t, 'shape', ()))}")
    if not t.is_cuda and n:
        v = t.numpy()
        if not ((v >= lo) & (v <= hi)).all():
            raise ValueError(f"{who}: {name} must lie in [{lo}, {hi}], got {v.tolist()}")
    return t


def low_spectrum(frames_u8, bmax):
    """float64 ``[N,3,K,K,2]`` on the device, ``K = 2*bmax+1``: the coefficients ``(re, im)`` of the frequencies ``u, v in [-bmax,
    bmax]`` (index ``u + bmax``, ``v + bmax``) of every channel of uint8 ``[N,H,W,3]`` frames.  A host tensor is moved with one
    asynchronous copy; no synchronisation."""
    n, h, w = _frames_shape("low_spectrum", "frames", frames_u8)
    bmax = _check_bmax("low_spectrum", bmax, h, w)
    dev = A.current_gpu()
    frames = frames_u8.to(dev, non_blocking=True).contiguous()
    k = 2 * bmax + 1
    rows = torch.empty((n, 3, h, k, 2), dtype=torch.float64, device=dev)
    coeffs = torch.empty((n, 3, k, k, 2), dtype=torch.float64, device=dev)
    A.on_device(dev, K.fda_spectrum_u8, frames, _tables(h, dev)[0], _tables(w, dev)[0], n, h, w, bmax, rows, coeffs)
    return coeffs


def amplitudes(frames_u8, bmax, out=None):
    """float64 ``[N,3,K,K]`` on the device: ``|F|`` of ``low_spectrum(frames_u8, bmax)``, what ``transfer`` takes as a target.
    ``out``: a contiguous device tensor of that shape to write into (rows of an ``AmplitudeBank``)."""
    coeffs = low_spectrum(frames_u8, bmax)
    out = A.out_tensor("amplitudes", "out", out, coeffs.shape[:4], torch.float64, coeffs.device, contiguous=True)
    A.on_device(coeffs.device, K.fda_amplitude, coeffs, out.numel(), out)
    return out


def transfer(src_frames, tgt_frames_or_amps, b, lam=None, pick=None, out=None, counts=None, dtype=torch.uint8, bmax=None):
    """``(frames, counts)`` on the device: the source frames (uint8 ``[N,H,W,3]``) in the style of the targets.

    ``tgt_frames_or_amps``: uint8 target frames ``[M,H,W,3]``, a float64 amplitude table ``[M,3,K,K]`` (``amplitudes``) or an
    ``AmplitudeBank``; ``pick`` (int32 ``[N]``, default ``0 .. N-1``) names the target row that styles each sample.  ``b``: int32
    ``[N]`` band half-widths, ``-1`` copies the sample; ``lam``: float32 ``[N]`` in [0, 1], default all 1.  The block of frequencies
    the kernels work on is ``bmax``: ``(K-1)//2`` of a table or bank; with target frames the keyword, or ``max(b)`` of a host ``b``
    (a device ``b`` is not read back: give ``bmax``).  Host tensors are moved with one asynchronous copy each, and the values of
    host ``b``, ``lam`` and ``pick`` are checked; device tables are the caller's word (the kernels clamp ``b`` and ``pick``).
    ``out``: a contiguous device tensor of the result's shape and dtype to write into (rows of a larger batch); ``counts``: a
    device int64 ``[N,2]`` table to accumulate into, None for a fresh zeroed one, False to keep none.  ``dtype``: ``torch.uint8``
    (rounded and clamped) or ``torch.float32`` (the real field)."""
    who = "transfer"
    n, h, w = _frames_shape(who, "src_frames", src_frames)
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"transfer: dtype must be torch.uint8 or torch.float32, got {dtype}")
    target = tgt_frames_or_amps.table() if isinstance(tgt_frames_or_amps, AmplitudeBank) else tgt_frames_or_amps
    if not torch.is_tensor(target):
        raise ValueError(f"transfer: the target must be uint8 frames, a float64 amplitude table or an AmplitudeBank, got "
                         f"{type(target).__name__}")
    if target.dtype == torch.float64:
        if target.dim() != 4 or target.shape[0] < 1 or target.shape[1] != 3 or target.shape[2] != target.shape[3] or target.shape[2] % 2 != 1:
            raise ValueError(f"transfer: an amplitude table must be float64 [M,3,K,K] with M >= 1 and K odd, got {list(target.shape)}")
        kmax = (int(target.shape[2]) - 1) // 2
        if bmax is not None and bmax != kmax:
            raise ValueError(f"transfer: bmax={bmax} does not match the amplitude table's {kmax}")
        bmax = _check_bmax(who, kmax, h, w)
        m = int(target.shape[0])
    else:
        m, ht, wt = _frames_shape(who, "target frames", target)
        if (ht, wt) != (h, w):
            raise ValueError(f"transfer: source frames are {h} x {w}, target frames {ht} x {wt}")
        if bmax is None:
            if not torch.is_tensor(b) or b.is_cuda:
                raise ValueError("transfer: with target frames and a band table on the device, bmax is required (no read-back)")
            bmax = max(int(b.numpy().max()), 0) if b.numel() else 0
        bmax = _check_bmax(who, bmax, h, w)
    _vector(who, "b", b, torch.int32, n, -1, bmax)
    if lam is None:
        lam = torch.from_numpy(np.ones(n, dtype=np.float32))
    _vector(who, "lam", lam, torch.float32, n, 0.0, 1.0)
    if pick is None:
        if m < n:
            raise ValueError(f"transfer: {n} source samples but {m} target rows and no pick")
        pick = torch.from_numpy(np.arange(n, dtype=np.int32))
    _vector(who, "pick", pick, torch.int32, n, 0, m - 1)
    dev = A.current_gpu()
    mv = lambda t: t.to(dev, non_blocking=True).contiguous()      # noqa: E731
    src, b, lam, pick = mv(src_frames), mv(b), mv(lam), mv(pick)
    out = A.out_tensor(who, "out", out, (n, h, w, 3), dtype, dev, contiguous=True)
    if counts is None:
        counts = K.zeros((n, 2), torch.int64, dev)
    elif counts is False:
        counts = None
    else:
        A.counts_tensor(who, "counts", counts, (n, 2), dev)
    amps = mv(target) if target.dtype == torch.float64 else amplitudes(target, bmax)
    k = 2 * bmax + 1
    coeffs = low_spectrum(src, bmax)
    delta = torch.empty((n, 3, k, k, 2), dtype=torch.float32, device=dev)
    A.on_device(dev, K.fda_delta, coeffs, amps, pick, b, lam, n, m, h, w, bmax, delta)
    cols = torch.empty((n, 3, k, w, 2), dtype=torch.float32, device=dev)
    u8 = dtype == torch.uint8
    A.on_device(dev, K.fda_apply_u8, src, delta, b, _tables(h, dev)[1], _tables(w, dev)[1], n, h, w, bmax, cols,
                out if u8 else None, None if u8 else out, counts)
    return out, counts


class AmplitudeBank:
    """Low-frequency amplitudes of up to ``capacity`` target frames on the device: float64 ``[capacity,3,K,K]``, ``K = 2*bmax+1``
    (a row is ``3*K*K`` doubles, so thousands of target frames fit in a few MB).  With a bank, source-only training phases need no
    target loader at step time.  ``add(frames)`` appends the amplitudes of uint8 ``[N,H,W,3]`` frames (all of one ``H x W``; frames
    past the capacity are dropped) and returns how many rows it took; ``fit(loader)`` adds every batch of a loader of frames or
    ``(frames, ...)`` tuples until the bank is full; ``draw(n, generator)`` returns an int32 ``[n]`` host ``pick``; ``table()`` the
    filled rows."""

    def __init__(self, bmax, capacity):
        self.bmax = _check_size("bmax", bmax, 0)
        self.capacity = _check_size("capacity", capacity)
        self.size = None                      # (H, W) of the frames, fixed by the first add
        self._amps = None
        self._len = 0

    def __len__(self):
        return self._len

    def add(self, frames):
        n, h, w = _frames_shape("AmplitudeBank.add", "frames", frames)
        if self.size is None:
            _check_bmax("AmplitudeBank", self.bmax, h, w)
            k = 2 * self.bmax + 1
            self._amps = torch.empty((self.capacity, 3, k, k), dtype=torch.float64, device=A.current_gpu())
            self.size = (h, w)
        elif self.size != (h, w):
            raise ValueError(f"AmplitudeBank.add: the bank holds {self.size[0]} x {self.size[1]} frames, got {h} x {w}")
        take = min(n, self.capacity - self._len)
        if take > 0:
            amplitudes(frames[:take], self.bmax, out=self._amps[self._len:self._len + take])
            self._len += take
        return take

    def fit(self, target_loader):
        for batch in target_loader:
            if self._len >= self.capacity:
                break
            self.add(batch if torch.is_tensor(batch) else batch[0])
        return self

    def table(self):
        if not self._len:
            raise ValueError("AmplitudeBank: the bank is empty")
        return self._amps[:self._len]

    def draw(self, n, generator=None):
        if not self._len:
            raise ValueError("AmplitudeBank: the bank is empty")
        pick = torch.randint(0, self._len, (_check_size("n", n),), generator=generator, dtype=torch.int64)
        return pick.to(torch.int32)


class StyledLoader:
    """Wraps a source loader of uint8 ``(frames [N,H,W,3], masks [N,H,W])`` batches and yields ``(frames_u8, masks_u8)`` device
    batches, the frames in the style of targets, the masks passed through: what ``data.DeviceAugmentedLoader`` or
    ``mix.MixedLoader`` wraps.

    ``target``: a loader of uint8 frames (or ``(frames, masks)`` pairs), zipped with the source as ``mix.MixedLoader`` zips (the
    length is the shorter loader's; a target batch must hold at least as many frames as the source batch, sample ``i`` takes
    target ``i``), or an ``AmplitudeBank`` (the length is the source's; every sample draws a bank row).  Different ``H, W`` raise
    ``ValueError``.  Per batch the ``generator`` (a CPU ``torch.Generator``) is consumed in a fixed order: the bands
    (``draw_bands`` with ``beta`` and ``p``), the strengths (``draw_strengths`` with ``lam``), then, with a bank, the pick
    (``AmplitudeBank.draw``).  The kernels work on the block of ``bmax = band_of(beta[1], H, W)``, or the bank's, which must be
    at least that.  ``last_bands`` (int32 ``[N]``) and ``last_counts`` (int64 ``[N,2]``) are the device tensors of the latest
    batch, for logging; nothing is read back here."""

    def __init__(self, source_loader, target, beta=(0.01, 0.05), lam=(1.0, 1.0), p=1.0, generator=None):
        self.beta = _check_pair("beta", beta, 0.0, 0.5)
        self.lam = _check_pair("lam", lam, 0.0, 1.0)
        self.p = _check_p(p)
        self.source_loader, self.target, self.generator = source_loader, target, generator
        self.last_bands = self.last_counts = None

    def __len__(self):
        if isinstance(self.target, AmplitudeBank):
            return len(self.source_loader)
        return min(len(self.source_loader), len(self.target))

    def __iter__(self):
        dev = A.current_gpu()
        bank = self.target if isinstance(self.target, AmplitudeBank) else None
        pairs = ((s, None) for s in self.source_loader) if bank is not None else zip(self.source_loader, self.target)
        for source, target in pairs:
            if torch.is_tensor(source) or len(source) != 2:
                raise ValueError("StyledLoader: a source batch must be a (frames, masks) pair")
            frames, masks = source
            n, h, w = _frames_shape("StyledLoader", "source frames", frames)
            if not torch.is_tensor(masks) or masks.dtype != torch.uint8 or tuple(masks.shape) != (n, h, w):
                raise ValueError(f"StyledLoader: source masks must be uint8 [{n}, {h}, {w}], got "
                                 f"{getattr(masks, 'dtype', type(masks).__name__)} {list(getattr(masks, 'shape', ()))}")
            bmax = band_of(self.beta[1], h, w)
            if bank is not None:
                if bank.size is not None and bank.size != (h, w):
                    raise ValueError(f"StyledLoader: source frames are {h} x {w}, the bank's {bank.size[0]} x {bank.size[1]}")
                if bank.bmax < bmax:
                    raise ValueError(f"StyledLoader: beta up to {self.beta[1]} needs bmax >= {bmax}, the bank has {bank.bmax}")
                tgt = bank
            else:
                tgt = target if torch.is_tensor(target) else target[0]
                nt, ht, wt = _frames_shape("StyledLoader", "target frames", tgt)
                if (ht, wt) != (h, w):
                    raise ValueError(f"StyledLoader: source frames are {h} x {w}, target frames {ht} x {wt}")
                if nt < n:
                    raise ValueError(f"StyledLoader: a target batch of {nt} frames for {n} source samples")
            b = draw_bands(n, h, w, self.generator, self.beta, self.p)
            lam = draw_strengths(n, self.generator, self.lam)
            pick = bank.draw(n, self.generator) if bank is not None else None
            b = b.to(dev, non_blocking=True)
            styled, counts = transfer(frames, tgt, b, lam, pick, bmax=None if bank is not None else bmax)
            self.last_bands, self.last_counts = b, counts
            yield styled, masks.to(dev, non_blocking=True)
