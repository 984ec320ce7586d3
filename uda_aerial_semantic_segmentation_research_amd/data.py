"""Device-side input pipeline: decoded uint8 batches -> model input, on the GPU.

Upstream does this per sample on the host: ``cv2`` decode -> albumentations pipeline -> ``ToTensorV2``
(reference ``src/data/dataset.py:116-138``, ``src/models/augmentation.py:8-38``).  The parts with an exact definition
move to one HIP kernel (csrc/data_prep.hip): the D4 geometric augmentations (``RandomRotate90``, ``Flip``, ``Transpose``;
image and mask together), ``A.Normalize()`` and the layout change -- the output is already the channel-padded NHWC tensor
the stem convolution reads, handed to ``Unet`` as an ``[N,3,H,W]``-shaped view (no further copy).
``prepare_batch`` stops there.  The rest of that basic pipeline (noise, blur, shift-scale-rotate, optical / grid / elastic
distortion, CLAHE / sharpen / emboss / brightness-contrast, HSV) runs on the device too, through ``train_batch``
(csrc/augment.hip, csrc/elastic_field.hip): uint8 frames and uint8 masks in, augmented model input and int64 masks out, image and mask carried
through the same geometry, from a pipeline this build defines itself ("Training augmentation") with all
randomness except the per-pixel Philox streams drawn on the host by ``draw_training_params``.  ``DeviceAugmentedLoader`` wraps
a loader of uint8 batches so that ``SegmentationTrainer`` / ``AdversarialTrainer`` consume it as they are.

Phase 3 (``src/models/unsupervised_trainer.py:100-114``) needs two STRONGLY augmented views of every unlabelled batch
(``augmentation.py:40-88``); ``strong_views`` makes both on the device from a pipeline this build defines itself (INTEGRATION.md,
"Phase 3": D4, Gaussian noise, blur, shift-scale-rotate, CLAHE / sharpen / emboss / brightness-contrast, HSV shift, Normalize;
csrc/augment.hip, csrc/clahe.hip), with all randomness except the per-pixel noise drawn on the host by ``draw_strong_params``.
"""
import ctypes

import torch

from . import _lib
from ._lib import check
from ._operands import ops
from .engine import mark_padded_input

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # A.Normalize() defaults
IMAGENET_STD = (0.229, 0.224, 0.225)

# D4 code bits (see include/udaseg.h): out = fliph^b2(flipv^b1(transpose^b0(in)))
TRANSPOSE, FLIP_ROWS, FLIP_COLS = 1, 2, 4


def _apply_code(code, y, x, n):
    """Source coordinate read by output (y, x) of an n x n image under ``code``."""
    if code & FLIP_ROWS:
        y = n - 1 - y
    if code & FLIP_COLS:
        x = n - 1 - x
    return (x, y) if code & TRANSPOSE else (y, x)


def _code_of(fn):
    """The D4 code whose gather equals ``fn`` (a function on index grids), found on a 3 x 3 probe."""
    import numpy as np
    probe = np.arange(9).reshape(3, 3)
    want = fn(probe)
    for code in range(8):
        got = np.array([[probe[_apply_code(code, y, x, 3)] for x in range(3)] for y in range(3)])
        if np.array_equal(got, want):
            return code
    raise AssertionError("not a D4 element")


def compose_d4(rot90_k=0, flip=None, transpose=False):
    """D4 code of the basic pipeline's geometric steps in upstream's order (``augmentation.py:11-13``):
    ``np.rot90(img, rot90_k)`` (RandomRotate90), then ``cv2.flip(img, flip)`` for flip in {0: rows, 1: columns, -1: both}
    (Flip), then ``img.transpose(1, 0, 2)`` (Transpose)."""
    import numpy as np

    def fn(a):
        a = np.rot90(a, rot90_k % 4)
        if flip is not None:
            a = {0: a[::-1, :], 1: a[:, ::-1], -1: a[::-1, ::-1]}[flip]
        return a.T if transpose else a
    return _code_of(fn)


_COMPOSED = {}


def random_d4_codes(n, generator=None, p_rot90=0.5, p_flip=0.5, p_transpose=0.5):
    """One D4 code per sample, drawn with the basic training pipeline's branch probabilities (each step applied with
    p = 0.5; rotation factor uniform in {0..3}; flip code uniform in {-1, 0, 1}).  int32 CPU tensor."""
    g = generator
    u = torch.rand(n, 3, generator=g)
    k = torch.randint(0, 4, (n,), generator=g)
    d = torch.randint(-1, 2, (n,), generator=g)
    codes = []
    for i in range(n):
        key = (int(k[i]) if u[i, 0] < p_rot90 else 0, int(d[i]) if u[i, 1] < p_flip else None, bool(u[i, 2] < p_transpose))
        if key not in _COMPOSED:
            _COMPOSED[key] = compose_d4(*key)
        codes.append(_COMPOSED[key])
    return torch.tensor(codes, dtype=torch.int32)


def normalize_constants(mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0):
    """A.Normalize's two fp32 vectors as host arrays for the kernels: mean*max_pixel_value and reciprocal(std*max_pixel_value),
    both rounded to fp32 first."""
    f3 = ctypes.c_float * 3
    m255 = f3(*[float(torch.tensor(m, dtype=torch.float32) * max_pixel_value) for m in mean])
    r255 = f3(*[float(1.0 / (torch.tensor(s, dtype=torch.float32) * max_pixel_value)) for s in std])
    return m255, r255


def _check_frames(who, images_u8, masks_u8=None, dtype=torch.float32):
    """The checks every entry point makes of (frames, masks, output dtype), arguments that are no tensors included -> n, h, w."""
    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"{who}: images must be uint8 [N,H,W,3], got {getattr(images_u8, 'dtype', type(images_u8))} "
                         f"{tuple(getattr(images_u8, 'shape', ()))}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{who}: dtype must be torch.float32 or torch.bfloat16")
    n, h, w, _ = images_u8.shape
    if masks_u8 is not None and (not torch.is_tensor(masks_u8) or masks_u8.dtype != torch.uint8 or tuple(masks_u8.shape) != (n, h, w)):
        raise ValueError(f"{who}: masks must be uint8 [{n},{h},{w}], got {getattr(masks_u8, 'dtype', type(masks_u8))} "
                         f"{tuple(getattr(masks_u8, 'shape', ()))}")
    return n, h, w


def _device_batch(images_u8, masks_u8, records, n, h, w, dtype, views=1):
    """The device side of a call: frames, masks and ``records`` (the parameter table or the D4 codes; masks and records may be
    None) moved with one async copy each -- all copies go out before anything is allocated, so that they run meanwhile -- then
    the channel padding of ``dtype`` and the unwritten outputs: ``views`` x N padded NHWC images in one buffer and the int64
    masks (None without masks).  -> (device, frames, masks, records, cpad, images out, masks out)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    img = images_u8.to(dev, non_blocking=True).contiguous()
    msk = None if masks_u8 is None else masks_u8.to(dev, non_blocking=True).contiguous()
    rec = None if records is None else records.to(dev, non_blocking=True).contiguous()
    cpad = 8 if dtype == torch.bfloat16 else 4
    out = torch.empty((views * n, h, w, cpad), device=dev, dtype=dtype)
    out_m = None if msk is None else torch.empty((n, h, w), device=dev, dtype=torch.int64)
    return dev, img, msk, rec, cpad, out, out_m


def _model_input(out):
    """A padded NHWC buffer ``[N,H,W,cpad]`` as the model takes it: registered for the stem convolution to read in place, handed
    out as its ``[N,3,H,W]``-shaped view."""
    mark_padded_input(out)
    return out.permute(0, 3, 1, 2)[:, :3]


def prepare_batch(images_u8, masks_u8=None, d4_codes=None, dtype=torch.float32, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                  max_pixel_value=255.0):
    """images_u8 ``[N,H,W,3]`` uint8 (RGB, as decoded), masks_u8 ``[N,H,W]`` uint8 or None, d4_codes ``[N]`` int32 or None
    -> (images ``[N,3,H,W]``-shaped view of the padded NHWC buffer in ``dtype``, masks ``[N,H,W]`` int64 or None).
    Inputs may live on the host (moved with one async copy each) or on the GPU."""
    _lib.require_gpu()
    n, h, w = _check_frames("prepare_batch", images_u8, masks_u8, dtype)
    square_ok = 0
    if d4_codes is not None:
        if d4_codes.dtype != torch.int32 or tuple(d4_codes.shape) != (n,):
            raise ValueError("prepare_batch: d4_codes must be int32 [N]")
        if h != w:
            if d4_codes.device.type != "cpu":
                raise ValueError("prepare_batch: non-square images need host-side d4_codes (to rule out transposes)")
            if bool((d4_codes & TRANSPOSE).any()):
                raise ValueError("prepare_batch: transposing D4 codes need square images")
            square_ok = 1
    _, img, msk, codes, cpad, out, out_m = _device_batch(images_u8, masks_u8, d4_codes, n, h, w, dtype)
    m255, r255 = normalize_constants(mean, std, max_pixel_value)
    check(ops.udaseg_prepare_batch_u8(img, msk, codes, n, h, w, m255, r255, out, cpad, int(dtype == torch.bfloat16), out_m, square_ok,
                                      None), "prepare_batch_u8")
    return _model_input(out), out_m


def synthetic_u8_batch(n, h, w, classes=23, seed=0, device="cuda"):
    """Seeded uint8 images / masks generated on the device (bench / smoke input: no dataset ships with the build)."""
    g = torch.Generator(device=device).manual_seed(seed)
    images = torch.randint(0, 256, (n, h, w, 3), generator=g, device=device, dtype=torch.uint8)
    masks = torch.randint(0, classes, (n, h, w), generator=g, device=device, dtype=torch.uint8)
    return images, masks


# ----------------------------------------------------------------------------------------------- strong augmentation (phase 3)
# Flag bits and record words of udaseg_strong_aug_u8 (include/udaseg.h); the pipeline is defined in INTEGRATION.md, "Phase 3".
SA_WORDS = 32
SA_NOISE, SA_BLUR, SA_AFFINE, SA_STAGE5, SA_HSV = 1, 2, 4, 8, 16
BLUR_BOX, BLUR_MEDIAN, BLUR_MOTION = 0, 1, 2
STAGE5_SHARPEN, STAGE5_EMBOSS, STAGE5_BRIGHTNESS_CONTRAST = 0, 1, 2
STAGE5_CLAHE = 3                           # stage 5's fourth child: its own setter (set_clahe), its own pass and entry points
CLAHE_GRID, CLAHE_LUT_BYTES = 8, 8 * 8 * 256
(_W_FLAGS, _W_D4, _W_BLUR_KIND, _W_BLUR_K, _W_MOTION_DIR, _W_S5_KIND, _W_KEY, _W_SIGMA, _W_AFFINE, _W_S5_PARAMS, _W_HSV,
 _W_NOOP_DISTORT, _W_NOOP_CLAHE) = 0, 1, 2, 3, 4, 5, 6, 8, 9, 15, 17, 20, 21


def inverse_affine(h, w, shift_x=0.0, shift_y=0.0, scale=1.0, angle_deg=0.0):
    """The 2 x 3 map from an output pixel to its source position for: rotate by ``angle_deg`` and scale by ``scale`` about the
    frame centre ``((w-1)/2, (h-1)/2)``, then shift by (``shift_x``, ``shift_y``) pixels.  Composed in float64; six numbers,
    row-major."""
    import math
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    a = math.radians(angle_deg)
    c, s = math.cos(a) / scale, math.sin(a) / scale
    # forward: p' = C + scale * R (p - C) + t  =>  p = C + R^T (p' - C - t) / scale
    m = [c, s, 0.0, -s, c, 0.0]
    m[2] = cx - (m[0] * (cx + shift_x) + m[1] * (cy + shift_y))
    m[5] = cy - (m[3] * (cx + shift_x) + m[4] * (cy + shift_y))
    return m


class StrongAugParams:
    """One parameter record per sample for ``strong_views``: an int32 ``[n, 32]`` host table (floats stored as their bit patterns,
    layout in include/udaseg.h).  A fresh object has every stage off and the identity D4 code; the ``set_*`` methods switch
    one stage of one sample on, ``draw_strong_params`` fills a table with the reference pipeline's branch probabilities."""

    WORDS = SA_WORDS

    def __init__(self, n, h, w, d4_codes=None):
        import numpy as np
        self.n, self.h, self.w = int(n), int(h), int(w)
        self._i = np.zeros((self.n, self.WORDS), dtype=np.int32)
        self._f = self._i.view(np.float32)
        self._f[:, _W_AFFINE + 0] = 1.0
        self._f[:, _W_AFFINE + 4] = 1.0
        if d4_codes is not None:
            self._i[:, _W_D4] = np.asarray(d4_codes, dtype=np.int32).reshape(self.n)
        self.any_clahe = False                               # whether a record is on CLAHE, as of the last check()

    # ---- one stage of one sample
    def set_d4(self, i, code):
        self._i[i, _W_D4] = int(code)

    def set_noise(self, i, sigma, key):
        """``key``: the two 32-bit Philox key words."""
        self._i[i, _W_FLAGS] |= SA_NOISE
        self._f[i, _W_SIGMA] = sigma
        self._i.view("uint32")[i, _W_KEY:_W_KEY + 2] = [int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF]

    def set_blur(self, i, kind, k, direction=0):
        if kind not in (BLUR_BOX, BLUR_MEDIAN, BLUR_MOTION) or k not in (3, 5) or direction not in (0, 1, 2, 3):
            raise ValueError("set_blur: kind in {0 box, 1 median, 2 motion}, k in {3, 5}, direction in 0..3")
        self._i[i, _W_FLAGS] |= SA_BLUR
        self._i[i, _W_BLUR_KIND], self._i[i, _W_BLUR_K], self._i[i, _W_MOTION_DIR] = kind, k, direction

    def set_affine(self, i, shift_x=0.0, shift_y=0.0, scale=1.0, angle_deg=0.0):
        self.set_affine_matrix(i, inverse_affine(self.h, self.w, shift_x, shift_y, scale, angle_deg))

    def set_affine_matrix(self, i, m):
        """``m``: six numbers, the row-major 2 x 3 map from an output pixel (x, y, 1) to its source position."""
        self._i[i, _W_FLAGS] |= SA_AFFINE
        self._f[i, _W_AFFINE:_W_AFFINE + 6] = m

    def set_stage5(self, i, kind, p0, p1):
        """sharpen (alpha, lightness) | emboss (alpha, strength) | brightness-contrast (brightness, contrast)."""
        if kind not in (STAGE5_SHARPEN, STAGE5_EMBOSS, STAGE5_BRIGHTNESS_CONTRAST):
            raise ValueError("set_stage5: kind in {0 sharpen, 1 emboss, 2 brightness-contrast}")
        self._i[i, _W_FLAGS] |= SA_STAGE5
        self._i[i, _W_S5_KIND] = kind
        self._f[i, _W_S5_PARAMS:_W_S5_PARAMS + 2] = (p0, p1)

    def set_clahe(self, i, clip_limit):
        """CLAHE on the Lab lightness (8 x 8 tiles) as the sample's stage 5, in place of sharpen / emboss / brightness-contrast;
        ``clip_limit >= 1`` as albumentations draws it.  The frame sides must be multiples of 8 (``check``)."""
        if not clip_limit >= 1.0:
            raise ValueError("set_clahe: clip_limit must be at least 1")
        self._i[i, _W_FLAGS] |= SA_STAGE5
        self._i[i, _W_S5_KIND] = STAGE5_CLAHE
        self._f[i, _W_S5_PARAMS:_W_S5_PARAMS + 2] = (clip_limit, 0.0)

    def set_hsv(self, i, dh, ds, dv):
        self._i[i, _W_FLAGS] |= SA_HSV
        self._f[i, _W_HSV:_W_HSV + 3] = (dh, ds, dv)

    # ---- views of the table
    @property
    def table(self):
        """int32 ``[n, 32]`` CPU tensor sharing the object's memory."""
        return torch.from_numpy(self._i)

    @property
    def ints(self):
        return self._i

    @property
    def floats(self):
        return self._f

    @property
    def flags(self):
        return self._i[:, _W_FLAGS]

    @property
    def d4(self):
        return self._i[:, _W_D4]

    @property
    def clahe(self):
        """Per sample: whether the record is on CLAHE."""
        return ((self._i[:, _W_FLAGS] & SA_STAGE5) != 0) & (self._i[:, _W_S5_KIND] == STAGE5_CLAHE)

    def check(self, n, h, w):
        if (self.n, self.h, self.w) != (n, h, w):
            raise ValueError(f"strong_views: records drawn for {self.n} x {self.h} x {self.w} frames, batch is {n} x {h} x {w}")
        i = self._i
        if h != w and bool((i[:, _W_D4] & TRANSPOSE).any()):
            raise ValueError("strong_views: transposing D4 codes need square images")
        if bool(((i[:, _W_D4] < 0) | (i[:, _W_D4] > 7)).any()):
            raise ValueError("strong_views: D4 codes are 0..7")
        blur = (i[:, _W_FLAGS] & SA_BLUR) != 0
        if bool((blur & ((i[:, _W_BLUR_K] != 3) & (i[:, _W_BLUR_K] != 5))).any()):
            raise ValueError("strong_views: blur sizes are 3 or 5")
        self.any_clahe = bool((i[:, _W_S5_KIND] == STAGE5_CLAHE).any()) and bool(self.clahe.any())   # one comparison when none is
        if self.any_clahe:
            on = self.clahe
            if h % CLAHE_GRID or w % CLAHE_GRID:
                raise ValueError(f"CLAHE records need frame sides that are multiples of {CLAHE_GRID}, batch is {h} x {w}")
            if not bool((self._f[on, _W_S5_PARAMS] >= 1.0).all()):
                raise ValueError("CLAHE records need a clip limit of at least 1")


def _clahe_frames(who, clahe, h, w):
    if clahe and (h % CLAHE_GRID or w % CLAHE_GRID):
        raise ValueError(f"{who}: clahe=True needs frame sides that are multiples of {CLAHE_GRID}, got {h} x {w}")


def _draw_stage5_hsv(P, i, r, clahe, p5, clip_hi, bc, p_hsv):
    """Stages 5 and 6 of record ``i`` of either draw from its eight uniforms ``r`` (stage 5: apply, child, two parameters; HSV:
    apply, three shifts): ``OneOf(CLAHE, Sharpen, Emboss, BrightnessContrast)`` with equal weights at ``p5`` -- the clip limit
    uniform in [1, ``clip_hi``], brightness and contrast in +-``bc`` -- then ``HueSaturationValue(20, 30, 20)`` at ``p_hsv``."""
    if r[0] < p5:
        child = min(int(r[1] * 4), 3)
        if child == 0 and clahe:
            P.set_clahe(i, 1.0 + r[2] * (clip_hi - 1.0))
        elif child == 0:
            P.ints[i, _W_NOOP_CLAHE] = 1                     # left out, a no-op
        elif child == 1:
            P.set_stage5(i, STAGE5_SHARPEN, 0.2 + 0.3 * r[2], 0.5 + 0.5 * r[3])
        elif child == 2:
            P.set_stage5(i, STAGE5_EMBOSS, 0.2 + 0.3 * r[2], 0.2 + 0.5 * r[3])
        else:
            P.set_stage5(i, STAGE5_BRIGHTNESS_CONTRAST, (2 * r[2] - 1) * bc, (2 * r[3] - 1) * bc)
    if r[4] < p_hsv:
        P.set_hsv(i, (2 * r[5] - 1) * 20.0, (2 * r[6] - 1) * 30.0, (2 * r[7] - 1) * 20.0)


def draw_strong_params(n, h, w, generator=None, clahe=False):
    """One record per sample with the branch probabilities of the reference's strong pipeline (``augmentation.py:42-88``);
    ``OneOf(p=P)``: apply with probability P, pick a child with probability proportional to the child's own ``p``.  Drawn on the
    host from ``generator`` (a CPU ``torch.Generator``).  The distortions, which the strong pipeline leaves out, are drawn too and
    recorded as a no-op (word 20), so every other rate is the reference's.  CLAHE (``clip_limit=4``: uniform in [1, 4]) is opt-in:
    by default it is drawn and recorded as a no-op (word 21); with ``clahe=True`` the same draws switch the stage on
    (``set_clahe``) and word 21 stays 0 -- every other word of every record is the same either way.  On non-square frames the
    transpose bit of the D4 code is dropped."""
    import math
    _clahe_frames("draw_strong_params", clahe, h, w)
    g = generator
    codes = random_d4_codes(n, g, 0.7, 0.7, 0.7).numpy()
    if h != w:
        codes = codes & ~TRANSPOSE
    u = torch.rand(n, 24, generator=g, dtype=torch.float64).numpy()
    keys = torch.randint(0, 1 << 32, (n, 2), generator=g, dtype=torch.int64).numpy()
    P = StrongAugParams(n, h, w, codes)
    for i in range(n):
        r = u[i]
        if r[0] < 0.4:                                       # OneOf(GaussNoise(30..80), GaussNoise(20..60)), p = 0.4
            lo, hi = (30.0, 80.0) if r[1] < 0.5 else (20.0, 60.0)
            P.set_noise(i, math.sqrt(lo + r[2] * (hi - lo)), keys[i])
        if r[3] < 0.4:                                       # OneOf(MotionBlur 0.4, MedianBlur 0.3, Blur 0.3), p = 0.4
            kind = BLUR_MOTION if r[4] < 0.4 else (BLUR_MEDIAN if r[4] < 0.7 else BLUR_BOX)
            P.set_blur(i, kind, 3 if r[5] < 0.5 else 5, min(int(r[6] * 4), 3))
        if r[7] < 0.5:                                       # ShiftScaleRotate(0.1, 0.3, 60), p = 0.5
            P.set_affine(i, (2 * r[8] - 1) * 0.1 * w, (2 * r[9] - 1) * 0.1 * h, 1.0 + (2 * r[10] - 1) * 0.3, (2 * r[11] - 1) * 60.0)
        if r[12] < 0.4:                                      # OneOf(Optical, Grid, Elastic), p = 0.4: left out, a no-op
            P.ints[i, _W_NOOP_DISTORT] = 1
        # OneOf(CLAHE, Sharpen, Emboss, BrightnessContrast) at 0.4 each, p = 0.5; HueSaturationValue(20, 30, 20), p = 0.4
        _draw_stage5_hsv(P, i, r[13:21], clahe, 0.5, 4.0, 0.3, 0.4)
    return P


def _clahe_buffer(clahe_tables, slots, dev):
    """The table buffer of a call with a record on CLAHE: the caller's (tests and tools read the tables back) or a fresh one."""
    if clahe_tables is None:
        return torch.empty(slots * CLAHE_LUT_BYTES, device=dev, dtype=torch.uint8)
    if (not torch.is_tensor(clahe_tables) or clahe_tables.dtype != torch.uint8 or clahe_tables.device != dev
            or clahe_tables.numel() != slots * CLAHE_LUT_BYTES or not clahe_tables.is_contiguous()):
        raise ValueError(f"clahe_tables must be a contiguous uint8 tensor of {slots} x 8 x 8 x 256 elements on {dev}")
    return clahe_tables


def strong_views(images_u8, params_a, params_b=None, dtype=torch.float32, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 max_pixel_value=255.0, clahe_tables=None):
    """images_u8 ``[N,H,W,3]`` uint8 (host or device) + one ``StrongAugParams`` per view -> one or two strongly augmented model
    inputs (``[N,3,H,W]``-shaped views of channel-padded NHWC buffers in ``dtype``, as ``prepare_batch`` hands them out).  Both
    views come from one upload of the frames and one of the records, in at most two kernel launches -- three when a record is
    on CLAHE (the table pass) -- and without a host synchronisation.  ``clahe_tables``: an optional uint8 device tensor
    ``[views*N,8,8,256]`` that receives the CLAHE tables of such a call (rows of samples not on CLAHE are left as they are)."""
    _lib.require_gpu()
    n, h, w = _check_frames("strong_views", images_u8, None, dtype)
    params = [params_a] if params_b is None else [params_a, params_b]
    for p in params:
        if not isinstance(p, StrongAugParams) or p.WORDS != SA_WORDS:
            raise ValueError("strong_views: parameters must be StrongAugParams (see draw_strong_params)")
        p.check(n, h, w)
    views = len(params)
    host = params[0].table if views == 1 else torch.cat([p.table for p in params])
    source_pass = int(bool((host[:, _W_FLAGS] & (SA_NOISE | SA_BLUR)).any()))
    dev, img, _, table, cpad, buf, _ = _device_batch(images_u8, None, host, n, h, w, dtype, views)
    mid = torch.empty(views * n * h * w * 4, device=dev, dtype=torch.float32) if source_pass else None
    m255, r255 = normalize_constants(mean, std, max_pixel_value)
    if any(p.any_clahe for p in params):                         # set by check()
        lut = _clahe_buffer(clahe_tables, views * n, dev)
        check(ops.udaseg_strong_aug_clahe_u8(img, table, views, n, h, w, mid, m255, r255, buf, cpad, int(dtype == torch.bfloat16),
                                             source_pass, lut, None), "strong_aug_clahe_u8")
    else:
        check(ops.udaseg_strong_aug_u8(img, table, views, n, h, w, mid, m255, r255, buf, cpad, int(dtype == torch.bfloat16),
                                       source_pass, None), "strong_aug_u8")
    outs = []
    for v in range(views):
        # a tensor of its own over the view's part of the storage (not a view of ``buf``): it is what the model recognises
        o = torch.empty(0, device=dev, dtype=dtype).set_(buf.untyped_storage(), v * n * h * w * cpad, (n, h, w, cpad),
                                                         (h * w * cpad, w * cpad, cpad, 1))
        outs.append(_model_input(o))
    return outs[0] if views == 1 else tuple(outs)


def philox4x32(counters, keys):
    """Raw Philox4x32-10 words of the noise stage's generator: counters int32 ``[count,4]``, keys int32 ``[count,2]`` (bit
    patterns) on the GPU -> int32 ``[count,4]``.  For tests."""
    _lib.require_gpu()
    count = counters.shape[0]
    out = torch.empty((count, 4), device=counters.device, dtype=torch.int32)
    check(ops.udaseg_philox4x32_debug(counters.contiguous(), keys.contiguous(), out, count, None), "philox4x32_debug")
    return out


# ------------------------------------------------------------------------------------- labelled training augmentation
# Record of udaseg_train_aug_u8 (include/udaseg.h): words 0..31 are the strong record, the rest the distortion stage; the
# pipeline is defined in INTEGRATION.md, "Training augmentation".
TA_WORDS = 64
TA_DISTORT = 32
DISTORT_OPTICAL, DISTORT_GRID, DISTORT_ELASTIC = 1, 2, 3
ELASTIC_MAX_RADIUS = 18
_W_DISTORT_KIND, _W_OPTICAL, _W_GRID_X, _W_GRID_Y, _W_ELASTIC_ALPHA, _W_ELASTIC_KEY = 32, 33, 36, 42, 48, 50


def gaussian_weights(sigma):
    """The elastic field's filter: radius ``R = ceil(3 sigma)``, ``exp(-i^2 / (2 sigma^2))`` for i = -R..R normalised to sum 1 in
    float64, then rounded once to fp32.  -> (fp32 numpy array of 2R + 1 taps, R)."""
    import math
    import numpy as np
    if not sigma > 0:
        raise ValueError("gaussian_weights: sigma must be positive")
    radius = int(math.ceil(3.0 * sigma))
    if radius > ELASTIC_MAX_RADIUS:
        raise ValueError(f"gaussian_weights: radius ceil(3 sigma) = {radius} is above {ELASTIC_MAX_RADIUS}")
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    wts = np.exp(-i * i / (2.0 * float(sigma) ** 2))
    return (wts / wts.sum()).astype(np.float32), radius


class TrainAugParams(StrongAugParams):
    """One parameter record per sample for ``train_batch``: an int32 ``[n, 64]`` host table whose words 0..31 are exactly the
    ``StrongAugParams`` record (same setters) and whose words 32.. hold the distortion stage: at most one of
    ``set_optical`` / ``set_grid`` / ``set_elastic`` per sample."""
    WORDS = TA_WORDS

    def __init__(self, n, h, w, d4_codes=None):
        import numpy as np
        super().__init__(n, h, w, d4_codes)
        self._kinds = np.zeros(self.n, dtype=np.int32)        # bit k: set_<kind k> was called for the sample

    def _distort(self, i, kind):
        self._i[i, _W_FLAGS] |= TA_DISTORT
        self._i[i, _W_DISTORT_KIND] = kind
        self._kinds[i] |= 1 << kind

    def set_optical(self, i, k, dx=0.0, dy=0.0):
        """Radial distortion ``1 + k r^2 + k r^4`` about the frame centre moved by (``dx``, ``dy``) pixels."""
        self._distort(i, DISTORT_OPTICAL)
        self._f[i, _W_OPTICAL:_W_OPTICAL + 3] = (k, dx, dy)

    def set_grid(self, i, steps_x, steps_y):
        """Six step factors per axis: cell ``i`` (of width ``side // 5``) is read ``steps[i]`` times as fast as it is written."""
        if len(steps_x) != 6 or len(steps_y) != 6:
            raise ValueError("set_grid: six step factors per axis")
        self._distort(i, DISTORT_GRID)
        self._f[i, _W_GRID_X:_W_GRID_X + 6] = steps_x
        self._f[i, _W_GRID_Y:_W_GRID_Y + 6] = steps_y

    def set_elastic(self, i, alpha, key):
        """Displacement ``alpha`` x the smoothed Philox field under ``key`` (two 32-bit words)."""
        self._distort(i, DISTORT_ELASTIC)
        self._f[i, _W_ELASTIC_ALPHA] = alpha
        self._i.view("uint32")[i, _W_ELASTIC_KEY:_W_ELASTIC_KEY + 2] = [int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF]

    @property
    def distortion(self):
        """Per sample: 0 none, 1 optical, 2 grid, 3 elastic."""
        import numpy as np
        return np.where((self._i[:, _W_FLAGS] & TA_DISTORT) != 0, self._i[:, _W_DISTORT_KIND], 0)

    def check(self, n, h, w):
        super().check(n, h, w)
        kind = self.distortion
        if bool(((self._kinds & (self._kinds - 1)) != 0).any()):
            raise ValueError("train_batch: at most one distortion kind per sample")
        on = (self._i[:, _W_FLAGS] & TA_DISTORT) != 0
        if bool((on & ((kind < DISTORT_OPTICAL) | (kind > DISTORT_ELASTIC))).any()):
            raise ValueError("train_batch: distortion kinds are 1 optical, 2 grid, 3 elastic")
        if min(h, w) < 5 and bool((kind == DISTORT_GRID).any()):
            raise ValueError("train_batch: grid distortion needs frames of at least 5 x 5")


def draw_training_params(n, h, w, generator=None, clahe=False):
    """One record per sample with the rates and ranges of the reference's basic training pipeline (``augmentation.py:10-35``;
    ``OneOf(p=P)`` as in ``draw_strong_params``).  Drawn on the host from ``generator`` (a CPU ``torch.Generator``).  CLAHE
    (``clip_limit=2``: uniform in [1, 2]) is opt-in as in ``draw_strong_params``: a recorded no-op (word 21) by default, the
    stage itself with ``clahe=True``, every other word unchanged.  On non-square frames the transpose bit of the D4 code is
    dropped; frames with a side below 5 are refused (the grid child needs five cells per axis)."""
    import math
    _clahe_frames("draw_training_params", clahe, h, w)
    if min(h, w) < 5:
        raise ValueError("draw_training_params: frames of at least 5 x 5 (grid distortion)")
    g = generator
    codes = random_d4_codes(n, g).numpy()
    if h != w:
        codes = codes & ~TRANSPOSE
    u = torch.rand(n, 40, generator=g, dtype=torch.float64).numpy()
    keys = torch.randint(0, 1 << 32, (n, 4), generator=g, dtype=torch.int64).numpy()
    P = TrainAugParams(n, h, w, codes)
    for i in range(n):
        r = u[i]
        if r[0] < 0.2:                                       # OneOf(GaussNoise(10..50), GaussNoise()), p = 0.2: variance in (10, 50)
            P.set_noise(i, math.sqrt(10.0 + 40.0 * r[1]), keys[i, :2])
        if r[2] < 0.2:                                       # OneOf(MotionBlur 0.2, MedianBlur(3) 0.1, Blur(3) 0.1), p = 0.2
            if r[3] < 0.5:
                P.set_blur(i, BLUR_MOTION, 3 if r[4] < 0.5 else 5, min(int(r[5] * 4), 3))
            else:
                P.set_blur(i, BLUR_MEDIAN if r[3] < 0.75 else BLUR_BOX, 3)
        if r[6] < 0.2:                                       # ShiftScaleRotate(0.0625, 0.2, 45), p = 0.2
            P.set_affine(i, (2 * r[7] - 1) * 0.0625 * w, (2 * r[8] - 1) * 0.0625 * h, 1.0 + (2 * r[9] - 1) * 0.2, (2 * r[10] - 1) * 45.0)
        if r[11] < 0.2:                                      # OneOf(Optical 0.3, Grid 0.1, Elastic 0.3), p = 0.2
            if r[12] < 3.0 / 7.0:
                P.set_optical(i, (2 * r[13] - 1) * 0.05, (2 * r[14] - 1) * 0.05, (2 * r[15] - 1) * 0.05)
            elif r[12] < 4.0 / 7.0:
                P.set_grid(i, 1.0 + (2 * r[16:22] - 1) * 0.3, 1.0 + (2 * r[22:28] - 1) * 0.3)
            else:
                P.set_elastic(i, 120.0, keys[i, 2:])
        # OneOf(CLAHE, Sharpen, Emboss, BrightnessContrast), equal, p = 0.3; HueSaturationValue(20, 30, 20), p = 0.3
        _draw_stage5_hsv(P, i, r[28:36], clahe, 0.3, 2.0, 0.2, 0.3)
    return P


def _weights_array(sigma):
    wts, radius = gaussian_weights(sigma)
    return (ctypes.c_float * len(wts))(*[float(v) for v in wts]), radius


def elastic_field(params, elastic_sigma=6.0):
    """The smoothed displacement field of the samples of ``params`` (a ``TrainAugParams``) that are on elastic: fp32
    ``[n, h, w, 2]`` (x, y) on the GPU; samples on anything else stay zero.  For tests and tools."""
    _lib.require_gpu()
    if not isinstance(params, TrainAugParams):
        raise ValueError("elastic_field: parameters must be TrainAugParams")
    n, h, w = params.n, params.h, params.w
    params.check(n, h, w)
    dev = torch.device("cuda", torch.cuda.current_device())
    wts, radius = _weights_array(elastic_sigma)
    field = torch.zeros((n, h, w, 2), device=dev, dtype=torch.float32)
    check(ops.udaseg_elastic_field_f32(params.table.to(dev), n, h, w, wts, radius, field, None), "elastic_field_f32")
    return field


def clahe_tables(images_u8, params_a, params_b=None):
    """The CLAHE table pass alone (udaseg_clahe_lut_u8), for tests and tools: uint8 ``[views*N,8,8,256]`` on the GPU, zero rows
    for samples not on CLAHE.  Records whose stage-4 image needs the source or the field pass (noise, blur, elastic) are
    refused: ``strong_views`` / ``train_batch`` hand their tables out through ``clahe_tables=``."""
    _lib.require_gpu()
    n, h, w = _check_frames("clahe_tables", images_u8)
    params = [params_a] if params_b is None else [params_a, params_b]
    words = params_a.WORDS if isinstance(params_a, StrongAugParams) else 0
    for p in params:
        if not isinstance(p, StrongAugParams) or p.WORDS != words or (len(params) == 2 and words != SA_WORDS):
            raise ValueError("clahe_tables: one StrongAugParams per view, or one TrainAugParams")
        p.check(n, h, w)
        if bool((p.flags & (SA_NOISE | SA_BLUR)).any()) or (words == TA_WORDS and bool((p.distortion == DISTORT_ELASTIC).any())):
            raise ValueError("clahe_tables: records with noise, blur or elastic distortion take the full call (clahe_tables=)")
    if h % CLAHE_GRID or w % CLAHE_GRID:
        raise ValueError(f"clahe_tables: frame sides must be multiples of {CLAHE_GRID}, got {h} x {w}")
    views = len(params)
    host = params[0].table if views == 1 else torch.cat([p.table for p in params])
    dev = torch.device("cuda", torch.cuda.current_device())
    lut = torch.zeros((views * n, CLAHE_GRID, CLAHE_GRID, 256), device=dev, dtype=torch.uint8)
    check(ops.udaseg_clahe_lut_u8(images_u8.to(dev, non_blocking=True).contiguous(), host.to(dev, non_blocking=True), words, views, n,
                                  h, w, None, None, lut, None), "clahe_lut_u8")
    return lut


def train_batch(images_u8, masks_u8=None, params=None, generator=None, dtype=torch.float32, elastic_sigma=6.0,
                mean=IMAGENET_MEAN, std=IMAGENET_STD, max_pixel_value=255.0, clahe=False, clahe_tables=None):
    """images_u8 ``[N,H,W,3]`` uint8, masks_u8 ``[N,H,W]`` uint8 or None (host or device), params: a ``TrainAugParams`` or None
    (drawn with ``draw_training_params(N, H, W, generator, clahe)``) -> ``(images, masks)`` exactly in ``prepare_batch``'s output
    form: the ``[N,3,H,W]``-shaped view of the padded NHWC buffer in ``dtype`` and int64 masks (or None), augmented by the
    training pipeline of INTEGRATION.md with image and mask carried through the same geometry.  At most three kernel launches --
    four when a record is on CLAHE (the table pass) -- and no host synchronisation; a record with every stage off equals
    ``prepare_batch`` bit for bit.  ``clahe_tables``: as in ``strong_views``, ``[N,8,8,256]``."""
    _lib.require_gpu()
    n, h, w = _check_frames("train_batch", images_u8, masks_u8, dtype)
    if params is None:
        params = draw_training_params(n, h, w, generator, clahe)
    if not isinstance(params, TrainAugParams):
        raise ValueError("train_batch: parameters must be TrainAugParams (64-word records, see draw_training_params)")
    params.check(n, h, w)
    host = params.table
    source_pass = int(bool((host[:, _W_FLAGS] & (SA_NOISE | SA_BLUR)).any()))
    field_pass = int(bool((params.distortion == DISTORT_ELASTIC).any()))
    wts, radius = _weights_array(elastic_sigma) if field_pass else (None, 0)
    dev, img, msk, table, cpad, out, out_m = _device_batch(images_u8, masks_u8, host, n, h, w, dtype)
    mid = torch.empty(n * h * w * 4, device=dev, dtype=torch.float32) if source_pass else None
    field = torch.empty(n * h * w * 2, device=dev, dtype=torch.float32) if field_pass else None
    m255, r255 = normalize_constants(mean, std, max_pixel_value)
    if params.any_clahe:                                         # set by check()
        lut = _clahe_buffer(clahe_tables, n, dev)
        check(ops.udaseg_train_aug_clahe_u8(img, msk, table, n, h, w, mid, field, wts, radius, m255, r255, out, cpad,
                                            int(dtype == torch.bfloat16), out_m, source_pass, field_pass, lut, None),
              "train_aug_clahe_u8")
    else:
        check(ops.udaseg_train_aug_u8(img, msk, table, n, h, w, mid, field, wts, radius, m255, r255, out, cpad,
                                      int(dtype == torch.bfloat16), out_m, source_pass, field_pass, None), "train_aug_u8")
    return _model_input(out), out_m


class DeviceAugmentedLoader:
    """Wraps a loader of uint8 ``(images [N,H,W,3], masks [N,H,W])`` batches -- or of images alone -- and yields ``train_batch``'s
    output in the same structure: ``(images, masks)`` pairs, or image tensors.  Fresh records are drawn for every batch from
    ``generator``, with CLAHE switched on by ``clahe=True`` (``draw_training_params``).  ``SegmentationTrainer.train_epoch`` /
    ``AdversarialTrainer.train_epoch`` consume it as they are."""

    def __init__(self, loader, dtype=torch.float32, generator=None, elastic_sigma=6.0, clahe=False):
        self.loader, self.dtype, self.generator, self.elastic_sigma, self.clahe = loader, dtype, generator, elastic_sigma, clahe

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            if torch.is_tensor(batch):
                yield train_batch(batch, None, None, self.generator, self.dtype, self.elastic_sigma, clahe=self.clahe)[0]
            else:
                images, masks = batch
                yield train_batch(images, masks, None, self.generator, self.dtype, self.elastic_sigma, clahe=self.clahe)
