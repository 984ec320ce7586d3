"""Calibration of the segmenter's confidence on the device: reliability tables, expected calibration error, temperature scaling.

Every self-training recipe here turns the winner's softmax probability into a decision -- ``PseudoLabeler`` / ``OnlineLabeler``
threshold it, ``pseudo.confidence_share`` counts it, ``DistillTrainer`` weights images by it -- and under domain shift a segmenter
is over-confident on the target domain.  ``curves`` measures ranking, ``metrics`` / ``boundary`` overlap; this module measures
whether a confidence of 0.9 means 90 % correct and fits the one scalar that corrects it.  (The reference bins a host copy of the
softmax with numpy.)

The confidence and its grid (part of the public contract)
    For a pixel with logits ``z`` and a reciprocal temperature ``beta``: ``c^`` = the first maximal channel (the one tie rule of
    ``PseudoLabeler``, ``confusion_matrix`` and ``ScoreHistogram``), ``p = 1 / sum_j exp((z_j - z[c^]) * beta)``.  At ``beta = 1`` this
    is bit for bit the confidence ``PseudoLabeler`` and ``confidence_share`` use.  With ``probs=True`` the buffer holds
    probabilities (``proto.rectify`` output) and ``p`` is the winner's value.  ``B`` uniform bins over ``[0, 1]``:
    ``b = min(floor(p * B), B - 1)``, lower edge ``b / B``, ``p == 1`` in the top bin.

    ``tables [3, C, B]`` int64, indexed by the PREDICTED class: ``count``, ``correct`` (``c^ == target``) and ``conf_q``, the sum of
    ``round(p * 2^24)``: the confidence in fixed point, so every sum is an integer, independent of order and the same on every
    run.  ``counters [3]``: the pixels in the tables, the void pixels (target outside ``[0, C)``), the non-finite pixels (valid
    target, but ``p`` is not a finite number in ``[0, 1]``).  Tables and counters ACCUMULATE across ``update`` calls.

From the tables, with ``n_b, a_b, q_b`` summed over the classes and ``N = sum n_b``
    ``accuracy = sum a_b / N``, ``mean_conf = sum q_b / 2^24 / N``, ``ece = sum_b |a_b - q_b / 2^24| / N`` (the expected calibration
    error: the count-weighted mean of ``|accuracy_b - confidence_b|``), ``mce`` = the largest ``|accuracy_b - confidence_b|`` over the
    non-empty bins, ``gap = mean_conf - accuracy`` (positive: over-confident).  ``per_class [4, C]``: ``n_c, acc_c, conf_c, ece_c``,
    the same over the pixels predicted as ``c`` -- they tell a class-balanced labeller which classes its thresholds flatter.
    Everything is NaN where its denominator is 0.

Temperature scaling
    ``TemperatureScaler`` holds ``inv_temp [1]`` fp32 ON THE DEVICE (``PrototypeBank.inv_tau``'s pattern) and fits it by Newton's
    method on the negative log likelihood of the targets under ``softmax(beta z)``.  The NLL is convex in ``beta`` (not in the
    temperature), each step is clamped to ``[beta / 4, 4 beta]`` and to ``[1 / 64, 64]`` -- on over-confident logits the raw Newton
    step from ``beta = 1`` is negative -- and nothing is read back while fitting.
"""
import numpy as np
import torch

from . import _args as A
from . import kernels as K

DEFAULT_BINS = 15
MAX_BINS = 64
_Q_ONE = 16777216.0
OUT_KEYS = ("n", "accuracy", "mean_conf", "ece", "mce", "gap")
CLASS_KEYS = ("n", "accuracy", "mean_conf", "ece")


def reliability_from_tables(tables):
    """The finishing arithmetic on the host, float64 numpy (what ``udaseg_calib_finish`` does on the device, plus the diagram
    arrays).  ``tables``: ``[3, C, B]`` integer tables (numpy or a tensor).  Returns a dict:

    ``n``, ``accuracy``, ``mean_conf``, ``ece``, ``mce``, ``gap``: floats; ``per_class``: dict of ``[C]`` float64 arrays ``n``,
    ``accuracy``, ``mean_conf``, ``ece``; and the reliability diagram, ``[B]`` arrays: ``bin_lower`` (``b / B``), ``bin_count`` (int64),
    ``bin_accuracy``, ``bin_confidence`` (NaN for an empty bin).  Everything is NaN where its denominator is 0.
    """
    if torch.is_tensor(tables):
        tables = tables.detach().cpu().numpy()
    tab = np.asarray(tables).astype(np.int64)
    if tab.ndim != 3 or tab.shape[0] != 3:
        raise ValueError(f"tables must be [3, C, B] (count, correct, conf_q), got {tab.shape}")
    _, C, B = tab.shape
    nan = float("nan")
    n_b, a_b, q_b = tab[0].sum(axis=0), tab[1].sum(axis=0), tab[2].sum(axis=0)        # exact integers
    N = int(n_b.sum())
    af, qf, nf = a_b.astype(np.float64), q_b.astype(np.float64) / _Q_ONE, n_b.astype(np.float64)
    e = 0.0
    for b in range(B):                                                                 # the device's order
        e += abs(af[b] - qf[b])
    full = n_b > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        bin_acc = np.where(full, af / nf, nan)
        bin_conf = np.where(full, qf / nf, nan)
    acc = float(a_b.sum()) / N if N else nan
    conf = float(q_b.sum()) / _Q_ONE / N if N else nan
    out = {"n": float(N), "accuracy": acc, "mean_conf": conf, "ece": e / N if N else nan,
           "mce": float(np.abs(bin_acc[full] - bin_conf[full]).max()) if full.any() else nan, "gap": conf - acc}
    n_c = tab[0].sum(axis=1)
    has = n_c > 0
    ncf = n_c.astype(np.float64)
    ece_c = np.zeros(C)
    for b in range(B):
        ece_c += np.abs(tab[1, :, b].astype(np.float64) - tab[2, :, b].astype(np.float64) / _Q_ONE)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["per_class"] = {"n": ncf, "accuracy": np.where(has, tab[1].sum(axis=1).astype(np.float64) / ncf, nan),
                            "mean_conf": np.where(has, tab[2].sum(axis=1).astype(np.float64) / _Q_ONE / ncf, nan),
                            "ece": np.where(has, ece_c / ncf, nan)}
    out.update(bin_lower=np.arange(B, dtype=np.float64) / B, bin_count=n_b, bin_accuracy=bin_acc, bin_confidence=bin_conf)
    return out


class TemperatureScaler(A.DeviceState):
    """One scalar on the device: ``inv_temp [1]`` fp32, the reciprocal temperature ``beta`` (1 until fitted).  ``fit_logits`` and
    ``fit`` enqueue kernels and never read back; ``scale`` is the bridge to ``PseudoLabeler``, ``confidence_share``, ``predict_large``
    and the trainers, none of which know about temperatures; ``temperature()`` is the one host read, for
    ``SoftCrossEntropyLoss(teacher_temperature=...)``."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else None
        self.inv_temp = None             # [1] fp32
        self.sums = None                 # [4] f64: n, sum nll, sum g1, sum g2 of the pass in flight
        self.state = None                # [4] f64: mean nll, mean g1, last move of beta, steps taken
        self.counters = None             # [3] i64: counted, void, non-finite pixels of every pass so far

    _need_state = A.DeviceState._ensure       # the spelling the GPU tests build their scalers with (tests/test_gpu_calibration.py)

    def _allocate(self, device):
        self.inv_temp = torch.ones(1, dtype=torch.float32, device=device)
        self.sums = torch.zeros(4, dtype=torch.float64, device=device)
        self.state = torch.zeros(4, dtype=torch.float64, device=device)
        self.counters = torch.zeros(3, dtype=torch.int64, device=device)

    def reset(self):
        """beta = 1, no steps taken."""
        if self.inv_temp is not None:
            self.inv_temp.fill_(1.0)
            self.sums.zero_()
            self.state.zero_()
            self.counters.zero_()
        return self

    def accumulate(self, logits, masks):
        """Adds one batch's NLL sums at the current beta to the pass in flight (one launch, no sync)."""
        who = "TemperatureScaler"
        n, c, h, w = A.scores_shape(who, logits, name="logits")
        tgt = A.flat_targets(who, masks, n * h * w)
        dev = self._ensure(A.same_gpu(who, logits=logits, masks=masks)).device
        buf, ldc = A.padded_nhwc(logits.detach())
        parts = torch.empty(4 * K.seg_partials(), dtype=torch.float64, device=dev)
        A.on_device(dev, K.calib_nll, buf, tgt, n * h * w, c, ldc, self.inv_temp, parts, self.sums, self.counters)
        return self

    def step(self):
        """One guarded Newton step from the accumulated sums (one launch, no sync); the sums start over."""
        self._ensure()
        A.on_device(self.device, K.calib_step, self.sums, self.inv_temp, self.state)
        return self

    def fit_logits(self, logits, masks, iters=8):
        """``iters`` x (NLL sums of this batch, one step): 3 x ``iters`` launches and no host read."""
        for _ in range(int(iters)):
            self.accumulate(logits, masks).step()
        return self

    def fit(self, model, loader, device, iters=8):
        """Fits beta on ``loader`` (batches of ``(images, masks)``) with the model in eval mode.  Every iteration is ONE FULL PASS over
        the loader -- the sums accumulate on the device and one step ends the pass -- so this costs ``iters`` forward passes over
        the set; nothing is read back.  Hold out a small labelled set for it."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TemperatureScaler.fit: the model runs on the GPU (no CPU path in this build)")
        self._ensure(device)
        with A.eval_mode(model), torch.no_grad():
            for _ in range(int(iters)):
                for images, masks in loader:
                    self.accumulate(model(images.to(device)), masks.to(device))
                self.step()
        return self

    def scale(self, logits):
        """``logits * beta`` as a device op (no sync): what to hand to anything that takes logits."""
        if logits.device.type != "cuda":
            raise RuntimeError("TemperatureScaler.scale: logits must live on the GPU (no CPU path in this build)")
        self._ensure(logits.device)
        return logits * self.inv_temp.to(logits.dtype)

    def temperature(self):
        """``1 / beta`` as a Python float: one host read."""
        return 1.0 / float(self._ensure().inv_temp.item())

    def report(self):
        """One host read: ``beta``, ``temperature``, the last pass's ``mean_nll`` and ``mean_grad`` (d nll / d beta at the beta before
        the last step), ``last_move`` (of beta), ``steps`` and the pixel counters over all passes."""
        self._ensure()
        packed = torch.cat([self.inv_temp.double(), self.state, self.counters.double()]).cpu().numpy()
        beta = float(packed[0])
        return {"beta": beta, "temperature": 1.0 / beta, "mean_nll": float(packed[1]), "mean_grad": float(packed[2]),
                "last_move": float(packed[3]), "steps": int(packed[4]), "counted": int(packed[5]), "void": int(packed[6]),
                "nonfinite": int(packed[7])}

    _STATE = ("inv_temp", "sums", "state", "counters")

    def state_dict(self):
        self._ensure()
        return {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}

    def load_state_dict(self, state):
        """Restores the device state bit for bit."""
        self._ensure()
        for k in self._STATE:
            dst, src = getattr(self, k), state[k]
            if src.dtype != dst.dtype or src.shape != dst.shape:
                raise ValueError(f"TemperatureScaler.load_state_dict: {k} must be {dst.dtype} {tuple(dst.shape)}, "
                                 f"got {src.dtype} {tuple(src.shape)}")
        for k in self._STATE:
            getattr(self, k).copy_(state[k])
        return self


class ReliabilityHistogram(A.DeviceState):
    """Accumulates the reliability tables of ``[N,C,H,W]`` scores against ``[N,H,W]`` (or ``[N,1,H,W]``) masks on the device.
    ``update`` enqueues one kernel and does not synchronise; ``compute`` enqueues the finishing kernel and returns device tensors;
    ``tables`` reads tables and counters back in ONE transfer."""

    def __init__(self, num_classes, bins=DEFAULT_BINS, device=None):
        self.num_classes = A.int_in("ReliabilityHistogram", "num_classes", num_classes, 1, 32)
        self.bins = A.int_in("ReliabilityHistogram", "bins", bins, 2, MAX_BINS)
        self.device = torch.device(device) if device is not None else None
        self.buffer = None               # [3 * C * B + 3] int64 on the device: the tables, then the counters (one transfer)

    def _allocate(self, device):
        self.buffer = torch.zeros(3 * self.num_classes * self.bins + 3, dtype=torch.int64, device=device)

    def _views(self):
        buf = self._ensure().buffer
        return buf[:-3], buf[-3:]

    @property
    def device_tables(self):
        """``[3, C, B]`` int64 view of the device tables."""
        return self._views()[0].view(3, self.num_classes, self.bins)

    @property
    def counters(self):
        return self._views()[1]

    def reset(self):
        if self.buffer is not None:
            self.buffer.zero_()
        return self

    def update(self, outputs, masks, probs=False, scaler=None):
        """``outputs``: logits, or probabilities with ``probs``; ``scaler``: a ``TemperatureScaler`` whose beta the kernel reads from
        device memory (logits only)."""
        who = "ReliabilityHistogram.update"
        n, c, h, w = A.scores_shape(who, outputs, self.num_classes)
        if probs and scaler is not None:
            raise ValueError(f"{who}: probabilities take no temperature (probs=True with a scaler)")
        tgt = A.flat_targets(who, masks, n * h * w)
        dev = self._ensure(A.same_gpu(who, scores=outputs, masks=masks)).device
        tables, counters = self._views()
        buf, ldc = A.padded_nhwc(outputs.detach())
        inv_temp = None if scaler is None else scaler._ensure(dev).inv_temp
        A.on_device(dev, K.calib_hist, buf, tgt, n * h * w, c, ldc, probs, inv_temp, self.bins, tables, counters)
        return self

    def compute(self):
        """{'out': [6] float64 (``OUT_KEYS``: n, accuracy, mean_conf, ece, mce, gap), 'per_class': [4, C] float64 (``CLASS_KEYS``),
        'counters': [3] int64} as DEVICE tensors (no host sync)."""
        tables, counters = self._views()
        f = torch.empty(6 + 4 * self.num_classes, dtype=torch.float64, device=tables.device)
        A.on_device(tables.device, K.calib_finish, tables, self.num_classes, self.bins, f[:6], f[6:])
        return {"out": f[:6], "per_class": f[6:].view(4, self.num_classes), "counters": counters}

    def tables(self):
        """(tables ``[3, C, B]``, counters ``[3]``) as int64 numpy arrays: ONE device->host transfer."""
        self._views()
        packed = self.buffer.cpu().numpy()
        return packed[:-3].reshape(3, self.num_classes, self.bins), packed[-3:]

    def reliability(self):
        """``reliability_from_tables`` of the accumulated tables plus ``counted`` / ``void`` / ``nonfinite``: one transfer."""
        tab, cnt = self.tables()
        out = reliability_from_tables(tab)
        out.update(counted=int(cnt[0]), void=int(cnt[1]), nonfinite=int(cnt[2]), tables=tab)
        return out


def evaluate(model, loader, num_classes, device, bins=DEFAULT_BINS, scaler=None):
    """Eval-mode pass over ``loader`` (batches of ``(images, masks)``); the tables accumulate on the device and are read back ONCE.
    Returns ``ReliabilityHistogram.reliability()``: the ``out`` / ``per_class`` values, the counters, the diagram arrays and the
    tables.  ``scaler``: measure the calibration at its fitted temperature."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evaluate: the model runs on the GPU (no CPU path in this build)")
    hist = ReliabilityHistogram(num_classes, bins, device)
    with A.eval_mode(model), torch.no_grad():
        for images, masks in loader:
            hist.update(model(images.to(device)), masks.to(device), scaler=scaler)
    return hist.reliability()
