"""The shared host-side argument rules (``_args.py``), each checked directly with CPU tensors, and one regression per module for
the drift the shared rules removed.  No GPU is needed: the place rules are what raise here, kernels and device queries are stubbed."""
import contextlib

import numpy as np
import pytest
import torch

from uda_aerial_semantic_segmentation_research_amd import _args as A


@pytest.fixture
def layout_calls(monkeypatch):
    """The layout kernel behind ``padded_nhwc`` replaced by a recorder that returns a buffer of the right shape."""
    calls = []

    def fake(x, cpad=None, st=None, dtype=torch.float32):
        calls.append(tuple(x.shape))
        n, c, h, w = x.shape
        return torch.zeros((n, h, w, cpad), dtype=dtype)
    monkeypatch.setattr(A.K, "nchw_to_nhwc", fake)
    return calls


# ----------------------------------------------------------------------------------------------------------------- scalars
def test_int_in():
    assert A.int_in("f", "radius", 3, 0, 5) == 3 and type(A.int_in("f", "radius", np.int64(3), 0, 5)) is int
    assert A.int_in("f", "radius", 0, 0, 5) == 0 and A.int_in("f", "radius", 5, 0, 5) == 5 and A.int_in("f", "n", 10 ** 12, 1) == 10 ** 12
    for bad in (True, 3.0, "3", -1, 6, None):
        with pytest.raises(ValueError, match=r"f: radius .*0\.\.5"):
            A.int_in("f", "radius", bad, 0, 5)
    assert A.int_in("f", "radius", None, 0, 5, none_ok=True) is None and A.int_in("f", "radius", 2, 0, 5, none_ok=True) == 2
    with pytest.raises(ValueError, match="or None"):
        A.int_in("f", "radius", 6, 0, 5, none_ok=True)
    with pytest.raises(ValueError, match="f: n must be an int >= 1"):
        A.int_in("f", "n", 0, 1)


def test_number_pair_choice():
    assert A.number("f", "x", 0, 0.0, 1.0) == 0.0 and A.number("f", "x", np.float32(0.5), 0.0, 1.0) == 0.5 and A.number("f", "x", 7) == 7.0
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "x", None, [1]):
        with pytest.raises(ValueError, match="f: x"):
            A.number("f", "x", bad, 0.0, 1.0)
    with pytest.raises(ValueError, match="f: x"):
        A.number("f", "x", 0.0, 0.0, lo_open=True)
    assert A.number("f", "x", 1e-9, 0.0, lo_open=True) == 1e-9
    assert A.pair("f", "share", (0.25, 0.5), 0.0, 1.0) == (0.25, 0.5) and A.pair("f", "share", [0, 0], 0.0, 1.0) == (0.0, 0.0)
    for bad in ((0.5, 0.25), (0.25, 1.5), (-0.1, 0.5), (0.5,), 0.3, (0.1, 0.2, 0.3), ("a", "b")):
        with pytest.raises(ValueError, match="f: share"):
            A.pair("f", "share", bad, 0.0, 1.0)
    with pytest.raises(ValueError, match="f: share"):
        A.pair("f", "share", (0.0, 0.5), 0.0, 1.0, lo_open=True)
    assert A.choice("f", "kind", "a", ("a", "b")) == "a" and A.choice("f", "bins", 256, (256, 512)) == 256
    assert A.choice("f", "kind", "b", {"a": 0, "b": 1}) == "b"
    for bad in ("c", None, True, 1, ["a"]):
        with pytest.raises(ValueError, match="f: kind"):
            A.choice("f", "kind", bad, ("a", "b"))


# ----------------------------------------------------------------------------------------------------------------- tensors
def test_label_maps_value_then_place(monkeypatch):
    for bad in (torch.zeros(4, 4), torch.zeros(2, 4, 4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8),
                torch.zeros(1, 2, 4, 4, dtype=torch.uint8), torch.zeros(0, 4, 4, dtype=torch.uint8), "labels", None):
        with pytest.raises(ValueError, match="f: masks"):               # the value: a ValueError on any device
            A.label_maps("f", bad, "masks")
    for good in (torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="no CPU path"):           # the place, once the value is right
            A.label_maps("f", good)
    monkeypatch.setattr(A, "same_gpu", lambda who, **t: None)            # the value rule's results, without the place rule
    lab, single = A.label_maps("f", torch.arange(16, dtype=torch.uint8).reshape(4, 4).t())
    assert tuple(lab.shape) == (1, 4, 4) and single and lab.is_contiguous() and lab[0, 0, 1] == 4
    lab, single = A.label_maps("f", torch.zeros(2, 4, 4, dtype=torch.int64))
    assert tuple(lab.shape) == (2, 4, 4) and not single


def test_same_gpu_names_the_tensor():
    cpu = torch.zeros(1)
    assert A.same_gpu("f", a=None, b=None) is None
    with pytest.raises(RuntimeError, match="f: masks must live on the GPU .no CPU path in this build"):
        A.same_gpu("f", scores=None, masks=cpu)

    class On:                                                            # a well-formed tensor on some GPU, as far as the rule looks
        def __init__(self, index):
            self.device = torch.device("cuda", index)
    assert A.same_gpu("f", a=On(1), b=None, c=On(1)) == torch.device("cuda", 1)
    with pytest.raises(ValueError, match="a is on cuda:0, c on cuda:1"):
        A.same_gpu("f", a=On(0), b=None, c=On(1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        A.same_gpu("f", a=On(0), b=cpu)


def test_scores_nchw_never_reaches_the_layout_kernel_on_a_refusal(layout_calls):
    z = torch.zeros(1, 5, 4, 4)
    for bad in (z[0], z.double(), z.half(), torch.zeros(1, 0, 4, 4), torch.zeros(1, 33, 4, 4), torch.zeros(0, 5, 4, 4),
                torch.zeros(1, 5, 0, 4), "scores", None):
        with pytest.raises(ValueError, match="f: scores"):
            A.scores_nchw("f", bad)
    with pytest.raises(ValueError, match=r"\[N,6,H,W\]"):
        A.scores_nchw("f", z, 6)
    with pytest.raises(ValueError, match="f: features"):
        A.scores_nchw("f", torch.zeros(1, 64, 4, 4), name="features")
    for good, kw in ((z, {}), (z, dict(classes=5)), (z.bfloat16(), {}), (torch.zeros(1, 64, 4, 4), dict(classes=64, max_classes=64))):
        assert A.scores_shape("f", good, **kw) == tuple(good.shape)
        with pytest.raises(RuntimeError, match="no CPU path"):
            A.scores_nchw("f", good, **kw)
    assert not layout_calls


def test_zero_copy_rule_of_the_padded_layout(layout_calls):
    n, c, h, w, ld = 2, 5, 3, 4, 8
    strides = (h * w * ld, 1, w * ld, ld)
    base = torch.arange(n * h * w * ld, dtype=torch.float32)
    view = base.as_strided((n, c, h, w), strides)                        # what Unet.forward hands out: channels innermost, padded to 8
    buf, ldc = A.padded_nhwc(view)
    assert ldc == ld and buf.data_ptr() == base.data_ptr() and tuple(buf.shape) == (n, h, w, ld) and buf.is_contiguous()
    assert buf[1, 2, 3, 4] == view[1, 4, 2, 3] and not layout_calls
    # the same strides over a buffer one element too short: the last pixel's pad lanes would lie outside the storage
    last = sum((s - 1) * st for s, st in zip((n, c, h, w), strides))
    short = torch.zeros(n * h * w * ld - 1).as_strided((n, c, h, w), strides)
    assert last < short.untyped_storage().nbytes() // 4
    buf, ldc = A.padded_nhwc(short)
    assert layout_calls == [(n, c, h, w)] and ldc == ld and buf.data_ptr() != short.data_ptr()
    A.padded_nhwc(torch.zeros(n, c, h, w))                               # plain NCHW: the layout kernel
    A.padded_nhwc(view.bfloat16())                                       # not fp32: widened by the layout kernel
    assert len(layout_calls) == 3
    wide = torch.zeros(n * h * w * 12).as_strided((n, c, h, w), (h * w * 12, 1, w * 12, 12))
    assert A.logits_nhwc(wide)[1] == 12 and A.logits_nhwc(wide)[0].data_ptr() == wide.data_ptr() and len(layout_calls) == 3
    A.padded_nhwc(wide)                                                  # padded_nhwc itself takes ceil4(C) alone
    assert len(layout_calls) == 4


def test_flat_targets():
    m = torch.arange(2 * 3 * 4, dtype=torch.int32).reshape(2, 1, 3, 4)
    t = A.flat_targets("f", m, 24)
    assert t.dtype == torch.int64 and tuple(t.shape) == (24,) and t.is_contiguous() and t.tolist() == list(range(24))
    same = torch.zeros(2, 3, 4, dtype=torch.int64)
    assert A.flat_targets("f", same, 24).data_ptr() == same.data_ptr()
    assert A.flat_targets("f", same.permute(0, 2, 1), 24).is_contiguous()
    for bad in (m, "m", None):
        with pytest.raises(ValueError, match="f: masks"):
            A.flat_targets("f", bad, 25)


def test_frames_u8():
    f = torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    assert A.frames_u8("f", f) == (2, 4, 6) and A.frames_u8("f", f, (2, 4, 6)) == (2, 4, 6)
    for bad in (f.float(), f[..., :2], f[0], f[:0], "f", None):
        with pytest.raises(ValueError, match="f: target frames"):
            A.frames_u8("f", bad, name="target frames")
    with pytest.raises(ValueError, match=r"\[2, 4, 5, 3\]"):
        A.frames_u8("f", f, (2, 4, 5))
    huge = torch.zeros(1, dtype=torch.uint8).expand(2 ** 16, 2 ** 15, 1, 3)       # N*H*W = 2^31 without the memory
    assert A.frames_u8("f", huge) == (2 ** 16, 2 ** 15, 1)
    with pytest.raises(ValueError, match="2\\^31"):
        A.frames_u8("f", huge, below_2_31=True)


def test_out_and_counts_tensors():
    cpu, meta = torch.device("cpu"), torch.device("meta")
    out = A.out_tensor("f", "out", None, (2, 3), torch.int32, cpu)
    assert out.dtype == torch.int32 and tuple(out.shape) == (2, 3) and out.device == cpu
    assert A.out_tensor("f", "out", out, (2, 3), torch.int32, cpu) is out
    assert A.out_tensor("f", "out", out.t(), (3, 2), torch.int32, cpu).shape == (3, 2)
    for bad, dev, kw in ((out.long(), cpu, {}), (out[:1], cpu, {}), (out, meta, {}), ("out", cpu, {}),
                         (out.t(), cpu, dict(contiguous=True))):
        with pytest.raises(ValueError, match="f: out"):
            A.out_tensor("f", "out", bad, tuple(bad.shape) if bad is out.t() else (2, 3), torch.int32, dev, **kw)
    counts = torch.zeros(4, 2, dtype=torch.int64)
    assert A.counts_tensor("f", "counts", None, (4, 2), cpu) is None and A.counts_tensor("f", "counts", counts, (4, 2), cpu) is counts
    for bad, dev in ((counts.int(), cpu), (counts[:3], cpu), (counts, meta), ([0, 0], cpu)):
        with pytest.raises(ValueError, match="f: counts"):
            A.counts_tensor("f", "counts", bad, (4, 2), dev)


# --------------------------------------------------------------------------------------------------------- device and mode
def test_on_device(monkeypatch):
    entered = []

    @contextlib.contextmanager
    def device(dev):
        entered.append(dev)
        yield
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", device)
    seen = []
    fn = lambda a, b: seen.append((a, b, len(entered))) or a + b      # noqa: E731
    assert A.on_device(torch.device("cuda", 0), fn, 1, 2) == 3 and not entered and seen == [(1, 2, 0)]
    assert A.on_device(torch.device("cuda", 1), fn, 3, 4) == 7 and entered == [torch.device("cuda", 1)] and seen[-1] == (3, 4, 1)
    with pytest.raises(KeyError):                                       # an exception of fn's passes through the guard
        A.on_device(torch.device("cuda", 1), lambda: {}["x"])
    assert len(entered) == 2


def test_current_gpu_asks_for_a_gpu_first(monkeypatch):
    order = []
    monkeypatch.setattr(A._lib, "require_gpu", lambda: order.append("require"))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: order.append("current") or 3)
    assert A.current_gpu() == torch.device("cuda", 3) and order == ["require", "current"]


def test_eval_mode():
    net = torch.nn.Sequential(torch.nn.Dropout())
    assert net.training
    with A.eval_mode(net) as m:
        assert m is net and not net.training and not net[0].training
    assert net.training and net[0].training
    with pytest.raises(KeyError):
        with A.eval_mode(net):
            assert not net.training
            raise KeyError("mid-loader")
    assert net.training
    net.eval()
    with A.eval_mode(net):
        assert not net.training
    assert not net.training


def test_const_table(monkeypatch):
    monkeypatch.setattr(A, "_CONST", {})
    cpu, made = torch.device("cpu"), []

    def make(v):
        def f():
            made.append(v)
            return np.full(3, v, dtype=np.float32)
        return f
    t = A.const_table("a", 1, make(1.0), cpu)
    assert A.const_table("a", 1, make(9.0), cpu) is t and made == [1.0] and t.tolist() == [1.0, 1.0, 1.0]
    assert A.const_table("b", 1, make(2.0), cpu).tolist() == [2.0] * 3 and A.const_table("a", 1, make(9.0), cpu) is t    # namespaces
    assert A.const_table("a", 1, make(3.0), torch.device("meta")).device.type == "meta" and made == [1.0, 2.0, 3.0]     # per device
    pair = A.const_table("a", 2, lambda: (np.zeros(2), np.ones(2, dtype=np.int32)), cpu)
    assert isinstance(pair, tuple) and pair[0].dtype == torch.float64 and pair[1].tolist() == [1, 1]
    for k in range(3 * A.CONST_TABLES):
        A.const_table("fill", k, make(float(k)), cpu)
        assert len(A._CONST) <= A.CONST_TABLES
    assert A.const_table("fill", 3 * A.CONST_TABLES - 1, make(-1.0), cpu)[0] == 3 * A.CONST_TABLES - 1


def test_device_state(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)

    class Counter(A.DeviceState):
        def __init__(self, device=None):
            self.device = torch.device(device) if device is not None else None
            self.made = []

        def _allocate(self, device):
            self.made.append(device)
    with pytest.raises(RuntimeError, match="Counter: .*no CPU path"):
        Counter()._ensure(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        Counter("cpu")._ensure()
    c = Counter()
    assert c._ensure(torch.device("cuda")) is c and c.made == [torch.device("cuda", 0)] and c.device == torch.device("cuda", 0)
    assert c._ensure() is c and c._ensure(torch.device("cuda", 0)) is c and len(c.made) == 1
    with pytest.raises(ValueError, match="lives on cuda:0, the tensors on cuda:1"):
        c._ensure(torch.device("cuda", 1))
    assert Counter("cuda:1")._ensure().made == [torch.device("cuda", 1)]


# ------------------------------------------------------------------------------------------ the drift the shared rules removed
def test_label_map_entries_raise_alike():
    from uda_aerial_semantic_segmentation_research_amd import active, boundary, regions, render
    entries = (lambda m: boundary.distance2(m, 2), lambda m: boundary.erode(m, 2), lambda m: render.colorize(m),
               lambda m: active.mode_filter(m, 1, 5), lambda m: active.impurity(m, 1, 5), lambda m: regions.label(m),
               lambda m: regions.sieve(m, 4))
    for call in entries:
        with pytest.raises(ValueError):
            call(torch.zeros(1, 4, 4))                                   # float32: the value, on any device
        with pytest.raises(ValueError):
            call(torch.zeros(0, 4, 4, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_a_bool_is_no_class_count():
    from uda_aerial_semantic_segmentation_research_amd import boundary, calibration, curves, mix, proto, pseudo, regions
    for make in (pseudo.ConfidenceHistogram, curves.ScoreHistogram, calibration.ReliabilityHistogram, proto.PrototypeBank,
                 lambda c: boundary.BoundaryStats(c, 2), regions.RegionStats, lambda c: mix.MixedLoader([], [], c),
                 lambda c: pseudo.PseudoLabeler(torch.nn.Identity(), c)):
        with pytest.raises(ValueError, match="num_classes"):
            make(True)
        with pytest.raises(ValueError, match="num_classes"):
            make(5.0)
    for bad in (dict(bins=15.5), dict(bins=True), dict(bins="15")):
        with pytest.raises(ValueError, match="bins"):
            calibration.ReliabilityHistogram(23, **bad)


def test_evaluate_restores_training_mode_when_the_model_raises(monkeypatch):
    from uda_aerial_semantic_segmentation_research_amd import boundary, calibration, curves, regions

    class Net(torch.nn.Module):
        def forward(self, x):
            raise KeyError("mid-loader")

    class Stays(torch.Tensor):                   # a batch that is "moved to the device" without one
        def to(self, *args, **kwargs):
            return self
    batch = [(torch.zeros(1, 3, 8, 8).as_subclass(Stays), torch.zeros(1, 8, 8, dtype=torch.int64).as_subclass(Stays))]
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(calibration.TemperatureScaler, "_allocate", lambda self, device: None)
    dev = torch.device("cuda", 0)
    calls = [lambda net: boundary.evaluate(net, batch, 5, dev), lambda net: regions.evaluate(net, batch, 5, dev),
             lambda net: calibration.evaluate(net, batch, 5, dev), lambda net: calibration.TemperatureScaler().fit(net, batch, dev)]
    for call in calls:
        net = Net()
        with pytest.raises(KeyError, match="mid-loader"):
            call(net)
        assert net.training
    net = Net()
    with monkeypatch.context() as m:             # curves.evaluate makes its confusion matrix on the device before the loop
        m.setattr(curves.torch, "zeros", lambda *a, **kw: None)
        with pytest.raises(KeyError, match="mid-loader"):
            curves.evaluate(net, batch, 5, dev)
    assert net.training
