"""GPU checks of the mean teacher: ``udaseg_ema_flat`` (csrc/optim.hip) element-wise against the float64 mirror tests/_teacher_ref.py,
and teacher.py (``MeanTeacher``, ``OnlineLabeler``), the trainer hook and the checkpoint argument on an r18 Unet at 64 x 64."""
import warnings

import numpy as np
import pytest
import torch

from _teacher_ref import dist2_ref, ema_ref, operands

pytestmark = pytest.mark.gpu

PARTIALS = 256                                                       # UDASEG_SUMSQ_PARTIALS (include/udaseg.h)
COUNTS = (1, 3, 4, 5, 1023, 4097, 2 * 4 * 1024 * PARTIALS + 7)        # the last: every thread at least twice round the grid-stride loop
DECAYS = (0.0, 0.5, 0.99, 0.999, 1.0 - 2.0 ** -20, 1.0)
OFFSETS = ((0, 0), (1, 0), (3, 0), (0, 1), (0, 3), (1, 3), (3, 1), (1, 1))   # storage offsets (floats) of t and s: vector form, scalar form, mixed
GUARD = 8
SENTINEL = np.float32(-7.25)
CLASSES = 5


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    return kernels


def _scratch():
    return torch.zeros(PARTIALS + 1, dtype=torch.float64, device="cuda"), torch.zeros((), dtype=torch.float64, device="cuda")


def _placed(values, off):
    """``values`` as a view at storage offset ``off`` (floats) of a 16-byte aligned buffer with sentinels all round it."""
    buf = torch.full((off + len(values) + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + len(values)]
    view.copy_(torch.from_numpy(values))
    return buf, view


def _guards_intact(buf, off, count):
    b = buf.cpu().numpy()
    return bool(np.all(b[:off] == SENTINEL) and np.all(b[off + count:] == SENTINEL))


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("count", COUNTS)
def test_ema_flat_against_float64(K, count):
    t0, s0 = operands(count, seed=count, same_share=0.05)
    same = s0 == t0
    assert count < 16 or same.any()
    partials, dist2 = _scratch()
    for decay in DECAYS:
        e, B = ema_ref(t0, s0, decay)
        for ot, os_ in OFFSETS:
            tb, t = _placed(t0, ot)
            sb, s = _placed(s0, os_)
            K.ema_flat(t, s, count, decay, partials, dist2)
            got = t.cpu().numpy()
            where = f"count {count} decay {decay} offsets {(ot, os_)}"
            assert _guards_intact(tb, ot, count) and np.array_equal(sb.cpu().numpy()[os_:os_ + count], s0), where
            err = np.abs(got.astype(np.float64) - e)
            assert np.all(err <= B), (where, float((err / B).max()))
            if decay == 0.0:
                assert np.array_equal(got.view(np.int32), s0.view(np.int32)), where          # the copy, bit for bit
            if decay == 1.0:
                assert np.array_equal(got.view(np.int32), t0.view(np.int32)), where          # unchanged, bit for bit
            assert np.array_equal(got.view(np.int32)[same], t0.view(np.int32)[same]), where    # s == t: unchanged, bit for bit
            want = dist2_ref(s0, got)
            assert abs(float(dist2) - want) <= count * 2.0 ** -53 * want, (where, float(dist2), want)
            if (ot, os_) in ((0, 0), (1, 3)):                                                  # without dist2: the same bits
                tb2, t2 = _placed(t0, ot)
                K.ema_flat(t2, s, count, decay)
                assert np.array_equal(t2.cpu().numpy().view(np.int32), got.view(np.int32)) and _guards_intact(tb2, ot, count), where


@pytest.mark.parametrize("count", (4097, COUNTS[-1]))
def test_ema_flat_distance_is_reproducible_and_accumulates(K, count):
    t0, s0 = operands(count, seed=3 * count)
    partials, dist2 = _scratch()
    runs = []
    for _ in range(2):
        t = torch.from_numpy(t0).cuda()
        K.ema_flat(t, torch.from_numpy(s0).cuda(), count, 0.99, partials, dist2)
        runs.append((t.cpu().numpy().view(np.int32), dist2.cpu().numpy().view(np.int64).copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    once = float(dist2)
    t = torch.from_numpy(t0).cuda()
    K.ema_flat(t, torch.from_numpy(s0).cuda(), count, 0.99, partials, dist2, accumulate=True)
    assert float(dist2) == once + once
    K.ema_flat(t, torch.from_numpy(s0).cuda(), count, 1.0, partials, dist2)                   # decay 1: nothing written, the distance still summed
    want = dist2_ref(s0, t.cpu().numpy())
    assert abs(float(dist2) - want) <= count * 2.0 ** -53 * want
    assert int(partials[PARTIALS:].view(torch.int64)[0]) == 0                                     # the arrival counter is cleared again


def test_ema_flat_refuses_bad_calls_before_any_launch(K):
    base = torch.arange(100, dtype=torch.float32, device="cuda")
    keep = base.clone()
    other = torch.ones(60, dtype=torch.float32, device="cuda")
    partials, dist2 = _scratch()
    with pytest.raises(RuntimeError, match="overlap"):
        K.ema_flat(base[:60], base[40:], 60, 0.5)
    with pytest.raises(RuntimeError, match="overlap"):
        K.ema_flat(base[40:], base[:60], 60, 0.5)
    for decay in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="decay"):
            K.ema_flat(base[:60], other, 60, decay)
    with pytest.raises(RuntimeError, match="partials"):
        K.ema_flat(base[:60], other, 60, 0.5, None, dist2)
    with pytest.raises(ValueError):
        K.ema_flat(base[:60], other, 61, 0.5)                                                 # s shorter than count
    with pytest.raises(ValueError):
        K.ema_flat(base[:60], other.double(), 60, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(base, keep) and float(dist2) == 0.0
    K.ema_flat(base[:60], base[60:], 40, 0.0)                                                 # adjacent ranges do not overlap
    assert torch.equal(base[:40], keep[60:]) and torch.equal(base[40:], keep[40:])


# ----------------------------------------------------------------------------------------------------------------- the network
def _unet(seed=0):
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(seed)
    return Unet("resnet18", encoder_weights=None, in_channels=3, classes=CLASSES).to("cuda").train()


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 64, 64, generator=g).cuda(), torch.randint(0, CLASSES, (2, 64, 64), generator=g).cuda()


def _trainer(net):
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    tr = SegmentationTrainer(net, torch.device("cuda", 0))
    return tr, FusedAdam(net.parameters(), lr=1e-3)


def _numpy_state(model):
    return {k: v.detach().cpu().contiguous().numpy().copy() for k, v in model.state_dict().items()}


def _bits_equal(a, b):
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def _drift(net, factor):
    """Moves every parameter of the student (in place, through its arena views), as an optimiser step would."""
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(factor)


def test_construction():
    from uda_aerial_semantic_segmentation_research_amd import engine
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    net = _unet()
    mt = MeanTeacher(net)
    assert type(mt.model) is type(net) and mt.model is not net
    assert _bits_equal(_numpy_state(net), _numpy_state(mt.model))
    ptr = lambda t: t.untyped_storage().data_ptr()      # noqa: E731
    mine = {ptr(t) for t in list(mt.model.parameters()) + list(mt.model.buffers())}
    theirs = {ptr(t) for t in list(net.parameters()) + list(net.buffers())}
    assert not mine & theirs
    assert engine.arena_owner(ptr(mt.model._arena)) is mt.model and engine.arena_owner(ptr(net._arena)) is net
    assert mt.model._arena_ok() and net._arena_ok()
    assert all(not p.requires_grad for p in mt.model.parameters()) and all(p.requires_grad for p in net.parameters())
    assert not mt.model.training and net.training
    assert all(p.device == q.device for p, q in zip(mt.model.parameters(), net.parameters()))
    assert mt.model.compute_dtype == net.compute_dtype and mt.step == 0


@pytest.mark.parametrize("buffers", ["copy", "ema", "keep"])
def test_three_train_steps(buffers):
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    net = _unet()
    tr, opt = _trainer(net)
    x, y = _batch()
    mt = MeanTeacher(net, alpha=0.99, buffers=buffers)
    params = {k for k, _ in net.named_parameters()}
    start = _numpy_state(mt.model)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*MeanTeacher.*")      # the whole-arena path does not warn
        for step in range(3):
            prev = _numpy_state(mt.model)
            tr.train_step(x, y, opt)
            mt.update()
            decay = mt.decay_at(step)
            assert decay == (0.0, 0.5, 1.0 - 1.0 / 3)[step] and mt.step == step + 1
            assert mt.flat_launches == (2 if buffers == "ema" else 1)
            stu, tea = _numpy_state(net), _numpy_state(mt.model)
            d2 = 0.0
            for k in tea:
                if k in params:
                    e, B = ema_ref(prev[k], stu[k], decay)
                    assert np.all(np.abs(tea[k].astype(np.float64) - e) <= B), (step, k)
                    if step == 0:
                        assert np.array_equal(tea[k].view(np.int32), stu[k].view(np.int32)), k      # warm-up: the first update is the copy
                    d2 += dist2_ref(stu[k], tea[k])
                elif buffers == "copy":
                    assert np.array_equal(tea[k], stu[k]), (step, k)
                elif buffers == "keep":
                    assert np.array_equal(tea[k], start[k]), (step, k)
                elif k.endswith("num_batches_tracked"):
                    assert np.array_equal(tea[k], stu[k]) and int(tea[k]) > 0, (step, k)
                else:
                    e, B = ema_ref(prev[k], stu[k], decay)
                    assert np.all(np.abs(tea[k].astype(np.float64) - e) <= B), (step, k)
            n = mt.model._arena.numel()
            got = float(mt.distance()) ** 2
            assert abs(got - d2) <= 2 * n * 2.0 ** -53 * d2 and (d2 > 0) == (step > 0), (step, got, d2)
            # the padding lanes stay zero: blank every logical view of a copy of the arena, and nothing is left
            a = mt.model._arena.clone()
            for p, o, cnt, shp, mod, name in mt.model._entries:
                mt.model._logical_view(a[o:o + cnt], mod, name, tuple(p.shape)).zero_()
            assert not bool(a.any()), step


def test_teacher_forward_sees_the_update():
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    net = _unet()
    tr, opt = _trainer(net)
    x, y = _batch()
    mt = MeanTeacher(net, alpha=0.9, warmup=False)
    with torch.no_grad():
        before = mt.model(x).clone()
    tr.train_step(x, y, opt)
    mt.update()
    fresh = Unet("resnet18", encoder_weights=None, in_channels=3, classes=CLASSES).to("cuda").eval()
    fresh.load_state_dict(mt.model.state_dict())
    with torch.no_grad():
        got, want = mt.model(x), fresh(x)
    assert torch.equal(got, want)
    assert not torch.equal(got, before)


def test_relaying_follows_the_student():
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    net = _unet()
    mt = MeanTeacher(net, alpha=1.0, warmup=False)
    _drift(net, 1.25)
    before = _numpy_state(mt.model)
    n0 = mt.model._arena.numel()
    net.set_compute_dtype(torch.bfloat16)
    assert net._arena.numel() != n0                                     # the student's arena was re-laid (8-channel padding)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*MeanTeacher.*")
        mt.update()                                                     # decay 1: re-lays the teacher, changes no value
        assert mt.flat_launches == 1 and mt.model.compute_dtype == torch.bfloat16
        assert mt.model._arena.numel() == net._arena.numel() and mt.model._arena_ok()
        assert _bits_equal(before, _numpy_state(mt.model))
        mt.alpha = 0.5
        mt.update()
        assert mt.flat_launches == 1
    stu, tea = _numpy_state(net), _numpy_state(mt.model)
    for k, _ in net.named_parameters():
        e, B = ema_ref(before[k], stu[k], 0.5)
        assert np.all(np.abs(tea[k].astype(np.float64) - e) <= B), k


def test_state_dict_round_trip_and_sync():
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    net = _unet()
    mt = MeanTeacher(net, alpha=0.97, buffers="ema")
    for f in (1.5, 0.75):
        _drift(net, f)
        mt.update()
    sd = mt.state_dict()
    assert sorted(sd) == ["alpha", "buffers", "model", "step", "warmup"]
    assert all(v.device.type == "cpu" and v.is_contiguous() for v in sd["model"].values())
    net2 = _unet(seed=5)
    mt2 = MeanTeacher(net2)
    mt2.load_state_dict(sd)
    assert _bits_equal(_numpy_state(mt.model), _numpy_state(mt2.model))
    assert (mt2.step, mt2.alpha, mt2.warmup, mt2.buffers) == (2, 0.97, True, "ema")
    assert mt2.decay_at(mt2.step) == 1.0 - 1.0 / 3                      # the schedule continues
    assert not _bits_equal(_numpy_state(net2), _numpy_state(mt2.model))
    mt2.sync()
    assert _bits_equal(_numpy_state(net2), _numpy_state(mt2.model)) and mt2.step == 2
    assert float(mt2.distance()) == 0.0


def test_per_tensor_fallback_warns_once():
    """A student that is no ArenaModule: same arithmetic per tensor, dense fp32 tensors through the kernel."""
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    torch.manual_seed(2)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3), torch.nn.BatchNorm2d(6)).cuda()
    mt = MeanTeacher(net, alpha=0.9, warmup=False)
    with torch.no_grad():
        net[1].running_mean.add_(0.25)
        net[1].num_batches_tracked.add_(3)
    for step in range(2):
        prev = _numpy_state(mt.model)
        _drift(net, 1.5)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            mt.update()
        assert len([w for w in caught if "per-tensor" in str(w.message)]) == (1 if step == 0 else 0)      # warns once
        stu, tea = _numpy_state(net), _numpy_state(mt.model)
        d2 = 0.0
        for k, _ in net.named_parameters():
            e, B = ema_ref(prev[k], stu[k], 0.9)
            assert np.all(np.abs(tea[k].astype(np.float64) - e) <= B), (step, k)
            d2 += dist2_ref(stu[k], tea[k])
        assert np.array_equal(tea["1.running_mean"], stu["1.running_mean"]) and int(tea["1.num_batches_tracked"]) == 3
        assert abs(float(mt.distance()) ** 2 - d2) <= 1e-12 * d2 and mt.flat_launches == 0


class _Recorder:
    """Stands in for a teacher, and wraps an optimiser's ``step``: both write into one list, so that the order can be read off."""

    def __init__(self):
        self.events = []

    def update(self):
        self.events.append("update")

    def watch(self, optimizer):
        step = optimizer.step

        def recorded(*a, **k):
            self.events.append("step")
            return step(*a, **k)
        optimizer.step = recorded
        return optimizer


def _two_steps(teacher):
    """Two train steps of a freshly seeded network -> (fp32 losses, the order of optimiser steps and teacher updates, trainer);
    ``teacher``: "untouched" (the attribute is never assigned), "none" (assigned None), "stub" (a recorder) or "set" (a MeanTeacher)."""
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    x, y = _batch()
    net = _unet(seed=7)
    tr, opt = _trainer(net)
    rec = _Recorder()
    rec.watch(opt)
    if teacher == "untouched":
        assert tr.teacher is None
    elif teacher == "none":
        tr.teacher = None
    else:
        tr.teacher = rec if teacher == "stub" else MeanTeacher(net)
    losses = [tr.train_step(x, y, opt)[0].detach().cpu().numpy().copy() for _ in range(2)]
    return losses, rec.events, tr


def test_trainer_hook():
    """With a teacher, every optimiser step is followed at once by one update; with ``teacher = None`` (assigned or never touched)
    the step reaches no update, and the student's losses are those of a trainer with a teacher: the teacher only reads it.
    Compared bit for bit: the first loss (the forward is bitwise reproducible).  The second loss follows a backward pass whose
    weight gradients are not bitwise reproducible between two runs of the same code (fp32 split-K atomics),
    so across runs it is held to the relative run-to-run spread tests/test_gpu_suites.py allows the step, 2e-6."""
    runs = {k: _two_steps(k) for k in ("untouched", "none", "stub", "set")}
    assert runs["untouched"][1] == runs["none"][1] == ["step", "step"]
    assert runs["stub"][1] == ["step", "update", "step", "update"]
    assert runs["set"][1] == ["step", "step"] and runs["set"][2].teacher.step == 2
    assert float(runs["set"][2].teacher.distance()) > 0.0
    first, second = runs["untouched"][0]
    for name, (losses, _, _) in runs.items():
        print(f"{name}: losses {losses[0]!r} {losses[1]!r}")
        assert losses[0].tobytes() == first.tobytes(), name
        assert abs(float(losses[1]) - float(second)) <= 2e-6 * abs(float(second)), name


def test_adversarial_and_finetuning_trainers_update_the_teacher():
    """The same one line after the segmenter's optimiser step in ``AdversarialTrainer`` and ``UnsupervisedTrainer``; phase 3 logs
    the teacher's scalars on its own schedule."""
    from uda_aerial_semantic_segmentation_research_amd.adversarial_trainer import AdversarialTrainer
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    from uda_aerial_semantic_segmentation_research_amd.unsupervised_trainer import UnsupervisedTrainer
    dev = torch.device("cuda", 0)
    x, y = _batch()
    g = torch.Generator().manual_seed(6)
    target = torch.randn(2, 3, 64, 64, generator=g)
    net = _unet(seed=11)
    at = AdversarialTrainer(net, dev, lambda_adv=0.001)
    rec = _Recorder()
    opt = rec.watch(FusedAdam(net.parameters(), lr=1e-4))
    at.teacher = rec
    at.train_epoch([(x, y), (x, y)], [target], opt, epoch=1)
    assert rec.events == ["step", "update", "step", "update"]              # the segmenter's optimiser, not the discriminator's
    at.teacher = mt = MeanTeacher(net)
    at.train_epoch([(x, y), (x, y)], [target], opt, epoch=2)
    assert mt.step == 2 and float(mt.distance()) > 0.0
    at.teacher = None
    rec.events.clear()
    at.train_epoch([(x, y)], [target], opt, epoch=3)
    assert rec.events == ["step"]

    seg = _unet(seed=12)
    ut = UnsupervisedTrainer(seg, dev, rampup_length=1, log_interval=1, seed=3)
    rec = _Recorder()
    opt = rec.watch(FusedAdam(ut.model.parameters(), lr=1e-4))
    frames = [_frames(g), _frames(g)]
    ut.teacher = rec
    assert not ut.finetune_step(frames[0], opt, 1)["skipped"] and rec.events == ["step", "update"]
    ut.teacher = mt = MeanTeacher(seg)
    ut.train_epoch(frames, opt, 1)
    assert mt.step == 2 and ut.skipped == 0
    assert [v for _, v in ut.logger.scalars["train/teacher_decay"]] == [0.0, 0.5]
    assert [v >= 0.0 for _, v in ut.logger.scalars["train/teacher_distance"]] == [True, True]


# ------------------------------------------------------------------------------------------------------------------ the labeler
class _Batches:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _frames(g, n=2, h=64, w=64):
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)


def test_online_labeler_thresholds_follow_its_own_batches():
    from uda_aerial_semantic_segmentation_research_amd import pseudo
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher, OnlineLabeler
    net = _unet(seed=9)
    mt = MeanTeacher(net)
    lab = OnlineLabeler(mt, CLASSES, portion=0.3, floor=0.1, cap=0.9, halve_every=2)
    assert lab.model is mt.model
    with pytest.raises(RuntimeError):
        lab.report()
    g = torch.Generator().manual_seed(10)
    table = np.zeros((CLASSES, pseudo.BINS), dtype=np.int64)
    for i in range(3):
        frames = _frames(g).cuda()
        with torch.no_grad():
            logits = lab._forward(frames)                               # the teacher is in eval mode: the forward label() makes
        own = pseudo.ConfidenceHistogram(CLASSES).update(logits).table.cpu().numpy()
        if i == 2:
            table >>= 1                                                 # halve_every = 2: before the third update
        table += own
        masks = lab.label(frames)
        assert np.array_equal(lab.hist.table.cpu().numpy(), table), i
        thr, _ = pseudo.thresholds_from_hist(lab.hist.table, 0.3, 0.1, 0.9)
        assert np.array_equal(lab.thr_bins.cpu().numpy(), thr), i
        want = pseudo.pseudo_labels(logits, torch.from_numpy(thr).cuda(), 255)
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (2, 64, 64) and torch.equal(masks, want), i
    assert lab.calls == 3 and not mt.model.training
    # any model will do, and its training flag is restored
    lab2 = OnlineLabeler(net, CLASSES)
    lab2.label(frames)
    assert net.training and lab2.model is net


def test_whole_chain_and_report():
    from uda_aerial_semantic_segmentation_research_amd import data as D, mix as M, pseudo
    from uda_aerial_semantic_segmentation_research_amd.config import Config
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher, OnlineLabeler
    from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer
    net = _unet(seed=3)
    g = torch.Generator().manual_seed(4)
    source = _Batches([(_frames(g), torch.randint(0, CLASSES, (2, 64, 64), generator=g).to(torch.uint8)) for _ in range(2)])
    target = _Batches([_frames(g) for _ in range(2)])
    mt = MeanTeacher(net, alpha=0.99)
    lab = OnlineLabeler(mt, num_classes=CLASSES, portion=0.2, cap=0.9, halve_every=100)
    mixed = M.MixedLoader(source, lab.loader(target), num_classes=CLASSES, generator=torch.Generator().manual_seed(5))
    tr = SegmentationTrainer(net, torch.device("cuda", 0), criterion=CrossEntropyLoss(ignore_index=255))
    tr.teacher = mt
    loader = D.DeviceAugmentedLoader(mixed, generator=torch.Generator().manual_seed(9))
    loss = tr.train_epoch(loader, FusedAdam(net.parameters(), lr=1e-4), 1)
    assert np.isfinite(loss) and mt.step == len(loader) == 2 and lab.calls == 2
    fitted = pseudo.PseudoLabeler(net, CLASSES).fit(target)
    rep = lab.report()
    assert set(rep) == set(fitted.report()) and len(rep["threshold"]) == CLASSES
    assert sum(rep["support"]) + rep["nonfinite"] == 2 * 2 * 64 * 64
    assert Config.LOG_INTERVAL >= 2                                      # two batches: logged at batch 0 only
    assert tr.logger.scalars["train/teacher_decay"] == [(0, 0.0)]
    (step, dist), = tr.logger.scalars["train/teacher_distance"]
    assert step == 0 and dist == 0.0                                     # the warm-up's first update is the copy


def test_phase_checkpoint_carries_the_teacher(tmp_path):
    from uda_aerial_semantic_segmentation_research_amd import checkpoint as C
    from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher
    net = _unet()
    mt = MeanTeacher(net, alpha=0.95)
    for f in (1.5, 0.75, 1.1):
        _drift(net, f)
        mt.update()
    today = ["metrics", "model_state_dict", "phase", "timestamp"]
    p = C.save_phase_checkpoint(tmp_path / "plain", net, {}, "SEGMENTATION")
    assert sorted(torch.load(p, weights_only=False)) == today
    p = C.save_phase_checkpoint(tmp_path / "t", net, {"iou": 0.5}, "SEGMENTATION", teacher=mt)
    assert sorted(torch.load(p, weights_only=False)) == sorted(today + ["teacher_state_dict"])
    net2 = _unet(seed=8)
    mt2 = MeanTeacher(net2)
    ck = C.load_phase_checkpoint(tmp_path / "t", net2, load_best=False, teacher=mt2)
    assert ck["metrics"] == {"iou": 0.5}
    assert _bits_equal(_numpy_state(net), _numpy_state(net2)) and _bits_equal(_numpy_state(mt.model), _numpy_state(mt2.model))
    assert mt2.step == 3 and mt2.alpha == 0.95
    net3 = _unet(seed=8)
    mt3 = MeanTeacher(net3)
    C.load_phase_checkpoint(tmp_path / "plain", net3, load_best=False, teacher=mt3)          # no teacher in the file: left as it is
    assert mt3.step == 0
