"""Phase 3 on the device: ``data.strong_views`` (csrc/augment.hip) stage by stage against the float64 numpy restatement of
its definition (tests/_strong_aug_ref.py), ``optim.clip_grad_norm_`` against a float64 restatement on the real gradient arenas,
two live ``Unet`` plans in one autograd graph, and ``UnsupervisedTrainer.finetune_step`` against a torch restatement built
from the oracle classes.

How the augmentation bars come about: the restatement is evaluated in float32 as well as in float64 on the same records; the
largest distance between the two (per sample, on the normalised output) is what a float32 evaluation of the definition may
differ by, and the kernel has to stay within 4 x that (another summation order and fused multiply-adds earn the factor).
Where the two evaluations agree exactly the bar is 2 ulp of fp32 at the output's magnitude.  Pixels whose chroma entering the
HSV stage is above 0 and below 0.5 level (hue decided by rounding noise) are left out of the HSV and full-chain comparisons;
their share is capped at 0.2 % of a batch.  Set UDASEG_DEVIATION_LOG to a file name to collect the measured figures.
"""
import math
import os

import numpy as np
import pytest
import torch

import _strong_aug_ref as R

pytestmark = pytest.mark.gpu

LABELS = ("d4", "noise", "box", "median", "motion", "affine", "sharpen", "emboss", "bc", "hsv", "chain")
SIZES = ((24, 24), (65, 65), (17, 33), (512, 512))
MASKED = ("hsv", "chain")
ILL_CAP = 0.002


def frames(name, n, h, w):
    """"random": independent uniform channels (colourful: the worst case for interpolation); "smooth": a colour gradient."""
    if name == "random":
        return np.random.default_rng(1000 + h * 7 + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        t = i / max(n - 1, 1)
        out[i, :, :, 0] = np.round(40 + 150 * x + 20 * t)
        out[i, :, :, 1] = np.round(215 - 120 * y - 15 * t)
        out[i, :, :, 2] = np.round(25 + 50 * (x + y) + 60 * t * x)
    return out


def records(D, n, h, w, labels):
    """(label, StrongAugParams) with sample i on D4 code i (non-transposing codes on non-square frames) and the label's
    stage(s) switched on with parameters that sweep the stated ranges."""
    codes = list(range(8)) if h == w else [0, 2, 4, 6]
    for label in labels:
        P = D.StrongAugParams(n, h, w, [codes[i % len(codes)] for i in range(n)])
        chain = label == "chain"
        for i in range(n):
            t = i / max(n - 1, 1)
            if label == "noise" or chain:
                P.set_noise(i, math.sqrt(20 + 60 * t), ((0x9E3779B9 * (i + 1)) & 0xFFFFFFFF, 0xDEADBEEF ^ (i * 2654435761 & 0xFFFFFFFF)))
            if label == "box":
                P.set_blur(i, D.BLUR_BOX, 3 if i % 2 == 0 else 5)
            if label == "median":
                P.set_blur(i, D.BLUR_MEDIAN, 3 if i % 2 == 0 else 5)
            if label == "motion":
                P.set_blur(i, D.BLUR_MOTION, 3 if i < n // 2 else 5, i % 4)
            if chain:
                P.set_blur(i, i % 3, 3 if (i // 3) % 2 == 0 else 5, (i + 1) % 4)
            if label == "affine" or chain:
                P.set_affine(i, (2 * t - 1) * 0.1 * w, (1 - 2 * t) * 0.1 * h, 0.7 + 0.6 * t, -60 + 120 * t)
            if label == "sharpen" or (chain and i % 3 == 0):
                P.set_stage5(i, D.STAGE5_SHARPEN, 0.2 + 0.3 * t, 1.0 - 0.5 * t)
            if label == "emboss" or (chain and i % 3 == 1):
                P.set_stage5(i, D.STAGE5_EMBOSS, 0.5 - 0.3 * t, 0.2 + 0.5 * t)
            if label == "bc" or (chain and i % 3 == 2):
                P.set_stage5(i, D.STAGE5_BRIGHTNESS_CONTRAST, -0.3 + 0.6 * t, 0.3 - 0.6 * ((i * 3) % n) / max(n - 1, 1))
            if label == "hsv" or chain:
                P.set_hsv(i, -20 + 40 * t, 30 - 60 * ((i * 3) % n) / max(n - 1, 1), -20 + 40 * ((i * 5) % n) / max(n - 1, 1))
        yield label, P


@pytest.fixture(scope="module")
def D():
    from uda_aerial_semantic_segmentation_research_amd import _lib, data
    _lib.require_gpu()
    return data


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).float().cpu().numpy()


# --------------------------------------------------------------------------------------------------- the generator
def test_philox_words_on_device(D):
    from test_finetune_host import PHILOX_KAT
    ctr = torch.from_numpy(np.array([k[0] for k in PHILOX_KAT], dtype=np.uint32).view(np.int32)).cuda()
    key = torch.from_numpy(np.array([k[1] for k in PHILOX_KAT], dtype=np.uint32).view(np.int32)).cuda()
    got = D.philox4x32(ctr, key).cpu().numpy().view(np.uint32)
    assert [tuple(int(x) for x in row) for row in got] == [k[2] for k in PHILOX_KAT]
    rng = np.random.default_rng(0)
    c, k = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint32), rng.integers(0, 1 << 32, (1000, 2), dtype=np.uint32)
    got = D.philox4x32(torch.from_numpy(c.view(np.int32)).cuda(), torch.from_numpy(k.view(np.int32)).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.philox4x32_10(c, k))


# ------------------------------------------------------------------------------- every stage and the chain, value by value
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("name", ("random", "smooth"))
@pytest.mark.parametrize("label", LABELS)
def test_stage_against_float64_definition(D, label, name, h, w):
    n = 8
    imgs = frames(name, n, h, w)
    (_, P), = records(D, n, h, w, (label,))
    ref64, ill = R.run(imgs, P, np.float64)
    ref32, _ = R.run(imgs, P, np.float32)
    assert ill.mean() <= ILL_CAP, f"ill-conditioned share {ill.mean():.5f} above the cap: change the input"
    keep = ~ill if label in MASKED else np.ones_like(ill)
    dev_img = torch.from_numpy(imgs).cuda()
    got32 = D.strong_views(dev_img, P)
    assert got32.shape == (n, 3, h, w) and got32.dtype == torch.float32
    got = _nhwc(got32).astype(np.float64)
    assert np.isfinite(got).all()
    worst, failures = None, []
    for i in range(n):
        k = keep[i]
        dev = np.abs(ref32[i].astype(np.float64) - ref64[i])[k].max()
        floor = 2 * float(np.spacing(np.float32(np.abs(ref64[i]).max())))
        bar = max(4 * dev, floor)
        err = np.abs(got[i] - ref64[i])[k].max()
        if worst is None or err / bar > worst[0] / worst[2]:
            worst = (err, dev, bar)
        if not err <= bar:
            failures.append((i, err, dev, bar))
    _log(f"strong_aug {label:8s} {name:6s} {h:3d}x{w:<3d}  kernel-vs-f64 {worst[0]:.3e}  f32-vs-f64 {worst[1]:.3e}  bar {worst[2]:.3e}  "
         f"left out {ill.mean() if label in MASKED else 0.0:.5f}")
    assert not failures, failures
    if label == "d4":                                           # nothing but the basic pipeline: exact
        assert np.array_equal(_nhwc(got32), ref32)
    got16 = D.strong_views(dev_img, P, dtype=torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, got32.to(torch.bfloat16))


def test_drawn_records_full_pipeline(D):
    """Records as training draws them (mixed stages per sample), both views of one call."""
    n, h, w = 16, 64, 64
    imgs = frames("random", n, h, w)
    g = torch.Generator().manual_seed(11)
    Pa, Pb = D.draw_strong_params(n, h, w, g), D.draw_strong_params(n, h, w, g)
    va, vb = D.strong_views(torch.from_numpy(imgs), Pa, Pb)                    # host frames: one upload for both views
    for P, v in ((Pa, va), (Pb, vb)):
        ref64, ill = R.run(imgs, P, np.float64)
        ref32, _ = R.run(imgs, P, np.float32)
        assert ill.mean() <= ILL_CAP
        got = _nhwc(v).astype(np.float64)
        for i in range(n):
            k = ~ill[i]
            dev = np.abs(ref32[i].astype(np.float64) - ref64[i])[k].max()
            bar = max(4 * dev, 2 * float(np.spacing(np.float32(np.abs(ref64[i]).max()))))
            err = np.abs(got[i] - ref64[i])[k].max()
            assert err <= bar, (i, int(P.flags[i]), err, dev, bar)


# --------------------------------------------------------------------------------------------- exactness and determinism
@pytest.mark.parametrize("h,w", [(24, 24), (17, 33), (512, 512)])
def test_all_off_is_prepare_batch_and_calls_are_deterministic(D, h, w):
    n = 8
    imgs = torch.from_numpy(frames("random", n, h, w)).cuda()
    codes = torch.tensor(list(range(8)) if h == w else [0, 2, 4, 6, 0, 2, 4, 6], dtype=torch.int32)
    off = D.StrongAugParams(n, h, w, codes.numpy())
    for dtype in (torch.float32, torch.bfloat16):
        want, _ = D.prepare_batch(imgs, None, codes, dtype=dtype)
        got = D.strong_views(imgs, off, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got, want)
        assert got.stride() == want.stride()
    g = torch.Generator().manual_seed(3)
    Pa, Pb = D.draw_strong_params(n, h, w, g), D.draw_strong_params(n, h, w, g)
    (_, chain), = records(D, n, h, w, ("chain",))
    a1, b1 = D.strong_views(imgs, Pa, Pb)
    a2, b2 = D.strong_views(imgs, Pa, Pb)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)                        # the same records twice: the same bits
    assert torch.equal(D.strong_views(imgs, Pa), a1) and torch.equal(D.strong_views(imgs, Pb), b1)   # = two single-view calls
    c1, o1 = D.strong_views(imgs, chain, off)                                 # a view that needs the source pass next to one that does not
    assert torch.equal(c1, D.strong_views(imgs, chain)) and torch.equal(o1, D.strong_views(imgs, off))
    with pytest.raises(ValueError):
        D.strong_views(imgs.float(), Pa)
    with pytest.raises(ValueError):
        D.strong_views(imgs[:4], Pa)
    with pytest.raises(ValueError):
        D.strong_views(imgs, Pa.table)


def test_views_feed_the_stem_without_a_copy(D):
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda().eval()
    imgs, _ = D.synthetic_u8_batch(2, 64, 64, seed=4)
    g = torch.Generator().manual_seed(2)
    a, b = D.strong_views(imgs, D.draw_strong_params(2, 64, 64, g), D.draw_strong_params(2, 64, 64, g))
    for v in (a, b):
        pv = net._padded_input_view(v)
        assert pv is not None and pv.data_ptr() == v.data_ptr()
        with torch.no_grad():
            assert torch.equal(net(v), net(v.contiguous()))


def test_noise_statistics(D):
    n, h, w, sigma = 2, 512, 512, 8.0
    imgs = torch.full((n, h, w, 3), 128, dtype=torch.uint8).cuda()
    P = D.StrongAugParams(n, h, w)
    for i in range(n):
        P.set_noise(i, sigma, (123 + i, 456))
    out = _nhwc(D.strong_views(imgs, P)).astype(np.float64)
    level = out / np.reciprocal(R.STD * np.float32(255.0), dtype=np.float32).astype(np.float64) + (R.MEAN * np.float32(255.0)).astype(np.float64)
    for i in range(n):
        z = level[i] - 128.0
        cnt = z.size
        assert abs(z.mean()) <= 4 * sigma / math.sqrt(cnt), z.mean()
        assert abs(z.var() - sigma ** 2) <= 4 * sigma ** 2 * math.sqrt(2 / cnt), z.var()
    assert not np.array_equal(level[0], level[1])                             # another key, another field


def test_no_host_synchronisation(D):
    """``strong_views`` and ``clip_grad_norm_`` return while the stream is still busy with work queued before them (a host
    synchronisation anywhere inside would have drained it), and run under torch's sync debug mode where this build honours it."""
    from uda_aerial_semantic_segmentation_research_amd.optim import clip_grad_norm_
    n, h, w = 8, 512, 512
    imgs = torch.from_numpy(frames("random", n, h, w)).cuda()
    g = torch.Generator().manual_seed(5)
    Pa, Pb = D.draw_strong_params(n, h, w, g), D.draw_strong_params(n, h, w, g)
    ps = [torch.nn.Parameter(torch.randn(1000, 33, device="cuda")) for _ in range(3)]
    ps.append(torch.nn.Parameter(torch.randn(64, 50, device="cuda")))
    for p in ps:
        p.grad = torch.randn_like(p)
    ps[-1].grad = torch.randn(50, 64, device="cuda").t()                       # a strided gradient: the torch-op path
    D.strong_views(imgs, Pa, Pb), clip_grad_norm_(ps, 1.0)                     # warm up (allocations, module loads)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    torch.cuda._sleep(int(2e9))                                                # about a second of queued device work
    D.strong_views(imgs, Pa, Pb)
    clip_grad_norm_(ps, 1.0)
    assert not stream.query(), "the calls waited for the device"
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            D.strong_views(imgs, Pa, Pb)
            clip_grad_norm_(ps, 1.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"sync debug mode honoured by this torch build: {honoured}")


# ------------------------------------------------------------------------------------------------- gradient clipping
def _filled_arenas():
    from oracle.adversarial_ref import synthetic_batch
    from uda_aerial_semantic_segmentation_research_amd.discriminator import DomainDiscriminator
    from uda_aerial_semantic_segmentation_research_amd.losses import AdversarialLoss, CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(7)
    seg = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda().train()
    disc = DomainDiscriminator().cuda().train()
    x, y, _ = synthetic_batch(2, 64, 64, seed=3)
    CrossEntropyLoss()(seg(x.cuda()), y.cuda()).backward()
    AdversarialLoss(1.0).generator_loss(disc(x.cuda())).backward()
    torch.cuda.synchronize()
    return seg, disc, list(seg.parameters()) + list(disc.parameters())


def _ulp_ok(got, want):
    want = want.cpu()
    return bool(((got.cpu().double() - want.double()).abs() <= torch.from_numpy(np.spacing(want.abs().numpy())).double()).all())


def test_clip_grad_norm_on_the_real_arenas():
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam, clip_grad_norm_
    seg, disc, ps = _filled_arenas()
    for net in (seg, disc):
        part = list(net.parameters())
        assert FusedAdam._flat_view(part) is not None, "the gradients do not form a whole arena"
    saved = [p.grad.detach().clone() for p in ps]

    def restore():
        for p, s in zip(ps, saved):
            p.grad.copy_(s)

    sumsq = sum(float(s.double().square().sum()) for s in saved)
    total64 = math.sqrt(sumsq)
    assert total64 > 0
    max_norm = 0.37 * total64                                                 # clipping happens
    coef = max_norm / (total64 + 1e-6)
    total = clip_grad_norm_(ps, max_norm)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
    rel = abs(float(total) - total64) / total64
    print(f"clip_grad_norm_: total_norm {float(total):.9g} (fp64 {total64:.12g}) relative error {rel:.2e}")
    assert rel <= 2.5e-7                                                      # one fp32 rounding of an fp64 sum, doubled
    first = [p.grad.detach().clone() for p in ps]
    for p, s in zip(ps, saved):
        assert _ulp_ok(p.grad, (s.double() * coef).float()), "scaled gradient off by more than 1 ulp"
    # torch's own clip on another clone, as a sanity check: its distance from the fp64 norm, times 4, plus our own allowance
    clones = [torch.nn.Parameter(torch.zeros_like(s)) for s in saved]
    for c, s in zip(clones, saved):
        c.grad = s.clone()
    t_total = float(torch.nn.utils.clip_grad_norm_(clones, max_norm))
    assert abs(float(total) - t_total) <= 4 * abs(t_total - total64) + 2.5e-7 * total64
    for c, p in zip(clones, ps):
        assert (c.grad - p.grad).abs().max() <= 1e-5 * max(float(c.grad.abs().max()), 1e-30)
    # two runs: the same bits
    restore()
    total2 = clip_grad_norm_(ps, max_norm)
    assert torch.equal(total, total2) and all(torch.equal(p.grad, f) for p, f in zip(ps, first))
    # a norm below max_norm leaves the gradients bit-identical
    restore()
    arena_before = seg._grad_arena.clone()
    total3 = clip_grad_norm_(ps, 2.0 * total64)
    assert torch.equal(total3, total) and all(torch.equal(p.grad, s) for p, s in zip(ps, saved))
    assert torch.equal(seg._grad_arena, arena_before)
    # a subset takes the per-tensor path (dense tensors through the kernels, strided views through torch ops) and touches
    # nothing else
    restore()
    sub_idx = list(range(0, len(ps), 7))
    sub = [ps[i] for i in sub_idx]
    assert any(p.grad.is_contiguous() for p in sub) and any(not p.grad.is_contiguous() for p in sub)
    sub64 = math.sqrt(sum(float(saved[i].double().square().sum()) for i in sub_idx))
    sub_total = clip_grad_norm_(sub, 0.5 * sub64)
    assert abs(float(sub_total) - sub64) / sub64 <= 2.5e-7
    c2 = 0.5 * sub64 / (sub64 + 1e-6)
    for i, (p, s) in enumerate(zip(ps, saved)):
        if i in sub_idx:
            assert _ulp_ok(p.grad, (s.double() * c2).float())
        else:
            assert torch.equal(p.grad, s)
    # a non-finite norm propagates as torch's does with error_if_nonfinite=False
    restore()
    ps[1].grad[(0,) * ps[1].grad.dim()] = float("nan")
    tn = clip_grad_norm_(ps, 1.0)
    assert math.isnan(float(tn)) and all(bool(torch.isnan(p.grad).all()) for p in ps)


# ----------------------------------------------------------------------------------------------- two live Unet plans
def test_two_live_unet_plans_sum_their_gradients():
    from oracle.adversarial_ref import synthetic_batch
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(21)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23).cuda().train()
    a, y, _ = synthetic_batch(2, 64, 64, seed=5)
    b, _, _ = synthetic_batch(2, 64, 64, seed=6)
    a, b, y = a.cuda(), b.cuda(), y.cuda()
    ce = CrossEntropyLoss()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net.zero_grad()
    la, lb = net(a), net(b)                                                    # both plans alive until the one backward
    (ce(la, y) + ce(lb, y)).backward()
    joint = net._grad_arena.clone()
    stats = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    assert all(p.grad is not None for p in net.parameters())
    net.load_state_dict(state)
    singles = []
    for x in (a, b):
        net.zero_grad()
        ce(net(x), y).backward()
        singles.append(net._grad_arena.clone())
    want = singles[0].double() + singles[1].double()
    e = ((joint.double() - want).abs().max() / want.abs().max()).item()
    print(f"two live plans vs the sum of two backward passes: {e:.3e}")
    assert e <= 1e-5
    after = net.state_dict()
    for k, v in stats.items():                                                 # the running statistics moved twice
        assert torch.equal(v, after[k]), k
        if "num_batches" in k:
            assert int(v) == int(state[k]) + 2


# ------------------------------------------------------------------------------------------- one step against the oracle
def _trainer_pair(**kw):
    from _parity import pair
    from oracle.adversarial_ref import DomainDiscriminatorRef
    from uda_aerial_semantic_segmentation_research_amd.unsupervised_trainer import UnsupervisedTrainer
    ref, net = pair("resnet18")
    torch.manual_seed(99)
    dref = DomainDiscriminatorRef().train()
    tr = UnsupervisedTrainer(net, torch.device("cuda", 0), **kw)
    tr.model.discriminator.load_state_dict(dref.state_dict())
    tr.model.train()
    return ref, dref, tr


def test_finetune_step_against_the_oracle(D):
    from _parity import check
    from oracle.losses_ref import FineTuningLossRef
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    lr, epoch = 1e-4, 3
    kw = dict(consistency_weight=1.0, domain_weight=0.1, supervised_weight=0.1, rampup_length=3)
    ref, dref, tr = _trainer_pair(**kw)
    n, h, w = 2, 64, 64
    imgs, _ = D.synthetic_u8_batch(n, h, w, seed=8)
    g = torch.Generator().manual_seed(4)
    params = (D.draw_strong_params(n, h, w, g), D.draw_strong_params(n, h, w, g))
    v1, v2 = D.strong_views(imgs, *params)                                     # the kernel's own views feed the restatement
    plain, _ = D.prepare_batch(imgs)
    v1, v2, plain = v1.float().cpu().contiguous(), v2.float().cpu().contiguous(), plain.float().cpu().contiguous()

    ref_params = list(ref.parameters()) + list(dref.parameters())
    names = ["segmentation_model." + k for k, _ in ref.named_parameters()] + ["discriminator." + k for k, _ in dref.named_parameters()]
    opt_ref = torch.optim.Adam(ref_params, lr=lr)
    p1, p2 = ref(v1), ref(v2)                                                  # two training-mode forwards
    want = FineTuningLossRef(**kw)(p1, p2, dref(plain), epoch)
    opt_ref.zero_grad()
    want["total"].backward()
    norm_ref = torch.nn.utils.clip_grad_norm_(ref_params, 1.0)
    before = [p.detach().clone() for p in ref_params]

    model = tr.model
    opt = FusedAdam(model.parameters(), lr=lr)
    got = tr.finetune_step(imgs, opt, epoch, params=params)
    assert not got["skipped"] and opt.flat_launches == 2, "FusedAdam did not take one flat pass per network"
    for k in ("total", "consistency", "domain_confusion"):
        a, b = float(got[k].detach()), float(want[k].detach())
        print(f"finetune_step {k}: {a:.9g} (oracle {b:.9g}) relative {abs(a - b) / abs(b):.2e}")
    for k in ("total", "consistency", "domain_confusion"):
        assert abs(float(got[k].detach()) - float(want[k].detach())) <= 1e-5 * abs(float(want[k].detach())), k
    assert float(got["supervised"]) == 0.0 and float(got["rampup_weight"]) == 1.0
    assert abs(float(tr.last_grad_norm) - float(norm_ref)) <= 1e-3 * float(norm_ref)
    # BatchNorm running statistics: the segmenter's moved twice, the discriminator's once
    sd = model.state_dict()
    sdr = {**{"segmentation_model." + k: v for k, v in ref.state_dict().items()},
           **{"discriminator." + k: v for k, v in dref.state_dict().items()}}
    assert list(sd) == list(sdr)
    for k in sdr:
        if "running" in k:
            check(sd[k], sdr[k], k, 1e-4)
        if "num_batches" in k:
            assert int(sd[k]) == int(sdr[k]) == (2 if k.startswith("segmentation_model.") else 1), k
    # the Adam update, on entries whose (clipped) gradient agrees with the oracle's and is far above the noise
    gpu_grads = [p.grad.detach().cpu().clone() for p in model.parameters()]
    opt_ref.step()
    compared = 0
    for k, p, pr, b4, gg in zip(names, model.parameters(), ref_params, before, gpu_grads):
        gr = pr.grad
        sel = (gr.abs() > 0.05 * gr.abs().max()) & ((gr - gg).abs() <= 1e-3 * gr.abs())
        if not sel.any():
            continue
        compared += 1
        upd = (p.detach().cpu() - b4)[sel]
        upd_ref = (pr.detach() - b4)[sel]
        assert (upd - upd_ref).abs().max() <= 0.01 * lr, k
    assert compared >= len(names) // 2, compared


def test_nonfinite_total_skips_the_step(D):
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    _, _, tr = _trainer_pair(consistency_weight=float("inf"), rampup_length=1)
    model = tr.model
    opt = FusedAdam(model.parameters(), lr=1e-3)
    imgs, _ = D.synthetic_u8_batch(2, 64, 64, seed=9)
    # one regular step first, so that moments and step counters exist
    tr.fine_tuning_loss.consistency_weight = 1.0
    assert not tr.finetune_step(imgs, opt, 1, params=None)["skipped"]
    tr.fine_tuning_loss.consistency_weight = float("inf")
    ps = [p.detach().clone() for p in model.parameters()]
    state = opt.state_dict()["state"]
    out = tr.finetune_step(imgs, opt, 1)
    assert out["skipped"] and tr.skipped == 1 and not math.isfinite(tr.last_losses["total"])
    assert all(torch.equal(a, b.detach()) for a, b in zip(ps, model.parameters()))
    after = opt.state_dict()["state"]
    assert list(state) == list(after)
    for k in state:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(state[k][name]), torch.as_tensor(after[k][name])), (k, name)


# ------------------------------------------------------------------------------------------------ the flagship shape
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ten_iterations_reduce_the_consistency_loss(D, dtype):
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    from uda_aerial_semantic_segmentation_research_amd.unsupervised_trainer import UnsupervisedTrainer
    torch.manual_seed(0)
    n, h, w = 8, 512, 512
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23, compute_dtype=dtype)
    tr = UnsupervisedTrainer(net, torch.device("cuda", 0), rampup_length=1, log_interval=1)
    imgs, _ = D.synthetic_u8_batch(n, h, w, seed=12)
    g = torch.Generator().manual_seed(13)
    params = (D.draw_strong_params(n, h, w, g), D.draw_strong_params(n, h, w, g))
    opt = FusedAdam(tr.model.parameters(), lr=1e-4)
    mean_loss, metrics = tr.train_epoch([imgs] * 10, opt, 1, params=params)
    series = {k: [v for _, v in tr.logger.scalars[f"train/loss_{k}"]] for k in ("total", "consistency", "domain_confusion")}
    print(f"{dtype}: consistency {series['consistency'][0]:.5f} -> {series['consistency'][-1]:.5f}, grad norm {float(tr.last_grad_norm):.4f}")
    assert tr.skipped == 0 and all(len(v) == 10 and all(math.isfinite(x) for x in v) for v in series.values())
    assert math.isfinite(mean_loss) and set(metrics) == {"source_domain_acc", "target_domain_acc", "domain_confusion"}
    assert series["consistency"][-1] < series["consistency"][0]
    assert opt.flat_launches == 2 and all(torch.isfinite(p).all() for p in tr.model.parameters())
