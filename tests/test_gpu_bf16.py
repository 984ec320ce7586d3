"""GPU parity of the bf16 storage path (BASELINE configs 3 / 5): bf16 activations and weights, fp32 accumulation.

Reference = the same op in fp32 on CPU applied to the bf16-ROUNDED inputs (so only accumulation order and the final rounding
of the output to bf16 differ).  Tolerance: 2^-7 relative to the tensor's largest magnitude (``BF_TOL``: one bf16 spacing at the
bottom of the largest value's binade), norm-wise.  The element-wise float64 bar of the same kernels is
tests/test_gpu_conv_bf16_grade.py.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF_TOL = 2.0 ** -7


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    return kernels


def rb(t):
    """round to bf16 and back (what the device tensors hold)"""
    return t.to(torch.bfloat16).to(torch.float32)


def nhwc_bf(t):
    return t.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)


def nchw32(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).contiguous()


def close(got, ref, what, tol=BF_TOL):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    e = ((got.double() - ref.double()).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.3e}"


BF_CASES = [
    (2, 16, 16, 64, 64, 3, 1, 1), (2, 16, 16, 64, 128, 3, 2, 1), (2, 16, 16, 64, 128, 1, 2, 0), (1, 8, 8, 256, 256, 3, 1, 1),
    (2, 32, 32, 8, 64, 7, 2, 3), (2, 32, 32, 8, 64, 4, 2, 1), (1, 24, 24, 32, 16, 3, 1, 1), (1, 24, 24, 16, 24, 3, 1, 1),
    (1, 12, 20, 192, 64, 3, 1, 1), (3, 9, 7, 8, 40, 3, 1, 1), (8, 64, 64, 64, 64, 3, 1, 1),
    # pixel folding (csrc/conv_igemm.hip fold_plan): 16 / 32 gathered channels, forward and data gradient, width a multiple of
    # the fold or not (fallback to the generic loop), the head's 24 outputs, a full-size decoder-tail shape
    (2, 32, 32, 32, 32, 3, 1, 1), (2, 16, 64, 16, 16, 3, 1, 1), (1, 10, 14, 16, 24, 3, 1, 1), (1, 10, 14, 32, 16, 3, 1, 1),
    (2, 20, 36, 16, 32, 3, 1, 1), (4, 128, 128, 32, 16, 3, 1, 1),
    # 1x1 / stride 1: the weight gradient treats the batch as one row of M pixels (row-uniform gather at any image width)
    (2, 24, 24, 64, 256, 1, 1, 0), (1, 7, 9, 64, 128, 1, 1, 0), (3, 48, 48, 256, 64, 1, 1, 0),
]


@pytest.mark.parametrize("case", BF_CASES, ids=[("n%d_%dx%d_ci%d_co%d_k%d_s%d_p%d" % c) for c in BF_CASES])
def test_conv_bf16_fwd_dgrad(K, case):
    n, h, w, ci, co, k, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = rb(torch.randn(n, ci, h, w, generator=g))
    wt = rb(torch.randn(co, ci, k, k, generator=g) / math.sqrt(ci * k * k))
    bias = torch.randn(co, generator=g)
    xr = x.clone().requires_grad_(True)
    y_ref = F.conv2d(xr, wt, bias, stride=s, padding=p)
    dy = rb(torch.randn(y_ref.shape, generator=g))
    y_ref.backward(dy)
    d = K.conv_desc(n, h, w, ci, co, k, s, p)
    xd = nhwc_bf(x)
    wd = wt.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)
    y = torch.empty((n, d.ho, d.wo, co), device="cuda", dtype=torch.bfloat16)
    R = K.bn_replicas()
    st = torch.zeros(R * 2 * co, dtype=torch.float64, device="cuda")
    K.conv2d_fwd_bf16(d, xd, wd, bias.cuda(), None, y, stats=st)
    close(nchw32(y), y_ref.detach(), "bf16 fwd")
    tot = st.view(R, 2, co).sum(0).cpu()
    yd = y_ref.detach().double().permute(0, 2, 3, 1).reshape(-1, co)
    assert (tot[0] - yd.sum(0)).abs().max().item() <= 1e-4 * yd.abs().sum(0).max().item(), "bf16 fused sum"
    close(tot[1], (yd * yd).sum(0), "bf16 fused sum of squares", 1e-3)
    # fp32 output + leaky + residual variants
    y32 = torch.empty((n, d.ho, d.wo, co), device="cuda", dtype=torch.float32)
    K.conv2d_fwd_bf16(d, xd, wd, bias.cuda(), None, y32, act=1, slope=0.2)
    close(nchw32(y32), F.leaky_relu(y_ref.detach(), 0.2), "bf16 fwd -> fp32 out", 1e-4)
    res = rb(torch.randn(y_ref.shape, generator=g))
    y3 = torch.empty_like(y)
    K.conv2d_fwd_bf16(d, xd, wd, None, nhwc_bf(res), y3, act=1, slope=0.0)
    close(nchw32(y3), F.relu(y_ref.detach() - bias.view(1, -1, 1, 1) + res), "bf16 fwd + residual + relu")
    # dgrad
    wtp = wt.permute(1, 2, 3, 0).contiguous().to("cuda", torch.bfloat16)        # [ci][kh][kw][co]
    dx = torch.empty((n, h, w, ci), device="cuda", dtype=torch.bfloat16)
    K.conv2d_dgrad_bf16(d, nhwc_bf(dy), wtp, dx)
    close(nchw32(dx), xr.grad, "bf16 dgrad")
    # wgrad: fp32 master gradient from bf16 operands (ds_read_b64_tr_b16 fragments)
    wr = wt.clone().requires_grad_(True)
    F.conv2d(x, wr, None, stride=s, padding=p).backward(dy)
    dw = torch.full((co, k, k, ci), float("nan"), device="cuda")
    K.conv2d_wgrad_bf16(d, xd, nhwc_bf(dy), dw)
    close(dw.cpu().permute(0, 3, 1, 2), wr.grad, "bf16 wgrad", 1e-4)
    dw2 = torch.full((co, k, k, ci), 0.25, device="cuda")
    K.conv2d_wgrad_bf16(d, xd, nhwc_bf(dy), dw2, accumulate=True)
    close(dw2.cpu().permute(0, 3, 1, 2), wr.grad + 0.25, "bf16 wgrad + acc", 1e-4)
    dx2 = torch.full((n, h, w, ci), 0.5, device="cuda", dtype=torch.bfloat16)
    K.conv2d_dgrad_bf16(d, nhwc_bf(dy), wtp, dx2, accumulate=True)
    close(nchw32(dx2), xr.grad + 0.5, "bf16 dgrad + acc")


def bf(t):  # NCHW cpu fp32 -> NHWC cuda bf16
    return t.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)


@pytest.mark.parametrize("n,h,w,c1,c2,act,slope", [(8, 64, 64, 64, 64, 1, 0.0), (2, 32, 32, 256, 128, 1, 0.0),
                                                    (3, 9, 7, 40, 64, 1, 0.2), (1, 16, 16, 512, 512, 1, 0.0),
                                                    (2, 24, 24, 16, 24, 1, 0.0), (2, 32, 32, 32, 16, 1, 0.0),
                                                    (2, 16, 64, 16, 32, 1, 0.2)])
def test_dgrad_with_bn_backward_reductions_bf16(K, n, h, w, c1, c2, act, slope):
    """udaseg_conv2d_dgrad_bnreduce_bf16 == udaseg_conv2d_dgrad_bf16 followed by udaseg_bn_bwd_reduce_bf16 on what it stored
    (dz = the bf16 dx, z = the bf16 activation the forward wrote): dx bit for bit, the two per-channel sums to fp32
    block-partial rounding.  Ragged tiles, a channel tail and the <= 32-channel generic loop included (the reductions are made
    in the LDS-staged epilogue, which guards rows and chunks itself)."""
    g = torch.Generator().manual_seed(c1 + c2 + h)
    d = K.conv_desc(n, h, w, c1, c2, 3, 1, 1)
    assert K.conv2d_dgrad_bnreduce_ok(d, torch.bfloat16)
    assert not K.conv2d_dgrad_bnreduce_ok(K.conv_desc(n, h, w, c1, c2, 3, 2, 1), torch.bfloat16)
    bf = torch.bfloat16
    dy = torch.randn(n, h, w, c2, generator=g).to(bf).cuda()
    wt = (torch.randn(c1, 3, 3, c2, generator=g) / math.sqrt(9 * c2)).to(bf).cuda()          # already [ci][taps][co]
    prev_y = torch.randn(n, h, w, c1, generator=g).to(bf).cuda()
    mean, rstd = torch.randn(c1, generator=g).cuda() * 0.1, (torch.rand(c1, generator=g) + 0.5).cuda()
    gamma, beta = (torch.rand(c1, generator=g) + 0.5).cuda(), (torch.randn(c1, generator=g) * 0.3).cuda()
    # the activation the forward stored: act(bn(y)) rounded to bf16 (what the stand-alone reduction reads as z)
    t = prev_y.float() * (gamma * rstd) + (beta - mean * (gamma * rstd))
    z = torch.where(t > 0, t, slope * t).to(bf)
    R = K.bn_replicas()
    dx_ref = torch.empty(n, h, w, c1, device="cuda", dtype=bf)
    K.conv2d_dgrad(d, dy, wt, dx_ref)
    bs_ref = torch.zeros(R * 2 * c1, dtype=torch.float64, device="cuda")
    K.bn_bwd_reduce(dx_ref, z, prev_y, mean, rstd, bs_ref, act, slope)
    dx = torch.full_like(dx_ref, float("nan"))
    bs = torch.zeros_like(bs_ref)
    K.conv2d_dgrad_bnreduce(d, dy, wt, dx, prev_y, mean, rstd, gamma, beta, act, slope, bs)
    assert torch.equal(dx, dx_ref)
    s, s_ref = bs.view(R, 2, c1).sum(0), bs_ref.view(R, 2, c1).sum(0)
    scale = s_ref.abs().max(dim=1, keepdim=True).values
    # a sign flip of one near-zero pre-activation (fma vs the rounded z) would show as ~1e-4 of a channel sum; none expected
    assert ((s - s_ref).abs() / scale).max().item() < 2e-5, ((s - s_ref).abs() / scale).max().item()
    gm = dx_ref.float() * torch.where(t > 0, 1.0, slope)
    want = torch.stack([gm.double().sum((0, 1, 2)), (gm.double() * ((prev_y.float() - mean) * rstd).double()).sum((0, 1, 2))])
    assert ((s - want).abs() / want.abs().max(dim=1, keepdim=True).values).max().item() < 1e-4


BN_SMALL = [(c, *v, None) for c in (16, 64, 512) for v in ((0, 0.0, False), (1, 0.0, True), (1, 0.2, False))]
BN_FULL = [(16, 1, 0.0, False, (8, 512, 512)), (16, 1, 0.0, True, (8, 512, 512))]


@pytest.mark.parametrize("c,act,slope,with_res,nhw", BN_SMALL + BN_FULL,
                         ids=[f"c{c}_act{a}_{sl}_{'res' if r else 'nores'}_{'full' if s else 'small'}" for c, a, sl, r, s in BN_SMALL + BN_FULL])
def test_bn_bf16_fwd_bwd(K, c, act, slope, with_res, nhw):
    """The `full` cases run at 8 x 512 x 512 x 16 = 2 097 152 pixels x 16 channels, the first shape of tools/bn_bandwidth.py
    (the launch that faulted in round 2, profiles/r02_bn_bandwidth.txt): grid-stride loops with four loads in flight, the
    block-count caps and the tail iterations at a size the small cases never reach."""
    n, h, w = nhw or ((2, 6, 10) if c > 64 else (4, 24, 20))
    g = torch.Generator().manual_seed(c + act)
    x = rb(torch.randn(n, c, h, w, generator=g) * 2 + 0.5).requires_grad_(True)
    res = rb(torch.randn(n, c, h, w, generator=g)).requires_grad_(True) if with_res else None
    bn = torch.nn.BatchNorm2d(c).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    u = bn(x)
    if with_res:
        u = u + res
    z_ref = F.leaky_relu(u, slope) if act else u
    dz = rb(torch.randn(z_ref.shape, generator=g))
    z_ref.backward(dz)
    yd = bf(x.detach())
    R = K.bn_replicas()
    sums = torch.zeros(2 * c * R, dtype=torch.float64, device="cuda")
    xs = x.detach().double().permute(0, 2, 3, 1).reshape(-1, c)
    sums[:c] = xs.sum(0).cuda()                     # statistics normally come from the conv epilogue (fp32 accumulators)
    sums[c:2 * c] = (xs * xs).sum(0).cuda()
    z = torch.empty_like(yd)
    rm, rv = rm0.cuda(), rv0.cuda()
    sm, sr = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    gam, bet = bn.weight.detach().cuda(), bn.bias.detach().cuda()
    resd = bf(res.detach()) if with_res else None
    K.bn_apply(yd, sums, gam, bet, resd, z, bn.eps, bn.momentum, rm, rv, sm, sr, act, slope)
    close(nchw32(z), z_ref.detach(), "bn bf16 fwd")
    close(rm.cpu(), bn.running_mean, "running_mean", 1e-5)
    close(rv.cpu(), bn.running_var, "running_var", 1e-5)
    bs = torch.zeros(2 * c * R, dtype=torch.float64, device="cuda")
    K.bn_bwd_reduce(bf(dz), z, yd, sm, sr, bs, act, slope)
    dy = torch.empty_like(yd)
    dres = torch.empty_like(yd) if with_res else None
    dg, db = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    K.bn_bwd_apply(bf(dz), z, yd, sm, sr, gam, bs, dy, dres, dg, db, act, slope)
    # masks come from the bf16-rounded z: a handful of near-zero pre-activations can flip -> compare norm-wise, loosely
    close(nchw32(dy), x.grad, "bn bf16 dx", 4 * BF_TOL)
    close(dg.cpu(), bn.weight.grad, "bn bf16 dgamma", 4 * BF_TOL)
    close(db.cpu(), bn.bias.grad, "bn bf16 dbeta", 4 * BF_TOL)
    if with_res:
        close(nchw32(dres), res.grad, "bn bf16 dres", 4 * BF_TOL)


def test_pool_resize_layout_bf16(K):
    g = torch.Generator().manual_seed(1)
    x = rb(torch.relu(torch.randn(2, 64, 16, 12, generator=g))).requires_grad_(True)
    y_ref = F.max_pool2d(x, 3, 2, 1)
    dy = rb(torch.randn(y_ref.shape, generator=g))
    y_ref.backward(dy)
    y, idx = K.maxpool_fwd(bf(x.detach()))
    assert y.dtype == torch.bfloat16 and torch.equal(nchw32(y), y_ref.detach())
    dx = torch.empty((2, 16, 12, 64), device="cuda", dtype=torch.bfloat16)
    K.maxpool_bwd(bf(dy), idx, dx)
    close(nchw32(dx), x.grad, "maxpool bf16 bwd")
    a = rb(torch.randn(2, 32, 5, 6, generator=g)).requires_grad_(True)
    s = rb(torch.randn(2, 16, 10, 12, generator=g)).requires_grad_(True)
    ref = torch.cat([F.interpolate(a, scale_factor=2.0, mode="nearest"), s], dim=1)
    dout = rb(torch.randn(ref.shape, generator=g))
    ref.backward(dout)
    out = K.upsample2x_concat_fwd(bf(a.detach()), bf(s.detach()))
    assert torch.equal(nchw32(out), ref.detach())
    da = torch.empty((2, 5, 6, 32), device="cuda", dtype=torch.bfloat16)
    ds = torch.empty((2, 10, 12, 16), device="cuda", dtype=torch.bfloat16)
    K.upsample2x_concat_bwd(bf(dout), da, ds, 32, 16)
    close(nchw32(da), a.grad, "upcat bf16 da")
    assert torch.equal(nchw32(ds), s.grad)
    img = torch.randn(3, 3, 10, 14, generator=g)
    yb = K.nchw_to_nhwc(img.cuda(), dtype=torch.bfloat16)
    assert yb.shape == (3, 10, 14, 8) and torch.equal(yb[..., :3].float().cpu(), rb(img).permute(0, 2, 3, 1))
    assert float(yb[..., 3:].float().abs().max()) == 0.0
    v = torch.randn(4096, generator=g)
    assert torch.equal(K.cast_to_bf16(v.cuda()).cpu(), v.to(torch.bfloat16))


def _net_pair_bf16(name):
    from oracle.unet_ref import UnetRef
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    torch.manual_seed(1234)
    ref = UnetRef(name, classes=23).train()
    net = Unet(encoder_name=name, encoder_weights=None, in_channels=3, classes=23, compute_dtype=torch.bfloat16)
    net.load_state_dict(ref.state_dict())
    return ref, net.to("cuda").train()


@pytest.mark.parametrize("name,size,policy", [("resnet18", 128, "auto"), ("resnet50", 128, "auto"), ("resnet18", 128, "always"),
                                              ("resnet50", 64, "always")])
def test_unet_bf16_vs_fp32_oracle(K, name, size, policy, monkeypatch):
    """bf16 storage / bf16 MFMA against the fp32 CPU oracle.  Stated tolerance ('bf16 configs compared to the
    fp32 CPU result with a stated, looser tolerance'): the logits may be no farther from the fp32 oracle than 1.5x what
    PyTorch's OWN bf16 execution of the same oracle is (measured in the test: 9e-2 for r18, 0.22 for r50 at random init,
    norm-wise -- a 30-60-layer train-mode-BN net amplifies bf16 rounding that much); loss 1e-2; EVERY parameter gradient
    against the fp32 oracle and its bf16-storage emulation under the HIP path's ReLU masks, each tensor within 2x the
    emulation's own distance from the fp32 gradient + 2^-8 (tests/_parity.py::bf16_grads_vs_oracle; round 2 only compared a
    median cosine with PyTorch's bf16 run, which any finite gradient passed for r50)."""
    import copy
    from oracle.adversarial_ref import synthetic_batch
    from uda_aerial_semantic_segmentation_research_amd import engine
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    # "always": every supported layer on the bf16-first kernels (csrc/conv_halo_bf16.hip) -- at these sizes "auto" (the
    # library's speed heuristic) leaves the deep layers on the shared implicit-GEMM source; both routes are held to the same bar
    monkeypatch.setattr(engine, "FRAG_POLICY", policy)
    ref, net = _net_pair_bf16(name)
    x, y, _ = synthetic_batch(2, size, size, seed=0)
    t16 = copy.deepcopy(ref).bfloat16()
    torch_bf16 = t16(x.bfloat16()).float()
    F.cross_entropy(torch_bf16, y).backward()              # PyTorch's own bf16 forward/backward of the oracle, for scale
    torch_bf16 = torch_bf16.detach()
    logits_ref = ref(x)
    loss_ref = F.cross_entropy(logits_ref, y)
    loss_ref.backward()
    e_torch = ((torch_bf16 - logits_ref.detach()).abs().max() / logits_ref.abs().max()).item()
    opt = FusedAdam(net.parameters(), lr=1e-4)
    net.debug_keep_tape = True               # the gradient check below takes the ReLU masks from this forward's activations
    logits = net(x.cuda())
    assert logits.dtype == torch.float32 and logits.shape == logits_ref.shape
    loss = CrossEntropyLoss()(logits, y.cuda())
    loss.backward()
    e = ((logits.detach().cpu() - logits_ref.detach()).abs().max() / logits_ref.abs().max()).item()
    assert e <= 1.5 * e_torch + 1e-2, f"bf16 logits rel err {e:.3e} vs torch-bf16 {e_torch:.3e}"
    assert abs(loss.item() - loss_ref.item()) <= 1e-2 * loss_ref.item()
    # EVERY parameter gradient against an oracle value: the fp32 oracle and its bf16-storage emulation, both with the HIP
    # path's ReLU masks forced in (tests/_parity.py::bf16_grads_vs_oracle states the rule and why it has this form)
    from _parity import bf16_grads_vs_oracle
    bf16_grads_vs_oracle(net, ref, x, lambda out: F.cross_entropy(out, y), f"{name} bf16 2x{size}x{size}")
    print(f"{name} bf16: logits rel err {e:.2e} (torch bf16 on CPU: {e_torch:.2e})")
    net.debug_keep_tape, net._last_tape = False, None
    opt.step()
    losses = []
    for _ in range(8):
        opt.zero_grad()
        l = CrossEntropyLoss()(net(x.cuda()), y.cuda())
        l.backward()
        opt.step()
        losses.append(l.item())
    assert losses[-1] < losses[0], losses
    # eval mode (BatchNorm folded, bf16)
    net.eval()
    ref.eval()
    with torch.no_grad():
        ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
        oe, oref = net(x.cuda()).cpu(), ref(x)
        oref16 = copy.deepcopy(ref).bfloat16()(x.bfloat16()).float()
    e_eval, e_eval_torch = (((t - oref).abs().max() / oref.abs().max()).item() for t in (oe, oref16))
    assert e_eval <= 1.5 * e_eval_torch + 1e-2, (e_eval, e_eval_torch)


def test_adversarial_iteration_bf16(K):
    from uda_aerial_semantic_segmentation_research_amd.adversarial_trainer import AdversarialTrainer
    from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam
    from uda_aerial_semantic_segmentation_research_amd.unet import Unet
    from oracle.adversarial_ref import (AdversarialLossRef, DomainDiscriminatorRef, adversarial_step, synthetic_batch)
    from oracle.unet_ref import UnetRef
    torch.manual_seed(1234)
    ref = UnetRef("resnet18", classes=23).train()
    Dr = DomainDiscriminatorRef(3).train()
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=23, compute_dtype=torch.bfloat16)
    net.load_state_dict(ref.state_dict())
    tr = AdversarialTrainer(net, torch.device("cuda"), lambda_adv=0.001)
    assert tr.discriminator.compute_dtype == torch.bfloat16
    tr.discriminator.load_state_dict(Dr.state_dict())
    src, masks, tgt = synthetic_batch(2, 128, 128, seed=0)
    opt = FusedAdam(net.parameters(), lr=1e-4)
    avg, dm = tr.train_epoch([(src, masks)], [tgt], opt, epoch=1)
    r = adversarial_step(ref, Dr, AdversarialLossRef(0.001), torch.optim.Adam(ref.parameters(), lr=1e-4),
                         torch.optim.Adam(Dr.parameters(), lr=1e-4), src, masks, tgt)
    for k in ("seg_loss", "d_loss", "adv_loss"):
        assert abs(tr.last_losses[k] - r[k].item()) <= 2e-2 * abs(r[k].item()) + 1e-6, (k, tr.last_losses[k], r[k].item())
