"""The stem's weight gradient with its BatchNorm backward in the staging (csrc/conv_stem_wgrad.hip, conv_small_ci_wgrad_kernel) against
the two launches it replaces: bn_bwd_apply (which wrote dy) followed by conv2d_wgrad.  All shapes are 7x7 / stride 2 / pad 3, 3 -> 4
physical channels in, 64 out.

Shapes (n x input h x w): 1x16x16 (8x8 outputs: every tile a border tile), 2x22x38 (11x19 outputs, ragged both ways), 3x64x96 with the
block count capped at 5 (24 slabs: every block takes more than one trip through the persistent loop), 1x64x64 accumulated onto a
non-zero dW and, with accumulate_param, onto non-zero dgamma / dbeta; ReLU and a leaky slope.

Tier A, against float64: the reference restates BatchNorm backward and the 7x7 weight gradient in float64 from the same fp32 inputs and
the same fp32 means of the same f64 sums (bn_bwd_reduce's).  e = the kernel's deviation, d = the existing path's on the same inputs, both
max |got - ref| / max |ref|; bar max(4 d, 2^-22), the project's standing rule.  The inputs exercise the mask: channels 0..7 have mean 0
and beta 0, hence shift exactly 0, and there y holds exact zeros (fma(y, scale, shift) == 0) and +-1e-30; elsewhere a tenth of the y sit
a relative 2^-10 either side of the zero crossing -shift / scale; a tenth of the dz are exactly 0.
Tier B, bit for bit: mean 0, rstd 1, gamma 1, beta 0, zero sums, so dy = dz * mask exactly; small-integer x and dz (|v| <= 3, at most
4608 products of at most 9 per element: exact in fp32 in any order); the result must torch.equal the old path's.
In every case of both tiers dgamma and dbeta must torch.equal bn_bwd_apply's and dW's fourth-channel entries must be what they were.
Network level: one r18 fp32 step at 2x64x64 with the route on and off.

Set UDASEG_DEVIATION_LOG to a file name to collect the figures (profiles/stem_wgrad_grade.txt).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
PREFIX = "stem_wgrad_grade |"
FLOOR = 2.0 ** -22
#         id             n  h   w   blocks accumulate
SHAPES = {"1x16x16": (1, 16, 16, 0, False), "2x22x38": (2, 22, 38, 0, False), "3x64x96_capped": (3, 64, 96, 5, False),
          "1x64x64_accumulate": (1, 64, 64, 0, True)}


def _log(line):
    print(line)
    path = os.environ.get("UDASEG_DEVIATION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def K():
    from uda_aerial_semantic_segmentation_research_amd import _lib, kernels
    _lib.require_gpu()
    kernels.ensure_workspace(torch.device("cuda", 0))
    kernels.set_option("STEM_WGRAD_BN", 1)           # the route under test, whatever default the environment supplies
    yield kernels
    kernels.set_option("STEM_WGRAD_BN", -1)
    kernels.stem_wgrad_set_blocks(0)


def both_paths(K, d, o, act, slope, blocks, accumulate, base):
    """(dW, dgamma, dbeta) of the fused launch and of bn_bwd_apply + conv2d_wgrad (the option off), from the same operands and the
    same starting contents of dW / dgamma / dbeta."""
    dev = {k: v.cuda() for k, v in o.items()}
    args = (dev["mean"], dev["rstd"], dev["gamma"])
    new, old = [(base["dw"].clone().cuda(), base["dg"].clone().cuda(), base["db"].clone().cuda()) for _ in range(2)]
    assert K.conv_stem_wgrad_bn_ok(d)
    K.stem_wgrad_set_blocks(blocks)
    try:
        K.conv2d_wgrad_stem_bn(d, dev["x"], dev["dz"], dev["y"], *args, dev["beta"], dev["bsums"], act, slope, *new, accumulate, accumulate)
    finally:
        K.stem_wgrad_set_blocks(0)
    K.set_option("STEM_WGRAD_BN", 0)
    try:
        assert not K.conv_stem_wgrad_bn_ok(d)
        dy = torch.empty_like(dev["dz"])
        K.bn_bwd_apply(dev["dz"], None, dev["y"], *args, dev["bsums"], dy, None, old[1], old[2], act, slope, False, False, accumulate,
                       beta=dev["beta"])
        K.conv2d_wgrad(d, dev["x"], dy, old[0], accumulate)
    finally:
        K.set_option("STEM_WGRAD_BN", 1)
    torch.cuda.synchronize()
    return [t.cpu() for t in new], [t.cpu() for t in old]


def start_contents(g, accumulate, integers=False):
    """dW / dgamma / dbeta before the call: non-zero everywhere when the call accumulates (the padded lanes included), else a marker."""
    if accumulate:
        draw = (lambda *s: torch.randint(-3, 4, s, generator=g).float()) if integers else (lambda *s: torch.randn(*s, generator=g))
        return {"dw": draw(64, 7, 7, 4), "dg": draw(64), "db": draw(64)}
    return {"dw": torch.full((64, 7, 7, 4), 7.0), "dg": torch.full((64,), 7.0), "db": torch.full((64,), 7.0)}


def ref_wgrad(x, dy64):
    """[64][7][7][3] float64 from the NHWC operands."""
    x64 = x[..., :3].permute(0, 3, 1, 2).double()
    return torch.nn.grad.conv2d_weight(x64, (64, 3, 7, 7), dy64.permute(0, 3, 1, 2), stride=2, padding=3).permute(0, 2, 3, 1).contiguous()


def tier_a_operands(K, n, h, w, slope, seed):
    g = torch.Generator().manual_seed(seed)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = torch.randn(n, h, w, 4, generator=g)
    x[..., 3] = 0.0
    y = torch.randn(n, ho, wo, 64, generator=g) * 1.5 + torch.randn(64, generator=g) * 0.5
    mean = y.reshape(-1, 64).mean(0)
    rstd = 1.0 / torch.sqrt(y.reshape(-1, 64).var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(64, generator=g) + 0.5
    beta = torch.randn(64, generator=g) * 0.3
    mean[:8], beta[:8] = 0.0, 0.0                                   # shift == 0 exactly on these channels
    scale = gamma * rstd                                            # fp32, as the kernels form it
    shift64 = beta.double() - mean.double() * scale.double()
    pick = torch.rand(n, ho, wo, 64, generator=g)
    cross = (-shift64 / scale.double()).expand_as(y)                # the zero crossing of the activation's argument
    y = torch.where(pick < 0.05, (cross * (1 + 2.0 ** -10)).float(), y)
    y = torch.where((pick >= 0.05) & (pick < 0.10), (cross * (1 - 2.0 ** -10)).float(), y)
    tiny = torch.where(pick < 0.03, 0.0, torch.where(pick < 0.06, 1e-30, -1e-30))
    y[..., :8] = torch.where(pick[..., :8] < 0.10, tiny[..., :8].float(), y[..., :8])
    dz = torch.randn(n, ho, wo, 64, generator=g)
    dz = torch.where(torch.rand(n, ho, wo, 64, generator=g) < 0.1, torch.zeros(()), dz)
    o = {"x": x, "y": y.contiguous(), "dz": dz.contiguous(), "mean": mean, "rstd": rstd, "gamma": gamma, "beta": beta}
    bsums = torch.zeros(2 * 64 * K.bn_replicas(), dtype=f64, device="cuda")
    K.bn_bwd_reduce(o["dz"].cuda(), None, o["y"].cuda(), mean.cuda(), rstd.cuda(), bsums, 1, slope, gamma=gamma.cuda(), beta=beta.cuda())
    torch.cuda.synchronize()
    o["bsums"] = bsums.cpu()
    # float64 restatement: the mask from the argument in float64, the two means cast to fp32 as the kernels cast them
    arg = y.double() * scale.double() + shift64
    s = o["bsums"].reshape(-1, 2, 64).sum(0)
    pixels = n * ho * wo
    mg, mgx = (s[0] / pixels).float().double(), (s[1] / pixels).float().double()
    gz = dz.double() * torch.where(arg > 0, 1.0, float(torch.tensor(slope, dtype=f32)))
    xh = (y.double() - mean.double()) * rstd.double()
    dy64 = scale.double() * (gz - mg - xh * mgx)
    exact0 = int((arg == 0).sum())
    assert exact0 > 0 and int((dz == 0).sum()) > 0
    return o, ref_wgrad(x, dy64), exact0


def dev_of(got, ref64):
    assert torch.isfinite(got).all()
    return ((got.double() - ref64).abs().max() / ref64.abs().max()).item()


@pytest.mark.parametrize("slope", [0.0, 0.2], ids=["relu", "leaky"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tier_a_against_float64(K, shape, slope):
    n, h, w, blocks, accumulate = SHAPES[shape]
    d = K.conv_desc(n, h, w, 4, 64, 7, 2, 3)
    o, ref, exact0 = tier_a_operands(K, n, h, w, slope, seed=n * 1000 + h + w)
    base = start_contents(torch.Generator().manual_seed(5), accumulate)
    (dw, dg, db), (dw_old, dg_old, db_old) = both_paths(K, d, o, 1, slope, blocks, accumulate, base)
    if accumulate:
        ref = ref + base["dw"][..., :3].double()
    e, dd = dev_of(dw[..., :3], ref), dev_of(dw_old[..., :3], ref)
    bar = max(4.0 * dd, FLOOR)
    _log(f"{PREFIX} tier A | {shape} {'leaky' if slope else 'relu'} | e {e:.3e} d {dd:.3e} e/bar {e / bar:.3f} | arguments exactly 0: {exact0}")
    assert torch.equal(dg, dg_old) and torch.equal(db, db_old), "dgamma / dbeta differ from bn_bwd_apply's"
    assert torch.equal(dw[..., 3], base["dw"][..., 3]), "the fourth-channel entries of dW were written"
    assert e <= bar, f"{shape}: e {e:.3e} > max(4 d, 2^-22) = {bar:.3e} (d {dd:.3e})"


@pytest.mark.parametrize("slope", [0.0, 0.25], ids=["relu", "leaky"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tier_b_bit_for_bit(K, shape, slope):
    n, h, w, blocks, accumulate = SHAPES[shape]
    d = K.conv_desc(n, h, w, 4, 64, 7, 2, 3)
    g = torch.Generator().manual_seed(n * 100 + h)
    ho, wo = d.ho, d.wo
    x = torch.randint(-3, 4, (n, h, w, 4), generator=g).float()
    x[..., 3] = 0.0
    y = torch.randn(n, ho, wo, 64, generator=g)
    y = torch.where(torch.rand(n, ho, wo, 64, generator=g) < 0.1, torch.zeros(()), y)
    dz = torch.randint(-3, 4, (n, ho, wo, 64), generator=g).float()
    o = {"x": x, "y": y, "dz": dz, "mean": torch.zeros(64), "rstd": torch.ones(64), "gamma": torch.ones(64), "beta": torch.zeros(64),
         "bsums": torch.zeros(2 * 64 * K.bn_replicas(), dtype=f64)}
    base = start_contents(g, accumulate, integers=True)
    (dw, dg, db), (dw_old, dg_old, db_old) = both_paths(K, d, o, 1, slope, blocks, accumulate, base)
    want = ref_wgrad(x, dz.double() * torch.where(y > 0, 1.0, slope))
    if accumulate:
        want = want + base["dw"][..., :3].double()
    _log(f"{PREFIX} tier B | {shape} {'leaky' if slope else 'relu'} | differing elements vs the old path {int((dw[..., :3] != dw_old[..., :3]).sum())}"
         f" vs the exact sums {int((dw[..., :3].double() != want).sum())}")
    assert torch.equal(dw[..., :3], dw_old[..., :3]), "not the old path's gradient, bit for bit"
    assert torch.equal(dw[..., :3].double(), want), "not the exact integer sums"
    assert torch.equal(dg, dg_old) and torch.equal(db, db_old), "dgamma / dbeta differ from bn_bwd_apply's"
    assert torch.equal(dw[..., 3], base["dw"][..., 3]), "the fourth-channel entries of dW were written"


def test_query_refuses_other_layers(K):
    ok = K.conv_stem_wgrad_bn_ok
    assert ok(K.conv_desc(2, 64, 64, 4, 64, 7, 2, 3))
    for d in (K.conv_desc(2, 64, 64, 8, 64, 7, 2, 3), K.conv_desc(2, 64, 64, 4, 32, 7, 2, 3), K.conv_desc(2, 64, 64, 4, 64, 3, 1, 1),
              K.conv_desc(2, 64, 64, 4, 64, 7, 1, 3), K.conv_desc(2, 64, 64, 4, 64, 7, 2, 2)):
        assert not ok(d)
    with pytest.raises(RuntimeError, match="ReLU / leaky"):
        z = torch.zeros(2 * 32 * 32 * 64, device="cuda")
        v = torch.zeros(64, device="cuda")
        K.conv2d_wgrad_stem_bn(K.conv_desc(2, 64, 64, 4, 64, 7, 2, 3), torch.zeros(2 * 64 * 64 * 4, device="cuda"), z, z, v, v, v, v,
                               torch.zeros(2 * 64 * K.bn_replicas(), dtype=f64, device="cuda"), 0, 0.0,
                               torch.zeros(64 * 49 * 4, device="cuda"), v.clone(), v.clone())


def test_r18_step_takes_the_route(K, monkeypatch):
    """One r18 fp32 step at 2x64x64, route on against route off: conv1's weight gradient within 4 x the difference of two runs with the
    route OFF (the weight gradients add with fp32 atomics: the old path's own run-to-run spread is the yardstick), loss and logits bit
    for bit (the forward is untouched), and the launches counted: the fused launch once and one bn_bwd_apply fewer.

    Measured (profiles/stem_wgrad_grade.txt): on vs off 4.47e-8 against off vs off 1.49e-8 and 2.98e-8 in two runs, i.e. 3 ulp of the
    largest element (0.1485) against 1 and 2: at this shape the bar is quantised to single ulps."""
    from _parity import pair
    from oracle.adversarial_ref import synthetic_batch
    from uda_aerial_semantic_segmentation_research_amd import engine
    from uda_aerial_semantic_segmentation_research_amd.losses import CrossEntropyLoss
    calls = {}
    for name in ("conv2d_wgrad_stem_bn", "bn_bwd_apply", "conv2d_wgrad"):
        def counted(*a, _f=getattr(engine.K, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(engine.K, name, counted)
    x, y, _ = synthetic_batch(2, 64, 64, seed=0)

    def run(on):
        K.set_option("STEM_WGRAD_BN", 1 if on else 0)
        try:
            calls.clear()
            _, net = pair("resnet18")
            out = net(x.cuda())
            loss = CrossEntropyLoss()(out, y.cuda())
            loss.backward()
            torch.cuda.synchronize()
            return loss.detach().cpu(), out.detach().cpu(), net.encoder.conv1.weight.grad.detach().cpu().clone(), dict(calls)
        finally:
            K.set_option("STEM_WGRAD_BN", 1)

    off1, off2, on = run(False), run(False), run(True)
    assert off1[3].get("conv2d_wgrad_stem_bn", 0) == 0
    assert on[3].get("conv2d_wgrad_stem_bn", 0) == 1, on[3]
    assert on[3]["bn_bwd_apply"] == off1[3]["bn_bwd_apply"] - 1 and on[3].get("conv2d_wgrad", 0) == off1[3].get("conv2d_wgrad", 0) - 1
    assert torch.equal(on[0], off1[0]) and torch.equal(on[1], off1[1]), "loss / logits changed"
    spread = (off1[2] - off2[2]).abs().max().item()
    diff = (on[2] - off1[2]).abs().max().item()
    scale = off1[2].abs().max().item()
    _log(f"{PREFIX} r18 2x64x64 step | conv1.weight.grad: route on vs off {diff:.3e}, off vs off {spread:.3e}, largest element {scale:.3e}"
         f" | l2: {(on[2] - off1[2]).norm().item():.3e} / {(off1[2] - off2[2]).norm().item():.3e}")
    assert diff <= 4.0 * spread, f"on vs off {diff:.3e} > 4 x the old path's run-to-run spread {spread:.3e}"
