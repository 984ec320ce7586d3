"""tests/_norm_ref.py is right: its float64 leg agrees with torch.nn.BatchNorm2d + residual add + leaky_relu under
double-precision autograd and with torch.optim.Adam on float64 parameters to 1e-12 of each output's magnitude.  Runs anywhere;
without it tests/test_gpu_norm_grade.py would hold the kernels to an unproven restatement.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _norm_ref as N

RTOL = 1e-12
SHAPES = [(2, 16), (7, 24), (260, 64)]                       # (pixels, channels): three of the GPU test's shapes
MODES = [(N.NONE, 0.0, False), (N.LEAKY, 0.0, True), (N.LEAKY, 0.2, False), (N.LEAKY, 0.2, True)]


def close(got, ref, mag, what, rtol=RTOL):
    e = N.normalised(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64), mag).max()
    assert e <= rtol, f"{what}: {e:.3e} of the magnitude"


def data(p, c, with_res, seed=0):
    g = np.random.default_rng(seed + 1000 * p + c)
    y = g.standard_normal((p, c)) * 2 + 0.5
    res = g.standard_normal((p, c)) if with_res else None
    return (y, res, g.standard_normal((p, c)), g.random(c) + 0.5, g.standard_normal(c), g.standard_normal(c), g.random(c) + 0.5)


def t4(a, grad=False):        # [P, C] -> torch [P, C, 1, 1] double
    return torch.from_numpy(np.ascontiguousarray(a)).double()[:, :, None, None].requires_grad_(grad)


@pytest.mark.parametrize("p,c", SHAPES)
@pytest.mark.parametrize("act,slope,with_res", MODES)
def test_float64_leg_is_torch_double_autograd(p, c, act, slope, with_res):
    y, res, dz, gamma, beta, rm0, rv0 = data(p, c, with_res)
    bn = torch.nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
    x, r = t4(y, True), (t4(res, True) if with_res else None)
    bn.train()
    u = bn(x)
    u = u + r if with_res else u
    z_t = F.leaky_relu(u, slope) if act else u
    z_t.backward(t4(dz))

    z, _, mag = N.bn_forward(y, gamma, beta, res, bn.eps, act, slope, stat=np.float64)
    close(z, z_t.detach()[:, :, 0, 0].numpy(), mag, "z")
    mean, var, _ = N.stats(y, bn.eps)
    rm, rv, mag_rm, mag_rv = N.running(mean, var, p, bn.momentum, rm0, rv0)
    close(rm, bn.running_mean.numpy(), mag_rm, "running_mean")
    close(rv, bn.running_var.numpy(), mag_rv, "running_var")
    b = N.bn_backward(dz, z, y, gamma, bn.eps, act, slope, stat=np.float64)
    close(b["dy"][0], x.grad[:, :, 0, 0].numpy(), b["dy"][1], "dx")
    close(b["dgamma"][0], bn.weight.grad.numpy(), b["dgamma"][1], "dgamma")
    close(b["dbeta"][0], bn.bias.grad.numpy(), b["dbeta"][1], "dbeta")
    if with_res:
        close(b["dres"][0], r.grad[:, :, 0, 0].numpy(), b["dres"][1], "dres")
    if not with_res:
        g, mag_g = N.act_bwd(dz, z, act, slope)
        close(g, b["dres"][0], mag_g, "act_bwd")
        s, mag_s = N.channel_sum(g)
        close(s, bn.bias.grad.numpy(), mag_s, "channel_sum")
    sc, sh, mag_sc, mag_sh = N.bn_finalize(y, gamma, beta, bn.eps, stat=np.float64)
    plain = F.batch_norm(x.detach(), None, None, bn.weight, bn.bias, True, 0.0, bn.eps)[:, :, 0, 0].detach().numpy()
    close(y * sc + sh, plain, np.abs(y) * mag_sc + mag_sh, "bn_finalize's scale and shift")

    bn.eval()
    with torch.no_grad():
        ze = bn(x.detach())
        ze = ze + r.detach() if with_res else ze
        ze = F.leaky_relu(ze, slope) if act else ze
    got, _, mag_e = N.bn_eval(y, gamma, beta, bn.running_mean.numpy(), bn.running_var.numpy(), res, bn.eps, act, slope)
    close(got, ze[:, :, 0, 0].numpy(), mag_e, "eval-mode z")


def test_one_pixel_takes_the_biased_variance():
    y = np.array([[1.5, -2.0, 0.0, 3.0]])
    mean, var, rstd = N.stats(y, 1e-5)
    assert np.array_equal(mean, y[0]) and not var.any() and np.allclose(rstd, 1e-5 ** -0.5, rtol=1e-15)
    _, rv, _, _ = N.running(mean, var + 2.0, 1, 0.1, np.zeros(4), np.ones(4))
    assert np.allclose(rv, 0.9 + 0.2, rtol=1e-15)                          # factor 1, not 1 / 0
    _, rv2, _, _ = N.running(mean, var + 2.0, 2, 0.1, np.zeros(4), np.ones(4))
    assert np.allclose(rv2, 0.9 + 0.4, rtol=1e-15)                         # P / (P - 1) = 2


def test_documented_casts_stay_within_fp32_rounding():
    """stat=float32 (mean and rstd rounded to fp32, as the kernels store them) moves the float64 leg by a few fp32 roundings of
    the magnitude at most; the mask is taken from the output's sign, so +-0.0 and negatives take the slope."""
    y, res, dz, gamma, beta, _, _ = data(260, 64, True)
    z64, _, _ = N.bn_forward(y, gamma, beta, res, 1e-5, N.LEAKY, 0.2, stat=np.float64)
    z32, _, _ = N.bn_forward(y, gamma, beta, res, 1e-5, N.LEAKY, 0.2, stat=np.float32)
    # the casts move y * scale by one rounding and mean * scale by two; shift itself may cancel, so its two terms are counted apart
    mean, _, rstd = N.stats(y, 1e-5)
    mag = np.abs(y * gamma * rstd) + np.abs(beta) + np.abs(mean * gamma * rstd) + np.abs(res)
    assert 0 < N.normalised(z32 - z64, mag).max() <= 2 * 2.0 ** -24
    g, _ = N.act_bwd(np.ones(4), np.array([0.0, -0.0, -1.0, 1.0]), N.LEAKY, 0.2)
    assert np.array_equal(g, [0.2, 0.2, 0.2, 1.0])
    g, _ = N.act_bwd(np.ones(2), np.array([0.0, 1.0]), N.LEAKY, 0.0)
    assert np.array_equal(g, [0.0, 1.0])


def test_bf16_rounding_is_torchs():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 3
    x[:4] = torch.tensor([1.00390625, 1.01171875, 0.0, -1.00390625])        # ties: to even
    assert np.array_equal(N.bf16_round(x.numpy()), x.bfloat16().float().numpy())
    assert N.bf16_half_ulp(np.array([1.0, 1.99, 2.0, 0.0]), 0.0).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0]
    assert N.bf16_half_ulp(np.array([1.99]), 0.02).tolist() == [2.0 ** -7]


@pytest.mark.parametrize("lr,betas,eps", [(1e-3, (0.9, 0.999), 1e-8), (3e-2, (0.5, 0.9), 1e-3)])
def test_adam_float64_leg_is_torch(lr, betas, eps):
    g = np.random.default_rng(5)
    p = g.standard_normal(1027)
    pt = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=betas, eps=eps, foreach=False)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, 6):
        grad = g.standard_normal(1027) * 10.0 ** (t - 3)
        grad[::10] = 0.0
        pt.grad = torch.from_numpy(grad.copy())
        opt.step()
        (p, m, v), (mag_p, mag_m, mag_v) = N.adam_step(p, grad, m, v, lr, betas[0], betas[1], eps, t)
        st = opt.state[pt]
        close(p, pt.detach().numpy(), mag_p, f"p, step {t}")
        close(m, st["exp_avg"].numpy(), mag_m, f"m, step {t}")
        close(v, st["exp_avg_sq"].numpy(), mag_v, f"v, step {t}")
    assert not m[::10].any() and not v[::10].any()
