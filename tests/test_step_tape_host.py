"""tests/_step_tape.py judged on the host: a CPU stand-in that lays one training step of oracle.unet_ref.UnetRef out as the recorder
lays the engine's out must be accepted, ten wrong steps must each be refused by the check meant for them, and the activation band of
the reference legs alone (fp32 against float64 on the same inputs) must stay far inside the cap the GPU test applies.

The stand-in takes UnetRef's modules and seeded weights (as tests/_parity.py::pair seeds them) and walks them by hand, in the engine's
order and with the engine's buffers: BatchNorm from float64 statistics cast to fp32, the unwritten activations of the full-resolution
decoder tail as (y, scale, shift), the fused decoder inputs as (a, skip), gradient slots whose first writer overwrites and later
writers accumulate (dx_acc, dres), UpGrad.da at half resolution.  It does not go through autograd hooks: autograd sums the
gradients of a tensor with several consumers in an order of its own, and a layer-local grade needs every recorded output to be the
fp32 function of the recorded inputs to the last bit of the legs.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_ref as R
import _norm_ref as N
import _step_tape as T

F32, F64 = np.float32, np.float64
CASES = (("resnet18", 2, 64, 64), ("resnet50", 2, 64, 64), ("resnet18", 1, 64, 96))       # network and size of every GPU case
LAZY = ("decoder.blocks.3.conv1.0", "decoder.blocks.4.conv1.0", "decoder.blocks.4.conv2.0")     # never written (<= 32 channels)
# forward routes of the fp32 engine (test_forward_routes_of_r18_fp32_at_8x512): they choose the grader
ROUTE = {"encoder.conv1": "stem", "decoder.blocks.3.conv2.0": "frag_bnin", "decoder.blocks.4.conv2.0": "n16", "segmentation_head.0": "frag_bnin"}


def nhwc(t, pad_to=None):
    a = np.ascontiguousarray(t.detach().permute(0, 2, 3, 1).numpy().astype(F32))
    return a if pad_to is None or a.shape[-1] == pad_to else np.pad(a, ((0, 0),) * 3 + ((0, pad_to - a.shape[-1]),))


def vec(t, pad_to=None):
    a = t.detach().numpy().astype(F32)
    return a if pad_to is None else np.pad(a, (0, pad_to - a.shape[0]))


class Standin:
    def __init__(self, name, n, h, w):
        from oracle.adversarial_ref import synthetic_batch
        from oracle.unet_ref import UnetRef
        torch.manual_seed(1234)
        self.ref = UnetRef(name, classes=23).train()
        self.x, self.target, _ = synthetic_batch(n, h, w, seed=0)
        self.names = {id(m): k for k, m in self.ref.named_modules()}
        self.layers, self.t, self.calls, self.slots, self.pool = {}, {}, [], {}, None

    # ---- forward
    def cba(self, conv, bn, xin, act=True, residual=None):
        """xin: a tensor, a layer name (that layer's unwritten activation) or ("up", a, skip)."""
        name = self.names[id(conv)]
        route = ROUTE.get(name, "phase" if isinstance(xin, tuple) else "frag" if conv.stride == (1, 1) and conv.kernel_size == (3, 3) else "igemm")
        if isinstance(xin, tuple):
            _, a, skip = xin
            inp = T.Inp("upcat", a=T.Inp("plain", t=nhwc(a)), skip=None if skip is None else nhwc(skip))
            up = F.interpolate(a, scale_factor=2.0, mode="nearest")
            xt = up if skip is None else torch.cat([up, skip], 1)
        elif isinstance(xin, str):
            p = self.t[xin]
            inp = T.Inp("lazy", y=nhwc(p["y"]), scale=vec(p["scale"]), shift=vec(p["shift"]), act=N.LEAKY, slope=0.0)
            xt = p["z"]
        else:
            xt = xin
            inp = T.Inp("plain", t=nhwc(xin, 4 if xin.shape[1] == 3 else None))
        y = F.conv2d(xt, conv.weight, conv.bias, conv.stride, conv.padding)
        L = T.Layer(name=name, k=conv.kernel_size[0], stride=conv.stride[0], pad=conv.padding[0], route=route, x=inp,
                    w=np.ascontiguousarray(conv.weight.detach().permute(0, 2, 3, 1).numpy()), bias=None if conv.bias is None else vec(conv.bias))
        self.layers[name] = L
        tt = self.t[name] = {"conv": conv, "bn": bn, "x": xt, "xin": xin, "y": y, "residual": residual}
        if bn is None:
            L.y = nhwc(y, T.R.cdiv(y.shape[1], 4) * 4)
            return y
        yd = y.double()
        mean = yd.mean((0, 2, 3))
        var = ((yd * yd).mean((0, 2, 3)) - mean * mean).clamp_min(0.0)
        mean, rstd = mean.float(), (1.0 / torch.sqrt(var + bn.eps)).float()
        scale = bn.weight * rstd
        shift = bn.bias - mean * scale
        t = (yd * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).float()
        if residual is not None:
            t = t + residual
        z = F.relu(t) if act else t
        tt.update(mean=mean, rstd=rstd, scale=scale, shift=shift, pre=t, z=z, act=act)
        lazy = name in LAZY
        L.__dict__.update(y=nhwc(y), z=None if lazy else nhwc(z), lazy=(vec(scale), vec(shift)) if lazy else None, mean=vec(mean), rstd=vec(rstd),
                          gamma=vec(bn.weight), beta=vec(bn.bias), eps=bn.eps, act=N.LEAKY if act else N.NONE, slope=0.0,
                          residual=None if residual is None else nhwc(residual))
        return z

    def block(self, blk, x):
        bottleneck = hasattr(blk, "conv3")
        a = self.cba(blk.conv1, blk.bn1, x)
        if bottleneck:
            a = self.cba(blk.conv2, blk.bn2, a)
        idt = x if blk.downsample is None else self.cba(blk.downsample[0], blk.downsample[1], x, act=False)
        last = (blk.conv3, blk.bn3) if bottleneck else (blk.conv2, blk.bn2)
        return self.cba(*last, a, residual=idt)

    @torch.no_grad()
    def forward(self):
        enc = self.ref.encoder
        f1 = self.cba(enc.conv1, enc.bn1, self.x)
        pooled, idx = F.max_pool2d(f1, 3, 2, 1, return_indices=True)
        wi = f1.shape[3]
        oy, ox = torch.meshgrid(torch.arange(pooled.shape[2]), torch.arange(pooled.shape[3]), indexing="ij")
        tap = (idx // wi - (2 * oy - 1)) * 3 + (idx % wi - (2 * ox - 1))
        self.pool = (nhwc(f1), nhwc(pooled), np.ascontiguousarray(tap.permute(0, 2, 3, 1).numpy().astype(np.uint8)))
        self.f1, self.pooled, self.pool_idx = f1, pooled, idx
        feats, h = [f1], pooled
        self.blocks = []
        for stage in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
            for blk in stage:
                x, h = h, self.block(blk, h)
                self.blocks.append((blk, x, h))
            feats.append(h)
        skips = feats[:-1][::-1]
        self.dec = []
        for i, blk in enumerate(self.ref.decoder.blocks):
            skip = skips[i] if i < len(skips) else None
            x = h
            n1 = self.names[id(blk.conv1[0])]
            self.cba(blk.conv1[0], blk.conv1[1], ("up", x, skip))
            h = self.cba(blk.conv2[0], blk.conv2[1], n1 if n1 in LAZY else self.t[n1]["z"])
            self.dec.append((blk, x, skip, h))
        head = self.ref.segmentation_head[0]
        last = self.names[id(self.ref.decoder.blocks[-1].conv2[0])]
        self.logits = self.cba(head, None, last if last in LAZY else h)
        return self

    # ---- backward, in the engine's order
    def slot(self, t):
        return self.slots.get(id(t))

    def bn_bwd(self, name, dz, dres_to=None):
        """-> dy; dres_to: the tensor whose gradient slot takes the masked gradient (first writer overwrites)."""
        tt = self.t[name]
        y, mean, rstd, gamma = tt["y"], tt["mean"], tt["rstd"], tt["bn"].weight.detach()
        g = dz * (tt["pre"] > 0) if tt["act"] else dz
        p = y.numel() // y.shape[1]
        b = lambda v: v[None, :, None, None]  # noqa: E731
        xhat = (y - b(mean)) * b(rstd)
        dbeta, dgamma = g.double().sum((0, 2, 3)).float(), (g * xhat).double().sum((0, 2, 3)).float()
        dy = b(gamma * rstd) * (g - b(dbeta / p) - xhat * b(dgamma / p))
        call = {"kind": "bn", "layer": name, "dz": nhwc(dz), "dy": nhwc(dy), "dgamma": vec(dgamma), "dbeta": vec(dbeta), "fused": False,
                "mask": "none" if not tt["act"] else "z" if tt["residual"] is not None else "recompute", "dres": None, "dres_old": None}
        if dres_to is not None:
            old = self.slot(dres_to)
            call.update(dres_old=None if old is None else nhwc(old), dres=nhwc(g if old is None else old + g))
            self.slots[id(dres_to)] = g if old is None else old + g
        self.calls.append(call)
        return dy

    def conv_bwd(self, name, dy, dx_to=None, form="plain"):
        """dx_to: the tensor whose slot takes the data gradient (accumulated when the slot exists); form 'upgrad' / 'pair' for a fused input."""
        tt, L = self.t[name], self.layers[name]
        conv, x = tt["conv"], tt["x"]
        w = conv.weight.detach()
        cout_p, cin_p = (w.shape[0] + 3) // 4 * 4, (w.shape[1] + 3) // 4 * 4
        gw = torch.nn.grad.conv2d_weight(x, w.shape, dy, conv.stride, conv.padding)
        gwp = np.zeros((cout_p, L.k, L.k, cin_p), dtype=F32)
        gwp[:w.shape[0], :, :, :w.shape[1]] = gw.permute(0, 2, 3, 1).numpy()
        call = {"kind": "conv", "layer": name, "dy": nhwc(dy, cout_p), "gw_old": np.zeros_like(gwp), "gw": gwp, "gb_old": None, "gb": None,
                "wgrad_route": "bnin" if isinstance(tt["xin"], str) else "halo" if L.k == 3 and L.stride == 1 else "generic",
                "dgrad_route": None, "dx_kind": None, "dx_old": None, "da_old": None, "d_skip": None, "bn_fused": False}
        if conv.bias is not None:
            call.update(gb_old=np.zeros(cout_p, dtype=F32), gb=vec(dy.double().sum((0, 2, 3)).float(), cout_p))
        if form != "plain" or dx_to is not None:
            dx = torch.nn.grad.conv2d_input(x.shape, w, dy, conv.stride, conv.padding)
            call["dgrad_route"] = "phase" if form == "upgrad" else "n16" if w.shape[1] == 16 else "frag" if L.k == 3 and L.stride == 1 else "igemm"
        if form == "plain" and dx_to is not None:
            old = self.slot(dx_to)
            new = dx if old is None else old + dx
            call.update(dx_kind="plain", dx_old=None if old is None else nhwc(old), dx=nhwc(new))
            self.slots[id(dx_to)] = new
        elif form != "plain":
            _, a, skip = tt["xin"]
            ca = a.shape[1]
            d_up = dx[:, :ca]
            da = ((d_up[:, :, 0::2, 0::2] + d_up[:, :, 0::2, 1::2]) + d_up[:, :, 1::2, 0::2]) + d_up[:, :, 1::2, 1::2]
            assert self.slot(a) is None
            self.slots[id(a)] = da
            call.update(dx_kind=form, **({"da": nhwc(da)} if form == "upgrad" else {"d_up": nhwc(d_up)}))
            if skip is not None:
                assert self.slot(skip) is None             # the decoder is the first writer of every skip gradient
                self.slots[id(skip)] = dx[:, ca:]
                call["d_skip"] = nhwc(dx[:, ca:])
        self.calls.append(call)

    def backward(self):
        nm = lambda m: self.names[id(m)]  # noqa: E731
        lg = self.logits.detach().requires_grad_(True)
        F.cross_entropy(lg, self.target).backward()
        head = self.ref.segmentation_head[0]
        with torch.no_grad():
            h_last = self.dec[-1][3]
            self.conv_bwd(nm(head), lg.grad, dx_to=h_last)
            for i, (blk, x, skip, out) in reversed(list(enumerate(self.dec))):
                n1, n2 = nm(blk.conv1[0]), nm(blk.conv2[0])
                self.conv_bwd(n2, self.bn_bwd(n2, self.slots.pop(id(out))), dx_to=self.t[n1]["z"])
                self.conv_bwd(n1, self.bn_bwd(n1, self.slots.pop(id(self.t[n1]["z"]))), form="pair" if i == 3 else "upgrad")
            for blk, x, out in reversed(self.blocks):
                n1, n2 = nm(blk.conv1), nm(blk.conv2)
                a1 = self.t[n1]["z"]
                d_out = self.slots.pop(id(out))
                if blk.downsample is None:
                    dy2 = self.bn_bwd(n2, d_out, dres_to=x)
                    self.conv_bwd(n2, dy2, dx_to=a1)
                else:
                    nd = nm(blk.downsample[0])
                    idt = self.t[nd]["z"]
                    dy2 = self.bn_bwd(n2, d_out, dres_to=idt)
                    self.conv_bwd(n2, dy2, dx_to=a1)
                    self.conv_bwd(nd, self.bn_bwd(nd, self.slots.pop(id(idt))), dx_to=x)
                self.conv_bwd(n1, self.bn_bwd(n1, self.slots.pop(id(a1))), dx_to=x)
            d_pooled = self.slots.pop(id(self.pooled))
            d_f1 = self.slots.pop(id(self.f1)) + F.max_unpool2d(d_pooled, self.pool_idx, 3, 2, 1, self.f1.shape[2:])
            stem = nm(self.ref.encoder.conv1)
            self.conv_bwd(stem, self.bn_bwd(stem, d_f1))
        return self

    def tape(self):
        return {"layers": self.layers, "pool": self.pool, "calls": self.calls}


@pytest.fixture(scope="module")
def base():
    return Standin("resnet18", 2, 64, 64).forward().backward().tape()


def test_the_stand_in_is_accepted(base):
    layers, calls = base["layers"], base["calls"]
    assert len(layers) == 31 and sum(c["kind"] == "conv" for c in calls) == 31 and sum(c["kind"] == "bn" for c in calls) == 30
    assert any(c["dx_old"] is not None for c in calls if c["kind"] == "conv"), "no accumulating data gradient"
    assert any(c["dres"] is not None for c in calls if c["kind"] == "bn") and any(c["dx_kind"] == "upgrad" for c in calls if c["kind"] == "conv")
    assert "encoder.layer2.0.downsample.0" in layers and layers["decoder.blocks.3.conv1.0"].lazy is not None
    rep = T.Report("stand-in r18 fp32 2x64x64")
    T.check_step(rep, base)
    rep.done()
    assert set(rep.worst) >= {"y", "mean", "rstd", "scale", "shift", "z", "pooled", "pidx", "dy", "dgamma", "dbeta", "dres", "wgrad", "dbias",
                              "dx", "da", "d_up", "d_skip", "gw-pad", "gw-old", "y-pad", "band", "visits"}
    assert max(rep.band.values()) <= T.BAND_CAP / 10


def _call(tape, layer, kind):
    return next(c for c in tape["calls"] if c["layer"] == layer and c["kind"] == kind)


def _reforward(tape, layer, mm=None, w=None):
    """y of one layer evaluated again in float64 from its recorded input: with another product, or other weights."""
    L = tape["layers"][layer]
    _, x32 = T.materialise(L.x)
    wp = T.phys_weight(L, x32.shape[-1], L.y.shape[-1]) if w is None else w
    L.y = R.im2col_fwd(x32, wp, L.stride, L.pad, mm or np.matmul).astype(F32)


def m_dx_acc_without_old(t):
    c = _call(t, "encoder.layer2.0.conv1", "conv")
    assert c["dx_old"] is not None
    c["dx"] = c["dx"] - c["dx_old"]


def m_border_column(t):
    _call(t, "encoder.layer1.1.conv2", "conv")["dx"][:, :, -1] = 0


def m_wgrad_without_one_image(t):
    c, L = _call(t, "decoder.blocks.2.conv2.0", "conv"), t["layers"]["decoder.blocks.2.conv2.0"]
    x = T.materialise(L.x)[1]
    c["gw"] = R.torch_wgrad(x[:1], c["dy"][:1], 3, 1, 1, torch.float32)


def m_bf16_weights(t):
    L = t["layers"]["encoder.layer1.0.conv1"]
    _reforward(t, L.name, w=N.bf16_round(T.phys_weight(L, 64, 64)))


def m_low_split_term(t):
    """About 2^-17 / sqrt(K) of the magnitude.  The split pipe's bar is set by its truncating leg (5 to 20 x the round-to-nearest leg,
    growing with K), so this mutant stays under it on every 3x3 layer of the network (e/bar 0.01 .. 0.47) and is refused only where K is
    shortest: the 64-channel 1x1 projection, e/bar 1.18."""
    _reforward(t, "encoder.layer2.0.downsample.0", mm=lambda A, B: R.x3_exact(A, B, drop=((2, 0),)))


def m_shift_from_running_mean(t):
    L = t["layers"]["decoder.blocks.3.conv1.0"]
    running = (0.1 * L.mean).astype(F32)                    # momentum 0.1 on the initial zeros
    L.lazy = (L.lazy[0], (L.beta - running * L.lazy[0]).astype(F32))


def m_dgamma_without_last_row(t):
    c, L = _call(t, "encoder.layer3.1.conv1", "bn"), t["layers"]["encoder.layer3.1.conv1"]
    xhat = (L.y.astype(F64) - L.mean) * L.rstd.astype(F64)
    g = c["dz"].astype(F64) * (xhat * L.gamma + L.beta > 0)
    c["dgamma"] = (g * xhat)[:, :-1].sum((0, 1, 2)).astype(F32)


def m_da_three_phases(t):
    c = _call(t, "decoder.blocks.1.conv1.0", "conv")
    L = t["layers"][c["layer"]]
    x = T.materialise(L.x)[1]
    d = R.torch_dgrad(c["dy"], T.phys_weight(L, x.shape[-1], c["dy"].shape[-1]), 1, 1, x.shape[1], x.shape[2], torch.float32)[..., :c["da"].shape[-1]]
    c["da"] = d[:, 0::2, 0::2] + d[:, 0::2, 1::2] + d[:, 1::2, 0::2]


def m_rstd_without_eps(t):
    L = t["layers"]["encoder.layer4.1.conv1"]
    var = N.stats(L.y.reshape(-1, L.y.shape[-1]), L.eps)[1]
    L.rstd = (1.0 / np.sqrt(var)).astype(F32)


def m_pool_index_one_window_right(t):
    f1, pooled, tap = t["pool"]
    t["pool"] = (f1, pooled, np.concatenate([tap[:, :, 1:], tap[:, :, -1:]], axis=2))


MUTANTS = [(m_dx_acc_without_old, "encoder.layer2.0.conv1", "dx"), (m_border_column, "encoder.layer1.1.conv2", "dx"),
           (m_wgrad_without_one_image, "decoder.blocks.2.conv2.0", "wgrad"), (m_bf16_weights, "encoder.layer1.0.conv1", "y"),
           (m_low_split_term, "encoder.layer2.0.downsample.0", "y"), (m_shift_from_running_mean, "decoder.blocks.3.conv1.0", "shift"),
           (m_dgamma_without_last_row, "encoder.layer3.1.conv1", "dgamma"), (m_da_three_phases, "decoder.blocks.1.conv1.0", "da"),
           (m_rstd_without_eps, "encoder.layer4.1.conv1", "rstd"), (m_pool_index_one_window_right, "maxpool", "pidx")]


@pytest.mark.parametrize("mutate,layer,kind", MUTANTS, ids=[m[0].__name__[2:] for m in MUTANTS])
def test_a_wrong_step_is_refused_by_the_check_meant_for_it(base, mutate, layer, kind):
    tape = copy.deepcopy(base)
    mutate(tape)
    rep = T.Report(f"mutant {mutate.__name__[2:]}")
    T.check_step(rep, tape, only=lambda name: name == layer)
    assert (layer, kind) in rep.failed, f"{mutate.__name__}: passed {layer}:{kind} (failed: {rep.failed})"
    with pytest.raises(AssertionError):
        rep.done()


@pytest.mark.parametrize("name,n,h,w", CASES, ids=["%s-%dx%dx%d" % c for c in CASES])
def test_band_share_of_the_reference_legs(base, name, n, h, w):
    """fp32 against float64 on the same inputs: the share of a layer's elements whose activation argument lies inside the band must be
    at most a tenth of the cap, for every layer of every GPU case's network and size."""
    layers = base["layers"] if (name, n, h, w) == CASES[0] else Standin(name, n, h, w).forward().layers
    worst = 0.0
    for L in layers.values():
        if L.gamma is not None and L.act == N.LEAKY:
            band = T.band_of(L)[2]
            share = band.mean()
            worst = max(worst, share)
            T._log(f"{T.PREFIX} band-host {name} {n}x{h}x{w} | {L.name} | {int(band.sum())} of {band.size} ({share:.3e})")
            assert share <= T.BAND_CAP / 10, f"{L.name}: band share {share:.3e} of the reference alone"
    assert worst <= T.BAND_CAP / 10
