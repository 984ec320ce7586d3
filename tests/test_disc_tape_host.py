"""The discriminators' part of tests/_step_tape.py judged on the host (the pattern of tests/test_step_tape_host.py): a CPU stand-in
that lays the steps of oracle.adversarial_ref.DomainDiscriminatorRef and oracle.uda_ref.FeatureDiscriminatorRef out as the recorder's
builders lay the engine's out must be accepted at every case shape of tests/test_gpu_disc_tape.py, fifteen wrong steps must each be
refused by the check meant for them, and the activation band of the reference legs alone must stay far inside the cap.

The stand-in walks the reference's modules and seeded weights by hand, in the engine's order and with the engine's buffers: channels
padded to the storage's granule (4 fp32, 8 bf16), the first image-level convolution's output stored post-activation, a conv bias in
front of every BatchNorm, BatchNorm from float64 statistics cast to fp32, the pooled tails from the forward's own outputs, the
in-place act_bwd, one gradient arena per backward (the concatenation of its gradients) summed in fp32, running statistics moved once
per forward, and the folded eval pass.  Every value is the fp32 function of the recorded inputs (rounded once to bf16 where the
engine stores bf16).
"""
import copy

import numpy as np
import pytest
import torch

import _conv_ref as R
import _loss_ref as LR
import _norm_ref as N
import _step_tape as T

F32, F64 = np.float32, np.float64
MOM = float(np.float32(0.1))
f32 = torch.float32


def nhwc(t, pad_to):
    a = np.ascontiguousarray(t.detach().permute(0, 2, 3, 1).numpy().astype(F32))
    return np.pad(a, ((0, 0),) * 3 + ((0, pad_to - a.shape[-1]),))


def vec(t):
    return t.detach().numpy().astype(F32)


def ceil_to(c, a):
    return (c + a - 1) // a * a


def phys(w, cin_p, cout_p):
    out = np.zeros((cout_p,) + w.shape[1:3] + (cin_p,), dtype=F32)
    out[:w.shape[0], :, :, :w.shape[3]] = w
    return out


def self_info(z):
    return -torch.softmax(z, 1) * torch.log_softmax(z, 1) / float(np.log(z.shape[1]))


class Standin:
    """kind 'image' (DomainDiscriminatorRef over ``cin`` channels, sigmoid tail) or 'feature' (FeatureDiscriminatorRef(512), the row-0
    tail); storage 'fp32' | 'bf16'."""

    def __init__(self, kind, storage="fp32", cin=3):
        self.kind, self.storage, self.bf16, self.align = kind, storage, storage == "bf16", 8 if storage == "bf16" else 4
        if kind == "image":
            from oracle.adversarial_ref import DomainDiscriminatorRef
            torch.manual_seed(1234)
            ref = DomainDiscriminatorRef(cin).train()
            f = ref.features
            self.stack = [("features.0", f[0], None, None), ("features.2", f[2], "features.3", f[3]), ("features.5", f[5], "features.6", f[6]),
                          ("features.8", f[8], "features.9", f[9])]
            lin = ref.classifier[2]
            self.slope, self.tail = 0.2, ("classifier.2", True, vec(lin.weight)[0], vec(lin.bias))
        else:
            from oracle.uda_ref import FeatureDiscriminatorRef
            torch.manual_seed(7)
            d = FeatureDiscriminatorRef(512).train().discriminator
            self.stack = [(f"discriminator.{i}", d[i], f"discriminator.{i + 1}", d[i + 1]) for i in (0, 3, 6)]
            self.slope, self.tail = 0.0, ("discriminator.9", False, vec(d[9].weight)[0, :, 0, 0], vec(d[9].bias))
        self.state = {bn: (np.zeros(m.num_features, F32), np.ones(m.num_features, F32), 0) for _, _, bn, m in self.stack if m is not None}
        self.delivered, self.arena = [], None

    def q(self, v):
        return N.bf16_round(v) if self.bf16 else np.asarray(v, dtype=F32)

    def _conv(self, name, conv, h):
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        L = T.Layer(name=name, k=k, stride=s, pad=p, route="igemm", x=T.Inp("plain", t=h), storage=self.storage,
                    w=np.ascontiguousarray(conv.weight.detach().permute(0, 2, 3, 1).numpy()), bias=vec(conv.bias))
        cout_p = ceil_to(L.w.shape[0], self.align)
        y = (R.torch_fwd(h, T.phys_weight(L, h.shape[-1], cout_p), s, p, f32) + np.pad(L.bias, (0, cout_p - L.bias.shape[0]))).astype(F32)
        return L, y

    def _tail(self, h):
        name, sigmoid, w, b = self.tail
        n, _, _, c = h.shape
        r = LR.tail_forward(h.reshape(n, -1, c), w, b, sigmoid, F32)
        return {"layer": name, "sigmoid": sigmoid, "bf16": self.bf16, "z": h, "w": w, "b": b, "pooled": r["pooled"][0], "out": r["out"][0], "dp": None}

    def forward(self, x):
        """A training forward of x [n, c, h, w]: the record the backward continues."""
        h, layers = self.q(nhwc(x, ceil_to(x.shape[1], self.align))), {}
        before = copy.deepcopy(self.state)
        for name, conv, bn_name, bn in self.stack:
            L, y = self._conv(name, conv, h)
            if bn is None:
                L.y, L.fused_act, L.fused_slope = self.q(R.leaky(y, self.slope, F32)), N.LEAKY, self.slope
                h = L.y
            else:
                y = self.q(y)
                c = y.shape[-1]
                mean, var, rstd = N.stats(y.reshape(-1, c), bn.eps)
                rm, rv, nbt = self.state[bn_name]
                rm, rv, _, _ = N.running(mean, var, y.size // c, MOM, rm, rv)
                self.state[bn_name] = (rm.astype(F32), rv.astype(F32), nbt + 1)
                mean, rstd = mean.astype(F32), rstd.astype(F32)
                _, _, sc, sh = N._coeffs(vec(bn.weight), vec(bn.bias), mean, rstd, F32, F32)
                L.__dict__.update(y=y, z=self.q(R.bn_apply_f32(y, sc, sh, self.slope)), mean=mean, rstd=rstd, gamma=vec(bn.weight), beta=vec(bn.bias),
                                  eps=bn.eps, act=N.LEAKY, slope=self.slope, bn_name=bn_name)
                h = L.z
            layers[name] = L
        return {"layers": layers, "pool": None, "calls": [], "tail": self._tail(h), "bn": (before, copy.deepcopy(self.state))}

    def backward(self, f, dp, want_dx=False):
        """The backward of forward record ``f`` in the engine's order; delivers its arena."""
        t, calls, grads = f["tail"], f["calls"], []
        n, hh, ww, c = t["z"].shape
        r = LR.tail_backward(dp, t["out"], t["pooled"], t["w"], hh * ww, t["sigmoid"], F32)
        dz = self.q(np.broadcast_to(r["dz"][0][:, None, None, :], (n, hh, ww, c)).copy())
        t.update(dp=np.asarray(dp, dtype=F32), dz=dz, gw=r["dw"][0].astype(F32), gb=F32(r["db"][0]), gw_old=np.zeros(c, F32), gb_old=np.zeros(1, F32))
        grads += [t["gw"], np.reshape(t["gb"], 1)]
        if self.kind == "feature":
            block = np.zeros((4, c), F32)
            block[0] = t["gw"]
            t.update(block=block, block_old=np.zeros_like(block))
            grads.append(block[1:])
        stack = list(f["layers"].values())
        for i in range(len(stack) - 1, -1, -1):
            L = stack[i]
            cp = L.y.shape[-1]
            if L.gamma is None:
                new = self.q(N.act_bwd(dz, L.y, N.LEAKY, self.slope, F32)[0])
                calls.append({"kind": "act", "layer": L.name, "dz": dz, "dy": new})
                dy = new
            else:
                y2 = L.y.reshape(-1, cp)
                sl = F64(F32(self.slope))
                if self.bf16:
                    factor, mask = np.where(L.z.reshape(-1, cp) > 0, 1.0, sl), "z"
                else:
                    factor, mask = np.where(T.band_of(L)[1] > 0, 1.0, sl), "recompute"
                b = T.bn_backward_from(dz.reshape(-1, cp), factor, y2, L.mean, L.rstd, L.gamma, F32)
                dy = self.q(b["dy"][0]).reshape(L.y.shape)
                calls.append({"kind": "bn", "layer": L.name, "dz": dz, "dy": dy, "dgamma": b["dgamma"][0], "dbeta": b["dbeta"][0], "fused": False,
                              "mask": mask, "dres": None, "dres_old": None})
                grads += [b["dgamma"][0], b["dbeta"][0]]
            x = L.x.t
            gw = R.torch_wgrad(x, dy, L.k, L.stride, L.pad, f32)
            gb = N.channel_sum(dy.reshape(-1, cp), F32)[0]
            call = {"kind": "conv", "layer": L.name, "dy": dy, "gw_old": np.zeros_like(gw), "gw": gw, "gb_old": np.zeros(cp, F32), "gb": gb,
                    "wgrad_route": "generic", "dgrad_route": None, "dx_kind": None, "dx_old": None, "da_old": None, "d_skip": None, "bn_fused": False}
            grads += [gw, gb]
            if i > 0 or want_dx:
                dx = self.q(R.torch_dgrad(dy, T.phys_weight(L, x.shape[-1], cp), L.stride, L.pad, x.shape[1], x.shape[2], f32))
                call.update(dgrad_route="igemm", dx_kind="plain", dx=dx)
                dz = dx
            calls.append(call)
        arena = np.concatenate([np.ravel(g) for g in grads]).astype(F32)
        self.delivered.append(arena)
        self.arena = arena if self.arena is None else (self.arena + arena).astype(F32)
        return f

    def running(self, forwards):
        out = []
        for name, _, bn_name, bn in self.stack:
            if bn is not None:
                (rm0, rv0, nbt0), (rm, rv, nbt) = forwards[0]["bn"][0][bn_name], forwards[-1]["bn"][1][bn_name]
                out.append({"layer": bn_name, "ys": [f["layers"][name].y for f in forwards], "eps": bn.eps, "momentum": bn.momentum, "bf16": self.bf16,
                            "rm0": rm0, "rv0": rv0, "nbt0": nbt0, "rm": rm, "rv": rv, "nbt": nbt})
        return out

    def eval_forward(self, x):
        """The folded eval pass with the running statistics as they stand."""
        h, evals = self.q(nhwc(x, ceil_to(x.shape[1], self.align))), []
        for name, conv, bn_name, bn in self.stack:
            L, y = self._conv(name, conv, h)
            if bn is None:
                h = self.q(R.leaky(y, self.slope, F32))
                continue
            cout_p = y.shape[-1]
            w32, (rm, rv, _) = phys(L.w, h.shape[-1], cout_p), self.state[bn_name]
            wf, bf, _ = R.bn_fold_ref(w32, np.pad(L.bias, (0, cout_p - L.bias.shape[0])), vec(bn.weight), vec(bn.bias), rm, rv, bn.eps, F32)
            wf16 = N.bf16_round(wf) if self.bf16 else None
            z = self.q(R.leaky((R.torch_fwd(h, wf16 if self.bf16 else wf, L.stride, L.pad, f32) + bf).astype(F32), self.slope, F32))
            evals.append({"layer": name, "storage": self.storage, "x": T.Inp("plain", t=h), "k": L.k, "stride": L.stride, "pad": L.pad, "w32": w32,
                          "bias": np.pad(L.bias, (0, cout_p - L.bias.shape[0])), "gamma": vec(bn.weight), "beta": vec(bn.bias), "rm": rm, "rv": rv,
                          "eps": bn.eps, "wf": wf, "bf": bf, "wf16": wf16, "z": z, "act": N.LEAKY, "slope": self.slope, "residual": None})
            h = z
        return {"evals": evals, "tail": self._tail(h)}


def _dp(out, label, weight):
    """The gradient of weight x mean BCE-with-logits(out, label) with respect to out, in fp32 (the discriminators' verdicts enter the
    loss as logits, the image-level probabilities included)."""
    return LR.bce(out, label, weight, 1.0, F32)["dx"][0].astype(F32)


def _inputs(case):
    from oracle.adversarial_ref import synthetic_batch
    g = torch.Generator().manual_seed(5)
    if case.startswith("img"):
        n, h, w = (1, 32, 96) if case.endswith("1x32x96") else (2, 64, 64)
        src, _, tgt = synthetic_batch(n, h, w, seed=0)
        return [src] if n == 1 else [src, tgt]
    if case.startswith("out"):
        return [self_info(3.0 * torch.randn(2, int(case.rsplit("-", 1)[1]), 64, 64, generator=g))]
    return [torch.randn(2, 512, 2, 2, generator=g), torch.randn(2, 512, 4, 4, generator=g)]


CASES = {"img-fp32": ("image", "fp32", 3), "img-bf16": ("image", "bf16", 3), "img-fp32-1x32x96": ("image", "fp32", 3),
         "out-fp32-23": ("image", "fp32", 23), "out-bf16-23": ("image", "bf16", 23), "out-bf16-5": ("image", "bf16", 5),
         "feat-fp32": ("feature", "fp32", 512)}
_RUNS = {}


def run(case):
    """{"steps": the tapes of the case's forwards, "delivered", "arena", "running", "eval"}: the case's step(s) as tests/test_gpu_disc_tape.py
    takes them, then one eval forward of the first input."""
    if case not in _RUNS:
        S = Standin(*CASES[case])
        xs = _inputs(case)
        if case.startswith("img"):                       # D(src), D(tgt), one backward: the later forward's backward runs first
            fs = [S.forward(x) for x in xs]
            for f, label in reversed(list(zip(fs, (1.0, 0.0)))):
                S.backward(f, _dp(f["tail"]["out"], label, 0.5 if len(fs) == 2 else 1.0))
        elif case.startswith("out"):
            fs = [S.forward(xs[0])]
            S.backward(fs[0], _dp(fs[0]["tail"]["out"], 1.0, 0.001), want_dx=True)
        else:                                            # two steps onto one gradient arena: with and without the input's gradient
            fs = []
            for x, label, want in zip(xs, (1.0, 0.0), (True, False)):
                f = S.forward(x)
                fs.append(S.backward(f, _dp(f["tail"]["out"], label, 1.0), want_dx=want))
        _RUNS[case] = {"steps": fs, "delivered": S.delivered, "arena": S.arena, "running": S.running(fs), "eval": S.eval_forward(xs[0])}
    return _RUNS[case]


def check_case(rep, r, only=None):
    keep = only or (lambda name: True)
    for f in r["steps"]:
        T.check_step(rep, f, only)
    if keep("arena"):
        T.check_grad_sum(rep, "arena", r["delivered"], r["arena"])
    for b in r["running"]:
        if keep(b["layer"]):
            T.check_running(rep, b)
    T.check_eval(rep, r["eval"], only)


KINDS = {"y", "mean", "rstd", "z", "dy", "dgamma", "dbeta", "wgrad", "dbias", "gw-old", "gb-old", "gw-pad", "dx", "visits", "pooled", "out",
         "dz", "dw", "db", "dw-old", "db-old", "grad-sum", "running_mean", "running_var", "batches", "fold", "z-eval"}
EXTRA = {"img-fp32": {"act-bwd", "band"}, "img-bf16": {"act-bwd", "fold-bf16"}, "img-fp32-1x32x96": {"act-bwd", "band"},
         "out-fp32-23": {"act-bwd", "band", "dx-pad"}, "out-bf16-23": {"act-bwd", "dx-pad", "fold-bf16"}, "out-bf16-5": {"act-bwd", "dx-pad", "fold-bf16"},
         "feat-fp32": {"band", "block-old", "dw-rows", "dw-row0"}}


@pytest.mark.parametrize("case", list(CASES))
def test_the_stand_in_is_accepted(case):
    r = run(case)
    assert len(r["delivered"]) == (1 if case.startswith("out") or case.endswith("1x32x96") else 2)
    rep = T.Report(f"stand-in {case}")
    check_case(rep, r)
    rep.done()
    assert set(rep.worst) >= KINDS | EXTRA[case], sorted((KINDS | EXTRA[case]) - set(rep.worst))
    if rep.band:
        assert max(rep.band.values()) <= T.BAND_CAP / 10


# --------------------------------------------------------------------------------------------------------------------- mutants
def _call(f, layer, kind):
    return next(c for c in f["calls"] if c["layer"] == layer and c["kind"] == kind)


def _conv0(r, slope, bias):
    L = r["steps"][0]["layers"]["features.0"]
    x = L.x.t
    y = R.torch_fwd(x, T.phys_weight(L, x.shape[-1], L.y.shape[-1]), L.stride, L.pad, f32)
    L.y = R.leaky((y + (L.bias if bias else 0.0)).astype(F32), slope, F32)


def m_conv0_relu(r):
    _conv0(r, 0.0, True)


def m_conv0_without_bias(r):
    _conv0(r, 0.2, False)


def m_act_mask_from_dz(r):
    c = _call(r["steps"][0], "features.0", "act")
    c["dy"] = (c["dz"] * np.where(c["dz"] > 0, F32(1), F32(0.2))).astype(F32)


def m_y_without_bias(r):
    L = r["steps"][0]["layers"]["discriminator.3"]
    L.y = (L.y - L.bias).astype(F32)


def m_dbias_from_dz(r):
    f = r["steps"][0]
    c = _call(f, "discriminator.3", "conv")
    c["gb"] = N.channel_sum(_call(f, "discriminator.3", "bn")["dz"].reshape(-1, c["dy"].shape[-1]), F32)[0]


def m_pooled_wrong_count(r):
    t = r["steps"][0]["tail"]
    hw = t["z"].shape[1] * t["z"].shape[2]
    t["pooled"] = (t["pooled"] * F32(hw / (hw + 1.0))).astype(F32)


def m_tail_dz_without_sigmoid_factor(r):
    t = r["steps"][0]["tail"]
    n, hh, ww, c = t["z"].shape
    t["dz"] = np.broadcast_to((t["w"][None, :] * (t["dp"] / F32(hh * ww))[:, None])[:, None, None, :], t["z"].shape).astype(F32)


def m_row1_written(r):
    t = r["steps"][0]["tail"]
    t["block"][1] = t["block"][0]


def m_second_arena_overwrites(r):
    r["arena"] = r["delivered"][1].copy()


def m_running_moved_once(r):
    b = r["running"][0]
    L = r["steps"][0]["layers"]["features.2"]
    mean, var, _ = N.stats(L.y.reshape(-1, L.y.shape[-1]), L.eps)
    rm, rv, _, _ = N.running(mean, var, L.y.size // L.y.shape[-1], MOM, b["rm0"], b["rv0"])
    b["rm"], b["rv"] = rm.astype(F32), rv.astype(F32)


def m_dx_pad_lane(r):
    _call(r["steps"][0], "features.0", "conv")["dx"][0, 3, 5, 23] = F32(1e-30)


def _refold(ev, eps=None, bias=True):
    wf, bf, _ = R.bn_fold_ref(ev["w32"], ev["bias"] if bias else None, ev["gamma"], ev["beta"], ev["rm"], ev["rv"], ev["eps"] if eps is None else eps, F32)
    ev["wf"], ev["bf"] = wf, bf


def m_fold_without_eps(r):
    _refold(r["eval"]["evals"][0], eps=0.0)


def m_fold_drops_conv_bias(r):
    _refold(r["eval"]["evals"][1], bias=False)


def m_eval_without_activation(r):
    ev = r["eval"]["evals"][2]
    ev["z"] = (R.torch_fwd(ev["x"].t, ev["wf"], ev["stride"], ev["pad"], f32) + ev["bf"]).astype(F32)


def m_bf16_fold_not_rounded(r):
    ev = r["eval"]["evals"][0]
    ev["wf16"] = ev["wf"].copy()


MUTANTS = [(m_conv0_relu, "img-fp32", "features.0", "y"), (m_conv0_without_bias, "img-fp32", "features.0", "y"),
           (m_act_mask_from_dz, "img-fp32", "features.0", "act-bwd"), (m_y_without_bias, "feat-fp32", "discriminator.3", "y"),
           (m_dbias_from_dz, "feat-fp32", "discriminator.3", "dbias"), (m_pooled_wrong_count, "img-fp32", "classifier.2", "pooled"),
           (m_tail_dz_without_sigmoid_factor, "img-fp32", "classifier.2", "dz"), (m_row1_written, "feat-fp32", "discriminator.9", "dw-rows"),
           (m_second_arena_overwrites, "img-fp32", "arena", "grad-sum"), (m_running_moved_once, "img-fp32", "features.3", "running_mean"),
           (m_dx_pad_lane, "out-fp32-23", "features.0", "dx-pad"), (m_fold_without_eps, "img-fp32", "features.2", "fold"),
           (m_fold_drops_conv_bias, "feat-fp32", "discriminator.3", "fold"), (m_eval_without_activation, "img-fp32", "features.8", "z-eval"),
           (m_bf16_fold_not_rounded, "img-bf16", "features.2", "fold-bf16")]


@pytest.mark.parametrize("mutate,case,layer,kind", MUTANTS, ids=[m[0].__name__[2:] for m in MUTANTS])
def test_a_wrong_step_is_refused_by_the_check_meant_for_it(mutate, case, layer, kind):
    r = copy.deepcopy(run(case))
    only = lambda name: name == layer  # noqa: E731
    clean = T.Report(f"unmutated {case} {layer}")
    check_case(clean, r, only)
    assert (layer, kind) not in clean.failed and kind in clean.worst, f"{layer}:{kind} is not checked on the unmutated {case}"
    mutate(r)
    rep = T.Report(f"mutant {mutate.__name__[2:]}")
    check_case(rep, r, only)
    assert (layer, kind) in rep.failed, f"{mutate.__name__}: passed {layer}:{kind} (failed: {rep.failed})"
    with pytest.raises(AssertionError):
        rep.done()


@pytest.mark.parametrize("case", ["img-bf16", "feat-fp32"])
def test_the_eval_pass_is_graded_with_its_tail(case):
    r = copy.deepcopy(run(case))
    rep = T.Report(f"stand-in {case} eval")
    T.check_eval(rep, r["eval"])
    rep.done()
    assert set(rep.worst) == {"fold", "z-eval", "pooled", "out"} | ({"fold-bf16"} if case == "img-bf16" else set())
    r["eval"]["tail"]["out"] = r["eval"]["tail"]["out"] * F32(1.001)           # a verdict that is not the tail of the last folded layer
    rep = T.Report(f"stand-in {case} eval, wrong verdict")
    T.check_eval(rep, r["eval"])
    assert rep.failed == [(r["eval"]["tail"]["layer"], "out")]


def test_calls_of_another_forward_are_missed():
    """Two forwards, then one backward: a forward whose act_bwd (or BatchNorm backward) was attributed to the other plan misses its
    visit count, and so does the forward that got it twice."""
    r = copy.deepcopy(run("img-fp32"))
    a, b = r["steps"]
    for layer, kind in (("features.0", "act"), ("features.5", "bn")):
        b["calls"].append(a["calls"].pop(a["calls"].index(_call(a, layer, kind))))
    for f in (a, b):
        rep = T.Report("misattributed calls")
        T.check_step(rep, f, only=lambda name: name in ("features.0", "features.5"))
        assert ("features.0", "visits") in rep.failed and ("features.5", "visits") in rep.failed, rep.failed


@pytest.mark.parametrize("case", list(CASES))
def test_band_share_of_the_reference_legs(case):
    """fp32 against float64 on the same inputs: wherever a BatchNorm backward re-evaluates its mask from y, the share of the layer's
    elements whose activation argument lies inside the band must be at most a tenth of the cap."""
    worst = 0.0
    for i, f in enumerate(run(case)["steps"]):
        for L in f["layers"].values():
            if L.gamma is not None and L.act == N.LEAKY:
                band = T.band_of(L)[2]
                share = float(band.mean())
                worst = max(worst, share)
                T._log(f"{T.PREFIX} band-host {case} forward {i} | {L.name} | {int(band.sum())} of {band.size} ({share:.3e})")
                assert share <= T.BAND_CAP / 10, f"{L.name}: band share {share:.3e} of the reference alone"
    assert worst <= T.BAND_CAP / 10
