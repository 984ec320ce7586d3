#!/usr/bin/env python
"""Cost of the CRF refinement at the headline batch (8 x 23 x 512 x 512 fp32 logits, uint8 frames) on one MI355X, for a smooth and
a per-pixel-random frame.

Seeded inputs: logits of spread 2 in the padded NHWC layout of Unet.forward; the "smooth" frame is a slow colour ramp (neighbours
a few levels apart: the colour term stays near 1), the "random" one has independent uniform bytes (the colour term is almost
always 0).  The kernels' work does not depend on the data; the two frames show that.  HIP-event medians over --reps rounds after
--warmup rounds; the legs ALTERNATE inside every round, all in ONE process, every leg runs --inner back-to-back calls between its
two events and reports the time PER CALL.  Per frame and per (radius, dilation, sweeps) in (3,1,5), (3,2,5), (5,2,5):
  * prepare_ms       udaseg_crf_prepare (scores -> log P0, Q0, flags), outputs preallocated
  * step_ms          ONE udaseg_crf_step, outputs preallocated; with it the class chunk the launch used, the LDS bytes its window
                     loops read (every ds_read of a Q row and a frame word, counted from the shapes; staging stores not counted)
                     per clock and CU against the guide's 256 B/clk/CU for wide reads, and the FMA rate of the class updates
  * refine_ms        crf.refine: prepare + sweeps, its buffers and the two small tables allocated per call
and beside them in every round:
  * copy_ms          a device-to-device copy of the score bytes (8 x 512 x 512 x 24 floats)
once per window, on the random frame (--unfold-reps runs, its own events):
  * unfold_ms        the torch composition of the same refinement: torch.nn.functional.unfold of Q, of the frame and of the valid
                     mask per sweep, CHUNKED ONE IMAGE AT A TIME (the [C K^2, H W] block of one image is 1.2 GB at K = 7 and
                     2.9 GB at K = 11); its result is compared with refine's in the run (max difference reported and asserted
                     below 1e-4)
and once:
  * forward_eval_ms  ONE eval-mode r18 segmenter forward of an 8 x 3 x 512 x 512 batch
  * online_label_ms / crf_label_ms   teacher.OnlineLabeler.label beside crf.CrfLabeler.label (defaults) on 8 uint8 frames
Reported, not judged.  One JSON line; --out also writes it to a file together with the git HEAD.  The process ends itself after
--time-limit seconds.

    python tools/bench_crf.py [--reps 10 --warmup 2 --inner 3 --out profiles/crf_bench.txt]
"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, crf, kernels as K, teacher  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402

WINDOWS = ((3, 1, 5), (3, 2, 5), (5, 2, 5))
LDS_BUDGET = 80 * 1024                   # csrc/crf.hip: CRF_LDS_BUDGET, and its rule for the class chunk
GUIDE_LDS_B_PER_CLK_CU = 256


def alternating(legs, reps, warmup, inner):
    """{name: sorted HIP-event times per call in ms}: every round runs each leg once, in order, `inner` calls between two events."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: sorted(v) for k, v in ms.items()}


def step_shape(classes, radius, dilation, n, h, w):
    """(class chunk, LDS bytes read by the window loops, fused multiply-adds of the class updates) of one udaseg_crf_step."""
    th, tw = K.crf_tile(radius, dilation)
    nv, halo, k = (classes + 3) // 4, radius * dilation, 2 * radius + 1
    hp = (th + 2 * halo) * (tw + 2 * halo)
    fits = lambda cv: (16 * cv + 4) * hp + 1024 <= LDS_BUDGET      # noqa: E731
    cv = nv if nv <= 2 or fits(nv) else (3 if nv > 3 and fits(3) else 2)
    chunks = [min(cv, nv - c0) for c0 in range(0, nv, cv)]
    threads = -(-h // th) * -(-w // tw) * n * (th // 2) * tw
    lds = threads * sum(k * (k + 1) * (16 * c + 4) for c in chunks)
    fma = n * h * w * (k * k) * 4 * nv
    return cv, lds, fma


def torch_refine(scores_nchw, frames, p, probs=False):
    """The refinement as a torch composition, one image at a time: unfold of Q, of the frame and of the valid mask per sweep."""
    r, d, k = p["radius"], p["dilation"], 2 * p["radius"] + 1
    dev = scores_nchw.device
    sa = torch.from_numpy(crf.spatial_table(r, d, p["theta_alpha"])).to(dev).view(1, 1, k * k, 1)
    sg = torch.from_numpy(crf.spatial_table(r, d, p["theta_gamma"])).to(dev).view(1, 1, k * k, 1)
    centre = torch.ones(k * k, device=dev)
    centre[k * k // 2] = 0.0
    centre = centre.view(1, 1, k * k, 1)
    inv2b = float(crf.inv2b_of(p["theta_beta"]))
    outs = []
    for i in range(scores_nchw.shape[0]):
        s = scores_nchw[i:i + 1].float()
        _, c, h, w = s.shape
        logp = torch.log_softmax(s, 1) if not probs else torch.log(s / s.sum(1, keepdim=True))
        q = logp.exp()
        img = frames[i:i + 1].permute(0, 3, 1, 2).float()
        unf = lambda t: F.unfold(t, k, dilation=d, padding=r * d).view(1, t.shape[1], k * k, h * w)      # noqa: E731
        inside = unf(torch.ones(1, 1, h, w, device=dev)) * centre
        c2 = (unf(img) - img.view(1, 3, 1, h * w)).square().sum(1, keepdim=True)
        kern = (p["w_app"] * sa * torch.exp(-c2 * inv2b) + p["w_smooth"] * sg) * inside
        z = ((p["w_app"] * sa + p["w_smooth"] * sg) * inside).sum(2)
        for _ in range(p["iterations"]):
            m = p["strength"] * (kern * unf(q)).sum(2) / z
            q = torch.softmax(logp + m.view(1, c, h, w), 1)
        outs.append(q)
    return torch.cat(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--unfold-reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock the per-clock figures assume (MI355X peak: 2400)")
    ap.add_argument("--time-limit", type=int, default=540)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    signal.alarm(a.time_limit)
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, h, w, c = a.batch, a.size, a.size, a.classes
    ldq = (c + 3) // 4 * 4
    g = torch.Generator().manual_seed(3)
    sbuf = torch.zeros((n, h, w, ldq), dtype=torch.float32)
    sbuf[..., :c] = 2.0 * torch.randn((n, h, w, c), generator=g)
    sbuf = sbuf.to(dev)
    scores = sbuf.permute(0, 3, 1, 2)[:, :c]
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ramp = torch.stack([(xx // 3) % 256, (yy // 3) % 256, ((xx + yy) // 4) % 256], -1).to(torch.uint8)
    frames = {"smooth": ramp[None].repeat(n, 1, 1, 1).contiguous().to(dev),
              "random": torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).to(dev)}
    logp, q0, q1 = (torch.empty((n, h, w, ldq), dtype=torch.float32, device=dev) for _ in range(3))
    valid = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(sbuf)
    props = torch.cuda.get_device_properties(0)
    clock_hz, cus = a.clock_mhz * 1e6, props.multi_processor_count
    r4 = lambda v: round(v, 4)      # noqa: E731
    res = {}
    for fname, fr in frames.items():
        out = {}
        for r, d, t in WINDOWS:
            p = crf.check_params(radius=r, dilation=d, iterations=t)
            sa = torch.from_numpy(crf.spatial_table(r, d, p["theta_alpha"])).to(dev)
            sg = torch.from_numpy(crf.spatial_table(r, d, p["theta_gamma"])).to(dev)
            inv2b = float(crf.inv2b_of(p["theta_beta"]))
            K.crf_prepare(sbuf, ldq, c, False, n * h * w, logp, q0, ldq, valid)
            legs = {
                "prepare": lambda: K.crf_prepare(sbuf, ldq, c, False, n * h * w, logp, q0, ldq, valid),
                "step": lambda: K.crf_step(logp, q0, valid, fr, c, ldq, r, d, sa, sg, p["w_app"], p["w_smooth"], inv2b, p["strength"], q1),
                "refine": lambda: crf.refine(scores, fr, **p),
                "copy": lambda: copy_dst.copy_(sbuf),
            }
            ms = alternating(legs, a.reps, a.warmup, a.inner)
            med = {k: statistics.median(v) for k, v in ms.items()}
            cv, lds, fma = step_shape(c, r, d, n, h, w)
            row = {
                **{f"{k}_ms": r4(v) for k, v in med.items()},
                **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
                "step_over_copy": r4(med["step"] / med["copy"]), "refine_over_copy": r4(med["refine"] / med["copy"]),
                "tile": list(K.crf_tile(r, d)), "class_chunk_vectors": cv,
                "step_lds_read_bytes_per_clk_cu": r4(lds / (med["step"] * 1e-3 * clock_hz * cus)),
                "guide_lds_bytes_per_clk_cu": GUIDE_LDS_B_PER_CLK_CU,
                "step_fma_tflops": r4(2.0 * fma / (med["step"] * 1e-3) / 1e12),
            }
            if fname == "random":
                want = crf.refine(scores, fr, **p)
                got = torch_refine(scores, fr, p)
                diff = float((got - want).abs().max())
                assert diff < 1e-4, f"the torch composition differs from refine by {diff}"
                del got
                uf = alternating({"unfold": lambda: torch_refine(scores, fr, p)}, a.unfold_reps, 0, 1)["unfold"]
                row.update(unfold_ms=r4(statistics.median(uf)), unfold_over_refine=r4(statistics.median(uf) / med["refine"]),
                           unfold_max_difference=diff, unfold_chunk="one image at a time")
            out[f"r{r}d{d}t{t}"] = row
            print(f"{fname} radius {r} dilation {d} sweeps {t}: " + json.dumps(row), flush=True)
        res[fname] = out

    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=c).to(dev).eval()
    x = torch.randn(n, 3, h, w, generator=g).to(dev)

    def forward_leg():
        with torch.no_grad():
            net(x)

    online = teacher.OnlineLabeler(net, c)
    refined = crf.CrfLabeler(net, c)
    fr = frames["smooth"]
    tail = alternating({"forward_eval": forward_leg, "online_label": lambda: online.label(fr), "crf_label": lambda: refined.label(fr)},
                       a.reps, a.warmup, a.inner)
    tm = {k: statistics.median(v) for k, v in tail.items()}
    for out in res.values():
        for v in out.values():
            v["refine_over_forward"] = r4(v["refine_ms"] / tm["forward_eval"])
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    line = json.dumps({"scores": [n, c, h, w], "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "unfold_reps": a.unfold_reps,
                       "device": torch.cuda.get_device_name(0), "clock_mhz": clock_hz / 1e6, "cus": cus,
                       **{f"{k}_ms": r4(v) for k, v in tm.items()}, **{f"{k}_ms_min_max": [r4(tail[k][0]), r4(tail[k][-1])] for k in tail},
                       "crf_label_over_online_label": r4(tm["crf_label"] / tm["online_label"]), **res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_crf.py: CRF refinement at 8 x 23 x 512 x 512 fp32 logits and uint8 frames on 1 x MI355X "
                     "(HIP-event medians per call, legs alternating in one process, back-to-back calls; the unfold composition is "
                     "chunked one image at a time)\n")
            fh.write(f"# git HEAD {head}\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
