#!/usr/bin/env python
"""Cost of the mean teacher's update on the r18 segmenter (23 classes, fp32) on one MI355X.

HIP-event medians over --reps rounds after --warmup rounds; the legs ALTERNATE inside every round, all in ONE process, so that the
ratios compare like with like.  Every leg runs --inner back-to-back calls between its two events and reports the time PER CALL (the
train step: one call per timing, it is long enough).
  * update_ms          teacher.MeanTeacher.update() with buffers="copy": udaseg_ema_flat over the parameter arena with the distance,
                       a device copy of the BatchNorm statistics and of the counters
  * kernel_ms          udaseg_ema_flat alone on the parameter arena, with dist2
  * kernel_nodist_ms   the same call without dist2
  * copy_ms            a device-to-device copy of the parameter arena: 8 bytes per element against the kernel's 12
  * torch_ms           torch._foreach_lerp_ over the two parameter lists plus copy_ of every buffer
  * adam_ms            one FusedAdam.step() (28 bytes per parameter)
  * step_ms            one 8 x 3 x 512 x 512 fp32 train step (forward, cross entropy, backward, FusedAdam), no teacher
Reported, not judged: the kernel as a multiple of the copy measured beside it (1.5 by bytes moved), update() as a fraction of the
torch composition and of the train step.  The back-to-back calls of a leg keep both arenas (115 MB for r18) in the 256 MiB Infinity
Cache: the kernel, copy and update legs are cache-resident times, and update over step is a lower bound on what the update costs
inside a step, where the arenas come from HBM.  One JSON line; --out also writes it to a file together with the git HEAD.

    python tools/bench_teacher.py [--reps 30 --warmup 5 --inner 20 --out profiles/teacher_bench.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from uda_aerial_semantic_segmentation_research_amd import _lib, kernels as K  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.optim import FusedAdam, _sumsq_scratch  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.teacher import MeanTeacher  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.train import SegmentationTrainer  # noqa: E402
from uda_aerial_semantic_segmentation_research_amd.unet import Unet  # noqa: E402


def alternating(legs, reps, warmup):
    """{name: sorted HIP-event times per call in ms}: every round runs each leg (fn, calls) once, in order."""
    for _ in range(warmup):
        for fn, _ in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, (fn, calls) in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return {k: sorted(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=23)
    ap.add_argument("--alpha", type=float, default=0.99)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", default=None, help="commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = Unet("resnet18", encoder_weights=None, in_channels=3, classes=a.classes).to(dev).train()
    trainer = SegmentationTrainer(net, dev)
    opt = FusedAdam(net.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, a.size, a.size, generator=g).to(dev)
    y = torch.randint(0, a.classes, (a.batch, a.size, a.size), generator=g).to(dev)
    trainer.train_step(x, y, opt)                                   # gradients and Adam state exist from here on
    mt = MeanTeacher(net, alpha=a.alpha, warmup=False)
    mt.update()
    assert mt.flat_launches == 1
    n = net._arena.numel()
    # operands of the bare legs: arenas of their own, so that no leg disturbs the teacher or the student
    t_arena, s_arena = mt.model._arena.clone(), net._arena.clone()
    copy_dst = torch.empty_like(s_arena)
    scratch, dist2 = _sumsq_scratch(dev), torch.zeros((), device=dev, dtype=torch.float64)
    torch_teacher = Unet("resnet18", encoder_weights=None, in_channels=3, classes=a.classes).to(dev).eval()
    torch_teacher.load_state_dict(net.state_dict())
    tp, sp = [p.detach() for p in torch_teacher.parameters()], [p.detach() for p in net.parameters()]
    tb, sb = list(torch_teacher.buffers()), list(net.buffers())
    w = 1.0 - a.alpha

    def torch_leg():
        with torch.no_grad():
            torch._foreach_lerp_(tp, sp, w)
            for d, s in zip(tb, sb):
                d.copy_(s)

    legs = {
        "update": (mt.update, a.inner),
        "kernel": (lambda: K.ema_flat(t_arena, s_arena, n, a.alpha, scratch, dist2), a.inner),
        "kernel_nodist": (lambda: K.ema_flat(t_arena, s_arena, n, a.alpha), a.inner),
        "copy": (lambda: copy_dst.copy_(s_arena), a.inner),
        "torch": (torch_leg, a.inner),
        "adam": (opt.step, a.inner),
        "step": (lambda: trainer.train_step(x, y, opt), 1),
    }
    ms = alternating(legs, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in ms.items()}
    assert mt.step == 1 + a.warmup + a.reps * a.inner and opt.flat_launches == 1 and torch.isfinite(mt.distance())
    moved = {"kernel": 12 * n, "kernel_nodist": 12 * n, "copy": 8 * n, "adam": 28 * n}
    head = a.head
    if head is None:
        try:
            head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    r4 = lambda v: round(v, 4)      # noqa: E731
    line = json.dumps({
        "model": "u-resnet18", "classes": a.classes, "arena_elements": n, "alpha": a.alpha, "step_batch": [a.batch, 3, a.size, a.size],
        "reps": a.reps, "warmup": a.warmup, "inner": a.inner, "device": torch.cuda.get_device_name(0),
        **{f"{k}_ms": r4(v) for k, v in med.items()},
        **{f"{k}_ms_min_max": [r4(ms[k][0]), r4(ms[k][-1])] for k in ms},
        **{f"{k}_TB_per_s": r4(b / (med[k] * 1e-3) / 1e12) for k, b in moved.items()},
        "kernel_over_copy": r4(med["kernel"] / med["copy"]), "kernel_nodist_over_copy": r4(med["kernel_nodist"] / med["copy"]),
        "kernel_over_adam": r4(med["kernel"] / med["adam"]),
        "update_over_torch": r4(med["update"] / med["torch"]), "update_over_step": r4(med["update"] / med["step"]),
    })
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/bench_teacher.py: the mean teacher's update on the r18 segmenter, fp32, on 1 x MI355X "
                     "(HIP-event medians per call, legs alternating in one process)\n")
            fh.write(f"# git HEAD {head}" + (" (--head: the commit the measured tree was based on; the tree itself may be ahead of it)"
                                                if a.head else "") + "\n")
            fh.write("# back-to-back calls keep the arenas in the Infinity Cache: the kernel, copy and update legs are cache-resident times\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
