"""bench.py's command line: a plain run measures the headline only (the other legs need --full), --steps sets the timed
steps, and --dump-outputs writes what the last timed step computed as float npy files of bounded size, sampled the same way on
every run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    bench = _bench()
    a = bench.parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parser().parse_args(["--full", "--no-also", "--dump-outputs", "d"])
    assert a.full and a.no_also and a.dump_outputs == "d"


def test_dump_sample_is_seeded_and_bounded():
    bench = _bench()
    small = torch.arange(10, dtype=torch.float32)
    assert np.array_equal(bench.dump_sample(small), small.numpy())
    counts = bench.dump_sample(torch.arange(6, dtype=torch.int64).reshape(2, 3))
    assert counts.dtype == np.float64 and counts.tolist() == [0, 1, 2, 3, 4, 5]
    big = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32).reshape(3, -1)
    s1, s2 = bench.dump_sample(big), bench.dump_sample(big.clone())
    assert s1.dtype == np.float32 and s1.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(s1, s2)                                  # same indices on every call
    assert np.all(np.diff(s1) >= 0) and s1[-1] > bench.DUMP_SAMPLE   # sorted, spread over the whole tensor


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    files = sorted(os.listdir(out_dir))
    assert files == ["logits.npy", "loss.npy"], files
    return json.loads(lines[0]), {f[:-4]: np.load(out_dir / f) for f in files}


@pytest.mark.gpu
def test_plain_run_with_dump_outputs(tmp_path):
    """Two plain runs with the same arguments: the result line of the headline alone, and the same logits and loss.  Without the
    restart of the last timed step, five chained Adam steps carry the atomic order of the weight gradients into the logits."""
    from uda_aerial_semantic_segmentation_research_amd import _lib
    _lib.require_gpu()
    out, arrays = _plain_run(tmp_path / "a")
    assert out["metric"] == "training images/sec at 512x512" and out["unit"] == "images/s" and out["higher_is_better"]
    assert out["dtype"] == "fp32" and out["steps"] == 3 and out["warmup"] == 2
    assert abs(out["value"] - 8 * 3 / (out["ms_per_step"] * 3e-3)) <= 0.01 * out["value"]
    assert out["sustained"] is None and out["roofline"] is None and "cpu_baseline" not in out and "also" not in out
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["logits"].size == 1 << 22
    assert abs(float(arrays["loss"]) - out["config"]["final_loss"]) <= 1e-5 * abs(out["config"]["final_loss"])
    _, again = _plain_run(tmp_path / "b")
    for name, a in arrays.items():
        err = float(np.abs(a.astype(np.float64) - again[name]).max())
        assert err <= 1e-6 * float(np.abs(a).max()), f"{name}: two runs differ by {err:.3e}"
