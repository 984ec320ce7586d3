"""N > 1 path on the REAL network: two data-parallel ranks (fresh child processes, both on device 0, gloo) run
``GradAllReducer`` attached to ``Unet`` -- tests/ddp_worker.py.  What would break silently on an 8-GPU box is asserted
here: a wrong "offsets >= o are final" report in ``Unet._backward_plan`` (a bucket all-reduced while its weight gradient
is still being written), buckets that do not tile the arena, ranks drifting apart after optimizer steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_real_unet(tmp_path):
    from uda_aerial_semantic_segmentation_research_amd import _lib
    _lib.require_gpu()
    world, port = 2, 29541
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [tmp_path / f"rank{r}.json" for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ddp_worker.py"), str(r), str(world), str(port),
                               str(outs[r])], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=420)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-4000:]}"
    for r in range(world):
        res = json.load(open(outs[r]))
        print(res)
        assert res["broadcast_equal"], "broadcast_parameters left the ranks with different weights"
        assert res["violations"] == [], f"a 'final' report preceded the launch of a gradient it covers: {res['violations']}"
        assert res["reports_descending"] and res["n_reports"] >= 15
        assert res["covers_once"] and res["launched_back_to_front"] and res["n_buckets"] >= 3
        assert res["local_vs_mean"] > 1e-2                      # the two shards really produce different gradients
        # observed 8.2e-7: the two backward passes differ by the order of the fp32 split-K atomics only
        assert res["avg_err"] <= 5e-6, f"all-reduced arena differs from the mean of the ranks' gradients by {res['avg_err']:.3e}"
        # stream order: weight gradients held back 50 ms on the side stream are still inside the averaged arena ...
        assert res["side_stream_in_use"]
        assert res["avg_err_delayed_side_stream"] <= 5e-6, \
            f"a bucket was all-reduced before its side-stream weight gradients landed: {res['avg_err_delayed_side_stream']:.3e}"
        # ... and the same run with the side stream's event dropped from Plan.ready_events() is caught (the test has teeth)
        assert res["control_err_without_side_event"] > 1e-2, res["control_err_without_side_event"]
        assert res["weights_equal_after_steps"] and res["weights_moved"]
        assert res["bn_buffers_local"]
        assert res["double_backward_raises"]


def test_bench_n_gt_1_control_flow_four_ranks_one_gpu():
    """bench.py's N > 1 path end to end as the driver launches it (torch.distributed.run, one JSON line from rank 0): four ranks
    sharing device 0 over gloo (UDASEG_BENCH_SHARE_GPU / UDASEG_BENCH_BACKEND: this pool hands out one-GPU boxes and allows six
    GPU processes; the real run is one rank per GPU over RCCL).  Asserts what the driver parses: n_gpus, global batch, weak
    scaling, a whole-job value, the roofline leg run by rank 0 while the others wait on the rendezvous store (host side), and that
    every rank exits cleanly."""
    from uda_aerial_semantic_segmentation_research_amd import _lib
    _lib.require_gpu()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", UDASEG_BENCH_SHARE_GPU="1", UDASEG_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1", "--full"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["config"]["global_batch"] == 32 and out["scaling"] == "weak" and out["steps"] == 2
    assert out["metric"] == "training images/sec at 512x512" and out["value"] > 0
    assert abs(out["value"] - 32 * 2 / (out["ms_per_step"] * 2e-3)) <= 0.01 * out["value"]      # whole-job images / max-over-ranks time
    assert out["roofline"] is not None and out["roofline"]["frac"] > 0
    assert out["config"]["host_cores_per_rank"] >= 1
    assert "cpu_baseline" not in out                       # N = 1 only
