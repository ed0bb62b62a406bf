"""bench.py on one GPU: contract line and parity of its own inputs.  (The two-rank rehearsal, with its result
checked against the global MSM, is tests/test_sharded_gpu.py.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("schedule", ["pipeline3", "pipeline", "streams"])
def test_bench_single_gpu_contract_and_parity(schedule):
    # bench.py --full asserts GPU bytes == C oracle bytes on its own inputs (cpu_baseline leg) in every schedule
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "1", "--logn", "16",
                          "--schedule", schedule, "--full"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["vs_baseline"] is None and d["config"]["schedule"] == schedule
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0
    # the level-1 kernel is timed twice: device clock inside the timed region, HIP events in a second pass
    k, e = d["roofline"]["kernel_ms"], d["roofline"]["kernel_ms_hip_events"]
    assert d["roofline"]["launches_timed"] == 6 and k["min"] <= k["median"] <= k["max"] and k["min"] > 0
    assert e["launches"] == 6 and e["min"] > 0


def test_bench_default_schedule_is_the_three_stage_pipeline():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--logn", "14",
                          "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["config"]["schedule"] == "pipeline3" and d["config"]["msms_in_flight"] == 3


def test_bench_plain_run_is_lean_and_dumps_the_oracle_point(tmp_path):
    # a plain run: no `roofline`, no CPU baseline; --dump-outputs writes the last timed step's result, the same from
    # run to run, and that result is the C oracle's point on bench.py's own seeded inputs
    import numpy as np
    import torch
    from octopuszk_amd import device as dev
    from oracle import coracle
    sys.path.insert(0, ROOT)
    import bench
    logn, dumps = 14, []
    for run in range(2):
        d_out = tmp_path / ("run%d" % run)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "1", "--logn",
                              str(logn), "--dump-outputs", str(d_out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Mscalar-mul/s"
        assert d["roofline"] is None and d["cpu_baseline"] is None
        got = np.load(d_out / "msm_result.npy")
        assert got.dtype == np.float32 and got.shape == (192,)
        assert got.astype(np.uint8).tobytes() == bytes.fromhex(d["config"]["result_hex"])
        dumps.append(got)
    assert np.array_equal(dumps[0], dumps[1])
    n = 1 << logn
    bases = dev.gen_g1_bases(n, seed=bench.base_seed(0))
    torch.cuda.synchronize()
    want = coracle.pippenger_g1(bytes(bases.cpu().numpy()), bytes(bench.rand_scalars(n, bench.scalar_seed(0))), n)
    assert dumps[0].astype(np.uint8).tobytes() == want
