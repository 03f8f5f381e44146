"""bench.py's multi-GPU launch logic, on the CPU: `--gpus N` must never degrade silently to one rank
(`--gpus 8` without WORLD_SIZE ran ONE rank and printed n_gpus: 1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(extra)
    return env


def test_launch_command_is_one_rank_per_gpu_on_localhost():
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.launch_command(["--gpus", "4", "--steps", "3"], 4, port=29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-5] == BENCH and cmd[-4:] == ["--gpus", "4", "--steps", "3"]


def test_more_gpus_than_the_node_has_fails_loudly():
    # (this container has no GPU; on a 1-GPU box the same path refuses --gpus 2)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 2
    assert "refusing to run fewer ranks" in r.stderr
    assert "n_gpus" not in r.stdout


def test_world_size_must_equal_gpus():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr and "n_gpus" not in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and "n_gpus" not in r.stdout


def test_eight_ranks_compose_and_refuse_on_fewer_devices():
    """`--gpus 8` (the driver's scaling run): the launch command is 8 ranks on 127.0.0.1, and a node with fewer than 8
    visible GPUs refuses (exit code 2, no JSON line) instead of printing a smaller job's number."""
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.launch_command(["--gpus", "8", "--steps", "20", "--warmup", "5"], 8, port=29533)
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29533"
    assert cmd[-7] == BENCH and cmd[-6:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 2
    assert "refusing to run fewer ranks" in r.stderr and "n_gpus" not in r.stdout


def test_dump_outputs_writes_float32_and_samples_large_arrays_at_fixed_positions(tmp_path):
    """--dump-outputs: small arrays whole, larger ones as the same seeded sample of positions on every call."""
    sys.path.insert(0, ROOT)
    import bench
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4).to(torch.bfloat16)
    big = torch.randn(bench.DUMP_MAX_ELEMS + 1000, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.float().numpy())
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,) and np.array_equal(a, b)
    assert np.isin(a, big.float().numpy()).all()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run: the headline line with exactly --steps timed steps and none of --full's figures; --dump-outputs
    writes the last step's out and gradients (grad_value, the one array above the size cap, as a sample)."""
    sys.path.insert(0, ROOT)
    import bench
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--nq", "256",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res
    assert res["steps"] == 3 and res["dtype"] == "bf16" and res["ms_per_step"] > 0
    assert not {"roofline", "kernels_mean_us", "fp16", "dropin_unchanged_ms", "cpu_baseline", "exchange"} & set(res)
    want = {"out": (8, 256, 1024), "grad_value": (bench.DUMP_MAX_ELEMS,), "grad_loc": (8, 256, 8, 4, 4, 2),
            "grad_attn": (8, 256, 8, 4, 4)}
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(n + ".npy" for n in want)
    for name, shape in want.items():
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), name
    assert 0.0 <= np.load(tmp_path / "out.npy").min() and np.load(tmp_path / "out.npy").max() <= 1.01
