"""bench.py's multi-rank launch rehearsed on the one GPU of the box (VERDICT r3 "next" 7).

The driver's SCALE run launches ``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N``, one
process per GPU.  Here both ranks of a 2-process launch are put on device 0 (SO100_BENCH_DEVICE, a test hook),
and the run is checked against a single-process run of the same workload: the two shards' final states must
equal the ``env_offset`` slices of the one-process state bit for bit, and rank 0 alone prints one JSON line
with ``n_gpus: 2``."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run(cmd, env, timeout=240):
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def _check_plain_line_and_outputs(line, tmp_path, total, steps):
    """The one-process run is a plain run (no --full) with --dump-outputs: its line carries the headline fields and
    nulls for what only --full measures, and the dumped arrays are the last timed step's outputs: float32, one row
    per env, equal to the state the run ended in (a plain run steps no further after the timed steps)."""
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "env_steps/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - total) < 1e-6 * total     # value = envs / step time
    r = line["roofline"]
    assert line["cpu_baseline"] is None and r["fused_kernel_ms"] is None and r["contacts_per_env"] is None
    assert r["pool_requests_none_free"] is None and r["lib_source_hash"]
    state = np.load(tmp_path / "one" / "state_rank0.npz")
    names = {"obs": 15, "reward": None, "terminated": None, "truncated": None, "is_success": None,
             "final_observation": 15, "qpos": 13, "qvel": 12, "env_index": None}
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(n + ".npy" for n in names)
    out = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in names}
    for n, width in names.items():
        assert out[n].dtype == np.float32 and out[n].shape == ((total,) if width is None else (total, width)), n
    np.testing.assert_array_equal(out["env_index"], np.arange(total))
    for k in ("obs", "reward", "qpos", "qvel"):
        np.testing.assert_array_equal(out[k], state[k], err_msg=k)
    assert set(np.unique(out["terminated"])) <= {0.0, 1.0} and set(np.unique(out["truncated"])) <= {0.0, 1.0}


def test_full_run_adds_the_other_measurements():
    """--full: the same line with the per-kernel time, the pool counters, the contact sample and the CPU baseline
    filled in (a small shard, a short CPU sample)."""
    lines = _run([sys.executable, "bench.py", "--gpus", "1", "--full", "--total-envs", "512", "--steps", "4",
                  "--warmup", "2", "--contact-steps", "2", "--cpu-seconds", "0.2"],
                 dict(os.environ, OMP_NUM_THREADS="2"))
    assert len(lines) == 1
    line, r = lines[0], lines[0]["roofline"]
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert r["fused_kernel_ms"] > 0 and r["contacts_per_env"] >= 0 and r["contacts_dropped_per_env_step"] == 0
    assert r["pool_requests_none_free"] == 0 and r["pool_entries_per_xcd"] > 0


def test_two_rank_launch_matches_one_process(tmp_path):
    total, steps = 2048, 12
    common = ["--total-envs", str(total), "--steps", str(steps), "--warmup", "3", "--no-cpu-baseline",
              "--contact-steps", "2"]
    env = dict(os.environ, SO100_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    lines2 = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                   "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
                   *common, "--dump-state", str(tmp_path / "two")], env)
    lines1 = _run([sys.executable, "bench.py", "--gpus", "1", *common, "--dump-state", str(tmp_path / "one"),
                   "--dump-outputs", str(tmp_path / "out")], dict(os.environ, OMP_NUM_THREADS="2"))
    assert len(lines2) == 1 and len(lines1) == 1
    _check_plain_line_and_outputs(lines1[0], tmp_path, total, steps)
    l2 = lines2[0]
    assert l2["n_gpus"] == 2 and l2["config"]["envs_total"] == total and l2["config"]["envs_per_gpu"] == total // 2
    assert l2["value"] > 0 and l2["scaling"] == "strong" and l2["cpu_baseline"] is None
    one = np.load(tmp_path / "one" / "state_rank0.npz")
    for r in range(2):
        part = np.load(tmp_path / "two" / f"state_rank{r}.npz")
        o, c = int(part["offset"]), int(part["count"])
        assert (o, c) == (r * total // 2, total // 2)
        for k in ("qpos", "qvel", "obs", "reward", "episode"):
            np.testing.assert_array_equal(part[k], one[k][o:o + c], err_msg=f"rank {r} {k}")
