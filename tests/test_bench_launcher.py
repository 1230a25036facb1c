"""bench.py's multi-rank contract on the CPU: ``--gpus N`` without a launcher spawns N
rank processes itself, the JSON's n_gpus / world_size come from the process group, a mismatch with
WORLD_SIZE and an RCCL request for more GPUs than visible both fail loudly."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TINY = ["--device", "cpu", "--model", "raftstereo-realtime", "--per-gpu-batch", "1", "--height", "128",
        "--width", "160", "--iters", "1", "--steps", "2", "--warmup", "1"]


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], env=e, capture_output=True,
                          text=True, timeout=600)


def _json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks_gloo():
    r = _run(["--gpus", "2", "--full", *TINY], SA_DIST_BACKEND="gloo")  # --full: the all-gather alone is timed too
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json(r.stdout)
    assert rec["n_gpus"] == 2 and rec["world_size"] == 2
    assert rec["config"]["parallelism"] == "dp2" and rec["config"]["global_batch"] == 2
    assert sorted(x["rank"] for x in rec["ranks"]) == [0, 1]
    assert rec["allgather_ms"] is not None and rec["value"] > 0
    assert "oracle" in rec["engine"]


def test_single_rank_cpu():
    r = _run(["--gpus", "1", *TINY])
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json(r.stdout)
    assert rec["n_gpus"] == 1 and rec["config"]["parallelism"] == "dp1"


def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times its --steps steps and nothing else (no latency block, no all-gather timing), and
    --dump-outputs writes the last step's disparity and point cloud as float32 .npy, the same from run to run."""
    import numpy as np
    recs = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", *TINY, "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        recs.append(_json(r.stdout))
    rec = recs[0]
    assert rec["full"] is False and rec["latency_b1"] == {} and rec["allgather_ms"] is None
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 1000.0 / rec["ms_per_step"]) < 0.01 * rec["value"]  # 1 pair per step
    files = {k: v["file"] for k, v in rec["dumped_outputs"].items()}
    assert files == {"disparity": "disparity.npy", "cloud": "cloud.npy"}
    a = {p.name: np.load(p) for p in sorted((tmp_path / "a").iterdir())}
    b = {p.name: np.load(p) for p in sorted((tmp_path / "b").iterdir())}
    assert sorted(a) == sorted(b) == ["cloud.npy", "disparity.npy"]
    assert a["disparity.npy"].shape == (1, 128, 160) and a["cloud.npy"].shape == (1, 128, 160, 6)
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k], equal_nan=True)
    assert np.isfinite(a["disparity.npy"]).all() and a["disparity.npy"].std() > 0


def test_dump_outputs_samples_what_does_not_fit(tmp_path, monkeypatch):
    """An output larger than its share of the byte budget is written as a fixed, seeded sample of its rows."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    rng = np.random.default_rng(0)
    disp = rng.standard_normal((2, 5, 7)).astype(np.float32)      # 280 B: whole
    cloud = rng.standard_normal((2, 5, 7, 6)).astype(np.float64)  # 1680 B as float32: whole (share 1860)
    big = rng.standard_normal((3, 11, 13, 6)).astype(np.float32)  # 10296 B: sampled to what is left
    info = bench.dump_outputs(str(tmp_path), {"disparity": (disp, 1), "cloud": (cloud, 6), "big": (big, 6)})
    assert np.array_equal(np.load(tmp_path / "disparity.npy"), disp)
    got = np.load(tmp_path / "cloud.npy")
    assert got.dtype == np.float32 and np.array_equal(got, cloud.astype(np.float32))
    s = np.load(tmp_path / "big_sample.npy")
    keep = (4000 - 280 - 1680) // 24
    assert info["big"] == {"file": "big_sample.npy", "shape": [keep, 6], "sampled_rows": keep}
    idx = bench.dump_sample_index(3 * 11 * 13, keep)
    assert len(set(idx.tolist())) == keep and (np.diff(idx) > 0).all()
    assert np.array_equal(idx, bench.dump_sample_index(3 * 11 * 13, keep))
    assert np.array_equal(s, big.reshape(-1, 6)[idx])
    assert sum(np.load(p).nbytes for p in tmp_path.iterdir()) <= 4000
    # a 1-wide output (disparity) samples to a flat vector
    monkeypatch.setattr(bench, "DUMP_BUDGET", 400)
    info = bench.dump_outputs(str(tmp_path / "small"), {"disparity": (disp, 1), "cloud": (cloud, 6)})
    assert info["disparity"]["shape"] == [50] and info["cloud"]["shape"] == [8, 6]
    assert np.array_equal(np.load(tmp_path / "small" / "disparity_sample.npy"),
                          disp.reshape(-1)[bench.dump_sample_index(70, 50)])


def test_committed_plan_of_the_default_workload():
    """The default workload has a committed tactic plan in the native plan format (one entry per conv shape, gfx950
    keys, no duplicates); other workloads have none and are tuned."""
    import bench
    from stereoalgorithms_amd.utils.plan import read_plan
    path = bench.committed_plan_path(bench.parse([]))
    assert path and Path(path).parent == ROOT / "bench_plans"
    _, entries = read_plan(path)
    assert len(entries) > 20 and len({e.key for e in entries}) == len(entries)
    assert all(e.key.startswith("gfx950|") and e.cfg >= 0 and e.splitk >= 0 for e in entries)
    assert bench.committed_plan_path(bench.parse(["--iters", "4"])) is None
    assert bench.committed_plan_path(bench.parse(["--model", "raftstereo-realtime"])) is None
    assert bench.committed_plan_path(bench.parse(["--per-gpu-batch", "3"])) is None


@pytest.mark.gpu
def test_default_workload_runs_the_committed_plan(tmp_path):
    """bench.py pins the committed plan for its default workload: no shape is tuned (every conv shape of the frame is
    in the file), whatever the plan cache holds, so every run launches the same kernels."""
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], SA_PLAN_DIR=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json(r.stdout)
    assert rec["plan_source"]["committed"] == "raftstereo-sceneflow_b8_480x640_gfx950.plan"
    assert rec["plan_source"]["entries"] > 20 and rec["plan"]["tuned_shapes"] == 0


def test_more_gpus_than_visible_fails():
    r = _run(["--gpus", "9", "--steps", "1", "--warmup", "0"], SA_DIST_BACKEND="nccl")
    assert r.returncode != 0
    assert "GPU" in r.stderr


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "4", *TINY], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_scale_report_cpu(tmp_path):
    out = tmp_path / "scale.md"
    e = dict(os.environ, SA_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "scale_report.py"), "--sizes", "1,2", "--out", str(out),
                        *TINY], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = json.loads(out.with_suffix(".json").read_text())
    assert [x["n_gpus"] for x in rows] == [1, 2]
    assert "| 2 |" in out.read_text()
