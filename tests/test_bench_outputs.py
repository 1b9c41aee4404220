"""bench.py's plain run and its --dump-outputs files: the plain line holds the headline and nothing that takes a run of
its own (those sit behind --full), and the dumped arrays are what the timed solve returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = ("parity", "cpu_baseline", "box", "strong_scaling_cfg4", "general_path", "cfg2", "stress",
             "cfg4_rank_share", "cfg1_drop_in", "mpc_cfg5")


def test_dump_sample_is_fixed_and_bounded():
    """The sampled lanes are the same in every run, sorted, distinct, lane 0 first; a small batch is kept whole; the
    headline dump stays under 64 MB."""
    import bench
    a, b = bench.dump_sample(262144), bench.dump_sample(262144)
    assert np.array_equal(a, b) and a[0] == 0 and len(a) == bench.DUMP_SAMPLE_LANES
    assert (np.diff(a) > 0).all() and a[-1] < 262144
    assert np.array_equal(bench.dump_sample(96), np.arange(96))
    assert np.array_equal(bench.dump_sample(bench.DUMP_SAMPLE_LANES), np.arange(bench.DUMP_SAMPLE_LANES))
    N, T = 501, 500
    per_lane = 8 * (4 * N + 2 * T + 8 * T + 2 * T)          # x, u, K, sigma
    assert len(a) * per_lane + 262144 * 8 * 5 + 8 * len(a) < 64e6


def test_write_dump_writes_float64(tmp_path):
    import bench
    out = tmp_path / "a" / "b"
    bench.write_dump(str(out), {"n_iter": np.arange(5, dtype=np.int32), "x": np.ones((2, 3), np.float32)[:, ::2]})
    n, x = np.load(out / "n_iter.npy"), np.load(out / "x.npy")
    assert n.dtype == x.dtype == np.float64 and np.array_equal(n, np.arange(5)) and x.shape == (2, 2)


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_solve(tmp_path):
    """A plain bench run (no --full) of 700 lanes: the line holds the headline fields with --steps timed steps and none
    of the --full records; the dump holds every lane's results and the sampled lanes' trajectories, equal to the C
    oracle's solve of the same inputs (counts and statuses exactly, trajectories to smoke()'s 1e-9)."""
    import bench
    from oracle import c_oracle
    B = 700                                              # above DUMP_SAMPLE_LANES: the sample is a proper subset
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps",
                        "2", "--warmup", "0", "--dump-outputs", str(tmp_path / "d")], env=env, capture_output=True,
                       text=True, timeout=200)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "Newton iterations/s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is True and out["steps"] == 2 and out["warmup"] == 0 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in out]
    d = {f[:-4]: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert set(d) == {"x", "u", "K", "sigma", "cost", "gamma", "n_iter", "status", "n_rollouts", "sample_lanes"}
    assert all(v.dtype == np.float64 for v in d.values()) and sum(v.nbytes for v in d.values()) < 64e6
    lanes = d["sample_lanes"].astype(int)
    assert np.array_equal(lanes, bench.dump_sample(B))
    n = len(lanes)
    assert d["x"].shape == (n, 501, 4) and d["u"].shape == (n, 500, 2) and d["K"].shape == (n, 500, 2, 4)
    assert d["sigma"].shape == (n, 500, 2) and all(d[k].shape == (B,) for k in ("cost", "gamma", "n_iter", "status"))
    # value x seconds = the lane-iterations of the two timed solves
    assert abs(out["value"] * out["ms_per_step"] * 2 / 1e3 - 2 * d["n_iter"].sum()) <= 1
    x_ref, u_ref = bench.load_refs()
    o = c_oracle.newton_solve(bench.make_x0(B), x_ref, u_ref, max_iters=5000, tol=1e-4, gamma_0=0.1)
    assert np.array_equal(d["n_iter"], o["n_iter"]) and np.array_equal(d["status"], o["status"])
    assert np.linalg.norm(d["x"] - o["x"][lanes]) / np.linalg.norm(o["x"][lanes]) < 1e-9
    assert np.max(np.abs(d["cost"] - o["cost"]) / np.abs(o["cost"])) < 1e-10
