"""Measure the Newton solve on the RK4-exact linearisation (BatchedNewtonSolver(linearization="rk4"),
gym_newton_run_rk4); bench.py is untouched.

  a  kernel time (timing kind 8, HIP events around every launch) of the rk4 kernel against the box kernel, both at
     tau_max = inf: same process, 4,096 lanes, N = 501, 40 iterations, the two alternated (A B B A A B), three
     repeats each after one warm-up each (the shape and protocol of tools/newton_box_probe.py, arm a).
  b  the floor: the 12 starts of tests/golden/lanes.npz at tau_max inf, 18, 16, 14 and tol 1e-4, 1e-5
     (gamma_0 = 0.1), for both linearisations: how many lanes converge, and per lane the iterations, the status,
     max|sigma| and the clamped stages at which the solve ends.

    python tools/newton_rk4lin_probe.py [--arms ab] [--out profiles/newton_rk4lin/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(beta=0.7, c=0.5, gamma_0=0.1, max_ls=20)


def refs():
    d = np.load(os.path.join(ROOT, "gymnast_optimalcontrol_amd", "data", "fully_actuated_trajectory.npz"))
    u_ref = np.zeros(d["u"].shape)
    u_ref[:, 1] = 2.0 * d["u"][:, 1]
    return d["x"], u_ref


def arm_a(eng, x_ref, u_ref):
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    B, iters = 4096, 40
    x0 = np.zeros((B, 4))
    x0[1:, :2] = np.random.default_rng(3).uniform(-0.5, 0.5, (B - 1, 2))
    solvers = {k: BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, tau_max=float("inf"), chunk=0, linearization=lin,
                                      **KW).enable_timing() for k, lin in (("box", "euler"), ("rk4", "rk4"))}
    lane_its = {k: s.solve(x0, iters).lane_iterations for k, s in solvers.items()}   # warm-up
    ms = {"box": [], "rk4": []}
    for k in ("box", "rk4", "rk4", "box", "box", "rk4"):
        s = solvers[k]
        s.reset_timing()
        s.solve(x0, iters)
        t, n = s.kernel_times()["run"]
        assert n == 1, n
        ms[k].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"lanes": B, "iterations": iters, "lane_iterations": lane_its, "run_ms": ms, "median_ms": med,
            "ms_per_iteration": {k: v / iters for k, v in med.items()}, "rk4_over_box": med["rk4"] / med["box"]}


def arm_b(eng, x_ref, u_ref):
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    x0 = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))["x0"]
    out = {}
    for lin in ("euler", "rk4"):
        for tol in (1e-4, 1e-5):
            for tau in (float("inf"), 18.0, 16.0, 14.0):
                s = BatchedNewtonSolver(eng, x_ref, u_ref, len(x0), tol=tol, tau_max=tau, reorder=False,
                                        linearization=lin, **KW)
                r = s.solve(x0, 5000)
                out[f"{lin} tol={tol:g} tau_max={tau:g}"] = {
                    "converged": int((r.status == _lib.CONVERGED).sum()), "n_iter": r.n_iter.tolist(),
                    "n_rollouts": r.n_rollouts.tolist(), "status": [_lib.STATUS_NAMES[int(v)] for v in r.status],
                    "smax": [float(v) for v in s.smax[:len(x0)]], "cost": r.cost.tolist(),
                    "clamped": (~r.K[:, :, 1].any(-1)).sum(1).tolist(), "u_max": r.u[:, :, 1].abs().amax(1).tolist()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arms", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_rk4lin", "probe.json"))
    args = ap.parse_args()
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine
    eng = AcrobotEngine()
    x_ref, u_ref = refs()
    out = {}
    for arm, fn in (("a", arm_a), ("b", arm_b)):
        if arm in args.arms:
            out[arm] = fn(eng, x_ref, u_ref)
            print(arm, json.dumps(out[arm]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
