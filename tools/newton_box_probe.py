"""Measure the torque-limited Newton solve (BatchedNewtonSolver(tau_max=), gym_newton_run_box); bench.py is untouched.

  a  kernel time (timing kind 8, HIP events around every launch) of the box solver at tau_max = inf against the
     single-wavefront persistent solver without a limit (persistent=True, split_waves=False): same process, 4,096
     lanes, N = 501, 40 iterations, the two alternated (A B B A A B), three repeats each after one warm-up each.
  b  the floor: the 12 starts of tests/golden/lanes.npz at tau_max 18, 16, 14 and tol = 1e-4 (gamma_0 = 0.1): the
     iteration, status and max|sigma| at which each limited solve ends.
  c  the same starts planned at tau_max = 16 (tol = 5e-3) and without a limit (tol = 1e-4), each tracked with
     result.track_mpc(dx0=three starts per lane, tau_max=TorqueLimit(18.0)): unconverged QPs and QP iterations.

    python tools/newton_box_probe.py [--arms abc] [--out profiles/newton_box/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

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
    mk = {"plain": lambda: BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, persistent=True, split_waves=False,
                                               chunk=0, **KW).enable_timing(),
          "box": lambda: BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, tau_max=float("inf"), chunk=0,
                                             **KW).enable_timing()}
    solvers = {k: f() for k, f in mk.items()}
    res = {}
    for k, s in solvers.items():       # warm-up, and the bits
        res[k] = s.solve(x0, iters)
    same = all(torch.equal(getattr(res["plain"], f), getattr(res["box"], f)) for f in ("x", "u", "cost", "n_iter"))
    ms = {"plain": [], "box": []}
    for k in ("plain", "box", "box", "plain", "plain", "box"):
        s = solvers[k]
        s.reset_timing()
        s.solve(x0, iters)
        t, n = s.kernel_times()["run"]
        assert n == 1, n
        ms[k].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"lanes": B, "iterations": iters, "run_ms": ms, "median_ms": med,
            "box_over_plain": med["box"] / med["plain"], "same_bits": bool(same)}


def lanes_starts():
    return np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))["x0"]


def arm_b(eng, x_ref, u_ref):
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    x0 = lanes_starts()
    out = {}
    for tau in (18.0, 16.0, 14.0):
        s = BatchedNewtonSolver(eng, x_ref, u_ref, len(x0), tol=1e-4, tau_max=tau, reorder=False, **KW)
        r = s.solve(x0, 5000)
        out[str(tau)] = {"n_iter": r.n_iter.tolist(), "status": [_lib.STATUS_NAMES[int(v)] for v in r.status],
                         "smax": [float(v) for v in s.smax[:len(x0)]], "cost": r.cost.tolist(),
                         "clamped": (~r.K[:, :, 1].any(-1)).sum(1).tolist(),
                         "u_max": r.u[:, :, 1].abs().amax(1).tolist()}
    return out


def arm_c(eng, x_ref, u_ref):
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    from gymnast_optimalcontrol_amd.trajectory_tracking import TorqueLimit
    x0 = lanes_starts()
    dx0 = np.broadcast_to(np.array([[0.0] * 4, [0.1] * 4, [-0.05, 0.05, 0.1, -0.1]]), (len(x0), 3, 4)).copy()
    out = {}
    for name, kw in (("planned_tau16_tol5e-3", dict(tol=5e-3, tau_max=16.0)), ("unlimited_tol1e-4", dict(tol=1e-4))):
        r = BatchedNewtonSolver(eng, x_ref, u_ref, len(x0), **kw, **KW).solve(x0, 5000)
        t = r.track_mpc(dx0=dx0, tau_max=TorqueLimit(18.0))
        out[name] = {"plan_status": [_lib.STATUS_NAMES[int(v)] for v in r.status], "plan_n_iter": r.n_iter.tolist(),
                     "plan_u_max": r.u[:, :, 1].abs().amax(1).tolist(), "plan_cost": r.cost.tolist(),
                     "unconverged": t.unconverged.tolist(), "unconverged_total": int(t.unconverged.sum()),
                     "qp_iters_total": int(t.qp_iters.sum()), "qp_iters_max": int(t.qp_iters.max()),
                     "qp_iters_mean": float(t.qp_iters.double().mean()),
                     "err_final_max": float(t.err_final.max()), "track_u_max": float(t.u_max.max())}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arms", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_box", "probe.json"))
    args = ap.parse_args()
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine
    eng = AcrobotEngine()
    x_ref, u_ref = refs()
    out = {}
    for arm, fn in (("a", arm_a), ("b", arm_b), ("c", arm_c)):
        if arm in args.arms:
            out[arm] = fn(eng, x_ref, u_ref)
            print(arm, json.dumps(out[arm]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
