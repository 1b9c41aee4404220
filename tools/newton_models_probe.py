"""Measure the Newton solve on per-lane models (BatchedNewtonSolver(models=), gym_newton_run_models); bench.py is
untouched.

  a  the cost of per-thread coefficients: kernel time (timing kind 8, HIP events around every launch) of
     the models kernel on a table of the engine's own rows against the box kernel, both at tau_max = inf: same process,
     4,096 lanes, N = 501, 40 iterations, the two alternated (A B B A A B), three repeats each after one warm-up each
     (the shape and protocol of tools/newton_box_probe.py, arm a), after checking that the two solves' outputs are
     equal bit for bit.  The clocks, power and temperatures of every timed solve are sampled from sysfs
     (tools/box_state.py) and recorded beside its time.
  b  the use case: the 12 starts of tests/golden/lanes.npz, lane b on plant sample_plants(12, 1, rel=0.05)[b].
     nominal: planned on the engine's model, LQR designed on it, the closed loop simulated on the sampled plant
     (track_lqr(plant=...)).  per plant: planned, designed and simulated on the sampled plant (models=...).  Per lane
     the plan's status, iterations and cost and the closed loop's err_max, err_final and u_max, from three perturbed
     starts per lane.

    python tools/newton_models_probe.py [--arms ab] [--out profiles/newton_models/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KW = dict(beta=0.7, c=0.5, gamma_0=0.1, max_ls=20)
FIELDS = ("x", "u", "K", "sigma", "cost", "n_iter", "status", "n_rollouts", "gamma")


def refs():
    d = np.load(os.path.join(ROOT, "gymnast_optimalcontrol_amd", "data", "fully_actuated_trajectory.npz"))
    u_ref = np.zeros(d["u"].shape)
    u_ref[:, 1] = 2.0 * d["u"][:, 1]
    return d["x"], u_ref


def arm_a(eng, x_ref, u_ref):
    import torch
    import box_state
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    B, iters = 4096, 40
    x0 = np.zeros((B, 4))
    x0[1:, :2] = np.random.default_rng(3).uniform(-0.5, 0.5, (B - 1, 2))
    solvers = {k: BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, tau_max=float("inf"), chunk=0, **kw,
                                      **KW).enable_timing() for k, kw in (("box", {}), ("models", dict(models={})))}
    warm = {k: s.solve(x0, iters) for k, s in solvers.items()}                       # warm-up, and the equality check
    equal = {f: bool(torch.equal(getattr(warm["box"], f), getattr(warm["models"], f))) for f in FIELDS}
    assert all(equal.values()), equal
    sampler = box_state.Sampler(period=0.02).start()
    ms, box = {"box": [], "models": []}, []
    for k in ("box", "models", "models", "box", "box", "models"):
        s = solvers[k]
        s.reset_timing()
        sampler.mark()
        s.solve(x0, iters)
        t, n = s.kernel_times()["run"]
        assert n == 1, n
        ms[k].append(t)
        box.append({"arm": k, **sampler.window()})
    sampler.stop()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    return {"lanes": B, "iterations": iters, "lane_iterations": {k: r.lane_iterations for k, r in warm.items()},
            "outputs_equal": equal, "run_ms": ms, "median_ms": med, "spread": spread,
            "ms_per_iteration": {k: v / iters for k, v in med.items()}, "models_over_box": med["models"] / med["box"],
            "box_state": box}


def arm_b(eng, x_ref, u_ref):
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    from gymnast_optimalcontrol_amd.trajectory_tracking import sample_plants
    x0 = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))["x0"]
    B = len(x0)
    plants = sample_plants(B, 1, rel=0.05)
    dx0 = np.array([[0.0, 0.0, 0.0, 0.0], [0.05, -0.05, 0.0, 0.0], [-0.05, 0.05, 0.1, -0.1]])
    dx0 = np.broadcast_to(dx0, (B, 3, 4))
    out = {"plants": plants[:, 0].tolist()}
    for name, kw, track in (("nominal", {}, dict(plant=plants, models=None)),
                            ("per_plant", dict(models=plants), {})):
        s = BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, reorder=False, **kw, **KW)
        r = s.solve(x0, 5000)
        t = r.track_lqr(dx0=dx0, trajectories=False, gains=False, **track)
        out[name] = {"converged": int((r.status == _lib.CONVERGED).sum()), "n_iter": r.n_iter.tolist(),
                     "status": [_lib.STATUS_NAMES[int(v)] for v in r.status], "cost": r.cost.tolist(),
                     "smax": [float(v) for v in s.smax[:B]], "u_plan_max": r.u[:, :, 1].abs().amax(1).tolist(),
                     "err_max": t.err_max.tolist(), "err_final": t.err_final.tolist(), "u_max": t.u_max.tolist()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arms", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_models", "probe.json"))
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
