"""Measure the Newton solve on per-lane cost weights (BatchedNewtonSolver(weights=), gym_newton_run_weights); bench.py
is untouched.

  a  the cost of per-thread weights: kernel time (timing kind 8, HIP events around every launch) of the weights kernel
     on a table of the engine's own rows against the box kernel, both at tau_max = inf: same process, 4,096 lanes,
     N = 501, 40 iterations, the two alternated (A B B A A B), three repeats each after one warm-up each (the shape and
     protocol of tools/newton_models_probe.py, arm a), after checking that the two solves' outputs are equal bit for
     bit.  The clocks, power and temperatures of every timed solve are sampled from sysfs (tools/box_state.py) and
     recorded beside its time.
  b  the use case, a study over weight sets in ONE batch: the 12 starts of tests/golden/lanes.npz under each of the
     sets of GRID (the defaults scaled: 4 Q, R[1] / 4, 0.1 Q_T, and 4 Q with R[1] / 4), 12 x len(GRID) lanes, lane
     12 g + i = start i under set g.  Per set: how many lanes converged, iterations, final cost, the plan's peak
     |tau2| and, from result.track_lqr on three perturbed starts per lane, err_max.

    python tools/newton_weights_probe.py [--arms ab] [--out profiles/newton_weights/probe.json]
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
# name -> factors on (Q, R[1], Q_T)
GRID = {"default": (1.0, 1.0, 1.0), "stiff": (4.0, 1.0, 1.0), "cheap": (1.0, 0.25, 1.0), "soft_end": (1.0, 1.0, 0.1),
        "stiff_cheap": (4.0, 0.25, 1.0)}


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
                                      **KW).enable_timing() for k, kw in (("box", {}), ("weights", dict(weights={})))}
    assert solvers["weights"]._run_fn == "gym_newton_run_weights" and solvers["box"]._run_fn == "gym_newton_run_box"
    warm = {k: s.solve(x0, iters) for k, s in solvers.items()}                       # warm-up, and the equality check
    equal = {f: bool(torch.equal(getattr(warm["box"], f), getattr(warm["weights"], f))) for f in FIELDS}
    assert all(equal.values()), equal
    sampler = box_state.Sampler(period=0.02).start()
    ms, box = {"box": [], "weights": []}, []
    for k in ("box", "weights", "weights", "box", "box", "weights"):
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
            "ms_per_iteration": {k: v / iters for k, v in med.items()}, "weights_over_box": med["weights"] / med["box"],
            "box_state": box}


def arm_b(eng, x_ref, u_ref):
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.engine import check_weights
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    starts = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))["x0"]
    n = len(starts)
    own = check_weights({}, 1, eng.weights)[0]
    rows = np.repeat(np.array([own * np.array([q] * 4 + [1.0, r1] + [qt] * 4) for q, r1, qt in GRID.values()]), n, axis=0)
    x0 = np.tile(starts, (len(GRID), 1))
    B = len(x0)
    dx0 = np.array([[0.0, 0.0, 0.0, 0.0], [0.05, -0.05, 0.0, 0.0], [-0.05, 0.05, 0.1, -0.1]])
    s = BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, reorder=False, weights=rows, **KW)
    r = s.solve(x0, 5000)
    t = r.track_lqr(dx0=np.broadcast_to(dx0, (B, 3, 4)), trajectories=False, gains=False)
    out = {"lanes": B, "seconds": r.seconds, "lane_iterations": r.lane_iterations, "sets": {}}
    for g, name in enumerate(GRID):
        ln = slice(g * n, (g + 1) * n)
        out["sets"][name] = {"factors_Q_R1_QT": list(GRID[name]), "weights": rows[g * n].tolist(),
                             "converged": int((r.status[ln] == _lib.CONVERGED).sum()),
                             "status": [_lib.STATUS_NAMES[int(v)] for v in r.status[ln]],
                             "n_iter": r.n_iter[ln].tolist(), "cost": r.cost[ln].tolist(),
                             "u_plan_max": r.u[ln, :, 1].abs().amax(1).tolist(),
                             "err_max": t.err_max[ln].tolist(), "err_final": t.err_final[ln].tolist()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arms", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_weights", "probe.json"))
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
