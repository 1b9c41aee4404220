"""Measure closed-loop replanning (BatchedNewtonSolver.closed_loop, gym_newton_mpc_run); bench.py is untouched.

  a  the cost of a closed loop: kernel time (timing kind 8, HIP events around every launch) of one whole loop -- 500
     control steps, iters = 1, design plant, cold start -- beside the same lanes' gym_newton_run_box time per iteration:
     same process, 4,096 lanes, N = 501, tau_max = inf, the two alternated (A B B A A B), three repeats each after one
     warm-up each (the shape and protocol of tools/newton_models_probe.py, arm a).  The clocks, power and temperatures
     of every timed run are sampled from sysfs (tools/box_state.py) and recorded beside its time.
  b  the motivating case: the 12 solved lanes of tests/golden/lanes.npz from the three starts of
     tests/mpc_box_lanes_ref.starts on the README's two mismatched plants (m2, I2 + 10 %; m2 + 2 %, friction + 10 %) and
     on the design model: closed_loop(iters=1) and closed_loop(iters=0) warm-started from the lane's solved controls,
     beside LQR_tracking_lanes and MPC_tracking_lanes (T_pred 75, no limit) on the same plants.  Per (lane, start) the
     distance of the last state from the target x_ref[-1] (max abs; ClosedLoopResult.err_final's definition, applied
     to every controller), the largest torque, and for the replanning loops the rollouts and stop codes.

    python tools/newton_mpc_probe.py [--arms ab] [--out profiles/newton_mpc/probe.json]
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
PLANTS = {"design": {}, "heavy_m2_I2_+10pct": {"m2": 1.1, "I2": 0.363},
          "m2_+2pct_f_+10pct": {"m2": 1.02, "f1": 1.1, "f2": 1.1}}


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
    solvers = {k: BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, tau_max=float("inf"), chunk=0,
                                      **KW).enable_timing() for k in ("box", "loop")}

    def run(k):
        s = solvers[k]
        s.reset_timing()
        r = s.solve(x0, iters) if k == "box" else s.closed_loop(x0, iters=1)
        torch.cuda.synchronize()
        s.collect_timing()
        return r, s.kernel_times()["run"]

    warm = {k: run(k)[0] for k in solvers}                                          # warm-up
    sampler = box_state.Sampler(period=0.02).start()
    ms, box = {"box": [], "loop": []}, []
    for k in ("box", "loop", "loop", "box", "box", "loop"):
        sampler.mark()
        _, (t, n) = run(k)
        assert n == (1 if k == "box" else 2), n
        ms[k].append(t)
        box.append({"arm": k, **sampler.window()})
    sampler.stop()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    loop = warm["loop"]
    per_it = med["box"] / iters
    return {"lanes": B, "N": int(x_ref.shape[0]), "box_iterations": iters,
            "box_lane_iterations": warm["box"].lane_iterations, "run_ms": ms, "median_ms": med,
            "spread": {k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
            "box_ms_per_iteration": per_it, "loop_ms": med["loop"],
            "loop_in_box_iterations": med["loop"] / per_it,
            "loop_iterations_per_lane": [int(loop.iters.sum(1).min()), int(loop.iters.sum(1).max())],
            "loop_rollouts_per_lane": [int(loop.rollouts.sum(1).min()), int(loop.rollouts.sum(1).max())],
            "loop_steps_stopped": {"converged": int((loop.stop == 1).sum()), "ls_failed": int((loop.stop == 2).sum()),
                                   "of": int(loop.stop.numel())},
            "loop_finite": bool(torch.isfinite(loop.x).all()), "box_state": box}


def arm_b(eng, x_ref, u_ref):
    import time
    import torch
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    d = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))
    x_opt, u_opt = d["x"], d["u"]
    n = len(x_opt)
    s0 = x_opt[:, 0]
    x0 = np.stack([s0, s0 + 0.1, s0 + np.array([-0.05, 0.05, 0.1, -0.1])], axis=1)       # (12,3,4)
    goal = np.asarray(x_ref, float)[-1]
    flat, u_init = x0.reshape(-1, 4), np.repeat(u_opt, 3, axis=0)
    # the reference's own settings (newton_Algorithm's defaults), under which the lanes were solved
    solver = BatchedNewtonSolver(eng, x_ref, u_ref, 3 * n, tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0, max_ls=20)

    def goal_err(x_last):
        e = np.abs(np.asarray(x_last, float) - goal).max(-1)
        return [[float(v) if np.isfinite(v) else "nan" for v in row] for row in e.reshape(n, 3)]

    def summary(err):
        worst = [max((v for v in row if v != "nan"), default=-1.0) if "nan" not in row else "nan" for row in err]
        fin = [w for w in worst if w != "nan"]
        return {"err_final": err, "worst_per_lane": worst, "lanes_with_a_nonfinite_start": len(worst) - len(fin),
                "lanes_all_starts_within_0.1": sum(w <= 0.1 for w in fin),
                "lanes_all_starts_within_0.5": sum(w <= 0.5 for w in fin)}

    out = {"lanes": n, "starts": 3, "settings": dict(tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0, max_ls=20),
           "plan_err_final": goal_err(np.repeat(x_opt[:, -1], 3, axis=0)), "plants": {}}
    for name, plant in PLANTS.items():
        rec = {"plant": plant}
        for iters in (1, 0):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = solver.closed_loop(flat, u_init, iters=iters, plant=plant)
            torch.cuda.synchronize()
            rec[f"closed_loop_iters{iters}"] = {
                **summary(goal_err(r.x[:, -1].cpu().numpy())), "seconds": time.perf_counter() - t0,
                "u_max": float(torch.nan_to_num(r.u_max, nan=float("inf")).max()),
                "rollouts_per_loop": [int(r.rollouts.sum(1).min()), int(r.rollouts.sum(1).max())],
                "steps_converged": int((r.stop == 1).sum()), "steps_ls_failed": int((r.stop == 2).sum()),
                "steps": int(r.stop.numel())}
        lq = tt.LQR_tracking_lanes(x_opt, u_opt, x0, plant=plant or None, gains=False)
        rec["track_lqr"] = summary(goal_err(lq.x[:, :, -1].reshape(-1, 4).cpu().numpy()))
        mp = tt.MPC_tracking_lanes(x_opt, u_opt, x0, plant=plant or None, gains=False)
        rec["track_mpc75"] = summary(goal_err(mp.x[:, :, -1].reshape(-1, 4).cpu().numpy()))
        out["plants"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arms", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_mpc", "probe.json"))
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
