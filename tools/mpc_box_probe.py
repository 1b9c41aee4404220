"""Time the torque-limited MPC closed loop (measurement tool; bench.py is untouched).

The cfg 5 shape -- 8,192 starts x 500 control steps, horizon 50 and 75 -- at tau_max = 18 (the reference's limit:
stages 175-184 of the headline trajectory saturate) and at a limit that never binds (every QP is one linear forward
pass over the shared gain table).  Each arm: warm-up launches, then timed repetitions with HIP events around the
launch alone (workspace and outputs allocated once, outside the timed region); median, min, max and the spread are
reported, with the per-step iteration histogram and the ratio to the shipped unconstrained rollout
(k_track_rollout_pair, 363 us at cfg 5 in VERDICT round 6 -- not re-timed here).

    python tools/mpc_box_probe.py [--starts 8192] [--reps 7] [--warmup 2] [--out profiles/mpc_box/probe.json]

Arms per horizon: gains_all (k_mpc_gains<true>), rollout at tau_max = 18, rollout at tau_max = 18 with one sweep per
QP (max_qp_iters = 1: the forward pass and update only, every bound-violating QP clipped -- what the active-set
sweeps add is the difference to the full arm), rollout at tau_max = 1e6.
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

UNCONSTRAINED_ROLLOUT_US = 363.0      # k_track_rollout_pair at cfg 5


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out = np.array(out)
    return {"median_us": float(np.median(out)), "min_us": float(out.min()), "max_us": float(out.max()),
            "spread_pct": float(100.0 * (out.max() - out.min()) / np.median(out)), "reps_us": [float(v) for v in out]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_box", "probe.json"))
    args = ap.parse_args()
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    eng = tt._eng()
    trk = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
    x_ref, u_ref = eng.t(trk["x_opt"]), eng.t(trk["u_opt"])
    N = x_ref.shape[0]
    x_f, u_f = tt._final_state(eng)
    B = args.starts
    x0 = eng.t(trk["x_opt"][0] + np.random.default_rng(5).uniform(-0.1, 0.1, (B, 4)))
    res = {"device": torch.cuda.get_device_name(), "starts": B, "steps": N - 1, "reps": args.reps,
           "warmup": args.warmup, "unconstrained_rollout_us": UNCONSTRAINED_ROLLOUT_US, "arms": {}}
    for T_pred in (50, 75):
        ws = eng.mpc_box_workspace(B, T_pred, N)
        K_all, QT, _ = eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, L=T_pred, nwin=N - 1)
        arm = {"workspace_MB": ws.numel() / 1e6,
               "gains_all": timed(lambda: eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, L=T_pred,
                                                            nwin=N - 1), args.warmup, args.reps)}
        for name, tau, cap in (("tau18", 18.0, 32), ("tau18_one_sweep", 18.0, 1), ("never_binds", 1e6, 32)):
            run = lambda: eng.mpc_box_rollout(x0, x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, QT, K_all, tau, cap,  # noqa: E731
                                              ws=ws)
            t = timed(run, args.warmup, args.reps)
            x, u, it, unconv = run()
            it = it.cpu().numpy()
            t["ratio_to_unconstrained_rollout"] = t["median_us"] / UNCONSTRAINED_ROLLOUT_US
            t["iteration_histogram"] = np.bincount(it.ravel(), minlength=2).tolist()
            t["mean_iterations_per_step"] = it.mean(axis=0).round(3).tolist()      # per control step, over lanes
            t["qps_with_more_than_one_sweep_pct"] = float(100.0 * (it > 1).mean())
            t["unconverged_qps"] = int(unconv.sum().item())
            t["max_abs_torque"] = float(u[..., 1].abs().max().item())
            t["finite"] = bool(torch.isfinite(x).all().item())
            arm[name] = t
            print(f"T_pred {T_pred} {name}: median {t['median_us']:.0f} us (min {t['min_us']:.0f}, max "
                  f"{t['max_us']:.0f}, spread {t['spread_pct']:.1f}%), x{t['ratio_to_unconstrained_rollout']:.1f} "
                  f"the unconstrained rollout; iterations {t['iteration_histogram']}", flush=True)
        print(f"T_pred {T_pred} gains_all: median {arm['gains_all']['median_us']:.0f} us", flush=True)
        res["arms"][f"T_pred_{T_pred}"] = arm
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
