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

--fallback N adds, in the same process and with the same protocol, the projected-Newton fallback's arms at
tau_max = 18: cap 32 with the fallback (against the tau18 arm above: the QPs that reach the cap are what that arm pays
for at horizon 50; at horizon 75 none does, so the pair shows what the switch costs a workload that never uses it),
cap 8 without and with it (profiles/mpc_box_fallback/).  The box state over that run (tools/box_state.py) goes into
the file as ``box``.
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
    ap.add_argument("--fallback", type=int, default=0, help="fallback_iters of the fallback arms (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mpc_box_fallback" if args.fallback else "mpc_box", "probe.json")
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    eng = tt._eng()
    trk = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
    x_ref, u_ref = eng.t(trk["x_opt"]), eng.t(trk["u_opt"])
    N = x_ref.shape[0]
    x_f, u_f = tt._final_state(eng)
    B = args.starts
    x0 = eng.t(trk["x_opt"][0] + np.random.default_rng(5).uniform(-0.1, 0.1, (B, 4)))
    res = {"device": torch.cuda.get_device_name(), "starts": B, "steps": N - 1, "reps": args.reps,
           "warmup": args.warmup, "unconstrained_rollout_us": UNCONSTRAINED_ROLLOUT_US,
           "fallback_iters": args.fallback, "arms": {}}
    box = None
    if args.fallback:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import box_state                  # this GPU's clocks and power over the whole probe (sysfs, read only)
        box = box_state.Sampler(torch.cuda.current_device(), 0.02).start()
        box.mark()
    arms = [("tau18", 18.0, 32, 0), ("tau18_one_sweep", 18.0, 1, 0), ("never_binds", 1e6, 32, 0)]
    if args.fallback:
        arms += [("tau18_fallback", 18.0, 32, args.fallback), ("tau18_cap8", 18.0, 8, 0),
                 ("tau18_cap8_fallback", 18.0, 8, args.fallback)]
    for T_pred in (50, 75):
        ws = eng.mpc_box_workspace(B, T_pred, N)
        K_all, QT, _ = eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, L=T_pred, nwin=N - 1)
        arm = {"workspace_MB": ws.numel() / 1e6,
               "gains_all": timed(lambda: eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, L=T_pred,
                                                            nwin=N - 1), args.warmup, args.reps)}
        for name, tau, cap, fb in arms:
            run = lambda: eng.mpc_box_rollout(x0, x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, QT, K_all, tau, cap,  # noqa: E731
                                              ws=ws, fallback_iters=fb)
            t = timed(run, args.warmup, args.reps)
            x, u, it, unconv = run()
            it = it.cpu().numpy()
            t["ratio_to_unconstrained_rollout"] = t["median_us"] / UNCONSTRAINED_ROLLOUT_US
            t["iteration_histogram"] = np.bincount(it.ravel(), minlength=2).tolist()
            t["mean_iterations_per_step"] = it.mean(axis=0).round(3).tolist()      # per control step, over lanes
            t["qps_with_more_than_one_sweep_pct"] = float(100.0 * (it > 1).mean())
            t["unconverged_qps"] = int(unconv.sum().item())
            t["qps_past_the_cap"] = int((it > cap).sum())            # the fallback ran (0 without it)
            t["max_iterations"] = int(it.max())
            t["max_abs_torque"] = float(u[..., 1].abs().max().item())
            t["finite"] = bool(torch.isfinite(x).all().item())
            arm[name] = t
            print(f"T_pred {T_pred} {name}: median {t['median_us']:.0f} us (min {t['min_us']:.0f}, max "
                  f"{t['max_us']:.0f}, spread {t['spread_pct']:.1f}%), x{t['ratio_to_unconstrained_rollout']:.1f} "
                  f"the unconstrained rollout; unconverged {t['unconverged_qps']}, past the cap "
                  f"{t['qps_past_the_cap']}; iterations {t['iteration_histogram']}", flush=True)
        print(f"T_pred {T_pred} gains_all: median {arm['gains_all']['median_us']:.0f} us", flush=True)
        res["arms"][f"T_pred_{T_pred}"] = arm
    if box is not None:
        res["box"] = box.window() if box.available else {"unmeasured": "no sysfs channels for this device"}
        box.stop()
        print("box", json.dumps(res["box"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
