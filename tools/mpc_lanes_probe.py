"""Time the per-lane MPC tracker (measurement tool; bench.py is untouched).

(a) 262,144 lanes, N = 501, T_pred = 75 -- the 12 reference-solved lanes of tests/golden/lanes.npz tiled -- with HIP
    events around each C-ABI call (workspace and outputs allocated once, outside the timed region), warm-up launches
    then timed repetitions; median, min, max and spread.  Arms:
      gains        gym_mpc_lanes_gains without K_out: the two tiled packs + k_mpc_lane_gains
      gains_K      the same with the lane-major K_out (adds k_lqr_unpack_gains)
      rollout_P1   gym_lqr_lanes_rollout on that workspace, one start per lane, summaries only
    The kernel's own time comes from a kernel trace of this script (--arms gains; profiles/mpc_lanes/README.md), which
    one HIP-event pair around the call cannot give.  The arithmetic yardstick: the fp64 VALU instructions of one window
    step in the shipped ISA (--step-insts, counted with tools/loop_isa.py) x B (N-1) (T_pred-1) steps / the fp64 issue
    rate (one wave64 fp64 instruction per SIMD every 4 cycles: 16 lanes per cycle) at the shader clock the box state
    recorded.
(b) 256 lanes: MPC_tracking_lanes against the only route without it, a Python loop of mpc_gains per lane plus one-lane
    rollouts (solve_mpc_tracking_batch; wall clock around a synchronised loop).

    python tools/mpc_lanes_probe.py [--lanes 262144] [--reps 7] [--warmup 2] [--arms all] [--tag NAME]
                                    [--out profiles/mpc_lanes/probe.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lqr_lanes_probe import stats, timed  # noqa: E402

STEP_FP64_INSTS = 111      # v_fmac/fma/mul/add/rcp _f64 in k_mpc_lane_gains' window loop (tools/loop_isa.py)
SIMD_PER_CU = 4
FP64_LANES_PER_CLK = 16    # per SIMD: a wave64 fp64 instruction issues over 4 cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--t-pred", type=int, default=75)
    ap.add_argument("--arms", default="all", help="comma list of gains,rollout,loop (default all)")
    ap.add_argument("--step-insts", type=int, default=STEP_FP64_INSTS)
    ap.add_argument("--tag", default="shipped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_lanes", "probe.json"))
    args = ap.parse_args()
    arms = {"gains", "rollout", "loop"} if args.arms == "all" else set(args.arms.split(","))
    from gymnast_optimalcontrol_amd import _lib, trajectory_tracking as tt
    import box_state                      # this GPU's clocks, power and cap over the whole probe (sysfs, read only)
    eng = tt._eng()
    lib = eng.lib
    g = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))
    B, N, L = args.lanes, g["x"].shape[1], args.t_pred
    T = N - 1
    idx = torch.arange(B, device=eng.device) % 12
    x_opt = eng.t(g["x"])[idx].contiguous()
    u_opt = eng.t(g["u"])[idx].contiguous()
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(), "tag": args.tag, "library": os.path.basename(_lib.LIB_PATH),
           "lanes": B, "N": N, "T_pred": L, "reps": args.reps, "warmup": args.warmup,
           "compute_units": props.multi_processor_count, "arms": {}}
    Q, R = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_MPC, tt.R_MPC))
    QT = tt._mpc_terminal_weight(eng, Q, R)
    box = box_state.Sampler(torch.cuda.current_device(), 0.02).start()
    box.mark()
    ws = eng.lqr_lanes_workspace(B, N)
    res["workspace_GB"] = ws.numel() / 1e9
    m = C.byref(eng.model)

    def gains(K):
        _lib.check(lib.gym_mpc_lanes_gains(m, x_opt.data_ptr(), u_opt.data_ptr(), B, N, L, Q.ctypes.data,
                                           R.ctypes.data, QT.data_ptr(), ws.data_ptr(), ws.numel(), _lib.ptr(K),
                                           eng.stream), "gains")

    steps = B * T * (L - 1)
    if "gains" in arms:
        t = timed(lambda: gains(None), args.warmup, args.reps)
        t["window_steps"] = steps
        t["bytes_read_once_per_lane"] = 8 * (4 * N + 2 * T)
        res["arms"]["gains"] = t
        print(f"[{args.tag}] gains (pack x, pack u, window gains): median {t['median_us']:.0f} us, spread "
              f"{t['spread_pct']:.1f}%", flush=True)
        if B * T * 64 <= 40e9:
            K = torch.empty((B, T, 2, 4), dtype=torch.float64, device=eng.device)
            t = timed(lambda: gains(K), args.warmup, args.reps)
            res["arms"]["gains_K"] = t
            print(f"[{args.tag}] gains with K_out: median {t['median_us']:.0f} us, spread {t['spread_pct']:.1f}%",
                  flush=True)
            t["tiles_equal"] = bool(torch.equal(K, K[:12][idx]))   # every copy of a lane has that lane's bits
            del K
        if box.available:
            res["box_gains"] = box.window()                 # the clocks the gains arms ran at
            box.mark()
    else:
        gains(None)
    if "rollout" in arms:
        x0 = (x_opt[:, 0] + 0.05).reshape(B, 1, 4).contiguous()
        sm = torch.empty((3, B, 1), dtype=torch.float64, device=eng.device)

        def run():
            _lib.check(lib.gym_lqr_lanes_rollout(m, x0.data_ptr(), B, 1, N, ws.data_ptr(), ws.numel(), None, None,
                                                 sm.data_ptr(), eng.stream), "rollout")
        t = timed(run, args.warmup, args.reps)
        t["bytes"] = (32 * N + 16 * T + 32 * T + 32 + 24) * B
        t["TBps"] = t["bytes"] / (t["median_us"] * 1e-6) / 1e12
        t["finite"] = bool(torch.isfinite(sm).all().item())
        res["arms"]["rollout_P1"] = t
        print(f"[{args.tag}] rollout_P1 (summaries only): median {t['median_us']:.0f} us, spread "
              f"{t['spread_pct']:.1f}%, {t['TBps']:.2f} TB/s, finite {t['finite']}", flush=True)
    if "loop" in arms:
        Bs = 256
        xs, us = x_opt[:Bs].contiguous(), u_opt[:Bs].contiguous()
        x0 = (xs[:, 0] + 0.05).contiguous()

        def lanes():
            return tt.MPC_tracking_lanes(xs, us, x0, T_pred=L)

        def loop():
            return [tt.solve_mpc_tracking_batch(x0[b:b + 1], xs[b], us[b], L) for b in range(Bs)]

        out = {}
        for name, fn in (("lanes", lanes), ("python_loop", loop)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            us_ = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                us_.append((time.perf_counter() - t0) * 1e6)
            out[name] = stats(us_)
        out["lanes_n"] = Bs
        out["ratio_loop_over_lanes"] = out["python_loop"]["median_us"] / out["lanes"]["median_us"]
        res["arms"]["B256"] = out
        print(f"[{args.tag}] B = 256: MPC_tracking_lanes {out['lanes']['median_us']:.0f} us, Python loop of "
              f"solve_mpc_tracking_batch {out['python_loop']['median_us']:.0f} us, ratio "
              f"{out['ratio_loop_over_lanes']:.0f}x", flush=True)
    # the timed regions are tens of milliseconds each, between allocations and host work: the window shows the state
    # the box was in (clock levels, the cap), not a steady state at the power cap as bench.py's seconds-long legs do
    res["box"] = box.window() if box.available else {"unmeasured": "no sysfs channels for this device"}
    box.stop()
    # the arithmetic yardstick, at the shader clock the box state saw (its mean over the gains arms)
    sclk = None
    for key in ("freq_sclk_mhz", "dpm_sclk_mhz"):          # [mean, min, max] over the gains arms
        val = res.get("box_gains", {}).get(key)
        if sclk is None and isinstance(val, (list, tuple)) and val and val[0]:
            sclk = float(val[0])
    y = {"fp64_valu_per_step": args.step_insts, "window_steps": steps, "sclk_mhz": sclk}
    if sclk:
        rate = props.multi_processor_count * SIMD_PER_CU * FP64_LANES_PER_CLK * sclk * 1e6   # lane-instructions / s
        y["issue_bound_us"] = 1e6 * args.step_insts * steps / rate
        if "gains" in res["arms"]:
            y["call_over_issue_bound"] = res["arms"]["gains"]["median_us"] / y["issue_bound_us"]
        print(f"[{args.tag}] fp64 issue bound at {sclk:.0f} MHz: {y['issue_bound_us']:.0f} us", flush=True)
    res["yardstick"] = y
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
