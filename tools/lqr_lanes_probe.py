"""Time the per-lane LQR tracker (measurement tool; bench.py is untouched).

(a) The cfg-3 shape -- 262,144 lanes, N = 501, the 12 reference-solved lanes of tests/golden/lanes.npz tiled -- with
    HIP events around each C-ABI call (workspace and outputs allocated once, outside the timed region), warm-up
    launches then timed repetitions; median, min, max and spread.  Arms:
      gains            gym_lqr_lanes_gains without K_out: the two tiled packs + k_lqr_lane_gains (three launches)
      gains_K          the same with the lane-major K_out (adds k_lqr_unpack_gains)
      rollout_P{1,8}   gym_lqr_lanes_rollout, summaries only
      rollout_P{1,8}_traj   the same with lane-major x_out / u_out (direct 16-byte non-temporal stores per step)
      backward         k_nt_backward of the Newton solver on a batch of the same shape (serial schedule, the solver's
                       own event timing), the yardstick with the same access pattern: 44,032 B per lane
    The split of ``gains`` into pack and sweep comes from a kernel trace of this script (--arms gains; see
    profiles/lqr_lanes/README.md), which one HIP-event pair around the call cannot give.
(b) 256 lanes: LQR_tracking_lanes against the only route without it, a Python loop of LQR_tracking_batch per lane
    (wall clock around a synchronised loop: the loop is bound by the host and its single-thread gains kernel).

(c) --plant, alone: gym_lqr_lanes_rollout_plant beside gym_lqr_lanes_rollout (plant_arm), written to
    profiles/plant_mismatch/lqr_lanes_probe.json.

The box state over the whole probe (tools/box_state.py) goes into the file as ``box``.

    python tools/lqr_lanes_probe.py [--lanes 262144] [--reps 7] [--warmup 2] [--arms all] [--plant]
                                    [--out profiles/lqr_lanes/probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8.0e12                     # MI355X HBM3E peak
BACKWARD_BYTES = 44032                # k_nt_backward per lane and sweep at N = 501


def stats(us):
    us = np.array(us)
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max()),
            "spread_pct": float(100.0 * (us.max() - us.min()) / np.median(us)), "reps_us": [float(v) for v in us]}


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
    return stats(out)


def timed_round(fns, warmup, reps):
    """Several calls timed in alternation (a, b, c, a, b, c, ...), so that a drift of the box meets all alike."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for fn, us in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
    return [stats(us) for us in out]


def plant_arm(eng, tt, lib, m, g, total, N, warmup, reps):
    """--plant: gym_lqr_lanes_rollout_plant beside gym_lqr_lanes_rollout on the same workspace, B, P, N: ``total``
    closed loops as total lanes x 1 start and as total / 64 lanes x 64 starts, summaries only and with trajectories.
    The new entry point runs twice: on a table whose every row is the design model (the same closed loops bit for
    bit: what per-thread coefficients cost) and on sample_plants' +-5 % on masses, inertias and friction, one plant
    per closed loop."""
    from gymnast_optimalcontrol_amd import _lib
    Q, R, QT = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_REG, tt.R_REG, tt.QT_REG))
    T = N - 1
    out = {}
    for B, P in ((total, 1), (max(total // 64, 1), 64)):
        idx = torch.arange(B, device=eng.device) % 12
        x_opt, u_opt = eng.t(g["x"])[idx].contiguous(), eng.t(g["u"])[idx].contiguous()
        ws = eng.lqr_lanes_workspace(B, N)
        _lib.check(lib.gym_lqr_lanes_gains(m, x_opt.data_ptr(), u_opt.data_ptr(), B, N, Q.ctypes.data, R.ctypes.data,
                                           QT.ctypes.data, ws.data_ptr(), ws.numel(), None, eng.stream), "gains")
        x0 = (x_opt[:, 0][:, None] + eng.t(np.random.default_rng(11).uniform(-0.1, 0.1, (12, P, 4)))[idx]).contiguous()
        tables = (eng.plant_table(1, 12, P)[idx].contiguous(),
                  eng.plant_table(tt.sample_plants(12, P, seed=0), 12, P)[idx].contiguous())
        sm = [torch.empty((3, B, P), dtype=torch.float64, device=eng.device) for _ in range(3)]
        del x_opt, u_opt
        for traj in (False, True):
            xo = uo = None
            if traj:
                xo = torch.empty((B, P, N, 4), dtype=torch.float64, device=eng.device)
                uo = torch.empty((B, P, T, 2), dtype=torch.float64, device=eng.device)

            def old():
                _lib.check(lib.gym_lqr_lanes_rollout(m, x0.data_ptr(), B, P, N, ws.data_ptr(), ws.numel(), _lib.ptr(xo),
                                                     _lib.ptr(uo), sm[0].data_ptr(), eng.stream), "rollout")

            def new(i):
                _lib.check(lib.gym_lqr_lanes_rollout_plant(m, tables[i].data_ptr(), x0.data_ptr(), B, P, N,
                                                           ws.data_ptr(), ws.numel(), _lib.ptr(xo), _lib.ptr(uo),
                                                           sm[1 + i].data_ptr(), eng.stream), "rollout_plant")
            a, b, c = timed_round([old, lambda: new(0), lambda: new(1)], warmup, reps)
            name = f"B{B}_P{P}" + ("_traj" if traj else "")
            out[name] = {"existing": a, "plant_same_model": b, "plant_sampled": c,
                         "ratio_same_model_over_existing": b["median_us"] / a["median_us"],
                         "ratio_sampled_over_existing": c["median_us"] / a["median_us"],
                         "same_model_summaries_equal_existing": bool(torch.equal(sm[0], sm[1])),
                         "finite": [bool(torch.isfinite(t).all().item()) for t in sm]}
            rs, rp = out[name]["ratio_same_model_over_existing"], out[name]["ratio_sampled_over_existing"]
            print(f"plant {name}: existing {a['median_us']:.0f} us (spread {a['spread_pct']:.1f}%), same model "
                  f"{b['median_us']:.0f} us (spread {b['spread_pct']:.1f}%, x{rs:.3f}), sampled {c['median_us']:.0f} us "
                  f"(spread {c['spread_pct']:.1f}%, x{rp:.3f})", flush=True)
            del xo, uo
        del ws, x0, tables, sm
        torch.cuda.empty_cache()
    return out


def with_rate(t, nbytes):
    t["bytes"] = int(nbytes)
    t["TBps"] = nbytes / (t["median_us"] * 1e-6) / 1e12
    t["frac_of_peak"] = t["TBps"] * 1e12 / PEAK_BPS
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arms", default="all", help="comma list of gains,rollout,backward,loop (default all)")
    ap.add_argument("--plant", action="store_true", help="only the mismatched-plant arm: the new rollout entry point "
                    "beside the existing one (written to profiles/plant_mismatch/lqr_lanes_probe.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", *(("plant_mismatch", "lqr_lanes_probe.json") if args.plant else
                                                    ("lqr_lanes", "probe.json")))
    arms = {"gains", "rollout", "backward", "loop"} if args.arms == "all" else set(args.arms.split(","))
    if args.plant:
        arms = {"plant"}
    from gymnast_optimalcontrol_amd import _lib, trajectory_tracking as tt
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    import ctypes as C
    eng = tt._eng()
    lib = eng.lib
    g = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))
    B = args.lanes
    N = g["x"].shape[1]
    T = N - 1
    idx = torch.arange(B, device=eng.device) % 12
    x_opt = eng.t(g["x"])[idx].contiguous()
    u_opt = eng.t(g["u"])[idx].contiguous()
    res = {"device": torch.cuda.get_device_name(), "lanes": B, "N": N, "reps": args.reps, "warmup": args.warmup,
           "peak_TBps": PEAK_BPS / 1e12, "arms": {}}
    Q, R, QT = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_REG, tt.R_REG, tt.QT_REG))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import box_state                      # this GPU's clocks, power and cap over the whole probe (sysfs, read only)
    box = box_state.Sampler(torch.cuda.current_device(), 0.02).start()
    box.mark()

    def finish():
        # the timed regions are milliseconds each, between allocations and host work: the window shows the state the
        # box was in (clock levels, the cap), not a steady state at the power cap as bench.py's seconds-long legs do
        res["box"] = box.window() if box.available else {"unmeasured": "no sysfs channels for this device"}
        box.stop()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", args.out)

    if "plant" in arms:
        del x_opt, u_opt
        res["arms"]["plant"] = plant_arm(eng, tt, lib, C.byref(eng.model), g, B, N, args.warmup, args.reps)
        return finish()
    ws = eng.lqr_lanes_workspace(B, N)
    res["workspace_GB"] = ws.numel() / 1e9
    m = C.byref(eng.model)

    def gains(K):
        _lib.check(lib.gym_lqr_lanes_gains(m, x_opt.data_ptr(), u_opt.data_ptr(), B, N, Q.ctypes.data, R.ctypes.data,
                                           QT.ctypes.data, ws.data_ptr(), ws.numel(), _lib.ptr(K), eng.stream), "gains")

    pack_bytes = 2 * 8 * (4 * N + 2 * T) * B
    sweep_bytes = (8 * (4 * N + 2 * T) + 8 * 4 * T) * B            # the issue's algorithmic figure: 40,032 B per lane
    if "gains" in arms:
        t = timed(lambda: gains(None), args.warmup, args.reps)
        res["arms"]["gains"] = with_rate(t, pack_bytes + sweep_bytes)
        t["sweep_bytes_per_lane"] = sweep_bytes // B
        t["sweep_bytes_streamed_per_lane"] = 8 * (4 * T + T) + 32 * T   # x_{N-1} and the tau1 plane are not read
        t["pack_bytes_per_lane"] = pack_bytes // B
        print(f"gains (pack x, pack u, sweep): median {t['median_us']:.0f} us, spread {t['spread_pct']:.1f}%, "
              f"{t['TBps']:.2f} TB/s over pack + sweep bytes", flush=True)
        if B * T * 64 <= 40e9:
            K = torch.empty((B, T, 2, 4), dtype=torch.float64, device=eng.device)
            t = timed(lambda: gains(K), args.warmup, args.reps)
            res["arms"]["gains_K"] = with_rate(t, pack_bytes + sweep_bytes + (32 + 64) * T * B)
            print(f"gains with K_out: median {t['median_us']:.0f} us, spread {t['spread_pct']:.1f}%", flush=True)
            del K
    else:
        gains(None)
    if "rollout" in arms:
        rng = np.random.default_rng(11)
        for P in (1, 8):
            x0 = (x_opt[:, 0][:, None] + eng.t(rng.uniform(-0.1, 0.1, (12, P, 4)))[idx]).contiguous()
            sm = torch.empty((3, B, P), dtype=torch.float64, device=eng.device)
            read = (32 * N + 16 * T + 32 * T + 32) * B * P
            for traj in (False, True):
                xo = uo = None
                if traj:
                    if B * P * (32 * N + 16 * T) > 80e9:
                        continue
                    xo = torch.empty((B, P, N, 4), dtype=torch.float64, device=eng.device)
                    uo = torch.empty((B, P, T, 2), dtype=torch.float64, device=eng.device)

                def run():
                    _lib.check(lib.gym_lqr_lanes_rollout(m, x0.data_ptr(), B, P, N, ws.data_ptr(), ws.numel(),
                                                         _lib.ptr(xo), _lib.ptr(uo), sm.data_ptr(), eng.stream), "rollout")
                t = timed(run, args.warmup, args.reps)
                nbytes = read + 24 * B * P + ((32 * N + 16 * T) * B * P if traj else 0)
                name = f"rollout_P{P}" + ("_traj" if traj else "")
                res["arms"][name] = with_rate(t, nbytes)
                t["hbm_bytes_if_L2_serves_repeats"] = int(nbytes - read * (P - 1) / P)
                t["finite"] = bool(torch.isfinite(sm).all().item())
                print(f"{name}: median {t['median_us']:.0f} us, spread {t['spread_pct']:.1f}%, {t['TBps']:.2f} TB/s "
                      f"requested", flush=True)
                del xo, uo
    if "backward" in arms:
        try:
            from gymnast_optimalcontrol_amd import trajectory_generation as tg
            x_ref, u_ref, _ = tg.get_fully_actuated_ref(os.path.join(ROOT, "gymnast_optimalcontrol_amd", "data",
                                                                      "fully_actuated_trajectory.npz"))
            sol = BatchedNewtonSolver(eng, x_ref, u_ref, B, tol=1e-4, gamma_0=0.1, pipeline=False, persistent=False,
                                      placement_trials=1)
            sol.enable_timing()
            x0s = torch.zeros((B, 4), dtype=torch.float64, device=eng.device)
            x0s[:, :2] = eng.t(np.random.default_rng(0).uniform(-0.5, 0.5, (4096, 2)))[torch.arange(B, device=eng.device) % 4096]
            sol.init(x0s)
            for _ in range(args.warmup):
                sol.iteration()
            sol.reset_timing()
            for _ in range(args.reps):
                sol.iteration()
            torch.cuda.synchronize()
            sol.collect_timing()
            ms, n = sol.kernel_times()["backward"]
            t = {"mean_us": 1e3 * ms / max(n, 1), "launches": n, "schedule": sol.schedule, "bytes": BACKWARD_BYTES * B}
            t["TBps"] = t["bytes"] / (t["mean_us"] * 1e-6) / 1e12
            t["frac_of_peak"] = t["TBps"] * 1e12 / PEAK_BPS
            res["arms"]["backward"] = t
            print(f"k_nt_backward: mean {t['mean_us']:.0f} us over {n} launches, {t['TBps']:.2f} TB/s", flush=True)
            del sol
        except Exception as e:   # the yardstick arm must not lose the other arms' figures
            res["arms"]["backward"] = {"unmeasured": repr(e)}
            print("backward arm failed:", repr(e), flush=True)
    if "loop" in arms:
        Bs = 256
        xs, us = x_opt[:Bs].contiguous(), u_opt[:Bs].contiguous()
        x0 = (xs[:, 0] + 0.05).contiguous()

        def lanes():
            return tt.LQR_tracking_lanes(xs, us, x0)

        def loop():
            return [tt.LQR_tracking_batch(xs[b], us[b], x0[b:b + 1]) for b in range(Bs)]

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
        print(f"B = 256: LQR_tracking_lanes {out['lanes']['median_us']:.0f} us, Python loop of LQR_tracking_batch "
              f"{out['python_loop']['median_us']:.0f} us, ratio {out['ratio_loop_over_lanes']:.0f}x", flush=True)
    finish()


if __name__ == "__main__":
    main()
