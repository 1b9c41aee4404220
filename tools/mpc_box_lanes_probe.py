"""Time the per-lane torque-limited MPC closed loop, gym_mpc_box_lanes_rollout (measurement tool; bench.py is untouched).

HIP events around the C-ABI call alone (inputs, workspace and outputs allocated once, outside the timed region), 2
warm-up and 7 timed repetitions per arm unless stated; median, min, max and the spread are reported.

  a  8,192 lanes x 1 start, every lane the headline trajectory (tests/golden/tracking.npz): the cfg 5 shape, arm by arm
     with tools/mpc_box_probe.py (limit never binds / tau_max 18, horizon 75 and 50), and gym_mpc_box_rollout (the
     shared-reference kernel) on the same starts in the same process.  One start per wavefront.
  b  the same 8,192 closed loops as 128 lanes x 64 starts: full wavefronts.  a / b is the cost of the idle threads.
  c  256 distinct lanes (tests/golden/lanes.npz tiled) x 1 start at tau_max 18, horizon 75, against what the call
     replaces: a Python loop of solve_mpc_tracking_box_batch, one call per lane (wall clock around the synchronised
     loop, one pass after two warm-up calls; the new call by wall clock too).
  d  262,144 lanes x 1 start, summaries only, tau_max 18, horizon 75: time (1 warm-up, 3 repetitions) and workspace
     bytes; the ratio to the unconstrained per-lane path's 43 ms is the price of the limit.  A workspace
     above half the free device memory goes through the engine's lane chunks instead of one call.
  f  the projected-Newton fallback (gym_mpc_box_lanes_rollout_fallback, --fallback iterations) on b's shape, 128 lanes
     x 64 starts at tau_max 18, each against the fallback-off kernel in the same process: horizon 50 at cap 32 and
     cap 8 (QPs reach the cap and the off arm pays for them), horizon 75 at cap 32 (none does: what the switch costs
     a workload that never uses it).  Not in the default arms; written to profiles/mpc_box_fallback/.
  p  --plant, alone: gym_mpc_box_lanes_rollout_plant beside the existing entry points on b's shape at tau_max 18,
     horizon 75, without and with the fallback; written to profiles/plant_mismatch/.

    python tools/mpc_box_lanes_probe.py [--arms abcd] [--reps 7] [--warmup 2] [--big-lanes 262144] [--plant]
                                        [--out profiles/mpc_box_lanes/probe.json]
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

UNCONSTRAINED_LANES_MS = 43.0        # gym_mpc_lanes_gains + gym_lqr_lanes_rollout at 262,144 lanes
F64 = torch.float64


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


class Call:
    """One gym_mpc_box_lanes_rollout call on preallocated buffers: x_opt (B,N,4), u_opt (B,N-1,2), x0 (B,P,4)."""

    def __init__(self, eng, tt, x_opt, u_opt, x0, L, tau, cap=32, trajectories=True, fb=0, plant=None):
        from gymnast_optimalcontrol_amd import _lib
        self.eng, self._lib, self.fb = eng, _lib, fb
        self.plant = plant                # a plant_table (B,P,8): gym_mpc_box_lanes_rollout_plant, fb = 0 included
        self.x_opt, self.u_opt, self.x0 = eng.t(x_opt), eng.t(u_opt), eng.t(x0)
        self.B, self.N, self.P, self.L, self.tau, self.cap = x_opt.shape[0], x_opt.shape[1], x0.shape[1], L, tau, cap
        self.Q, self.R = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_MPC, tt.R_MPC))
        self.QT = tt._mpc_terminal_weight(eng, tt.Q_MPC, tt.R_MPC)
        self.ws_bytes = eng.mpc_box_lanes_workspace(self.B, self.P, L)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=eng.device)
        B, P, N, dev = self.B, self.P, self.N, eng.device
        self.x = torch.empty((B, P, N, 4), dtype=F64, device=dev) if trajectories else None
        self.u = torch.empty((B, P, N - 1, 2), dtype=F64, device=dev) if trajectories else None
        self.it = torch.empty((B, P, N - 1), dtype=torch.int32, device=dev) if trajectories else None
        self.sm = torch.empty((3, B, P), dtype=F64, device=dev)
        self.un = torch.empty((B, P), dtype=torch.int32, device=dev)

    def __call__(self):
        e, p = self.eng, self._lib.ptr
        head = (C.byref(e.model), self.x_opt.data_ptr(), self.u_opt.data_ptr(), self.x0.data_ptr(), self.B, self.P,
                self.N, self.L, self.Q.ctypes.data, self.R.ctypes.data, self.QT.data_ptr(), float(self.tau), self.cap)
        tail = (self.ws.data_ptr(), self.ws_bytes, p(self.x), p(self.u), self.sm.data_ptr(), p(self.it),
                self.un.data_ptr(), e.stream)
        if self.plant is not None:
            self._lib.check(e.lib.gym_mpc_box_lanes_rollout_plant(head[0], self.plant.data_ptr(), *head[1:], self.fb,
                                                                  *tail), "gym_mpc_box_lanes_rollout_plant")
        elif self.fb:
            self._lib.check(e.lib.gym_mpc_box_lanes_rollout_fallback(*head, self.fb, *tail),
                            "gym_mpc_box_lanes_rollout_fallback")
        else:
            self._lib.check(e.lib.gym_mpc_box_lanes_rollout(*head, *tail), "gym_mpc_box_lanes_rollout")

    def facts(self):
        out = {"workspace_MB": self.ws_bytes / 1e6, "unconverged_qps": int(self.un.sum().item()),
               "max_abs_torque": float(self.sm[2].max().item()), "finite": bool(torch.isfinite(self.sm).all().item())}
        if self.it is not None:
            it = self.it.cpu().numpy()
            out["iteration_histogram"] = np.bincount(it.ravel(), minlength=2).tolist()
            out["qps_with_more_than_one_sweep_pct"] = float(100.0 * (it > 1).mean())
            out["qps_past_the_cap"] = int((it > self.cap).sum())     # the fallback ran (0 without it)
            out["max_iterations"] = int(it.max())
        return out


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
    res = []
    for us in out:
        us = np.array(us)
        res.append({"median_us": float(np.median(us)), "min_us": float(us.min()), "max_us": float(us.max()),
                    "spread_pct": float(100.0 * (us.max() - us.min()) / np.median(us)),
                    "reps_us": [float(v) for v in us]})
    return res


def line(name, t):
    print(f"{name}: median {t['median_us'] / 1e3:.2f} ms (min {t['min_us'] / 1e3:.2f}, max {t['max_us'] / 1e3:.2f}, "
          f"spread {t['spread_pct']:.1f}%)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="abcd")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-lanes", type=int, default=262144)
    ap.add_argument("--fallback", type=int, default=128, help="fallback_iters of arm f")
    ap.add_argument("--plant", action="store_true", help="only the mismatched-plant arm: "
                    "gym_mpc_box_lanes_rollout_plant beside the existing entry points on arm b's shape (written to "
                    "profiles/plant_mismatch/mpc_box_lanes_probe.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.plant:
        args.arms = "p"
        args.out = args.out or os.path.join(ROOT, "profiles", "plant_mismatch", "mpc_box_lanes_probe.json")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mpc_box_fallback" if args.arms == "f" else "mpc_box_lanes",
                                "probe.json" if args.arms != "f" else "lanes_probe.json")
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    eng = tt._eng()
    trk = np.load(os.path.join(ROOT, "tests", "golden", "tracking.npz"))
    lanes = np.load(os.path.join(ROOT, "tests", "golden", "lanes.npz"))
    xr, ur = trk["x_opt"], trk["u_opt"][:trk["x_opt"].shape[0] - 1]
    N = xr.shape[0]
    res = {"device": torch.cuda.get_device_name(), "steps": N - 1, "reps": args.reps, "warmup": args.warmup, "arms": {}}
    starts = eng.t(xr[0] + np.random.default_rng(5).uniform(-0.1, 0.1, (8192, 4)))   # tools/mpc_box_probe.py's starts

    if "a" in args.arms or "b" in args.arms:
        x_ref, u_ref = eng.t(xr), eng.t(ur)
        x_f, u_f = tt._final_state(eng)
        for T_pred in (75, 50):
            K_all, QT, _ = eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, L=T_pred, nwin=N - 1)
            ws = eng.mpc_box_workspace(8192, T_pred, N)
            for name, tau in (("never_binds", 1e6), ("tau18", 18.0)):
                arm = {}
                shared = timed(lambda: eng.mpc_box_rollout(starts, x_ref, u_ref, x_f, u_f, tt.Q_MPC, tt.R_MPC, QT,
                                                           K_all, tau, 32, ws=ws), args.warmup, args.reps)
                arm["shared_reference_kernel"] = shared
                line(f"T_pred {T_pred} {name} gym_mpc_box_rollout 8192 starts", shared)
                for key, B, P in (("a_8192x1", 8192, 1), ("b_128x64", 128, 64)):
                    if key[0] not in args.arms:
                        continue
                    call = Call(eng, tt, x_ref[None].expand(B, N, 4), u_ref[None].expand(B, N - 1, 2),
                                starts.reshape(B, P, 4), T_pred, tau)
                    t = timed(call, args.warmup, args.reps)
                    t.update(call.facts())
                    t["ratio_to_shared_reference_kernel"] = t["median_us"] / shared["median_us"]
                    arm[key] = t
                    line(f"T_pred {T_pred} {name} {key} (x{t['ratio_to_shared_reference_kernel']:.2f} the shared "
                         f"kernel, iterations {t['iteration_histogram']})", t)
                    del call
                if "a_8192x1" in arm and "b_128x64" in arm:
                    arm["a_over_b"] = arm["a_8192x1"]["median_us"] / arm["b_128x64"]["median_us"]
                    print(f"T_pred {T_pred} {name}: a / b = {arm['a_over_b']:.2f}", flush=True)
                res["arms"][f"T_pred_{T_pred}_{name}"] = arm
            del ws, K_all
        torch.cuda.empty_cache()

    if "f" in args.arms:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import box_state                  # this GPU's clocks and power over arm f (sysfs, read only)
        box = box_state.Sampler(torch.cuda.current_device(), 0.02).start()
        box.mark()
        x_ref, u_ref = eng.t(xr), eng.t(ur)
        B, P = 128, 64
        for T_pred, cap in ((50, 32), (50, 8), (75, 32)):
            arm = {}
            for key, fb in (("off", 0), ("fallback", args.fallback)):
                call = Call(eng, tt, x_ref[None].expand(B, N, 4), u_ref[None].expand(B, N - 1, 2),
                            starts.reshape(B, P, 4), T_pred, 18.0, cap=cap, fb=fb)
                t = timed(call, args.warmup, args.reps)
                t.update(call.facts())
                arm[key] = t
                line(f"f T_pred {T_pred} cap {cap} {key} (unconverged {t['unconverged_qps']}, past the cap "
                     f"{t['qps_past_the_cap']}, iterations <= {t['max_iterations']})", t)
                del call
            arm["fallback_over_off"] = arm["fallback"]["median_us"] / arm["off"]["median_us"]
            res["arms"][f"f_T_pred_{T_pred}_cap_{cap}"] = arm
        res["box_arm_f"] = box.window() if box.available else {"unmeasured": "no sysfs channels for this device"}
        box.stop()
        print("box", json.dumps(res["box_arm_f"]), flush=True)
        torch.cuda.empty_cache()

    if "p" in args.arms:
        # arm b's shape, 128 lanes x 64 starts of the headline trajectory at tau_max 18, horizon 75, cap 32, without and
        # with the fallback: the existing entry point, the new one on a table whose every row is the design model (the
        # same closed loops bit for bit, so the ratio is what per-thread coefficients cost), and the new one on
        # sample_plants' +-5 % (other closed loops with other QPs: a wavefront runs the sweeps of its slowest start),
        # alternating in the same process on the same inputs and sizes
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import box_state                  # this GPU's clocks and power over the arm (sysfs, read only)
        box = box_state.Sampler(torch.cuda.current_device(), 0.02).start()
        box.mark()
        x_ref, u_ref = eng.t(xr), eng.t(ur)
        B, P = 128, 64
        same, table = eng.plant_table(1, B, P), eng.plant_table(tt.sample_plants(B, P, seed=0), B, P)
        for key, fb in (("active_set", 0), ("fallback", args.fallback)):
            mk = lambda plant: Call(eng, tt, x_ref[None].expand(B, N, 4), u_ref[None].expand(B, N - 1, 2),   # noqa: E731
                                    starts.reshape(B, P, 4), 75, 18.0, fb=fb, plant=plant)
            calls = {"existing": mk(None), "plant_same_model": mk(same), "plant_sampled": mk(table)}
            arm = dict(zip(calls, timed_round(list(calls.values()), args.warmup, args.reps)))
            for name, call in calls.items():
                arm[name].update(call.facts())
                arm[name]["ratio_to_existing"] = arm[name]["median_us"] / arm["existing"]["median_us"]
                line(f"p {key} {name} (x{arm[name]['ratio_to_existing']:.3f}, unconverged "
                     f"{arm[name]['unconverged_qps']}, iterations <= {arm[name]['max_iterations']})", arm[name])
            arm["same_model_outputs_equal_existing"] = all(
                torch.equal(getattr(calls["existing"], f), getattr(calls["plant_same_model"], f))
                for f in ("x", "u", "it", "sm", "un"))
            res["arms"][f"p_128x64_{key}"] = arm
            del calls
        res["box_arm_p"] = box.window() if box.available else {"unmeasured": "no sysfs channels for this device"}
        box.stop()
        print("box", json.dumps(res["box_arm_p"]), flush=True)
        torch.cuda.empty_cache()

    if "c" in args.arms:
        B = 256
        idx = np.arange(B) % lanes["x"].shape[0]
        x, u = lanes["x"][idx], lanes["u"][idx]
        x0 = x[:, 0] + 0.02
        xd, ud, x0d = eng.t(x), eng.t(u), eng.t(x0)
        for b in range(2):
            tt.solve_mpc_tracking_box_batch(x0d[b:b + 1], xd[b], ud[b], 18.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        unconv = 0
        for b in range(B):
            r = tt.solve_mpc_tracking_box_batch(x0d[b:b + 1], xd[b], ud[b], 18.0)
            unconv += r.unconverged
        torch.cuda.synchronize()
        loop_s = time.perf_counter() - t0
        run = lambda: tt.MPC_tracking_lanes(xd, ud, x0d, tau_max=18.0)   # noqa: E731
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = run()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        call = Call(eng, tt, x, u, x0[:, None], 75, 18.0)
        t = timed(call, args.warmup, args.reps)
        t.update(call.facts())
        t.update({"lanes": B, "per_lane_loop_wall_s": loop_s, "per_lane_loop_unconverged_qps": int(unconv.sum().item()),
                  "MPC_tracking_lanes_wall_s_median": float(np.median(walls)), "MPC_tracking_lanes_wall_s": walls,
                  "loop_over_new_call_wall": loop_s / float(np.median(walls))})
        res["arms"]["c_256_distinct_lanes"] = t
        line("c 256 distinct lanes, kernel", t)
        print(f"c: per-lane loop {loop_s:.2f} s wall, MPC_tracking_lanes(tau_max=18) {np.median(walls) * 1e3:.1f} ms "
              f"wall: x{t['loop_over_new_call_wall']:.0f}", flush=True)
        del call

    if "d" in args.arms:
        B = args.big_lanes
        idx = torch.arange(B, device=eng.device) % lanes["x"].shape[0]
        xd, ud = eng.t(lanes["x"])[idx].contiguous(), eng.t(lanes["u"])[idx].contiguous()
        x0d = (xd[:, 0] + 0.02)[:, None].contiguous()
        need = eng.mpc_box_lanes_workspace(B, 1, 75)
        free = torch.cuda.mem_get_info(eng.device)[0]
        if need <= eng.BOX_LANES_WS_SHARE * free:
            call = Call(eng, tt, xd, ud, x0d, 75, 18.0, trajectories=False)
            t = timed(call, 1, 3)
            t.update(call.facts())
            t["path"] = "one call"
        else:
            QT = tt._mpc_terminal_weight(eng, tt.Q_MPC, tt.R_MPC)
            t = timed(lambda: eng.mpc_box_lanes_rollout(xd, ud, x0d, tt.Q_MPC, tt.R_MPC, QT, 75, 18.0,
                                                        trajectories=False), 1, 3)
            t["path"] = "lane chunks (engine)"
            t["workspace_MB"] = need / 1e6
        t.update({"lanes": B, "free_device_memory_MB": free / 1e6,
                  "ratio_to_unconstrained_lanes_path": t["median_us"] / 1e3 / UNCONSTRAINED_LANES_MS})
        res["arms"][f"d_{B}_lanes_summaries"] = t
        line(f"d {B} lanes, summaries only ({t['path']}, workspace {t['workspace_MB']:.0f} MB, "
             f"x{t['ratio_to_unconstrained_lanes_path']:.0f} the unconstrained 43 ms)", t)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
