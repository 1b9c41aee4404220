"""Times of the warm start's init path at a batch shape (default BASELINE cfg 3: 262,144 lanes, T = 500), by HIP events
on the solver's stream: gym_newton_init_warm (identity and Morton lane map) against gym_newton_init, and
gym_pack_lanes (the parent's lane-major -> planes kernel) on the same u_init array.  One JSON line.

    python tools/warm_profile.py [--lanes 262144] [--reps 5] [--out FILE]

The gather-pack kernel has no entry point of its own; its time comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/warm_profile.py: k_gather_pack_u against k_pack), see
profiles/warm_start/README.md.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import load_refs, make_x0  # noqa: E402
from gymnast_optimalcontrol_amd import _lib  # noqa: E402
from gymnast_optimalcontrol_amd.engine import AcrobotEngine  # noqa: E402
from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver, morton_order  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.lanes
    xr, ur = load_refs()
    eng = AcrobotEngine()
    dev = eng.device
    s = BatchedNewtonSolver(eng, xr, ur, B, tol=1e-4, gamma_0=0.1, pipeline=True)   # one stream set, no placement race
    T, Bp = s.T, s.Bp
    x0 = eng.t(make_x0(B))
    perm = morton_order(x0)
    # a control iterate with the tau1 plane zero (the solver runs with GYM_FLAG_U0_ZERO): the reference controls, scaled
    u = torch.zeros((B, T, 2), dtype=torch.float64, device=dev)
    u[:, :, 1] = eng.t(ur)[:, 1][None] * torch.linspace(0.5, 1.0, B, dtype=torch.float64, device=dev)[:, None]
    planes = torch.empty((T, 2, Bp, 1), dtype=torch.float64, device=dev)
    m, w, b, lib = C.byref(eng.model), C.byref(eng._w), C.byref(s.batch), eng.lib

    def cold():
        _lib.check(lib.gym_newton_init(m, w, x0.data_ptr(), b, eng.stream), "gym_newton_init")

    def warm(lane_map):
        s.batch.lane_map = None if lane_map is None else lane_map.data_ptr()
        try:
            _lib.check(lib.gym_newton_init_warm(m, w, x0.data_ptr(), u.data_ptr(), None, b, eng.stream),
                       "gym_newton_init_warm")
        finally:
            s.batch.lane_map = None

    def pack():
        _lib.check(lib.gym_pack_lanes(u.data_ptr(), planes.data_ptr(), B, Bp, T, 2, 1, eng.stream), "gym_pack_lanes")

    def timed(fn):
        ms = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms[1:]                                   # the first call warms the code object up

    res = {"lanes": B, "T": T, "u_init_GB": u.numel() * 8 / 1e9, "reps": a.reps,
           "device": torch.cuda.get_device_name(dev)}
    for name, fn in (("gym_newton_init", cold), ("gym_newton_init_warm", lambda: warm(None)),
                     ("gym_newton_init_warm_morton", lambda: warm(perm)), ("gym_pack_lanes_u", pack)):
        ms = timed(fn)
        res[name + "_ms"] = {"min": min(ms), "median": float(np.median(ms)), "all": [round(v, 4) for v in ms]}
    # the warm init with the Morton map computes what the identity map computes on permuted inputs
    warm(perm)
    a_u, a_c = s.u[0].clone(), s.cost.clone()
    up = u[perm].contiguous()
    x0p = x0[perm].contiguous()
    _lib.check(lib.gym_newton_init_warm(m, w, x0p.data_ptr(), up.data_ptr(), None, b, eng.stream),
               "gym_newton_init_warm")
    torch.cuda.synchronize(dev)
    res["morton_map_equals_permuted_inputs"] = bool(torch.equal(a_u, s.u[0]) and torch.equal(a_c, s.cost))
    _lib.check(lib.gym_pack_lanes(up.data_ptr(), planes.data_ptr(), B, Bp, T, 2, 1, eng.stream), "gym_pack_lanes")
    torch.cuda.synchronize(dev)
    res["gather_pack_equals_pack_lanes"] = bool(torch.equal(planes.view(-1), s.u[0].view(-1)))
    # bytes the pack moves: the lane-major array in, the planes (Bp lanes) out
    moved = 8.0 * (B * T * 2 + Bp * T * 2)
    res["pack_bytes"] = moved
    res["gym_pack_lanes_u_GBps"] = moved / (res["gym_pack_lanes_u_ms"]["median"] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
