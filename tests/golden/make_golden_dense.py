"""Generate tests/golden/dense_kats.npz by running the REFERENCE on the dense generators of tests/dense_ref.py
(test infrastructure).

Runs in the build container only (the read-only reference is mounted at /root/reference); never on the GPU box,
never imported by the product.  Writes plain data (expected outputs; the inputs are re-created from the seeded
generators, a digest of them is stored); no reference source is copied into the repository.

trajectory_generation is imported as make_golden.py does (_import_reference); compute_P_inf and simulate_tracking
are compiled from trajectory_tracking.py's own syntax tree as make_golden_tracking.py does (the module imports
casadi, which is absent; these two functions never touch it).

Four lanes of each call (the reference is one lane at a time):
  ric_K, ric_sigma, ric_dJ      calculate_K_and_sigma on gen_riccati's pivot-forcing data, T = 9
  sc_l, sc_gx, sc_gu, sc_lT, sc_gT   derivatives_Cost (stage, terminal) with gen_dense_weights' non-symmetric
                                Q, R, Q_T on the first 8 of gen_points' points
  tc_J                          total_cost with those weights on gen_trajectories' lanes, N = 9
  cl_x, cl_u                    forward_closed_loop_update with gen_gains' dense K, sigma and per-lane gamma
  pinf_dense, pinf_pad          compute_P_inf on gen_dare's pair and on tracking.npz's pad with gen_mpc_weights
  trk_x, trk_u                  simulate_tracking with gen_track's dense K, N = 9

Usage:  python tests/golden/make_golden_dense.py
"""
import ast
import contextlib
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

REF = "/root/reference"
NL = 4          # lanes per call
NP = 8          # points of the stage-cost calls
FUNCS = ("compute_P_inf", "simulate_tracking")


def inputs_digest():
    """sha256 over every generator's output: a changed seed or generator invalidates the fixture visibly."""
    import dense_ref as dr
    h = hashlib.sha256()
    gens = [dr.gen_points(), dict(zip("QRT", dr.gen_dense_weights())), dr.gen_trajectories(), dr.gen_gains(),
            dr.gen_riccati(), dr.gen_dare(), dict(zip("QR", dr.gen_mpc_weights())), dr.gen_track()]
    for g in gens:
        for k in sorted(g):
            h.update(k.encode() + np.ascontiguousarray(g[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def main():
    import dense_ref as dr
    from make_golden import _import_reference
    trk = np.load(os.path.join(HERE, "tracking.npz"))     # before _import_reference changes directory
    A_f, B_f = trk["A_f"], trk["B_f"]
    digest = inputs_digest()
    tg = _import_reference()
    tree = ast.parse(open(os.path.join(REF, "trajectory_tracking.py")).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(d.name for d in defs) == sorted(FUNCS)
    ns = {k: getattr(tg, k) for k in dir(tg) if not k.startswith("__")}
    ns["np"] = np
    exec(compile(ast.Module(body=defs, type_ignores=[]), os.path.join(REF, "trajectory_tracking.py"), "exec"), ns)

    out = {"digest": np.array(digest)}
    d = dr.gen_riccati()
    Ks, ss, dJs = [], [], []
    for l in range(NL):
        a = [list(d[k][l]) for k in ("A", "B", "Q", "R", "S", "q", "r")]
        K, s, dJ = tg.calculate_K_and_sigma(*a, d["QT"][l], d["qT"][l])
        Ks.append(np.asarray(K)); ss.append(np.asarray(s)); dJs.append(float(dJ))
    out.update(ric_K=np.array(Ks), ric_sigma=np.array(ss), ric_dJ=np.array(dJs))

    p = dr.gen_points()
    Q, R, QT = dr.gen_dense_weights()
    sc = {k: [] for k in ("sc_l", "sc_gx", "sc_gu", "sc_lT", "sc_gT")}
    for i in range(NP):
        l, gx, gu, _, _ = tg.derivatives_Cost(p["X"][i], p["xr"][i], p["U"][i], p["ur"][i], Q, R)
        lT, gT, _ = tg.derivatives_Cost(p["X"][i], p["xr"][i], p["U"][i], p["ur"][i], None, None, Q_T=QT,
                                        terminal=True)
        for k, v in zip(sc, (l, gx, gu, lT, gT)):
            sc[k].append(v)
    out.update({k: np.array(v) for k, v in sc.items()})

    t = dr.gen_trajectories()
    g = dr.gen_gains()
    out["tc_J"] = np.array([tg.total_cost(t["x"][l], t["u"][l], t["x_ref"], t["u_ref"], Q, R, QT) for l in range(NL)])
    xs, us = [], []
    for l in range(NL):
        xn, un = tg.forward_closed_loop_update(t["x"][l], t["u"][l], list(g["K"][l]), list(g["sigma"][l]),
                                               gamma=float(g["gamma"][l]))
        xs.append(xn); us.append(un)
    out.update(cl_x=np.array(xs), cl_u=np.array(us))

    dd = dr.gen_dare()
    Qm, Rm = dr.gen_mpc_weights()
    with contextlib.redirect_stdout(io.StringIO()):
        out["pinf_dense"] = ns["compute_P_inf"](dd["A"], dd["B"], dd["Q"], dd["R"])
        out["pinf_pad"] = ns["compute_P_inf"](A_f, B_f, Qm, Rm)

    k = dr.gen_track()
    xs, us = [], []
    for l in range(NL):
        x, u = ns["simulate_tracking"](k["x_ff"], k["u_ff"], list(k["K"]), k["x0"][l].copy())
        xs.append(x); us.append(u)
    out.update(trk_x=np.array(xs), trk_u=np.array(us))

    np.savez_compressed(os.path.join(HERE, "dense_kats.npz"), **out)
    print("wrote dense_kats.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
