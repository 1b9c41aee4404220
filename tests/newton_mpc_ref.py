"""NumPy restatement of closed-loop replanning on the batched Newton solver (test helper, not a test).

BatchedNewtonSolver.closed_loop / gym_newton_mpc_run, line by line, built only from
tests/newton_box_ref.py's box_sweep, closed_loop_box and clip_nan and oracle.acrobot_np; the plant of lane b is the
parameter set of its key (tests/plant_ref.py's KEYS), the design model is set 1.

One closed loop per lane.  After the start (u = 0 or u_init, rolled out on the design model) lane b holds a plan x, u
over the knots 0 .. N-1 and its cost J.  Control step t, 0 <= t < T, on the horizon of stages t .. T-1 (every array from
row t):
  1. replan, at most ``iters`` times (``iters_first`` at t = 0): box_sweep of the horizon; if max|sigma| < tol the plan
     is kept, no trial runs and the step stops CONVERGED (the test comes BEFORE the trials); else the Armijo trials
     closed_loop_box at gamma_0, gamma_0 beta, ... (at most max_ls, strict test J_new < J + c gamma dJ): the first
     accepted one replaces the plan and J, none accepted stops the step LS_FAILED with the plan kept.  An iteration is
     counted when its trials ran.  Either stop ends this step only.
  2. act: u_t = u[t], x_t = x[t] are recorded, x_{t+1} = rk4(x_t, u_t) on the lane's plant, J <- J - l_t with
     l_t = dx_t' Q dx_t + du_t' R du_t (one subtraction, no pass).
  3. re-anchor, only if t + 1 < T and x_{t+1} differs in any bit from x[t + 1]: box_sweep of horizon t + 1, the policy
     rolled out at step size 0 from x_{t+1} (u_new = u + K (x_new - x) + 0 sigma, clipped as every trial, design-model
     RK4), accepted unconditionally with its cost as the new J.  One rollout, no iteration.
``margin`` (B,T): per step the smallest relative distance of any Armijo or stop decision from a tie
(newton_box_ref.newton_box_solve's measure: |J_new - bound| / |J|, |max|sigma| - tol| / tol).
"""
from __future__ import annotations

import numpy as np

import newton_box_ref as nb
import plant_ref as pr
from oracle import acrobot_np as onp

ACTIVE, CONVERGED, LS_FAILED = nb.ACTIVE, nb.CONVERGED, nb.LS_FAILED
KEYS = pr.KEYS
# the decision-parity settings of the tests (N = 41, nb.short_setup): far from every tie at tol = 1e-2
SHORT = dict(tol=1e-2, beta=0.7, c=0.5, gamma_0=0.5, max_ls=20)


def keys_of(B):
    """Lane b runs on plant KEYS[b % 4]."""
    return [KEYS[b % 4] for b in range(B)]


def params_of(keys):
    """(B,11) parameter rows of a list of keys, to hand to ``plant=``."""
    return pr.params_of([keys])[0]


def plant_step(x, u, keys):
    """x (B,4), u (B,2) -> x_next (B,4), lane b on keys[b]: every lane of one key through one rk4 call."""
    return pr.plant_step(x[:, None], u[:, None], [[k] for k in keys])[:, 0]


def _stage_cost(x, u, xr, ur, Q, R):
    dx, du = x - xr, u - ur
    return np.einsum("bi,ij,bj->b", dx, Q, dx) + np.einsum("bi,ij,bj->b", du, R, du)


def _reanchor_rollout(x, u, K, sig, xhat, tau):
    """closed_loop_box at gamma = 0 from another start: the plan's policy from the measured state."""
    xn = x.copy(); un = u.copy()
    xn[:, 0] = xhat
    for s in range(x.shape[1] - 1):
        un[:, s] = u[:, s] + np.einsum("bij,bj->bi", K[:, s], xn[:, s] - x[:, s]) + 0.0 * sig[:, s]
        un[:, s, 1] = nb.clip_nan(un[:, s, 1], tau)
        xn[:, s + 1] = onp.rk4(xn[:, s], un[:, s], pset=1)
    return xn, un


def mpc_closed_loop(x0, x_ref, u_ref, tau_max, keys, iters=1, iters_first=None, u_init=None, n_steps=None, tol=1e-6,
                    beta=0.7, c=0.5, gamma_0=1.0, max_ls=20, Q=onp.Q_DEFAULT, R=onp.R_DEFAULT, QT=onp.QT_DEFAULT):
    """x0 (B,4); x_ref (N,4), u_ref (T,2) shared or (B,N,4), (B,T,2) per lane; tau_max None, a number or (B,); keys
    (B) plant keys -> dict of x (B,N,4), u (B,T,2), iters, rollouts, stop (B,T) int, cost, margin (B,T), reanchors (B,),
    err_final, u_max (B,)."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    x_ref = np.asarray(x_ref, float); u_ref = np.asarray(u_ref, float)
    Bn = x0.shape[0]
    tau = np.broadcast_to(np.asarray(np.inf if tau_max is None else tau_max, float), (Bn,)).copy()
    kw = dict(iters=iters, iters_first=iters_first, n_steps=n_steps, tol=tol, beta=beta, c=c, gamma_0=gamma_0,
              max_ls=max_ls, Q=Q, R=R, QT=QT)
    if x_ref.ndim == 3:            # per-lane references: the lanes of one reference together, every group on its own
        out = None
        ids = [x_ref[b].tobytes() + u_ref[b].tobytes() for b in range(Bn)]
        for key in dict.fromkeys(ids):
            ln = np.array([b for b in range(Bn) if ids[b] == key])
            r = mpc_closed_loop(x0[ln], x_ref[ln[0]], u_ref[ln[0]], tau[ln], [keys[b] for b in ln],
                                u_init=None if u_init is None else np.asarray(u_init, float)[ln], **kw)
            if out is None:
                out = {k: np.zeros((Bn,) + v.shape[1:], v.dtype) for k, v in r.items()}
            for k, v in r.items():
                out[k][ln] = v
        return out
    T = u_ref.shape[0]
    N = T + 1
    n_steps = T if n_steps is None else int(n_steps)
    iters_first = iters if iters_first is None else iters_first
    u = np.zeros((Bn, T, 2)) if u_init is None else np.array(u_init, float)
    x = onp.simulate_open_loop(x0, u, 1)
    J = onp.total_cost(x, u, x_ref, u_ref, Q, R, QT)
    X = np.zeros((Bn, N, 4)); U = np.zeros((Bn, T, 2))
    n_it = np.zeros((Bn, T), int); n_ro = np.zeros((Bn, T), int); stop = np.zeros((Bn, T), int)
    cost = np.zeros((Bn, T)); margin = np.full((Bn, T), np.inf); reanchors = np.zeros(Bn, int)
    with np.errstate(all="ignore"):
        for t in range(n_steps):
            xr, ur = x_ref[t:], u_ref[t:]
            st = np.full(Bn, ACTIVE)
            for _k in range(iters_first if t == 0 else iters):                      # ---- 1. replan
                ia = np.nonzero(st == ACTIVE)[0]
                if ia.size == 0:
                    break
                Ka, sa, dJ, _ = nb.box_sweep(x[ia, t:], u[ia, t:], xr, ur, tau[ia], Q, R, QT, 1)
                smax = np.max(np.abs(sa), axis=(1, 2))
                margin[ia, t] = np.fmin(margin[ia, t], np.abs(smax - tol) / tol)
                conv = smax < tol                                                   # before the trials
                st[ia[conv]] = CONVERGED
                go = np.nonzero(~conv)[0]
                gam = np.full(go.size, float(gamma_0))
                done = np.zeros(go.size, bool)
                for _i in range(max_ls):
                    todo = np.nonzero(~done)[0]
                    if todo.size == 0:
                        break
                    sel = go[todo]
                    ln = ia[sel]
                    xn, un = nb.closed_loop_box(x[ln, t:], u[ln, t:], Ka[sel], sa[sel], gam[todo], tau[ln], 1)
                    Jn = onp.total_cost(xn, un, xr, ur, Q, R, QT)
                    n_ro[ln, t] += 1
                    bound = J[ln] + c * gam[todo] * dJ[sel]
                    margin[ln, t] = np.fmin(margin[ln, t], np.abs(Jn - bound) / np.abs(J[ln]))
                    ok = Jn < bound
                    good = ln[ok]
                    x[good, t:] = xn[ok]; u[good, t:] = un[ok]; J[good] = Jn[ok]
                    done[todo[ok]] = True
                    gam[todo[~ok]] *= beta
                n_it[ia[go], t] += 1
                st[ia[go[~done]]] = LS_FAILED
            stop[:, t] = st
            cost[:, t] = J                                                          # ---- 2. act
            X[:, t] = x[:, t]; U[:, t] = u[:, t]
            J = J - _stage_cost(x[:, t], u[:, t], x_ref[t], u_ref[t], Q, R)
            xh = plant_step(x[:, t], u[:, t], keys)
            X[:, t + 1] = xh
            if t + 1 < T:                                                           # ---- 3. re-anchor
                plan = np.ascontiguousarray(x[:, t + 1])
                ir = np.nonzero((np.ascontiguousarray(xh).view(np.int64) != plan.view(np.int64)).any(1))[0]
                if ir.size:
                    Ka, sa, _, _ = nb.box_sweep(x[ir, t + 1:], u[ir, t + 1:], x_ref[t + 1:], u_ref[t + 1:], tau[ir],
                                                Q, R, QT, 1)
                    xn, un = _reanchor_rollout(x[ir, t + 1:], u[ir, t + 1:], Ka, sa, xh[ir], tau[ir])
                    x[ir, t + 1:] = xn; u[ir, t + 1:] = un
                    J[ir] = onp.total_cost(xn, un, x_ref[t + 1:], u_ref[t + 1:], Q, R, QT)
                    n_ro[ir, t] += 1
                    reanchors[ir] += 1
        err = np.max(np.abs(X[:, -1] - x_ref[-1]), axis=1)
    return dict(x=X, u=U, iters=n_it, rollouts=n_ro, stop=stop, cost=cost, margin=margin, reanchors=reanchors,
                err_final=err, u_max=np.max(np.abs(U), axis=(1, 2)))


# ---------------------------------------------------------------------------------------------- the parity cases
# tests/golden/newton_mpc_ref.npz holds mpc_closed_loop's answers for the GPU parity test, so that the GPU suite does
# not spend a minute of NumPy on them; tests/test_newton_mpc_host.py recomputes every case and compares bit for bit.
# Written by ``PYTHONPATH=. python tests/newton_mpc_ref.py`` from the repository root.
PARITY_LANES = 70            # two wavefronts, one of them ragged
DISTINCT = 20                # start b % 5, plant KEYS[b % 4], reference variant b % 2: period 20
PARITY_CASES = [(tau, u0, ref) for tau in (None, 2.0) for u0 in ("zero", "live") for ref in ("shared", "lane")]
PARITY_FIELDS = ("x", "u", "iters", "rollouts", "stop", "cost", "margin", "reanchors")
PARITY_ITERS = dict(iters=1, iters_first=3)
GOLDEN_FILE = "newton_mpc_ref.npz"


def case_name(tau, u0, ref):
    return f"tau{'inf' if tau is None else f'{tau:g}'}_{u0}_{ref}"


def parity_inputs(x_ref, u_ref, u0, ref, B=PARITY_LANES):
    """The inputs of a parity case for B lanes: x0 (B,4), x_ref, u_ref (shared, or per lane with two variants), keys.
    ``u0`` "live": a tau1 reference that is not zero (the general kernels); ``ref`` "lane": per-lane references."""
    x0, xr, ur = nb.short_setup(x_ref, u_ref)
    b = np.arange(B)
    if u0 == "live":
        ur = ur.copy()
        ur[:, 0] = 0.05 * np.cos(0.3 * np.arange(ur.shape[0]))
    if ref == "lane":
        v = (b % 2)[:, None, None]
        xr = xr[None] + 0.02 * v * np.array([1.0, 1.0, 0.0, 0.0])
        ur = ur[None] * (1.0 + 0.01 * v)
    return x0[b % 5], xr, ur, keys_of(B)


def parity_case(x_ref, u_ref, tau, u0, ref):
    """mpc_closed_loop's answer for the DISTINCT lanes of a case (lane b of the 70 is lane b % DISTINCT)."""
    x0, xr, ur, keys = parity_inputs(x_ref, u_ref, u0, ref, DISTINCT)
    r = mpc_closed_loop(x0, xr, ur, tau, keys, **PARITY_ITERS, **SHORT)
    return {k: r[k] for k in PARITY_FIELDS}


if __name__ == "__main__":
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    xr_, ur_, _ = onp.load_task2_refs(os.path.join(here, "golden", "task2_input_fully_actuated.npz"))
    out = {}
    for case in PARITY_CASES:
        r_ = parity_case(xr_, ur_, *case)
        print(case_name(*case), "margin", r_["margin"].min(), "iters", r_["iters"].sum(1).tolist(), "rollouts",
              r_["rollouts"].sum(1).tolist(), flush=True)
        out.update({f"{case_name(*case)}/{k}": v for k, v in r_.items()})
    np.savez_compressed(os.path.join(here, "golden", GOLDEN_FILE), **out)
