"""NumPy restatement of the Newton solve on the RK4-exact linearisation (test helper, not a test).

The sweep of newton_Algorithm linearises the dynamics by forward Euler (A_d = I + dt A_c) while every rollout is RK4,
so dJ is not the directional derivative of the cost the Armijo test measures.  Here the stage matrices are the exact
Jacobians of one RK4 step x+ = x + h/6 (k1 + 2 k2 + 2 k3 + k4) at (x_t, u_t), by the chain rule through its four stage
points X1 = x, X2 = x + h/2 k1, X3 = x + h/2 k2, X4 = x + h k3 (J_i, B_i: the continuous Jacobians at (X_i, u)):
    d1 = J1,  d2 = J2 (I + h/2 d1),  d3 = J3 (I + h/2 d2),  d4 = J4 (I + h d3),  A_d = I + h/6 (d1 + 2 d2 + 2 d3 + d4)
    e1 = B1,  e2 = J2 (h/2 e1) + B2, e3 = J3 (h/2 e2) + B3, e4 = J4 (h e3) + B4, B_d = h/6 (e1 + 2 e2 + 2 e3 + e4)
Column 0 of B_d is exactly zero (tau1 never enters f), so channel 0 still never couples.

The sweep, the closed loop and the solve are tests/newton_box_ref.py's (the control-limited form, tau_max = inf: no
limit), with the stage-list function a parameter: with oracle.acrobot_np.stage_lists they are newton_box_solve.
"""
from __future__ import annotations

import numpy as np

import newton_box_ref as nb
from oracle import acrobot_np as onp

ACTIVE, CONVERGED, LS_FAILED, MAX_ITERS = onp.ACTIVE, onp.CONVERGED, onp.LS_FAILED, onp.MAX_ITERS
short_setup = nb.short_setup


def rk4_lin(x, u, pset=1, dt=onp.DT):
    """x (B,4), u (B,2) -> A_d (B,4,4), B_d (B,4,2): the Jacobians of onp.rk4(x, u) with respect to x and u."""
    x = np.atleast_2d(np.asarray(x, float)); u = np.atleast_2d(np.asarray(u, float))
    I = np.eye(4)
    k1 = onp.continuous_dynamics(x, u, pset)
    J1, B1 = onp.jacobians(x, u, pset)
    x2 = x + (dt / 2) * k1
    k2 = onp.continuous_dynamics(x2, u, pset)
    J2, B2 = onp.jacobians(x2, u, pset)
    x3 = x + (dt / 2) * k2
    k3 = onp.continuous_dynamics(x3, u, pset)
    J3, B3 = onp.jacobians(x3, u, pset)
    J4, B4 = onp.jacobians(x + dt * k3, u, pset)
    d1 = J1
    d2 = J2 @ (I + (dt / 2) * d1)
    d3 = J3 @ (I + (dt / 2) * d2)
    d4 = J4 @ (I + dt * d3)
    e1 = B1
    e2 = J2 @ ((dt / 2) * e1) + B2
    e3 = J3 @ ((dt / 2) * e2) + B3
    e4 = J4 @ (dt * e3) + B4
    return I + (dt / 6) * (d1 + 2 * d2 + 2 * d3 + d4), (dt / 6) * (e1 + 2 * e2 + 2 * e3 + e4)


def stage_lists_rk4(x, u, x_ref, u_ref, Q=onp.Q_DEFAULT, R=onp.R_DEFAULT, QT=onp.QT_DEFAULT, pset=1):
    """onp.stage_lists with the RK4-exact A_d, B_d: the same return shape, the same q, r, 2 Q_T, q_T."""
    B, N = x.shape[:2]
    T = N - 1
    A_d = np.zeros((B, T, 4, 4)); B_d = np.zeros((B, T, 4, 2))
    for t in range(T):
        A_d[:, t], B_d[:, t] = rk4_lin(x[:, t], u[:, t], pset)
    q = np.einsum("ij,btj->bti", 2 * Q, x[:, :T] - x_ref[:T])
    r = np.einsum("ij,btj->bti", 2 * R, u - u_ref)
    qT = np.einsum("ij,bj->bi", 2 * QT, x[:, -1] - x_ref[-1])
    return A_d, B_d, q, r, 2 * QT, qT


def box_sweep(x, u, x_ref, u_ref, tau, Q=onp.Q_DEFAULT, R=onp.R_DEFAULT, QT=onp.QT_DEFAULT, pset=1,
              stage_lists=stage_lists_rk4):
    """newton_box_ref.box_sweep on ``stage_lists``' stage data: K (B,T,2,4), sigma (B,T,2), dJ (B,), clamped (B,T)."""
    A_d, B_d, q, r, QTb, qT = stage_lists(x, u, x_ref, u_ref, Q, R, QT, pset)
    Bn, T = A_d.shape[:2]
    assert R[0, 1] == 0 and R[1, 0] == 0 and not B_d[..., 0].any(), "channel 0 must not couple"
    P = np.broadcast_to(QTb, (Bn, 4, 4)).copy()
    p = qT.copy()
    K = np.zeros((Bn, T, 2, 4)); sig = np.zeros((Bn, T, 2)); dJ = np.zeros(Bn)
    clamped = np.zeros((Bn, T), bool)
    with np.errstate(invalid="ignore"):
        for t in range(T - 1, -1, -1):
            A = A_d[:, t]; b = B_d[:, t, :, 1]
            AT = np.swapaxes(A, 1, 2)
            Pb = np.einsum("bij,bj->bi", P, b)
            G11 = 2 * R[1, 1] + np.einsum("bi,bi->b", b, Pb)
            F = np.einsum("bi,bij->bj", Pb, A)
            g1 = r[:, t, 1] + np.einsum("bi,bi->b", b, p)
            s1u = -g1 / G11
            lo, hi = -tau - u[:, t, 1], tau - u[:, t, 1]
            cl = (s1u < lo) | (s1u > hi)
            s1 = np.where(s1u < lo, lo, np.where(s1u > hi, hi, s1u))
            k = np.where(cl[:, None], 0.0, -F / G11[:, None])
            s0 = -r[:, t, 0] / (2 * R[0, 0])
            dJ += r[:, t, 0] * s0 + g1 * s1
            Ap = np.einsum("bij,bj->bi", AT, p)
            p = q[:, t] + Ap + np.where(cl[:, None], F * s1[:, None], -k * (G11 * s1)[:, None])
            P = 2 * Q + AT @ P @ A - G11[:, None, None] * k[:, :, None] * k[:, None, :]
            K[:, t, 1] = k
            sig[:, t, 0] = s0; sig[:, t, 1] = s1
            clamped[:, t] = cl
    return K, sig, dJ, clamped


def newton_rk4lin_solve(x0, x_ref, u_ref, max_iters, tau_max=np.inf, tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0,
                        max_ls=20, Q=onp.Q_DEFAULT, R=onp.R_DEFAULT, QT=onp.QT_DEFAULT, pset=1,
                        stage_lists=stage_lists_rk4):
    """newton_box_ref.newton_box_solve with the sweep on ``stage_lists`` (default: the RK4-exact ones); the same
    fields and the same record of the decisions (accepted, n_clamped, clamped, margin)."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    x_ref = np.asarray(x_ref, float); u_ref = np.asarray(u_ref, float)
    if u_ref.shape[0] == x_ref.shape[0]:
        u_ref = u_ref[:-1]
    Bn, T = x0.shape[0], u_ref.shape[0]
    tau = np.broadcast_to(np.asarray(tau_max, float), (Bn,)).copy()
    if not (tau > 0).all():
        raise ValueError("tau_max must be positive")
    u = np.zeros((Bn, T, 2))
    x = onp.simulate_open_loop(x0, u, pset)
    J = onp.total_cost(x, u, x_ref, u_ref, Q, R, QT)
    status = np.full(Bn, ACTIVE); n_iter = np.zeros(Bn, int); n_roll = np.zeros(Bn, int)
    K = np.zeros((Bn, T, 2, 4)); sig = np.zeros((Bn, T, 2)); clamped = np.zeros((Bn, T), bool)
    margin = np.full(Bn, np.inf)
    accepted, n_clamped = [], []
    with np.errstate(invalid="ignore"):
        for _k in range(int(max_iters)):
            ia = np.nonzero(status == ACTIVE)[0]
            if ia.size == 0:
                break
            acc_k = np.zeros(Bn, int); ncl_k = np.full(Bn, -1)
            Ka, sa, dJ, cl = box_sweep(x[ia], u[ia], x_ref, u_ref, tau[ia], Q, R, QT, pset, stage_lists)
            K[ia] = Ka; sig[ia] = sa; clamped[ia] = cl
            ncl_k[ia] = cl.sum(1)
            smax = np.max(np.abs(sa), axis=(1, 2))
            gam = np.full(ia.size, float(gamma_0))
            done = np.zeros(ia.size, bool)
            for i in range(max_ls):
                todo = np.nonzero(~done)[0]
                if todo.size == 0:
                    break
                ln = ia[todo]
                xn, un = nb.closed_loop_box(x[ln], u[ln], Ka[todo], sa[todo], gam[todo], tau[ln], pset)
                Jn = onp.total_cost(xn, un, x_ref, u_ref, Q, R, QT)
                n_roll[ln] += 1
                bound = J[ln] + c * gam[todo] * dJ[todo]
                margin[ln] = np.fmin(margin[ln], np.abs(Jn - bound) / np.abs(J[ln]))
                ok = Jn < bound
                good = ln[ok]
                x[good] = xn[ok]; u[good] = un[ok]; J[good] = Jn[ok]
                acc_k[good] = i + 1
                done[todo[ok]] = True
                gam[todo[~ok]] *= beta
            n_iter[ia] += 1
            status[ia[~done]] = LS_FAILED
            margin[ia[done]] = np.fmin(margin[ia[done]], np.abs(smax[done] - tol) / tol)
            status[ia[done & (smax < tol)]] = CONVERGED
            accepted.append(acc_k); n_clamped.append(ncl_k)
    status = status.copy()
    status[status == ACTIVE] = MAX_ITERS
    return dict(x=x, u=u, K=K, sigma=sig, n_iter=n_iter, status=status, cost=J, n_rollouts=n_roll, clamped=clamped,
                accepted=np.array(accepted).reshape(-1, Bn), n_clamped=np.array(n_clamped).reshape(-1, Bn),
                margin=margin)
