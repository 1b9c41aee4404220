"""NumPy restatement of the torque-limited Newton solve (test helper, not a test).

The control-limited form of newton_Algorithm (control-limited DDP, Tassa, Mansard and Todorov 2014) specialised to the
acrobot, on top of oracle.acrobot_np's dense stage data.  Only tau2 enters the dynamics, R is diagonal and S = 0, so
channel 0 never couples (sigma0 = -r0 / 2R0, K row 0 = 0) and channel 1's box QP is a scalar clip.  Per lane a limit
tau with 0 < tau <= inf; |u_t[1]| <= tau on every stage of every iterate (u = 0 at the start satisfies it).

Backward sweep, stage t (b = column 1 of B_d):
    G11 = 2 R11 + b'Pb,  F = b'P A_d,  g1 = r1 + b'p,  s1u = -g1 / G11,  lo = -tau - u_t[1],  hi = tau - u_t[1]
    clamped iff s1u < lo or s1u > hi (a NaN s1u is not)
    not clamped: k = -F / G11, s1 = s1u, P <- 2Q + A'PA - G11 k k', p <- q + A'p - k G11 s1
    clamped:     k = 0, s1 = the bound,  P <- 2Q + A'PA,              p <- q + A'p + F s1
    dJ += r0 s0 + g1 s1;  max|sigma| over s0 and the clamped s1
Trials: u_new = u + K (x_new - x) + gamma sigma, then u_new[1] = clip(u_new[1], -tau, tau) with NaN kept, before the
cost and the RK4 step.  Armijo test, gamma <- beta gamma, update, stop test, LS failure, statuses and counters are
oracle.acrobot_np.NewtonStepper's.
"""
from __future__ import annotations

import numpy as np

from oracle import acrobot_np as onp

ACTIVE, CONVERGED, LS_FAILED, MAX_ITERS = onp.ACTIVE, onp.CONVERGED, onp.LS_FAILED, onp.MAX_ITERS


def short_setup(x_ref, u_ref):
    """The short-horizon setup of the tests: the first 41 knots of the task-2 references and five starts (joint
    angles rng(0).uniform(-0.5, 0.5), at rest).  Returns x0 (5,4), x_ref (41,4), u_ref (40,2)."""
    x0 = np.zeros((5, 4))
    x0[:, :2] = np.random.default_rng(0).uniform(-0.5, 0.5, (5, 2))
    return x0, np.asarray(x_ref, float)[:41], np.asarray(u_ref, float)[:40]


def clip_nan(v, tau):
    """clip(v, -tau, tau) that keeps a NaN a NaN (never a bound)."""
    v = np.asarray(v, float)
    with np.errstate(invalid="ignore"):
        return np.where(v != v, v, np.minimum(np.maximum(v, -tau), tau))


def box_sweep(x, u, x_ref, u_ref, tau, Q=onp.Q_DEFAULT, R=onp.R_DEFAULT, QT=onp.QT_DEFAULT, pset=1):
    """x (B,N,4), u (B,T,2), tau (B,) -> K (B,T,2,4), sigma (B,T,2), dJ (B,), clamped (B,T) bool."""
    A_d, B_d, q, r, QTb, qT = onp.stage_lists(x, u, x_ref, u_ref, Q, R, QT, pset)
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


def closed_loop_box(x, u, K, sig, gamma, tau, pset=1):
    """oracle.acrobot_np.closed_loop with u_new[1] clipped to the lane's box before the RK4 step."""
    B, N = x.shape[:2]
    gamma = np.broadcast_to(np.asarray(gamma, float), (B,))
    xn = x.copy(); un = u.copy()
    for t in range(N - 1):
        dx = xn[:, t] - x[:, t]
        un[:, t] = u[:, t] + np.einsum("bij,bj->bi", K[:, t], dx) + gamma[:, None] * sig[:, t]
        un[:, t, 1] = clip_nan(un[:, t, 1], tau)
        xn[:, t + 1] = onp.rk4(xn[:, t], un[:, t], pset=pset)
    return xn, un


def newton_box_solve(x0, x_ref, u_ref, max_iters, tau_max, tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0, max_ls=20,
                     Q=onp.Q_DEFAULT, R=onp.R_DEFAULT, QT=onp.QT_DEFAULT, pset=1):
    """Per-lane torque-limited newton_Algorithm, vectorised over lanes.  Returns NewtonStepper.result()'s fields plus
    clamped (B,T) of each lane's last sweep and the record of the decisions:
      accepted (iterations, B)  the Armijo trial each lane accepted (1-based; 0: failed or did not run)
      n_clamped (iterations, B) clamped stages of each lane's sweep (-1: did not run)
      margin (B,)               the smallest relative distance of any Armijo or stop decision from a tie."""
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
            Ka, sa, dJ, cl = box_sweep(x[ia], u[ia], x_ref, u_ref, tau[ia], Q, R, QT, pset)
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
                xn, un = closed_loop_box(x[ln], u[ln], Ka[todo], sa[todo], gam[todo], tau[ln], pset)
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
