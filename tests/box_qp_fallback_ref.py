"""CPU reference (test infrastructure only, NumPy) of the projected-Newton second phase of the torque-limited window QP.

box_qp_ref.solve_active_set solves the window QP exactly when its active set settles, and cycles on some windows.
The QP is strictly convex with a non-empty box, so the minimiser exists; this file restates the fallback that
finishes such a QP (Bertsekas' projected Newton with an Armijo search along the projection arc), as the HIP
kernels run it, on the two formulations of box_qp_ref:

  * newton_riccati     channel 1 of a batch of QPs on the stage data: gradient by the costate pass, Newton target by
                       the clamped Riccati sweep of the current active set, cost of a trial by a linear rollout;
  * newton_condensed   the same iteration on the dense QP  min 1/2 u'H u + u'F x0  of one lane.

One iteration, from a feasible u:
  1. q = gradient of J at u;
  2. stage t is at lo when u_t <= lo_t and q_t > 0, at hi when u_t >= hi_t and q_t < 0, free otherwise;
  3. ubar = the minimiser on that face (clamped stages on their bound), whether or not it respects the other bounds;
  4. u(a) = clip(u + a (ubar - u), lo, hi) for a = 1, 1/2, ... (at most TRIALS): the first a with
     J(u(a)) <= J(u) + SIGMA q'(u(a) - u) is taken; no such a: the QP is unconverged and returns u.  J is quadratic,
     so J(u(a)) - J(u) = q'D + J0(D) with D = u(a) - u and J0 the cost of the linear rollout of D from a zero state;
     the difference is evaluated that way (one rollout, no cancellation: J is 2e9 on a diverged closed loop, and a
     last step may move nothing, which must be accepted);
  5. converged when a = 1 was taken, ubar violated no bound at a free stage and the active set of the new point is
     the one just used: ubar is then stationary on its face with correctly signed multipliers.
solve_hybrid / closed_loop run the active set first and hand the QPs that reach its cap to the fallback; a hybrid
QP's iteration count is active-set sweeps plus Newton iterations, so count > cap exactly when the fallback ran.
"""
from __future__ import annotations

import numpy as np

import box_qp_ref as bq
from oracle import acrobot_np as ref
from oracle import tracking_np as tr

SIGMA = 1e-4
TRIALS = 30
FALLBACK_ITERS = 128
FREE, AT_HI, AT_LO = bq.FREE, bq.AT_HI, bq.AT_LO


def _rollout_cost(x0, u, A, b, Q, r, QT):
    """x0 (..., 4), u (..., T): X (..., T+1, 4) and J = sum x'Qx + r u^2 + x_T'Q_T x_T (channel 1's cost)."""
    T = A.shape[0]
    X = np.zeros(u.shape[:-1] + (T + 1, 4))
    x = np.broadcast_to(x0, u.shape[:-1] + (4,)).copy()
    J = np.zeros(u.shape[:-1])
    for t in range(T):
        X[..., t, :] = x
        J += np.einsum("...i,ij,...j->...", x, Q, x) + r * u[..., t] ** 2
        x = x @ A[t].T + u[..., t, None] * b[t]
    X[..., T, :] = x
    J += np.einsum("...i,ij,...j->...", x, QT, x)
    return X, J


def _gradient(X, u, A, b, Q, r, QT):
    """The reduced-cost gradient q (B, T) by box_update's costate pass."""
    T = A.shape[0]
    q = np.zeros_like(u)
    lam = 2.0 * X[:, T] @ QT.T
    for t in reversed(range(T)):
        q[:, t] = 2.0 * r * u[:, t] + lam @ b[t]
        lam = 2.0 * X[:, t] @ Q.T + lam @ A[t]
    return q


def _active(u, q, lo, hi):
    return np.where((u <= lo) & (q > 0), AT_LO, np.where((u >= hi) & (q < 0), AT_HI, FREE))


def _newton_target(x0, state, A, b, Q, r, QT, lo, hi):
    """box_backward on the stage states, then the forward pass along its own states: ubar (B, T) and whether a free
    stage of ubar lies outside its bounds."""
    Bn, T = state.shape
    k = np.zeros((Bn, T, 4)); d = np.zeros((Bn, T))
    P = np.broadcast_to(QT, (Bn, 4, 4)).copy(); p = np.zeros((Bn, 4))
    for t in reversed(range(T)):
        At, bt = A[t], b[t]
        Pb = P @ bt
        g = r + Pb @ bt
        free = state[:, t] == FREE
        bound = np.where(state[:, t] == AT_HI, hi[t], lo[t])
        kt = np.where(free[:, None], -(Pb @ At) / g[:, None], 0.0)
        dt_ = np.where(free, -(p @ bt) / g, bound)
        Acl = At[None] + bt[None, :, None] * kt[:, None, :]
        p = r * kt * dt_[:, None] + np.einsum("bji,bj->bi", Acl, Pb * dt_[:, None] + p)
        P = Q[None] + r * kt[:, :, None] * kt[:, None, :] + np.einsum("bji,bjk,bkl->bil", Acl, P, Acl)
        P = 0.5 * (P + P.transpose(0, 2, 1))
        k[:, t], d[:, t] = kt, dt_
    x = x0.copy()
    ubar = np.zeros((Bn, T))
    viol = np.zeros(Bn, bool)
    for t in range(T):
        free = state[:, t] == FREE
        u = np.where(free, np.einsum("bi,bi->b", k[:, t], x) + d[:, t], d[:, t])
        viol |= free & ((u > hi[t]) | (u < lo[t]))
        ubar[:, t] = u
        x = x @ A[t].T + u[:, None] * b[t][None]
    return ubar, viol


def newton_riccati(x0, u_start, A, b, Q, r, QT, lo, hi, max_iters=FALLBACK_ITERS):
    """Projected Newton from clip(u_start) for a batch x0 (B,4), u_start (B,T).  Returns u (B,T), X (B,T+1,4), Newton
    iterations (B,), converged (B,) bool and line-search trials (B,)."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    u = np.clip(np.atleast_2d(np.asarray(u_start, float)), lo[None], hi[None])
    Bn = x0.shape[0]
    X = _rollout_cost(x0, u, A, b, Q, r, QT)[0]
    iters = np.zeros(Bn, dtype=int); trials = np.zeros(Bn, dtype=int)
    conv = np.zeros(Bn, bool); active = np.ones(Bn, bool)
    state = np.zeros(u.shape, dtype=int); full = np.zeros(Bn, bool)
    alphas = 0.5 ** np.arange(TRIALS)
    for n in range(max_iters + 1):
        a = np.flatnonzero(active)
        if not a.size:
            break
        q = _gradient(X[a], u[a], A, b, Q, r, QT)
        new = _active(u[a], q, lo[None], hi[None])
        done = full[a] & (new == state[a]).all(axis=1) if n else np.zeros(a.size, bool)
        conv[a[done]] = True
        active[a[done]] = False
        state[a] = new
        if n == max_iters:
            break
        a, q = a[~done], q[~done]
        if not a.size:
            break
        iters[a] += 1
        ubar, viol = _newton_target(x0[a], state[a], A, b, Q, r, QT, lo, hi)
        ua = np.clip(u[a, None, :] + alphas[None, :, None] * (ubar - u[a])[:, None, :], lo[None, None], hi[None, None])
        slope = np.einsum("bt,bat->ba", q, ua - u[a, None, :])
        ok = slope + _rollout_cost(np.zeros(4), ua - u[a, None, :], A, b, Q, r, QT)[1] <= SIGMA * slope
        first = np.where(ok.any(axis=1), ok.argmax(axis=1), TRIALS)
        trials[a] += np.minimum(first + 1, TRIALS)
        took = first < TRIALS
        active[a[~took]] = False                            # no step found: unconverged, returns u
        i, j = np.flatnonzero(took), first[took]
        u[a[i]] = ua[i, j]
        X[a[i]] = _rollout_cost(x0[a[i]], u[a[i]], A, b, Q, r, QT)[0]
        full[a] = took & (first == 0) & ~viol
    return u, X, iters, conv, trials


def newton_condensed(x0, u_start, H, F, lo, hi, max_iters=FALLBACK_ITERS):
    """The same iteration on the dense QP of one lane: u (T,), Newton iterations, converged."""
    f = F @ x0
    u = np.clip(np.asarray(u_start, float), lo, hi)
    state, full = None, False
    for n in range(max_iters + 1):
        q = H @ u + f
        new = _active(u, q, lo, hi)
        if n and full and (new == state).all():
            return u, n, True
        state = new
        if n == max_iters:
            break
        fr = state == FREE
        ubar = np.where(state == AT_HI, hi, lo).astype(float)
        if fr.any():
            ubar[fr] = np.linalg.solve(H[np.ix_(fr, fr)], -(f[fr] + H[np.ix_(fr, ~fr)] @ ubar[~fr]))
        viol = bool((fr & ((ubar > hi) | (ubar < lo))).any())
        for j in range(TRIALS):
            ua = np.clip(u + 0.5 ** j * (ubar - u), lo, hi)
            D = ua - u
            if q @ D + 0.5 * D @ H @ D <= SIGMA * q @ D:
                break
        else:
            return u, n + 1, False
        u, full = ua, j == 0 and not viol
    return u, max_iters, False


def solve_hybrid(x0, A, b, Q, r, QT, lo, hi, max_iters=bq.MAX_QP_ITERS, fallback_iters=FALLBACK_ITERS):
    """Active set, then projected Newton for the lanes at the cap: u (B,T), X (B,T+1,4), iterations (active-set sweeps
    plus Newton iterations), converged.  Lanes that settle within the cap are solve_active_set's, untouched."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    U, X, it, conv = bq.solve_active_set(x0, A, b, Q, r, QT, lo, hi, max_iters)
    hard = np.flatnonzero(~conv)
    if hard.size:
        u, Xh, nit, c, _ = newton_riccati(x0[hard], U[hard], A, b, Q, r, QT, lo, hi, fallback_iters)
        U[hard], X[hard], conv[hard] = u, Xh, c
        it = it.copy()
        it[hard] += nit
    return U, X, it, conv


def solve_window(pb: bq.Problem, w, L, x0, tau_max, max_iters=bq.MAX_QP_ITERS, fallback_iters=FALLBACK_ITERS):
    """box_qp_ref.solve_window with the fallback: U (B,L-1,2), X (B,L,4), iterations, converged."""
    A, Bm, ur = pb.window(w, L)
    lo, hi = bq.bounds(ur, tau_max)
    u1, X, it, conv = solve_hybrid(x0, A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT, lo[:, 1], hi[:, 1], max_iters,
                                   fallback_iters)
    U = np.zeros(u1.shape + (2,))
    U[:, :, 0] = np.clip(0.0, lo[:, 0], hi[:, 0])[None]
    U[:, :, 1] = u1
    return U, X, it, conv


def closed_loop(pb: bq.Problem, x0, tau_max, T_pred=tr.T_PRED, max_iters=bq.MAX_QP_ITERS,
                fallback_iters=FALLBACK_ITERS):
    """box_qp_ref.closed_loop with every QP solved the hybrid way: x, u, qp_iters, unconverged."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    Bn, N = x0.shape[0], pb.x_ref.shape[0]
    x = np.zeros((Bn, N, 4)); u = np.zeros((Bn, N - 1, 2))
    qp_iters = np.zeros((Bn, N - 1), dtype=np.int32); unconv = np.zeros(Bn, dtype=np.int32)
    x[:, 0] = x0
    for s in range(N - 1):
        U, _, it, conv = solve_window(pb, s, T_pred, x[:, s] - pb.x_ref[s], tau_max, max_iters, fallback_iters)
        f = pb.u_ref[s]
        lo, hi = bq.bounds(f, tau_max)
        for c in range(2):
            u[:, s, c] = bq.apply_limit(f[c], U[:, 0, c], lo[c], hi[c], tau_max)
        qp_iters[:, s] = it
        unconv += ~conv
        x[:, s + 1] = ref.rk4(x[:, s], u[:, s])
    return x, u, qp_iters, unconv
