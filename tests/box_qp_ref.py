"""CPU reference (test infrastructure only, NumPy) of the torque-limited MPC window QP.

The window QP of solver_mpc with the torque limit on (trajectory_tracking.py:87-114), local stage index t:

    min  sum_{t<L-1} (x_t'Q x_t + u_t'R u_t) + x_{L-1}'Q_T x_{L-1}
    s.t. x_{t+1} = A_t x_t + B_t u_t,  x_0 given,  -tau_max <= u_t + u_ref_t <= tau_max  (t < L-1)

B_t's column 0 is exactly zero for the acrobot (tau1 is unactuated), so channel 0 separates
(u_t[0] = clip(0, lo, hi)) and channel 1 is a scalar-input LQ problem with a box: b = B_t[:, 1], r = R[1, 1].

Two independent formulations of channel 1, plus a certificate that depends on neither:
  * solve_active_set   primal-dual active set over a clamped Riccati sweep, vectorised over lanes (the method
                       of the HIP kernels, restated in NumPy);
  * solve_condensed    the condensed dense QP  min 1/2 u'H u + u'F x0  over the box, the same active-set rule
                       with a dense solve of the free block of H per iteration;
  * kkt_residual       max |u - clip(u - (H u + F x0) / diag(H), lo, hi)|: zero exactly at the minimiser.
Model and trajectory come from oracle.tracking_np and tests/golden/tracking.npz.
"""
from __future__ import annotations

import numpy as np

from oracle import acrobot_np as ref
from oracle import tracking_np as tr

TAU_MAX = 18.0
MAX_QP_ITERS = 32
FREE, AT_HI, AT_LO = 0, 1, -1


class Problem:
    """Stage linearisations of a reference trajectory, the pad stage and Q_T = P_inf (solve_mpc_tracking :14-40)."""

    def __init__(self, x_ref, u_ref, Q=tr.Q_MPC, R=tr.R_MPC):
        self.x_ref = np.asarray(x_ref, float)
        self.u_ref = np.asarray(u_ref, float)[: self.x_ref.shape[0] - 1]
        self.S = self.u_ref.shape[0]
        self.A, self.B = tr.linearize_along(self.x_ref, self.u_ref)
        A_f, B_f = ref.discretize(*ref.jacobians(tr.X_F[None], tr.U_F[None]))
        self.A_f, self.B_f = A_f[0], B_f[0]
        self.Q, self.R = np.asarray(Q, float), np.asarray(R, float)
        self.QT, _ = tr.compute_P_inf(self.A_f, self.B_f, self.Q, self.R)
        assert np.abs(self.B[:, :, 0]).max() == 0.0 and np.abs(self.B_f[:, 0]).max() == 0.0

    def window(self, w, L):
        """Stages w .. w+L-2 of control step w (pad past the end): A (L-1,4,4), B (L-1,4,2), u_ref (L-1,2)."""
        idx = np.arange(w, w + L - 1)
        inside = idx < self.S
        i = np.minimum(idx, self.S - 1)
        A = np.where(inside[:, None, None], self.A[i], self.A_f)
        B = np.where(inside[:, None, None], self.B[i], self.B_f)
        ur = np.where(inside[:, None], self.u_ref[i], tr.U_F)
        return A, B, ur


def bounds(ur, tau_max):
    """lo, hi (L-1, 2) of u_t: -tau_max - u_ref_t <= u_t <= tau_max - u_ref_t."""
    return -tau_max - ur, tau_max - ur


def solve_active_set(x0, A, b, Q, r, QT, lo, hi, max_iters=MAX_QP_ITERS):
    """Channel 1 of the window QP for a batch x0 (B,4): stages A (L-1,4,4), b (L-1,4), bounds lo, hi (L-1,).
    Returns u (B,L-1), X (B,L,4), iterations (B,), converged (B,) bool.  Converged: the active set settled in fewer
    than max_iters sweeps, so a lane is unconverged exactly when its iteration count is max_iters (a last sweep that
    happens to settle is still flagged; its clipped iterate is then the minimiser itself).  An unconverged lane
    returns clip(u, lo, hi) of its last iterate and that iterate's predicted states."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    Bn, T = x0.shape[0], A.shape[0]
    state = np.zeros((Bn, T), dtype=int)
    done = np.zeros(Bn, bool)
    iters = np.zeros(Bn, dtype=int)
    U = np.zeros((Bn, T)); X = np.zeros((Bn, T + 1, 4))
    for it in range(max_iters):
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
        Xn = np.zeros_like(X); Un = np.zeros_like(U)
        for t in range(T):
            Xn[:, t] = x
            u = np.where(state[:, t] == FREE, np.einsum("bi,bi->b", k[:, t], x) + d[:, t], d[:, t])
            Un[:, t] = u
            x = x @ A[t].T + u[:, None] * b[t][None]
        Xn[:, T] = x
        lam = 2.0 * x @ QT.T
        new = state.copy()
        for t in reversed(range(T)):
            q = 2.0 * r * Un[:, t] + lam @ b[t]
            s = state[:, t]
            nt = np.where(s == FREE, np.where(Un[:, t] > hi[t], AT_HI, np.where(Un[:, t] < lo[t], AT_LO, FREE)),
                          np.where(s == AT_HI, np.where(q < 0, AT_HI, FREE), np.where(q > 0, AT_LO, FREE)))
            new[:, t] = nt
            lam = 2.0 * Xn[:, t] @ Q.T + lam @ A[t]
        act = ~done
        U[act], X[act] = Un[act], Xn[act]
        iters[act] = it + 1
        changed = (new != state).any(axis=1)
        if it + 1 < max_iters:                  # a QP whose sweep count reaches the cap is reported unconverged
            done |= ~changed
        state[~done] = new[~done]
        if done.all():
            break
    U[~done] = np.clip(U[~done], lo[None], hi[None])
    return U, X, iters, done


def condense(A, b, Q, r, QT):
    """H (T,T), F (T,4) of channel 1: J = 1/2 u'H u + u'F x0 + const, gradient H u + F x0."""
    T = A.shape[0]
    Phi = np.zeros((T + 1, 4, 4)); Phi[0] = np.eye(4)
    for t in range(T):
        Phi[t + 1] = A[t] @ Phi[t]
    G = np.zeros((T + 1, 4, T))                     # x_t = Phi_t x0 + G_t u
    for s in range(T):
        v = b[s].copy()
        G[s + 1, :, s] = v
        for t in range(s + 1, T):
            v = A[t] @ v
            G[t + 1, :, s] = v
    H = 2.0 * r * np.eye(T); F = np.zeros((T, 4))
    for t in range(T + 1):
        W = QT if t == T else Q
        H += 2.0 * G[t].T @ W @ G[t]
        F += 2.0 * G[t].T @ W @ Phi[t]
    return 0.5 * (H + H.T), F, Phi, G


def solve_condensed(x0, H, F, lo, hi, max_iters=MAX_QP_ITERS):
    """The same primal-dual active-set rule on the dense QP of one lane x0 (4,): u (T,), iterations, converged."""
    T = H.shape[0]
    f = F @ x0
    state = np.zeros(T, dtype=int)
    u = np.zeros(T)
    for it in range(max_iters):
        fr = state == FREE
        u = np.where(state == AT_HI, hi, lo).astype(float)
        u[fr] = np.linalg.solve(H[np.ix_(fr, fr)], -(f[fr] + H[np.ix_(fr, ~fr)] @ u[~fr])) if fr.any() else u[fr]
        q = H @ u + f
        new = np.where(fr, np.where(u > hi, AT_HI, np.where(u < lo, AT_LO, FREE)),
                       np.where(state == AT_HI, np.where(q < 0, AT_HI, FREE), np.where(q > 0, AT_LO, FREE)))
        if (new == state).all() and it + 1 < max_iters:
            return u, it + 1, True
        state = new
    return np.clip(u, lo, hi), max_iters, False


def kkt_residual(u, x0, H, F, lo, hi):
    """max |u - clip(u - (H u + F x0) / diag(H), lo, hi)| (solver-independent optimality certificate)."""
    g = H @ u + F @ x0
    return float(np.abs(u - np.clip(u - g / np.diag(H), lo, hi)).max())


def solve_window(pb: Problem, w, L, x0, tau_max=TAU_MAX, max_iters=MAX_QP_ITERS):
    """Both channels of window w for a batch x0 (B,4): U (B,L-1,2), X (B,L,4), iterations, converged."""
    A, Bm, ur = pb.window(w, L)
    lo, hi = bounds(ur, tau_max)
    u1, X, it, conv = solve_active_set(x0, A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT, lo[:, 1], hi[:, 1], max_iters)
    U = np.zeros(u1.shape + (2,))
    U[:, :, 0] = np.clip(0.0, lo[:, 0], hi[:, 0])[None]
    U[:, :, 1] = u1
    return U, X, it, conv


def apply_limit(f, u0, lo, hi, tau_max):
    """The applied torque u_ref + u_0 of one channel: a first control on its bound is the limit itself (hi + u_ref is
    tau_max only up to rounding), and the sum is kept inside the limit."""
    v = np.where(u0 >= hi, tau_max, np.where(u0 <= lo, -tau_max, f + u0))
    return np.where(v > tau_max, tau_max, np.where(v < -tau_max, -tau_max, v))


def closed_loop(pb: Problem, x0, tau_max=TAU_MAX, T_pred=tr.T_PRED, max_iters=MAX_QP_ITERS):
    """solve_mpc_tracking :43-67 with the limit on, for a batch x0 (B,4): x (B,N,4), u (B,N-1,2),
    qp_iters (B,N-1), unconverged (B,)."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    Bn, N = x0.shape[0], pb.x_ref.shape[0]
    x = np.zeros((Bn, N, 4)); u = np.zeros((Bn, N - 1, 2))
    qp_iters = np.zeros((Bn, N - 1), dtype=np.int32); unconv = np.zeros(Bn, dtype=np.int32)
    x[:, 0] = x0
    for s in range(N - 1):
        U, _, it, conv = solve_window(pb, s, T_pred, x[:, s] - pb.x_ref[s], tau_max, max_iters)
        f = pb.u_ref[s]
        lo, hi = bounds(f, tau_max)
        for c in range(2):
            u[:, s, c] = apply_limit(f[c], U[:, 0, c], lo[c], hi[c], tau_max)
        qp_iters[:, s] = it
        unconv += ~conv
        x[:, s + 1] = ref.rk4(x[:, s], u[:, s])
    return x, u, qp_iters, unconv
