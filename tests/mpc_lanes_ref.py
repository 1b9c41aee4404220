"""Yardstick of the per-lane MPC tracking tests: the committed NumPy oracle (oracle.tracking_np, pinned to the
reference's own functions by tests/test_tracking.py) applied lane by lane.  Test infrastructure only."""
import numpy as np

from oracle import tracking_np as otr
from lqr_lanes_ref import summaries


def gains_ref(x_opt, u_opt, T_pred=otr.T_PRED, Q=otr.Q_MPC, R=otr.R_MPC):
    """x_opt (B,N,4), u_opt (B,N-1,2) -> (K0 (B,N-1,2,4), QT (4,4)): mpc_gains on each lane's own trajectory (the
    first gain of every control step's window, the pad at x_f past the lane's last stage, from Q_T = P_inf)."""
    x_opt, u_opt = np.asarray(x_opt, dtype=float), np.asarray(u_opt, dtype=float)
    B, N = x_opt.shape[:2]
    K = np.zeros((B, N - 1, 2, 4))
    QT = None
    for b in range(B):
        K[b], QT = otr.mpc_gains(x_opt[b], u_opt[b], T_pred, Q, R)
    return K, QT


def lanes_ref(x_opt, u_opt, x0, T_pred=otr.T_PRED, Q=otr.Q_MPC, R=otr.R_MPC):
    """x_opt (B,N,4), u_opt (B,N-1,2), x0 (B,P,4) -> dict of K (B,N-1,2,4), QT, x (B,P,N,4), u (B,P,N-1,2) and the
    three summaries (B,P): mpc_gains / simulate_tracking (solve_mpc_tracking's closed loop) on each lane's own
    trajectory."""
    x_opt, u_opt, x0 = (np.asarray(a, dtype=float) for a in (x_opt, u_opt, x0))
    B, N = x_opt.shape[:2]
    P = x0.shape[1]
    K, QT = gains_ref(x_opt, u_opt, T_pred, Q, R)
    x = np.zeros((B, P, N, 4)); u = np.zeros((B, P, N - 1, 2))
    for b in range(B):
        x[b], u[b] = otr.simulate_tracking(x_opt[b], u_opt[b], K[b], x0[b])
    out = {"K": K, "QT": QT, "x": x, "u": u}
    out.update(summaries(x, u, x_opt))
    return out


def window(x_opt, u_opt, t, T_pred=otr.T_PRED):
    """(Aw, Bw) of control step t of one lane (x_opt (N,4), u_opt (N-1,2)): the stage lists solver_mpc gets."""
    A, B = otr.linearize_along(np.asarray(x_opt, dtype=float), np.asarray(u_opt, dtype=float))
    A_f, B_f = otr.ref.discretize(*otr.ref.jacobians(otr.X_F[None], otr.U_F[None]))
    return list(otr.mpc_windows(A, B, A_f[0], B_f[0], T_pred, t + 1))[t]
