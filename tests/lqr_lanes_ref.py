"""Yardstick of the per-lane LQR tracking tests: the committed NumPy oracle (oracle.tracking_np, pinned to the
reference's own functions by tests/test_tracking.py) applied lane by lane.  Test infrastructure only."""
import numpy as np

from oracle import tracking_np as otr


def lanes_ref(x_opt, u_opt, x0, Q=otr.Q_REG, R=otr.R_REG, QT=otr.QT_REG):
    """x_opt (B,N,4), u_opt (B,N-1,2), x0 (B,P,4) -> dict of K (B,N-1,2,4), x (B,P,N,4), u (B,P,N-1,2) and the three
    summaries (B,P): solve_LQR_tracking / simulate_tracking on each lane's own trajectory."""
    x_opt, u_opt, x0 = (np.asarray(a, dtype=float) for a in (x_opt, u_opt, x0))
    B, N = x_opt.shape[:2]
    P = x0.shape[1]
    K = np.zeros((B, N - 1, 2, 4)); x = np.zeros((B, P, N, 4)); u = np.zeros((B, P, N - 1, 2))
    for b in range(B):
        K[b] = otr.solve_LQR_tracking(x_opt[b], u_opt[b], Q, R, QT)
        x[b], u[b] = otr.simulate_tracking(x_opt[b], u_opt[b], K[b], x0[b])
    out = {"K": K, "x": x, "u": u}
    out.update(summaries(x, u, x_opt))
    return out


def summaries(x, u, x_opt):
    """err_final = |x_{N-1} - x_opt_{N-1}|_inf, err_max = max_t |x_t - x_opt_t|_inf, u_max = max_t |u_t[1]| of
    x (B,P,N,4), u (B,P,N-1,2) against x_opt (B,N,4); NaN-propagating, as np.max is."""
    e = np.abs(x - x_opt[:, None])
    return {"err_final": e[:, :, -1].max(-1), "err_max": e.max((-1, -2)), "u_max": np.abs(u[..., 1]).max(-1)}
