"""Yardstick of the per-lane torque-limited MPC tracking tests: the NumPy reference of the shared-reference path
(tests/box_qp_ref.py: the active set, pinned to the condensed solve and the KKT certificate by
tests/test_mpc_box_host.py) applied lane by lane, every lane along its own trajectory.  Test infrastructure only."""
import numpy as np

import box_qp_ref as bq
from oracle import tracking_np as otr


def starts(x):
    """The three starts per lane of tests/test_gpu_mpc_lanes.py: the trajectory's own, + 0.1, + (-0.05, 0.05, 0.1,
    -0.1)."""
    s = np.asarray(x, dtype=float)[:, 0]
    return np.stack([s, s + 0.1, s + np.array([-0.05, 0.05, 0.1, -0.1])], axis=1)


def lanes_ref(x_opt, u_opt, x0, tau_max=bq.TAU_MAX, T_pred=otr.T_PRED, max_iters=bq.MAX_QP_ITERS):
    """x_opt (B,N,4), u_opt (B,N-1,2), x0 (B,P,4) -> dict of x (B,P,N,4), u (B,P,N-1,2), qp_iters (B,P,N-1) int32,
    unconverged (B,P) int32: box_qp_ref.closed_loop on box_qp_ref.Problem(x_opt[b], u_opt[b]), lane by lane."""
    x_opt, u_opt, x0 = (np.asarray(a, dtype=float) for a in (x_opt, u_opt, x0))
    B, N = x_opt.shape[:2]
    P = x0.shape[1]
    out = {"x": np.zeros((B, P, N, 4)), "u": np.zeros((B, P, N - 1, 2)),
           "qp_iters": np.zeros((B, P, N - 1), dtype=np.int32), "unconverged": np.zeros((B, P), dtype=np.int32)}
    for b in range(B):
        pb = bq.Problem(x_opt[b], u_opt[b])
        out["x"][b], out["u"][b], out["qp_iters"][b], out["unconverged"][b] = bq.closed_loop(
            pb, x0[b], tau_max, T_pred, max_iters)
    return out


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
