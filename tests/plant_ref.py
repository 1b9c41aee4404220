"""Yardstick of the mismatched-plant tests: the per-lane trackers' own yardsticks (tests/lqr_lanes_ref.py,
tests/mpc_lanes_ref.py, tests/mpc_box_lanes_ref.py) with the plant step of closed loop (b, p) on that loop's own
parameter set.  The controller side is theirs unchanged: gains by oracle.tracking_np.solve_LQR_tracking / mpc_gains
on set 1, the window QP and the limit by box_qp_ref.solve_window / apply_limit; only x_{t+1} = rk4(x_t, u_t, pset=key)
differs.  Test infrastructure only; nothing under oracle/ is edited: the two extra sets are registered in the module
dict oracle.acrobot_np.PARAM_SETS at import.

Four keys and no more: the oracle caches four lambdified models and would rebuild one per step with a fifth."""
import numpy as np

import box_qp_ref as bq
from lqr_lanes_ref import summaries
from oracle import acrobot_np as ref
from oracle import tracking_np as otr

ref.PARAM_SETS["heavy"] = dict(ref.PARAM_SETS[1], m2=1.1, I2=0.363)     # m2 + 10 %, I2 + 10 %
ref.PARAM_SETS["sticky"] = dict(ref.PARAM_SETS[1], f1=1.5, f2=1.5)      # joint friction + 50 %
KEYS = (1, "heavy", "sticky", 2)
NAMES = ("m1", "m2", "l1", "lc1", "l2", "lc2", "I1", "I2", "g", "f1", "f2")   # params.PARAM_NAMES' order


def starts(x, P):
    """x0 (B,P,4): start p of lane b is mpc_box_lanes_ref.starts(x)[b][p % 3]."""
    s = np.asarray(x, dtype=float)[:, 0]
    three = np.stack([s, s + 0.1, s + np.array([-0.05, 0.05, 0.1, -0.1])], axis=1)
    return three[:, np.arange(P) % 3]


def keys_of(B, P):
    """The plant of (b, p) is KEYS[(b + p) % 4]: a swapped or transposed table index cannot pass."""
    return [[KEYS[(b + p) % 4] for p in range(P)] for b in range(B)]


def params_of(keys):
    """The (B,P,11) parameter array of a (B,P) nest of keys, to hand to ``plant=``."""
    return np.array([[[ref.PARAM_SETS[k][n] for n in NAMES] for k in row] for row in keys], dtype=np.float64)


def plant_step(x, u, keys):
    """x (B,P,4), u (B,P,2) -> x_next (B,P,4): every (lane, start) of one key through one rk4 call."""
    kk = np.array([[KEYS.index(k) for k in row] for row in keys])
    out = np.empty_like(x)
    for i, key in enumerate(KEYS):
        sel = kk == i
        if sel.any():
            out[sel] = ref.rk4(x[sel], u[sel], pset=key)
    return out


def _feedback_loop(x_opt, u_opt, K, x0, keys):
    """simulate_tracking's loop (its feedback expression, lane by lane) with plant_step as the plant."""
    B, N = x_opt.shape[:2]
    P = x0.shape[1]
    x = np.zeros((B, P, N, 4)); u = np.zeros((B, P, N - 1, 2))
    x[:, :, 0] = x0
    with np.errstate(all="ignore"):                     # a diverging plant overflows: an outcome, not an error
        for t in range(N - 1):
            for b in range(B):
                u[b, :, t] = u_opt[b, t] + np.einsum("ij,bj->bi", K[b, t], x[b, :, t] - x_opt[b, t])
            x[:, :, t + 1] = plant_step(x[:, :, t], u[:, :, t], keys)
    out = {"K": K, "x": x, "u": u}
    with np.errstate(all="ignore"):
        out.update(summaries(x, u, x_opt))
    return out


def lqr_ref(x_opt, u_opt, x0, keys, Q=otr.Q_REG, R=otr.R_REG, QT=otr.QT_REG):
    """lqr_lanes_ref.lanes_ref with the plant of (b, p) on keys[b][p]: dict of K, x, u and the three summaries."""
    x_opt, u_opt, x0 = (np.asarray(a, dtype=float) for a in (x_opt, u_opt, x0))
    K = np.array([otr.solve_LQR_tracking(x_opt[b], u_opt[b], Q, R, QT) for b in range(x_opt.shape[0])])
    return _feedback_loop(x_opt, u_opt, K, x0, keys)


def mpc_ref(x_opt, u_opt, x0, keys, T_pred=otr.T_PRED, Q=otr.Q_MPC, R=otr.R_MPC):
    """mpc_lanes_ref.lanes_ref (no torque limit) with the plant of (b, p) on keys[b][p]."""
    x_opt, u_opt, x0 = (np.asarray(a, dtype=float) for a in (x_opt, u_opt, x0))
    K = np.array([otr.mpc_gains(x_opt[b], u_opt[b], T_pred, Q, R)[0] for b in range(x_opt.shape[0])])
    return _feedback_loop(x_opt, u_opt, K, x0, keys)


def box_ref(x_opt, u_opt, x0, keys, tau_max=bq.TAU_MAX, T_pred=otr.T_PRED, max_iters=bq.MAX_QP_ITERS):
    """mpc_box_lanes_ref.lanes_ref (box_qp_ref.closed_loop's steps, lane by lane) with the plant of (b, p) on
    keys[b][p]: dict of x (B,P,N,4), u (B,P,N-1,2), qp_iters (B,P,N-1) int32, unconverged (B,P) int32."""
    x_opt, u_opt, x0 = (np.asarray(a, dtype=float) for a in (x_opt, u_opt, x0))
    B, N = x_opt.shape[:2]
    P = x0.shape[1]
    pbs = [bq.Problem(x_opt[b], u_opt[b]) for b in range(B)]
    x = np.zeros((B, P, N, 4)); u = np.zeros((B, P, N - 1, 2))
    it = np.zeros((B, P, N - 1), dtype=np.int32); unconv = np.zeros((B, P), dtype=np.int32)
    x[:, :, 0] = x0
    for s in range(N - 1):
        for b, pb in enumerate(pbs):
            U, _, its, conv = bq.solve_window(pb, s, T_pred, x[b, :, s] - pb.x_ref[s], tau_max, max_iters)
            f = pb.u_ref[s]
            lo, hi = bq.bounds(f, tau_max)
            for c in range(2):
                u[b, :, s, c] = bq.apply_limit(f[c], U[:, 0, c], lo[c], hi[c], tau_max)
            it[b, :, s] = its
            unconv[b] += ~conv
        x[:, :, s + 1] = plant_step(x[:, :, s], u[:, :, s], keys)
    return {"x": x, "u": u, "qp_iters": it, "unconverged": unconv}


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
