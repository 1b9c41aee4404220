"""Yardstick of the per-lane-model tests (test helper, not a test): the torque-limited Newton restatement
tests/newton_box_ref.py and the reference's LQR recursion, each lane on its own parameter set.

Nothing under oracle/ is edited.  The sets are tests/plant_ref.py's four keys (1, "heavy", "sticky", 2: it registers
the two extra ones in oracle.acrobot_np.PARAM_SETS at import), and no more: the oracle caches four lambdified models.
Lanes are solved key by key, every lane of one key in one vectorised call, so a lane's numbers are those of
newton_box_ref.newton_box_solve(..., pset=key) on that lane alone (its arithmetic is per lane).
"""
import numpy as np

import newton_box_ref as nb
import plant_ref as pr
from oracle import acrobot_np as onp
from oracle import tracking_np as otr

KEYS, NAMES = pr.KEYS, pr.NAMES
short_setup = nb.short_setup


def keys_of(B):
    """Lane b plans on KEYS[b % 4]: a shifted table index cannot pass."""
    return [KEYS[b % 4] for b in range(B)]


def params_of(keys):
    """The (B,11) parameter array of a list of keys, to hand to ``models=``."""
    return np.array([[onp.PARAM_SETS[k][n] for n in NAMES] for k in keys], dtype=np.float64)


def newton_models_solve(x0, x_ref, u_ref, max_iters, tau_max, keys, **kw):
    """newton_box_ref.newton_box_solve with lane b on parameter set keys[b]; tau_max a number or (B,).  Returns its
    per-lane fields (x, u, K, sigma, n_iter, status, cost, n_rollouts, clamped, margin) stacked in lane order."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    B = x0.shape[0]
    tau = np.broadcast_to(np.asarray(tau_max, float), (B,))
    out = {}
    for key in dict.fromkeys(keys):
        ln = np.array([b for b in range(B) if keys[b] == key])
        r = nb.newton_box_solve(x0[ln], x_ref, u_ref, max_iters, tau[ln], pset=key, **kw)
        for f in ("x", "u", "K", "sigma", "n_iter", "status", "cost", "n_rollouts", "clamped", "margin"):
            out.setdefault(f, np.zeros((B,) + r[f].shape[1:], dtype=r[f].dtype))[ln] = r[f]
    return out


def solve_LQR_tracking(x_opt, u_opt, Q=otr.Q_REG, R=otr.R_REG, QT=otr.QT_REG, pset=1):
    """oracle.tracking_np.solve_LQR_tracking (trajectory_tracking.py:170-203) linearised on parameter set ``pset``:
    its own statements with oracle.acrobot_np.jacobians(x, u, pset) in linearize_along's place -> K (N-1, 2, 4)."""
    S = u_opt.shape[0]
    A, B = onp.discretize(*onp.jacobians(x_opt[:S], u_opt[:S], pset), otr.DT)
    P = QT.copy()
    K = np.zeros((S, 2, 4))
    for t in reversed(range(S)):
        K[t], P = otr.riccati_step(A[t], B[t], P, Q, R)
    return K


def lqr_gains(x_opt, u_opt, keys, **kw):
    """K (B,N-1,2,4): lane b's gains by solve_LQR_tracking on keys[b]."""
    return np.array([solve_LQR_tracking(np.asarray(x_opt[b], float), np.asarray(u_opt[b], float), pset=keys[b], **kw)
                     for b in range(len(keys))])
