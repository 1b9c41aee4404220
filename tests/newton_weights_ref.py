"""Yardstick of the per-lane-weights tests (test helper, not a test): the torque-limited Newton restatement
tests/newton_box_ref.py, each lane under its own Q, R, Q_T.

Nothing under oracle/ is edited.  Four sets, scaled from the defaults; lane b takes SETS[b % 4].  Lanes are solved set by
set, every lane of one set in one vectorised call, so a lane's numbers are those of
newton_box_ref.newton_box_solve(..., Q=, R=, QT=) on that lane alone (its arithmetic is per lane).

On the short setup (newton_box_ref.short_setup: N = 41, five starts; tol 1e-4, beta 0.7, c 0.5, gamma_0 0.5, max_ls 20,
60 iterations) with that assignment all five lanes converge at tau = inf in 20, 18, 20, 21, 20 iterations, and at
tau = 2 in 17 iterations each with 26-33 clamped stages; the tightest Armijo or stop margin of any lane is 3.9e-9, far
above the tie threshold of 3e-12.  (The default set on start 1 at tau = inf would end LS_FAILED at a margin of 3e-14,
a rounding tie: the assignment puts "stiff" there.)
"""
import numpy as np

import newton_box_ref as nb
from oracle import acrobot_np as onp

SETS = ("default", "stiff", "cheap", "soft_end")
short_setup = nb.short_setup


def diag_of(name):
    """(Q (4,), R (2,), QT (4,)) of a set: the defaults' diagonals, scaled."""
    Q, R, QT = (np.diag(M).astype(np.float64) for M in (onp.Q_DEFAULT, onp.R_DEFAULT, onp.QT_DEFAULT))
    if name == "stiff":
        Q = 4.0 * Q
    elif name == "cheap":
        R = R * np.array([1.0, 0.25])
    elif name == "soft_end":
        QT = 0.1 * QT
    elif name != "default":
        raise KeyError(name)
    return Q, R, QT


def names_of(B):
    """Lane b plans under SETS[b % 4]: a shifted table index cannot pass."""
    return [SETS[b % 4] for b in range(B)]


def rows_of(names):
    """The (B,10) array of a list of set names, rows Q[4], R[2], QT[4], to hand to ``weights=``."""
    return np.array([np.concatenate(diag_of(n)) for n in names], dtype=np.float64)


def newton_weights_solve(x0, x_ref, u_ref, max_iters, tau_max, names, **kw):
    """newton_box_ref.newton_box_solve with lane b under set names[b]; tau_max a number or (B,).  Returns its per-lane
    fields (x, u, K, sigma, n_iter, status, cost, n_rollouts, clamped, margin) stacked in lane order."""
    x0 = np.atleast_2d(np.asarray(x0, float))
    B = x0.shape[0]
    tau = np.broadcast_to(np.asarray(tau_max, float), (B,))
    out = {}
    for name in dict.fromkeys(names):
        ln = np.array([b for b in range(B) if names[b] == name])
        Q, R, QT = (np.diag(v) for v in diag_of(name))
        r = nb.newton_box_solve(x0[ln], x_ref, u_ref, max_iters, tau[ln], Q=Q, R=R, QT=QT, **kw)
        for f in ("x", "u", "K", "sigma", "n_iter", "status", "cost", "n_rollouts", "clamped", "margin"):
            out.setdefault(f, np.zeros((B,) + r[f].shape[1:], dtype=r[f].dtype))[ln] = r[f]
    return out
