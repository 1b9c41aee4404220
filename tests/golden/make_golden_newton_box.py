"""Writes tests/golden/newton_box_task2.npz: the torque-limited task-2 swing-up of four starts at the full horizon,
solved by the NumPy restatement tests/newton_box_ref.py (from that file and oracle/acrobot_np.py alone; about five
minutes of CPU).

    python tests/golden/make_golden_newton_box.py

Setup: the task-2 references (task2_input_fully_actuated.npz, N = 501), tau_max = 18, tol = 5e-3, gamma_0 = 0.1,
beta = 0.7, c = 0.5, max_ls = 20, at most 450 iterations; x0 = 0 and three starts whose joint angles are
rng(0).uniform(-0.5, 0.5, (3, 2)).  tol = 5e-3, not task 2's 1e-4: with the bounds active the Armijo search (Euler
linearisation against RK4 rollouts) stops the solve at max|sigma| of 1e-3 to 2e-3.
Contents: x0 (4,4), tau_max, tol, gamma_0, x (4,501,4), u (4,500,2), cost, n_iter, status, n_rollouts (4,),
clamped (4,500) bool: the clamped stages of each lane's last sweep.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import newton_box_ref as nb  # noqa: E402
from oracle import acrobot_np as onp  # noqa: E402

TAU, TOL, GAMMA0, MAX_ITERS = 18.0, 5e-3, 0.1, 450


def starts():
    x0 = np.zeros((4, 4))
    x0[1:, :2] = np.random.default_rng(0).uniform(-0.5, 0.5, (3, 2))
    return x0


def main():
    x_ref, u_ref, _ = onp.load_task2_refs(os.path.join(HERE, "task2_input_fully_actuated.npz"))
    x0 = starts()
    r = nb.newton_box_solve(x0, x_ref, u_ref, MAX_ITERS, TAU, tol=TOL, gamma_0=GAMMA0)
    print("n_iter", r["n_iter"], "status", r["status"], "rollouts", r["n_rollouts"])
    print("cost", r["cost"], "clamped stages", r["clamped"].sum(1), "max|u1|", np.abs(r["u"][:, :, 1]).max(1))
    print("decision margin", r["margin"])
    assert (r["status"] == nb.CONVERGED).all() and (np.abs(r["u"][:, :, 1]) <= TAU).all()
    np.savez_compressed(os.path.join(HERE, "newton_box_task2.npz"), x0=x0, tau_max=TAU, tol=TOL, gamma_0=GAMMA0,
                        x=r["x"], u=r["u"], cost=r["cost"], n_iter=r["n_iter"].astype(np.int32),
                        status=r["status"].astype(np.int32), n_rollouts=r["n_rollouts"].astype(np.int32),
                        clamped=r["clamped"], margin=r["margin"])


if __name__ == "__main__":
    main()
