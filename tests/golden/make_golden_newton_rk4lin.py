"""Writes tests/golden/newton_rk4lin_task2.npz: the torque-limited task-2 swing-up of two starts at the full horizon on
the RK4-exact linearisation, solved by the NumPy restatement tests/newton_rk4lin_ref.py (from that file,
tests/newton_box_ref.py and oracle/acrobot_np.py alone; about twelve minutes of CPU).

    python tests/golden/make_golden_newton_rk4lin.py

Setup: the task-2 references (task2_input_fully_actuated.npz, N = 501), tau_max = 16, tol = 1e-5, gamma_0 = 0.1,
beta = 0.7, c = 0.5, max_ls = 20, at most 450 iterations; x0 = [0, 0, 0, 0] and [0.05, -0.05, 0, 0].  On the Euler
linearisation this setup ends LS_FAILED at max|sigma| of 3.3e-4 / 1.8e-4.
Contents: x0 (2,4), tau_max, tol, gamma_0, x (2,501,4), u (2,500,2), cost, n_iter, status, n_rollouts (2,),
clamped (2,500) bool: the clamped stages of each lane's last sweep, smax (2,): max|sigma| of that sweep, and margin (2,):
the smallest relative distance of any Armijo or stop decision from a tie.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import newton_rk4lin_ref as nr  # noqa: E402
from oracle import acrobot_np as onp  # noqa: E402

TAU, TOL, GAMMA0, MAX_ITERS = 16.0, 1e-5, 0.1, 450
X0 = np.array([[0.0, 0.0, 0.0, 0.0], [0.05, -0.05, 0.0, 0.0]])


def main():
    x_ref, u_ref, _ = onp.load_task2_refs(os.path.join(HERE, "task2_input_fully_actuated.npz"))
    r = nr.newton_rk4lin_solve(X0, x_ref, u_ref, MAX_ITERS, TAU, tol=TOL, gamma_0=GAMMA0)
    smax = np.abs(r["sigma"]).max((1, 2))
    print("n_iter", r["n_iter"], "status", r["status"], "rollouts", r["n_rollouts"], "max|sigma|", smax)
    print("cost", r["cost"], "clamped stages", r["clamped"].sum(1), "max|u1|", np.abs(r["u"][:, :, 1]).max(1))
    print("decision margin", r["margin"])
    assert (r["status"] == nr.CONVERGED).all() and (np.abs(r["u"][:, :, 1]) <= TAU).all()
    np.savez_compressed(os.path.join(HERE, "newton_rk4lin_task2.npz"), x0=X0, tau_max=TAU, tol=TOL, gamma_0=GAMMA0,
                        x=r["x"], u=r["u"], cost=r["cost"], n_iter=r["n_iter"].astype(np.int32),
                        status=r["status"].astype(np.int32), n_rollouts=r["n_rollouts"].astype(np.int32),
                        clamped=r["clamped"], smax=smax, margin=r["margin"])


if __name__ == "__main__":
    main()
