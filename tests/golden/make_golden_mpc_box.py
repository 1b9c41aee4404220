"""Writes tests/golden/mpc_box.npz: recorded output of the CPU reference tests/box_qp_ref.py (NumPy only).

No reference program can produce this fixture (the reference's torque-limited QP needs casadi / IPOPT); what ties it
to the QP is the solver-independent KKT certificate (box_qp_ref.kkt_residual), stored per window case and re-checked
by tests/test_mpc_box_host.py.

    python tests/golden/make_golden_mpc_box.py

Contents (tau_max = 18, T_pred = 75, the headline optimal trajectory of tracking.npz):
  closed loop   x0 (6,4) = x_opt[0] + [dx,-dx,0,0], dx in DX;  x (6,501,4), u (6,500,2), qp_iters (6,500)
  windows       win_w (4,) = 101, 170, 180, 480;  win_x0 (4,65,4): lanes 0-5 the closed-loop lanes' tracking error at
                that step, lanes 6-64 random (scaled so every QP converges; lane 6 is picked for its bound pattern);
                win_U (4,8,74,2), win_X (4,8,75,4), win_iters (4,8), win_kkt (4,8) of lanes 0-7
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import box_qp_ref as bq  # noqa: E402

DX = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3)
WINDOWS = (101, 170, 180, 480)
SCALE = {101: 2.0, 170: 2.0, 180: 1.0, 480: 0.2}      # random x0 = U(-1,1) * [0.3,0.3,1,1] * SCALE
NB, NFULL, L = 65, 8, 75


def main():
    trk = np.load(os.path.join(HERE, "tracking.npz"))
    pb = bq.Problem(trk["x_opt"], trk["u_opt"])
    x0 = np.array([trk["x_opt"][0] + np.array([d, -d, 0.0, 0.0]) for d in DX])
    x, u, qp_iters, unconv = bq.closed_loop(pb, x0, bq.TAU_MAX, L)
    assert not unconv.any()
    rng = np.random.default_rng(20)
    win_x0 = np.zeros((len(WINDOWS), NB, 4))
    win_U = np.zeros((len(WINDOWS), NFULL, L - 1, 2)); win_X = np.zeros((len(WINDOWS), NFULL, L, 4))
    win_iters = np.zeros((len(WINDOWS), NFULL), dtype=np.int32); win_kkt = np.zeros((len(WINDOWS), NFULL))
    for i, w in enumerate(WINDOWS):
        A, Bm, ur = pb.window(w, L)
        lo, hi = bq.bounds(ur, bq.TAU_MAX)
        r = rng.uniform(-1.0, 1.0, (NB - 6, 4)) * np.array([0.3, 0.3, 1.0, 1.0]) * SCALE[w]
        U, _, _, conv = bq.solve_window(pb, w, L, r)
        assert conv.all(), (w, int(conv.sum()))
        nh = (U[:, :, 1] >= hi[:, 1]).sum(1); nl = (U[:, :, 1] <= lo[:, 1]).sum(1)
        pick = np.flatnonzero((nh > 0) & (nl > 0))            # a lane with both bounds active, if there is one
        if pick.size:
            r[[0, pick[0]]] = r[[pick[0], 0]]
        win_x0[i, :6] = x[:, w] - trk["x_opt"][w]
        win_x0[i, 6:] = r
        U, X, it, conv = bq.solve_window(pb, w, L, win_x0[i, :NFULL])
        assert conv.all()
        H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
        win_U[i], win_X[i], win_iters[i] = U, X, it
        win_kkt[i] = [bq.kkt_residual(U[l, :, 1], win_x0[i, l], H, F, lo[:, 1], hi[:, 1]) for l in range(NFULL)]
        print(w, "iters", it, "hi/lo active", (U[:, :, 1] >= hi[:, 1]).sum(1), (U[:, :, 1] <= lo[:, 1]).sum(1),
              "kkt %.1e" % win_kkt[i].max())
    np.savez_compressed(os.path.join(HERE, "mpc_box.npz"), dx=np.array(DX), x0=x0, x=x, u=u, qp_iters=qp_iters,
                        tau_max=bq.TAU_MAX, T_pred=L, win_w=np.array(WINDOWS), win_x0=win_x0, win_U=win_U,
                        win_X=win_X, win_iters=win_iters, win_kkt=win_kkt)
    print("iteration histogram", np.bincount(qp_iters.ravel()), "steps at the limit",
          (np.abs(u[..., 1]) == bq.TAU_MAX).sum(1))


if __name__ == "__main__":
    main()
