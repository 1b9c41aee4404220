"""Writes tests/golden/mpc_box_hard.npz: window QPs on which the active set of tests/box_qp_ref.py cycles, with the
solutions of the projected-Newton fallback tests/box_qp_fallback_ref.py (NumPy only, from those two files alone).

As for mpc_box.npz no reference program can produce this fixture; what ties it to the QP is the solver-independent
KKT certificate (box_qp_ref.kkt_residual), stored per QP and re-checked by tests/test_mpc_box_fallback_host.py.

    python tests/golden/make_golden_mpc_box_hard.py

Contents (tau_max = 14, T_pred = 75, cap 32, the headline optimal trajectory of tracking.npz, mpc_box.npz's six starts):
  closed loop   unconv_off (6,): unconverged QPs per lane of the fallback-off closed loop (111 in all)
  hard QPs      the QPs of that closed loop at the cap: hard_step, hard_lane (111,), hard_e (111,4) = x - x_ref;
                hard_u (111,74) channel 1 of the hybrid solution, hard_iters (111,) active-set sweeps + Newton
                iterations, hard_kkt (111,)
  windows       win_w = 227, 270;  win_x0 (2,65,4): lanes 0-5 the closed loop's errors at that step, lanes 6-64 those
                errors (lane j: error j mod 6) times (1 + SPREAD N(0,1)) per component, seed 7;
                win_U (2,65,74,2), win_iters (2,65), win_kkt (2,65) of the hybrid solve; win_conv_off (2,65): whether
                the active set alone settles below the cap.
SPREAD is 0.1 at step 270.  At step 227 that spread leaves 4 of 65 lanes below the cap, fewer than the 8 on each side
that the tests want in every batch, so that batch uses 0.3 (11 below, 54 at the cap).  Step 270 gives a mixed first
wavefront and lane 64 a ragged second one.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import box_qp_fallback_ref as fb  # noqa: E402
import box_qp_ref as bq  # noqa: E402

TAU, L, CAP = 14.0, 75, 32
WINDOWS = (227, 270)
SPREAD = {227: 0.3, 270: 0.1}
NB = 65


def main():
    trk = np.load(os.path.join(HERE, "tracking.npz"))
    x0 = np.load(os.path.join(HERE, "mpc_box.npz"))["x0"]
    pb = bq.Problem(trk["x_opt"], trk["u_opt"])
    x, _, it, unconv = bq.closed_loop(pb, x0, TAU, L, CAP)
    lanes, steps = np.nonzero(it == CAP)
    assert unconv.sum() == lanes.size == 111, unconv
    hard_e = x[lanes, steps] - pb.x_ref[steps]
    hard_u = np.zeros((lanes.size, L - 1)); hard_iters = np.zeros(lanes.size, dtype=np.int32)
    hard_kkt = np.zeros(lanes.size)
    for i, (s, e) in enumerate(zip(steps, hard_e)):
        A, Bm, ur = pb.window(s, L)
        lo, hi = bq.bounds(ur, TAU)
        U, _, n, conv = fb.solve_window(pb, s, L, e, TAU, CAP)
        assert conv.all() and n[0] > CAP
        H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
        hard_u[i], hard_iters[i] = U[0, :, 1], n[0]
        hard_kkt[i] = bq.kkt_residual(U[0, :, 1], e, H, F, lo[:, 1], hi[:, 1])
    print("hard QPs", lanes.size, "Newton iterations <=", (hard_iters - CAP).max(), "kkt %.1e" % hard_kkt.max())

    rng = np.random.default_rng(7)
    win_x0 = np.zeros((len(WINDOWS), NB, 4)); win_U = np.zeros((len(WINDOWS), NB, L - 1, 2))
    win_iters = np.zeros((len(WINDOWS), NB), dtype=np.int32); win_kkt = np.zeros((len(WINDOWS), NB))
    win_conv_off = np.zeros((len(WINDOWS), NB), dtype=bool)
    for i, w in enumerate(WINDOWS):
        e6 = x[:, w] - pb.x_ref[w]
        win_x0[i, :6] = e6
        win_x0[i, 6:] = e6[np.arange(NB - 6) % 6] * (1.0 + SPREAD[w] * rng.standard_normal((NB - 6, 4)))
        win_conv_off[i] = bq.solve_window(pb, w, L, win_x0[i], TAU, CAP)[3]
        below, at_cap = int(win_conv_off[i].sum()), int((~win_conv_off[i]).sum())
        assert below >= 8 and at_cap >= 8, (w, below, at_cap)
        U, _, n, conv = fb.solve_window(pb, w, L, win_x0[i], TAU, CAP)
        assert conv.all() and ((n > CAP) == ~win_conv_off[i]).all()
        A, Bm, ur = pb.window(w, L)
        lo, hi = bq.bounds(ur, TAU)
        H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
        win_U[i], win_iters[i] = U, n
        win_kkt[i] = [bq.kkt_residual(U[l, :, 1], win_x0[i, l], H, F, lo[:, 1], hi[:, 1]) for l in range(NB)]
        print(w, "below the cap", below, "at the cap", at_cap, "lane 64 below", bool(win_conv_off[i, 64]),
              "iters <=", n.max(), "kkt %.1e" % win_kkt[i].max())
    np.savez_compressed(os.path.join(HERE, "mpc_box_hard.npz"), x0=x0, tau_max=TAU, T_pred=L, cap=CAP,
                        unconv_off=unconv, hard_step=steps.astype(np.int32), hard_lane=lanes.astype(np.int32),
                        hard_e=hard_e, hard_u=hard_u, hard_iters=hard_iters, hard_kkt=hard_kkt,
                        win_w=np.array(WINDOWS), win_x0=win_x0, win_U=win_U, win_iters=win_iters, win_kkt=win_kkt,
                        win_conv_off=win_conv_off)


if __name__ == "__main__":
    main()
