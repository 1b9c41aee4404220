"""The tracker entry points on dense stage data and weights.

The acrobot's B_d has a zero column 0 and the trackers' Q, R are diagonal, so in every other test row 0 of each
tracking gain is zero and the terms it multiplies (i01, i10, apb0 K[j], column 0 of PB in lqr_step and
k_dare_fixed_point; u0 in k_lq_forward; v0's feedback in track_feedback; K0j and the R01 R10 term of
riccati_map_lane; r11 of sda16_init) are only ever multiplied by zero.  Here the generic kernels run a dense stage
array (A = I + 0.1 randn, B = 0.3 randn, 12 stages and a dense pad) with SPD non-diagonal Q, R, Q_T; the tracking
rollouts run dense gains and a non-zero u_ff channel 0; the fused MPC kernels run the acrobot's stages with
non-diagonal SPD Q, R (R01 != 0 makes row 0 of every gain non-zero: K[0] = -(R01 / R00) K[1]).

References: tests/dense_ref.py (np.longdouble) for the pure algebra, at 64 x the float64 evaluation's own deviation
from it on the same inputs (dense_ref.algebra_bound; floor 1.4e-14); oracle/tracking_np.py and the reference's own
results (tests/golden/dense_kats.npz) for the rollouts and the MPC gains, at tests/test_tracking.py's tolerances
(1e-9; fused vs generic path 1e-11).  Gains are compared row by row and controls channel by channel, each on its own
norm.  Iteration counts are compared exactly (the stop-count margins are asserted in test_dense_ref_host.py).

Measured kernel-vs-reference deviations (MI355X, largest over the cases; bound in brackets):
  tv_lqr_gains      4.2e-15 [1.7e-13] (L = 6, one window, its smallest entry), else <= 2.0e-15 [1.4e-14 .. 5.5e-14]
  dare_fixed_point  dense pair 7.3e-16 [2.7e-14], 99 maps; acrobot pad with dense Q, R 4.7e-13 [7.0e-11], 382 maps;
                    non-converging pair with dense R 7.1e-15 [4.6e-13], 1001 reported; every count exact
  lq_forward        X 2.5e-16, U 2.8e-16 [1.4e-14 .. 3.9e-14]
  track_rollout     x 3.4e-16, u 9.1e-17 per channel [1e-9]; pair = single lane bit for bit
  mpc_gains         K0 rows vs oracle 4.5e-13 [1e-9], vs generic path 2.7e-13 [1e-11]; Q_T vs oracle 6.5e-13 [1e-9],
                    vs generic 4.0e-13 [1e-11]; 382 maps on every path; K_all[w][0] = K0[w] bit for bit
"""
import numpy as np
import pytest

import dense_ref as dr
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-9          # tests/test_tracking.py: gains and closed-loop trajectories
TOL_GENERIC = 1e-11  # ... fused MPC gains against the generic path


def _np(t):
    return t.detach().cpu().numpy()


def _report(name, err, bound):
    print(f"DEV {name}: {err:.2e} (bound {bound:.1e})")
    assert err <= bound, (name, err, bound)


@pytest.fixture(scope="module")
def eng():
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine
    return AcrobotEngine(params=1)


@pytest.fixture(scope="module")
def kats():
    return load_golden("dense_kats")


@pytest.fixture(scope="module")
def stages():
    return dr.gen_tracking()


def _row_err(K, Kref):
    """Rows of a gain array (...,2,4), each on its own max norm (test_tracking's measure, per row)."""
    K = np.asarray(K, float); Kref = np.asarray(Kref, float)
    return max(np.abs(K[..., r, :] - Kref[..., r, :]).max() / np.abs(Kref[..., r, :]).max() for r in (0, 1))


# ---------------------------------------------------------------------------------------------- tv_lqr_gains
@pytest.mark.parametrize("disc", [False, True])
@pytest.mark.parametrize("L,nwin,allg", [(dr.TSTAGES + 1, 1, True), (2, 1, True), (6, 1, False), (6, 5, False),
                                         (6, 70, False)])
def test_tv_lqr_gains_dense(eng, stages, disc, L, nwin, allg):
    """All gains (L = S + 1, L = 2) and windowed first gains (L = 6: windows 8.. read the dense pad stage;
    nwin = 70: a second block), with and without discretisation."""
    g = stages
    kw = dict(L=L, nwin=nwin, all_gains=allg, A_pad=g["A_pad"], B_pad=g["B_pad"], discretize=disc)
    K = _np(eng.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], **kw))
    Kr = dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], dt=eng.dt, **kw)
    K64 = dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], dt=eng.dt, dtype=np.float64, **kw)
    assert K.shape == Kr.shape == (((L - 1) if allg else nwin), 2, 4)
    assert np.abs(K[:, 0]).max() > 1e-2 and np.abs(np.asarray(Kr[:, 0], float)).max() > 1e-2   # row 0 is live
    _report(f"tv_lqr_gains disc={disc} L={L} nwin={nwin}", dr.chan_err(K, Kr, 2),
            dr.algebra_bound(dr.chan_err(K64, Kr, 2), TOL))
    if not allg and nwin > 1:        # a window's gain does not depend on how many windows run beside it
        K1 = _np(eng.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], **dict(kw, nwin=1)))
        assert np.array_equal(K1[0], K[0])
        if nwin == 70:
            K5 = _np(eng.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], **dict(kw, nwin=65)))
            assert np.array_equal(K5, K[:65])


# ------------------------------------------------------------------------------------------ dare_fixed_point
def test_dare_fixed_point_dense(eng, kats):
    from oracle import tracking_np as tr
    trk = load_golden("tracking")
    dd = dr.gen_dare()
    Qm, Rm = dr.gen_mpc_weights()
    for name, (A, B, Q, R), fix, existing in (
            ("dense", (dd["A"], dd["B"], dd["Q"], dd["R"]), kats["pinf_dense"], 1e-10),
            ("pad", (trk["A_f"], trk["B_f"], Qm, Rm), kats["pinf_pad"], 1e-10)):
        P, it = eng.dare_fixed_point(A, B, Q, R)
        P, it = _np(P), int(it.item())
        Pr, itr, _ = dr.compute_P_inf(A, B, Q, R)
        Po, ito = tr.compute_P_inf(A, B, Q, R)
        assert it == itr == ito < 1000, (name, it, itr, ito)
        bound = dr.algebra_bound(dr.chan_err(Po, Pr, 0), existing)
        _report(f"dare_fixed_point {name} ({it} maps)", dr.chan_err(P, Pr, 0), bound)
        assert dr.chan_err(P, fix, 0) <= bound + dr.chan_err(fix, Pr, 0)      # the reference's own P_inf
    A, B, Q, R = dr.slow_pair_dense()                  # never within tol: 1000 maps, max_iter + 1 reported
    P, it = eng.dare_fixed_point(A, B, Q, R)
    P, it = _np(P), int(it.item())
    Pr, itr, _ = dr.compute_P_inf(A, B, Q, R)
    Po, ito = tr.compute_P_inf(A, B, Q, R)
    assert it == itr == ito == 1001 and np.isfinite(P).all()
    _report("dare_fixed_point slow pair, dense R", dr.chan_err(P, Pr, 0),
            dr.algebra_bound(dr.chan_err(Po, Pr, 0), 1e-12))


# ------------------------------------------------------------------------------------------------ lq_forward
@pytest.mark.parametrize("disc", [False, True])
@pytest.mark.parametrize("L", [2, 7, 16])
def test_lq_forward_dense(eng, stages, disc, L):
    """Dense stages and gains (u0 = K[0] x is live); L = 16 over 12 stages reads the pad stage."""
    g = stages
    Kall = np.asarray(dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], dr.TSTAGES + 1, discretize=disc,
                                      dt=eng.dt), float)
    K = np.concatenate([Kall, Kall[:4]])[:L - 1]
    kw = dict(A_pad=g["A_pad"], B_pad=g["B_pad"], discretize=disc)
    X, U = (_np(a) for a in eng.lq_forward(g["A"], g["B"], K, g["x0"], L, **kw))
    Xr, Ur = dr.lq_forward(g["A"], g["B"], K, g["x0"], L, dt=eng.dt, **kw)
    X64, U64 = dr.lq_forward(g["A"], g["B"], K, g["x0"], L, dt=eng.dt, dtype=np.float64, **kw)
    assert np.abs(U[:, 0]).min() > 0
    _report(f"lq_forward X disc={disc} L={L}", dr.chan_err(X, Xr), dr.algebra_bound(dr.chan_err(X64, Xr), 1e-8))
    _report(f"lq_forward U disc={disc} L={L}", dr.chan_err(U, Ur), dr.algebra_bound(dr.chan_err(U64, Ur), 1e-8))


# --------------------------------------------------------------------------------------------- track_rollout
@pytest.mark.parametrize("B", [1, 2, 63, 65])
def test_track_rollout_dense_gains(eng, kats, B):
    """Pair and single-lane rollouts under dense gains (row 0 non-zero) and a non-zero u_ff channel 0."""
    from oracle import tracking_np as tr
    k = dr.gen_track()
    assert np.abs(k["K"][:, 0]).min() > 0 and np.abs(k["u_ff"][:, 0]).min() > 0
    for N in dr.KNOTS:
        x_ff, u_ff, K, x0 = k["x_ff"][:N], k["u_ff"][:N - 1], k["K"][:N - 1], k["x0"][:B]
        xp, up = (_np(a) for a in eng.track_rollout(x0, x_ff, u_ff, K))
        xs, us = (_np(a) for a in eng.track_rollout(x0, x_ff, u_ff, K, single=True))
        assert np.array_equal(xp, xs) and np.array_equal(up, us), N
        xo, uo = tr.simulate_tracking(x_ff, u_ff, K, x0)
        ex, eu = dr.chan_err(xp, xo), dr.chan_err(up, uo)          # u[:, :, 0] on its own norm
        assert ex < TOL and eu < TOL, (N, ex, eu)
        for l in sorted({0, min(62, B - 1), B - 1}):
            for single in (False, True):
                x1, u1 = eng.track_rollout(x0[l:l + 1], x_ff, u_ff, K, single=single)
                assert np.array_equal(_np(x1)[0], xp[l]) and np.array_equal(_np(u1)[0], up[l]), (N, l, single)
        if N == dr.NMAX and B >= 4:                                # the reference's own simulate_tracking
            assert dr.chan_err(xp[:4], kats["trk_x"]) < TOL and dr.chan_err(up[:4], kats["trk_u"]) < TOL
    print(f"DEV track_rollout B={B}: x {ex:.2e}, u {eu:.2e}")


# ------------------------------------------------------------------------------------------------ MPC gains
@pytest.mark.parametrize("L", [2, 6])
def test_mpc_gains_nondiagonal_weights(eng, kats, L):
    """gym_mpc_gains / gym_mpc_gains_all with symmetric non-diagonal SPD Q, R: K0 (row 0 non-zero), Q_T and the
    iteration count against the NumPy oracle and against the generic path; K_all[w][0] is K0[w] bit for bit."""
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    from oracle import tracking_np as tr
    trk = load_golden("tracking")
    Q, R = dr.gen_mpc_weights()
    x_ref, u_ref = eng.t(trk["x_opt"][:40]), eng.t(trk["u_opt"][:39])
    S = nwin = 39
    x_f, u_f = tt._final_state(eng)
    K0, QT, it = eng.mpc_gains(x_ref, u_ref, x_f, u_f, Q, R, L=L, nwin=nwin)
    Kall, QTa, ita = eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, Q, R, L=L, nwin=nwin)
    K0, QT, it, Kall, QTa, ita = _np(K0), _np(QT), int(it.item()), _np(Kall), _np(QTa), int(ita.item())
    assert Kall.shape == (nwin, L - 1, 2, 4)
    assert np.array_equal(Kall[:, 0], K0) and np.array_equal(QTa, QT) and ita == it
    K0o, QTo = tr.mpc_gains(trk["x_opt"][:40], trk["u_opt"][:39], L, Q, R)
    _, ito = tr.compute_P_inf(trk["A_f"], trk["B_f"], Q, R)
    _, itr, _ = dr.compute_P_inf(trk["A_f"], trk["B_f"], Q, R)
    assert it == ito == itr < 1000, (it, ito, itr)
    assert np.abs(K0o[:, 0]).max() > 100 and np.abs(K0[:, 0]).max() > 100          # row 0 is live
    np.testing.assert_allclose(QT, QTo, rtol=TOL)
    np.testing.assert_allclose(QT, kats["pinf_pad"], rtol=TOL)                       # the reference's own P_inf
    eo = _row_err(K0, K0o)
    assert eo <= TOL, eo
    # the generic path on host-built Jacobians
    A_c, B_c = eng.jacobians(x_ref[:S], u_ref[:S])
    Af_c, Bf_c = eng.jacobians(x_f, u_f)
    A_f, B_f = tt._discrete(eng, Af_c[0], Bf_c[0])
    QTg, itg = eng.dare_fixed_point(A_f, B_f, Q, R)
    assert int(itg.item()) == it
    K0g = _np(eng.tv_lqr_gains(A_c, B_c, Q, R, QTg, L=L, nwin=nwin, all_gains=False, A_pad=Af_c[0], B_pad=Bf_c[0],
                               discretize=True))
    np.testing.assert_allclose(QT, _np(QTg), rtol=TOL_GENERIC)
    eg = _row_err(K0, K0g)
    assert eg <= TOL_GENERIC, eg
    # every stage's gain of window 0 and of the last window (all pad past S) against the generic recursion
    for w in (0, nwin - 1):
        Kw = _np(eng.tv_lqr_gains(A_c[w:], B_c[w:], Q, R, QTg, L=L, nwin=1, all_gains=True, A_pad=Af_c[0],
                                  B_pad=Bf_c[0], discretize=True))
        ew = _row_err(Kall[w], Kw)
        assert ew <= TOL_GENERIC, (w, ew)
    print(f"DEV mpc_gains L={L}: K0 vs oracle {eo:.2e}, vs generic {eg:.2e}, Q_T vs oracle "
          f"{np.abs(QT / QTo - 1).max():.2e}, vs generic {np.abs(QT / _np(QTg) - 1).max():.2e}, {it} maps")
