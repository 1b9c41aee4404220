"""Torque-limited MPC, CPU side: the NumPy reference (tests/box_qp_ref.py) against itself, scipy and the KKT
certificate on the recorded fixture (tests/golden/mpc_box.npz), and the new C-ABI entry points' host-side checks.
No kernel is launched here.

Bounds.  Two solvers of the same QP agree to the parity bar of the existing solver_mpc window test, 1e-8 relative
(measured CPU-vs-CPU: 3e-11 .. 6e-11).  The certificate max |u - clip(u - grad / diag(H), lo, hi)| is a step in u,
held to the same 1e-8 of the window's largest |u| (measured: <= 1.1e-10 absolute at |u| ~ 10).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_l2

import box_qp_ref as bq

REL = 1e-8


@pytest.fixture(scope="module")
def fx():
    return load_golden("mpc_box")


@pytest.fixture(scope="module")
def pb():
    trk = load_golden("tracking")
    return bq.Problem(trk["x_opt"], trk["u_opt"])


@pytest.fixture(scope="module")
def windows(fx, pb):
    """Per fixture window: stage data, bounds, the condensed QP."""
    out = []
    L = int(fx["T_pred"])
    for i, w in enumerate(fx["win_w"]):
        A, Bm, ur = pb.window(int(w), L)
        lo, hi = bq.bounds(ur, float(fx["tau_max"]))
        H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
        out.append((i, int(w), A, Bm, lo, hi, H, F))
    return out


def test_fixture_is_the_reference_output(fx, pb):
    """mpc_box.npz is make_golden_mpc_box.py's recording: the windows re-solved by the active-set formulation."""
    L = int(fx["T_pred"])
    for i, w in enumerate(fx["win_w"]):
        U, X, it, conv = bq.solve_window(pb, int(w), L, fx["win_x0"][i, :8])
        assert conv.all()
        np.testing.assert_array_equal(it, fx["win_iters"][i])
        assert rel_l2(U, fx["win_U"][i]) < 1e-12 and rel_l2(X, fx["win_X"][i]) < 1e-12


def test_two_formulations_agree_on_the_fixture_windows(fx, windows):
    for i, w, A, Bm, lo, hi, H, F in windows:
        for l in range(8):
            u_as = fx["win_U"][i, l, :, 1]
            u_c, _, conv = bq.solve_condensed(fx["win_x0"][i, l], H, F, lo[:, 1], hi[:, 1])
            assert conv
            assert np.abs(u_c - u_as).max() <= REL * max(1.0, np.abs(u_as).max()), (w, l)
            np.testing.assert_array_equal(fx["win_U"][i, l, :, 0], np.clip(0.0, lo[:, 0], hi[:, 0]))


def test_reference_agrees_with_scipy_bvls(fx, windows):
    lsq = pytest.importorskip("scipy.optimize").lsq_linear
    for i, w, A, Bm, lo, hi, H, F in windows:
        Cf = np.linalg.cholesky(H / 2.0).T                       # 1/2 u'Hu + u'f = |Cf u - y|^2 + const
        for l in range(8):
            y = -np.linalg.solve(Cf.T, F @ fx["win_x0"][i, l] / 2.0)
            res = lsq(Cf, y, bounds=(lo[:, 1], hi[:, 1]), method="bvls", tol=1e-14)
            u_as = fx["win_U"][i, l, :, 1]
            assert np.abs(res.x - u_as).max() <= REL * max(1.0, np.abs(u_as).max()), (w, l)


def test_kkt_certificate_holds_on_every_stored_case(fx, windows):
    seen = {"both": False, "stage0": False, "none": False}
    for i, w, A, Bm, lo, hi, H, F in windows:
        for l in range(8):
            u = fx["win_U"][i, l, :, 1]
            res = bq.kkt_residual(u, fx["win_x0"][i, l], H, F, lo[:, 1], hi[:, 1])
            assert res <= REL * max(1.0, np.abs(u).max()), (w, l, res)
            assert res == pytest.approx(float(fx["win_kkt"][i, l]), rel=1e-6, abs=1e-14)
            assert (u >= lo[:, 1]).all() and (u <= hi[:, 1]).all()
            at_hi, at_lo = u == hi[:, 1], u == lo[:, 1]
            seen["both"] |= bool(at_hi.any() and at_lo.any())
            seen["stage0"] |= bool(at_hi[0] or at_lo[0])
            seen["none"] |= not (at_hi.any() or at_lo.any())
    assert all(seen.values()), seen                              # the bound patterns the GPU tests rely on


@pytest.fixture(scope="module")
def loop(fx, pb):
    return bq.closed_loop(pb, fx["x0"], float(fx["tau_max"]), int(fx["T_pred"]))


def test_reference_closed_loop_converges_and_reproduces_the_fixture(fx, loop):
    x, u, qp_iters, unconv = loop
    assert not unconv.any()                                     # 0 of 3,000 QPs
    assert rel_l2(x, fx["x"]) < 1e-12 and rel_l2(u, fx["u"]) < 1e-12
    np.testing.assert_array_equal(qp_iters, fx["qp_iters"])
    assert qp_iters.max() <= 5 and (qp_iters == 1).sum() == 2484
    tau = float(fx["tau_max"])
    assert np.abs(u[..., 1]).max() == tau and (np.abs(fx["u"][2, :, 1]) == tau).any()
    assert np.abs(x[5, -1] - load_golden("tracking")["x_opt"][-1]).max() < 1e-5   # dx = 0.3 still ends upright


def test_closed_loop_controls_pass_the_certificate(fx, pb):
    """The applied first control of sampled closed-loop steps is the first control of a certified window solution."""
    L, tau = int(fx["T_pred"]), float(fx["tau_max"])
    trk = load_golden("tracking")
    for s in (0, 120, 172, 176, 184, 300, 499):
        A, Bm, ur = pb.window(s, L)
        lo, hi = bq.bounds(ur, tau)
        H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
        e = fx["x"][:, s] - trk["x_opt"][s]
        U, _, _, conv = bq.solve_window(pb, s, L, e, tau)
        assert conv.all()
        for l in range(6):
            assert bq.kkt_residual(U[l, :, 1], e[l], H, F, lo[:, 1], hi[:, 1]) <= REL * max(1.0, np.abs(U[l]).max())
            want = bq.apply_limit(ur[0, 1], U[l, 0, 1], lo[0, 1], hi[0, 1], tau)
            assert fx["u"][l, s, 1] == pytest.approx(want, rel=1e-9, abs=1e-12)


# ------------------------------------------------------------------------------------ C-ABI (host side)
NEW = ("gym_mpc_gains_all", "gym_mpc_box_workspace", "gym_mpc_box_qp", "gym_mpc_box_rollout")


def test_new_entry_points_are_declared_exported_and_bound():
    from gymnast_optimalcontrol_amd import _build, _lib
    lib = _lib.load(_build.build())
    header = open(os.path.join(ROOT, "include", "gymnast_acrobot.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name)
    assert lib.gym_abi_version() == 18 == _lib.ABI_VERSION
    assert re.search(r"#define GYM_ABI_VERSION 18\b", header)


def test_box_entry_points_reject_bad_arguments_without_a_device():
    from gymnast_optimalcontrol_amd import _lib
    lib = _lib.load()
    D = 0x10000                                                  # dummy device address: never dereferenced
    m = _lib.GymModel(dt=0.02)
    Q = np.diag([120.0, 100.0, 1e-4, 1e-4]); R = np.diag([1e-6, 10.0])
    S = 80
    A = np.tile(np.eye(4), (S, 1, 1)); Bm = np.zeros((S, 4, 2)); Bm[:, 2:, 1] = 0.02
    ur = np.zeros((S, 2))
    need = C.c_int64(-1)
    assert lib.gym_mpc_box_workspace(64, 75, 80, None) == 1
    for bad in ((0, 75, 80), (64, 1, 80), (64, 255, 80), (64, 75, 0)):
        assert lib.gym_mpc_box_workspace(*bad, C.byref(need)) == 1 and need.value == -1, bad
    assert lib.gym_mpc_box_workspace(65, 75, 80, C.byref(need)) == 0
    # the stage table, then per padded lane 10 doubles per stage + x_{L-1} and one int32 state per stage
    assert need.value == 80 * 26 * 8 + 128 * ((10 * 74 + 4) * 8 + 74 * 4)
    big = 1 << 40

    def qp(A=A, Bm=Bm, ur=ur, S=S, R=R, B=64, L=75, tau=18.0, it=32, ws=D, nbytes=big, x0=D):
        return lib.gym_mpc_box_qp(A.ctypes.data, Bm.ctypes.data, ur.ctypes.data, S, Q.ctypes.data, R.ctypes.data, D,
                                  x0, B, L, tau, it, ws, nbytes, D, D, D, D, None)

    def roll(B=64, N=501, L=75, tau=18.0, it=32, R=R, nbytes=big, x0=D):
        return lib.gym_mpc_box_rollout(C.byref(m), x0, D, D, D, D, Q.ctypes.data, R.ctypes.data, D, D, B, N, L, tau,
                                       it, D, nbytes, D, D, D, D, None)

    for kw in (dict(B=0), dict(L=1), dict(L=255), dict(tau=0.0), dict(tau=-18.0), dict(tau=float("nan")),
               dict(tau=float("inf")), dict(it=0), dict(x0=None), dict(nbytes=1024)):
        assert qp(**kw) == 1, kw
        assert roll(**kw) == 1, kw
    assert roll(N=1) == 1
    assert qp(S=73) == 1                                         # fewer stages than the window needs
    assert qp(ws=None) == 1
    B1 = Bm.copy(); B1[40, 3, 0] = 1e-300
    assert qp(Bm=B1) == 1                                        # a non-zero column 0: channel 0 does not separate
    for Rb in (np.array([[1e-6, 0.1], [0.0, 10.0]]), np.diag([1e-6, 0.0]), np.diag([1e-6, -1.0])):
        assert qp(R=Rb) == 1 and roll(R=Rb) == 1
    args = (C.byref(m), D, D, 500, D, D, Q.ctypes.data, R.ctypes.data)
    assert lib.gym_mpc_gains_all(*args, 1, 10, 1000, 1e-6, D, D, D, None) == 1      # L < 2
    assert lib.gym_mpc_gains_all(*args, 255, 10, 1000, 1e-6, D, D, D, None) == 1    # L + 2 > 256
    assert lib.gym_mpc_gains_all(*args, 75, 0, 1000, 1e-6, D, D, D, None) == 1      # no window
    assert lib.gym_mpc_gains_all(*args, 75, 10, 1000, 1e-6, None, D, D, None) == 1  # no output
