"""The projected-Newton fallback of the torque-limited window QP, host side (CPU only): the NumPy restatement
tests/box_qp_fallback_ref.py on the fixture tests/golden/mpc_box_hard.npz (QPs on which the active set cycles), the
ABI surface of the three ..._fallback entry points, their argument checks, TorqueLimit in every front end and the
engine's call lists.

Bars.  The KKT certificate (box_qp_ref.kkt_residual, which depends on no solver) and the agreement between solvers
are held to 1e-8 max(1, |u|), tests/test_mpc_box_host.py's bar.  scipy's BVLS is the outside solver.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import box_qp_fallback_ref as fb
import box_qp_ref as bq
import test_engine_launch_host as tl
from test_engine_launch_host import rig  # noqa: F401  (the recording-library fixture)

REL = 1e-8
HEADER = os.path.join(ROOT, "include", "gymnast_acrobot.h")
NEW = ("gym_mpc_box_qp_fallback", "gym_mpc_box_rollout_fallback", "gym_mpc_box_lanes_rollout_fallback")


@pytest.fixture(scope="module")
def fx():
    return load_golden("mpc_box_hard")


@pytest.fixture(scope="module")
def pb():
    trk = load_golden("tracking")
    return bq.Problem(trk["x_opt"], trk["u_opt"])


def _window(pb, w, fx):
    A, Bm, ur = pb.window(int(w), int(fx["T_pred"]))
    lo, hi = bq.bounds(ur, float(fx["tau_max"]))
    H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
    return A, Bm[:, :, 1], lo[:, 1], hi[:, 1], H, F


def _bvls(H, F, e, lo, hi):
    """The QP as a bounded least-squares problem for scipy: 1/2 u'H u + u'f = 1/2 |C'u + C^-1 f|^2 + const, H = C C'."""
    from scipy.linalg import solve_triangular
    from scipy.optimize import lsq_linear
    Cf = np.linalg.cholesky(H)
    r = lsq_linear(Cf.T, -solve_triangular(Cf, F @ e, lower=True), bounds=(lo, hi), method="bvls", tol=1e-14,
                   max_iter=2000)
    return r.x


# ------------------------------------------------------------------------------------ the NumPy fallback
def test_fallback_solves_every_window_qp_of_the_fixture(fx, pb):
    """Both 65-lane batches: the active set alone leaves at least 8 lanes at the cap and at least 8 below; the hybrid
    solve converges on all, passes the certificate, is the recorded solution, agrees with BVLS and with the condensed
    formulation, and leaves the lanes that settled within the cap untouched."""
    cap = int(fx["cap"])
    for i, w in enumerate(fx["win_w"]):
        A, b, lo, hi, H, F = _window(pb, w, fx)
        E = fx["win_x0"][i]
        U0, X0, it0, conv0 = bq.solve_active_set(E, A, b, pb.Q, pb.R[1, 1], pb.QT, lo, hi, cap)
        np.testing.assert_array_equal(conv0, fx["win_conv_off"][i])
        assert (~conv0).sum() >= 8 and conv0.sum() >= 8 and ((it0 == cap) == ~conv0).all()
        U, X, it, conv = fb.solve_hybrid(E, A, b, pb.Q, pb.R[1, 1], pb.QT, lo, hi, cap)
        assert conv.all() and ((it > cap) == ~conv0).all()
        np.testing.assert_array_equal(it, fx["win_iters"][i])
        np.testing.assert_array_equal(U[conv0], U0[conv0])
        np.testing.assert_array_equal(X[conv0], X0[conv0])
        assert (U >= lo).all() and (U <= hi).all()
        for l in range(E.shape[0]):
            bar = REL * max(1.0, np.abs(U[l]).max())
            assert bq.kkt_residual(U[l], E[l], H, F, lo, hi) <= bar, (w, l)
            assert np.abs(U[l] - fx["win_U"][i, l, :, 1]).max() <= bar
            assert np.abs(_bvls(H, F, E[l], lo, hi) - U[l]).max() <= bar, (w, l)
            uc, nc, cc = fb.newton_condensed(E[l], U0[l], H, F, lo, hi)
            assert cc and np.abs(uc - U[l]).max() <= bar, (w, l, nc)


def test_fallback_solves_the_111_cycling_qps_of_the_closed_loop(fx, pb):
    """The QPs the fallback-off closed loop left at the cap, re-solved one by one from their recorded errors."""
    cap, L, tau = int(fx["cap"]), int(fx["T_pred"]), float(fx["tau_max"])
    assert fx["hard_step"].size == 111 == int(fx["unconv_off"].sum())
    worst = 0.0
    for s in np.unique(fx["hard_step"]):
        A, b, lo, hi, H, F = _window(pb, s, fx)
        idx = np.flatnonzero(fx["hard_step"] == s)
        E = fx["hard_e"][idx]
        _, _, _, conv0 = bq.solve_active_set(E, A, b, pb.Q, pb.R[1, 1], pb.QT, lo, hi, cap)
        assert not conv0.any()
        U, _, it, conv = fb.solve_hybrid(E, A, b, pb.Q, pb.R[1, 1], pb.QT, lo, hi, cap)
        assert conv.all() and (it > cap).all()
        np.testing.assert_array_equal(it, fx["hard_iters"][idx])
        for k, i in enumerate(idx):
            bar = REL * max(1.0, np.abs(U[k]).max())
            res = bq.kkt_residual(U[k], E[k], H, F, lo, hi)
            worst = max(worst, res / max(1.0, np.abs(U[k]).max()))
            assert res <= bar and np.abs(U[k] - fx["hard_u"][i]).max() <= bar
            assert np.abs(_bvls(H, F, E[k], lo, hi) - U[k]).max() <= bar, (s, k)
            uc, _, cc = fb.newton_condensed(E[k], np.zeros(L - 1), H, F, lo, hi)
            assert cc and np.abs(uc - U[k]).max() <= bar, (s, k)
    print("worst relative certificate", worst, "Newton iterations <=", int((fx["hard_iters"] - cap).max()))


def test_closed_loop_has_no_unconverged_qp_with_the_fallback(fx, pb):
    """tau_max = 14 on the six starts.  Precondition: plain box_qp_ref leaves 111 QPs at the cap (15, 17, 15, 18, 22,
    24 per lane).  With the fallback none is left, the loops agree bit for bit up to the first such QP of each lane,
    and qp_iters > cap exactly where the fallback ran."""
    cap, L, tau = int(fx["cap"]), int(fx["T_pred"]), float(fx["tau_max"])
    x0, u0, it0, unc0 = bq.closed_loop(pb, fx["x0"], tau, L, cap)
    np.testing.assert_array_equal(unc0, fx["unconv_off"])
    assert unc0.sum() == 111 and list(unc0) == [15, 17, 15, 18, 22, 24]
    x, u, it, unc = fb.closed_loop(pb, fx["x0"], tau, L, cap)
    assert not unc.any() and np.isfinite(x).all() and np.abs(u).max() <= tau
    assert (it > cap).any() and (it != cap).all()
    for l in range(6):
        first = int(np.flatnonzero(it0[l] == cap)[0])
        np.testing.assert_array_equal(x[l, :first + 1], x0[l, :first + 1])
        np.testing.assert_array_equal(u[l, :first], u0[l, :first])
        np.testing.assert_array_equal(it[l, :first], it0[l, :first])
        assert it[l, first] > cap


def test_one_newton_iteration_is_not_enough_and_says_so(fx, pb):
    """fallback_iters = 1 on the step-227 batch: some QPs stay unconverged; they are feasible and counted once."""
    cap = int(fx["cap"])
    A, b, lo, hi, H, F = _window(pb, fx["win_w"][0], fx)
    U, _, it, conv = fb.solve_hybrid(fx["win_x0"][0], A, b, pb.Q, pb.R[1, 1], pb.QT, lo, hi, cap, 1)
    assert (~conv).any() and (it[~conv] == cap + 1).all() and (it <= cap + 1).all()
    assert (U >= lo).all() and (U <= hi).all()


# ------------------------------------------------------------------------------------ C-ABI (host side)
def test_fallback_entry_points_are_declared_exported_and_bound():
    from gymnast_optimalcontrol_amd import _build, _lib
    lib = _lib.load(_build.build())
    src = open(HEADER).read()
    assert re.search(r"^#define GYM_ABI_VERSION 18$", src, flags=re.M)
    assert lib.gym_abi_version() == 18 == _lib.ABI_VERSION
    for name in NEW:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in the header"
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name)
        base = name[:-len("_fallback")]
        assert len(_lib._SIGS[name]) == len(m.group(1).split(",")) == len(_lib._SIGS[base]) + 1, name
        k = _lib._SIGS[base].index(C.c_double) + 2              # tau_max, max_qp_iters, then fallback_iters
        assert _lib._SIGS[name] == _lib._SIGS[base][:k] + [C.c_int32] + _lib._SIGS[base][k:]
        assert "trajectory_tracking.py:87-114" in src[:m.start()].rsplit("/*", 1)[1], name
        assert "int32_t max_qp_iters, int32_t fallback_iters" in " ".join(m.group(1).split())
    order = [src.index("int " + n + "(") for n in ("gym_mpc_box_rollout", "gym_mpc_box_qp_fallback",
                                                    "gym_mpc_box_rollout_fallback", "gym_lqr_lanes_workspace",
                                                    "gym_mpc_box_lanes_rollout", "gym_mpc_box_lanes_rollout_fallback",
                                                    "gym_timing_create")]
    assert order == sorted(order)
    i = _lib.EXPORTS.index("gym_mpc_lanes_gains")
    assert _lib.EXPORTS[i + 1:i + 5] == ("gym_mpc_box_lanes_workspace", "gym_mpc_box_lanes_rollout",
                                         "gym_mpc_box_lanes_rollout_fallback", "gym_timing_create")


def test_fallback_entry_points_reject_bad_arguments_without_a_device():
    """Everything right but one argument returns GYM_EINVAL before any launch (dummy addresses: skipped where a
    device could run one): the checks of the entry points without the suffix, and fallback_iters < 1."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("dummy device addresses: CPU-only check")
    from gymnast_optimalcontrol_amd import _lib
    lib = _lib.load()
    D = 0x10000
    m = _lib.GymModel(dt=0.02)
    Q = np.diag([120.0, 100.0, 1e-4, 1e-4]); R = np.diag([1e-6, 10.0])
    S = 80
    A = np.tile(np.eye(4), (S, 1, 1)); Bm = np.zeros((S, 4, 2)); Bm[:, 2:, 1] = 0.02
    ur = np.zeros((S, 2))
    big = 1 << 40
    need = C.c_int64()
    assert lib.gym_mpc_box_lanes_workspace(12, 3, 75, C.byref(need)) == 0

    def qp(Bm=Bm, S=S, R=R, B=64, L=75, tau=14.0, it=32, fbi=128, ws=D, nbytes=big, x0=D):
        return lib.gym_mpc_box_qp_fallback(A.ctypes.data, Bm.ctypes.data, ur.ctypes.data, S, Q.ctypes.data,
                                           R.ctypes.data, D, x0, B, L, tau, it, fbi, ws, nbytes, D, D, D, D, None)

    def roll(B=64, N=501, L=75, tau=14.0, it=32, fbi=128, R=R, nbytes=big, x0=D):
        return lib.gym_mpc_box_rollout_fallback(C.byref(m), x0, D, D, D, D, Q.ctypes.data, R.ctypes.data, D, D, B, N,
                                                L, tau, it, fbi, D, nbytes, D, D, D, D, None)

    def lanes(B=12, P=3, N=501, L=75, Q=Q, R=R, tau=14.0, it=32, fbi=128, ws=D, nbytes=need.value, xo=D, uo=D, sm=D,
              un=D, x0=D):
        return lib.gym_mpc_box_lanes_rollout_fallback(C.byref(m), D, D, x0, B, P, N, L, Q.ctypes.data, R.ctypes.data,
                                                      D, tau, it, fbi, ws, nbytes, xo, uo, sm, D, un, None)

    for kw in (dict(fbi=0), dict(fbi=-1), dict(B=0), dict(L=1), dict(L=255), dict(tau=0.0), dict(tau=-14.0),
               dict(tau=float("nan")), dict(tau=float("inf")), dict(it=0), dict(x0=None), dict(nbytes=1024)):
        assert qp(**kw) == 1, kw
        assert roll(**kw) == 1, kw
        assert lanes(**kw) == 1, kw
    assert roll(N=1) == 1 and lanes(N=1) == 1 and lanes(P=0) == 1
    assert qp(S=73) == 1 and qp(ws=None) == 1 and lanes(ws=None) == 1
    B1 = Bm.copy(); B1[40, 3, 0] = 1e-300
    assert qp(Bm=B1) == 1
    for Rb in (np.array([[1e-6, 0.1], [0.0, 10.0]]), np.diag([1e-6, 0.0]), np.diag([1e-6, -1.0])):
        assert qp(R=Rb) == 1 and roll(R=Rb) == 1 and lanes(R=Rb) == 1
    nonsym = Q.copy(); nonsym[0, 1] = 1.0
    assert lanes(Q=nonsym) == 1 and lanes(xo=None) == 1 and lanes(uo=None) == 1 and lanes(sm=None) == 1
    assert lanes(un=None) == 1 and lanes(B=_lib.MAX_BP // 2) == 1


# ------------------------------------------------------------------------------------ front end
def test_torque_limit_is_accepted_by_every_front_end_and_a_number_takes_todays_path(monkeypatch):
    import dataclasses
    import torch
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine, check_box, check_fallback
    from gymnast_optimalcontrol_amd.solver import SolveResult
    tl14 = tt.TorqueLimit(14.0)
    assert (tl14.tau_max, tl14.fallback_iters) == (14.0, 128) and tt.TorqueLimit(14.0, 5).fallback_iters == 5
    with pytest.raises(dataclasses.FrozenInstanceError):
        tl14.fallback_iters = 3
    for name in ("mpc_box_qp", "mpc_box_rollout", "mpc_box_lanes_rollout"):
        par = inspect.signature(getattr(AcrobotEngine, name)).parameters
        assert list(par)[-1] == "fallback_iters" and par["fallback_iters"].default == 0
    assert check_box(14.0, 32) is None and check_box(14.0, 32, 7) is None and check_fallback(7) == 7
    for bad in (-1, 2.5, 2 ** 31):
        with pytest.raises(ValueError, match="fallback_iters"):
            check_box(14.0, 32, bad)
    for fn in (tt.solver_mpc, tt.solve_mpc_tracking, tt.solve_mpc_tracking_box_batch, tt.MPC_tracking_lanes,
               SolveResult.track_mpc, tt.MpcBoxResult, tt.MpcBoxLanesResult):
        assert "TorqueLimit" in fn.__doc__, fn

    class Eng:                                                      # records what the front ends ask the engine for
        device = "cpu"

        def __init__(self):
            self.calls, self.mpc_qt_cache = [], {}

        def t(self, a):
            return torch.as_tensor(np.asarray(a), dtype=torch.float64)

        def mpc_gains(self, *a, **k):
            return None, torch.eye(4, dtype=torch.float64), None

        def mpc_gains_all(self, x_ref, u_ref, x_f, u_f, Q, R, L, nwin):
            return torch.zeros(nwin, L - 1, 2, 4, dtype=torch.float64), torch.eye(4, dtype=torch.float64), None

        def mpc_lanes_gains(self, *a, **k):
            return None, None

        def mpc_box_qp(self, A, Bm, ur, Q, R, QT, x0, L, tau, *a, **k):
            self.calls.append(("qp", tau, a, k))
            return (torch.zeros(1, L - 1, 2), torch.zeros(1, L, 4), torch.ones(1, dtype=torch.int32),
                    torch.ones(1, dtype=torch.int32))

        def mpc_box_rollout(self, x0, x_ref, u_ref, x_f, u_f, Q, R, QT, K_all, tau, *a, **k):
            self.calls.append(("rollout", tau, a, k))
            N = x_ref.shape[0]
            return torch.zeros(1, N, 4), torch.zeros(1, N - 1, 2), None, None

        def mpc_box_lanes_rollout(self, x_opt, u_opt, x0, Q, R, QT, L, tau, *a, **k):
            self.calls.append(("lanes", tau, a, k))
            return None, None, torch.zeros(3, 1, 1), None, torch.zeros(1, 1)

    eng = Eng()
    monkeypatch.setattr(tt, "_eng", lambda: eng)
    monkeypatch.setattr(tt, "_FINAL_STATE", {})
    x, u = np.zeros((6, 4)), np.zeros((5, 2))
    A, Bm = [np.eye(4)] * 3, [np.zeros((4, 2))] * 3

    def every_front_end(tau):
        eng.calls.clear()
        tt.solver_mpc(x[0], A, Bm, np.eye(4), np.eye(2), np.eye(4), 3, u_ref=u, tau_max=tau)
        tt.solve_mpc_tracking_box_batch(x[:1], x, u, tau, 3)
        tt.solve_mpc_tracking(x[0], x, u, 6, 3, tau_max=tau)
        tt.MPC_tracking_lanes(x[None], u[None], x[None, 0], T_pred=3, tau_max=tau, trajectories=False, gains=False)
        r = SolveResult.__new__(SolveResult)
        r.x, r.u = eng.t(x[None]), eng.t(u[None])
        r.track_mpc(T_pred=3, tau_max=tau, trajectories=False, gains=False)
        return list(eng.calls)

    plain = every_front_end(14.0)
    assert [c[0] for c in plain] == ["qp", "rollout", "rollout", "lanes", "lanes"]
    assert all(c[1] == 14.0 and "fallback_iters" not in c[3] for c in plain)        # today's calls, nothing added
    for tau, want in ((tl14, 128), (tt.TorqueLimit(14.0, 9), 9)):
        calls = every_front_end(tau)
        assert [(c[0], c[1], c[2]) for c in calls] == [(c[0], c[1], c[2]) for c in plain]
        assert all(c[3].get("fallback_iters") == want for c in calls), calls
    assert every_front_end(tt.TorqueLimit(14.0, 0)) == plain                       # 0 is the plain number
    for bad in (tt.TorqueLimit(0.0), tt.TorqueLimit(np.inf), tt.TorqueLimit(14.0, -1), tt.TorqueLimit(14.0, 1.5)):
        with pytest.raises(ValueError):
            tt.solve_mpc_tracking_box_batch(x[:1], x, u, bad, 3)
        with pytest.raises(ValueError):
            tt.MPC_tracking_lanes(x[None], u[None], x[None, 0], T_pred=3, tau_max=bad)
        with pytest.raises(ValueError):
            tt.solver_mpc(x[0], A, Bm, np.eye(4), np.eye(2), np.eye(4), 3, u_ref=u, tau_max=bad)


# ------------------------------------------------------------------------------------ engine call lists
BOX_CASES = ("mpc_box_qp", "mpc_box_qp_ws", "mpc_box_rollout", "mpc_box_rollout_ws", "mpc_box_lanes_rollout",
             "mpc_box_lanes_rollout_summary", "mpc_box_lanes_rollout_two_chunks")


@pytest.mark.parametrize("case", BOX_CASES)
def test_engine_call_lists(rig, case):  # noqa: F811
    """fallback_iters = 0 makes today's call list; 7 calls the ..._fallback twin with 7 right after max_qp_iters and
    nothing else changed, chunk by chunk."""
    method, make = tl.CASES[case]
    _, calls = tl.run(rig, method, **make(), fallback_iters=0)
    assert calls == tl.EXPECTED[case]
    _, calls = tl.run(rig, method, **make(), fallback_iters=7)
    want = []
    for c in tl.EXPECTED[case]:
        if c[0].endswith("_workspace"):
            want.append(c)
        else:
            k = c.index(32) + 1
            want.append((c[0] + "_fallback",) + c[1:k] + (7,) + c[k:])
    assert calls == want and any(c[0].endswith("_fallback") for c in calls)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="fallback_iters"):
            tl.run(rig, method, **make(), fallback_iters=bad)
