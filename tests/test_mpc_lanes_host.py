"""Per-lane MPC tracking, host side (CPU only): the ABI surface, and the yardstick of the GPU tests.

The first three tests need the feature (header, binding, Python surface, the entry point's checks).
test_helper_first_gain_is_the_exact_qp_solution checks only the oracle helper tests/mpc_lanes_ref.py against the dense
KKT solution: it validates the yardstick, not the product."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "gymnast_acrobot.h")
NAMES = ("gym_mpc_lanes_gains",)


def test_header_and_binding_declare_the_entry_point():
    """The header declares gym_mpc_lanes_gains (citing the reference's solve_mpc_tracking), _lib lists it with the
    header's arity, and the ABI version the existing tests pin is unchanged (the addition is purely additive)."""
    from gymnast_optimalcontrol_amd import _lib
    src = open(HEADER).read()
    assert re.search(r"^#define GYM_ABI_VERSION 18$", src, flags=re.M) and _lib.ABI_VERSION == 18
    for name in NAMES:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in the header"
        assert name in _lib.EXPORTS and name in _lib._SIGS
        assert len(_lib._SIGS[name]) == len(m.group(1).split(",")), name
        doc = src[:m.start()].rsplit("/* ----------------", 1)[1]
        assert "trajectory_tracking.py:8-69" in doc, "the header cites the reference's solve_mpc_tracking"


def test_python_surface():
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine
    from gymnast_optimalcontrol_amd.solver import SolveResult
    for obj, n in ((tt, "MPC_tracking_lanes"), (tt, "mpc_gains_lanes"), (tt, "MpcLanesResult"),
                   (AcrobotEngine, "mpc_lanes_gains"), (SolveResult, "track_mpc"), (SolveResult, "track_lqr")):
        assert hasattr(obj, n), n
    sig = inspect.signature(tt.MPC_tracking_lanes)
    assert [p for p, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == ["trajectories", "gains", "T_pred",
                                                                                  "Q", "R", "tau_max", "max_qp_iters"]
    assert list(inspect.signature(AcrobotEngine.mpc_lanes_gains).parameters) == [
        "self", "x_opt", "u_opt", "Q", "R", "QT", "L", "gains", "ws"]
    lqr = [f for f in tt.LqrLanesResult.__dataclass_fields__]
    assert [f for f in tt.MpcLanesResult.__dataclass_fields__] == lqr + ["QT"]


def test_entry_point_refuses_bad_sizes_and_weights_on_the_host():
    """gym_mpc_lanes_gains' argument checks run before any launch (dummy addresses: skipped where a device could run
    one).  Everything right but one argument returns GYM_EINVAL."""
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("dummy device addresses: CPU-only check")
    from gymnast_optimalcontrol_amd import _lib
    lib = _lib.load()
    D = 0x10000
    m = _lib.GymModel(dt=0.02)
    Q, R = np.diag([120.0, 100.0, 1e-4, 1e-4]), np.diag([1e-6, 10.0])
    need = C.c_int64()
    assert lib.gym_lqr_lanes_workspace(12, 501, C.byref(need)) == 0

    def call(m=C.byref(m), x=D, u=D, B=12, N=501, L=75, Q=Q, R=R, QT=D, ws=D, nb=need.value, K=D):
        p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.gym_mpc_lanes_gains(m, x, u, B, N, L, p(Q), p(R), QT, ws, nb, K, None)

    nonsym = Q.copy(); nonsym[0, 1] = 1.0
    offdiag = R.copy(); offdiag[1, 0] = 0.5
    r0 = R.copy(); r0[1, 1] = 0.0
    rneg = R.copy(); rneg[1, 1] = -1.0
    for kw in (dict(m=None), dict(x=None), dict(u=None), dict(Q=None), dict(R=None), dict(QT=None), dict(ws=None),
               dict(B=0), dict(B=_lib.MAX_BP + 1), dict(N=1), dict(L=1), dict(L=255), dict(nb=need.value - 1),
               dict(R=offdiag), dict(R=r0), dict(R=rneg), dict(Q=nonsym)):
        assert call(**kw) == 1, list(kw)


@pytest.mark.parametrize("lane", [0, 9])
def test_helper_first_gain_is_the_exact_qp_solution(lane):
    """The yardstick of the GPU tests (tests/mpc_lanes_ref.py) on lanes of tests/golden/lanes.npz: u0 = K0[t] x0 is
    the dense KKT solution of solver_mpc's QP for the window of control step t of the lane's own trajectory -- the
    first window, two in the middle, and the last ones, whose stages are mostly (499: all but one) the pad.  Tolerances:
    tests/test_tracking.py::test_oracle_mpc_gain_is_the_exact_qp_solution's."""
    from oracle import tracking_np as tr
    from mpc_lanes_ref import gains_ref, window
    g = load_golden("lanes")
    x, u = g["x"][lane], g["u"][lane]
    for Tp in (50, 75):
        K0, QT = gains_ref(x[None], u[None], Tp)
        assert K0.shape == (1, 500, 2, 4) and np.array_equal(K0[0, :, 0], np.zeros((500, 4)))
        for t in (0, 137, 430, 499):
            Aw, Bw = window(x, u, t, Tp)
            x0 = np.random.default_rng(t).uniform(-0.2, 0.2, 4)
            U0, _, _ = tr.mpc_qp_kkt(x0, Aw, Bw, tr.Q_MPC, tr.R_MPC, QT)
            np.testing.assert_allclose(K0[0, t] @ x0, U0, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(U0).max()))
