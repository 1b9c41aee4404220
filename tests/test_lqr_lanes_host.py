"""Per-lane LQR tracking, host side (CPU only): the ABI surface, and the yardstick of the GPU tests."""
import inspect
import os
import re

import numpy as np

from conftest import ROOT, load_golden, rel_l2

HEADER = os.path.join(ROOT, "include", "gymnast_acrobot.h")
NAMES = ("gym_lqr_lanes_workspace", "gym_lqr_lanes_gains", "gym_lqr_lanes_rollout")


def test_header_and_binding_declare_the_three_entry_points():
    """The header declares the three functions, _lib lists them with the header's arity, and the ABI version the
    existing tests pin is unchanged (the addition is purely additive)."""
    from gymnast_optimalcontrol_amd import _lib
    src = open(HEADER).read()
    assert re.search(r"^#define GYM_ABI_VERSION 18$", src, flags=re.M) and _lib.ABI_VERSION == 18
    for name in NAMES:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in the header"
        assert name in _lib.EXPORTS and name in _lib._SIGS
        assert len(_lib._SIGS[name]) == len(m.group(1).split(",")), name
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine
    from gymnast_optimalcontrol_amd.solver import SolveResult
    for obj, n in ((tt, "LQR_tracking_lanes"), (tt, "lqr_gains_lanes"), (tt, "LqrLanesResult"),
                   (AcrobotEngine, "lqr_lanes_gains"), (AcrobotEngine, "lqr_lanes_rollout"), (SolveResult, "track_lqr")):
        assert hasattr(obj, n), n
    sig = inspect.signature(tt.LQR_tracking_lanes)
    assert [p for p, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == ["trajectories", "gains", "Q", "R", "QT"]


def test_helper_reproduces_the_reference_run_fixture():
    """The lane-by-lane helper fed tracking.npz's one trajectory as a one-lane batch gives the fixture's K_reg /
    x_track / u_track, which the reference's own solve_LQR_tracking / simulate_tracking produced.  The bound is the
    one tests/test_tracking.py pins the oracle's gains to the reference with (1e-10: the oracle's closed-form Jacobians
    against the reference's lambdified ones); the trajectories here run under the helper's own gains, so they carry
    that gain difference too and get the same bound (a factor 10 below the 1e-9 bar the GPU tests then apply)."""
    from lqr_lanes_ref import lanes_ref
    trk = load_golden("tracking")
    x0 = trk["x_opt"][0][None] + trk["dx"][:, None]                        # (2,4): P = 2 starts of the one lane
    r = lanes_ref(trk["x_opt"][None], trk["u_opt"][None], x0[None])
    assert np.abs(r["K"][0] - trk["K_reg"]).max() <= 1e-10 * np.abs(trk["K_reg"]).max()
    assert rel_l2(r["x"][0], trk["x_track"]) < 1e-10 and rel_l2(r["u"][0], trk["u_track"]) < 1e-10
    assert np.array_equal(r["K"][0][:, 0], np.zeros((500, 4)))           # gain row 0: exactly zero
    e = np.abs(trk["x_track"] - trk["x_opt"])
    assert np.allclose(r["err_max"][0], e.max((1, 2)), rtol=1e-9) and r["err_final"].shape == (1, 2)
