"""Torque-limited Newton solve, CPU side: the two entry points' host checks and the NumPy restatement
(tests/newton_box_ref.py) the GPU tests compare against.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

import newton_box_ref as nb
from conftest import rel_l2
from oracle import acrobot_np as onp

SHORT = dict(tol=1e-4, beta=0.7, c=0.5, max_ls=20)


def short_setup(task2_refs):
    return nb.short_setup(task2_refs[0], task2_refs[1])


def test_box_entry_points_are_exported_and_check_their_arguments():
    """gym_newton_run_box / gym_newton_sigma_box exist and return GYM_EINVAL from their host-side checks (NULL
    pointers, bad sizes, the flags no box kernel supports) before anything is launched."""
    from gymnast_optimalcontrol_amd import _build, _lib
    lib = _lib.load(_build.build())
    box = _lib.EXTENSIONS["gymnast_acrobot_box.h"]
    assert box == ("gym_newton_run_box", "gym_newton_sigma_box")
    assert not set(box) & set(_lib.EXPORTS)                         # the main header's ABI is unchanged
    P, S = _lib._P, C.POINTER
    assert _lib._EXT_SIGS["gym_newton_run_box"] == [S(_lib.GymModel), S(_lib.GymWeights), S(_lib.GymArmijo),
                                                    S(_lib.GymBatch), P, C.c_int32, C.c_int32, P]
    assert _lib._EXT_SIGS["gym_newton_sigma_box"] == [S(_lib.GymModel), S(_lib.GymWeights), S(_lib.GymBatch), P, P, P]
    assert lib.gym_newton_run_box.argtypes == _lib._EXT_SIGS["gym_newton_run_box"]
    D = 0x10000
    m, w, a = _lib.GymModel(dt=0.02), _lib.GymWeights(), _lib.GymArmijo(1e-4, 0.7, 0.5, 0.1, 20, 0)

    def batch(B=64, Bp=64, N=501, flags=0):
        b = _lib.GymBatch(B=B, Bp=Bp, N=N, flags=flags)
        for f, t in _lib.GymBatch._fields_:
            if f in ("x", "u"):
                getattr(b, f)[0] = getattr(b, f)[1] = D
            elif t is _lib._P and f not in ("hist_cost", "hist_smax", "lane_map"):
                setattr(b, f, D)
        return b

    R = C.byref
    ok = batch()
    assert lib.gym_newton_run_box(None, None, None, None, None, 0, 1, None) == 1
    assert lib.gym_newton_sigma_box(None, None, None, None, None, None) == 1
    assert lib.gym_newton_run_box(R(m), R(w), R(a), R(ok), None, 0, 1, None) == 1          # tau_max NULL
    assert lib.gym_newton_sigma_box(R(m), R(w), R(ok), None, D, None) == 1
    assert lib.gym_newton_sigma_box(R(m), R(w), R(ok), D, None, None) == 1                  # sigma_out NULL
    assert lib.gym_newton_run_box(None, R(w), R(a), R(ok), D, 0, 1, None) == 1
    assert lib.gym_newton_run_box(R(m), R(w), None, R(ok), D, 0, 1, None) == 1
    assert lib.gym_newton_run_box(R(m), R(w), R(a), R(ok), D, 5, 1, None) == 1             # k1 < k0
    assert lib.gym_newton_run_box(R(m), R(w), R(a), R(ok), D, -1, 1, None) == 1
    bad_ls = _lib.GymArmijo(1e-4, 0.7, 0.5, 0.1, 0, 0)
    assert lib.gym_newton_run_box(R(m), R(w), R(bad_ls), R(ok), D, 0, 1, None) == 1        # max_ls < 1
    for b in (batch(B=0), batch(B=65, Bp=64), batch(B=60, Bp=100), batch(N=1), batch(Bp=_lib.MAX_BP + 64),
              batch(flags=_lib.FLAG_X_CKPT), batch(flags=_lib.FLAG_REF_LANE | _lib.FLAG_X_CKPT)):
        assert lib.gym_newton_run_box(R(m), R(w), R(a), R(b), D, 0, 1, None) == 1, (b.B, b.Bp, b.N, b.flags)
        assert lib.gym_newton_sigma_box(R(m), R(w), R(b), D, D, None) == 1, (b.B, b.Bp, b.N, b.flags)
    assert lib.gym_newton_run_box(R(m), R(w), R(a), R(batch(flags=_lib.FLAG_SIGMA_STREAM)), D, 0, 1, None) == 1


def test_solve_result_carries_the_limits():
    """SolveResult.tau_max: None unless the solve was limited."""
    import dataclasses
    from gymnast_optimalcontrol_amd.results import SolveResult
    f = {x.name: x for x in dataclasses.fields(SolveResult)}
    assert "tau_max" in f and f["tau_max"].default is None


def test_restatement_without_a_limit_is_the_oracle(task2_refs):
    x0, xr, ur = short_setup(task2_refs)
    o = onp.newton_solve(x0, xr, ur, 60, gamma_0=0.5, **SHORT)
    r = nb.newton_box_solve(x0, xr, ur, 60, np.inf, gamma_0=0.5, **SHORT)
    for k in ("n_iter", "status", "n_rollouts"):
        assert np.array_equal(o[k], r[k]), k
    assert not r["clamped"].any()
    # the two differ only in how the 2x2 solve is written
    assert rel_l2(r["x"], o["x"]) < 1e-10 and rel_l2(r["u"], o["u"]) < 1e-10


@pytest.mark.parametrize("tau", [4.0, 2.0, 1.0])
def test_restatement_with_active_bounds(task2_refs, tau):
    x0, xr, ur = short_setup(task2_refs)
    r = nb.newton_box_solve(x0, xr, ur, 60, tau, gamma_0=0.5, **SHORT)
    print("tau", tau, "iterations", r["n_iter"], "rollouts", r["n_rollouts"], "clamped", r["clamped"].sum(1))
    assert (r["status"] == nb.CONVERGED).all()
    assert (np.abs(r["u"][:, :, 1]) <= tau).all()                 # no tolerance
    assert r["clamped"].any(1).all()
    assert not r["K"][r["clamped"]].any()                         # clamped stages: a zero gain row
    assert r["K"][~r["clamped"]][:, 1].any(1).all()               # the others keep theirs
    assert not r["K"][:, :, 0].any()


def test_clip_keeps_nan():
    v = nb.clip_nan(np.array([np.nan, -3.0, 0.5, 3.0, np.inf, -np.inf]), 2.0)
    assert np.isnan(v[0]) and np.array_equal(v[1:], [-2.0, 0.5, 2.0, 2.0, -2.0])
    assert np.array_equal(nb.clip_nan(np.array([-3.0, 7.0]), np.inf), [-3.0, 7.0])
    assert np.isnan(nb.clip_nan(np.nan, np.inf))
