"""The projected-Newton fallback of the torque-limited window QP on the device (gym_mpc_box_qp_fallback,
gym_mpc_box_rollout_fallback, gym_mpc_box_lanes_rollout_fallback, tau_max=TorqueLimit(...)) against the NumPy
restatement tests/box_qp_fallback_ref.py and its fixture tests/golden/mpc_box_hard.npz: window QPs at tau_max = 14 on
which the active set cycles.

Bars.  Window solutions and the solver-independent KKT certificate: 1e-8 max(1, |u|), the bar of
tests/test_gpu_mpc_box.py and tests/test_mpc_box_host.py (the NumPy fallback's own certificates on the fixture are at
most 9.1e-10 absolute, 6.5e-11 of |u|).  "X is the linear rollout of U": the device's X against a NumPy rollout of the
device's own U at 1e-9 max(1, |X|), the project's trajectory bar (74 stages of rounding, amplified by the unstable
window dynamics; two CPU rollouts of one U differ by 9e-13).  Applied controls against the CPU minimiser from the
device's own state: 1e-9 relative, 1e-12 absolute, the bar of test_unconverged_qps_are_reported_not_hidden.  Iteration
counts are compared with the cap only: a stage on its bound to rounding may classify either way.

The first three tests fail without the feature (no fallback_iters, no TorqueLimit): today the closed loops at
tau_max = 14 leave 15, 17, 15, 18, 22, 24 QPs per lane unconverged.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

import box_qp_fallback_ref as fb
import box_qp_ref as bq

pytestmark = pytest.mark.gpu
REL = 1e-8
TOL = 1e-9
CAP = 32
FB = 128
TAU = 14.0
SUMS = ("err_final", "err_max", "u_max")


def _np(t):
    return t.detach().cpu().numpy()


def _tt():
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    return tt


@pytest.fixture(scope="module")
def trk():
    return load_golden("tracking")


@pytest.fixture(scope="module")
def fx():
    return load_golden("mpc_box_hard")


@pytest.fixture(scope="module")
def pb(trk):
    return bq.Problem(trk["x_opt"], trk["u_opt"])


def _gpu_window(pb, w, L, x0, tau=TAU, cap=CAP, fallback_iters=0):
    A, Bm, ur = pb.window(w, L)
    U, X, it, conv = _tt()._eng().mpc_box_qp(A, Bm, ur, pb.Q, pb.R, pb.QT, x0, L, tau, cap,
                                              fallback_iters=fallback_iters)
    return _np(U), _np(X), _np(it), _np(conv)


def _condensed(pb, w, L, tau=TAU):
    A, Bm, ur = pb.window(w, L)
    lo, hi = bq.bounds(ur, tau)
    H, F, _, _ = bq.condense(A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
    return A, Bm, ur, lo, hi, H, F


def _check_applied_controls(pb, x, u, it, steps, L=75, tau=TAU):
    """u[l, s, 1] is apply_limit of the CPU minimiser's first control from the device's own x[l, s]."""
    for s in steps:
        A, Bm, ur = pb.window(s, L)
        lo, hi = bq.bounds(ur, tau)
        e = x[:, s] - pb.x_ref[s]
        U, _, _, conv = fb.solve_window(pb, s, L, e, tau, CAP)
        assert conv.all(), s
        for l in range(x.shape[0]):
            want = bq.apply_limit(ur[0, 1], U[l, 0, 1], lo[0, 1], hi[0, 1], tau)
            print(f"step {s} lane {l} iters {it[l, s]}: u {u[l, s, 1]!r} want {float(want)!r}")
            assert u[l, s, 1] == pytest.approx(want, rel=1e-9, abs=1e-12), (s, l)


def _check_prefix(on, off, it_off, axes):
    """Per closed loop, x and u of the fallback-on run are the fallback-off run's bit for bit up to that run's first
    step at the cap (x one knot further: the state that step starts from)."""
    for idx in np.ndindex(*axes):
        at_cap = np.flatnonzero(it_off[idx] == CAP)
        first = int(at_cap[0]) if at_cap.size else it_off.shape[-1]
        np.testing.assert_array_equal(on[0][idx][:first + 1], off[0][idx][:first + 1])
        np.testing.assert_array_equal(on[1][idx][:first], off[1][idx][:first])


# ------------------------------------------------------------------------------------ 1: window batches
@pytest.mark.parametrize("i", [0, 1], ids=["step227", "step270"])
def test_window_batches_are_solved_by_the_fallback(fx, pb, i):
    w, L = int(fx["win_w"][i]), int(fx["T_pred"])
    E = fx["win_x0"][i]
    A, Bm, ur, lo, hi, H, F = _condensed(pb, w, L)
    U0, X0, it0, conv0 = _gpu_window(pb, w, L, E)
    np.testing.assert_array_equal(conv0 == 0, it0 == CAP)
    hard = conv0 == 0
    assert hard.sum() >= 8 and (~hard).sum() >= 8, (hard.sum(), (~hard).sum())
    U, X, it, conv = _gpu_window(pb, w, L, E, fallback_iters=FB)
    assert (conv == 1).all(), np.flatnonzero(conv != 1)
    worst = 0.0
    for l in range(E.shape[0]):
        bar = REL * max(1.0, np.abs(U[l]).max())
        res = bq.kkt_residual(U[l, :, 1], E[l], H, F, lo[:, 1], hi[:, 1])
        worst = max(worst, res / max(1.0, np.abs(U[l]).max()))
        assert res <= bar, (l, res)
        assert np.abs(U[l] - fx["win_U"][i, l]).max() <= bar, (l, np.abs(U[l] - fx["win_U"][i, l]).max())
    print(f"step {w}: {hard.sum()} lanes in the fallback, iterations <= {it.max()}, worst relative certificate "
          f"{worst:.2e}, worst |U - fixture| {np.abs(U - fx['win_U'][i]).max():.2e}")
    assert (U >= lo[None]).all() and (U <= hi[None]).all()
    Xr, _ = fb._rollout_cost(E, U[:, :, 1], A, Bm[:, :, 1], pb.Q, pb.R[1, 1], pb.QT)
    assert np.abs(X - Xr).max() <= TOL * max(1.0, np.abs(Xr).max()), np.abs(X - Xr).max()
    np.testing.assert_array_equal(U[~hard], U0[~hard])
    np.testing.assert_array_equal(X[~hard], X0[~hard])
    np.testing.assert_array_equal(it[~hard], it0[~hard])
    assert (it[hard] > CAP).all() and (it[hard] <= CAP + FB).all()
    if i == 0:                                                       # B = 1 on one cycling lane
        l = int(np.flatnonzero(hard)[0])
        U1, X1, it1, conv1 = _gpu_window(pb, w, L, E[l:l + 1], fallback_iters=FB)
        assert conv1[0] == 1 and it1[0] > CAP
        np.testing.assert_array_equal(U1[0], U[l])
        np.testing.assert_array_equal(X1[0], X[l])


# ------------------------------------------------------------------------------------ 2: shared-reference closed loop
@pytest.fixture(scope="module")
def shared(fx, trk):
    tt = _tt()
    L = int(fx["T_pred"])
    off = tt.solve_mpc_tracking_box_batch(fx["x0"], trk["x_opt"], trk["u_opt"], TAU, L)
    on = tt.solve_mpc_tracking_box_batch(fx["x0"], trk["x_opt"], trk["u_opt"], tt.TorqueLimit(TAU), L)
    return off, on


def test_shared_reference_closed_loop_has_no_unconverged_qp(fx, trk, pb, shared):
    off, on = shared
    it0, it = _np(off.qp_iters), _np(on.qp_iters)
    assert _np(off.unconverged).tolist() == [15, 17, 15, 18, 22, 24]            # today's counts: the precondition
    assert _np(on.unconverged).tolist() == [0] * 6
    x, u = _np(on.x), _np(on.u)
    assert x.shape == (6, 501, 4) and u.shape == (6, 500, 2)
    assert np.isfinite(x).all() and np.isfinite(u).all() and np.abs(u).max() <= TAU
    assert (it != CAP).all() and (it > CAP).any() and it.max() <= CAP + FB and it.min() >= 1
    print("QPs in the fallback per lane", (it > CAP).sum(1), "iterations <=", it.max())
    _check_prefix((x, u), (_np(off.x), _np(off.u)), it0, (6,))
    assert torch.equal(on.K0, off.K0)
    _check_applied_controls(pb, x, u, it, (100, 222, 240, 262, 276, 400), int(fx["T_pred"]))


# ------------------------------------------------------------------------------------ 3: per-lane kernel
DX = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3)
LANE = 3            # the lane of lanes.npz that rides beside the headline trajectory


@pytest.fixture(scope="module")
def two_lanes(trk):
    g = load_golden("lanes")
    x = np.stack([trk["x_opt"], g["x"][LANE]])
    u = np.stack([trk["u_opt"][:x.shape[1] - 1], g["u"][LANE]])
    x0 = x[:, :1, :] + np.array([[d, -d, 0.0, 0.0] for d in DX])[None]
    return x, u, x0


@pytest.fixture(scope="module")
def lanes_runs(two_lanes):
    tt = _tt()
    x, u, x0 = two_lanes
    off = tt.MPC_tracking_lanes(x, u, x0, tau_max=TAU, gains=False)
    on = tt.MPC_tracking_lanes(x, u, x0, tau_max=tt.TorqueLimit(TAU), gains=False)
    return off, on


def test_per_lane_closed_loops_have_no_unconverged_qp(two_lanes, lanes_runs, pb):
    tt = _tt()
    xo, uo, x0 = two_lanes
    off, on = lanes_runs
    it0, it = _np(off.qp_iters), _np(on.qp_iters)
    assert int(off.unconverged[0].sum()) > 0                                     # precondition: lane 0 cycles today
    np.testing.assert_array_equal(_np(off.unconverged), (it0 == CAP).sum(-1))
    assert int(on.unconverged.abs().sum()) == 0 and (it != CAP).all() and (it[0] > CAP).any()
    x, u = _np(on.x), _np(on.u)
    assert x.shape == (2, 6, 501, 4) and np.isfinite(x).all() and np.isfinite(u).all() and np.abs(u).max() <= TAU
    print("QPs in the fallback per (lane, start)", (it > CAP).sum(-1).tolist(), "iterations <=", it.max())
    _check_prefix((x, u), (_np(off.x), _np(off.u)), it0, (2, 6))
    _check_applied_controls(pb, x[0], u[0], it[0], (100, 222, 250, 276))
    pb1 = bq.Problem(xo[1], uo[1])
    ran = np.flatnonzero((it[1] > CAP).any(0))
    _check_applied_controls(pb1, x[1], u[1], it[1], [int(s) for s in ran[:2]] + [150])
    # the summaries do not depend on whether trajectories are stored
    summ = tt.MPC_tracking_lanes(xo, uo, x0, tau_max=tt.TorqueLimit(TAU), gains=False, trajectories=False)
    assert summ.x is None and summ.qp_iters is None
    for f in SUMS + ("unconverged",):
        assert torch.equal(getattr(summ, f), getattr(on, f)), f
    # one lane per call equals one call
    eng = tt._eng()
    QT = tt._mpc_terminal_weight(eng, tt.Q_MPC, tt.R_MPC)
    args = (eng.t(xo), eng.t(uo), eng.t(x0), tt.Q_MPC, tt.R_MPC, QT, 75, TAU, CAP)
    one = eng.mpc_box_lanes_rollout(*args, fallback_iters=FB)
    chunked = eng.mpc_box_lanes_rollout(*args, max_ws_bytes=eng.mpc_box_lanes_workspace(1, 6, 75), fallback_iters=FB)
    for a, b in zip(one, chunked):
        assert torch.equal(a, b)
    assert torch.equal(one[0], on.x) and torch.equal(one[3], on.qp_iters)


# ------------------------------------------------------------------------------------ 4: invisibility
def test_fallback_is_invisible_where_no_qp_reaches_the_cap(fx, trk, two_lanes):
    tt = _tt()
    L = int(fx["T_pred"])
    xo, uo, x0 = two_lanes
    off = tt.solve_mpc_tracking_box_batch(fx["x0"], trk["x_opt"], trk["u_opt"], 18.0, L)
    on = tt.solve_mpc_tracking_box_batch(fx["x0"], trk["x_opt"], trk["u_opt"], tt.TorqueLimit(18.0), L)
    assert int(off.qp_iters.max()) < CAP and int(off.qp_iters.max()) > 1
    for f in ("x", "u", "K0", "qp_iters", "unconverged"):
        assert torch.equal(getattr(on, f), getattr(off, f)), f
    loff = tt.MPC_tracking_lanes(xo, uo, x0, tau_max=18.0)
    lon = tt.MPC_tracking_lanes(xo, uo, x0, tau_max=tt.TorqueLimit(18.0))
    assert int(loff.qp_iters.max()) < CAP and int(loff.qp_iters.max()) > 1
    for f in ("x", "u", "K", "qp_iters", "unconverged") + SUMS:
        assert torch.equal(getattr(lon, f), getattr(loff, f)), f
    # a limit that never binds: the unconstrained paths bit for bit
    r = tt.solve_mpc_tracking_box_batch(fx["x0"], trk["x_opt"], trk["u_opt"], tt.TorqueLimit(1e6), L)
    x, u, K0 = tt.solve_mpc_tracking_batch(fx["x0"], trk["x_opt"], trk["u_opt"], L)
    assert torch.equal(r.x, x) and torch.equal(r.u, u) and torch.equal(r.K0, K0)
    assert bool((r.qp_iters == 1).all()) and int(r.unconverged.abs().sum()) == 0
    lr = tt.MPC_tracking_lanes(xo, uo, x0, tau_max=tt.TorqueLimit(1e6))
    free = tt.MPC_tracking_lanes(xo, uo, x0)
    for f in ("x", "u", "K") + SUMS:
        assert torch.equal(getattr(lr, f), getattr(free, f)), f
    assert bool((lr.qp_iters == 1).all()) and int(lr.unconverged.abs().sum()) == 0


# ------------------------------------------------------------------------------------ 5: cap honesty
def test_one_newton_iteration_leaves_qps_unconverged_and_feasible(fx, pb):
    w, L = int(fx["win_w"][0]), int(fx["T_pred"])
    E = fx["win_x0"][0]
    lo, hi = bq.bounds(pb.window(w, L)[2], TAU)
    U0, _, it0, conv0 = _gpu_window(pb, w, L, E)
    U, X, it, conv = _gpu_window(pb, w, L, E, fallback_iters=1)
    hard = conv0 == 0
    assert set(np.unique(conv)) <= {0, 1} and (conv[~hard] == 1).all()
    left = conv == 0
    assert 1 <= left.sum() <= hard.sum()
    assert (it[hard] == CAP + 1).all()                              # one Newton iteration each, counted once
    np.testing.assert_array_equal(it[~hard], it0[~hard])
    assert np.isfinite(U).all() and np.isfinite(X).all()
    assert (U >= lo[None]).all() and (U <= hi[None]).all()
    print("unconverged after one Newton iteration:", int(left.sum()), "of", int(hard.sum()))
