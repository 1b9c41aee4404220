"""The trackers' argument checks (engine.check_*), called directly: CPU only, no engine, no device.

Every engine method and front-end function of the trackers refuses a bad call through these functions, so each
rejected class is pinned here once, with the message fragment the callers' tests match on."""
import inspect
import os
import re

import numpy as np
import pytest

from gymnast_optimalcontrol_amd import _build, _lib, engine as en

X, U, X0 = np.zeros((3, 5, 4)), np.zeros((3, 4, 2)), np.zeros((3, 2, 4))
Q, R = np.diag([120.0, 100.0, 1e-4, 1e-4]), np.diag([1e-6, 10.0])


def _shape(a):
    return str(tuple(a.shape)).replace("(", r"\(").replace(")", r"\)")


def test_lane_trajectories():
    assert en.check_lane_trajectories(X, U) == (3, 5)
    assert en.check_lane_trajectories(X[:, :2], U[:, :1]) == (3, 2)
    for x in (X[0], X[None], X[..., :3], X[:, :1]):          # wrong rank (2, 4), wrong last axis, N = 1
        with pytest.raises(ValueError, match=r"x_opt must be \(B,N,4\) with N >= 2, got " + _shape(x)):
            en.check_lane_trajectories(x, U[:, :max(x.shape[1] - 1, 0)] if x.ndim == 3 else U)
    for u in (U[:2], U[:, :3], U[..., :1], U[0], U[None], np.zeros((3, 5, 2))):   # B-1 lanes, N-2 rows, axis, rank, N rows
        with pytest.raises(ValueError, match=r"u_opt must be \(3,4,2\) for x_opt \(3, 5, 4\), got " + _shape(u)):
            en.check_lane_trajectories(X, u)
    # the front end's extra rule: N rows pass (it trims the last), nothing else does
    assert en.check_lane_trajectories(X, np.zeros((3, 5, 2)), or_n_rows=True) == (3, 5)
    assert en.check_lane_trajectories(X, U, or_n_rows=True) == (3, 5)
    for u in (U[:2], U[:, :3], np.zeros((3, 6, 2)), np.zeros((2, 5, 2)), np.zeros((3, 5, 3))):
        with pytest.raises(ValueError, match=r"\(or 5 rows\).*got " + _shape(u)):
            en.check_lane_trajectories(X, u, or_n_rows=True)


def test_lane_starts():
    assert en.check_lane_starts(X0) is None and en.check_lane_starts(X0, 3) is None
    assert en.check_lane_starts(X0[:, 0], 3, flat_ok=True) is None and en.check_lane_starts(X0, 3, flat_ok=True) is None
    for x0 in (X0[:, 0], X0[None], X0[..., :3], X0[:, :0], X0[:0]):             # rank 2 / 4, last axis 3, P = 0, B = 0
        with pytest.raises(ValueError, match=r"x0 must be \(B,P,4\), got " + _shape(x0)):
            en.check_lane_starts(x0)
    for x0 in (X0[:2], X0[..., :3], X0[:, 0], X0[:, :0], np.zeros((4, 2, 4))):   # wrong B, last axis 3, rank, P = 0
        with pytest.raises(ValueError, match=r"x0 must be \(3,P,4\), got " + _shape(x0)):
            en.check_lane_starts(x0, 3)
    for x0 in (X0[:2], X0[:2, 0], X0[..., :3], X0[:, 0, :3], X0[0, 0], X0[None], X0[:, :0]):
        with pytest.raises(ValueError, match=r"x0 must be \(3,4\) or \(3,P,4\), got " + _shape(x0)):
            en.check_lane_starts(x0, 3, flat_ok=True)


@pytest.mark.parametrize("what", ["per-lane LQR tracking", "per-lane MPC tracking", "the torque-limited QP"])
def test_diagonal_R(what):
    Rh = en.check_diagonal_R(R, what)
    assert Rh.dtype == np.float64 and Rh.flags.c_contiguous and np.array_equal(Rh, R)
    assert np.array_equal(en.check_diagonal_R(R.tolist(), what), R)
    assert en.check_diagonal_R(np.diag([0.0, 1e-300]), what)[1, 1] == 1e-300     # R[0][0] is not this check's business
    bad = []
    for ij in ((0, 1), (1, 0)):
        off = R.copy(); off[ij] = 0.5
        bad.append(off)
    for v in (0.0, -1.0, np.inf, -np.inf, np.nan):
        r = R.copy(); r[1, 1] = v
        bad.append(r)
    for r in bad:
        with pytest.raises(ValueError, match=what + r" needs a diagonal R with R\[1\]\[1\] > 0"):
            en.check_diagonal_R(r, what)
    with pytest.raises(ValueError, match="R must be 2x2"):
        en.check_diagonal_R(np.eye(3), what)


@pytest.mark.parametrize("name", ["Q", "QT"])
def test_symmetric_weight(name):
    M = Q.copy(); M[0, 3] = M[3, 0] = 2.5
    Mh = en.check_sym_weight(M, name)
    assert Mh.dtype == np.float64 and Mh.flags.c_contiguous and np.array_equal(Mh, M)
    for ij in ((0, 1), (3, 2), (2, 0)):
        bad = Q.copy(); bad[ij] = 1.0
        with pytest.raises(ValueError, match=name + " must be symmetric"):
            en.check_sym_weight(bad, name)
    nan = Q.copy(); nan[1, 2] = nan[2, 1] = np.nan                                  # NaN != NaN: not symmetric
    with pytest.raises(ValueError, match="symmetric"):
        en.check_sym_weight(nan, name)
    with pytest.raises(ValueError, match=name + " must be 4x4"):
        en.check_sym_weight(np.eye(2), name)


@pytest.mark.parametrize("what", ["per-lane MPC tracking", "the torque-limited QP"])
def test_window(what):
    assert _lib.MPC_MAX_STAGES == 256
    # one statement: the ABI header defines it and the kernels' LDS table takes its size from that name
    hdr = open(os.path.join(_build.INCLUDE, "gymnast_acrobot.h")).read()
    hpp = open(os.path.join(_build.CSRC, "mpc_gains.hpp")).read()
    assert re.findall(r"^#define GYM_MPC_MAX_STAGES (\d+)\b", hdr, flags=re.M) == ["256"]
    assert re.findall(r"\bkMpcMaxStages\s*=\s*(\w+)\s*;", hpp) == ["GYM_MPC_MAX_STAGES"]
    assert en.check_window(2, what) == 2 and en.check_window(254, what) == 254
    assert en.check_window(np.int64(75), what) == 75 and type(en.check_window(np.int64(75), what)) is int
    for L in (1, 255, 0, -3, 256, 1 << 20):
        with pytest.raises(ValueError, match=r"T_pred must be in \[2, 254\] for " + what + f", got {L}$"):
            en.check_window(L, what)


def test_box():
    assert en.check_box(18.0, 32) is None and en.check_box(1e-300, 1) is None and en.check_box(1.7e308, 1) is None
    for tau in (0.0, -1.0, np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="tau_max must be finite and positive"):
            en.check_box(tau, 32)
    for it in (0, -1):
        with pytest.raises(ValueError, match="max_qp_iters must be at least 1"):
            en.check_box(18.0, it)


def test_device_QT():
    QT = np.zeros((4, 4))
    assert en.check_device_QT(QT) is QT
    for bad in (np.zeros(16), np.zeros((1, 4, 4)), np.zeros((4, 2)), np.zeros((2, 4))):
        with pytest.raises(ValueError, match=r"QT must be \(4,4\), got " + _shape(bad)):
            en.check_device_QT(bad)


def test_rows():
    """At least the rows a kernel reads, of exactly the row shape it reads; spare trailing rows pass."""
    a = np.zeros((6, 4, 2))
    assert en.check_rows(a, 6, (4, 2), "Bm") is a and en.check_rows(a, 1, (4, 2), "Bm") is a
    assert en.check_rows(U[0], 4, (2,), "u_ref").shape == (4, 2) and en.check_rows(a[:0], 0, (4, 2), "Bm").shape[0] == 0
    with pytest.raises(ValueError, match=r"^Bm must be \(>=7,4,2\), got \(6, 4, 2\)$"):
        en.check_rows(a, 7, (4, 2), "Bm")
    for bad in (np.zeros((6, 2, 4)), np.zeros((6, 8)), np.zeros((6, 4, 2, 1)), np.zeros(6)):
        with pytest.raises(ValueError, match=r"^Bm must be \(>=6,4,2\), got " + _shape(bad)):
            en.check_rows(bad, 6, (4, 2), "Bm")
    with pytest.raises(ValueError, match=r"^x_ref must be \(>=5,4\), got \(4, 4\)$"):
        en.check_rows(np.zeros((4, 4)), 5, (4,), "x_ref")


def test_trajectory():
    """x (B,N,4); u and sigma (B,>=N-1,2); a shared reference of >= N and >= N-1 rows: what the kernels read."""
    xr, ur, s = np.zeros((5, 4)), np.zeros((4, 2)), np.zeros((3, 4, 2))
    assert en.check_trajectory(X, U, xr, ur) == (3, 5) and en.check_trajectory(X, U, xr, ur, s) == (3, 5)
    assert en.check_trajectory(X[:, :2], U[:, :1], xr[:2], ur[:1], s[:, :1]) == (3, 2)
    spare = np.zeros((3, 5, 2))
    assert en.check_trajectory(X, spare, np.zeros((7, 4)), np.zeros((6, 2)), spare) == (3, 5)
    for x in (X[0], X[None], X[..., :3], X[:, :1]):
        with pytest.raises(ValueError, match=r"^x must be \(B,N,4\) with N >= 2, got " + _shape(x)):
            en.check_trajectory(x, U, xr, ur)
    for bad in (U[:2], U[:, :3], U[..., :1], U[0], U[None], np.zeros((4, 4, 2))):   # lanes, rows, channels, rank
        with pytest.raises(ValueError, match=r"^u must be \(3,>=4,2\) for x \(3, 5, 4\), got " + _shape(bad)):
            en.check_trajectory(X, bad, xr, ur)
        with pytest.raises(ValueError, match=r"^sigma must be \(3,>=4,2\) for x \(3, 5, 4\), got " + _shape(bad)):
            en.check_trajectory(X, U, xr, ur, bad)
    for bad in (xr[:4], np.zeros((5, 3)), np.zeros((1, 5, 4))):
        with pytest.raises(ValueError, match=r"^x_ref must be \(>=5,4\), got " + _shape(bad)):
            en.check_trajectory(X, U, bad, ur)
    for bad in (ur[:3], np.zeros((4, 1)), np.zeros(4)):
        with pytest.raises(ValueError, match=r"^u_ref must be \(>=4,2\), got " + _shape(bad)):
            en.check_trajectory(X, U, xr, bad)


def test_select():
    import torch
    soa = torch.zeros((5, 2, 64, 2), dtype=torch.float64)
    sel = torch.zeros(3, dtype=torch.int32)
    assert en.check_select(soa, None, None, 3) is None and en.check_select(soa, soa.clone(), sel, 3) is None
    assert en.check_select(soa, soa, torch.zeros(64, dtype=torch.int32), 3) is None
    for bad in (soa[:4], soa[:, :1], soa[..., :1], soa[0]):
        with pytest.raises(ValueError, match=r"^soa1 must be \(5, 2, 64, 2\) like soa, got " + _shape(bad)):
            en.check_select(soa, bad, sel, 3)
    for bad in (sel[:2], sel.to(torch.int64), sel.to(torch.float64), torch.zeros((3, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"^sel must be int32 \(>=3,\), got "):
            en.check_select(soa, soa, bad, 3)


def test_front_end_refuses_through_the_same_checks_before_any_device():
    """trajectory_tracking's torque-limited paths run check_box / check_window first: no engine is made for a refused
    call.  MPC_tracking_lanes names its keywords, so an unknown one is Python's own TypeError."""
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    sig = inspect.signature(tt.MPC_tracking_lanes)
    assert not any(p.kind is p.VAR_KEYWORD for p in sig.parameters.values())
    assert sig.parameters["tau_max"].default is None and sig.parameters["max_qp_iters"].default == 32
    assert tt._check_box(18.0, 75, 32) is None
    for args, frag in (((0.0, 75, 32), "tau_max"), ((np.nan, 75, 32), "tau_max"), ((18.0, 75, 0), "max_qp_iters"),
                       ((18.0, 1, 32), "T_pred"), ((18.0, 255, 32), "T_pred")):
        with pytest.raises(ValueError, match=frag):
            tt._check_box(*args)
    x, u = np.zeros((1, 3, 4)), np.zeros((1, 2, 2))
    with pytest.raises(TypeError, match="taumax"):
        tt.MPC_tracking_lanes(x, u, x[:, 0], taumax=18.0)
    with pytest.raises(ValueError, match="max_qp_iters"):
        tt.MPC_tracking_lanes(x, u, x[:, 0], tau_max=18.0, max_qp_iters=0)
