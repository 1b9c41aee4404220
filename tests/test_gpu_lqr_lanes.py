"""Per-lane LQR tracking on the GPU (gym_lqr_lanes_gains / gym_lqr_lanes_rollout, LQR_tracking_lanes).

Expectation: the committed NumPy oracle applied lane by lane (tests/lqr_lanes_ref.py; pinned to the reference's own
run by tests/test_lqr_lanes_host.py).  Inputs: tests/golden/lanes.npz, 12 lanes the reference itself solved
(Armijo-failure and max-iteration lanes included, so the trajectories differ).  Bars, the project's own
(tests/test_tracking.py, TOL = 1e-9): gains within 1e-9 max|K| per lane, trajectories rel-L2 < 1e-9 per (lane, p).
A relative input perturbation of 1e-13 moves K by at most 16x that and x, u by 1.6x that on these lanes, so the bar
has three decades of room and a wrong index or dropped term cannot hide under it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from lqr_lanes_ref import lanes_ref

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _np(t):
    return t.detach().cpu().numpy()


def _tt():
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    return tt


@pytest.fixture(scope="module")
def lanes():
    g = load_golden("lanes")
    x, u = g["x"], g["u"]
    x0 = x[:, 0][:, None] + np.random.default_rng(11).uniform(-0.1, 0.1, (12, 3, 4))
    return {"x": x, "u": u, "x0": x0, "ref": lanes_ref(x, u, x0)}


def _check_against(res, ref, x_opt, u_opt):
    """K, x, u of an LqrLanesResult with (B,P,...) shapes against the oracle's, at the bars; exact zeros / copies."""
    K, x, u = _np(res.K), _np(res.x), _np(res.u)
    assert K.shape == ref["K"].shape and x.shape == ref["x"].shape and u.shape == ref["u"].shape
    assert np.isfinite(ref["x"]).all() and np.isfinite(ref["K"]).all()
    for b in range(K.shape[0]):
        assert np.abs(K[b] - ref["K"][b]).max() <= TOL * np.abs(ref["K"][b]).max(), b
        for p in range(x.shape[1]):
            ex = np.linalg.norm(x[b, p] - ref["x"][b, p]) / np.linalg.norm(ref["x"][b, p])
            eu = np.linalg.norm(u[b, p] - ref["u"][b, p]) / np.linalg.norm(ref["u"][b, p])
            assert ex < TOL and eu < TOL, (b, p, ex, eu)
    assert np.array_equal(K[:, :, 0, :], np.zeros_like(K[:, :, 0, :]))
    assert np.array_equal(u[..., 0], np.broadcast_to(u_opt[:, None, :, 0], u[..., 0].shape))


def _torch_summaries(res, x_opt):
    """The three maxima with torch from the returned x (B,P,N,4), u (B,P,T,2): subtraction, abs and max are exact."""
    e = (res.x - torch.as_tensor(x_opt, device=res.x.device)[:, None]).abs()
    return e[:, :, -1].amax(-1), e.amax((-1, -2)), res.u[..., 1].abs().amax(-1)


def test_parity_with_the_oracle_lane_by_lane(lanes):
    res = _tt().LQR_tracking_lanes(lanes["x"], lanes["u"], lanes["x0"])
    _check_against(res, lanes["ref"], lanes["x"], lanes["u"])
    ef, em, um = _torch_summaries(res, lanes["x"])
    assert res.err_final.shape == (12, 3)
    assert torch.equal(res.err_final, ef) and torch.equal(res.err_max, em) and torch.equal(res.u_max, um)
    # and they are the oracle's: a maximum of absolute values is 1-Lipschitz in the sup norm, which the 2-norm bounds,
    # so the trajectory bar TOL |ref|_2 carries over to each summary
    ref = lanes["ref"]
    nx, nu = np.linalg.norm(ref["x"], axis=(-1, -2)), np.linalg.norm(ref["u"], axis=(-1, -2))
    for name, bound in (("err_final", nx), ("err_max", nx), ("u_max", nu)):
        assert (np.abs(_np(getattr(res, name)) - ref[name]) <= TOL * bound).all(), name
    K = _tt().lqr_gains_lanes(lanes["x"], lanes["u"])
    assert torch.equal(K, res.K)


def test_lane_position_and_batch_shape_are_invisible(lanes):
    tt = _tt()
    idx = np.arange(130) % 12
    x, u = lanes["x"][idx].copy(), lanes["u"][idx].copy()
    x0 = x[:, 0][:, None] + np.random.default_rng(3).uniform(-0.1, 0.1, (130, 3, 4))
    same = [0, 63, 64, 129]                             # first / last lane of a wavefront, a ragged last group
    x[same], u[same], x0[same] = lanes["x"][5], lanes["u"][5], lanes["x0"][5]
    res = tt.LQR_tracking_lanes(x, u, x0)
    fields = ("x", "u", "K", "err_final", "err_max", "u_max")
    for f in fields:
        t = getattr(res, f)
        for l in same[1:]:
            assert torch.equal(t[l], t[0]), (f, l)
    one = tt.LQR_tracking_lanes(x[64:65], u[64:65], x0[64:65])
    for f in fields:
        assert torch.equal(getattr(one, f)[0], getattr(res, f)[64]), f
    for p in range(3):
        rp = tt.LQR_tracking_lanes(x, u, x0[:, p:p + 1])
        flat = tt.LQR_tracking_lanes(x, u, x0[:, p])    # (B,4): the same call without the P axis
        for f in ("x", "u", "err_final", "err_max", "u_max"):
            assert torch.equal(getattr(rp, f)[:, 0], getattr(res, f)[:, p]), (f, p)
            assert torch.equal(getattr(flat, f), getattr(res, f)[:, p]), (f, p)
        assert torch.equal(rp.K, res.K)
    lean = tt.LQR_tracking_lanes(x, u, x0, trajectories=False, gains=False)
    assert lean.x is None and lean.u is None and lean.K is None
    for f in ("err_final", "err_max", "u_max"):
        assert torch.equal(getattr(lean, f), getattr(res, f)), f


@pytest.fixture(scope="module")
def short(lanes):
    """65 lanes (the 12 tiled, each with its own start) and the oracle on every prefix length used below."""
    idx = np.arange(65) % 12
    x, u = lanes["x"][idx], lanes["u"][idx]
    x0 = x[:, 0][:, None] + np.random.default_rng(7).uniform(-0.1, 0.1, (65, 1, 4))
    return {"x": x, "u": u, "x0": x0, "ref": {n: lanes_ref(x[:, :n], u[:, :n - 1], x0) for n in (2, 3, 33, 34)}}


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("n", [2, 3, 33, 34])
def test_short_and_ragged_horizons(short, n, B):
    """A single stage, and both sides of a pack tile (16 knots of x, 32 of u); one lane and a ragged second group."""
    x, u, x0 = short["x"][:B, :n], short["u"][:B, :n - 1], short["x0"][:B]
    res = _tt().LQR_tracking_lanes(x, u, x0)
    ref = {k: v[:B] for k, v in short["ref"][n].items()}
    _check_against(res, ref, x, u)
    ef, em, um = _torch_summaries(res, x)
    assert torch.equal(res.err_final, ef) and torch.equal(res.err_max, em) and torch.equal(res.u_max, um)


def test_shared_reference_consistency():
    tt = _tt()
    trk = load_golden("tracking")
    x0 = trk["x_opt"][0][None] + trk["dx"][:, None]                       # (2,4)
    B = 70
    res = tt.LQR_tracking_lanes(np.repeat(trk["x_opt"][None], B, 0), np.repeat(trk["u_opt"][None], B, 0),
                                np.repeat(x0[None], B, 0))
    xb, ub, _ = tt.LQR_tracking_batch(trk["x_opt"], trk["u_opt"], x0)
    x, u, xb, ub = _np(res.x), _np(res.u), _np(xb), _np(ub)
    rl2 = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))   # noqa: E731
    for b in range(B):
        for p in range(2):
            assert rl2(x[b, p], trk["x_track"][p]) < TOL and rl2(u[b, p], trk["u_track"][p]) < TOL, (b, p)
            assert rl2(x[b, p], xb[p]) < TOL and rl2(u[b, p], ub[p]) < TOL, (b, p)


def test_nan_start_stays_in_its_lane(lanes):
    """One lane of 65 starts at NaN: its states, its torque channel and its summaries are NaN (channel 0 of u is the
    lane's u_opt[:, 0] itself, never computed, so it stays what it was); every other lane is bitwise the run
    without it."""
    tt = _tt()
    idx = np.arange(65) % 12
    x, u = lanes["x"][idx], lanes["u"][idx]
    x0 = x[:, 0] + np.random.default_rng(9).uniform(-0.1, 0.1, (65, 4))
    clean = tt.LQR_tracking_lanes(x, u, x0)
    bad = x0.copy()
    bad[17] = np.nan
    res = tt.LQR_tracking_lanes(x, u, bad)
    assert torch.isnan(res.x[17]).all() and torch.isnan(res.u[17, :, 1]).all()
    assert torch.equal(res.u[17, :, 0], torch.as_tensor(u[17, :, 0], device=res.u.device))
    for f in ("err_final", "err_max", "u_max"):
        assert torch.isnan(getattr(res, f)[17]), f
    keep = torch.arange(65, device=res.x.device) != 17
    for f in ("x", "u", "K", "err_final", "err_max", "u_max"):
        assert torch.equal(getattr(res, f)[keep], getattr(clean, f)[keep]), f
    assert torch.equal(res.K[17], clean.K[17])          # the gains do not depend on the start


def test_end_to_end_from_a_batched_solve(task2_refs):
    """newton_Algorithm_batch on 8 starts (task-2 settings), then result.track_lqr: the oracle applied to the result's
    own (x, u) copied to the host."""
    from gymnast_optimalcontrol_amd import trajectory_generation as tg
    x_ref, u_ref, _ = task2_refs
    rng = np.random.default_rng(5)
    x0 = np.zeros((8, 4))
    x0[:, :2] = rng.uniform(-0.5, 0.5, (8, 2))
    sol = tg.newton_Algorithm_batch(x0, x_ref, u_ref, max_iters=5000, tol=1e-4, gamma_0=0.1)
    dx0 = rng.uniform(-0.1, 0.1, (8, 2, 4))
    res = sol.track_lqr(dx0=dx0)
    xs, us = _np(sol.x), _np(sol.u)
    ref = lanes_ref(xs, us, xs[:, 0][:, None] + dx0)
    _check_against(res, ref, xs, us)
    one = sol.track_lqr(dx0=dx0[0, 0])                  # (4,): the same offset on every lane, no P axis
    assert one.x.shape == (8, 501, 4) and one.err_max.shape == (8,)
    assert torch.equal(one.x[0], res.x[0, 0])
    own = sol.track_lqr(trajectories=False)             # unperturbed: x0 = x[:, 0]
    assert own.x is None and own.err_max.shape == (8,) and bool(torch.isfinite(own.err_max).all())


def test_bad_arguments(lanes):
    from gymnast_optimalcontrol_amd import _lib
    tt = _tt()
    eng = tt._eng()
    lib = eng.lib
    B, N, P = 12, 501, 3
    x = eng.t(lanes["x"]); u = eng.t(lanes["u"]); x0 = eng.t(lanes["x0"])
    ws = eng.lqr_lanes_workspace(B, N)
    Kb = torch.empty((B, N - 1, 2, 4), dtype=torch.float64, device=eng.device)
    xo = torch.empty((B, P, N, 4), dtype=torch.float64, device=eng.device)
    uo = torch.empty((B, P, N - 1, 2), dtype=torch.float64, device=eng.device)
    sm = torch.empty((3, B, P), dtype=torch.float64, device=eng.device)
    Q, R, QT = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_REG, tt.R_REG, tt.QT_REG))
    m = C.byref(eng.model)
    need = C.c_int64()
    assert lib.gym_lqr_lanes_workspace(B, N, C.byref(need)) == 0 and need.value == ws.numel() == 64 * 8 * (4 * N + 6 * (N - 1))
    for b, n, out in ((B, 1, C.byref(need)), (0, N, C.byref(need)), (_lib.MAX_BP + 1, N, C.byref(need)), (B, N, None)):
        assert lib.gym_lqr_lanes_workspace(b, n, out) == 1, (b, n)

    def gains(m=m, x=x.data_ptr(), u=u.data_ptr(), B=B, N=N, Q=Q, R=R, QT=QT, ws=ws.data_ptr(), nb=ws.numel(),
              K=Kb.data_ptr()):
        p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.gym_lqr_lanes_gains(m, x, u, B, N, p(Q), p(R), p(QT), ws, nb, K, eng.stream)

    def rollout(m=m, x0=x0.data_ptr(), B=B, P=P, N=N, ws=ws.data_ptr(), nb=ws.numel(), xo=xo.data_ptr(),
                uo=uo.data_ptr(), sm=sm.data_ptr()):
        return lib.gym_lqr_lanes_rollout(m, x0, B, P, N, ws, nb, xo, uo, sm, eng.stream)

    assert gains() == 0 and gains(K=None) == 0 and rollout() == 0 and rollout(xo=None, uo=None) == 0
    nonsym = Q.copy(); nonsym[0, 1] = 1.0
    offdiag = R.copy(); offdiag[1, 0] = 0.5
    r0 = R.copy(); r0[1, 1] = 0.0
    rneg = R.copy(); rneg[1, 1] = -1.0
    bad_gains = [dict(N=1), dict(B=0), dict(B=_lib.MAX_BP + 1), dict(R=offdiag), dict(R=r0), dict(R=rneg),
                 dict(Q=nonsym), dict(QT=nonsym), dict(m=None), dict(x=None), dict(u=None), dict(Q=None), dict(R=None),
                 dict(QT=None), dict(ws=None), dict(nb=ws.numel() - 1)]
    for kw in bad_gains:
        assert gains(**kw) == 1, list(kw)
    bad_roll = [dict(N=1), dict(B=0), dict(P=0), dict(B=_lib.MAX_BP + 1), dict(B=1 << 20, P=65), dict(m=None),
                dict(x0=None), dict(ws=None), dict(sm=None), dict(xo=None), dict(uo=None), dict(nb=ws.numel() - 1)]
    for kw in bad_roll:
        assert rollout(**kw) == 1, list(kw)
    torch.cuda.synchronize()
    # the Python surface names the offending shape
    xs, us, x0s = lanes["x"], lanes["u"], lanes["x0"]
    for args, frag in (((xs, us[:11], x0s), "(11, 500, 2)"), ((xs, us[:, :499], x0s), "(12, 499, 2)"),
                       ((xs, us, x0s[:11]), "(11, 3, 4)"), ((xs, us, x0s[..., :3]), "(12, 3, 3)"),
                       ((xs[:, :, :3], us, x0s), "(12, 501, 3)"), ((xs[:, :1], us[:, :0], x0s), "(12, 1, 4)")):
        with pytest.raises(ValueError, match=frag.replace("(", r"\(").replace(")", r"\)")):
            tt.LQR_tracking_lanes(*args)
    with pytest.raises(ValueError, match="diagonal R"):
        tt.LQR_tracking_lanes(xs, us, x0s, R=offdiag)
    with pytest.raises(ValueError, match="symmetric"):
        tt.LQR_tracking_lanes(xs, us, x0s, Q=nonsym)
    # u_opt with N rows is trimmed, as newton_Algorithm trims u_ref
    full = np.concatenate([us, us[:, -1:]], axis=1)
    a, b = tt.LQR_tracking_lanes(xs, full, x0s), tt.LQR_tracking_lanes(xs, us, x0s)
    assert torch.equal(a.x, b.x) and torch.equal(a.K, b.K)
