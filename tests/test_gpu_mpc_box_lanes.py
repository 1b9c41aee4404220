"""Per-lane torque-limited MPC tracking on the GPU (gym_mpc_box_lanes_rollout, MPC_tracking_lanes(tau_max=...)).

Expectation: the NumPy reference of the torque-limited QP applied lane by lane (tests/mpc_box_lanes_ref.py:
box_qp_ref.Problem / closed_loop on every lane's own trajectory), recorded at full length for the 12 lanes of
tests/golden/lanes.npz in tests/golden/mpc_box_lanes.npz (tau_max 18, T_pred 75, the three starts of
tests/test_gpu_mpc_lanes.py) and computed here on short prefixes.  Bar: the project's rel-L2 < 1e-9 per (lane, start) on
x and u, applied to every pair whose reference run has no unconverged QP (35 of the fixture's 36: lane 9 from + 0.1 has
14 QPs whose active set cycles, and its closed loop diverges).  A 1e-13 relative perturbation of all inputs moves the
reference's own result by at most 38x that in x and 198x in u at full length, 88x and 782x on the prefixes used below,
so the bar has more than a decade and a half of room.  Iteration counts are only checked to lie in [1, cap]: a sweep
more or less near a tie is not an error.  Where no bound is ever active the kernel must reproduce the unlimited path
(gym_mpc_lanes_gains + gym_lqr_lanes_rollout) bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from mpc_box_lanes_ref import lanes_ref, rel_l2, starts

pytestmark = pytest.mark.gpu
TOL = 1e-9
CAP = 32
SUMS = ("err_final", "err_max", "u_max")
OUT = ("x", "u", "qp_iters", "unconverged") + SUMS


def _np(t):
    return t.detach().cpu().numpy()


def _tt():
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    return tt


@pytest.fixture(scope="module")
def lanes():
    g = load_golden("lanes")
    return {"x": g["x"], "u": g["u"], "x0": starts(g["x"]), "fx": load_golden("mpc_box_lanes")}


@pytest.fixture(scope="module")
def full(lanes):
    """The 12 lanes x 3 starts at full length, tau_max 18, T_pred 75: one call, shared by the tests that read it."""
    return _tt().MPC_tracking_lanes(lanes["x"], lanes["u"], lanes["x0"], tau_max=18.0)


def _check_summaries(res, x_opt):
    e = (res.x - torch.as_tensor(x_opt, device=res.x.device)[:, None]).abs()
    assert torch.equal(res.err_final, e[:, :, -1].amax(-1)) and torch.equal(res.err_max, e.amax((-1, -2)))
    assert torch.equal(res.u_max, res.u[..., 1].abs().amax(-1))


def _check_counts(res, cap=CAP):
    it = res.qp_iters
    assert it.dtype == torch.int32 and res.unconverged.dtype == torch.int32
    assert int(it.min()) >= 1 and int(it.max()) <= cap
    assert torch.equal(res.unconverged, (it == cap).sum(-1).to(torch.int32))


def _equal(a, b, fields=OUT):
    for f in fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_parity_at_full_length_against_the_fixture(lanes, full):
    tt = _tt()
    fx = lanes["fx"]
    assert isinstance(full, tt.MpcBoxLanesResult) and np.array_equal(fx["x0"], lanes["x0"])
    x, u = _np(full.x), _np(full.u)
    assert x.shape == (12, 3, 501, 4) and u.shape == (12, 3, 500, 2) and full.qp_iters.shape == (12, 3, 500)
    assert full.unconverged.shape == (12, 3) and full.err_max.shape == (12, 3)
    skipped = []
    for b in range(12):
        for p in range(3):
            if fx["unconverged"][b, p]:
                skipped.append((b, p))
                continue
            ex, eu = rel_l2(x[b, p], fx["x"][b, p]), rel_l2(u[b, p], fx["u"][b, p])
            print(f"lane {b} start {p}: rel-L2 x {ex:.2e} u {eu:.2e}")
            assert ex < TOL and eu < TOL, (b, p, ex, eu)
            assert int(full.unconverged[b, p]) == 0 and int(fx["qp_iters"][b, p].max()) <= 5
    assert len(skipped) <= 1, skipped
    assert np.abs(u).max() <= 18.0
    assert ((np.abs(u[..., 1]) == 18.0).sum((1, 2)) > 0).all()          # every lane has a step exactly on the limit
    assert np.array_equal(u[..., 0], np.broadcast_to(lanes["u"][:, None, :, 0], u[..., 0].shape))
    _check_counts(full)
    _check_summaries(full, lanes["x"])
    free = tt.MPC_tracking_lanes(lanes["x"], lanes["u"], lanes["x0"], trajectories=False)
    assert torch.equal(full.K, free.K) and torch.equal(full.QT, free.QT)   # the QPs' first iterate: the free gains
    assert bool((free.u_max > 18.0).all())                                 # which the limit forbids on every lane


@pytest.fixture(scope="module")
def prefix(lanes):
    """ref(lane, n, Tp): the reference's closed loop on the lane's prefix of n knots at horizon Tp from its three
    starts, tau_max = round(0.8 max|u_opt[:, 1]|, 3) so that the limit binds early; computed once per case."""
    cache = {}

    def ref(lane, n, Tp):
        if (lane, n, Tp) not in cache:
            x, u = lanes["x"][[lane], :n], lanes["u"][[lane], :n - 1]
            tau = round(0.8 * float(np.abs(u[0, :, 1]).max()), 3)
            cache[(lane, n, Tp)] = (x, u, lanes["x0"][[lane]], tau, lanes_ref(x, u, lanes["x0"][[lane]], tau, Tp))
        return cache[(lane, n, Tp)]

    return ref


CASES = [(lane, n, Tp) for lane in (0, 9, 10) for n in (34, 66, 130) for Tp in (2, 3, 12, 75)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["lane%d-N%d-T%d" % c for c in CASES])
def test_small_shapes(prefix, case):
    """Windows that are mostly pad, a ring of 1 or 2 rows, L - 1 > N - 1; P = 1, 3, 64, 65 (65: a second start block
    holding one thread) and B = 1, 3, dealt over the cases (every P meets every horizon and every B).  The starts are
    the reference's three, repeated; every (lane copy, start) is held to the reference."""
    lane, n, Tp = CASES[case]
    x, u, x0, tau, ref = prefix(lane, n, Tp)
    assert not ref["unconverged"].any() and 1 <= ref["qp_iters"].min() and ref["qp_iters"].max() <= 15
    assert (np.abs(ref["u"][0, :, :, 1]) == tau).any()
    P = (1, 3, 64, 65)[(case + case // 4) % 4]
    B = (1, 3)[(case // 4 + case // 12) % 2]
    pick = np.arange(P) % 3
    res = _tt().MPC_tracking_lanes(np.repeat(x, B, 0), np.repeat(u, B, 0), np.repeat(x0[:, pick], B, 0), T_pred=Tp,
                                   tau_max=tau)
    xs, us = _np(res.x), _np(res.u)
    assert xs.shape == (B, P, n, 4) and us.shape == (B, P, n - 1, 2)
    worst = [0.0, 0.0]
    for b in range(B):
        for p in range(P):
            ex, eu = rel_l2(xs[b, p], ref["x"][0, pick[p]]), rel_l2(us[b, p], ref["u"][0, pick[p]])
            worst = [max(worst[0], ex), max(worst[1], eu)]
            assert ex < TOL and eu < TOL, (b, p, ex, eu)
    print(f"lane {lane} N {n} T_pred {Tp} B {B} P {P} tau {tau}: worst rel-L2 x {worst[0]:.2e} u {worst[1]:.2e}")
    assert np.abs(us).max() <= tau and (np.abs(us[..., 1]) == tau).any()
    _check_counts(res)
    assert int(res.unconverged.max()) == 0
    _check_summaries(res, np.repeat(x, B, 0))


@pytest.mark.parametrize("Tp", [50, 75])
def test_a_limit_that_never_binds_is_the_unlimited_path_bit_for_bit(lanes, Tp):
    tt = _tt()
    free = tt.MPC_tracking_lanes(lanes["x"], lanes["u"], lanes["x0"], T_pred=Tp)
    box = tt.MPC_tracking_lanes(lanes["x"], lanes["u"], lanes["x0"], T_pred=Tp, tau_max=1e6)
    _equal(box, free, ("x", "u", "K", "QT") + SUMS)
    assert bool((box.qp_iters == 1).all()) and bool((box.unconverged == 0).all())
    assert type(free) is tt.MpcLanesResult and type(box) is tt.MpcBoxLanesResult


def test_without_a_limit_nothing_changed(lanes):
    """tau_max=None is the call without the keyword: the same type, fields and bits."""
    tt = _tt()
    a = tt.MPC_tracking_lanes(lanes["x"][:3], lanes["u"][:3], lanes["x0"][:3])
    b = tt.MPC_tracking_lanes(lanes["x"][:3], lanes["u"][:3], lanes["x0"][:3], tau_max=None, max_qp_iters=7)
    assert type(a) is tt.MpcLanesResult and type(b) is tt.MpcLanesResult
    assert [f for f in type(b).__dataclass_fields__] == ["x", "u", "K", "err_final", "err_max", "u_max", "QT"]
    _equal(a, b, ("x", "u", "K", "QT") + SUMS)


def test_batch_shape_position_and_options_are_invisible(lanes, full):
    """A lane's results depend on its inputs and the start only: not on B, its position, P (the start's block and
    thread), whether trajectories or gains are asked for, or the lane chunks of a small workspace."""
    tt = _tt()
    eng = tt._eng()
    n, Tp = 130, 75
    idx = np.array([3, 5, 9, 5, 0, 5])
    x, u = lanes["x"][idx, :n], lanes["u"][idx, :n - 1]
    x0 = lanes["x0"][idx][:, np.arange(67) % 3]                          # 67 starts: blocks of 64 and 3
    x0[:, 66] = x0[:, 1]
    res = tt.MPC_tracking_lanes(x, u, x0, T_pred=Tp, tau_max=12.0)
    _check_counts(res)
    assert bool((res.u.abs() <= 12.0).all()) and bool((res.u[..., 1].abs() == 12.0).any())
    for f in OUT:
        t = getattr(res, f)
        for l in (3, 5):                                                 # the same lane at positions 1, 3, 5
            assert torch.equal(t[l], t[1]), (f, l)
        for p in range(3, 67):                                           # the same start at other threads / blocks
            assert torch.equal(t[:, p], t[:, p % 3 if p < 66 else 1]), (f, p)
    one = tt.MPC_tracking_lanes(x[1:2], u[1:2], x0[1:2, 1:2], T_pred=Tp, tau_max=12.0)     # B = 1, P = 1
    flat = tt.MPC_tracking_lanes(x[1:2], u[1:2], x0[1:2, 1], T_pred=Tp, tau_max=12.0)      # (B,4): no P axis
    for f in OUT:
        assert torch.equal(getattr(one, f)[0, 0], getattr(res, f)[1, 1]), f
        assert torch.equal(getattr(flat, f)[0], getattr(res, f)[1, 1]), f
    assert flat.x.shape == (1, n, 4) and flat.unconverged.shape == (1,) and flat.qp_iters.shape == (1, n - 1)
    lean = tt.MPC_tracking_lanes(x, u, x0, T_pred=Tp, tau_max=12.0, trajectories=False, gains=False)
    assert lean.x is None and lean.u is None and lean.K is None and lean.qp_iters is None
    _equal(lean, res, SUMS + ("unconverged", "QT"))
    # lane chunks: a workspace limit of two lanes' worth, then of less than one lane's (one lane per call)
    per_lane = eng.mpc_box_lanes_workspace(1, 67, Tp)
    assert eng.mpc_box_lanes_workspace(6, 67, Tp) == 6 * per_lane
    xd, ud, x0d = eng.t(x), eng.t(u), eng.t(x0)
    for limit in (2 * per_lane + 5, 1):
        xs, us, sm, it, un = eng.mpc_box_lanes_rollout(xd, ud, x0d, tt.Q_MPC, tt.R_MPC, res.QT, Tp, 12.0,
                                                       max_ws_bytes=limit)
        assert torch.equal(xs, res.x) and torch.equal(us, res.u) and torch.equal(it, res.qp_iters)
        assert torch.equal(un, res.unconverged) and torch.equal(sm[0], res.err_final)
        assert torch.equal(sm[1], res.err_max) and torch.equal(sm[2], res.u_max)
    # the fixture's full-length call again, one lane and one start at a time
    solo = tt.MPC_tracking_lanes(lanes["x"][7:8], lanes["u"][7:8], lanes["x0"][7:8, 2:3], tau_max=18.0)
    for f in OUT:
        assert torch.equal(getattr(solo, f)[0, 0], getattr(full, f)[7, 2]), f


def test_shared_reference_kernel_agrees(lanes, full):
    """A one-lane batch against solve_mpc_tracking_box_batch on that lane as the shared reference: other kernels
    (k_mpc_gains<true>'s 16-lanes-per-map table, a stage table from disc_stage), so the bar is TOL."""
    tt = _tt()
    for b in (0, 10):
        sh = tt.solve_mpc_tracking_box_batch(lanes["x0"][b], lanes["x"][b], lanes["u"][b], 18.0)
        assert int(sh.unconverged.max()) == 0
        xs, us = _np(sh.x), _np(sh.u)
        for p in range(3):
            ex, eu = rel_l2(_np(full.x[b, p]), xs[p]), rel_l2(_np(full.u[b, p]), us[p])
            assert ex < TOL and eu < TOL, (b, p, ex, eu)


def test_unconverged_qps_are_reported(lanes, full):
    """Lane 9 from + 0.1: the reference's active set cycles on 14 QPs and the closed loop diverges.  The device reports
    what it did: finite outputs inside the limit, the count of QPs at the cap."""
    fx = lanes["fx"]
    assert int(fx["unconverged"][9, 1]) > 0
    x, u, it = full.x[9, 1], full.u[9, 1], full.qp_iters[9, 1]
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(u).all()) and bool((u.abs() <= 18.0).all())
    n = int(full.unconverged[9, 1])
    print(f"lane 9 start 1: {n} unconverged QPs on the device, {int(fx['unconverged'][9, 1])} in the reference")
    assert n == int((it == CAP).sum()) and 1 <= n <= 500
    assert all(bool(torch.isfinite(getattr(full, f)[9, 1])) for f in SUMS)
    # a cap of 1: every QP is its clipped first iterate, and every one is reported
    one = _tt().MPC_tracking_lanes(lanes["x"][9:10, :66], lanes["u"][9:10, :65], lanes["x0"][9:10], tau_max=18.0,
                                   max_qp_iters=1)
    assert bool((one.qp_iters == 1).all()) and bool((one.unconverged == 65).all())
    assert bool(torch.isfinite(one.x).all()) and bool((one.u.abs() <= 18.0).all())


def test_nan_stage_stays_in_its_lane(lanes):
    tt = _tt()
    n = 130
    x, u, x0 = lanes["x"][:3, :n].copy(), lanes["u"][:3, :n - 1], lanes["x0"][:3]
    clean = tt.MPC_tracking_lanes(x, u, x0, tau_max=12.0)
    x[1, 100, 2] = np.nan
    res = tt.MPC_tracking_lanes(x, u, x0, tau_max=12.0)
    for f in OUT:
        for b in (0, 2):
            assert torch.equal(getattr(res, f)[b], getattr(clean, f)[b]), (f, b)
    first = 100 - (tt.T_PRED - 2)                                          # the first window that holds stage 100
    assert torch.equal(res.x[1, :, :first + 1], clean.x[1, :, :first + 1])
    assert bool(torch.isnan(res.x[1, :, first + 1:]).any(-1).all()) and bool(torch.isnan(res.err_max[1]).all())
    _check_counts(res)


def test_bad_arguments(lanes):
    from gymnast_optimalcontrol_amd import _lib
    tt = _tt()
    eng = tt._eng()
    lib = eng.lib
    B, P, N, L = 2, 3, 34, 12
    x = eng.t(lanes["x"][:B, :N]); u = eng.t(lanes["u"][:B, :N - 1]); x0 = eng.t(lanes["x0"][:B])
    nb = eng.mpc_box_lanes_workspace(B, P, L)
    ws = torch.empty(nb, dtype=torch.uint8, device=eng.device)
    xo = torch.empty((B, P, N, 4), dtype=torch.float64, device=eng.device)
    uo = torch.empty((B, P, N - 1, 2), dtype=torch.float64, device=eng.device)
    sm = torch.empty((3, B, P), dtype=torch.float64, device=eng.device)
    it = torch.empty((B, P, N - 1), dtype=torch.int32, device=eng.device)
    un = torch.empty((B, P), dtype=torch.int32, device=eng.device)
    Q, R = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_MPC, tt.R_MPC))
    QT = tt.mpc_gains(lanes["x"][0], lanes["u"][0])[1]
    m = C.byref(eng.model)

    def call(m=m, x=x.data_ptr(), u=u.data_ptr(), x0=x0.data_ptr(), B=B, P=P, N=N, L=L, Q=Q, R=R, QT=QT.data_ptr(),
             tau=18.0, cap=32, ws=ws.data_ptr(), nb=nb, xo=xo.data_ptr(), uo=uo.data_ptr(), sm=sm.data_ptr(),
             it=it.data_ptr(), un=un.data_ptr()):
        p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        return lib.gym_mpc_box_lanes_rollout(m, x, u, x0, B, P, N, L, p(Q), p(R), QT, tau, cap, ws, nb, xo, uo, sm, it,
                                             un, eng.stream)

    assert call() == 0
    torch.cuda.synchronize()
    keep = (xo.clone(), uo.clone(), sm.clone(), un.clone())
    assert call(it=None) == 0 and call(xo=None, uo=None) == 0            # the optional outputs
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (xo, uo, sm, un)))
    nonsym = Q.copy(); nonsym[0, 1] = 1.0
    offdiag = R.copy(); offdiag[1, 0] = 0.5
    r0 = R.copy(); r0[1, 1] = 0.0
    for kw in (dict(m=None), dict(x=None), dict(u=None), dict(x0=None), dict(Q=None), dict(R=None), dict(QT=None),
               dict(ws=None), dict(sm=None), dict(un=None), dict(B=0), dict(P=0), dict(N=1), dict(L=1), dict(L=255),
               dict(B=_lib.MAX_BP // 2), dict(tau=0.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(cap=0),
               dict(R=offdiag), dict(R=r0), dict(Q=nonsym), dict(xo=None), dict(uo=None), dict(nb=nb - 1)):
        assert call(**kw) == 1, list(kw)
    torch.cuda.synchronize()
    xs, us, x0s = lanes["x"][:B, :N], lanes["u"][:B, :N - 1], lanes["x0"][:B]
    for kw, frag in ((dict(tau_max=0.0), "tau_max"), (dict(tau_max=float("nan")), "tau_max"),
                     (dict(tau_max=18.0, max_qp_iters=0), "max_qp_iters"), (dict(tau_max=18.0, T_pred=1), "T_pred"),
                     (dict(tau_max=18.0, T_pred=255), "T_pred"), (dict(tau_max=18.0, R=offdiag), "diagonal R"),
                     (dict(tau_max=18.0, Q=nonsym), "symmetric")):
        with pytest.raises(ValueError, match=frag):
            tt.MPC_tracking_lanes(xs, us, x0s, **kw)
    with pytest.raises(ValueError, match=r"\(1, 3, 4\)"):
        tt.MPC_tracking_lanes(xs, us, x0s[:1], tau_max=18.0)
    with pytest.raises(TypeError, match="tau"):
        tt.MPC_tracking_lanes(xs, us, x0s, tau=18.0)


def test_end_to_end_from_a_batched_solve(task2_refs):
    """newton_Algorithm_batch on 3 starts (task-2 settings), then result.track_mpc(dx0=..., tau_max=18): every lane's
    closed loop stays inside the limit the unlimited controller exceeds, and agrees with the shared-reference path
    (solve_mpc_tracking_box_batch, itself held to the NumPy reference by tests/test_gpu_mpc_box.py) run on that lane's
    result alone, wherever that run settles every QP."""
    from gymnast_optimalcontrol_amd import trajectory_generation as tg
    tt = _tt()
    x_ref, u_ref, _ = task2_refs
    rng = np.random.default_rng(5)
    x0 = np.zeros((3, 4))
    x0[:, :2] = rng.uniform(-0.5, 0.5, (3, 2))
    sol = tg.newton_Algorithm_batch(x0, x_ref, u_ref, max_iters=5000, tol=1e-4, gamma_0=0.1)
    dx = 0.02 * np.ones(4)
    res = sol.track_mpc(dx0=dx, tau_max=18)
    assert isinstance(res, tt.MpcBoxLanesResult)
    assert res.x.shape == (3, 501, 4) and res.unconverged.shape == (3,) and res.qp_iters.shape == (3, 500)
    assert bool((res.u.abs() <= 18.0).all()) and bool(torch.equal(res.u_max, res.u[..., 1].abs().amax(-1)))
    free = sol.track_mpc(dx0=dx, trajectories=False)
    assert torch.equal(res.K, free.K)
    compared = 0
    for b in range(3):
        sh = tt.solve_mpc_tracking_box_batch((sol.x[b, 0] + torch.as_tensor(dx, device=sol.x.device))[None], sol.x[b],
                                             sol.u[b], 18.0)
        if int(sh.unconverged[0]):
            continue
        compared += 1
        ex, eu = rel_l2(_np(res.x[b]), _np(sh.x[0])), rel_l2(_np(res.u[b]), _np(sh.u[0]))
        print(f"lane {b}: rel-L2 x {ex:.2e} u {eu:.2e}, free u_max {float(free.u_max[b]):.2f}")
        assert ex < TOL and eu < TOL, (b, ex, eu)
        assert int(res.unconverged[b]) == 0
    assert compared >= 2
    both = sol.track_mpc(x0=sol.x[:, 0][:, None] + torch.as_tensor(dx, device=sol.x.device), tau_max=18)
    assert torch.equal(both.x[:, 0], res.x) and torch.equal(both.unconverged[:, 0], res.unconverged)
