"""Per-lane trackers on a mismatched plant (``plant=``; gym_lqr_lanes_rollout_plant, gym_mpc_box_lanes_rollout_plant).

Expectation: tests/plant_ref.py, the per-lane trackers' own yardsticks with the plant step of closed loop (b, p) on
that loop's own parameter set (anchored to them by tests/test_plant_host.py).  Inputs: the 12 lanes of
tests/golden/lanes.npz and their prefixes.  The plant of (b, p) is plant_ref.KEYS[(b + p) % 4] and its start
mpc_box_lanes_ref.starts(x)[b][p % 3], so neither index can be swapped or transposed unnoticed.

Bars, the project's own (tests/test_gpu_lqr_lanes.py, tests/test_gpu_mpc_box_lanes.py): rel-L2 < 1e-9 per (lane,
start) on x and u; qp_iters only within [1, cap].  Measured on the CPU with the oracle alone, a relative perturbation
of 1e-13 of all inputs moves the mismatched reference by at most 2.2e-13 in x and 6.2e-13 in u on the LQR prefixes,
2.1e-12 and 1.5e-11 at full length on the heavy plant, 2.5e-12 and 1.1e-11 for the unlimited MPC at N 22, 3.6e-12 and
1.0e-11 on the box cases: about two decades under the bar everywhere.

The two properties of DESIGN 4.8 are bit-for-bit tests: identity (a plant equal to the design model is the call without
``plant``) and independence (a closed loop's result depends on its lane, its start and its plant only)."""
import ctypes as C

import numpy as np
import pytest
import torch

import plant_ref as pr
from conftest import load_golden
from plant_ref import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-9
CAP = 32
SUMS = ("err_final", "err_max", "u_max")
LQR = ("x", "u", "K") + SUMS
MPC = LQR + ("QT",)
BOX = MPC + ("qp_iters", "unconverged")
SET1 = pr.params_of([[1]])[0, 0]


def _np(t):
    return t.detach().cpu().numpy()


def _tt():
    from gymnast_optimalcontrol_amd import trajectory_tracking as tt
    return tt


def _equal(a, b, fields):
    for f in fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def _tau(u):
    """test_small_shapes' limit: 0.8 of the lane's own peak torque, so that it binds early."""
    return round(0.8 * float(np.abs(u[0, :, 1]).max()), 3)


@pytest.fixture(scope="module")
def lanes():
    g = load_golden("lanes")
    return g["x"], g["u"]


def _check_traj(res, ref, where=""):
    """x, u of a result with (B,P,...) shapes against the reference's, per (lane, start), at the bar."""
    x, u = _np(res.x), _np(res.u)
    assert x.shape == ref["x"].shape and u.shape == ref["u"].shape
    assert np.isfinite(ref["x"]).all() and np.isfinite(ref["u"]).all(), "a wrong case: the reference is not finite"
    worst = [0.0, 0.0]
    for b in range(x.shape[0]):
        for p in range(x.shape[1]):
            ex, eu = rel_l2(x[b, p], ref["x"][b, p]), rel_l2(u[b, p], ref["u"][b, p])
            worst = [max(worst[0], ex), max(worst[1], eu)]
            assert ex < TOL and eu < TOL, (where, b, p, ex, eu)
    print(f"{where}: worst rel-L2 x {worst[0]:.2e} u {worst[1]:.2e}")


def _check_summaries(res, ref, x_opt):
    """The summaries are torch's maxima of the returned x, u exactly, and the oracle's within the trajectory bar (a
    maximum of absolute values is 1-Lipschitz in the sup norm, which the 2-norm bounds)."""
    e = (res.x - torch.as_tensor(x_opt, device=res.x.device)[:, None]).abs()
    assert torch.equal(res.err_final, e[:, :, -1].amax(-1)) and torch.equal(res.err_max, e.amax((-1, -2)))
    assert torch.equal(res.u_max, res.u[..., 1].abs().amax(-1))
    nx, nu = np.linalg.norm(ref["x"], axis=(-1, -2)), np.linalg.norm(ref["u"], axis=(-1, -2))
    for name, bound in (("err_final", nx), ("err_max", nx), ("u_max", nu)):
        assert (np.abs(_np(getattr(res, name)) - ref[name]) <= TOL * bound).all(), name


# ------------------------------------------------------------------------------------------------ 1. identity
def _forms(B, P):
    return {"set": 1, "dict": {}, "row": SET1, "table": np.broadcast_to(SET1, (B, P, 11)).copy()}


@pytest.mark.parametrize("loop", ["lqr", "mpc", "box", "box_fallback"])
def test_a_plant_equal_to_the_design_model_is_the_call_without_one(lanes, loop):
    tt = _tt()
    x, u = lanes[0][:, :66], lanes[1][:, :65]
    if loop in ("box", "box_fallback"):
        x, u = x[:1], u[:1]
    x0 = pr.starts(x, 3)
    lim = {"box": 10.502, "box_fallback": tt.TorqueLimit(10.502)}.get(loop)
    call = {"lqr": lambda **kw: tt.LQR_tracking_lanes(x, u, x0, **kw),
            "mpc": lambda **kw: tt.MPC_tracking_lanes(x, u, x0, T_pred=12, **kw)}.get(
                loop, lambda **kw: tt.MPC_tracking_lanes(x, u, x0, T_pred=12, tau_max=lim, **kw))
    fields = {"lqr": LQR, "mpc": MPC}.get(loop, BOX)
    base = call()
    if lim is not None:
        assert bool((base.u[..., 1].abs() == 10.502).any()) and int(base.unconverged.max()) == 0
    for name, form in _forms(*x0.shape[:2]).items():
        res = call(plant=form)
        assert type(res) is type(base), name
        _equal(res, base, fields)
    lean = call(plant=1, trajectories=False, gains=False)
    assert lean.x is None and lean.K is None
    _equal(lean, base, SUMS)


def test_identity_at_full_length(lanes):
    tt = _tt()
    x, u = lanes
    x0 = pr.starts(x, 3)
    _equal(tt.LQR_tracking_lanes(x, u, x0, plant=np.broadcast_to(SET1, (12, 3, 11))), tt.LQR_tracking_lanes(x, u, x0),
           LQR)


# ------------------------------------------------------------------------------------- 2. LQR parity with the oracle
@pytest.fixture(scope="module")
def lqr_refs(lanes):
    """65 lanes (the 12 tiled: a ragged second group) x 4 starts on the prefixes of 22 and 66 knots: T = 21 is two
    full 8-step LDS stagings plus one of 5, T = 65 eight plus one.  One reference per N; B = 1 and P = 1 are slices."""
    idx = np.arange(65) % 12
    out = {}
    for n in (22, 66):
        x, u = lanes[0][idx, :n], lanes[1][idx, :n - 1]
        x0, keys = pr.starts(x, 4), pr.keys_of(65, 4)
        out[n] = (x, u, x0, pr.params_of(keys), pr.lqr_ref(x, u, x0, keys))
    return out


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("n", [22, 66])
def test_lqr_parity(lqr_refs, n, B, P):
    x, u, x0, par, full = lqr_refs[n]
    x, u, x0, par = x[:B], u[:B], x0[:B, :P], par[:B, :P]
    ref = {k: v[:B] if k == "K" else v[:B, :P] for k, v in full.items()}
    res = _tt().LQR_tracking_lanes(x, u, x0, plant=par)
    _check_traj(res, ref, f"LQR N {n} B {B} P {P}")
    K = _np(res.K)
    for b in range(B):
        assert np.abs(K[b] - ref["K"][b]).max() <= TOL * np.abs(ref["K"][b]).max(), b
    _check_summaries(res, ref, x)
    assert res.err_max.shape == (B, P)
    if P == 1:                                           # x0 (B,4): P is 1 and (B,11) is the per-lane form
        flat = _tt().LQR_tracking_lanes(x, u, x0[:, 0], plant=par[:, 0])
        assert flat.x.shape == (B, n, 4) and torch.equal(flat.x, res.x[:, 0]) and torch.equal(flat.u, res.u[:, 0])


def test_lqr_parity_at_full_length(lanes):
    """N 501, every lane but 9, its three starts; the plants alternate heavy and set 1 (sticky and set 2 overflow at
    full length in the reference itself)."""
    keep = [b for b in range(12) if b != 9]
    x, u = lanes[0][keep], lanes[1][keep]
    x0 = pr.starts(x, 3)
    keys = [[("heavy", 1)[(b + p) % 2] for p in range(3)] for b in range(11)]
    ref = pr.lqr_ref(x, u, x0, keys)
    res = _tt().LQR_tracking_lanes(x, u, x0, plant=pr.params_of(keys))
    _check_traj(res, ref, "LQR N 501 heavy / set 1")
    _check_summaries(res, ref, x)


# --------------------------------------------------------------------------------------- 3. unlimited MPC parity
def test_mpc_parity_short(lanes):
    x, u = lanes[0][:, :22], lanes[1][:, :21]
    x0, keys = pr.starts(x, 4), pr.keys_of(12, 4)
    ref = pr.mpc_ref(x, u, x0, keys, T_pred=20)
    res = _tt().MPC_tracking_lanes(x, u, x0, T_pred=20, plant=pr.params_of(keys))
    assert type(res) is _tt().MpcLanesResult
    _check_traj(res, ref, "MPC N 22 T_pred 20")
    _check_summaries(res, ref, x)


def test_mpc_parity_at_full_length(lanes):
    """N 501, T_pred 75, lanes 0 and 10 (two lanes only: the host-side oracle stays within seconds), plant heavy from
    all three starts."""
    x, u = lanes[0][[0, 10]], lanes[1][[0, 10]]
    x0, keys = pr.starts(x, 3), [["heavy"] * 3] * 2
    ref = pr.mpc_ref(x, u, x0, keys)
    res = _tt().MPC_tracking_lanes(x, u, x0, plant={"m2": 1.1, "I2": 0.363})
    _check_traj(res, ref, "MPC N 501 T_pred 75 heavy")
    _check_summaries(res, ref, x)


# --------------------------------------------------------------------------------------------------- 4. box parity
BOX_CASES = [(0, 34, 12), (10, 34, 3), (0, 66, 12), (9, 34, 12), (0, 34, 2)]


@pytest.mark.parametrize("case", BOX_CASES, ids=["lane%d-N%d-T%d" % c for c in BOX_CASES])
def test_box_parity(lanes, case):
    """B 1, P 12; the first case at B 3, P 65 (a second start block holding one thread)."""
    tt = _tt()
    lane, n, Tp = case
    B, P = (3, 65) if case == BOX_CASES[0] else (1, 12)
    x, u = np.repeat(lanes[0][[lane], :n], B, 0), np.repeat(lanes[1][[lane], :n - 1], B, 0)
    tau = _tau(u)
    x0, keys = pr.starts(x, P), pr.keys_of(B, P)
    ref = pr.box_ref(x, u, x0, keys, tau, Tp, CAP)
    assert np.isfinite(ref["x"]).all() and not ref["unconverged"].any(), "a wrong case"
    assert (np.abs(ref["u"][..., 1]) == tau).any() and ref["qp_iters"].min() >= 1
    par = pr.params_of(keys)
    res = tt.MPC_tracking_lanes(x, u, x0, T_pred=Tp, tau_max=tau, plant=par)
    assert type(res) is tt.MpcBoxLanesResult
    _check_traj(res, ref, f"box lane {lane} N {n} T_pred {Tp} B {B} P {P} tau {tau}")
    us = _np(res.u)
    assert int(res.unconverged.max()) == 0 and np.abs(us).max() <= tau and (np.abs(us[..., 1]) == tau).any()
    it = res.qp_iters
    assert it.dtype == torch.int32 and int(it.min()) >= 1 and int(it.max()) <= CAP
    e = (res.x - torch.as_tensor(x, device=res.x.device)[:, None]).abs()
    assert torch.equal(res.err_final, e[:, :, -1].amax(-1)) and torch.equal(res.err_max, e.amax((-1, -2)))
    assert torch.equal(res.u_max, res.u[..., 1].abs().amax(-1))
    fb = tt.MPC_tracking_lanes(x, u, x0, T_pred=Tp, tau_max=tt.TorqueLimit(tau), plant=par)
    _equal(fb, res, BOX)                                 # every QP settles: the fallback never runs


# -------------------------------------------------------------------------------------------------- 5. independence
def test_a_closed_loop_depends_on_its_lane_its_start_and_its_plant_only(lanes):
    tt = _tt()
    idx = np.arange(130) % 12
    x, u = lanes[0][idx, :66].copy(), lanes[1][idx, :65].copy()
    x0 = pr.starts(x, 3)
    par = tt.sample_plants(130, 3, seed=5)
    same = [0, 63, 64, 129]                              # first / last lane of a wavefront, a ragged last group
    x[same], u[same], x0[same], par[same] = x[5], u[5], x0[5], par[5]
    tau = _tau(u[64:65])
    calls = {"lqr": (lambda xx, uu, s, **kw: tt.LQR_tracking_lanes(xx, uu, s, **kw), LQR),
             "box": (lambda xx, uu, s, **kw: tt.MPC_tracking_lanes(xx, uu, s, T_pred=12, tau_max=tau, **kw), BOX)}
    for name, (call, fields) in calls.items():
        res = call(x, u, x0, plant=par)
        assert bool(torch.isfinite(res.x).all()), name
        assert not torch.equal(res.x[0, 0], call(x[:1], u[:1], x0[:1, :1]).x[0, 0]), name     # the plants do differ
        per_lane = [f for f in fields if f != "QT"]
        for f in per_lane:
            t = getattr(res, f)
            for l in same[1:]:
                assert torch.equal(t[l], t[0]), (name, f, l)
        one = call(x[64:65], u[64:65], x0[64:65, 1:2], plant=par[64:65, 1:2])                 # B 1, P 1
        for f in per_lane:
            got, want = getattr(one, f)[0], getattr(res, f)[64]
            assert torch.equal(got if f == "K" else got[0], want if f == "K" else want[1]), (name, f)
        lean = call(x, u, x0, plant=par, trajectories=False, gains=False)
        assert lean.x is None and lean.u is None
        _equal(lean, res, SUMS + (("unconverged",) if name == "box" else ()))
    # the box path's lane chunks slice the table with the other lane-major buffers
    eng = tt._eng()
    res = calls["box"][0](x[:6], u[:6], x0[:6], plant=par[:6])
    per_lane_bytes = eng.mpc_box_lanes_workspace(1, 3, 12)
    xs, us, sm, it, un = eng.mpc_box_lanes_rollout(eng.t(x[:6]), eng.t(u[:6]), eng.t(x0[:6]), tt.Q_MPC, tt.R_MPC, res.QT,
                                                   12, tau, max_ws_bytes=2 * per_lane_bytes + 5,
                                                   plant=eng.plant_table(par[:6], 6, 3))
    assert torch.equal(xs, res.x) and torch.equal(us, res.u) and torch.equal(it, res.qp_iters)
    assert torch.equal(un, res.unconverged) and torch.equal(sm[1], res.err_max)


# ------------------------------------------------------------------------------ 6. a diverging plant stays in its loop
def test_a_diverging_plant_stays_in_its_loop(lanes):
    """LQR at full length, lanes 0-2 x 3 starts on set 1, except (1, 2) on set 2: that loop overflows (in the reference
    too).  A numerical outcome carried in the summaries, as a NaN start is; every other loop is the run without it."""
    tt = _tt()
    x, u = lanes[0][:3], lanes[1][:3]
    x0 = pr.starts(x, 3)
    keys = [[1] * 3 for _ in range(3)]
    clean = tt.LQR_tracking_lanes(x, u, x0, plant=pr.params_of(keys))
    keys[1][2] = 2
    res = tt.LQR_tracking_lanes(x, u, x0, plant=pr.params_of(keys))
    assert not bool(torch.isfinite(res.err_max[1, 2])) and not bool(torch.isfinite(res.x[1, 2]).all())
    keep = torch.ones((3, 3), dtype=torch.bool, device=res.x.device)
    keep[1, 2] = False
    for f in ("x", "u") + SUMS:
        assert torch.equal(getattr(res, f)[keep], getattr(clean, f)[keep]), f
    assert torch.equal(res.K, clean.K) and bool(torch.isfinite(clean.err_max).all())
    lean = tt.LQR_tracking_lanes(x, u, x0, plant=pr.params_of(keys), trajectories=False)
    for f in SUMS:
        assert torch.equal(getattr(lean, f)[keep], getattr(res, f)[keep]), f
    assert not bool(torch.isfinite(lean.err_max[1, 2]))


# ---------------------------------------------------------------------------------------------------- 7. end to end
def test_end_to_end_from_a_batched_solve(task2_refs):
    """newton_Algorithm_batch on 3 starts (task-2 settings), then result.track_lqr / track_mpc with ``plant=``: the
    direct *_tracking_lanes call on the result's own x, u bit for bit."""
    from gymnast_optimalcontrol_amd import trajectory_generation as tg
    tt = _tt()
    x_ref, u_ref, _ = task2_refs
    rng = np.random.default_rng(5)
    x0 = np.zeros((3, 4))
    x0[:, :2] = rng.uniform(-0.5, 0.5, (3, 2))
    sol = tg.newton_Algorithm_batch(x0, x_ref, u_ref, max_iters=5000, tol=1e-4, gamma_0=0.1)
    dx0 = rng.uniform(-0.05, 0.05, (3, 2, 4))
    par = tt.sample_plants(3, 2, seed=1)
    starts = sol.x[:, 0][:, None] + torch.as_tensor(dx0, device=sol.x.device)
    a, b = sol.track_lqr(dx0=dx0, plant=par), tt.LQR_tracking_lanes(sol.x, sol.u, starts, plant=par)
    _equal(a, b, LQR)
    assert a.err_max.shape == (3, 2) and a.x.shape == (3, 2, 501, 4)
    assert not torch.equal(a.x, sol.track_lqr(dx0=dx0).x)
    a, b = (sol.track_mpc(dx0=dx0, tau_max=18, plant=par),
            tt.MPC_tracking_lanes(sol.x, sol.u, starts, tau_max=18, plant=par))
    assert isinstance(a, tt.MpcBoxLanesResult)
    _equal(a, b, BOX)
    assert a.err_max.shape == (3, 2) and a.unconverged.shape == (3, 2) and bool((a.u.abs() <= 18.0).all())


# -------------------------------------------------------------------------------------------------- 8. bad arguments
def test_bad_arguments(lanes):
    tt = _tt()
    eng = tt._eng()
    lib = eng.lib
    B, P, N, L = 2, 3, 34, 12
    xs, us = lanes[0][:B, :N], lanes[1][:B, :N - 1]
    x0s = pr.starts(xs, P)
    x, u, x0 = eng.t(xs), eng.t(us), eng.t(x0s)
    table = eng.plant_table(1, B, P)
    assert table.shape == (B, P, 8) and table.data_ptr() % 16 == 0
    spare = torch.zeros(B * P * 8 + 2, dtype=torch.float64, device=eng.device)   # a copy 8 bytes off a 16-byte boundary
    spare[1:-1] = table.reshape(-1)
    off = spare.data_ptr() + 8
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=eng.device)   # noqa: E731
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=eng.device)       # noqa: E731
    m = C.byref(eng.model)
    # the LQR / unlimited-MPC closed loop
    ws, _ = eng.lqr_lanes_gains(x, u, tt.Q_REG, tt.R_REG, tt.QT_REG, gains=False)
    xo, uo, sm = f64(B, P, N, 4), f64(B, P, N - 1, 2), f64(3, B, P)

    def lqr(plant):
        return lib.gym_lqr_lanes_rollout_plant(m, plant, x0.data_ptr(), B, P, N, ws.data_ptr(), ws.numel(),
                                               xo.data_ptr(), uo.data_ptr(), sm.data_ptr(), eng.stream)

    assert lqr(None) == 1 and lqr(off) == 1
    torch.cuda.synchronize()
    assert bool((xo == -7.0).all()) and bool((uo == -7.0).all()) and bool((sm == -7.0).all())   # nothing was launched
    assert lqr(table.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xo).all()) and not bool((sm == -7.0).any())
    # the torque-limited closed loop, with and without the fallback
    Q, R = (np.ascontiguousarray(a, dtype=np.float64) for a in (tt.Q_MPC, tt.R_MPC))
    QT = tt.mpc_gains(lanes[0][0], lanes[1][0])[1]
    nb = eng.mpc_box_lanes_workspace(B, P, L)
    bws = torch.empty(nb, dtype=torch.uint8, device=eng.device)
    it, un = i32(B, P, N - 1), i32(B, P)
    xo.fill_(-7.0); uo.fill_(-7.0); sm.fill_(-7.0)

    def box(plant, fb=0):
        return lib.gym_mpc_box_lanes_rollout_plant(m, plant, x.data_ptr(), u.data_ptr(), x0.data_ptr(), B, P, N, L,
                                                   Q.ctypes.data, R.ctypes.data, QT.data_ptr(), 18.0, CAP, fb,
                                                   bws.data_ptr(), nb, xo.data_ptr(), uo.data_ptr(), sm.data_ptr(),
                                                   it.data_ptr(), un.data_ptr(), eng.stream)

    for fb in (0, 8):
        assert box(None, fb) == 1 and box(off, fb) == 1
    assert box(table.data_ptr(), -1) == 1
    torch.cuda.synchronize()
    assert bool((xo == -7.0).all()) and bool((it == -7).all()) and bool((un == -7).all())       # nothing was launched
    for fb in (0, 8):
        assert box(table.data_ptr(), fb) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xo).all()) and int(it.min()) >= 1 and int(un.max()) == 0
    # the Python surface: check_plant's refusals, and a set with a singular mass matrix
    for bad, words in ((dict(mass=1.0), "unknown plant parameter"), (np.zeros((B, P, 7)), "11 parameters"),
                       (np.tile(SET1, (5, 1)), "does not broadcast"), (dict(m1=np.nan), "must be finite"),
                       (9, "plant set"), (dict(m1=0.0, I1=0.0, lc1=0.0, I2=0.0), "mass matrix")):
        with pytest.raises(ValueError, match=words):
            tt.LQR_tracking_lanes(xs, us, x0s, plant=bad)
        with pytest.raises(ValueError, match=words):
            tt.MPC_tracking_lanes(xs, us, x0s, tau_max=18.0, plant=bad)
    with pytest.raises(ValueError, match="plant must be a plant_table"):
        eng.lqr_lanes_rollout(ws, x0, N, plant=table[:1])
