"""Warm start and checkpoint / resume of the batched Newton solver (gym_newton_init_warm, BatchedNewtonSolver.init /
solve with u_init, SolveResult.save_npz, load_checkpoint, BatchedNewtonSolver.resume), through the C-ABI.

The yardstick is the uninterrupted solve: a lane's bits do not depend on the schedule, its position or the launch it
runs in, and the warm rollout is the Armijo trial's own arithmetic, so a solve split at iteration k, written to a
file, read back and resumed on a new solver must equal the uninterrupted one bit for bit.

The lanes (T = 500, the committed task-2 references, tol 1e-4, gamma_0 0.1) were chosen on the CPU with
oracle/c_oracle.newton_solve: of the 70 lanes, in 400 iterations 53 converge (the first after 364), 9 fail the line
search (lane 9 at iteration 92, lane 46 at iteration index 380, the others between 377 and 398 after one to four
backtracking iterations that accept) and 8 are cut off; the splits 380 / 381 leave converged, failed, backtracking
and plainly active lanes on both sides.  The tests assert those preconditions on the GPU's own uninterrupted run.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

B, M = 70, 400
KW = dict(tol=1e-4, beta=0.7, c=0.5, gamma_0=0.1, max_ls=20)
SCHEDULES = {"serial": dict(pipeline=False), "pipelined": dict(pipeline=True), "persistent": dict(persistent=True)}
TOL_TRAJ = 1e-8        # the project's north-star bar for converged trajectories (tests/test_gpu_parity.py)


def _lanes():
    """A few starts near the golden lane (x0 = 0), the rest wide (theta0 ~ U(+-1.5), every ninth with initial
    velocities: the stress distribution of test_gpu_stress.py / test_gpu_tail.py)."""
    rng = np.random.default_rng(5)
    x0 = np.zeros((B, 4))
    x0[:, :2] = rng.uniform(-1.5, 1.5, (B, 2))
    x0[::9, 2:] = rng.uniform(-2.0, 2.0, (len(x0[::9]), 2))
    x0[1:8, :2] = rng.uniform(-0.05, 0.05, (7, 2))
    x0[0] = 0.0
    return x0


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.is_floating_point() else t


def _same(a, b, what):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(_bits(a), _bits(b)):
        bad = (_bits(a) != _bits(b)).reshape(a.shape[0], -1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: lanes {bad[:10]} differ")


class _Ctx:
    """The engine, the references, the lanes and the solves the tests share (each computed once, left unchanged)."""

    def __init__(self, task2_refs, tmp):
        from gymnast_optimalcontrol_amd.engine import AcrobotEngine
        self.eng = AcrobotEngine()
        self.xr, self.ur, _ = task2_refs
        self.x0 = _lanes()
        self.tmp = tmp
        self._whole, self._ckpt = {}, {}

    def solver(self, schedule="serial", lanes=B, **kw):
        from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
        return BatchedNewtonSolver(self.eng, self.xr, self.ur, lanes, **SCHEDULES[schedule], **KW, **kw)

    def whole(self, schedule):
        """M iterations uninterrupted: the parent's path."""
        if schedule not in self._whole:
            s = self.solver(schedule)
            assert s.schedule == schedule and s.reorder and s.Bp == 128
            self._whole[schedule] = s.solve(self.x0, M)
        return self._whole[schedule]

    def ckpt(self, schedule, k):
        """k iterations, written with save_npz and read back with load_checkpoint."""
        from gymnast_optimalcontrol_amd.solver import load_checkpoint
        if (schedule, k) not in self._ckpt:
            path = self.tmp / f"ckpt_{schedule}_{k}.npz"
            self.solver(schedule).solve(self.x0, k).save_npz(path)
            self._ckpt[schedule, k] = load_checkpoint(path, self.eng.device)
        return self._ckpt[schedule, k]


@pytest.fixture(scope="module")
def ctx(task2_refs, tmp_path_factory):
    return _Ctx(task2_refs, tmp_path_factory.mktemp("warm"))


@pytest.mark.parametrize("k", [380, 381])        # even and odd: the iterate saved from either buffer
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_split_and_resumed_equals_whole_bit_for_bit(ctx, schedule, k):
    from gymnast_optimalcontrol_amd import _lib
    whole = ctx.whole(schedule)
    ck = ctx.ckpt(schedule, k)
    st, cst = whole.status, ck.status
    # the preconditions (module docstring), on the GPU's own runs
    assert bool(((cst == _lib.CONVERGED) & (ck.n_iter <= k)).any()), "no lane converged before the split"
    open_ = cst == _lib.MAX_ITERS                                    # interrupted at k
    more_it, more_roll = whole.n_iter - ck.n_iter, whole.n_rollouts - ck.n_rollouts
    assert bool((open_ & (more_roll > more_it)).any()), "no lane backtracks after the split"
    # ... and accepts a shortened step: more extra rollouts than a final failed search's max_ls - 1 alone
    extra = more_roll - more_it - (KW["max_ls"] - 1) * (st == _lib.LS_FAILED).to(more_it.dtype)
    assert bool((open_ & (extra > 0)).any()), "no lane accepts a backtracked step after the split"
    assert bool((st == _lib.LS_FAILED).any()) and bool(((st == _lib.LS_FAILED) & open_).any())
    assert bool((cst == _lib.LS_FAILED).any()), "no lane had failed before the split"
    assert bool((st == _lib.MAX_ITERS).any()), "no lane still active at M"
    assert int(ck.n_iter.max()) == k and int(whole.n_iter.max()) == M
    s = ctx.solver(schedule)
    res = s.resume(ck, M - k)
    for f in ("x", "u", "cost", "status", "n_iter", "gamma", "n_rollouts"):
        _same(getattr(res, f), getattr(whole, f), f"{schedule}, k={k}: {f}")
    again = open_ & (more_it > 0)                                    # lanes that iterated after k
    assert int(again.sum()) >= 40
    _same(res.K[again], whole.K[again], f"{schedule}, k={k}: K")
    _same(res.sigma[again], whole.sigma[again], f"{schedule}, k={k}: sigma")
    # finished lanes carry the checkpoint's own K and sigma (the device ran no sweep for them)
    _same(res.K[~open_], ck.K[~open_], "K of finished lanes")
    _same(res.sigma[~open_], ck.sigma[~open_], "sigma of finished lanes")
    # the segment's own counts
    assert res.lane_iterations == int(more_it.sum()) and res.iterations == M - k


@pytest.mark.parametrize("reorder", [True, False])
def test_warm_rollout_is_the_trials_rollout(ctx, reorder):
    """After the warm init and before any iteration, the states and the cost are the checkpoint's, bit for bit: the
    rollout of controls that Armijo trials produced is those trials' rollout.  Morton order on (through solve() with
    no iteration: the lane map on the input side) and off (init() and the raw buffers)."""
    ck = ctx.ckpt("serial", 380)
    s = ctx.solver("serial", reorder=reorder)
    assert s.u0_zero
    if reorder:
        r = s.solve(ck.x[:, 0], 0, u_init=ck.u, status_init=ck.status)
        assert s.lane_order is not None and not np.array_equal(s.lane_order.cpu().numpy(), np.arange(B))
        x, u, cost = r.x, r.u, r.cost
        _same(r.status, ck.status, "status")
        assert int(r.n_iter.abs().sum()) == 0 and r.iterations == 0
    else:
        s.init(ck.x[:, 0], u_init=ck.u)
        x, u, cost = ctx.eng.unpack(s.states(0), B), s.controls(0), s.cost[:B]
        assert int(s.status[:B].abs().sum()) == 0                  # no status_init: every lane ACTIVE
    _same(x, ck.x, "x")
    _same(u, ck.u, "u")
    _same(cost, ck.cost, "cost")


def test_lane_map_on_the_input_side(ctx):
    """gym_newton_init_warm with a permutation in gym_batch.lane_map: internal lane i takes row lane_map[i] of x0,
    u_init and status_init, so the device state equals the identity-map call on the pre-permuted inputs; padding
    lanes are GYM_PAD with zero controls."""
    import ctypes as C
    import torch
    from gymnast_optimalcontrol_amd import _lib
    eng = ctx.eng
    dev = eng.device
    s = ctx.solver("serial", u0_zero=False)
    T, Bp = s.T, s.Bp
    g = torch.Generator().manual_seed(3)
    u = (0.3 * torch.randn(B, T, 2, dtype=torch.float64, generator=g)).to(dev)     # both tau planes live
    x0 = (0.2 * torch.randn(B, 4, dtype=torch.float64, generator=g)).to(dev)
    st = torch.tensor([_lib.ACTIVE, _lib.CONVERGED, _lib.LS_FAILED, _lib.MAX_ITERS, _lib.PAD, 77, -5] * 10,
                      dtype=torch.int32, device=dev)
    perm = torch.randperm(B, generator=g).to(dev)
    assert not torch.equal(perm, torch.arange(B, device=dev))

    def warm(x0_, u_, st_, lane_map):
        for t in (*s.x, *s.u):
            t.fill_(7.0)                                           # stale contents, also in the padding lanes
        s.x[0].zero_()
        s.batch.lane_map = None if lane_map is None else lane_map.data_ptr()
        try:
            _lib.check(eng.lib.gym_newton_init_warm(C.byref(eng.model), C.byref(eng._w), x0_.data_ptr(),
                                                    u_.data_ptr(), st_.data_ptr(), C.byref(s.batch), eng.stream),
                       "gym_newton_init_warm")
        finally:
            s.batch.lane_map = None
        torch.cuda.synchronize(dev)
        return dict(x=s.x[0].clone(), u=s.u[0].clone(), status=s.status.clone(), cost=s.cost.clone(),
                    n_iter=s.n_iter.clone(), res_buf=s.res_buf.clone(), n_roll=s.n_roll.clone())

    a = warm(x0, u, st, perm)
    xa = torch.empty((B, s.N, 4), dtype=torch.float64, device=dev)
    ua = torch.empty((B, T, 2), dtype=torch.float64, device=dev)
    s.batch.lane_map = perm.data_ptr()                              # the same map on the output side
    try:
        _lib.check(eng.lib.gym_newton_finalize(C.byref(eng.model), C.byref(eng._w), C.byref(s.batch), 0,
                                               xa.data_ptr(), ua.data_ptr(), None, None, eng.stream),
                   "gym_newton_finalize")
    finally:
        s.batch.lane_map = None
    torch.cuda.synchronize(dev)
    b = warm(x0[perm].contiguous(), u[perm].contiguous(), st[perm].contiguous(), None)
    for f in a:
        _same(a[f], b[f], f)
    _same(eng.unpack(a["u"], B), u[perm], "u[0] in internal lane order")
    _same(ua, u, "u unpacked with the same map")
    _same(xa[:, 0], x0, "x_0 unpacked with the same map")
    want = st[perm].clone()
    want[(want != _lib.CONVERGED) & (want != _lib.LS_FAILED)] = _lib.ACTIVE
    assert torch.equal(a["status"][:B], want)
    assert bool((a["status"][B:] == _lib.PAD).all()) and Bp - B == 58
    assert not bool(a["u"].view(T, 2, Bp)[:, :, B:].any()), "padding lanes' controls are not zero"
    assert not bool(a["n_iter"].any()) and not bool(a["res_buf"].any()) and not bool(a["n_roll"].any())


def test_warm_start_with_live_tau1_clears_the_u0_zero_flag(ctx):
    """A solver that skips the tau1 planes (u_ref[:, 0] == 0) warm-started with tau1 != 0 runs that solve on the
    general kernels: x / J_0 after init are the NumPy oracle's open-loop rollout and cost, u after one iteration is
    the oracle's stage_lists -> riccati -> closed_loop at the accepted step (the Gauss-Newton blocks take no
    costate: S = 0), and the flag is back afterwards.  Tolerances: those of tests/test_gpu_parity.py for the same
    quantities (open-loop rollout 1e-12, cost rtol 1e-11, closed-loop update 1e-10)."""
    from gymnast_optimalcontrol_amd import _lib
    from oracle import acrobot_np as onp
    n = 5
    rng = np.random.default_rng(11)
    x0 = np.zeros((n, 4))
    x0[:, :2] = rng.uniform(-0.05, 0.05, (n, 2))
    t = np.arange(ctx.ur.shape[0])
    u = np.zeros((n,) + ctx.ur.shape)
    u[:, :, 1] = 0.05 * ctx.ur[:, 1] * rng.uniform(0.5, 1.0, (n, 1))
    u[:, :, 0] = 1e-3 * np.sin(0.05 * t)[None] * rng.uniform(0.5, 1.0, (n, 1))      # the small tau1 plane
    s = ctx.solver("serial", lanes=n)
    assert s.u0_zero and s.batch.flags & _lib.FLAG_U0_ZERO
    r0 = s.solve(x0, 0, u_init=u)
    assert s.u0_zero and s.batch.flags & _lib.FLAG_U0_ZERO, "the flag was not restored"
    x_np = onp.simulate_open_loop(x0, u)
    J_np = onp.total_cost(x_np, u, ctx.xr, ctx.ur)
    print("init: rel_l2(x)", rel_l2(r0.x.cpu().numpy(), x_np), "max rel cost err",
          np.max(np.abs(r0.cost.cpu().numpy() - J_np) / np.abs(J_np)))
    assert np.array_equal(r0.u.cpu().numpy(), u)
    assert rel_l2(r0.x.cpu().numpy(), x_np) < 1e-12
    np.testing.assert_allclose(r0.cost.cpu().numpy(), J_np, rtol=1e-11)
    r1 = s.solve(x0, 1, u_init=u)
    assert s.u0_zero and s.batch.flags & _lib.FLAG_U0_ZERO, "the flag was not restored"
    assert r1.n_iter.tolist() == [1] * n and not bool((r1.status == _lib.LS_FAILED).any())
    gam = r1.gamma.cpu().numpy()
    A_d, B_d, q, rr, QTb, qT = onp.stage_lists(x_np, u, ctx.xr, ctx.ur)
    K, sig, _ = onp.riccati(A_d, B_d, 2 * onp.Q_DEFAULT, 2 * onp.R_DEFAULT, np.zeros((2, 4)), q, rr, QTb, qT)
    xn, un = onp.closed_loop(x_np, u, K, sig, gam)
    got_u = r1.u.cpu().numpy()
    print("iteration 1: gamma", gam, "rel_l2(u)", rel_l2(got_u, un), "rel_l2(u tau1)", rel_l2(got_u[..., 0], un[..., 0]),
          "rel_l2(x)", rel_l2(r1.x.cpu().numpy(), xn))
    assert np.abs(un[..., 0] - u[..., 0]).max() > 0 and np.abs(got_u[..., 0]).max() > 0     # the tau1 channel moved
    assert rel_l2(got_u, un) < 1e-10
    assert rel_l2(got_u[..., 0], un[..., 0]) < 1e-10
    assert rel_l2(r1.x.cpu().numpy(), xn) < 1e-10
    # and a cold solve on the same solver afterwards is the flag's path again, bit for bit a fresh solver's
    cold = s.solve(x0, 3)
    fresh = ctx.solver("serial", lanes=n).solve(x0, 3)
    _same(cold.x, fresh.x, "cold solve after a warm one: x")
    _same(cold.u, fresh.u, "cold solve after a warm one: u")


def test_task2_resumed_lands_on_the_references_file(ctx, tmp_path):
    """The task-2 lane (main.py:65-71: x0 = 0, tol 1e-4, gamma_0 0.1) interrupted after 200 iterations, saved, loaded
    and resumed: the reference's acrobot_optimal_trajectory.npz within 1e-8, the uninterrupted GPU solve bit for
    bit, the same total iteration count.  And the reference's own file, loaded as a checkpoint, converges again in
    no more iterations than the cold solve took."""
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver, load_checkpoint
    ref_path = os.path.join(GOLDEN, "task2_reference_output.npz")
    ref = np.load(ref_path)
    kw = dict(tol=1e-4, gamma_0=0.1)
    x0 = np.zeros((1, 4))
    new = lambda: BatchedNewtonSolver(ctx.eng, ctx.xr, ctx.ur, 1, **kw)   # noqa: E731
    whole = new().solve(x0, 5000)
    assert whole.status.tolist() == [_lib.CONVERGED] and whole.n_iter.tolist() == [393]
    path = tmp_path / "task2_200.npz"
    new().solve(x0, 200).save_npz(path)
    ck = load_checkpoint(path, ctx.eng.device)
    assert ck.n_iter.tolist() == [200] and ck.status.tolist() == [_lib.MAX_ITERS]
    res = new().resume(ck, 5000)
    assert res.status.tolist() == [_lib.CONVERGED]
    assert rel_l2(res.x[0].cpu().numpy(), ref["x"]) < TOL_TRAJ
    assert rel_l2(res.u[0].cpu().numpy(), ref["u"]) < TOL_TRAJ
    for f in ("x", "u", "cost", "status", "n_iter", "gamma", "n_rollouts", "K", "sigma"):
        _same(getattr(res, f), getattr(whole, f), f)
    assert res.n_iter.tolist() == whole.n_iter.tolist() and res.iterations == 193
    # the reference's own file as a checkpoint
    again = new().resume(load_checkpoint(ref_path, ctx.eng.device), 5000)
    print("resumed from the reference's file: iterations", again.n_iter.tolist(), "status", again.status.tolist())
    assert again.status.tolist() == [_lib.CONVERGED]
    assert 1 <= int(again.n_iter[0]) <= int(whole.n_iter[0])      # observed: 1


def test_status_init_freezes_finished_lanes(ctx):
    """A lane handed over as CONVERGED never changes: no iteration in the segment, its x / u / cost untouched after
    five more iterations; lanes handed over as MAX_ITERS -- or with a value outside the status codes -- iterate."""
    import torch
    from gymnast_optimalcontrol_amd import _lib
    ck = ctx.ckpt("serial", 380)
    whole = ctx.whole("serial")
    live = ((ck.status == _lib.MAX_ITERS) & (whole.status == _lib.MAX_ITERS)).nonzero().flatten().tolist()
    assert len(live) >= 3                                           # still active at M: they run all five iterations
    frozen, cut, odd = live[:3]
    st = ck.status.clone()
    st[frozen] = _lib.CONVERGED
    st[odd] = 9
    assert int(st[cut]) == _lib.MAX_ITERS
    s = ctx.solver("serial")
    r = s.solve(ck.x[:, 0], 5, u_init=ck.u, status_init=st)
    assert int(r.n_iter[frozen]) == 0 and int(r.status[frozen]) == _lib.CONVERGED and int(r.n_rollouts[frozen]) == 0
    for f in ("x", "u", "cost"):
        _same(getattr(r, f)[frozen], getattr(ck, f)[frozen], f"frozen lane: {f}")
    assert int(r.n_iter[cut]) == 5 and int(r.n_iter[odd]) == 5
    assert int(r.status[cut]) == int(r.status[odd]) == _lib.MAX_ITERS
    assert not torch.equal(r.u[cut], ck.u[cut]) and float(r.cost[cut]) < float(ck.cost[cut])
    # lanes the checkpoint had finished did not move either
    done = (ck.status == _lib.CONVERGED) | (ck.status == _lib.LS_FAILED)
    assert bool(done.any()) and int(r.n_iter[done].abs().sum()) == 0
    _same(r.x[done], ck.x[done], "finished lanes: x")
    _same(r.status[done], ck.status[done], "finished lanes: status")
    # wrong shapes and dtypes are refused before anything is launched
    with pytest.raises(ValueError):
        s.solve(ck.x[:, 0], 1, u_init=ck.u[:, :-1])
    with pytest.raises(ValueError):
        s.solve(ck.x[:, 0], 1, u_init=ck.u.to(torch.float32))
    with pytest.raises(ValueError):
        s.solve(ck.x[:, 0], 1, u_init=ck.u, status_init=st[:-1])
    with pytest.raises(ValueError):
        s.solve(ck.x[:, 0], 1, u_init=ck.u, status_init=st.to(torch.float64))
    with pytest.raises(ValueError):
        s.solve(ck.x[:, 0], 1, status_init=st)
