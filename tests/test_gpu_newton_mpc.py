"""Closed-loop replanning on the GPU: BatchedNewtonSolver.closed_loop (gym_newton_mpc_run, k_nt_mpc_run).

Yardsticks: the NumPy restatement tests/newton_mpc_ref.py through its fixture tests/golden/newton_mpc_ref.npz
(tests/test_newton_mpc_host.py recomputes it) -- per step and lane the same iterations, rollouts and stop codes, x and u
within 1e-8 rel-L2 and the cost-to-go within 1e-9 relative, DESIGN 3's bars for trajectories and cost histories; and,
bit for bit, the solver's own solve (a loop that never replans on its design model applies its plan), the same loop in
other chunks, and every lane alone against the lane in a batch, whatever its position and its neighbours.

Shapes: the short setup of tests/newton_box_ref.py (N = 41) on 70 lanes (two wavefronts, one ragged) and 130 lanes
(three), lane b on plant KEYS[b % 4]; one loop on the headline references (their first 251 knots) on 4 lanes.
"""
import time

import numpy as np
import pytest

import newton_box_ref as nb
import newton_mpc_ref as nm
from conftest import load_golden, rel_l2
from oracle import acrobot_np as onp

pytestmark = pytest.mark.gpu

TOL_TRAJ = 1e-8        # trajectories, rel-L2
TOL_COST = 1e-9        # cost histories, relative
FIELDS = ("x", "u", "iters", "rollouts", "stop", "cost", "err_final", "u_max")
PUMP = dict(onp.PARAM_SETS[1], f1=-30.0, f2=-30.0)      # tests/test_gpu_newton_models.py's diverging plant


def _same(a, b, what, la=slice(None), lb=None):
    """Every field of result a's lanes la is result b's lanes lb (default: the same), bit for bit."""
    import torch
    lb = la if lb is None else lb
    for f in FIELDS:
        va, vb = getattr(a, f)[la].contiguous(), getattr(b, f)[lb].contiguous()
        bits = lambda v: v.view(torch.uint8) if v.dtype.is_floating_point else v   # noqa: E731  (NaNs by their bits)
        assert torch.equal(bits(va), bits(vb)), f"{what}: {f} differs"


def _starts(B, seed):
    """B starts, every seventh with initial velocities (tests/test_gpu_newton_models.py's)."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 4))
    x0[:, :2] = rng.uniform(-0.5, 0.5, (B, 2))
    n = len(x0[::7])
    x0[::7, 2:] = rng.uniform(-1.0, 1.0, (n, 2))
    return x0


class _Ctx:
    def __init__(self, task2_refs):
        from gymnast_optimalcontrol_amd.engine import AcrobotEngine
        self.eng = AcrobotEngine()
        self.refs = task2_refs[:2]
        self.x0, self.xr, self.ur = nb.short_setup(task2_refs[0], task2_refs[1])
        self.golden = load_golden(nm.GOLDEN_FILE)
        self.many = _starts(130, 12)
        self.par_many = nm.params_of(nm.keys_of(130))
        self.tau_many = np.array([np.inf, 4.0, 2.0, 1.0, 2.0] * 26)              # period 5 against the keys' 4
        self._cache = {}

    def solver(self, B, refs=None, **kw):
        from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
        xr, ur = refs or (self.xr, self.ur)
        return BatchedNewtonSolver(self.eng, xr, ur, B, **{**nm.SHORT, **kw})

    def many_loop(self, **kw):
        """The 130 starts, per-lane limits, lane b on KEYS[b % 4], iters 1 / 3 at step 0 (computed once per variant)."""
        key = tuple(sorted(kw.items()))
        if key not in self._cache:
            self._cache[key] = self.solver(130, tau_max=self.tau_many, **kw).closed_loop(
                self.many, plant=self.par_many, **nm.PARITY_ITERS)
        return self._cache[key]


@pytest.fixture(scope="module")
def ctx(task2_refs):
    return _Ctx(task2_refs)


# --------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("case", nm.PARITY_CASES, ids=[nm.case_name(*c) for c in nm.PARITY_CASES])
def test_restatement_parity(ctx, case):
    tau, u0, ref = case
    x0, xr, ur, keys = nm.parity_inputs(ctx.refs[0], ctx.refs[1], u0, ref)
    s = ctx.solver(nm.PARITY_LANES, refs=(xr, ur), **({} if tau is None else dict(tau_max=tau)))
    assert s.u0_zero == (u0 == "zero") and s.ref_lane == (ref == "lane")
    r = s.closed_loop(x0, plant=nm.params_of(keys), **nm.PARITY_ITERS)
    idx = np.arange(nm.PARITY_LANES) % nm.DISTINCT
    want = {k: ctx.golden[f"{nm.case_name(*case)}/{k}"][idx] for k in nm.PARITY_FIELDS}
    got = {k: getattr(r, k).cpu().numpy() for k in ("x", "u", "iters", "rollouts", "stop", "cost")}
    ex, eu = rel_l2(got["x"], want["x"]), rel_l2(got["u"], want["u"])
    ec = float(np.max(np.abs(got["cost"] - want["cost"]) / np.abs(want["cost"])))
    bad = {k: int((got[k] != want[k]).sum()) for k in ("iters", "rollouts", "stop")}
    print(nm.case_name(*case), "x", ex, "u", eu, "cost", ec, "count mismatches", bad, "margin", want["margin"].min())
    for k in ("iters", "rollouts", "stop"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5])
    assert ex <= TOL_TRAJ and eu <= TOL_TRAJ and ec <= TOL_COST
    # what the case exercises: re-anchors on the mismatched plants, line-search failures without a limit
    assert (want["reanchors"][np.arange(nm.PARITY_LANES) % 4 != 0] == 39).all()
    assert (got["stop"] == nb.CONVERGED).any() and (tau is not None or (got["stop"] == nb.LS_FAILED).any())
    if tau is not None:
        assert float(r.u_max.max()) <= tau
    goal = xr[:, -1] if xr.ndim == 3 else xr[-1]                            # the lane's own reference row
    assert np.array_equal(r.err_final.cpu().numpy(), np.abs(got["x"][:, -1] - goal).max(1))


# --------------------------------------------------------------------------------------- 2. the prefix is the solve
@pytest.mark.parametrize("tau", [None, 2.0])
def test_without_replanning_on_the_design_model_the_loop_applies_the_solve(ctx, tau):
    import torch
    from gymnast_optimalcontrol_amd import _lib
    kw = dict(tol=1e-4, **({} if tau is None else dict(tau_max=tau)))
    x0 = ctx.x0[np.arange(70) % 5]
    plan = ctx.solver(70, **kw).solve(x0, 3)
    assert bool((plan.status == _lib.MAX_ITERS).all())                    # no lane reaches tol within 3 iterations
    r = ctx.solver(70, **kw).closed_loop(x0, iters=0, iters_first=3)
    assert torch.equal(r.x, plan.x) and torch.equal(r.u, plan.u)
    assert not bool(r.rollouts[:, 1:].any()) and torch.equal(r.rollouts[:, 0], plan.n_rollouts)
    assert bool((r.iters[:, 0] == 3).all()) and not bool(r.iters[:, 1:].any()) and bool((r.stop == _lib.ACTIVE).all())
    assert torch.equal(r.cost[:, 0], plan.cost)


# ------------------------------------------------------------------------------------------------- 3. chunking
def test_chunks_give_the_same_bits(ctx):
    x0, xr, ur, keys = nm.parity_inputs(ctx.refs[0], ctx.refs[1], "live", "lane")
    tau = np.array([np.inf, 2.0] * 35)
    runs = [ctx.solver(70, refs=(xr, ur), tau_max=tau).closed_loop(x0, plant=nm.params_of(keys), steps_per_launch=n,
                                                                  **nm.PARITY_ITERS) for n in (None, 1, 7)]
    assert bool((runs[0].rollouts > 1).any()) and bool((runs[0].stop != 0).any())
    for r, n in zip(runs[1:], (1, 7)):
        _same(r, runs[0], f"steps_per_launch={n}")


# ---------------------------------------------------------------------------------------------- 4. lane = itself
def test_every_lane_is_itself_whatever_its_place_and_neighbours(ctx):
    base = ctx.many_loop()
    plain = ctx.many_loop(reorder=False)                                   # the caller's lane order, no lane map
    _same(plain, base, "reorder=False")
    # lanes diverge from one another: limits, plants and decisions differ across the batch
    assert len({tuple(r) for r in base.rollouts.cpu().numpy().tolist()}) > 20
    rev = ctx.solver(130, tau_max=ctx.tau_many[::-1].copy()).closed_loop(
        ctx.many[::-1].copy(), plant=ctx.par_many[::-1].copy(), **nm.PARITY_ITERS)
    import torch
    back = torch.arange(129, -1, -1, device=base.x.device)
    _same(rev, base, "reversed batch", back, slice(None))
    lanes = [0, 63, 64, 77, 129]
    alone = ctx.solver(5, tau_max=ctx.tau_many[lanes]).closed_loop(ctx.many[lanes], plant=ctx.par_many[lanes],
                                                                   **nm.PARITY_ITERS)
    pick = torch.as_tensor(lanes, device=base.x.device)
    _same(alone, base, "five lanes alone", slice(None), pick)
    # every other lane's start, limit and plant replaced
    others = np.setdiff1d(np.arange(130), lanes)
    x0, tau, par = ctx.many.copy(), ctx.tau_many.copy(), ctx.par_many.copy()
    x0[others] = _starts(130, 99)[others]
    tau[others] = 1.5
    par[others] = nm.params_of([2])[0]
    swapped = ctx.solver(130, tau_max=tau).closed_loop(x0, plant=par, **nm.PARITY_ITERS)
    _same(swapped, base, "other lanes replaced", pick, pick)
    assert not torch.equal(swapped.x[1], base.x[1])


# ------------------------------------------------------------------------------------- 5. a plant that blows up
def test_a_plant_that_drives_its_loop_non_finite_stays_in_its_lane(ctx):
    import torch
    from gymnast_optimalcontrol_amd import _lib
    x0 = ctx.x0[np.arange(70) % 5]
    keys = nm.keys_of(70)
    par = nm.params_of(keys)
    base = ctx.solver(70, tau_max=2.0).closed_loop(x0, plant=par, **nm.PARITY_ITERS)
    bad = par.copy()
    hit = [7, 64]                                                           # one lane in each wavefront
    bad[hit] = [PUMP[k] for k in ("m1", "m2", "l1", "lc1", "l2", "lc2", "I1", "I2", "g", "f1", "f2")]
    r = ctx.solver(70, tau_max=2.0).closed_loop(x0, plant=bad, **nm.PARITY_ITERS)
    keep = torch.as_tensor(np.setdiff1d(np.arange(70), hit), device=r.x.device)
    _same(r, base, "neighbours of the diverging lanes", keep, keep)
    for b in hit:
        finite = torch.isfinite(r.x[b]).all(dim=1).cpu().numpy()
        assert not finite.all(), "the plant must drive the loop non-finite within the horizon"
        t = int(np.argmin(finite))                                          # the first non-finite applied state
        print("lane", b, "breaks at step", t, "stop", r.stop[b].tolist())
        assert 0 < t < 40 and bool((r.stop[b, t:] == _lib.LS_FAILED).all())
        assert bool((r.rollouts[b, t:] >= 20).all()) and not bool(torch.isfinite(r.err_final[b]))


# ------------------------------------------------------------------------------------------------ 6. full length
def test_full_length_loop(ctx):
    """The headline references, 4 lanes, every step, iters = 1, tau_max = 18, two lanes on "heavy".  On all 501 knots
    one loop takes 3.56 s on the MI355X and this test, which runs it whole and in chunks, 7.2 s (profiles/newton_mpc/
    README.md): over the 5 s at which it runs on the first 251 knots instead, as it does."""
    import torch
    N = 251
    xr, ur = np.asarray(ctx.refs[0], float)[:N], np.asarray(ctx.refs[1], float)[:N - 1]
    assert xr.shape == (N, 4) and ur.shape == (N - 1, 2)
    x0 = np.zeros((4, 4))
    x0[:, :2] = np.random.default_rng(3).uniform(-0.2, 0.2, (4, 2))
    par = nm.params_of([1, "heavy", 1, "heavy"])
    kw = dict(tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0, max_ls=20, tau_max=18.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ctx.solver(4, refs=(xr, ur), **kw).closed_loop(x0, plant=par, iters=1)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    print(f"full-length loop: 4 lanes, N = {N}, {N - 1} steps, iters = 1:", round(secs, 3), "s; steps with stop != 0:",
          int((r.stop != 0).sum()), "of", r.stop.numel(), "rollouts", r.rollouts.sum(1).tolist(), "err_final",
          r.err_final.tolist())
    assert r.x.shape == (4, N, 4) and r.n_steps == N - 1
    assert bool(torch.isfinite(r.x).all()) and bool(torch.isfinite(r.u).all()) and bool(torch.isfinite(r.cost).all())
    assert float(r.u.abs().max()) <= 18.0 and float(r.u_max.max()) <= 18.0
    assert bool((r.rollouts[[1, 3], :-1] >= 1).all())                       # the heavy plants re-anchor at every step
    chunked = ctx.solver(4, refs=(xr, ur), **kw).closed_loop(x0, plant=par, iters=1, steps_per_launch=64)
    _same(chunked, r, "chunks of 64 steps")


# ---------------------------------------------------------------------------------------------- 7. ABI refusals
def test_abi_refusals_launch_nothing(ctx):
    import torch
    s = ctx.solver(70, tau_max=2.0, reorder=False)
    x0 = ctx.x0[np.arange(70) % 5]
    r = s.closed_loop(x0, n_steps=3, **nm.PARITY_ITERS)
    table = ctx.eng.model_table({}, 128)                                    # Bp rows
    outs = [r.x, r.u, r.iters, r.rollouts, r.cost, r.stop]
    state = [*s.x, *s.u, s.K1, s.cs, s.cost, s.res_buf, s.n_iter, s.n_roll, *outs]
    before = [t.clone() for t in state]
    tau, ptrs = s.tau_buf.data_ptr(), [t.data_ptr() for t in outs]

    def run(plant=table.data_ptr(), t0=3, t1=4, iters=1, out=ptrs):
        return s._launch(s.MPC_RUN, tau, plant, t0, t1, iters, *out, armijo=True, check=False)

    EINVAL = 1
    assert run(plant=None) == EINVAL and run(plant=table.data_ptr() + 8) == EINVAL
    assert run(t0=-1) == EINVAL and run(t1=41) == EINVAL and run(t0=5, t1=4) == EINVAL and run(iters=-1) == EINVAL
    assert run(out=[None] + ptrs[1:]) == EINVAL and run(out=ptrs[:5] + [None]) == EINVAL
    torch.cuda.synchronize()
    for a, b in zip(state, before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert run(t0=3, t1=3) == 0                                             # an empty range: valid, nothing launched
    torch.cuda.synchronize()
    for a, b in zip(state, before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert run() == 0                                                        # and the same call, valid, does run
    torch.cuda.synchronize()
    assert bool((r.x[:, 4] != 0).any())
