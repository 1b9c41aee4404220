"""The stand-alone entry points on dense data and on batch shapes past one lane and one workgroup.

Every other fixture has the acrobot's sparsity (row 0 of each gain zero, diagonal weights, a pivot test that never
swaps) and calls these entry points with one lane.  Here each lane has its own random states, controls (tau1
non-zero) and, where they are inputs, gains (row 0 non-zero), sigma (channel 0 non-zero) and step size; the lane
counts 1, 63, 64, 65, 130 and knot counts 2, 3, 9 cover a partial wavefront, a second wavefront group and workgroup
and the T = 1 and T = 2 loop edges; the point kernels run 600 points (three 256-thread blocks, the last partial).

References: oracle/acrobot_np.py for everything that carries dynamics, at the tolerance tests/test_gpu_parity.py or
tests/test_armijo_sweep.py applies to the same entry point; tests/dense_ref.py (np.longdouble) and the reference's
own results (tests/golden/dense_kats.npz) for the pure algebra, at 64 x the float64 oracle's own deviation from the
extended-precision result on the same inputs (dense_ref.algebra_bound; floor 64 x 2^-52 = 1.4e-14).  Comparisons are
per output and per channel, each channel on its own norm (dense_ref.chan_err).  Every batched call's lanes 0, 62 (or
the last) and B-1 equal, bit for bit, a one-lane call on that lane's inputs.

Measured kernel-vs-reference deviations (MI355X, largest over the shapes; bound in brackets):
  continuous_dynamics 3.1e-16, rk4 7.2e-17 (per channel), jacobians A 4.4e-16, B 7.5e-16 of max  [rtol 1e-11 / 1e-10]
  stage_cost_derivs   l 3.3e-16 [2.3e-14], gx 8.7e-17, gu 8.0e-17, gT 9.0e-17 [1.4e-14], lT 3.5e-16 [2.7e-14]
  total_cost          3.8e-16 [1.4e-14 .. 3.4e-14]
  rollout_open_loop   x 3.2e-16 [1e-12], J 3.8e-16 [1e-11]
  closed_loop         x_new 3.9e-16, u_new 1.1e-16 [1e-10], J 3.7e-16 [1e-11]
  gamma_sweep         5.6e-16 [1e-10]; padding lanes NaN, exactly
  backward            K row 1 6.6e-16, sigma 1.0e-16, dJ 3.3e-16 [1e-10], lambda 3.1e-16 [1e-12]; K row 0 = 0 exactly
  linearize           A_d 3.6e-15 absolute [rtol 1e-11 + atol 1e-11]
  riccati_general     K 9.9e-16 [2.0e-14 .. 3.9e-14], sigma 4.9e-16 [1.4e-14 .. 3.8e-14], dJ 9.6e-16 [1.4e-14 .. 8.2e-14];
                      pivot-critical data: K 2.1e-16, sigma 1.3e-16 [1.4e-14], dJ 3.2e-15 [1.6e-13]
Every lane-independence comparison is bit for bit.  Both modules together run in 4 s.

The tests bite (value mutations of the kernels, run once, nothing committed): swapping k0.x / k0.y in rollout_ref
fails test_closed_loop_dense_gains (u_new channel 0 off by 0.05 .. 0.25) and test_gamma_sweep_block_permutation;
transposing Q's index in k_stage_cost_derivs' gradient fails test_stage_cost_derivs_nonsymmetric_weights (gx off by
0.53); in solve2, dropping the swap of the right-hand-side columns fails every test_riccati_general_pivoting case
(K off by ~2), and never swapping at all fails test_riccati_general_needs_its_pivot (3.4e-8) -- on the other data an
unpivoted elimination is only a reordering at rounding level, which the bound accepts.  The earlier tests of the same
entry points (test_armijo_sweep, test_tracking, test_gpu_parity's primitive and iteration tests) pass under each.
"""
import ctypes as C

import numpy as np
import pytest

import dense_ref as dr
from conftest import load_golden

pytestmark = pytest.mark.gpu

NONDEFAULT = dict(Q=(3.0, 7.0, 0.5, 0.2), R=(0.4, 2.5), QT=(11.0, 5.0, 2.0, 0.7))


def _np(t):
    return t.detach().cpu().numpy()


def _lanes(B):
    return sorted({0, min(62, B - 1), B - 1})


def _report(name, err, bound):
    print(f"DEV {name}: {err:.2e} (bound {bound:.1e})")
    assert err <= bound, (name, err, bound)


@pytest.fixture(scope="module", params=["default", "nondefault"])
def wcase(request):
    """(engine, Q, R, QT matrices): the default weights and one non-default diagonal set, model parameter set 1."""
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine, Weights
    w = Weights() if request.param == "default" else Weights(**NONDEFAULT)
    return AcrobotEngine(params=1, weights=w), np.diag(w.Q), np.diag(w.R), np.diag(w.QT)


@pytest.fixture(scope="module")
def eng():
    from gymnast_optimalcontrol_amd.engine import AcrobotEngine
    return AcrobotEngine(params=1)


@pytest.fixture(scope="module")
def kats():
    return load_golden("dense_kats")


@pytest.fixture(scope="module")
def traj():
    """The generators' trajectories and gains with the oracle's rollouts of all LANES lanes over NMAX knots, computed
    once (both rollouts are causal: the first N knots are the N-knot rollout)."""
    from oracle import acrobot_np as ref
    t = dr.gen_trajectories()
    g = dr.gen_gains()
    d = dict(t, **g)
    d["x_open"] = ref.simulate_open_loop(t["x"][:, 0], t["u"])
    d["x_cl"], d["u_cl"] = ref.closed_loop(t["x"], t["u"], g["K"], g["sigma"], g["gamma"])
    return d


# ------------------------------------------------------------------------------------------------ point kernels
def test_point_kernels_over_three_blocks(eng):
    from oracle import acrobot_np as ref
    p = dr.gen_points()
    X, U = p["X"], p["U"]
    assert X.shape[0] == 600 and np.abs(U[:, 0]).min() > 0
    f = _np(eng.continuous_dynamics(X, U)); r = _np(eng.rk4(X, U))
    A, B = (_np(a) for a in eng.jacobians(X, U))
    Ao, Bo = ref.jacobians(X, U)
    np.testing.assert_allclose(f, ref.continuous_dynamics(X, U), rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(r, ref.rk4(X, U), rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(A, Ao, rtol=1e-10, atol=1e-8)
    np.testing.assert_allclose(B, Bo, rtol=1e-10, atol=1e-12)
    print(f"DEV point kernels: f {dr.chan_err(f, ref.continuous_dynamics(X, U)):.2e}, rk4 "
          f"{dr.chan_err(r, ref.rk4(X, U)):.2e}, A {np.abs(A - Ao).max() / np.abs(Ao).max():.2e}, "
          f"B {np.abs(B - Bo).max() / np.abs(Bo).max():.2e}")
    for i in (0, 255, 256, 511, 512, 599):          # block edges: each point alone gives the same bits
        s = slice(i, i + 1)
        assert np.array_equal(_np(eng.continuous_dynamics(X[s], U[s])), f[s])
        assert np.array_equal(_np(eng.rk4(X[s], U[s])), r[s])
        A1, B1 = eng.jacobians(X[s], U[s])
        assert np.array_equal(_np(A1), A[s]) and np.array_equal(_np(B1), B[s])


def test_stage_cost_derivs_nonsymmetric_weights(eng, kats):
    p = dr.gen_points()
    Q, R, QT = dr.gen_dense_weights()
    X, xr, U, ur = p["X"], p["xr"], p["U"], p["ur"]
    l, gx, gu = (_np(a) for a in eng.stage_cost_derivs(X, xr, U, ur, Q, R))
    lT, gT, none = eng.stage_cost_derivs(X, xr, None, None, QT, None, terminal=True)
    lT, gT = _np(lT), _np(gT)
    assert none is None
    ref = dr.derivatives_cost(X, xr, U, ur, Q, R) + dr.derivatives_cost_terminal(X, xr, QT)
    f64 = dr.derivatives_cost(X, xr, U, ur, Q, R, dtype=np.float64) + \
        dr.derivatives_cost_terminal(X, xr, QT, dtype=np.float64)
    m = kats["sc_l"].shape[0]
    fix = (kats["sc_l"], kats["sc_gx"], kats["sc_gu"], kats["sc_lT"], kats["sc_gT"])
    for name, got, want, o, fx in zip(("l", "gx", "gu", "lT", "gT"), (l, gx, gu, lT, gT), ref, f64, fix):
        err = dr.lane_err if got.ndim == 1 else dr.chan_err
        bound = dr.algebra_bound(err(o, want))
        _report(f"stage_cost_derivs {name}", err(got, want), bound)
        assert err(got[:m], fx) <= bound + err(fx, want[:m]), name      # the reference's own numbers
    for i in (0, 255, 256, 599):
        s = slice(i, i + 1)
        l1, gx1, gu1 = eng.stage_cost_derivs(X[s], xr[s], U[s], ur[s], Q, R)
        assert np.array_equal(_np(l1), l[s]) and np.array_equal(_np(gx1), gx[s]) and np.array_equal(_np(gu1), gu[s])


# ----------------------------------------------------------------------------------------------- total cost
@pytest.mark.parametrize("B", dr.LANE_COUNTS)
def test_total_cost_dense_weights(eng, traj, kats, B):
    from gymnast_optimalcontrol_amd import trajectory_generation as tg
    from oracle import acrobot_np as ref
    Q, R, QT = dr.gen_dense_weights()
    for N in dr.KNOTS:
        x, u, xr, ur = traj["x"][:B, :N], traj["u"][:B, :N - 1], traj["x_ref"][:N], traj["u_ref"][:N - 1]
        J = _np(eng.total_cost(x, u, xr, ur, Q, R, QT))
        want = dr.total_cost(x, u, xr, ur, Q, R, QT)
        bound = dr.algebra_bound(dr.lane_err(ref.total_cost(x, u, xr, ur, Q, R, QT), want))
        _report(f"total_cost B={B} N={N}", dr.lane_err(J, want), bound)
        for l in _lanes(B):
            assert _np(eng.total_cost(x[l:l + 1], u[l:l + 1], xr, ur, Q, R, QT))[0] == J[l], (N, l)
        assert tg.total_cost(x[B - 1], u[B - 1], xr, ur, Q, R, QT) == J[B - 1]      # the reference-style call
        if N == dr.NMAX and B >= 4:
            fx = kats["tc_J"]
            assert dr.lane_err(J[:4], fx) <= bound + dr.lane_err(fx, want[:4])


# ------------------------------------------------------------------------------------------------- rollouts
@pytest.mark.parametrize("B", dr.LANE_COUNTS)
def test_rollout_open_loop_per_lane_controls(wcase, traj, B):
    from oracle import acrobot_np as ref
    e, Q, R, QT = wcase
    for N in dr.KNOTS:
        x0, u, xr, ur = traj["x"][:B, 0], traj["u"][:B, :N - 1], traj["x_ref"][:N], traj["u_ref"][:N - 1]
        x, J = e.rollout_open_loop(x0, u, xr, ur)
        x, J = _np(x), _np(J)
        xo = traj["x_open"][:B, :N]
        assert dr.chan_err(x, xo) < 1e-12, (N, dr.chan_err(x, xo))
        np.testing.assert_allclose(J, ref.total_cost(xo, u, xr, ur, Q, R, QT), rtol=1e-11)
        for l in _lanes(B):
            x1, J1 = e.rollout_open_loop(x0[l:l + 1], u[l:l + 1], xr, ur)
            assert np.array_equal(_np(x1)[0], x[l]) and _np(J1)[0] == J[l], (N, l)
    print(f"DEV rollout_open_loop B={B}: x {dr.chan_err(x, xo):.2e}, J "
          f"{dr.lane_err(J, ref.total_cost(xo, u, xr, ur, Q, R, QT)):.2e}")


@pytest.mark.parametrize("B", dr.LANE_COUNTS)
def test_closed_loop_dense_gains(wcase, traj, kats, B):
    from oracle import acrobot_np as ref
    e, Q, R, QT = wcase
    assert np.abs(traj["K"][:, :, 0]).min() > 0 and np.abs(traj["sigma"][:, :, 0]).min() > 0
    for N in dr.KNOTS:
        T = N - 1
        x, u, xr, ur = traj["x"][:B, :N], traj["u"][:B, :T], traj["x_ref"][:N], traj["u_ref"][:T]
        K, s, gam = traj["K"][:B, :T], traj["sigma"][:B, :T], traj["gamma"][:B]
        xn, un, J = (_np(a) for a in e.closed_loop(x, u, K, s, gam, xr, ur))
        xo, uo = traj["x_cl"][:B, :N], traj["u_cl"][:B, :T]
        ex, eu = dr.chan_err(xn, xo), dr.chan_err(un, uo)         # u channel 0 on its own norm
        assert ex < 1e-10 and eu < 1e-10, (N, ex, eu)
        Jo = ref.total_cost(xo, uo, xr, ur, Q, R, QT)
        np.testing.assert_allclose(J, Jo, rtol=1e-11)
        for l in _lanes(B):
            a = e.closed_loop(x[l:l + 1], u[l:l + 1], K[l:l + 1], s[l:l + 1], gam[l:l + 1], xr, ur)
            assert np.array_equal(_np(a[0])[0], xn[l]) and np.array_equal(_np(a[1])[0], un[l]), (N, l)
            assert _np(a[2])[0] == J[l], (N, l)
        if N == dr.NMAX and B >= 4:                               # the reference's own update
            assert dr.chan_err(xn[:4], kats["cl_x"]) < 1e-10 and dr.chan_err(un[:4], kats["cl_u"]) < 1e-10
    print(f"DEV closed_loop B={B}: x_new {ex:.2e}, u_new {eu:.2e}, J {dr.lane_err(J, Jo):.2e}")


@pytest.mark.parametrize("B,G", [(130, 5), (65, 1), (1, 9), (64, 8)])
def test_gamma_sweep_block_permutation(wcase, traj, B, G):
    """(Bp/64) G = 15, 2, 9, 8 blocks on a grid rounded up to a multiple of 8: idle tail blocks, a non-trivial
    XCD permutation, and the exact multiple.  Every (lane, step) entry against the oracle; padding lanes NaN."""
    import torch
    from gymnast_optimalcontrol_amd import _lib
    from gymnast_optimalcontrol_amd.engine import padded
    from oracle import acrobot_np as ref
    e, Q, R, QT = wcase
    N = dr.NMAX
    T = N - 1
    x, u, xr, ur = traj["x"][:B, :N], traj["u"][:B, :T], traj["x_ref"][:N], traj["u_ref"][:T]
    K, s = traj["K"][:B, :T], traj["sigma"][:B, :T]
    gammas = np.linspace(0.07, 1.0, G) if G > 1 else np.array([0.37])
    J = _np(e.gamma_sweep(x, u, K, s, gammas, xr, ur))
    assert J.shape == (B, G)
    want = np.empty((B, G))
    for g in range(G):
        xo, uo = ref.closed_loop(x, u, K, s, gammas[g])
        want[:, g] = ref.total_cost(xo, uo, xr, ur, Q, R, QT)
    np.testing.assert_allclose(J, want, rtol=1e-10)
    print(f"DEV gamma_sweep B={B} G={G}: {np.abs(J / want - 1).max():.2e}")
    for l in _lanes(B):
        J1 = _np(e.gamma_sweep(x[l:l + 1], u[l:l + 1], K[l:l + 1], s[l:l + 1], gammas, xr, ur))
        assert np.array_equal(J1[0], J[l]), l
    # the raw (G, Bp) buffer: real lanes as above, padding lanes NaN (include/gymnast_acrobot.h)
    Bp = padded(B)
    xs, us = e.pack(e.t(x), Bp), e.pack(e.t(u), Bp, W=1)
    Ks, ss = e.pack(e.t(K).reshape(B, T, 8), Bp), e.pack(e.t(s), Bp, W=1)
    gd, xrd, urd = e.t(gammas), e.t(xr), e.t(ur)
    raw = torch.zeros((G, Bp), dtype=torch.float64, device=e.device)
    _lib.check(e.lib.gym_gamma_sweep(C.byref(e.model), C.byref(e._w), xs.data_ptr(), us.data_ptr(), Ks.data_ptr(),
                                     ss.data_ptr(), gd.data_ptr(), G, xrd.data_ptr(), urd.data_ptr(), raw.data_ptr(),
                                     B, Bp, N, e.stream), "gym_gamma_sweep")
    raw = _np(raw)
    assert np.array_equal(raw[:, :B].T, J)
    assert np.isnan(raw[:, B:]).all() and raw[:, B:].size == G * (Bp - B)


# ------------------------------------------------------------------------------- backward sweep, linearisation
@pytest.mark.parametrize("B", dr.LANE_COUNTS)
def test_backward_sweep_and_linearize_per_lane(wcase, traj, B):
    from oracle import acrobot_np as ref
    e, Q, R, QT = wcase
    dev = {}
    for N in dr.KNOTS:
        T = N - 1
        x, u, xr, ur = traj["x"][:B, :N], traj["u"][:B, :T], traj["x_ref"][:N], traj["u_ref"][:T]
        Ad, Bd, q, r, QTb, qT = ref.stage_lists(x, u, xr, ur, Q, R, QT)
        Ko, so, dJo = ref.riccati(Ad, Bd, 2 * Q, 2 * R, np.zeros((2, 4)), q, r, QTb, qT)
        lamo = ref.costate(x, u, xr, ur, Q, QT)
        K, sig, dJ, smax, lam = (_np(a) for a in e.backward(x, u, xr, ur, want_lambda=True))
        assert np.all(K[:, :, 0, :] == 0)
        assert np.array_equal(smax, np.abs(sig).max(axis=(1, 2)))
        assert np.abs(sig[:, :, 0]).min() > 0                       # tau1 != tau1_ref: sigma channel 0 is live
        dev = dict(K1=dr.chan_err(K[:, :, 1], Ko[:, :, 1]), sigma=dr.chan_err(sig, so), dJ=dr.lane_err(dJ, dJo),
                   lam=dr.chan_err(lam, lamo))
        assert dev["K1"] < 1e-10 and dev["sigma"] < 1e-10 and dev["dJ"] < 1e-10 and dev["lam"] < 1e-12, (N, dev)
        np.testing.assert_allclose(smax, np.abs(so).max(axis=(1, 2)), rtol=1e-10)
        lin = [_np(a) for a in e.linearize(x, u, xr, ur)]
        np.testing.assert_allclose(lin[0], Ad, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(lin[1], Bd, rtol=1e-11, atol=1e-14)
        np.testing.assert_allclose(lin[2], q, rtol=1e-13)
        np.testing.assert_allclose(lin[3], r, rtol=1e-13)
        np.testing.assert_allclose(lin[4], qT, rtol=1e-13)
        assert np.abs(lin[3][:, :, 0]).min() > 0
        for l in _lanes(B):
            s1 = slice(l, l + 1)
            b1 = e.backward(x[s1], u[s1], xr, ur, want_lambda=True)
            for got, full in zip(b1, (K, sig, dJ, smax, lam)):
                assert np.array_equal(_np(got)[0], full[l]), (N, l)
            for got, full in zip(e.linearize(x[s1], u[s1], xr, ur), lin):
                assert np.array_equal(_np(got)[0], full[l]), (N, l)
    print(f"DEV backward B={B}: {dev}; linearize A_d {np.abs(lin[0] - Ad).max():.2e}")


@pytest.mark.parametrize("B", [3, 65])
def test_spare_rows_are_invisible(eng, traj, B):
    """The engine asks for at least the rows a kernel reads: u and sigma of N rows (one spare) under a reference of
    N + 2 rows give, bit for bit, what the exact-size call gives, on the rows the exact-size call returns.  N = 6;
    one partial wavefront, and one lane past a full one."""
    N = 6
    T = N - 1
    x, K, gam = traj["x"][:B, :N], traj["K"][:B, :T], traj["gamma"][:B]
    gammas = np.array([0.3, 1.0])
    Q, R, QT = dr.gen_dense_weights()

    def results(nu, nxr, nur):
        u, s, xr, ur = traj["u"][:B, :nu], traj["sigma"][:B, :nu], traj["x_ref"][:nxr], traj["u_ref"][:nur]
        return dict(closed_loop=eng.closed_loop(x, u, K, s, gam, xr, ur),
                    gamma_sweep=(eng.gamma_sweep(x, u, K, s, gammas, xr, ur),),
                    backward=eng.backward(x, u, xr, ur, want_lambda=True), linearize=eng.linearize(x, u, xr, ur),
                    total_cost=(eng.total_cost(x, u, xr, ur, Q, R, QT),))

    exact, spare = results(T, N, T), results(N, N + 2, N + 1)
    for name in exact:
        for i, (a, b) in enumerate(zip(exact[name], spare[name])):
            a, b = _np(a), _np(b)
            if name == "closed_loop" and i == 1:          # u_new has as many rows as u; the spare one is not written
                assert b.shape == (B, N, 2)
                b = b[:, :T]
            assert a.shape == b.shape and np.array_equal(a, b), (name, i)


# ------------------------------------------------------------------------------------------- dense Riccati
@pytest.mark.parametrize("B,T", dr.RICCATI_SHAPES + [(4, dr.NMAX)])
def test_riccati_general_pivoting(eng, kats, B, T):
    """calculate_K_and_sigma on data whose 2x2 solve swaps rows at about half of the (lane, stage) pairs; swapped
    and unswapped stages are also compared separately, so neither can hide in the other's norm."""
    from gymnast_optimalcontrol_amd import trajectory_generation as tg
    from oracle import acrobot_np as ref
    d = dr.gen_riccati()
    a = dr.riccati_args(d, B, T)
    K, sig, dJ = (_np(t) for t in eng.riccati_general(*a))
    Kr, sr, dJr, swap = dr.calculate_K_and_sigma(*a)
    Ko, so, dJo = ref.riccati(*a)
    bK = dr.algebra_bound(dr.chan_err(Ko, Kr, 2), 1e-12)
    bs = dr.algebra_bound(dr.chan_err(so, sr), 1e-12)
    bJ = dr.algebra_bound(dr.lane_err(dJo, dJr), 1e-12)
    _report(f"riccati_general K B={B} T={T}", dr.chan_err(K, Kr, 2), bK)
    _report(f"riccati_general sigma B={B} T={T}", dr.chan_err(sig, sr), bs)
    _report(f"riccati_general dJ B={B} T={T}", dr.lane_err(dJ, dJr), bJ)
    for name, m in (("swapped", swap), ("unswapped", ~swap)):
        if m.any():
            _report(f"riccati_general K {name} B={B} T={T}", dr.chan_err(K[m], Kr[m], 2), bK)
            _report(f"riccati_general sigma {name} B={B} T={T}", dr.chan_err(sig[m], sr[m]), bs)
    if B > 1:
        assert swap.any() and (~swap).any()
    for l in sorted(set(_lanes(B)) | {min(1, B - 1)}):        # lane 1: the no-swap parity alone
        a1 = tuple(v[l:l + 1] for v in a)
        K1, s1, dJ1 = (_np(t) for t in eng.riccati_general(*a1))
        assert np.array_equal(K1[0], K[l]) and np.array_equal(s1[0], sig[l]) and dJ1[0] == dJ[l], l
    if (B, T) == (4, dr.NMAX):                                # the reference's own results, and its call style
        assert dr.chan_err(K, kats["ric_K"], 2) <= bK + dr.chan_err(kats["ric_K"], Kr, 2)
        assert dr.chan_err(sig, kats["ric_sigma"]) <= bs + dr.chan_err(kats["ric_sigma"], sr)
        assert dr.lane_err(dJ, kats["ric_dJ"]) <= bJ + dr.lane_err(kats["ric_dJ"], dJr)
        for l in (0, 1):
            Kl, sl, dJl = tg.calculate_K_and_sigma(*[list(v[l]) for v in a[:7]], a[7][l], a[8][l])
            assert np.array_equal(np.asarray(Kl), K[l]) and np.array_equal(np.asarray(sl), sig[l]) and dJl == dJ[l]


def test_riccati_general_needs_its_pivot(eng):
    """Data on which the row swap decides the accuracy (G00 ~ 1e-9 against G10 ~ 3, every stage swaps): elimination
    without the swap is off by ~1e-7, with it the kernel sits at rounding level like the LAPACK-pivoted oracle."""
    from oracle import acrobot_np as ref
    a = dr.riccati_args(dr.gen_riccati_pivot_critical(), 65, 2)
    K, sig, dJ = (_np(t) for t in eng.riccati_general(*a))
    Kr, sr, dJr, swap = dr.calculate_K_and_sigma(*a)
    Ko, so, dJo = ref.riccati(*a)
    assert swap.all()
    _report("riccati_general pivot-critical K", dr.chan_err(K, Kr, 2),
            dr.algebra_bound(dr.chan_err(Ko, Kr, 2), 1e-12))
    _report("riccati_general pivot-critical sigma", dr.chan_err(sig, sr), dr.algebra_bound(dr.chan_err(so, sr), 1e-12))
    _report("riccati_general pivot-critical dJ", dr.lane_err(dJ, dJr), dr.algebra_bound(dr.lane_err(dJo, dJr), 1e-12))

