"""The dense restatements (tests/dense_ref.py) against the float64 oracles and the reference's own results
(tests/golden/dense_kats.npz), and the conditions the dense GPU tests rest on, checked once on the data those
tests use (CPU only).

  * float64 vs extended precision: how far the NumPy oracles (oracle/acrobot_np.py, oracle/tracking_np.py, or the
    restatement evaluated in float64 where the oracles have no function) sit from the np.longdouble result on every
    generator.  The GPU tests' pure-algebra bound is 64 x this deviation (dense_ref.algebra_bound); if it exceeded
    1e-14 the inputs would be too ill-conditioned to judge a kernel.
  * pivot share: at least a quarter of the (lane, stage) pairs of the riccati_general inputs take each branch of
    the partial-pivoting test |G10| > |G00|.
  * stop-count margin: wherever an iteration count of compute_P_inf is asserted equal, max|dP| - tol at the stop
    map and at the one before exceeds 100 float64 ulps of max|P| in extended precision.
"""
import os
import sys

import numpy as np
import pytest

import dense_ref as dr
from conftest import load_golden, rel_l2

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

COND = 1e-14        # float64 oracle within this of the extended-precision result, else the seed is unusable


@pytest.fixture(scope="module")
def kats():
    return load_golden("dense_kats")


def test_fixture_was_made_from_these_generators(kats):
    from make_golden_dense import inputs_digest
    assert str(kats["digest"]) == inputs_digest()


# ------------------------------------------------------------------------------ float64 vs extended precision
@pytest.mark.parametrize("B,T", dr.RICCATI_SHAPES + [(130, 9)])
def test_riccati_oracle_vs_extended_and_pivot_share(B, T):
    from oracle import acrobot_np as ref
    a = dr.riccati_args(dr.gen_riccati(), B, T)
    K, sig, dJ, swap = dr.calculate_K_and_sigma(*a)
    Ko, so, dJo = ref.riccati(*a)
    dev = dict(K=dr.chan_err(Ko, K, 2), sigma=dr.chan_err(so, sig, 1), dJ=dr.lane_err(dJo, dJ))
    print(f"riccati B={B} T={T}: swap share {swap.mean():.3f}, float64 oracle vs longdouble {dev}")
    assert max(dev.values()) < COND, dev
    assert np.abs(np.asarray(K[:, :, 0], float)).min() > 0          # row 0 of every gain is live
    if B > 1:       # one lane is one parity: lane 0 swaps at most stages (checked below), lane 1 at few
        assert 0.25 <= swap.mean() <= 0.75, swap.mean()
    # the same decision from the float64 G the kernel sees: no stage sits on the |G10| == |G00| tie
    K64, _, _, swap64 = dr.calculate_K_and_sigma(*a, dtype=np.float64)
    assert np.array_equal(swap, swap64)


def test_single_lanes_cover_both_pivot_branches():
    d = dr.gen_riccati()
    for T in (1, 2, 8):
        a = dr.riccati_args(d, 2, T)
        swap = dr.calculate_K_and_sigma(*a)[3]
        assert swap[0].mean() >= 0.75 and swap[1].mean() <= 0.25, swap     # B'PB moves a stage or two


def _solve2_unpivoted(G, Y):
    """float64 elimination of the 2x2 system without the row swap (what a kernel that lost its pivot computes)."""
    l10 = G[..., 1, 0] / G[..., 0, 0]
    u11 = G[..., 1, 1] - l10 * G[..., 0, 1]
    x1 = (Y[..., 1, :] - l10[..., None] * Y[..., 0, :]) / u11[..., None]
    return np.stack([(Y[..., 0, :] - G[..., 0, 1, None] * x1) / G[..., 0, 0, None], x1], -2)


def test_pivot_critical_data_needs_the_row_swap():
    """gen_riccati_pivot_critical: every stage swaps, the pivoted float64 oracle sits at rounding level, and the
    same elimination without the swap is off by orders of magnitude more than the GPU test's bound."""
    from oracle import acrobot_np as ref
    d = dr.gen_riccati_pivot_critical()
    a = dr.riccati_args(d, 65, 2)
    K, sig, dJ, swap = dr.calculate_K_and_sigma(*a)
    assert swap.all()
    Ko, so, dJo = ref.riccati(*a)
    dev = dict(K=dr.chan_err(Ko, K, 2), sigma=dr.chan_err(so, sig), dJ=dr.lane_err(dJo, dJ))
    print(f"pivot-critical riccati: float64 oracle vs longdouble {dev}")
    assert max(dev.values()) < COND, dev
    # last stage, where P = Q_T needs no recursion: K = -G^-1 F with and without the swap
    A, B, R, S, QT = d["A"][:, -1], d["B"][:, -1], d["R"][:, -1], d["S"][:, -1], d["QT"]
    G = R + np.swapaxes(B, 1, 2) @ QT @ B
    F = S + np.swapaxes(B, 1, 2) @ QT @ A
    bad = dr.chan_err(-_solve2_unpivoted(G, F), K[:, -1], 2)
    print(f"  ... the unpivoted elimination: {bad:.2e}")
    assert bad > 1e3 * dr.algebra_bound(dev["K"])


def test_cost_oracles_vs_extended():
    from oracle import acrobot_np as ref
    Q, R, QT = dr.gen_dense_weights()
    for M in (Q, R, QT):
        assert np.abs(M - M.T)[~np.eye(M.shape[0], dtype=bool)].min() > 1e-3     # no symmetric pair
    t = dr.gen_trajectories()
    for N in dr.KNOTS:
        x, u = t["x"][:, :N], t["u"][:, :N - 1]
        J = dr.total_cost(x, u, t["x_ref"], t["u_ref"], Q, R, QT)
        Jo = ref.total_cost(x, u, t["x_ref"][:N], t["u_ref"][:N - 1], Q, R, QT)
        dev = dr.lane_err(Jo, J)
        print(f"total_cost N={N}: float64 oracle vs longdouble {dev:.2e}")
        assert dev < COND and (np.asarray(J, float) > 0).all()
    p = dr.gen_points()
    l, gx, gu = dr.derivatives_cost(p["X"], p["xr"], p["U"], p["ur"], Q, R)
    l64, gx64, gu64 = dr.derivatives_cost(p["X"], p["xr"], p["U"], p["ur"], Q, R, dtype=np.float64)
    lT, gT = dr.derivatives_cost_terminal(p["X"], p["xr"], QT)
    lT64, gT64 = dr.derivatives_cost_terminal(p["X"], p["xr"], QT, dtype=np.float64)
    dev = dict(l=dr.lane_err(l64, l), gx=dr.chan_err(gx64, gx), gu=dr.chan_err(gu64, gu), lT=dr.lane_err(lT64, lT),
               gT=dr.chan_err(gT64, gT))
    print(f"derivatives_Cost: float64 vs longdouble {dev}")
    assert max(dev.values()) < COND, dev
    # a transposed Q index must be visible: 2 Q'e differs from 2 Q e by O(1)
    assert dr.chan_err(2 * (np.asarray(p["X"] - p["xr"]) @ Q), gx) > 1e-2


def test_tracking_oracles_vs_extended():
    from oracle import tracking_np as tr
    g = dr.gen_tracking()
    for M in (g["Q"], g["R"], g["QT"]):
        assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() > 0 and abs(M[0, 1]) > 1e-3
    assert np.abs(g["B"][:, :, 0]).min() > 0 and np.abs(g["B_pad"][:, 0]).min() > 0
    S = dr.TSTAGES
    # all gains, discretize off: tracking_np's riccati_step is the float64 oracle
    K = dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], S + 1)
    P = g["QT"]
    Ko = np.zeros((S, 2, 4))
    for s in reversed(range(S)):
        Ko[s], P = tr.riccati_step(g["A"][s], g["B"][s], P, g["Q"], g["R"])
    dev = dr.chan_err(Ko, K, 2)
    print(f"tv_lqr_gains all_gains: tracking_np vs longdouble {dev:.2e}")
    assert dev < COND and np.abs(np.asarray(K[:, 0], float)).min() > 0
    for disc in (False, True):
        for L, nwin, allg in ((S + 1, 1, True), (2, 1, True), (6, 1, False), (6, 5, False), (6, 70, False)):
            kw = dict(L=L, nwin=nwin, all_gains=allg, A_pad=g["A_pad"], B_pad=g["B_pad"], discretize=disc)
            K = dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], **kw)
            K64 = dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], dtype=np.float64, **kw)
            dev = dr.chan_err(K64, K, 2)
            print(f"tv_lqr_gains disc={disc} L={L} nwin={nwin} all={allg}: float64 vs longdouble {dev:.2e}")
            assert dev < COND
            assert np.abs(np.asarray(K[:, 0], float)).max() > 1e-2      # row 0 is live
        Kall = dr.tv_lqr_gains(g["A"], g["B"], g["Q"], g["R"], g["QT"], S + 1, discretize=disc)
        for L in (2, 7, 16):
            Kl = np.concatenate([Kall, Kall[:4]])[:L - 1]
            X, U = dr.lq_forward(g["A"], g["B"], Kl, g["x0"], L, g["A_pad"], g["B_pad"], disc)
            X64, U64 = dr.lq_forward(g["A"], g["B"], Kl, g["x0"], L, g["A_pad"], g["B_pad"], disc, dtype=np.float64)
            dev = max(dr.chan_err(X64, X), dr.chan_err(U64, U))
            print(f"lq_forward disc={disc} L={L}: float64 vs longdouble {dev:.2e}")
            assert dev < COND


def test_p_inf_oracle_vs_extended_and_stop_margins(kats):
    from oracle import tracking_np as tr
    trk = load_golden("tracking")
    dd = dr.gen_dare()
    Qm, Rm = dr.gen_mpc_weights()
    assert np.array_equal(Rm, Rm.T) and Rm[0, 1] != 0 and np.linalg.eigvalsh(Rm).min() > 0
    assert np.array_equal(Qm, Qm.T) and np.linalg.eigvalsh(Qm).min() > 0 and abs(Qm[0, 1]) > 0
    for name, (A, B, Q, R), fix in (("dense", (dd["A"], dd["B"], dd["Q"], dd["R"]), kats["pinf_dense"]),
                                    ("pad", (trk["A_f"], trk["B_f"], Qm, Rm), kats["pinf_pad"])):
        P, it, margin = dr.stop_margin_ulps(A, B, Q, R)
        Po, ito = tr.compute_P_inf(A, B, Q, R)
        dev = dr.chan_err(Po, P, 0)
        print(f"compute_P_inf {name}: stops at {it}, margin {margin:.0f} ulp of max|P|, tracking_np vs longdouble "
              f"{dev:.2e}, max|P| {float(np.abs(P).max()):.4g}")
        assert it == ito < 1000
        assert margin > 100, margin
        np.testing.assert_array_equal(Po, fix)            # the reference's own loop: the same NumPy operations
        # the pad (marginally stable, P ~ 2e5) moves its fixed point by ~1e-12 under float64 rounding: its P is
        # judged at the trackers' 1e-9 / 1e-10, and its stop count by the margin above (dP itself is clean)
        assert dev < (COND if name == "dense" else 1e-11)
    A, B, Q, R = dr.slow_pair_dense()
    P, it, _ = dr.compute_P_inf(A, B, Q, R)
    Po, ito = tr.compute_P_inf(A, B, Q, R)
    assert it == ito == 1001 and np.isfinite(np.asarray(P, float)).all()
    dev = dr.chan_err(Po, P, 0)
    print(f"compute_P_inf slow pair, dense R: 1000 maps, tracking_np vs longdouble {dev:.2e}")
    assert dev < 1e-13


# --------------------------------------------------------------------------------- against the reference's data
def test_restatements_and_oracles_match_the_reference(kats):
    from oracle import acrobot_np as ref
    from oracle import tracking_np as tr
    n = kats["ric_dJ"].shape[0]
    a = dr.riccati_args(dr.gen_riccati(), n, dr.NMAX)
    K, sig, dJ, swap = dr.calculate_K_and_sigma(*a)
    assert 0.25 <= swap.mean() <= 0.75
    assert dr.chan_err(kats["ric_K"], K, 2) < COND and dr.chan_err(kats["ric_sigma"], sig) < COND
    assert dr.lane_err(kats["ric_dJ"], dJ) < COND
    Ko, so, dJo = ref.riccati(*a)
    assert dr.chan_err(Ko, kats["ric_K"], 2) < COND and dr.lane_err(dJo, kats["ric_dJ"]) < COND

    Q, R, QT = dr.gen_dense_weights()
    p = dr.gen_points()
    m = kats["sc_l"].shape[0]
    l, gx, gu = dr.derivatives_cost(p["X"][:m], p["xr"][:m], p["U"][:m], p["ur"][:m], Q, R)
    lT, gT = dr.derivatives_cost_terminal(p["X"][:m], p["xr"][:m], QT)
    for got, want, keep in ((kats["sc_gx"], gx, 1), (kats["sc_gu"], gu, 1), (kats["sc_gT"], gT, 1)):
        assert dr.chan_err(got, want, keep) < COND
    assert dr.lane_err(kats["sc_l"], l) < COND and dr.lane_err(kats["sc_lT"], lT) < COND

    t = dr.gen_trajectories()
    g = dr.gen_gains()
    J = dr.total_cost(t["x"][:n], t["u"][:n], t["x_ref"], t["u_ref"], Q, R, QT)
    assert dr.lane_err(kats["tc_J"], J) < COND
    xn, un = ref.closed_loop(t["x"][:n], t["u"][:n], g["K"][:n], g["sigma"][:n], g["gamma"][:n])
    assert rel_l2(xn, kats["cl_x"]) < 1e-12 and dr.chan_err(un, kats["cl_u"]) < 1e-12
    assert np.abs(kats["cl_u"][:, :, 0] - t["u"][:n, :, 0]).min() > 1e-3      # channel 0 moved at every stage

    k = dr.gen_track()
    x, u = tr.simulate_tracking(k["x_ff"], k["u_ff"], k["K"], k["x0"][:n])
    assert rel_l2(x, kats["trk_x"]) < 1e-12 and dr.chan_err(u, kats["trk_u"]) < 1e-12
    assert np.abs(kats["trk_u"][:, :, 0] - k["u_ff"][:, 0]).min() > 1e-4
