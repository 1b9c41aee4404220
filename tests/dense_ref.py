"""Extended-precision restatements of the pure-algebra entry points, and the seeded dense input generators
(test infrastructure; CPU only).

Every existing fixture has the acrobot's own sparsity: B_d[:, 0] = 0 and diagonal Q, R, so row 0 of every gain is
identically zero, the pivot test of the 2x2 solve never swaps, and off-diagonal weight terms are multiplied by zero.
The generators here produce DENSE data (row 0 of K non-zero, sigma channel 0 non-zero, non-symmetric weights, R
whose pivot test takes both branches) for one lane up to LANES lanes; lane l's data does not depend on how many
lanes a test takes, so a B = 1 call on lane l is comparable, bit for bit, with lane l of a batched call.

The restatements are plain NumPy in np.longdouble (x87 80-bit: eps 1.08e-19) with the 2x2 solves written out by
Cramer's rule (np.linalg does not take longdouble).  Passing dtype=np.float64 evaluates the same text in double:
that is the float64 yardstick for the operations oracle/ has no function for.  Operations that carry dynamics
(rollouts, linearisations, sweeps) are NOT restated here: they are compared with oracle/acrobot_np.py and
oracle/tracking_np.py.

Restated (trajectory_generation.py / trajectory_tracking.py of the reference, from reading them; nothing copied):
  calculate_K_and_sigma   G = R + B'PB, F = S + B'PA, g = r + B'p, K = -G^-1 F, sigma = -G^-1 g,
                          dJ += g'sigma, P <- Q + A'PA - K'GK, p <- q + A'p - K'G sigma
  tracking recursion      aux1 = R + B'PB, aux2 = B'PA, K = -inv(aux1) aux2, P <- Q + A'PA + (A'PB) K
  compute_P_inf           that map from P = Q until max|dP| < tol (iteration count, max_iter + 1 if never)
  LQ forward pass         u_s = K_s x_s, x_{s+1} = A_s x_s + B_s u_s
  total_cost              sum_t dx'Q dx + du'R du, + dx_N'Q_T dx_N
  derivatives_Cost        l, 2 Q dx, 2 R du (stage) and l_T, 2 Q_T dx (terminal)
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS64 = 2.0 ** -52
DT = 2e-2

LANES = 130          # lanes the batched generators hold (tests slice [:B])
NMAX = 9             # knots the trajectory generators hold (tests slice [:N])
NPTS = 600           # points of the point-kernel generators: three 256-thread blocks, the last one partial
TSTAGES = 12         # stages of the dense tracking stage array
# The smallest shapes that still cover a partial wavefront (63, 65), a full one (64), a second wavefront group /
# workgroup (65, 130) and the T = 1 and T = 2 loop edges (N = 2, 3).
LANE_COUNTS = (1, 63, 64, 65, 130)
KNOTS = (2, 3, 9)
RICCATI_SHAPES = [(B, T) for B in (1, 65, 130) for T in (1, 2, 8)]


# ----------------------------------------------------------------------------------------------- small algebra
def _c(a, dtype):
    return np.asarray(a, dtype=dtype)


def _t(M):
    return np.swapaxes(M, -1, -2)


def _mv(M, v):
    return (M @ v[..., None])[..., 0]


def inv2(G):
    """Inverse of (...,2,2) by the adjugate, in G's dtype."""
    det = G[..., 0, 0] * G[..., 1, 1] - G[..., 0, 1] * G[..., 1, 0]
    adj = np.stack([np.stack([G[..., 1, 1], -G[..., 0, 1]], -1), np.stack([-G[..., 1, 0], G[..., 0, 0]], -1)], -2)
    return adj / det[..., None, None]


def solve2(G, Y):
    """G^-1 Y for (...,2,2), (...,2,n) by Cramer's rule."""
    return inv2(G) @ Y


# ------------------------------------------------------------------------------------ calculate_K_and_sigma
def calculate_K_and_sigma(A, B, Q, R, S, q, r, QT, qT, dtype=LD):
    """Dense per-lane stage data (Bn,T,...), terminal (Bn,4,4) / (Bn,4) -> K (Bn,T,2,4), sigma (Bn,T,2), dJ (Bn,)
    and the boolean (Bn,T) map of the stages where |G10| > |G00| (the partial-pivoting row swap)."""
    A, B, Q, R, S, q, r, QT, qT = (_c(a, dtype) for a in (A, B, Q, R, S, q, r, QT, qT))
    Bn, T = A.shape[:2]
    P = np.broadcast_to(QT, (Bn, 4, 4)).copy()
    p = np.broadcast_to(qT, (Bn, 4)).copy()
    K = np.zeros((Bn, T, 2, 4), dtype); sig = np.zeros((Bn, T, 2), dtype); dJ = np.zeros(Bn, dtype)
    swap = np.zeros((Bn, T), bool)
    for t in range(T - 1, -1, -1):
        a, b = A[:, t], B[:, t]
        G = R[:, t] + _t(b) @ P @ b
        F = S[:, t] + _t(b) @ P @ a
        g = r[:, t] + _mv(_t(b), p)
        swap[:, t] = np.abs(G[:, 1, 0]) > np.abs(G[:, 0, 0])
        Kt = -solve2(G, F)
        st = -solve2(G, g[..., None])[..., 0]
        dJ = dJ + np.sum(g * st, axis=-1)
        P = Q[:, t] + _t(a) @ P @ a - _t(Kt) @ G @ Kt
        p = q[:, t] + _mv(_t(a), p) - _mv(_t(Kt) @ G, st)
        K[:, t] = Kt; sig[:, t] = st
    return K, sig, dJ, swap


# ------------------------------------------------------------------------------------------ tracking recursion
def riccati_step(A, B, P, Q, R):
    aux1 = R + B.T @ P @ B
    aux2 = B.T @ P @ A
    K = -inv2(aux1) @ aux2
    return K, Q + (A.T @ P @ A) + (A.T @ P @ B) @ K


def _stage(A, B, s, A_pad, B_pad, discretize, dt, dtype):
    a, b = (A[s], B[s]) if s < A.shape[0] else (A_pad, B_pad)
    if discretize:
        return np.eye(4, dtype=dtype) + _c(dt, dtype) * a, _c(dt, dtype) * b
    return a, b


def tv_lqr_gains(A, B, Q, R, QT, L, nwin=1, all_gains=True, A_pad=None, B_pad=None, discretize=False, dt=DT,
                 dtype=LD):
    """Window w: the recursion over stages w+L-2 .. w (stage index >= S reads the pad) from P = QT.
    all_gains: (L-1,2,4) of window 0; else (nwin,2,4), each window's first gain."""
    A, B, Q, R, QT = (_c(a, dtype) for a in (A, B, Q, R, QT))
    A_pad = None if A_pad is None else _c(A_pad, dtype)
    B_pad = None if B_pad is None else _c(B_pad, dtype)
    out = np.zeros(((L - 1) if all_gains else nwin, 2, 4), dtype)
    for w in range(nwin):
        P = QT
        K = None
        for s in range(L - 2, -1, -1):
            a, b = _stage(A, B, w + s, A_pad, B_pad, discretize, dt, dtype)
            K, P = riccati_step(a, b, P, Q, R)
            if all_gains:
                out[s] = K
        if not all_gains:
            out[w] = K
    return out


def compute_P_inf(A, B, Q, R, max_iter=1000, tol=1e-6, dtype=LD):
    """-> (P, iterations, gaps): iterations = the 1-based index of the first map with max|dP| < tol, max_iter + 1
    if none; gaps[n] = max|dP| - tol of map n + 1 (every map that ran)."""
    A, B, Q, R = (_c(a, dtype) for a in (A, B, Q, R))
    tol = _c(tol, dtype)
    P = Q
    gaps = []
    for i in range(max_iter):
        P_prev = P
        _, P = riccati_step(A, B, P, Q, R)
        gaps.append(np.abs(P - P_prev).max() - tol)
        if gaps[-1] < 0:
            return P, i + 1, np.array(gaps)
    return P, max_iter + 1, np.array(gaps)


def stop_margin_ulps(A, B, Q, R, max_iter=1000, tol=1e-6):
    """The stop-count margin: min |max|dP| - tol| over the stop map and the one before, in float64 ulps of max|P|."""
    P, it, gaps = compute_P_inf(A, B, Q, R, max_iter, tol)
    if it > max_iter:
        return P, it, np.inf
    last = gaps[max(it - 2, 0):it]
    return P, it, float(np.abs(last).min() / (EPS64 * np.abs(P).max()))


def lq_forward(A, B, K, x0, L, A_pad=None, B_pad=None, discretize=False, dt=DT, dtype=LD):
    A, B, K, x0 = (_c(a, dtype) for a in (A, B, K, x0))
    A_pad = None if A_pad is None else _c(A_pad, dtype)
    B_pad = None if B_pad is None else _c(B_pad, dtype)
    X = np.zeros((L, 4), dtype); U = np.zeros((L - 1, 2), dtype)
    X[0] = x0
    for s in range(L - 1):
        a, b = _stage(A, B, s, A_pad, B_pad, discretize, dt, dtype)
        U[s] = K[s] @ X[s]
        X[s + 1] = a @ X[s] + b @ U[s]
    return X, U


# -------------------------------------------------------------------------------------------------- costs
def total_cost(x, u, x_ref, u_ref, Q, R, QT, dtype=LD):
    """x (Bn,N,4), u (Bn,N-1,2), shared refs -> J (Bn,)."""
    x, u, x_ref, u_ref, Q, R, QT = (_c(a, dtype) for a in (x, u, x_ref, u_ref, Q, R, QT))
    N = x.shape[1]
    dx = x - x_ref[:N]
    du = u - u_ref[:N - 1]
    J = np.zeros(x.shape[0], dtype)
    for t in range(N - 1):
        J = J + np.sum(dx[:, t] * _mv(Q, dx[:, t]), -1)
        J = J + np.sum(du[:, t] * _mv(R, du[:, t]), -1)
    return J + np.sum(dx[:, -1] * _mv(QT, dx[:, -1]), -1)


def derivatives_cost(x, x_ref, u, u_ref, Q, R, dtype=LD):
    """Stage form on points (n,4), (n,2): l (n,), 2 Q dx (n,4), 2 R du (n,2)."""
    x, x_ref, u, u_ref, Q, R = (_c(a, dtype) for a in (x, x_ref, u, u_ref, Q, R))
    e, f = x - x_ref, u - u_ref
    return np.sum(e * _mv(Q, e), -1) + np.sum(f * _mv(R, f), -1), 2 * _mv(Q, e), 2 * _mv(R, f)


def derivatives_cost_terminal(x, x_ref, QT, dtype=LD):
    x, x_ref, QT = (_c(a, dtype) for a in (x, x_ref, QT))
    e = x - x_ref
    return np.sum(e * _mv(QT, e), -1), 2 * _mv(QT, e)


# --------------------------------------------------------------------------------------------- error measures
def chan_err(got, ref, keep=1):
    """Largest per-channel relative L2 error: the last ``keep`` axes are channels, each compared on its own norm
    over all leading axes (so channel 0 of u or row 0 of K cannot hide under channel 1's magnitude).  A channel
    whose reference is identically zero must be reproduced exactly."""
    got = np.asarray(got, LD); ref = np.asarray(ref, LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nch = int(np.prod(ref.shape[ref.ndim - keep:])) if keep else 1
    g = got.reshape(-1, nch); r = ref.reshape(-1, nch)
    num = np.sqrt(np.sum((g - r) ** 2, 0)); den = np.sqrt(np.sum(r ** 2, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
    return float(e.max())


def lane_err(got, ref):
    """Largest relative error of a per-lane scalar (J, dJ), each lane on its own magnitude."""
    got = np.asarray(got, LD); ref = np.asarray(ref, LD)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def algebra_bound(oracle_dev, existing=None):
    """The pure-algebra tolerance: 64 x the float64 yardstick's own deviation from the extended-precision result on
    the same inputs, floored at 64 x 2^-52, never looser than the bound the suite already applies (``existing``).
    A reordered float64 evaluation and the NumPy one differ from the exact result by the same order; 64 leaves room
    for FMA contraction and sum order."""
    b = 64.0 * max(float(oracle_dev), EPS64)
    return b if existing is None else min(b, existing)


# -------------------------------------------------------------------------------------------------- generators
def _spd(rng, n, shape=()):
    M = rng.normal(size=shape + (n, n))
    return M @ _t(M) + np.eye(n)


def gen_points(n=NPTS, seed=101):
    """Points as kat_primitives draws them: angles within +-pi, rates within +-8, torques within +-20 (both
    channels non-zero), with their own random references."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-np.pi, np.pi, (n, 2)), rng.uniform(-8, 8, (n, 2))], 1)
    U = rng.uniform(-20, 20, (n, 2))
    xr = rng.normal(size=(n, 4)); ur = rng.normal(size=(n, 2))
    return dict(X=X, U=U, xr=xr, ur=ur)


def gen_dense_weights(seed=102):
    """Non-symmetric dense Q, R, Q_T (SPD symmetric part, so costs stay positive): every off-diagonal term of
    e'Me and every row / column index of 2 M e matters."""
    rng = np.random.default_rng(seed)
    Q = _spd(rng, 4) + 0.3 * rng.normal(size=(4, 4))
    R = _spd(rng, 2) + 0.3 * rng.normal(size=(2, 2))
    QT = _spd(rng, 4) + 0.3 * rng.normal(size=(4, 4))
    return Q, R, QT


def gen_trajectories(seed=103):
    """Per-lane states x (LANES,NMAX,4), controls u (LANES,NMAX-1,2) with a non-zero tau1 channel, and the shared
    references x_ref (NMAX,4), u_ref (NMAX-1,2) (u_ref[:,0] non-zero too)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-np.pi, np.pi, (LANES, NMAX, 2)), rng.uniform(-8, 8, (LANES, NMAX, 2))], -1)
    u = rng.uniform(-20, 20, (LANES, NMAX - 1, 2))
    x_ref = np.concatenate([rng.uniform(-np.pi, np.pi, (NMAX, 2)), rng.uniform(-2, 2, (NMAX, 2))], -1)
    u_ref = rng.uniform(-5, 5, (NMAX - 1, 2))
    return dict(x=x, u=u, x_ref=x_ref, u_ref=u_ref)


def gen_gains(seed=104):
    """Dense per-lane K (LANES,NMAX-1,2,4) with row 0 non-zero, sigma (LANES,NMAX-1,2) with channel 0 non-zero,
    and a per-lane step size gamma (LANES,)."""
    rng = np.random.default_rng(seed)
    return dict(K=rng.normal(size=(LANES, NMAX - 1, 2, 4)), sigma=rng.normal(size=(LANES, NMAX - 1, 2)),
                gamma=rng.uniform(0.05, 1.0, LANES))


def gen_riccati(seed=105):
    """Dense per-lane stage data for calculate_K_and_sigma, LANES x NMAX stages.  R makes the pivot test of the
    2x2 solve take both branches: even lanes R ~ [[1,3],[3,12]] (|G10| > |G00|: swap), odd lanes R ~ [[4,1],[1,3]]
    (no swap), each + 0.05 randn (so R is not symmetric either); B = 0.1 randn keeps B'PB from deciding it.
    S is a full (2,4) block, Q SPD, Q_T SPD."""
    rng = np.random.default_rng(seed)
    Bn, T = LANES, NMAX
    A = np.eye(4) + 0.1 * rng.normal(size=(Bn, T, 4, 4))
    B = 0.1 * rng.normal(size=(Bn, T, 4, 2))
    Q = _spd(rng, 4, (Bn, T))
    base = np.where((np.arange(Bn) % 2 == 0)[:, None, None, None], np.array([[1.0, 3.0], [3.0, 12.0]]),
                    np.array([[4.0, 1.0], [1.0, 3.0]]))
    R = base + 0.05 * rng.normal(size=(Bn, T, 2, 2))
    S = 0.1 * rng.normal(size=(Bn, T, 2, 4))
    q = rng.normal(size=(Bn, T, 4)); r = rng.normal(size=(Bn, T, 2))
    QT = _spd(rng, 4, (Bn,)); qT = rng.normal(size=(Bn, 4))
    return dict(A=A, B=B, Q=Q, R=R, S=S, q=q, r=r, QT=QT, qT=qT)


def gen_riccati_pivot_critical(seed=110, lanes=65, T=2):
    """gen_riccati's data with a G whose pivot matters: R00 ~ 1e-9 and column 0 of B ~ 1e-6, so G00 ~ 1e-9 against
    G10 ~ 3.  With the row swap the 2x2 solve is well conditioned (cond(G) ~ 5); elimination without it has the
    multiplier G10 / G00 ~ 3e9 and loses G11 to cancellation (relative error ~1e-7).  On gen_riccati's data the
    swap only reorders a benign elimination, which the rounding-level bound rightly accepts."""
    rng = np.random.default_rng(seed)
    d = {k: (v[:lanes] if k in ("QT", "qT") else v[:lanes, :T]).copy() for k, v in gen_riccati().items()}
    d["B"][..., 0] = 1e-6 * rng.normal(size=(lanes, T, 4))
    d["R"] = np.array([[1e-9, 3.0], [3.0, 12.0]]) * (1.0 + 0.05 * rng.normal(size=(lanes, T, 2, 2)))
    return d


def riccati_args(d, B, T):
    """The first B lanes and T stages of gen_riccati's data, in riccati_general's argument order."""
    return (d["A"][:B, :T], d["B"][:B, :T], d["Q"][:B, :T], d["R"][:B, :T], d["S"][:B, :T], d["q"][:B, :T],
            d["r"][:B, :T], d["QT"][:B], d["qT"][:B])


def gen_tracking(seed=106):
    """A dense stage array for the trackers: A = I + 0.1 randn, B = 0.3 randn (both columns non-zero), TSTAGES
    stages and a dense pad stage; Q, R, Q_T symmetric positive definite and non-diagonal; one start state."""
    rng = np.random.default_rng(seed)
    A = np.eye(4) + 0.1 * rng.normal(size=(TSTAGES, 4, 4))
    B = 0.3 * rng.normal(size=(TSTAGES, 4, 2))
    A_pad = np.eye(4) + 0.1 * rng.normal(size=(4, 4))
    B_pad = 0.3 * rng.normal(size=(4, 2))
    return dict(A=A, B=B, A_pad=A_pad, B_pad=B_pad, Q=_spd(rng, 4), R=_spd(rng, 2), QT=_spd(rng, 4),
                x0=rng.normal(size=4))


def gen_dare(seed=107):
    """A dense (A, B) with SPD non-diagonal Q, R for compute_P_inf."""
    rng = np.random.default_rng(seed)
    return dict(A=np.eye(4) + 0.1 * rng.normal(size=(4, 4)), B=0.3 * rng.normal(size=(4, 2)), Q=_spd(rng, 4),
                R=_spd(rng, 2))


def slow_pair_dense():
    """test_tracking's non-converging pair (two uncontrollable, marginally stable states: P grows by Q each map,
    never within tol) with a dense R."""
    A = np.eye(4)
    A[0, 2] = A[1, 3] = 0.02
    B = np.zeros((4, 2)); B[0, 0] = B[1, 1] = 0.05
    return A, B, np.eye(4), np.array([[1.0, 0.4], [0.4, 2.0]])


def gen_mpc_weights(seed=508, scale=1e-2):
    """Symmetric non-diagonal SPD Q, R on the MPC's scale (Q_mpc = diag(120,100,1e-4,1e-4), R_mpc = diag(1e-6,10))
    times ``scale``: Q_mpc plus a PSD low-rank term, and R = [[2, 0.6], [0.6, 10]] (a well-conditioned stand-in
    for R_mpc's 1e-6).  R01 != 0 makes row 0 of every MPC gain non-zero although B_d[:, 0] = 0:
    K[0] = -(R01 / R00) K[1]."""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(4, 2))
    Q = np.diag([120.0, 100.0, 1e-4, 1e-4]) + 5.0 * (C @ C.T)
    R = np.array([[2.0, 0.6], [0.6, 10.0]])
    return scale * Q, scale * R


def gen_track(seed=109):
    """Inputs of the tracking rollout: a feed-forward trajectory x_ff (NMAX,4), u_ff (NMAX-1,2) with a non-zero
    channel 0, dense gains K (NMAX-1,2,4) with row 0 non-zero, and 65 start states around x_ff[0]."""
    rng = np.random.default_rng(seed)
    x_ff = np.concatenate([rng.uniform(-np.pi, np.pi, (NMAX, 2)), rng.uniform(-8, 8, (NMAX, 2))], -1)
    u_ff = rng.uniform(-20, 20, (NMAX - 1, 2))
    K = rng.normal(size=(NMAX - 1, 2, 4))
    x0 = x_ff[0] + rng.uniform(-0.5, 0.5, (65, 4))
    return dict(x_ff=x_ff, u_ff=u_ff, K=K, x0=x0)
