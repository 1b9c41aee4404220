"""Batched tensor-level front end of the HIP engine (device tensors in, device tensors out).

Every method is a thin launcher over one C-ABI entry point of include/gymnast_acrobot.h; the
arithmetic runs in the gfx950 kernels of csrc/: the Newton solver and its primitives in acrobot_kernels.hip
(kernels in newton_*.hpp), the trackers in tracking_kernels.hip (kernels in tracking_dense.hpp, mpc_gains.hpp,
track_rollout.hpp, mpc_box.hpp and the per-lane lqr_lanes.hpp, mpc_lanes.hpp, mpc_box_lanes.hpp).  Inputs are fp64
tensors (any device / numpy are copied to the engine's HIP device); outputs stay on the device.

Each launch fact is stated once.  AcrobotEngine._call is the one path into the library: it turns structs, tensors
and host arrays into what the ABI takes, appends the stream and checks the return code.  _buf allocates every
buffer, _workspace hands over a caller's workspace or a fresh one, and one prelude per family (_trajectory, _gains,
_stages) converts, checks and packs the shared arguments.  The ABI takes buffer sizes on trust (B, Bp, N and bare
addresses), so the preludes compare every tensor with what the kernel reads and refuse a short one on the host,
before any launch; spare trailing rows are never read and stay legal.  The argument rules are the module-level
check_* functions at the end: they need no device and no engine.

Lane-major shapes follow the reference stacked over lanes: x (B,N,4), u (B,T,2), K (B,T,2,4),
sigma (B,T,2).  Internally trajectories live in the SoA "pairs" layout (see the header).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .params import PARAM_NAMES, PARAM_SETS, DT, Q_DIAG, R_DIAG, QT_DIAG

F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def padded(B: int) -> int:
    return max(64, (B + 63) // 64 * 64)


@dataclass
class Weights:
    Q: tuple = Q_DIAG
    R: tuple = R_DIAG
    QT: tuple = QT_DIAG

    def require_gain_solvable(self):
        """Checked wherever G is inverted (the solver, the gain sweeps; cost-only paths accept any weights, as the
        reference does).  R > 0: the reference's G = R_t + B^T P B is diag(2 R0, .) with B[:, 0] = 0, and
        np.linalg.solve raises on a singular G (trajectory_generation.py:203-204); the kernels divide by 2 R0 and
        2 R1 + b^T P b.  Q, Q_T >= 0: keeps every P positive semi-definite, so G11 = 2 R1 + b^T P b >= 2 R1 > 0 and
        1/G11 is in the range the kernels' reciprocal (rcp + two Newton steps, no IEEE range scaling) covers."""
        if not all(np.isfinite(v) and v > 0 for v in self.R):
            raise ValueError(f"R must be positive (G = diag(2 R0, 2 R1 + b^T P b) is inverted), got {self.R}")
        for name, v in (("Q", self.Q), ("Q_T", self.QT)):
            if not all(np.isfinite(x) and x >= 0 for x in v):
                raise ValueError(f"{name} must be non-negative for the gain sweeps (P stays PSD), got {v}")
        return self

    def c_struct(self) -> _lib.GymWeights:
        w = _lib.GymWeights()
        w.Q[:] = [float(v) for v in self.Q]
        w.R[:] = [float(v) for v in self.R]
        w.QT[:] = [float(v) for v in self.QT]
        return w

    @staticmethod
    def from_matrices(Q, R, QT) -> "Weights":
        """Diagonal weights from the reference's matrices; raises if they are not diagonal."""
        out = []
        for name, M, n in (("Q", Q, 4), ("R", R, 2), ("Q_T", QT, 4)):
            M = np.asarray(M, dtype=float)
            if M.shape != (n, n):
                raise ValueError(f"{name} must be {n}x{n}, got {M.shape}")
            if np.any(M - np.diag(np.diag(M))):
                raise NotImplementedError(f"the fused solver kernels take diagonal {name}; use the generic path")
            out.append(tuple(np.diag(M)))
        return Weights(*out)


class PlantTables:
    """The plant tables of the per-lane trackers (AcrobotEngine's base: the engine's own attributes stay its
    launchers, one per ABI entry point with a stream; this one is a host call and an upload)."""

    def plant_table(self, plant, B: int, P: int) -> torch.Tensor:
        """The (B,P,8) float64 device table of a mismatched plant, rows in gym_model's field order (a, b, d, g1, g2,
        f1, f2, dt), that lqr_lanes_rollout / mpc_box_lanes_rollout take as ``plant``: check_plant's (B,P,11)
        parameters, reduced by gym_models_from_params with the engine's dt (row i bit for bit gym_model_from_params'),
        then one upload.  ValueError: check_plant's, and a set whose mass matrix is not positive definite."""
        par = np.ascontiguousarray(check_plant(plant, B, P, self.params).reshape(B * P, 11))
        rows = np.empty((B * P, 8))
        try:
            self._call("gym_models_from_params", par, B * P, self.dt, rows, stream=False)
        except RuntimeError as e:          # the entries are finite (check_plant), so GYM_EINVAL is the other refusal
            raise ValueError("plant: a parameter set's mass matrix is not positive definite for every theta2 (it "
                             "needs d > 0 and d (a - d) > b^2 with a = I1 + I2 + lc1^2 m1 + m2 (l1^2 + lc2^2), "
                             "b = m2 l1 lc2, d = I2 + lc2^2 m2)") from e
        return torch.as_tensor(rows.reshape(B, P, 8), device=self.device)

    def model_table(self, models, B: int) -> torch.Tensor:
        """The (B,8) float64 device table of per-lane models (BatchedNewtonSolver's ``models``, lqr_lanes_gains'
        ``models``): plant_table's call and upload with one row per lane, check_models' forms and refusals."""
        return self.plant_table(check_models(models, B, self.params), B, 1).reshape(B, 8)


    def weight_table(self, weights, B: int) -> torch.Tensor:
        """The (B,10) float64 device table of per-lane cost weights (BatchedNewtonSolver's ``weights``), rows in
        gym_weights' field order (Q[4], R[2], QT[4]): check_weights' forms and refusals, then one upload."""
        return torch.as_tensor(check_weights(weights, B, self.weights), device=self.device)


class AcrobotEngine(PlantTables):
    """Launchers for one acrobot parameter set on one HIP device."""

    def __init__(self, params=1, dt: float = DT, weights: Weights | None = None, device=None,
                 lib_path: str = _lib.LIB_PATH):
        self.device = _lib.require_device(device, lib_path)
        self.lib = _lib.load(lib_path)
        p = PARAM_SETS[params] if isinstance(params, int) else params
        self.params = dict(p)
        self.dt = float(dt)
        self.model = _lib.GymModel()
        vec = np.array([p[k] for k in ("m1", "m2", "l1", "lc1", "l2", "lc2", "I1", "I2", "g", "f1", "f2")], float)
        self._call("gym_model_from_params", vec, self.dt, self.model, stream=False)
        self.weights = weights or Weights()
        self._w = self.weights.c_struct()
        self.mpc_qt_cache = {}     # (Q, R) -> Q_T of per-lane MPC tracking; it depends on this engine's model and dt

    # -------------------------------------------------------------------------------- utils
    def _call(self, name: str, *args, stream: bool = True):
        """The one path into the library: call its entry point ``name`` and raise on a non-zero return code.  A
        ctypes struct goes by reference, a tensor as its device address, a host array as its address; None, ints,
        floats and ready-made byref out-parameters pass as they are; the engine's stream comes last unless
        ``stream`` is off.  What the library would misread is a TypeError: a tensor that is not contiguous or not
        on the engine's device, an array that is not C-contiguous float64 (an invariant of this file's own code,
        not a check of the caller's arguments)."""
        a = []
        for v in args:
            if isinstance(v, torch.Tensor):
                dev = v.device
                if not v.is_contiguous() or dev.type != self.device.type or self.device.index not in (None, dev.index):
                    raise TypeError(f"{name}: tensor {tuple(v.shape)} on {dev} is not contiguous on {self.device}")
                v = v.data_ptr()
            elif isinstance(v, np.ndarray):
                if v.dtype != np.float64 or not v.flags.c_contiguous:
                    raise TypeError(f"{name}: host array {v.shape} {v.dtype} is not C-contiguous float64")
                v = v.ctypes.data
            elif isinstance(v, C.Structure):
                v = C.byref(v)
            a.append(v)
        if stream:
            a.append(self.stream)
        _lib.check(getattr(self.lib, name)(*a), name)

    def _buf(self, *shape, dtype=F64, zero: bool = False, want: bool = True):
        """An uninitialised (``zero``: zero-filled) buffer on the engine's device; None for an optional output the
        caller does not ``want``."""
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device) if want else None

    def t(self, a, shape=None) -> torch.Tensor:
        """fp64 contiguous tensor on the engine device."""
        if isinstance(a, torch.Tensor):
            out = a.to(device=self.device, dtype=F64)
        else:
            out = torch.as_tensor(np.asarray(a, dtype=np.float64), device=self.device)
        if shape is not None:
            out = out.reshape(shape)
        return out.contiguous()

    @property
    def stream(self) -> int:
        return _lib.stream_handle(self.device)

    def set_weights(self, weights: Weights):
        w = weights.c_struct()          # first: a failure leaves the engine's weights unchanged
        self.weights, self._w = weights, w

    def pack(self, a: torch.Tensor, Bp: int, W: int = 2) -> torch.Tensor:
        """(B,L,C) lane-major -> SoA (L, C/W, Bp, W): W = 2 pairs (states, gains; wave-blocked, see the ABI header),
        W = 1 planes (controls, sigma).  The tensor shape only sizes the buffer: pair elements are laid out as
        (L, Bp/64, C/W, 64, 2)."""
        B, L, Cc = a.shape
        out = self._buf(L, Cc // W, Bp, W)
        self._call("gym_pack_lanes", a, out, B, Bp, L, Cc, W)
        return out

    def unpack(self, soa: torch.Tensor, B: int, soa1: torch.Tensor | None = None,
               sel: torch.Tensor | None = None) -> torch.Tensor:
        """SoA (L, P, Bp, W) -> lane-major (B, L, P*W); lane b reads soa1 where sel[b] != 0."""
        L, P, Bp, W = soa.shape
        check_select(soa, soa1, sel, B)
        out = self._buf(B, L, P * W)
        self._call("gym_unpack_lanes", soa, soa1, sel, out, B, Bp, L, P * W, W)
        return out

    def unpack_gains(self, K1: torch.Tensor, B: int) -> torch.Tensor:
        """The stored gain row K1 (T, 2, Bp, 2) (pairs; row 0 of every gain is zero) -> K (B,T,2,4)."""
        T, _, Bp, _ = K1.shape
        K = self._buf(B, T, 2, 4)
        self._call("gym_unpack_gains", K1, K, B, Bp, T)
        return K

    def refs(self, x_ref, u_ref, per_lane: bool = False):
        """(x_ref (N,4), u_ref (N-1,2)) on the device, u_ref trimmed / checked as newton_Algorithm does; with
        ``per_lane`` also (B,N,4) / (B,N-1 or N,2) per-lane references (the batched solver, every schedule)."""
        x_ref = self.t(x_ref)
        u_ref = self.t(u_ref)
        lane = per_lane and x_ref.ndim == 3
        if (x_ref.ndim != (3 if lane else 2)) or x_ref.shape[-1] != 4:
            raise ValueError(f"x_ref must be (N,4){' or (B,N,4)' if per_lane else ''}, got {tuple(x_ref.shape)}")
        if u_ref.ndim != x_ref.ndim or u_ref.shape[-1] != 2 or (lane and u_ref.shape[0] != x_ref.shape[0]):
            raise ValueError(f"u_ref {tuple(u_ref.shape)} does not match x_ref {tuple(x_ref.shape)}")
        if u_ref.shape[-2] == x_ref.shape[-2]:      # trajectory_generation.py:301-303
            u_ref = u_ref[..., :-1, :].contiguous()
        if u_ref.shape[-2] != x_ref.shape[-2] - 1:
            raise ValueError(f"Incompatible dimensions: x_ref has {x_ref.shape[-2]} states but u_ref has "
                             f"{u_ref.shape[-2]} controls (expected {x_ref.shape[-2] - 1})")
        return x_ref.contiguous(), u_ref.contiguous()

    # --------------------------------------------------------------------- point primitives
    def _points(self, x, u):
        x = self.t(x); u = self.t(u)
        n = x.numel() // 4
        return x.reshape(n, 4), u.reshape(n, 2), n

    def continuous_dynamics(self, x, u) -> torch.Tensor:
        x, u, n = self._points(x, u)
        out = self._buf(n, 4)
        self._call("gym_continuous_dynamics", self.model, x, u, out, n)
        return out

    def rk4(self, x, u) -> torch.Tensor:
        x, u, n = self._points(x, u)
        out = self._buf(n, 4)
        self._call("gym_rk4_step", self.model, x, u, out, n)
        return out

    def jacobians(self, x, u):
        x, u, n = self._points(x, u)
        A, Bm = self._buf(n, 4, 4), self._buf(n, 4, 2)
        self._call("gym_jacobians", self.model, x, u, A, Bm, n)
        return A, Bm

    def stage_cost_derivs(self, x, x_ref, u, u_ref, Q, R, terminal=False):
        x = self.t(x).reshape(-1, 4)
        n = x.shape[0]
        xr = check_rows(self.t(x_ref).reshape(-1, 4), n, (4,), "x_ref")
        Qm = np.ascontiguousarray(np.asarray(Q, float).reshape(4, 4))
        u_ = ur_ = Rm = None
        if not terminal:
            u_ = check_rows(self.t(u).reshape(-1, 2), n, (2,), "u")
            ur_ = check_rows(self.t(u_ref).reshape(-1, 2), n, (2,), "u_ref")
            Rm = np.ascontiguousarray(np.asarray(R, float).reshape(2, 2))
        l, gx, gu = self._buf(n), self._buf(n, 4), self._buf(n, 2, want=not terminal)
        self._call("gym_stage_cost_derivs", x, xr, u_, ur_, Qm, Rm, int(bool(terminal)), l, gx, gu, n)
        return l, gx, gu

    # ----------------------------------------------------------------- trajectory kernels
    def _trajectory(self, x, u, x_ref, u_ref, sigma=None):
        """The prelude of the trajectory methods: x (B,N,4), u (B,>=N-1,2) to the device, check_trajectory's size
        rules against the shared reference (already on the device) and ``sigma`` where passed, then x and u packed.
        Returns (xs, us, B, Bp, N)."""
        x = self.t(x); u = self.t(u)
        B, N = check_trajectory(x, u, x_ref, u_ref, sigma)
        Bp = padded(B)
        return self.pack(x, Bp), self.pack(u, Bp, W=1), B, Bp, N

    def _gains(self, K, sigma, B, Bp, N):
        """K (B,N-1,2,4) and sigma (on the device, checked by _trajectory) packed: (Ks, ss)."""
        return self.pack(self.t(K).reshape(B, N - 1, 8), Bp), self.pack(sigma, Bp, W=1)

    def rollout_open_loop(self, x0, u, x_ref, u_ref):
        """simulate_open_loop (+ total_cost): x0 (B,4), u (B,T,2) -> x (B,N,4), J (B,)."""
        x0 = self.t(x0).reshape(-1, 4)
        B = x0.shape[0]
        x_ref, u_ref = self.refs(x_ref, u_ref)
        N = x_ref.shape[0]
        u = self.t(u)
        if u.ndim == 2:
            u = u.expand(B, -1, -1).contiguous()
        if u.shape != (B, N - 1, 2):
            raise ValueError(f"u must be ({B},{N - 1},2), got {tuple(u.shape)}")
        Bp = padded(B)
        us = self.pack(u, Bp, W=1)
        xs, J = self._buf(N, 2, Bp, 2), self._buf(Bp)
        self._call("gym_rollout_open_loop", self.model, self._w, x0, us, x_ref, u_ref, xs, J, B, Bp, N)
        return self.unpack(xs, B), J[:B]

    def closed_loop(self, x, u, K, sigma, gamma, x_ref, u_ref):
        """forward_closed_loop_update (+ total_cost of the result), full gains K (B,T,2,4)."""
        sigma, gamma = self.t(sigma), self.t(gamma)
        x_ref, u_ref = self.refs(x_ref, u_ref)
        xs, us, B, Bp, N = self._trajectory(x, u, x_ref, u_ref, sigma)
        g = self._buf(Bp, zero=True)
        g[:B] = gamma.reshape(-1).expand(B) if gamma.numel() == 1 else gamma.reshape(B)
        Ks, ss = self._gains(K, sigma, B, Bp, N)
        xn, un, J = self._buf(*xs.shape), self._buf(*us.shape), self._buf(Bp)
        self._call("gym_closed_loop", self.model, self._w, xs, us, Ks, ss, g, x_ref, u_ref, xn, un, J, B, Bp, N)
        return self.unpack(xn, B), self.unpack(un, B), J[:B]

    def gamma_sweep(self, x, u, K, sigma, gammas, x_ref, u_ref) -> torch.Tensor:
        """J(gamma_g) of forward_closed_loop_update + total_cost for each lane and step size (the reference's
        Armijo line-search curve, plot_armijo_line_search :258-264): x (B,N,4), u (B,T,2), K (B,T,2,4),
        sigma (B,T,2), gammas (G,) -> (B, G)."""
        sigma = self.t(sigma)
        g = self.t(gammas).reshape(-1)
        G = int(g.numel())
        if G < 1:
            raise ValueError("gamma_sweep needs at least one step size")
        x_ref, u_ref = self.refs(x_ref, u_ref)
        xs, us, B, Bp, N = self._trajectory(x, u, x_ref, u_ref, sigma)
        Ks, ss = self._gains(K, sigma, B, Bp, N)
        J = self._buf(G, Bp)
        self._call("gym_gamma_sweep", self.model, self._w, xs, us, Ks, ss, g, G, x_ref, u_ref, J, B, Bp, N)
        return J[:, :B].t()

    def total_cost(self, x, u, x_ref, u_ref, Q, R, QT):
        x_ref = self.t(x_ref); u_ref = self.t(u_ref)
        xs, us, B, Bp, N = self._trajectory(x, u, x_ref, u_ref)
        u_ref = u_ref[: N - 1].contiguous()
        mats = [np.ascontiguousarray(np.asarray(M, float)) for M in (Q, R, QT)]
        J = self._buf(Bp)
        self._call("gym_total_cost", xs, us, x_ref, u_ref, *mats, J, B, Bp, N)
        return J[:B]

    def backward(self, x, u, x_ref, u_ref, want_lambda=False, check_gains=True):
        """Fused costate + stage lists + Riccati: K (B,T,2,4), sigma (B,T,2), dJ (B,), max|sigma| (B,), lambda.
        ``check_gains=False``: the caller uses only lambda (compute_costate_trajectory), which needs no G^-1."""
        if check_gains:
            self.weights.require_gain_solvable()
        x_ref, u_ref = self.refs(x_ref, u_ref)
        xs, us, B, Bp, N = self._trajectory(x, u, x_ref, u_ref)
        T = N - 1
        K1, sg, dJ, sm = self._buf(T, 2, Bp, 2), self._buf(T, 2, Bp, 1), self._buf(Bp), self._buf(Bp)
        lam = self._buf(N, 2, Bp, 2, want=want_lambda)
        self._call("gym_backward_sweep", self.model, self._w, xs, us, x_ref, u_ref, K1, sg, dJ, sm, lam, B, Bp, N)
        return (self.unpack_gains(K1, B), self.unpack(sg, B), dJ[:B], sm[:B],
                self.unpack(lam, B) if want_lambda else None)

    def linearize(self, x, u, x_ref, u_ref, method: str = "euler"):
        """build_stage_lists: A_d (B,T,4,4), B_d (B,T,4,2), q (B,T,4), r (B,T,2), q_T (B,4).  ``method``: "euler", the
        reference's A_d = I + dt A_c, or "rk4", the exact Jacobians of the RK4 step (gym_linearize_rk4)."""
        if method not in ("euler", "rk4"):
            raise ValueError(f'method must be "euler" or "rk4", got {method!r}')
        x_ref, u_ref = self.refs(x_ref, u_ref)
        xs, us, B, Bp, N = self._trajectory(x, u, x_ref, u_ref)
        T = N - 1
        Ad, Bd, q, r = self._buf(T, 16, Bp), self._buf(T, 8, Bp), self._buf(T, 4, Bp), self._buf(T, 2, Bp)
        qT = self._buf(4, Bp)
        self._call("gym_linearize_rk4" if method == "rk4" else "gym_linearize", self.model, self._w, xs, us, x_ref,
                   u_ref, Ad, Bd, q, r, qT, B, Bp, N)
        lm = lambda a, *s: a[..., :B].permute(-1, *range(a.ndim - 1)).reshape(B, *s)  # noqa: E731
        return lm(Ad, T, 4, 4), lm(Bd, T, 4, 2), lm(q, T, 4), lm(r, T, 2), lm(qT, 4)

    def riccati_general(self, A, Bm, Q, R, S, q, r, QT, qT):
        """calculate_K_and_sigma on dense per-lane stage data (lane-major, broadcastable over lanes/time)."""
        A = self.t(A)
        B, T = A.shape[:2]
        Bp = padded(B)

        def soa(a, shape_tail):  # (B,T,*tail) or broadcastable -> (T, prod(tail), Bp)
            a = self.t(a).expand(B, T, *shape_tail) if a is not None else None
            n = int(np.prod(shape_tail))
            out = self._buf(T, n, Bp, zero=True)
            out[:, :, :B] = a.reshape(B, T, n).permute(1, 2, 0)
            return out

        def soa_t(a, shape_tail):
            a = self.t(a).expand(B, *shape_tail)
            n = int(np.prod(shape_tail))
            out = self._buf(n, Bp, zero=True)
            out[:, :B] = a.reshape(B, n).T
            return out

        As, Bs, Qs, Rs, Ss = soa(A, (4, 4)), soa(Bm, (4, 2)), soa(Q, (4, 4)), soa(R, (2, 2)), soa(S, (2, 4))
        qs, rs, QTs, qTs = soa(q, (4,)), soa(r, (2,)), soa_t(QT, (4, 4)), soa_t(qT, (4,))
        K, sg, dJ = self._buf(T, 8, Bp), self._buf(T, 2, Bp), self._buf(Bp)
        self._call("gym_riccati_general", As, Bs, Qs, Rs, Ss, qs, rs, QTs, qTs, K, sg, dJ, B, Bp, T)
        return (K[..., :B].permute(2, 0, 1).reshape(B, T, 2, 4), sg[..., :B].permute(2, 0, 1).contiguous(),
                dJ[:B])

    # ------------------------------------------------------------------ LQR / MPC trackers
    def _stages(self, A, Bm, A_pad, B_pad):
        """The stage arrays of tv_lqr_gains / lq_forward on the device: A (S,4,4), Bm (>=S,4,2) and the optional
        pad pair (None where not given)."""
        A = self.t(A).reshape(-1, 4, 4)
        Bm = check_rows(self.t(Bm).reshape(-1, 4, 2), A.shape[0], (4, 2), "Bm")
        return (A, Bm, None if A_pad is None else self.t(A_pad).reshape(4, 4),
                None if B_pad is None else self.t(B_pad).reshape(4, 2))

    def tv_lqr_gains(self, A, Bm, Q, R, QT, L: int, nwin: int = 1, all_gains: bool = True, A_pad=None,
                     B_pad=None, discretize: bool = False) -> torch.Tensor:
        """Windowed time-varying LQR gains (gym_tv_lqr_gains): stages A (S,4,4), B (S,4,2) on the device.
        all_gains: (L-1,2,4) gains of window 0; else (nwin,2,4) first gains of windows 0..nwin-1."""
        A, Bm, Ap, Bp_ = self._stages(A, Bm, A_pad, B_pad)
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        QTd = self.t(QT).reshape(4, 4)                 # device: e.g. dare_fixed_point's P, no host round trip
        out = self._buf((L - 1) if all_gains else nwin, 2, 4)
        self._call("gym_tv_lqr_gains", A, Bm, A.shape[0], Ap, Bp_, Qh, Rh, QTd, int(L), int(nwin),
                   int(bool(all_gains)), int(bool(discretize)), self.dt, out)
        return out

    def dare_fixed_point(self, A, Bm, Q, R, max_iter: int = 1000, tol: float = 1e-6):
        """compute_P_inf on the device: returns (P (4,4), iterations (1,) int32), both device tensors (no sync)."""
        A = self.t(A).reshape(4, 4); Bm = self.t(Bm).reshape(4, 2)
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        P, it = self._buf(4, 4), self._buf(1, dtype=I32, zero=True)
        self._call("gym_dare_fixed_point", A, Bm, Qh, Rh, int(max_iter), float(tol), P, it)
        return P, it

    def _mpc_gains(self, every, x_ref, u_ref, x_f, u_f, Q, R, L, nwin, max_iter, tol):
        """gym_mpc_gains_all (``every`` gain of every window) or gym_mpc_gains (each window's first gain)."""
        x_ref = self.t(x_ref).reshape(-1, 4); u_ref = self.t(u_ref).reshape(-1, 2)
        x_f = self.t(x_f).reshape(4); u_f = self.t(u_f).reshape(2)
        S = x_ref.shape[0] - 1
        if u_ref.shape[0] < S:
            raise ValueError(f"u_ref must hold {S} stages, got {u_ref.shape[0]}")
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        K = self._buf(nwin, int(L) - 1, 2, 4) if every else self._buf(nwin, 2, 4)
        P, it = self._buf(4, 4), self._buf(1, dtype=I32, zero=True)
        self._call("gym_mpc_gains_all" if every else "gym_mpc_gains", self.model, x_ref, u_ref, S, x_f, u_f, Qh, Rh,
                   int(L), int(nwin), int(max_iter), float(tol), K, P, it)
        return K, P, it

    def mpc_gains(self, x_ref, u_ref, x_f, u_f, Q, R, L: int, nwin: int, max_iter: int = 1000, tol: float = 1e-6):
        """Fused MPC gains (gym_mpc_gains): stage linearisations of (x_ref, u_ref) and of the pad (x_f, u_f),
        Q_T = compute_P_inf(A_f, B_f, Q, R), and each window's first gain.  Returns device tensors
        (K0 (nwin,2,4), Q_T (4,4), iterations (1,) int32); no host synchronisation."""
        return self._mpc_gains(False, x_ref, u_ref, x_f, u_f, Q, R, L, nwin, max_iter, tol)

    def mpc_gains_all(self, x_ref, u_ref, x_f, u_f, Q, R, L: int, nwin: int, max_iter: int = 1000,
                      tol: float = 1e-6):
        """gym_mpc_gains_all: mpc_gains with every stage's gain of every window.  Returns device tensors
        (K_all (nwin,L-1,2,4), Q_T (4,4), iterations (1,) int32); K_all[:, 0] is mpc_gains' K0 bit for bit."""
        return self._mpc_gains(True, x_ref, u_ref, x_f, u_f, Q, R, L, nwin, max_iter, tol)

    def lq_forward(self, A, Bm, K, x0, L: int, A_pad=None, B_pad=None, discretize: bool = False):
        """One window's LQ forward pass: X (L,4), U (L-1,2)."""
        A, Bm, Ap, Bp_ = self._stages(A, Bm, A_pad, B_pad)
        K = check_rows(self.t(K).reshape(-1, 2, 4), int(L) - 1, (2, 4), "K")
        x0 = self.t(x0).reshape(4)
        X, U = self._buf(L, 4), self._buf(L - 1, 2)
        self._call("gym_lq_forward", A, Bm, A.shape[0], Ap, Bp_, int(bool(discretize)), self.dt, K, x0, int(L), X, U)
        return X, U

    def track_rollout(self, x0, x_ff, u_ff, K, single: bool = False):
        """Batched closed-loop tracking: x0 (B,4) -> x (B,N,4), u (B,T,2) under the shared (x_ff, u_ff, K).
        single: one lane per trajectory instead of a lane pair (bit-identical; measurement / tests)."""
        x0 = self.t(x0).reshape(-1, 4)
        x_ff = self.t(x_ff).reshape(-1, 4); u_ff = self.t(u_ff).reshape(-1, 2); K = self.t(K).reshape(-1, 2, 4)
        N = x_ff.shape[0]
        if u_ff.shape[0] != N - 1 or K.shape[0] != N - 1:
            raise ValueError(f"feed-forward / gains must hold {N - 1} stages, got {u_ff.shape[0]} / {K.shape[0]}")
        B = x0.shape[0]
        x, u = self._buf(B, N, 4), self._buf(B, N - 1, 2)
        self._call("gym_track_rollout_ex", self.model, x0, x_ff, u_ff, K, B, N, _lib.TRACK_SINGLE if single else 0,
                   x, u)
        return x, u

    # ------------------------------------------------------------- caller-owned workspaces
    def _ws_bytes(self, name: str, *sizes) -> int:
        """What the workspace-size entry point ``name`` answers for ``sizes``."""
        need = C.c_int64()
        self._call(name, *(int(v) for v in sizes), C.byref(need), stream=False)
        return need.value

    def _workspace(self, ws, name: str | None = None, *sizes, holds: str | None = None):
        """The caller's workspace ``ws``, or a fresh one of the size the entry point ``name`` answers for ``sizes``
        (no ``name``: the workspace carries an earlier call's results, so the caller must give it), and its byte
        count: (ws, bytes).  The library refuses a short workspace; with ``holds`` (what it is to hold) the host
        does, before the launch."""
        if ws is None and name is None:
            raise TypeError("this call needs the workspace an earlier call filled")
        need = self._ws_bytes(name, *sizes) if ws is None or holds else None
        if ws is None:
            ws = self._buf(need, dtype=U8)
        ws_bytes = ws.numel() * ws.element_size()
        if holds and ws_bytes < need:
            raise ValueError(f"the workspace holds {ws_bytes} bytes, {holds} need {need}")
        return ws, ws_bytes

    # ------------------------------------------------------------- torque-limited MPC (box QP)
    def mpc_box_workspace(self, B: int, L: int, rows: int) -> torch.Tensor:
        """The caller-owned workspace of gym_mpc_box_qp (rows = stages given) / gym_mpc_box_rollout (rows = N)."""
        return self._workspace(None, "gym_mpc_box_workspace", B, L, rows)[0]

    def mpc_box_qp(self, A, Bm, u_ref, Q, R, QT, x0, L: int, tau_max: float, max_qp_iters: int = 32, ws=None,
                   fallback_iters: int = 0):
        """gym_mpc_box_qp: the torque-limited QP of one window for a batch x0 (B,4).  Stages A (S,4,4), Bm (S,4,2),
        u_ref (S,2) are host arrays (S >= L-1).  Returns device tensors U (B,L-1,2), X (B,L,4), iterations (B,)
        int32, converged (B,) int32.  ``fallback_iters`` > 0 (gym_mpc_box_qp_fallback): a QP at the cap goes on by
        projected Newton for at most that many iterations; iterations then counts both phases (> max_qp_iters
        exactly when the fallback ran) and converged is false only where neither phase finished."""
        fb = check_fallback(fallback_iters)
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64)).reshape(-1, 4, 4)
        Bm = np.ascontiguousarray(np.asarray(Bm, dtype=np.float64)).reshape(-1, 4, 2)
        ur = np.ascontiguousarray(np.asarray(u_ref, dtype=np.float64)).reshape(-1, 2)
        S, L = A.shape[0], int(L)
        if Bm.shape[0] != S or ur.shape[0] < S or S < L - 1:
            raise ValueError(f"a window of {L} stages needs {L - 1} rows of A, B and u_ref, got {S} / {Bm.shape[0]} / "
                             f"{ur.shape[0]}")
        ur = np.ascontiguousarray(ur[:S])
        if np.any(Bm[:, :, 0] != 0.0):
            raise ValueError("the torque-limited QP needs B[:, 0] = 0 at every stage (channel 0 must separate)")
        Qh, Rh = host_mat(Q, 4, "Q"), check_diagonal_R(R, "the torque-limited QP")
        QTd = self.t(QT).reshape(4, 4)
        x0 = self.t(x0).reshape(-1, 4)
        B = x0.shape[0]
        ws, ws_bytes = self._workspace(ws, "gym_mpc_box_workspace", B, L, S)
        U, X = self._buf(B, L - 1, 2), self._buf(B, L, 4)
        it, conv = self._buf(B, dtype=I32), self._buf(B, dtype=I32)
        self._call(*_with_fallback("gym_mpc_box_qp", fb, A, Bm, ur, S, Qh, Rh, QTd, x0, B, L, float(tau_max),
                                   int(max_qp_iters)), ws, ws_bytes, U, X, it, conv)
        return U, X, it, conv

    def mpc_box_rollout(self, x0, x_ref, u_ref, x_f, u_f, Q, R, QT, K_all, tau_max: float, max_qp_iters: int = 32,
                        ws=None, fallback_iters: int = 0):
        """gym_mpc_box_rollout: the torque-limited closed loop of B lanes.  Returns device tensors x (B,N,4),
        u (B,N-1,2), qp_iters (B,N-1) int32, unconverged (B,) int32.  ``fallback_iters`` > 0
        (gym_mpc_box_rollout_fallback): qp_iters counts active-set sweeps plus Newton iterations and unconverged only
        the QPs that neither phase finished."""
        fb = check_fallback(fallback_iters)
        x0 = self.t(x0).reshape(-1, 4)
        x_ref = self.t(x_ref).reshape(-1, 4); u_ref = self.t(u_ref).reshape(-1, 2)
        x_f = self.t(x_f).reshape(4); u_f = self.t(u_f).reshape(2)
        QTd = self.t(QT).reshape(4, 4)
        N = x_ref.shape[0]
        K_all = self.t(K_all)
        if K_all.ndim != 4 or K_all.shape[0] != N - 1 or K_all.shape[2:] != (2, 4):
            raise ValueError(f"K_all must be ({N - 1}, L-1, 2, 4), got {tuple(K_all.shape)}")
        if u_ref.shape[0] < N - 1:
            raise ValueError(f"u_ref must hold {N - 1} stages, got {u_ref.shape[0]}")
        L = K_all.shape[1] + 1
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        B = x0.shape[0]
        ws, ws_bytes = self._workspace(ws, "gym_mpc_box_workspace", B, L, N)
        x, u = self._buf(B, N, 4), self._buf(B, N - 1, 2)
        it, unconv = self._buf(B, N - 1, dtype=I32), self._buf(B, dtype=I32)
        self._call(*_with_fallback("gym_mpc_box_rollout", fb, self.model, x0, x_ref, u_ref, x_f, u_f, Qh, Rh, QTd,
                                   K_all, B, N, L, float(tau_max), int(max_qp_iters)), ws, ws_bytes, x, u, it, unconv)
        return x, u, it, unconv

    # ------------------------------------------------------------- per-lane LQR tracking
    def lqr_lanes_workspace(self, B: int, N: int) -> torch.Tensor:
        """The caller-owned workspace of gym_lqr_lanes_gains / gym_lqr_lanes_rollout for B lanes of N knots."""
        return self._workspace(None, "gym_lqr_lanes_workspace", B, N)[0]

    def lqr_lanes_gains(self, x_opt, u_opt, Q, R, QT, gains: bool = True, ws=None, models=None):
        """gym_lqr_lanes_gains: solve_LQR_tracking per lane along x_opt (B,N,4), u_opt (B,N-1,2).  Returns (ws, K):
        the filled workspace lqr_lanes_rollout takes, and K (B,N-1,2,4) on the device (None unless ``gains``).
        ``models``: a model_table (B,8); lane b is then linearised on its own row (gym_lqr_lanes_gains_models)."""
        x_opt = self.t(x_opt); u_opt = self.t(u_opt)
        B, N = check_lane_trajectories(x_opt, u_opt)
        Rh = check_diagonal_R(R, "per-lane LQR tracking")
        Qh, QTh = check_sym_weight(Q, "Q"), check_sym_weight(QT, "QT")
        ws, ws_bytes = self._workspace(ws, "gym_lqr_lanes_workspace", B, N)
        K = self._buf(B, N - 1, 2, 4, want=gains)
        if models is None:
            self._call("gym_lqr_lanes_gains", self.model, x_opt, u_opt, B, N, Qh, Rh, QTh, ws, ws_bytes, K)
        else:
            check_model_table(models, B)
            self._call("gym_lqr_lanes_gains_models", self.model, models, x_opt, u_opt, B, N, Qh, Rh, QTh, ws, ws_bytes,
                       K)
        return ws, K

    def lqr_lanes_rollout(self, ws, x0, N: int, trajectories: bool = True, plant=None):
        """gym_lqr_lanes_rollout on a workspace lqr_lanes_gains filled: x0 (B,P,4) -> (x (B,P,N,4), u (B,P,N-1,2),
        summary (3,B,P) = err_final, err_max, u_max) on the device; x, u are None unless ``trajectories``.
        ``plant``: a plant_table (B,P,8); closed loop (b, p) then integrates its own plant
        (gym_lqr_lanes_rollout_plant), the controller staying on this engine's model."""
        x0 = self.t(x0)
        check_lane_starts(x0)
        B, P, N = x0.shape[0], x0.shape[1], int(N)
        ws, ws_bytes = self._workspace(ws)
        if plant is not None:
            check_plant_table(plant, B, P)
        x, u = self._buf(B, P, N, 4, want=trajectories), self._buf(B, P, N - 1, 2, want=trajectories)
        summary = self._buf(3, B, P)
        if plant is None:
            self._call("gym_lqr_lanes_rollout", self.model, x0, B, P, N, ws, ws_bytes, x, u, summary)
        else:
            self._call("gym_lqr_lanes_rollout_plant", self.model, plant, x0, B, P, N, ws, ws_bytes, x, u, summary)
        return x, u, summary

    # ------------------------------------------------------------- per-lane MPC tracking
    def mpc_lanes_gains(self, x_opt, u_opt, Q, R, QT, L: int, gains: bool = True, ws=None):
        """gym_mpc_lanes_gains: the first gain of every MPC window (L = T_pred stages) of every lane along x_opt
        (B,N,4), u_opt (B,N-1,2).  QT (4,4) is a device tensor (mpc_gains' Q_T; a host array is copied once), never
        read back.  Returns (ws, K): the filled lqr_lanes_workspace lqr_lanes_rollout takes, and K0 (B,N-1,2,4) on the
        device (None unless ``gains``)."""
        x_opt = self.t(x_opt); u_opt = self.t(u_opt)
        B, N = check_lane_trajectories(x_opt, u_opt)
        L = check_window(L, "per-lane MPC tracking")
        Rh = check_diagonal_R(R, "per-lane MPC tracking")
        Qh = check_sym_weight(Q, "Q")
        QTd = check_device_QT(self.t(QT))
        ws, ws_bytes = self._workspace(ws, "gym_lqr_lanes_workspace", B, N, holds=f"{B} lanes of {N} knots")
        K = self._buf(B, N - 1, 2, 4, want=gains)
        self._call("gym_mpc_lanes_gains", self.model, x_opt, u_opt, B, N, L, Qh, Rh, QTd, ws, ws_bytes, K)
        return ws, K

    # ------------------------------------------------------------- per-lane torque-limited MPC tracking
    BOX_LANES_WS_SHARE = 0.5    # mpc_box_lanes_rollout's own workspace: at most this share of the free device memory

    def mpc_box_lanes_workspace(self, B: int, P: int, L: int) -> int:
        """Bytes of gym_mpc_box_lanes_rollout's caller-owned workspace for B lanes x P starts, windows of L stages."""
        return self._ws_bytes("gym_mpc_box_lanes_workspace", B, P, L)

    def mpc_box_lanes_rollout(self, x_opt, u_opt, x0, Q, R, QT, L: int, tau_max: float, max_qp_iters: int = 32,
                              trajectories: bool = True, max_ws_bytes: int | None = None, plant=None,
                              fallback_iters: int = 0):
        """gym_mpc_box_lanes_rollout: the torque-limited MPC closed loop of every lane along its own x_opt (B,N,4),
        u_opt (B,N-1,2) from the starts x0 (B,P,4); QT (4,4) a device tensor as in mpc_lanes_gains.  Returns device
        tensors (x (B,P,N,4), u (B,P,N-1,2), summary (3,B,P), qp_iters (B,P,N-1) int32, unconverged (B,P) int32); x, u
        and qp_iters are None unless ``trajectories``.  The sweep workspace (about 80 (L-1) bytes per lane and start) is
        allocated here; a batch whose workspace would exceed ``max_ws_bytes`` (default: BOX_LANES_WS_SHARE of the free
        device memory) runs in chunks of whole lanes, one call each -- the same results, lanes being independent.
        ``fallback_iters`` > 0 (gym_mpc_box_lanes_rollout_fallback, every chunk): qp_iters counts active-set sweeps
        plus Newton iterations and unconverged only the QPs that neither phase finished.  ``plant``: a plant_table
        (B,P,8); closed loop (b, p) then integrates its own plant (gym_mpc_box_lanes_rollout_plant, with or without
        the fallback; the table is sliced with the other lane-major buffers), the controller staying on this engine's
        model."""
        x_opt = self.t(x_opt); u_opt = self.t(u_opt); x0 = self.t(x0)
        B, N = check_lane_trajectories(x_opt, u_opt)
        check_lane_starts(x0, B)
        P, L = x0.shape[1], check_window(L, "the torque-limited QP")
        if B * P > _lib.MAX_BP:
            raise ValueError(f"{B} lanes x {P} starts exceed {_lib.MAX_BP} closed loops per call")
        if plant is not None:
            check_plant_table(plant, B, P)
        check_box(tau_max, max_qp_iters, fallback_iters)
        fb = int(fallback_iters)
        Rh = check_diagonal_R(R, "the torque-limited QP")
        Qh = check_sym_weight(Q, "Q")
        QTd = check_device_QT(self.t(QT))
        per_lane = self.mpc_box_lanes_workspace(1, P, L)
        if max_ws_bytes is None:
            max_ws_bytes = int(self.BOX_LANES_WS_SHARE * torch.cuda.mem_get_info(self.device)[0])
        chunk = max(1, min(B, int(max_ws_bytes) // per_lane))
        ws = self._buf(chunk * per_lane, dtype=U8)
        x, u = self._buf(B, P, N, 4, want=trajectories), self._buf(B, P, N - 1, 2, want=trajectories)
        it = self._buf(B, P, N - 1, dtype=I32, want=trajectories)
        summary, unconv = self._buf(3, B, P), self._buf(B, P, dtype=I32)
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            part = lambda a: None if a is None else a[b0:b1]  # noqa: E731 -- this chunk's lanes of a lane-major buffer
            sm = summary if chunk >= B else self._buf(3, b1 - b0, P)
            sizes = (b1 - b0, P, N, L, Qh, Rh, QTd, float(tau_max), int(max_qp_iters))
            if plant is None:
                head = _with_fallback("gym_mpc_box_lanes_rollout", fb, self.model, part(x_opt), part(u_opt), part(x0),
                                      *sizes)
            else:                                      # one entry point for both: fallback_iters 0 = the active set
                head = ("gym_mpc_box_lanes_rollout_plant", self.model, part(plant), part(x_opt), part(u_opt), part(x0),
                        *sizes, fb)
            self._call(*head, ws, ws.numel(), part(x), part(u), sm, part(it), part(unconv))
            if sm is not summary:
                summary[:, b0:b1] = sm
        return x, u, summary, it, unconv


# ------------------------------------------------------------------------------------- argument checks
# Plain functions of shapes and host values (torch tensors and numpy arrays alike): no device, no engine, so the
# front end (trajectory_tracking.py) refuses a bad call with the same words before it asks for either.  The size rules
# (check_rows, check_trajectory, check_select) ask for at least what the kernel reads: the ABI is given B, Bp, N and
# bare addresses, so a short buffer would be read past its end; spare trailing rows are never read and pass.
def host_mat(M, n, name):
    M = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    if M.shape != (n, n):
        raise ValueError(f"{name} must be {n}x{n}, got {M.shape}")
    return M


def check_rows(a, n: int, tail: tuple, name: str):
    """``a`` (the argument ``name``) holds at least the n rows of shape ``tail`` a kernel reads.  Returns a."""
    if tuple(a.shape[1:]) != tuple(tail) or a.shape[0] < n:
        raise ValueError(f"{name} must be (>={n},{','.join(str(v) for v in tail)}), got {tuple(a.shape)}")
    return a


def check_trajectory(x, u, x_ref, u_ref, sigma=None):
    """Lane trajectories under a shared reference, as the trajectory kernels read them for (B, N): x (B,N,4) with
    N >= 2, u -- and sigma where passed -- (B,>=N-1,2), x_ref (>=N,4), u_ref (>=N-1,2).  Returns (B, N)."""
    if x.ndim != 3 or x.shape[2] != 4 or x.shape[1] < 2:
        raise ValueError(f"x must be (B,N,4) with N >= 2, got {tuple(x.shape)}")
    B, N = x.shape[0], x.shape[1]
    for name, a in (("u", u), ("sigma", sigma)):
        if a is not None and (a.ndim != 3 or a.shape[0] != B or a.shape[1] < N - 1 or a.shape[2] != 2):
            raise ValueError(f"{name} must be ({B},>={N - 1},2) for x {tuple(x.shape)}, got {tuple(a.shape)}")
    check_rows(x_ref, N, (4,), "x_ref")
    check_rows(u_ref, N - 1, (2,), "u_ref")
    return B, N


def check_select(soa, soa1, sel, B: int):
    """unpack's per-lane select: soa1 shaped like soa, sel int32 with an entry for each of the B lanes."""
    if soa1 is not None and tuple(soa1.shape) != tuple(soa.shape):
        raise ValueError(f"soa1 must be {tuple(soa.shape)} like soa, got {tuple(soa1.shape)}")
    if sel is not None and (sel.dtype != torch.int32 or sel.ndim != 1 or sel.shape[0] < B):
        raise ValueError(f"sel must be int32 (>={B},), got {sel.dtype} {tuple(sel.shape)}")


def check_lane_trajectories(x_opt, u_opt, or_n_rows: bool = False):
    """Per-lane trajectories x_opt (B,N,4) with N >= 2 and u_opt (B,N-1,2); ``or_n_rows``: u_opt may hold N rows (the
    caller trims the last, as newton_Algorithm trims u_ref).  Returns (B, N)."""
    if x_opt.ndim != 3 or x_opt.shape[2] != 4 or x_opt.shape[1] < 2:
        raise ValueError(f"x_opt must be (B,N,4) with N >= 2, got {tuple(x_opt.shape)}")
    B, N = x_opt.shape[0], x_opt.shape[1]
    if tuple(u_opt.shape) != (B, N - 1, 2) and not (or_n_rows and tuple(u_opt.shape) == (B, N, 2)):
        raise ValueError(f"u_opt must be ({B},{N - 1},2){f' (or {N} rows)' if or_n_rows else ''} for x_opt "
                         f"{tuple(x_opt.shape)}, got {tuple(u_opt.shape)}")
    return B, N


def check_lane_starts(x0, B: int | None = None, flat_ok: bool = False):
    """Per-lane starts x0 (B,P,4) with P >= 1, for ``B`` lanes where it is given; ``flat_ok``: (B,4) passes too (the
    caller adds the P axis)."""
    lead = "B" if B is None else B
    if not (x0.ndim == 3 and x0.shape[1] >= 1 or flat_ok and x0.ndim == 2) or x0.shape[-1] != 4 or (
            x0.shape[0] < 1 if B is None else x0.shape[0] != B):
        raise ValueError(f"x0 must be {f'({lead},4) or ' if flat_ok else ''}({lead},P,4), got {tuple(x0.shape)}")


def check_diagonal_R(R, what: str) -> np.ndarray:
    """The host R (2,2) of a tracker that splits the channels (``what`` names it): diagonal, R[1][1] finite and > 0."""
    Rh = host_mat(R, 2, "R")
    if Rh[0, 1] != 0.0 or Rh[1, 0] != 0.0 or not (np.isfinite(Rh[1, 1]) and Rh[1, 1] > 0):
        raise ValueError(f"{what} needs a diagonal R with R[1][1] > 0, got {Rh.tolist()}")
    return Rh


def check_sym_weight(M, name: str) -> np.ndarray:
    """The host weight ``name`` (4,4) of a per-lane tracker (their recursions keep the upper triangle only)."""
    Mh = host_mat(M, 4, name)
    if not np.array_equal(Mh, Mh.T):
        raise ValueError(f"{name} must be symmetric, got {Mh.tolist()}")
    return Mh


def check_window(T_pred, what: str) -> int:
    """The MPC window of the fused kernels (``what`` names the caller): T_pred + 2 stages fit one LDS table."""
    L = int(T_pred)
    if L < 2 or L + 2 > _lib.MPC_MAX_STAGES:
        raise ValueError(f"T_pred must be in [2, {_lib.MPC_MAX_STAGES - 2}] for {what}, got {L}")
    return L


def check_box(tau_max, max_qp_iters, fallback_iters=0):
    """The torque limit, the active set's sweep cap and the fallback's iteration cap (0: no fallback)."""
    if not (np.isfinite(tau_max) and tau_max > 0):
        raise ValueError(f"tau_max must be finite and positive, got {tau_max}")
    if int(max_qp_iters) < 1:
        raise ValueError(f"max_qp_iters must be at least 1, got {max_qp_iters}")
    check_fallback(fallback_iters)


def check_fallback(fallback_iters) -> int:
    """The projected-Newton fallback's iteration cap, returned as an int: a whole number, 0 = off."""
    fb = int(fallback_iters)
    if fb != fallback_iters or fb < 0 or fb > 2 ** 31 - 1:
        raise ValueError(f"fallback_iters must be a whole number in [0, 2^31), got {fallback_iters}")
    return fb


def _with_fallback(name, fb, *head):
    """The call list up to max_qp_iters: the entry point itself, or with fb > 0 its ..._fallback twin, which takes
    fallback_iters right after max_qp_iters."""
    return (name + "_fallback",) + head + (fb,) if fb else (name,) + head


def check_plant(plant, B: int, P: int, own_params) -> np.ndarray:
    """The parameters of every closed loop's plant, (B,P,11) float64 in params.PARAM_NAMES order, from any of
      * a set number 1-3 (params.PARAM_SETS);
      * a dict of parameter names to scalars or arrays broadcastable to (B,P); names it leaves out are taken from
        ``own_params`` (the engine's own set), so {} is the design model itself;
      * an array (11,), (P,11) per start, (B,11) or (B,1,11) per lane, or (B,P,11).  NumPy's broadcasting reads a
        2-D array as per start, so (n,11) is per lane only where n = B != P (always with an x0 that came as (B,4),
        where P is 1); (B,1,11) says per lane for any P.
    ValueError, in these words: "unknown plant parameter" for a name not in PARAM_NAMES, "plant set" for a number
    that is no set, "plant rows must hold 11 parameters" for a wrong trailing size, "does not broadcast" for a shape
    that fits none of the forms, "must be finite" for a NaN or inf anywhere."""
    B, P = int(B), int(P)
    if isinstance(plant, (int, np.integer)) and not isinstance(plant, bool):
        if int(plant) not in PARAM_SETS:
            raise ValueError(f"plant set must be one of {sorted(PARAM_SETS)}, got {plant}")
        plant = dict(PARAM_SETS[int(plant)])
    if isinstance(plant, dict):
        unknown = [k for k in plant if k not in PARAM_NAMES]
        if unknown:
            raise ValueError(f"unknown plant parameter {unknown[0]!r}: the names are {', '.join(PARAM_NAMES)}")
        out = np.empty((B, P, 11))
        for j, name in enumerate(PARAM_NAMES):
            v = np.asarray(plant.get(name, own_params[name]), dtype=np.float64)
            try:
                out[:, :, j] = np.broadcast_to(v, (B, P))
            except ValueError:
                raise ValueError(f"plant[{name!r}] {v.shape} does not broadcast to ({B},{P})") from None
    else:
        a = np.asarray(plant.detach().cpu() if isinstance(plant, torch.Tensor) else plant, dtype=np.float64)
        if a.ndim < 1 or a.shape[-1] != 11:
            raise ValueError(f"plant rows must hold 11 parameters ({', '.join(PARAM_NAMES)}), got {a.shape}")
        if a.ndim == 2 and a.shape[0] == B != P:
            a = a[:, None, :]                          # (B,11): per lane
        try:
            out = np.broadcast_to(a, (B, P, 11))
        except ValueError:
            raise ValueError(f"plant {a.shape} does not broadcast to ({B},{P},11): give (11,), ({P},11), ({B},11), "
                             f"({B},1,11) or ({B},{P},11)") from None
    if not np.isfinite(out).all():
        raise ValueError("plant parameters must be finite")
    return out


def check_models(models, B: int, own_params) -> np.ndarray:
    """The parameters of every lane's own model, (B,11) float64 in params.PARAM_NAMES order: check_plant with one plant
    per lane (P = 1), so a set number, a dict of names to scalars or (B,) arrays, (11,), (B,11) or (B,1,11) such as
    sample_plants(B, 1), with check_plant's refusals in its words."""
    if isinstance(models, dict):       # (B,) arrays are per lane: one column of the (B,1) check_plant broadcasts to
        models = {k: (np.asarray(v, dtype=np.float64).reshape(-1, 1) if np.ndim(v) == 1 and k in PARAM_NAMES else v)
                  for k, v in models.items()}
    return check_plant(models, B, 1, own_params).reshape(int(B), 11)


def check_weights(weights, B: int, own: Weights) -> np.ndarray:
    """The cost weights of every lane, (B,10) float64 in gym_weights' field order (Q[4], R[2], QT[4]), from any of
      * a Weights instance: identical rows;
      * a dict with the keys "Q", "R", "QT", each (4,) / (2,) for every lane or (B,4) / (B,2) per lane; a key left
        out takes ``own``'s value (the engine's weights), so {} is the engine's weights on every lane;
      * an array (10,) or (B,10).
    Every row must pass Weights.require_gain_solvable (R > 0, Q and Q_T >= 0, all finite).  ValueError, in these words:
    "unknown weights key" for a key that is none of the three, "weights rows must hold 10 values" for an array's wrong
    trailing size, "does not broadcast" for a shape that fits none of the forms, and "weights of lane <b>:" followed by
    require_gain_solvable's own message for the first lane whose row it refuses."""
    B = int(B)
    sizes = (("Q", 4), ("R", 2), ("QT", 4))
    if isinstance(weights, Weights):
        weights = dict(Q=weights.Q, R=weights.R, QT=weights.QT)
    if isinstance(weights, dict):
        unknown = [k for k in weights if k not in ("Q", "R", "QT")]
        if unknown:
            raise ValueError(f"unknown weights key {unknown[0]!r}: the keys are Q, R, QT")
        cols = []
        for name, n in sizes:
            v = weights.get(name, getattr(own, name))
            v = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
            if v.shape not in ((n,), (B, n)):
                raise ValueError(f"weights[{name!r}] {v.shape} does not broadcast to ({B},{n}): give ({n},) or ({B},{n})")
            cols.append(np.broadcast_to(v, (B, n)))
        out = np.concatenate(cols, axis=1)
    else:
        a = np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
        if a.ndim < 1 or a.shape[-1] != 10:
            raise ValueError(f"weights rows must hold 10 values (Q[4], R[2], QT[4]), got {a.shape}")
        if a.shape not in ((10,), (B, 10)):
            raise ValueError(f"weights {a.shape} does not broadcast to ({B},10): give (10,) or ({B},10)")
        out = np.broadcast_to(a, (B, 10))
    out = np.array(out, dtype=np.float64, order="C")      # the caller's array is never aliased
    for b in range(B):
        try:
            Weights(tuple(out[b, :4]), tuple(out[b, 4:6]), tuple(out[b, 6:])).require_gain_solvable()
        except ValueError as e:
            raise ValueError(f"weights of lane {b}: {e}") from None
    return out


def check_model_table(table, B: int):
    """A per-lane model table as AcrobotEngine.model_table makes it: a float64 tensor (B,8), one gym_model per lane."""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float64 or tuple(table.shape) != (B, 8):
        raise ValueError(f"models must be a model_table ({B},8) float64 tensor, got "
                         f"{getattr(table, 'dtype', type(table).__name__)} {tuple(getattr(table, 'shape', ()))}")


def check_plant_table(table, B: int, P: int):
    """A plant table as AcrobotEngine.plant_table makes it: a float64 tensor (B,P,8), one gym_model per closed loop."""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float64 or tuple(table.shape) != (B, P, 8):
        raise ValueError(f"plant must be a plant_table ({B},{P},8) float64 tensor, got "
                         f"{getattr(table, 'dtype', type(table).__name__)} {tuple(getattr(table, 'shape', ()))}")


def check_device_QT(QT):
    """The terminal weight as a device tensor (mpc_gains' Q_T): (4,4)."""
    if tuple(QT.shape) != (4, 4):
        raise ValueError(f"QT must be (4,4), got {tuple(QT.shape)}")
    return QT
