"""Batched tensor-level front end of the HIP engine (device tensors in, device tensors out).

Every method is a thin launcher over one C-ABI entry point of include/gymnast_acrobot.h; the
arithmetic runs in the gfx950 kernels of csrc/: the Newton solver and its primitives in acrobot_kernels.hip
(kernels in newton_*.hpp), the trackers in tracking_kernels.hip (kernels in tracking_dense.hpp, mpc_gains.hpp,
track_rollout.hpp, mpc_box.hpp and the per-lane lqr_lanes.hpp, mpc_lanes.hpp, mpc_box_lanes.hpp).  Inputs are fp64
tensors (any device / numpy are copied to the engine's HIP device); outputs stay on the device.  The trackers'
argument checks are the module-level check_* functions at the end: they need no device and no engine.

Lane-major shapes follow the reference stacked over lanes: x (B,N,4), u (B,T,2), K (B,T,2,4),
sigma (B,T,2).  Internally trajectories live in the SoA "pairs" layout (see the header).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .params import PARAM_SETS, DT, Q_DIAG, R_DIAG, QT_DIAG

F64 = torch.float64


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


class AcrobotEngine:
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
        _lib.check(self.lib.gym_model_from_params(vec.ctypes.data, self.dt, C.byref(self.model)),
                   "gym_model_from_params")
        self.weights = weights or Weights()
        self._w = self.weights.c_struct()
        self.mpc_qt_cache = {}     # (Q, R) -> Q_T of per-lane MPC tracking; it depends on this engine's model and dt

    # -------------------------------------------------------------------------------- utils
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
        out = torch.empty((L, Cc // W, Bp, W), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_pack_lanes(a.data_ptr(), out.data_ptr(), B, Bp, L, Cc, W, self.stream),
                   "gym_pack_lanes")
        return out

    def unpack(self, soa: torch.Tensor, B: int, soa1: torch.Tensor | None = None,
               sel: torch.Tensor | None = None) -> torch.Tensor:
        """SoA (L, P, Bp, W) -> lane-major (B, L, P*W); lane b reads soa1 where sel[b] != 0."""
        L, P, Bp, W = soa.shape
        out = torch.empty((B, L, P * W), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_unpack_lanes(soa.data_ptr(), _lib.ptr(soa1), _lib.ptr(sel), out.data_ptr(), B, Bp,
                                             L, P * W, W, self.stream), "gym_unpack_lanes")
        return out

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
        out = torch.empty((n, 4), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_continuous_dynamics(C.byref(self.model), x.data_ptr(), u.data_ptr(), out.data_ptr(),
                                                    n, self.stream), "gym_continuous_dynamics")
        return out

    def rk4(self, x, u) -> torch.Tensor:
        x, u, n = self._points(x, u)
        out = torch.empty((n, 4), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_rk4_step(C.byref(self.model), x.data_ptr(), u.data_ptr(), out.data_ptr(), n,
                                         self.stream), "gym_rk4_step")
        return out

    def jacobians(self, x, u):
        x, u, n = self._points(x, u)
        A = torch.empty((n, 4, 4), dtype=F64, device=self.device)
        Bm = torch.empty((n, 4, 2), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_jacobians(C.byref(self.model), x.data_ptr(), u.data_ptr(), A.data_ptr(),
                                          Bm.data_ptr(), n, self.stream), "gym_jacobians")
        return A, Bm

    def stage_cost_derivs(self, x, x_ref, u, u_ref, Q, R, terminal=False):
        x = self.t(x).reshape(-1, 4); xr = self.t(x_ref).reshape(-1, 4)
        n = x.shape[0]
        Qm = np.ascontiguousarray(np.asarray(Q, float).reshape(4, 4))
        l = torch.empty(n, dtype=F64, device=self.device)
        gx = torch.empty((n, 4), dtype=F64, device=self.device)
        if terminal:
            u_ = ur_ = gu = None
            Rm = None
        else:
            u_ = self.t(u).reshape(-1, 2); ur_ = self.t(u_ref).reshape(-1, 2)
            Rm = np.ascontiguousarray(np.asarray(R, float).reshape(2, 2))
            gu = torch.empty((n, 2), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_stage_cost_derivs(
            x.data_ptr(), xr.data_ptr(), _lib.ptr(u_), _lib.ptr(ur_), Qm.ctypes.data,
            None if Rm is None else Rm.ctypes.data, int(bool(terminal)), l.data_ptr(), gx.data_ptr(), _lib.ptr(gu),
            n, self.stream), "gym_stage_cost_derivs")
        return l, gx, gu

    # ----------------------------------------------------------------- trajectory kernels
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
        xs = torch.empty((N, 2, Bp, 2), dtype=F64, device=self.device)
        J = torch.empty(Bp, dtype=F64, device=self.device)
        _lib.check(self.lib.gym_rollout_open_loop(C.byref(self.model), C.byref(self._w), x0.data_ptr(),
                                                  us.data_ptr(), x_ref.data_ptr(), u_ref.data_ptr(), xs.data_ptr(),
                                                  J.data_ptr(), B, Bp, N, self.stream), "gym_rollout_open_loop")
        return self.unpack(xs, B), J[:B]

    def closed_loop(self, x, u, K, sigma, gamma, x_ref, u_ref):
        """forward_closed_loop_update (+ total_cost of the result), full gains K (B,T,2,4)."""
        x = self.t(x); u = self.t(u); K = self.t(K); sigma = self.t(sigma)
        B, N, _ = x.shape
        T = N - 1
        x_ref, u_ref = self.refs(x_ref, u_ref)
        Bp = padded(B)
        g = torch.zeros(Bp, dtype=F64, device=self.device)
        g[:B] = self.t(gamma).reshape(-1).expand(B) if self.t(gamma).numel() == 1 else self.t(gamma).reshape(B)
        xs, us = self.pack(x, Bp), self.pack(u, Bp, W=1)
        Ks = self.pack(K.reshape(B, T, 8), Bp)
        ss = self.pack(sigma, Bp, W=1)
        xn = torch.empty_like(xs); un = torch.empty_like(us)
        J = torch.empty(Bp, dtype=F64, device=self.device)
        _lib.check(self.lib.gym_closed_loop(C.byref(self.model), C.byref(self._w), xs.data_ptr(), us.data_ptr(),
                                            Ks.data_ptr(), ss.data_ptr(), g.data_ptr(), x_ref.data_ptr(),
                                            u_ref.data_ptr(), xn.data_ptr(), un.data_ptr(), J.data_ptr(), B, Bp, N,
                                            self.stream), "gym_closed_loop")
        return self.unpack(xn, B), self.unpack(un, B), J[:B]

    def gamma_sweep(self, x, u, K, sigma, gammas, x_ref, u_ref) -> torch.Tensor:
        """J(gamma_g) of forward_closed_loop_update + total_cost for each lane and step size (the reference's
        Armijo line-search curve, plot_armijo_line_search :258-264): x (B,N,4), u (B,T,2), K (B,T,2,4),
        sigma (B,T,2), gammas (G,) -> (B, G)."""
        x = self.t(x); u = self.t(u); K = self.t(K); sigma = self.t(sigma)
        g = self.t(gammas).reshape(-1)
        B, N, _ = x.shape
        T = N - 1
        G = int(g.numel())
        if G < 1:
            raise ValueError("gamma_sweep needs at least one step size")
        x_ref, u_ref = self.refs(x_ref, u_ref)
        Bp = padded(B)
        xs, us = self.pack(x, Bp), self.pack(u, Bp, W=1)
        Ks = self.pack(K.reshape(B, T, 8), Bp)
        ss = self.pack(sigma, Bp, W=1)
        J = torch.empty((G, Bp), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_gamma_sweep(C.byref(self.model), C.byref(self._w), xs.data_ptr(), us.data_ptr(),
                                            Ks.data_ptr(), ss.data_ptr(), g.data_ptr(), G, x_ref.data_ptr(),
                                            u_ref.data_ptr(), J.data_ptr(), B, Bp, N, self.stream), "gym_gamma_sweep")
        return J[:, :B].t()

    def total_cost(self, x, u, x_ref, u_ref, Q, R, QT):
        x = self.t(x); u = self.t(u)
        B, N, _ = x.shape
        x_ref = self.t(x_ref); u_ref = self.t(u_ref)[: N - 1].contiguous()
        Bp = padded(B)
        xs, us = self.pack(x, Bp), self.pack(u, Bp, W=1)
        mats = [np.ascontiguousarray(np.asarray(M, float)) for M in (Q, R, QT)]
        J = torch.empty(Bp, dtype=F64, device=self.device)
        _lib.check(self.lib.gym_total_cost(xs.data_ptr(), us.data_ptr(), x_ref.data_ptr(), u_ref.data_ptr(),
                                           mats[0].ctypes.data, mats[1].ctypes.data, mats[2].ctypes.data,
                                           J.data_ptr(), B, Bp, N, self.stream), "gym_total_cost")
        return J[:B]

    def backward(self, x, u, x_ref, u_ref, want_lambda=False, check_gains=True):
        """Fused costate + stage lists + Riccati: K (B,T,2,4), sigma (B,T,2), dJ (B,), max|sigma| (B,), lambda.
        ``check_gains=False``: the caller uses only lambda (compute_costate_trajectory), which needs no G^-1."""
        if check_gains:
            self.weights.require_gain_solvable()
        x = self.t(x); u = self.t(u)
        B, N, _ = x.shape
        T = N - 1
        x_ref, u_ref = self.refs(x_ref, u_ref)
        Bp = padded(B)
        xs, us = self.pack(x, Bp), self.pack(u, Bp, W=1)
        K1 = torch.empty((T, 2, Bp, 2), dtype=F64, device=self.device)
        sg = torch.empty((T, 2, Bp, 1), dtype=F64, device=self.device)
        dJ = torch.empty(Bp, dtype=F64, device=self.device)
        sm = torch.empty(Bp, dtype=F64, device=self.device)
        lam = torch.empty((N, 2, Bp, 2), dtype=F64, device=self.device) if want_lambda else None
        _lib.check(self.lib.gym_backward_sweep(C.byref(self.model), C.byref(self._w), xs.data_ptr(), us.data_ptr(),
                                               x_ref.data_ptr(), u_ref.data_ptr(), K1.data_ptr(), sg.data_ptr(),
                                               dJ.data_ptr(), sm.data_ptr(), _lib.ptr(lam), B, Bp, N, self.stream),
                   "gym_backward_sweep")
        K = torch.empty((B, T, 2, 4), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_unpack_gains(K1.data_ptr(), K.data_ptr(), B, Bp, T, self.stream), "gym_unpack_gains")
        return K, self.unpack(sg, B), dJ[:B], sm[:B], (self.unpack(lam, B) if want_lambda else None)

    def linearize(self, x, u, x_ref, u_ref):
        """build_stage_lists: A_d (B,T,4,4), B_d (B,T,4,2), q (B,T,4), r (B,T,2), q_T (B,4)."""
        x = self.t(x); u = self.t(u)
        B, N, _ = x.shape
        T = N - 1
        x_ref, u_ref = self.refs(x_ref, u_ref)
        Bp = padded(B)
        xs, us = self.pack(x, Bp), self.pack(u, Bp, W=1)
        e = lambda *s: torch.empty(s, dtype=F64, device=self.device)  # noqa: E731
        Ad, Bd, q, r, qT = e(T, 16, Bp), e(T, 8, Bp), e(T, 4, Bp), e(T, 2, Bp), e(4, Bp)
        _lib.check(self.lib.gym_linearize(C.byref(self.model), C.byref(self._w), xs.data_ptr(), us.data_ptr(),
                                          x_ref.data_ptr(), u_ref.data_ptr(), Ad.data_ptr(), Bd.data_ptr(),
                                          q.data_ptr(), r.data_ptr(), qT.data_ptr(), B, Bp, N, self.stream),
                   "gym_linearize")
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
            out = torch.zeros((T, n, Bp), dtype=F64, device=self.device)
            out[:, :, :B] = a.reshape(B, T, n).permute(1, 2, 0)
            return out

        def soa_t(a, shape_tail):
            a = self.t(a).expand(B, *shape_tail)
            n = int(np.prod(shape_tail))
            out = torch.zeros((n, Bp), dtype=F64, device=self.device)
            out[:, :B] = a.reshape(B, n).T
            return out

        As, Bs, Qs, Rs, Ss = soa(A, (4, 4)), soa(Bm, (4, 2)), soa(Q, (4, 4)), soa(R, (2, 2)), soa(S, (2, 4))
        qs, rs, QTs, qTs = soa(q, (4,)), soa(r, (2,)), soa_t(QT, (4, 4)), soa_t(qT, (4,))
        K = torch.empty((T, 8, Bp), dtype=F64, device=self.device)
        sg = torch.empty((T, 2, Bp), dtype=F64, device=self.device)
        dJ = torch.empty(Bp, dtype=F64, device=self.device)
        _lib.check(self.lib.gym_riccati_general(As.data_ptr(), Bs.data_ptr(), Qs.data_ptr(), Rs.data_ptr(),
                                                Ss.data_ptr(), qs.data_ptr(), rs.data_ptr(), QTs.data_ptr(),
                                                qTs.data_ptr(), K.data_ptr(), sg.data_ptr(), dJ.data_ptr(), B, Bp, T,
                                                self.stream), "gym_riccati_general")
        return (K[..., :B].permute(2, 0, 1).reshape(B, T, 2, 4), sg[..., :B].permute(2, 0, 1).contiguous(),
                dJ[:B])

    # ------------------------------------------------------------------ LQR / MPC trackers
    def tv_lqr_gains(self, A, Bm, Q, R, QT, L: int, nwin: int = 1, all_gains: bool = True, A_pad=None,
                     B_pad=None, discretize: bool = False) -> torch.Tensor:
        """Windowed time-varying LQR gains (gym_tv_lqr_gains): stages A (S,4,4), B (S,4,2) on the device.
        all_gains: (L-1,2,4) gains of window 0; else (nwin,2,4) first gains of windows 0..nwin-1."""
        A = self.t(A).reshape(-1, 4, 4); Bm = self.t(Bm).reshape(-1, 4, 2)
        S = A.shape[0]
        Ap = None if A_pad is None else self.t(A_pad).reshape(4, 4)
        Bp_ = None if B_pad is None else self.t(B_pad).reshape(4, 2)
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        QTd = self.t(QT).reshape(4, 4)                 # device: e.g. dare_fixed_point's P, no host round trip
        out = torch.empty(((L - 1) if all_gains else nwin, 2, 4), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_tv_lqr_gains(A.data_ptr(), Bm.data_ptr(), S, _lib.ptr(Ap), _lib.ptr(Bp_),
                                             Qh.ctypes.data, Rh.ctypes.data, QTd.data_ptr(), int(L), int(nwin),
                                             int(bool(all_gains)), int(bool(discretize)), self.dt, out.data_ptr(),
                                             self.stream), "gym_tv_lqr_gains")
        return out

    def dare_fixed_point(self, A, Bm, Q, R, max_iter: int = 1000, tol: float = 1e-6):
        """compute_P_inf on the device: returns (P (4,4), iterations (1,) int32), both device tensors (no sync)."""
        A = self.t(A).reshape(4, 4); Bm = self.t(Bm).reshape(4, 2)
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        P = torch.empty((4, 4), dtype=F64, device=self.device)
        it = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gym_dare_fixed_point(A.data_ptr(), Bm.data_ptr(), Qh.ctypes.data, Rh.ctypes.data,
                                                 int(max_iter), float(tol), P.data_ptr(), it.data_ptr(), self.stream),
                   "gym_dare_fixed_point")
        return P, it

    def _mpc_gains(self, every, x_ref, u_ref, x_f, u_f, Q, R, L, nwin, max_iter, tol):
        """gym_mpc_gains_all (``every`` gain of every window) or gym_mpc_gains (each window's first gain)."""
        x_ref = self.t(x_ref).reshape(-1, 4); u_ref = self.t(u_ref).reshape(-1, 2)
        x_f = self.t(x_f).reshape(4); u_f = self.t(u_f).reshape(2)
        S = x_ref.shape[0] - 1
        if u_ref.shape[0] < S:
            raise ValueError(f"u_ref must hold {S} stages, got {u_ref.shape[0]}")
        Qh, Rh = host_mat(Q, 4, "Q"), host_mat(R, 2, "R")
        K = torch.empty((nwin, int(L) - 1, 2, 4) if every else (nwin, 2, 4), dtype=F64, device=self.device)
        P = torch.empty((4, 4), dtype=F64, device=self.device)
        it = torch.zeros(1, dtype=torch.int32, device=self.device)
        name = "gym_mpc_gains_all" if every else "gym_mpc_gains"
        _lib.check(getattr(self.lib, name)(C.byref(self.model), x_ref.data_ptr(), u_ref.data_ptr(), S, x_f.data_ptr(),
                                           u_f.data_ptr(), Qh.ctypes.data, Rh.ctypes.data, int(L), int(nwin),
                                           int(max_iter), float(tol), K.data_ptr(), P.data_ptr(), it.data_ptr(),
                                           self.stream), name)
        return K, P, it

    def mpc_gains(self, x_ref, u_ref, x_f, u_f, Q, R, L: int, nwin: int, max_iter: int = 1000, tol: float = 1e-6):
        """Fused MPC gains (gym_mpc_gains): stage linearisations of (x_ref, u_ref) and of the pad (x_f, u_f),
        Q_T = compute_P_inf(A_f, B_f, Q, R), and each window's first gain.  Returns device tensors
        (K0 (nwin,2,4), Q_T (4,4), iterations (1,) int32); no host synchronisation."""
        return self._mpc_gains(False, x_ref, u_ref, x_f, u_f, Q, R, L, nwin, max_iter, tol)

    def lq_forward(self, A, Bm, K, x0, L: int, A_pad=None, B_pad=None, discretize: bool = False):
        """One window's LQ forward pass: X (L,4), U (L-1,2)."""
        A = self.t(A).reshape(-1, 4, 4); Bm = self.t(Bm).reshape(-1, 4, 2)
        Ap = None if A_pad is None else self.t(A_pad).reshape(4, 4)
        Bp_ = None if B_pad is None else self.t(B_pad).reshape(4, 2)
        K = self.t(K).reshape(-1, 2, 4); x0 = self.t(x0).reshape(4)
        X = torch.empty((L, 4), dtype=F64, device=self.device)
        U = torch.empty((L - 1, 2), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_lq_forward(A.data_ptr(), Bm.data_ptr(), A.shape[0], _lib.ptr(Ap), _lib.ptr(Bp_),
                                           int(bool(discretize)), self.dt, K.data_ptr(), x0.data_ptr(), int(L),
                                           X.data_ptr(), U.data_ptr(), self.stream), "gym_lq_forward")
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
        x = torch.empty((B, N, 4), dtype=F64, device=self.device)
        u = torch.empty((B, N - 1, 2), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_track_rollout_ex(C.byref(self.model), x0.data_ptr(), x_ff.data_ptr(),
                                                 u_ff.data_ptr(), K.data_ptr(), B, N,
                                                 _lib.TRACK_SINGLE if single else 0, x.data_ptr(), u.data_ptr(),
                                                 self.stream), "gym_track_rollout_ex")
        return x, u

    # ------------------------------------------------------------- torque-limited MPC (box QP)
    def mpc_gains_all(self, x_ref, u_ref, x_f, u_f, Q, R, L: int, nwin: int, max_iter: int = 1000,
                      tol: float = 1e-6):
        """gym_mpc_gains_all: mpc_gains with every stage's gain of every window.  Returns device tensors
        (K_all (nwin,L-1,2,4), Q_T (4,4), iterations (1,) int32); K_all[:, 0] is mpc_gains' K0 bit for bit."""
        return self._mpc_gains(True, x_ref, u_ref, x_f, u_f, Q, R, L, nwin, max_iter, tol)

    def _ws_bytes(self, name: str, *sizes) -> int:
        """What the workspace-size entry point ``name`` answers for ``sizes``."""
        need = C.c_int64()
        _lib.check(getattr(self.lib, name)(*(int(v) for v in sizes), C.byref(need)), name)
        return need.value

    def mpc_box_workspace(self, B: int, L: int, rows: int) -> torch.Tensor:
        """The caller-owned workspace of gym_mpc_box_qp (rows = stages given) / gym_mpc_box_rollout (rows = N)."""
        return torch.empty(self._ws_bytes("gym_mpc_box_workspace", B, L, rows), dtype=torch.uint8, device=self.device)

    def mpc_box_qp(self, A, Bm, u_ref, Q, R, QT, x0, L: int, tau_max: float, max_qp_iters: int = 32, ws=None):
        """gym_mpc_box_qp: the torque-limited QP of one window for a batch x0 (B,4).  Stages A (S,4,4), Bm (S,4,2),
        u_ref (S,2) are host arrays (S >= L-1).  Returns device tensors U (B,L-1,2), X (B,L,4), iterations (B,)
        int32, converged (B,) int32."""
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
        ws = self.mpc_box_workspace(B, L, S) if ws is None else ws
        U = torch.empty((B, L - 1, 2), dtype=F64, device=self.device)
        X = torch.empty((B, L, 4), dtype=F64, device=self.device)
        it = torch.empty(B, dtype=torch.int32, device=self.device)
        conv = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gym_mpc_box_qp(A.ctypes.data, Bm.ctypes.data, ur.ctypes.data, S, Qh.ctypes.data,
                                           Rh.ctypes.data, QTd.data_ptr(), x0.data_ptr(), B, L, float(tau_max),
                                           int(max_qp_iters), ws.data_ptr(), ws.numel(), U.data_ptr(), X.data_ptr(),
                                           it.data_ptr(), conv.data_ptr(), self.stream), "gym_mpc_box_qp")
        return U, X, it, conv

    def mpc_box_rollout(self, x0, x_ref, u_ref, x_f, u_f, Q, R, QT, K_all, tau_max: float, max_qp_iters: int = 32,
                        ws=None):
        """gym_mpc_box_rollout: the torque-limited closed loop of B lanes.  Returns device tensors x (B,N,4),
        u (B,N-1,2), qp_iters (B,N-1) int32, unconverged (B,) int32."""
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
        ws = self.mpc_box_workspace(B, L, N) if ws is None else ws
        x = torch.empty((B, N, 4), dtype=F64, device=self.device)
        u = torch.empty((B, N - 1, 2), dtype=F64, device=self.device)
        it = torch.empty((B, N - 1), dtype=torch.int32, device=self.device)
        unconv = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.gym_mpc_box_rollout(C.byref(self.model), x0.data_ptr(), x_ref.data_ptr(),
                                                u_ref.data_ptr(), x_f.data_ptr(), u_f.data_ptr(), Qh.ctypes.data,
                                                Rh.ctypes.data, QTd.data_ptr(), K_all.data_ptr(), B, N, L,
                                                float(tau_max), int(max_qp_iters), ws.data_ptr(), ws.numel(),
                                                x.data_ptr(), u.data_ptr(), it.data_ptr(), unconv.data_ptr(),
                                                self.stream), "gym_mpc_box_rollout")
        return x, u, it, unconv

    # ------------------------------------------------------------- per-lane LQR tracking
    def lqr_lanes_workspace(self, B: int, N: int) -> torch.Tensor:
        """The caller-owned workspace of gym_lqr_lanes_gains / gym_lqr_lanes_rollout for B lanes of N knots."""
        return torch.empty(self._ws_bytes("gym_lqr_lanes_workspace", B, N), dtype=torch.uint8, device=self.device)

    def lqr_lanes_gains(self, x_opt, u_opt, Q, R, QT, gains: bool = True, ws=None):
        """gym_lqr_lanes_gains: solve_LQR_tracking per lane along x_opt (B,N,4), u_opt (B,N-1,2).  Returns (ws, K):
        the filled workspace lqr_lanes_rollout takes, and K (B,N-1,2,4) on the device (None unless ``gains``)."""
        x_opt = self.t(x_opt); u_opt = self.t(u_opt)
        B, N = check_lane_trajectories(x_opt, u_opt)
        Rh = check_diagonal_R(R, "per-lane LQR tracking")
        Qh, QTh = check_sym_weight(Q, "Q"), check_sym_weight(QT, "QT")
        ws = self.lqr_lanes_workspace(B, N) if ws is None else ws
        K = torch.empty((B, N - 1, 2, 4), dtype=F64, device=self.device) if gains else None
        _lib.check(self.lib.gym_lqr_lanes_gains(C.byref(self.model), x_opt.data_ptr(), u_opt.data_ptr(), B, N,
                                                Qh.ctypes.data, Rh.ctypes.data, QTh.ctypes.data, ws.data_ptr(),
                                                ws.numel(), _lib.ptr(K), self.stream), "gym_lqr_lanes_gains")
        return ws, K

    def lqr_lanes_rollout(self, ws, x0, N: int, trajectories: bool = True):
        """gym_lqr_lanes_rollout on a workspace lqr_lanes_gains filled: x0 (B,P,4) -> (x (B,P,N,4), u (B,P,N-1,2),
        summary (3,B,P) = err_final, err_max, u_max) on the device; x, u are None unless ``trajectories``."""
        x0 = self.t(x0)
        check_lane_starts(x0)
        B, P, N = x0.shape[0], x0.shape[1], int(N)
        x = torch.empty((B, P, N, 4), dtype=F64, device=self.device) if trajectories else None
        u = torch.empty((B, P, N - 1, 2), dtype=F64, device=self.device) if trajectories else None
        summary = torch.empty((3, B, P), dtype=F64, device=self.device)
        _lib.check(self.lib.gym_lqr_lanes_rollout(C.byref(self.model), x0.data_ptr(), B, P, N, ws.data_ptr(),
                                                  ws.numel(), _lib.ptr(x), _lib.ptr(u), summary.data_ptr(),
                                                  self.stream), "gym_lqr_lanes_rollout")
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
        need = self._ws_bytes("gym_lqr_lanes_workspace", B, N)
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws_bytes = ws.numel() * ws.element_size()
        if ws_bytes < need:
            raise ValueError(f"the workspace holds {ws_bytes} bytes, {B} lanes of {N} knots need {need}")
        K = torch.empty((B, N - 1, 2, 4), dtype=F64, device=self.device) if gains else None
        _lib.check(self.lib.gym_mpc_lanes_gains(C.byref(self.model), x_opt.data_ptr(), u_opt.data_ptr(), B, N, L,
                                                Qh.ctypes.data, Rh.ctypes.data, QTd.data_ptr(), ws.data_ptr(),
                                                ws_bytes, _lib.ptr(K), self.stream), "gym_mpc_lanes_gains")
        return ws, K

    # ------------------------------------------------------------- per-lane torque-limited MPC tracking
    BOX_LANES_WS_SHARE = 0.5    # mpc_box_lanes_rollout's own workspace: at most this share of the free device memory

    def mpc_box_lanes_workspace(self, B: int, P: int, L: int) -> int:
        """Bytes of gym_mpc_box_lanes_rollout's caller-owned workspace for B lanes x P starts, windows of L stages."""
        return self._ws_bytes("gym_mpc_box_lanes_workspace", B, P, L)

    def mpc_box_lanes_rollout(self, x_opt, u_opt, x0, Q, R, QT, L: int, tau_max: float, max_qp_iters: int = 32,
                              trajectories: bool = True, max_ws_bytes: int | None = None):
        """gym_mpc_box_lanes_rollout: the torque-limited MPC closed loop of every lane along its own x_opt (B,N,4),
        u_opt (B,N-1,2) from the starts x0 (B,P,4); QT (4,4) a device tensor as in mpc_lanes_gains.  Returns device
        tensors (x (B,P,N,4), u (B,P,N-1,2), summary (3,B,P), qp_iters (B,P,N-1) int32, unconverged (B,P) int32); x, u
        and qp_iters are None unless ``trajectories``.  The sweep workspace (about 80 (L-1) bytes per lane and start) is
        allocated here; a batch whose workspace would exceed ``max_ws_bytes`` (default: BOX_LANES_WS_SHARE of the free
        device memory) runs in chunks of whole lanes, one call each -- the same results, lanes being independent."""
        x_opt = self.t(x_opt); u_opt = self.t(u_opt); x0 = self.t(x0)
        B, N = check_lane_trajectories(x_opt, u_opt)
        check_lane_starts(x0, B)
        P, L = x0.shape[1], check_window(L, "the torque-limited QP")
        if B * P > _lib.MAX_BP:
            raise ValueError(f"{B} lanes x {P} starts exceed {_lib.MAX_BP} closed loops per call")
        check_box(tau_max, max_qp_iters)
        Rh = check_diagonal_R(R, "the torque-limited QP")
        Qh = check_sym_weight(Q, "Q")
        QTd = check_device_QT(self.t(QT))
        per_lane = self.mpc_box_lanes_workspace(1, P, L)
        if max_ws_bytes is None:
            max_ws_bytes = int(self.BOX_LANES_WS_SHARE * torch.cuda.mem_get_info(self.device)[0])
        chunk = max(1, min(B, int(max_ws_bytes) // per_lane))
        ws = torch.empty(chunk * per_lane, dtype=torch.uint8, device=self.device)
        x = torch.empty((B, P, N, 4), dtype=F64, device=self.device) if trajectories else None
        u = torch.empty((B, P, N - 1, 2), dtype=F64, device=self.device) if trajectories else None
        it = torch.empty((B, P, N - 1), dtype=torch.int32, device=self.device) if trajectories else None
        summary = torch.empty((3, B, P), dtype=F64, device=self.device)
        unconv = torch.empty((B, P), dtype=torch.int32, device=self.device)
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            sm = summary if chunk >= B else torch.empty((3, b1 - b0, P), dtype=F64, device=self.device)
            _lib.check(self.lib.gym_mpc_box_lanes_rollout(
                C.byref(self.model), x_opt[b0:b1].data_ptr(), u_opt[b0:b1].data_ptr(), x0[b0:b1].data_ptr(), b1 - b0,
                P, N, L, Qh.ctypes.data, Rh.ctypes.data, QTd.data_ptr(), float(tau_max), int(max_qp_iters),
                ws.data_ptr(), ws.numel(), _lib.ptr(None if x is None else x[b0:b1]),
                _lib.ptr(None if u is None else u[b0:b1]), sm.data_ptr(), _lib.ptr(None if it is None else it[b0:b1]),
                unconv[b0:b1].data_ptr(), self.stream), "gym_mpc_box_lanes_rollout")
            if sm is not summary:
                summary[:, b0:b1] = sm
        return x, u, summary, it, unconv


# ------------------------------------------------------------------ the trackers' argument checks
# Plain functions of shapes and host values (torch tensors and numpy arrays alike): no device, no engine, so the
# front end (trajectory_tracking.py) refuses a bad call with the same words before it asks for either.
def host_mat(M, n, name):
    M = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    if M.shape != (n, n):
        raise ValueError(f"{name} must be {n}x{n}, got {M.shape}")
    return M


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


def check_box(tau_max, max_qp_iters):
    """The torque limit and the active set's sweep cap."""
    if not (np.isfinite(tau_max) and tau_max > 0):
        raise ValueError(f"tau_max must be finite and positive, got {tau_max}")
    if int(max_qp_iters) < 1:
        raise ValueError(f"max_qp_iters must be at least 1, got {max_qp_iters}")


def check_device_QT(QT):
    """The terminal weight as a device tensor (mpc_gains' Q_T): (4,4)."""
    if tuple(QT.shape) != (4, 4):
        raise ValueError(f"QT must be (4,4), got {tuple(QT.shape)}")
    return QT
