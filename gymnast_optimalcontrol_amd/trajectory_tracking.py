"""Drop-in for the reference's ``trajectory_tracking`` module (LQR and receding-horizon MPC trackers).

Reference: /root/reference/trajectory_tracking.py (main.py task_3 / task_4).  Same names, arguments and
return values; the arithmetic runs in the gfx950 kernels of the csrc/tracking_kernels.hip translation unit
(tracking_dense.hpp: gym_tv_lqr_gains, gym_dare_fixed_point, gym_lq_forward; mpc_gains.hpp: gym_mpc_gains;
track_rollout.hpp: gym_track_rollout; mpc_box.hpp: the torque-limited QP) and the acrobot kernels (Jacobians, RK4).

Without a torque limit (the reference's default, test_constraints = False, :87) the MPC QP (solver_mpc
:73-140) has only equality constraints, so its solution is the finite-horizon LQ solution over the window; it
is computed exactly (no IPOPT iterations): u0 = K_0(t) x0 with K_0(t) the window's first gain.  Every lane
follows the same reference, so the gains of all T control steps are computed once (one window per thread) and
the B perturbed initial states are then simulated in closed loop in one batched kernel -- the same controls
the per-step re-solve produces.

With ``tau_max`` (the reference's test_constraints path, :87-114, tau_max = 18) every stage of the window obeys
-tau_max <= u_t + u_ref_t <= tau_max, and each lane at each control step owns an inequality-constrained QP.  It
is solved exactly by a primal-dual active set over a clamped Riccati sweep (gym_mpc_box_qp /
gym_mpc_box_rollout; DESIGN "Torque-limited MPC"), at most ``max_qp_iters`` sweeps per QP; a QP that has not
settled by then returns the clipped last iterate and is counted in ``unconverged``.  ``tau_max=TorqueLimit(18.0)``
turns the fallback on: such a QP goes on by projected Newton from that clipped iterate ("The fallback"),
``qp_iters`` counts both phases and ``unconverged`` only the QPs that neither phase finished.

Batched additions: ``LQR_tracking_batch``, ``solve_mpc_tracking_batch`` and ``solve_mpc_tracking_box_batch``
take x0 (B,4) and return device tensors; they follow one reference shared by every lane.  ``LQR_tracking_lanes`` /
``lqr_gains_lanes`` track every lane's own trajectory (x_opt (B,N,4), u_opt (B,N-1,2), e.g. a batched solve's result):
per-lane gains and closed-loop rollouts in the kernels of csrc/lqr_lanes.hpp (gym_lqr_lanes_gains /
gym_lqr_lanes_rollout).  ``MPC_tracking_lanes`` / ``mpc_gains_lanes`` do the same with the receding-horizon
MPC (no torque limit): the first gain of every T_pred-stage window along every lane's own trajectory in the kernel of
csrc/mpc_lanes.hpp (gym_mpc_lanes_gains), then the same closed-loop rollout; with ``tau_max`` every
closed loop solves its own torque-limited QPs along its own lane's trajectory in the kernel of csrc/mpc_box_lanes.hpp
(gym_mpc_box_lanes_rollout).  ``plant=`` on both simulates a mismatched plant per closed loop: the
controller stays on the design model and the RK4 step of closed loop (b, p) runs on its own parameter set
(gym_lqr_lanes_rollout_plant / gym_mpc_box_lanes_rollout_plant); ``sample_plants`` draws such sets.
There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import dynamics as _dyn
from .engine import check_box, check_lane_starts, check_lane_trajectories, check_models, check_plant, check_window
from .params import PARAM_NAMES, PARAM_SETS
from .dynamics import dt, ns, ni  # noqa: F401  (the reference module's namespace, trajectory_tracking.py:3)

nu = ni
Q_REG = np.diag([100.0, 100.0, 10.0, 10.0])        # trajectory_tracking.py:173
R_REG = np.diag([1.0, 1.0])                         # :174
QT_REG = Q_REG * 2.0                                # :175
Q_MPC = np.diag([120.0, 100.0, 0.0001, 0.0001])     # :36
R_MPC = np.diag([1e-6, 10.0])                       # :37
X_F = np.array([np.pi, 0.0, 0.0, 0.0])              # :31
U_F = np.array([0.0, 0.0])                          # :32
T_PRED = 75                                         # :10
TAU_MAX = 18.0                                      # :91 (solver_mpc's torque limit, test_constraints)
MPC_FUSED_MAX_STAGES = _lib.MPC_MAX_STAGES          # gym_mpc_gains: T_pred + 2 stages per workgroup's LDS table


@dataclass(frozen=True)
class TorqueLimit:
    """A torque limit with the projected-Newton fallback, accepted wherever ``tau_max=`` is (solver_mpc,
    solve_mpc_tracking, solve_mpc_tracking_box_batch, MPC_tracking_lanes, SolveResult.track_mpc).  A plain number
    keeps its meaning: the active set alone, a QP that reaches ``max_qp_iters`` is clipped and counted unconverged.
    With a TorqueLimit such a QP is continued by projected Newton from that clipped iterate for at most
    ``fallback_iters`` iterations (one Riccati sweep each).  Then qp_iters = active-set sweeps + Newton iterations
    (> max_qp_iters exactly when the fallback ran) and unconverged counts only QPs that neither phase finished.  QPs
    that settle within max_qp_iters are the plain number's QPs bit for bit.  128 is a cap, about twice the largest
    count seen on the CPU (69), not a tuned value; 0 is the plain number."""
    tau_max: float
    fallback_iters: int = 128


def _torque_limit(tau_max):
    """(tau_max, fallback_iters) of a ``tau_max=`` value: a number (no fallback), a TorqueLimit, or None."""
    if isinstance(tau_max, TorqueLimit):
        return tau_max.tau_max, tau_max.fallback_iters
    return tau_max, 0


def _fb_kw(fb) -> dict:
    """The engine keyword of the fallback; none without it, so a plain tau_max makes the call it always made."""
    return {"fallback_iters": int(fb)} if fb else {}


def _eng():
    return _dyn.engine()


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


_FINAL_STATE = {}


def _final_state(eng):
    """X_F, U_F (:31-32) as device tensors, made once per device: a pageable host-to-device copy inside every
    mpc_gains call would make the host wait for the GPU and leave the GPU idle while Python enqueues the run."""
    key = str(eng.device)
    if key not in _FINAL_STATE:
        _FINAL_STATE[key] = (eng.t(X_F.reshape(1, 4)), eng.t(U_F.reshape(1, 2)))
    return _FINAL_STATE[key]


def _discrete(eng, A_c, B_c):
    eye = torch.eye(4, dtype=A_c.dtype, device=A_c.device)
    return eye + eng.dt * A_c, eng.dt * B_c                      # trajectory_generation.py:161-164


def compute_P_inf(A, B, Q, R):
    """trajectory_tracking.py:144-165 (fixed-point iteration, max 1000 iterations, tol 1e-6)."""
    eng = _eng()
    P, it = eng.dare_fixed_point(A, B, Q, R, max_iter=1000, tol=1e-6)
    P = _np(P)
    if int(it.item()) > 1000:                    # the tolerance was never met in 1000 iterations (:164)
        print("P_inf did not converge!!!")
    return P


def solve_LQR_tracking(x_opt, u_opt):
    """trajectory_tracking.py:170-203 -> list of N-1 gains (2,4)."""
    K = lqr_gains(x_opt, u_opt)
    return list(_np(K))


def lqr_gains(x_opt, u_opt, Q=Q_REG, R=R_REG, QT=QT_REG) -> torch.Tensor:
    """Device form of solve_LQR_tracking: (N-1, 2, 4) tensor."""
    eng = _eng()
    x_opt = eng.t(x_opt).reshape(-1, 4)
    u_opt = eng.t(u_opt).reshape(-1, 2)
    S = x_opt.shape[0] - 1
    A_c, B_c = eng.jacobians(x_opt[:S], u_opt[:S])
    return eng.tv_lqr_gains(A_c, B_c, Q, R, QT, L=S + 1, nwin=1, all_gains=True, discretize=True)


def simulate_tracking(x_opt, u_opt, K_reg, x0_perturbed):
    """trajectory_tracking.py:206-216 -> (x_track (N,4), u_track (N-1,2)) numpy."""
    eng = _eng()
    K = eng.t(np.asarray([np.asarray(k, dtype=float) for k in K_reg]) if isinstance(K_reg, (list, tuple)) else K_reg)
    x, u = eng.track_rollout(np.asarray(x0_perturbed, dtype=float).reshape(1, 4), x_opt, u_opt, K)
    return _np(x[0]), _np(u[0])


def LQR_tracking(x_ref, u_ref, t_ref, x0_perturbed=None):
    """trajectory_tracking.py:219-249 (plotting omitted) -> (x_track, u_track)."""
    if x0_perturbed is None:
        x0_perturbed = np.asarray(x_ref)[0].copy()
    K_reg_seq = solve_LQR_tracking(x_ref, u_ref)
    return simulate_tracking(x_ref, u_ref, K_reg_seq, x0_perturbed)


def LQR_tracking_batch(x_ref, u_ref, x0):
    """Batched LQR tracking: x0 (B,4) -> (x (B,N,4), u (B,N-1,2), K (N-1,2,4)) device tensors."""
    eng = _eng()
    K = lqr_gains(x_ref, u_ref)
    x, u = eng.track_rollout(x0, x_ref, u_ref, K)
    return x, u, K


@dataclass
class LqrLanesResult:
    """LQR_tracking_lanes' result (device tensors; a field not asked for is None).  With x0 (B,4): x (B,N,4),
    u (B,N-1,2), summaries (B,); with x0 (B,P,4): x (B,P,N,4), u (B,P,N-1,2), summaries (B,P).  K (B,N-1,2,4).
    err_final = |x_{N-1} - x_opt_{N-1}|_inf, err_max = max_t |x_t - x_opt_t|_inf, u_max = max_t |u_t[1]|."""
    x: torch.Tensor | None
    u: torch.Tensor | None
    K: torch.Tensor | None
    err_final: torch.Tensor
    err_max: torch.Tensor
    u_max: torch.Tensor


def _lane_trajectories(eng, x_opt, u_opt):
    """(x_opt (B,N,4), u_opt (B,N-1,2)) on the device; u_opt with N rows is trimmed as newton_Algorithm trims u_ref
    (trajectory_generation.py:301-303), other mismatches raise."""
    x_opt = eng.t(x_opt)
    u_opt = eng.t(u_opt)
    B, N = check_lane_trajectories(x_opt, u_opt, or_n_rows=True)
    if u_opt.shape[1] == N:
        u_opt = u_opt[:, :N - 1].contiguous()
    return x_opt, u_opt


def _lane_starts(eng, x0, x_opt):
    """x0 (B,4) or (B,P,4) on the device as (B,P,4), and whether it came without the P axis."""
    B = x_opt.shape[0]
    x0 = eng.t(x0)
    check_lane_starts(x0, B, flat_ok=True)
    return x0.reshape(B, -1, 4), x0.ndim == 2


def _drop_starts_axis(flat, summary, *per_start):
    """The outputs of a closed loop of x0 (B,P,4) for an x0 that came as (B,4) (``flat``): summary (3,B,P) and the
    tensors (B,P,...) (or None) without the P axis again."""
    if not flat:
        return (summary, *per_start)
    return (summary[:, :, 0], *(None if t is None else t[:, 0] for t in per_start))


def _plant_kw(eng, plant, x0) -> dict:
    """The engine keyword of a mismatched plant for the starts x0 (B,P,4): its device table; none without one, so a
    call without ``plant`` is the call it always was."""
    return {} if plant is None else {"plant": eng.plant_table(plant, x0.shape[0], x0.shape[1])}


def _check_plant(plant, x_opt, x0):
    """``plant=`` refused before any device is needed (engine.check_plant on the caller's own shapes; the parameters
    a dict leaves out are those of the set dynamics.engine() runs on).  Malformed x_opt / x0 are left to their own
    checks."""
    xs, ss = tuple(np.shape(x_opt)), tuple(np.shape(x0))
    if plant is not None and len(xs) == 3 and len(ss) in (2, 3):
        check_plant(plant, xs[0], 1 if len(ss) == 2 else ss[1], PARAM_SETS[_dyn._pset])


def _lane_rollout(eng, ws, x0, N, trajectories, flat, plant=None):
    """The closed loop of x0 (B,P,4) on a workspace a per-lane gains call filled (gym_lqr_lanes_rollout; with
    ``plant`` gym_lqr_lanes_rollout_plant)."""
    x, u, s = eng.lqr_lanes_rollout(ws, x0, N, trajectories=trajectories, **_plant_kw(eng, plant, x0))
    s, x, u = _drop_starts_axis(flat, s, x, u)
    return x, u, s


def lqr_gains_lanes(x_opt, u_opt, Q=Q_REG, R=R_REG, QT=QT_REG) -> torch.Tensor:
    """solve_LQR_tracking (:170-203) per lane: x_opt (B,N,4), u_opt (B,N-1,2) -> K (B,N-1,2,4) on the device
    (row 0 of every gain is exactly zero: tau1 is unactuated)."""
    eng = _eng()
    x_opt, u_opt = _lane_trajectories(eng, x_opt, u_opt)
    return eng.lqr_lanes_gains(x_opt, u_opt, Q, R, QT, gains=True)[1]


def LQR_tracking_lanes(x_opt, u_opt, x0, plant=None, models=None, *, trajectories: bool = True, gains: bool = True,
                       Q=Q_REG, R=R_REG, QT=QT_REG) -> LqrLanesResult:
    """LQR tracking of every lane's OWN trajectory (main.py task_2's result into task_3, per lane): lane b's gains
    come from (x_opt[b], u_opt[b]) and its perturbed starts x0[b] ((B,4), or (B,P,4) for P starts per lane) are
    simulated in closed loop against them.  ``trajectories=False`` returns only the summaries (a Monte-Carlo run has
    no use for B P trajectories), ``gains=False`` skips the lane-major copy of K.

    ``plant`` (None: the model the gains are designed on) simulates a mismatched plant per closed loop:
    the gains stay on the design model, and only the plant step x_{t+1} = RK4(x_t, u_t) of closed loop (b, p) runs on
    plant[b][p], with the design model's dt.  It is a set number 1-3, a dict of parameter names (params.PARAM_NAMES)
    to scalars or arrays broadcastable to (B,P) (names left out: the design model's), or an array (11,), (P,11),
    (B,11), (B,1,11) or (B,P,11) in PARAM_NAMES order, e.g. ``sample_plants(B, P)``; engine.check_plant has the
    rules.  Where plant[b][p] is the design model the results of (b, p) are bit for bit the call's without
    ``plant``; a plant that drives its loop to inf or NaN shows in that loop's summaries and nowhere else.

    ``models`` (None: the engine's model on every lane) designs lane b's gains on models[b]: one
    parameter set per lane in any of engine.check_models' forms, e.g. the ``models`` of the solve that planned the
    trajectories (SolveResult.models).  Where ``plant`` is not given, closed loop (b, p) is then simulated on
    models[b] too; an explicit ``plant`` still wins."""
    _check_plant(plant, x_opt, x0)
    if models is not None and len(np.shape(x_opt)) == 3:
        models = check_models(models, np.shape(x_opt)[0], PARAM_SETS[_dyn._pset])
        if plant is None:
            plant = models[:, None, :]                     # (B,1,11): per lane for every start
    eng = _eng()
    x_opt, u_opt = _lane_trajectories(eng, x_opt, u_opt)
    x0, flat = _lane_starts(eng, x0, x_opt)
    mkw = {} if models is None else {"models": eng.model_table(models, x_opt.shape[0])}
    ws, K = eng.lqr_lanes_gains(x_opt, u_opt, Q, R, QT, gains=gains, **mkw)
    x, u, s = _lane_rollout(eng, ws, x0, x_opt.shape[1], trajectories, flat, plant)
    return LqrLanesResult(x, u, K, s[0], s[1], s[2])


def sample_plants(B: int, P: int, rel: float = 0.05, names=("m1", "m2", "I1", "I2", "f1", "f2"), seed: int = 0,
                  base=None) -> np.ndarray:
    """Plant parameters for a robustness Monte Carlo, (B,P,11) in params.PARAM_NAMES order, to pass as ``plant=``:
    each named parameter of ``base`` (a dict; default: set 1) times 1 + U(-rel, rel), independent per (b, p) and
    parameter, from numpy.random.default_rng(seed); parameters not named are base's own."""
    base = PARAM_SETS[1] if base is None else base
    unknown = [n for n in names if n not in PARAM_NAMES]
    if unknown:
        raise ValueError(f"unknown plant parameter {unknown[0]!r}: the names are {', '.join(PARAM_NAMES)}")
    out = np.empty((int(B), int(P), 11))
    out[:] = [float(base[k]) for k in PARAM_NAMES]
    rng = np.random.default_rng(seed)
    for n in names:
        out[:, :, PARAM_NAMES.index(n)] *= 1.0 + rng.uniform(-rel, rel, (int(B), int(P)))
    return out


def mpc_gains(x_ref, u_ref, T_pred: int = T_PRED, Q=Q_MPC, R=R_MPC, n_steps: int | None = None):
    """K_0(t) (n_steps, 2, 4) of every control step of solve_mpc_tracking, and Q_T = P_inf (:8-69)."""
    eng = _eng()
    x_ref = eng.t(x_ref).reshape(-1, 4)
    u_ref = eng.t(u_ref).reshape(-1, 2)
    S = x_ref.shape[0] - 1                                          # A_list: one stage per u_ref row (:19)
    n_steps = S if n_steps is None else int(n_steps)
    x_f, u_f = _final_state(eng)
    if int(T_pred) + 2 <= MPC_FUSED_MAX_STAGES:
        # one launch: stage linearisations, compute_P_inf and every window's recursion (gym_mpc_gains)
        K0, QT, _ = eng.mpc_gains(x_ref, u_ref, x_f, u_f, Q, R, L=int(T_pred), nwin=n_steps)
        return K0, QT
    A_c, B_c = eng.jacobians(x_ref[:S], u_ref[:S])
    Af_c, Bf_c = eng.jacobians(x_f, u_f)
    A_f, B_f = _discrete(eng, Af_c[0], Bf_c[0])
    QT, _ = eng.dare_fixed_point(A_f, B_f, Q, R)
    K0 = eng.tv_lqr_gains(A_c, B_c, Q, R, QT, L=int(T_pred), nwin=n_steps, all_gains=False,
                          A_pad=Af_c[0], B_pad=Bf_c[0], discretize=True)
    return K0, QT


def _mpc_terminal_weight(eng, Q, R) -> torch.Tensor:
    """Q_T = compute_P_inf on the pad (x_f, u_f) (:31-38) as a device tensor, made by gym_mpc_gains itself once per
    engine (its model and dt enter the pad's linearisation) and (Q, R): Q_T depends on neither the reference nor
    T_pred, so this is bit for bit the QT that ``mpc_gains`` returns on the same engine for the same Q, R, and no
    per-lane call computes or reads it back.  The cached tensor stays private: callers are handed a copy."""
    key = (np.asarray(Q, dtype=np.float64).tobytes(), np.asarray(R, dtype=np.float64).tobytes())
    if key not in eng.mpc_qt_cache:
        x_f, u_f = _final_state(eng)
        eng.mpc_qt_cache[key] = eng.mpc_gains(torch.cat([x_f, x_f]), u_f, x_f, u_f, Q, R, L=2, nwin=1)[1]
    return eng.mpc_qt_cache[key]


def mpc_gains_lanes(x_opt, u_opt, T_pred: int = T_PRED, Q=Q_MPC, R=R_MPC):
    """``mpc_gains`` per lane: x_opt (B,N,4), u_opt (B,N-1,2) -> (K0 (B,N-1,2,4), QT (4,4)) on the device.  K0[b, t]
    is the exact solution of solve_mpc_tracking's QP (:8-69, no torque limit) at control step t of lane b's own
    trajectory (row 0 of every gain is exactly zero: tau1 is unactuated); QT is ``mpc_gains``' bit for bit."""
    eng = _eng()
    x_opt, u_opt = _lane_trajectories(eng, x_opt, u_opt)
    QT = _mpc_terminal_weight(eng, Q, R)
    return eng.mpc_lanes_gains(x_opt, u_opt, Q, R, QT, int(T_pred), gains=True)[1], QT.clone()


@dataclass
class MpcLanesResult(LqrLanesResult):
    """MPC_tracking_lanes' result: LqrLanesResult's fields (K = the windows' first gains K0 (B,N-1,2,4)) and QT (4,4),
    the terminal weight compute_P_inf gives on the pad (a device tensor, the caller's own copy)."""
    QT: torch.Tensor


@dataclass
class MpcBoxLanesResult(MpcLanesResult):
    """MPC_tracking_lanes' result with a torque limit: MpcLanesResult's fields (K = the windows' unconstrained first
    gains, the first iterate of every QP), unconverged (B,P) int32 = the QPs of that closed loop that reached
    ``max_qp_iters`` without settling (their clipped last iterate was applied), and qp_iters (B,P,N-1) int32
    active-set sweeps per QP (None with ``trajectories=False``).  An x0 of shape (B,4) drops the P axis of both.
    With ``tau_max=TorqueLimit(...)``: qp_iters = active-set sweeps + Newton iterations of the fallback
    (> max_qp_iters exactly when it ran), unconverged = the QPs that neither phase finished."""
    unconverged: torch.Tensor
    qp_iters: torch.Tensor | None


def MPC_tracking_lanes(x_opt, u_opt, x0, plant=None, *, trajectories: bool = True, gains: bool = True,
                       T_pred: int = T_PRED, Q=Q_MPC, R=R_MPC, tau_max=None, max_qp_iters: int = 32) -> MpcLanesResult:
    """Receding-horizon MPC tracking of every lane's OWN trajectory (main.py task_2's result into task_4, per lane;
    solve_mpc_tracking :8-69): lane b's first gains come from the T_pred-stage windows along (x_opt[b], u_opt[b]) and
    its perturbed starts x0[b] ((B,4), or (B,P,4) for P starts per lane) are simulated in closed loop against them.
    Shapes, ``trajectories`` and ``gains`` as LQR_tracking_lanes.

    ``tau_max`` (None: the reference's default, no limit) is solver_mpc's torque limit (test_constraints, :87-114;
    the reference uses 18): every stage of every window obeys |u_opt[b][t] + u_t| <= tau_max, so every control step
    of every closed loop owns an inequality-constrained QP, solved by the active set of the shared-reference path
    (at most ``max_qp_iters`` sweeps each) in the kernel of csrc/mpc_box_lanes.hpp (gym_mpc_box_lanes_rollout; DESIGN
    4.7).  Returns an MpcBoxLanesResult then; where no bound is ever active its x, u and summaries are the
    unlimited call's bit for bit.  ``tau_max=TorqueLimit(18.0)`` adds the projected-Newton fallback to every QP:
    qp_iters then counts both phases and unconverged only the QPs that neither phase finished.

    ``plant`` as LQR_tracking_lanes, for every ``tau_max`` form: the windows, the pad, Q_T, the QPs and the torque
    limit stay on the design model, the plant step of closed loop (b, p) runs on plant[b][p]; summaries, qp_iters
    and unconverged keep their meaning."""
    tau_max, fb = _torque_limit(tau_max)
    if tau_max is not None:
        _check_box(tau_max, T_pred, max_qp_iters, fb)
    _check_plant(plant, x_opt, x0)
    eng = _eng()
    x_opt, u_opt = _lane_trajectories(eng, x_opt, u_opt)
    x0, flat = _lane_starts(eng, x0, x_opt)
    QT = _mpc_terminal_weight(eng, Q, R)
    if tau_max is None:
        ws, K = eng.mpc_lanes_gains(x_opt, u_opt, Q, R, QT, int(T_pred), gains=gains)
        x, u, s = _lane_rollout(eng, ws, x0, x_opt.shape[1], trajectories, flat, plant)
        return MpcLanesResult(x, u, K, s[0], s[1], s[2], QT.clone())
    K = eng.mpc_lanes_gains(x_opt, u_opt, Q, R, QT, int(T_pred), gains=True)[1] if gains else None
    x, u, s, it, unconv = eng.mpc_box_lanes_rollout(x_opt, u_opt, x0, Q, R, QT, int(T_pred), float(tau_max),
                                                    int(max_qp_iters), trajectories=trajectories, **_fb_kw(fb),
                                                    **_plant_kw(eng, plant, x0))
    s, x, u, it, unconv = _drop_starts_axis(flat, s, x, u, it, unconv)
    return MpcBoxLanesResult(x, u, K, s[0], s[1], s[2], QT.clone(), unconv, it)


def solve_mpc_tracking_batch(x0, x_ref, u_ref, T_pred: int = T_PRED):
    """Batched receding-horizon MPC: x0 (B,4) -> (x_real (B,N,4), u_real (B,N-1,2), K0 (N-1,2,4))."""
    eng = _eng()
    K0, _ = mpc_gains(x_ref, u_ref, T_pred)
    x, u = eng.track_rollout(x0, x_ref, u_ref, K0)
    return x, u, K0


@dataclass
class MpcBoxResult:
    """solve_mpc_tracking_box_batch's result (device tensors): x (B,N,4), u (B,N-1,2), K0 (N-1,2,4) the
    unconstrained first gains, qp_iters (B,N-1) int32 active-set sweeps per QP, unconverged (B,) int32 QPs per lane
    that reached max_qp_iters without settling.  With ``tau_max=TorqueLimit(...)``: qp_iters = active-set sweeps +
    Newton iterations of the fallback (> max_qp_iters exactly when it ran), unconverged = the QPs that neither phase
    finished."""
    x: torch.Tensor
    u: torch.Tensor
    K0: torch.Tensor
    qp_iters: torch.Tensor
    unconverged: torch.Tensor


def _check_box(tau_max, T_pred, max_qp_iters, fallback_iters=0):
    """The torque-limited paths' arguments, refused before any device is needed (the engine's own checks)."""
    check_box(tau_max, max_qp_iters, fallback_iters)
    check_window(T_pred, "the torque-limited QP")


def solve_mpc_tracking_box_batch(x0, x_ref, u_ref, tau_max: float = TAU_MAX, T_pred: int = T_PRED,
                                 max_qp_iters: int = 32, Q=Q_MPC, R=R_MPC) -> MpcBoxResult:
    """Batched receding-horizon MPC with the torque limit |u_ref + u| <= tau_max on every stage of every window
    (solve_mpc_tracking :8-69 with solver_mpc's test_constraints on): x0 (B,4) -> MpcBoxResult.  tau_max: a number,
    or a TorqueLimit for the projected-Newton fallback (MpcBoxResult says what qp_iters and unconverged mean then)."""
    tau_max, fb = _torque_limit(tau_max)
    _check_box(tau_max, T_pred, max_qp_iters, fb)
    eng = _eng()
    x_ref = eng.t(x_ref).reshape(-1, 4)
    u_ref = eng.t(u_ref).reshape(-1, 2)
    x_f, u_f = _final_state(eng)
    K_all, QT, _ = eng.mpc_gains_all(x_ref, u_ref, x_f, u_f, Q, R, L=int(T_pred), nwin=x_ref.shape[0] - 1)
    x, u, it, unconv = eng.mpc_box_rollout(x0, x_ref, u_ref, x_f, u_f, Q, R, QT, K_all, float(tau_max),
                                           int(max_qp_iters), **_fb_kw(fb))
    return MpcBoxResult(x, u, K_all[:, 0].contiguous(), it, unconv)


def solve_mpc_tracking(x0, x_ref, u_ref, T, T_pred: int = T_PRED, tau_max=None):
    """trajectory_tracking.py:8-69 -> (x_real (N,4), u_real (N-1,2)); control steps t < T-1.  tau_max: the torque
    limit of solver_mpc's test_constraints path (None: the reference's default, no limit; a TorqueLimit: with the
    projected-Newton fallback for QPs whose active set does not settle)."""
    x_ref = np.asarray(x_ref, dtype=float)
    u_ref = np.asarray(u_ref, dtype=float)
    steps = int(T) - 1
    x_real = np.zeros(x_ref.shape)
    u_real = np.zeros(u_ref.shape)
    x0 = np.asarray(x0, dtype=float).reshape(1, 4)
    if tau_max is not None:
        res = solve_mpc_tracking_box_batch(x0, x_ref, u_ref, tau_max, T_pred)
        x, u = res.x, res.u
    else:
        x, u, _ = solve_mpc_tracking_batch(x0, x_ref, u_ref, T_pred)
    x_real[:steps + 1] = _np(x[0])[:steps + 1]
    u_real[:steps] = _np(u[0])[:steps]
    return x_real, u_real


def solver_mpc(x0, A_list, B_list, Q, R, Q_T, T_pred, u_ref=None, tau_max=None):
    """trajectory_tracking.py:73-140: the window's QP solved exactly -> (U0 (2,), X_opt (T_pred,4),
    U_opt (T_pred,2)); U_opt's last row (no cost, no constraint in the reference's QP) is 0.  tau_max: the torque
    limit -tau_max <= u_t + u_ref_t <= tau_max of the test_constraints path (:87-114; needs u_ref, as the reference
    does); None: no limit; a TorqueLimit: a QP whose active set does not settle in 32 sweeps goes on by projected
    Newton, and the warning is printed only if that does not finish either."""
    eng = _eng()
    tau_max, fb = _torque_limit(tau_max)
    if tau_max is not None:
        if u_ref is None:
            raise ValueError("solver_mpc needs u_ref to apply tau_max (the limit is on u_t + u_ref_t)")
        _check_box(tau_max, T_pred, 32, fb)
        Lw = int(T_pred)
        A = np.asarray(A_list[:Lw - 1], dtype=float).reshape(-1, 4, 4)
        B = np.asarray(B_list[:Lw - 1], dtype=float).reshape(-1, 4, 2)
        ur = np.asarray(u_ref, dtype=float).reshape(-1, 2)[:Lw - 1]
        U, X, _, conv = eng.mpc_box_qp(A, B, ur, Q, R, Q_T, np.asarray(x0, dtype=float).reshape(1, 4), Lw,
                                       float(tau_max), **_fb_kw(fb))
        if not int(conv[0].item()):
            print("Attention! mpc solver did not settle its active set: clipped last iterate returned")
        U_opt = np.zeros((Lw, 2))
        U_opt[:-1] = _np(U[0])
        return U_opt[0].copy(), _np(X[0]), U_opt
    A = eng.t(np.asarray(A_list[:T_pred], dtype=float)).reshape(-1, 4, 4)
    B = eng.t(np.asarray(B_list[:T_pred], dtype=float)).reshape(-1, 4, 2)
    K = eng.tv_lqr_gains(A, B, Q, R, Q_T, L=int(T_pred), nwin=1, all_gains=True,
                         A_pad=A[-1], B_pad=B[-1], discretize=False)
    X, U = eng.lq_forward(A, B, K, np.asarray(x0, dtype=float).reshape(4), int(T_pred), A_pad=A[-1], B_pad=B[-1])
    U_opt = np.zeros((int(T_pred), 2))
    U_opt[:-1] = _np(U)
    return U_opt[0].copy(), _np(X), U_opt
