"""What a batched Newton solve returns and what it continues from: SolveResult (with its .npz writer and the
tracking front ends on its lanes), Checkpoint and load_checkpoint; ClosedLoopResult, what
BatchedNewtonSolver.closed_loop returns.  Host I/O and dataclasses only."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .params import DT


@dataclass
class SolveResult:
    x: torch.Tensor          # (B,N,4)
    u: torch.Tensor          # (B,T,2)
    K: torch.Tensor          # (B,T,2,4)  gains of each lane's last iteration
    sigma: torch.Tensor      # (B,T,2)
    cost: torch.Tensor       # (B,)
    n_iter: torch.Tensor     # (B,) outer iterations executed (incl. a final failed one)
    status: torch.Tensor     # (B,) _lib.CONVERGED / LS_FAILED / MAX_ITERS
    n_rollouts: torch.Tensor # (B,)
    gamma: torch.Tensor      # (B,) last accepted step
    iterations: int          # outer loop iterations run for the whole batch
    lane_iterations: int     # sum of n_iter over lanes (the throughput numerator)
    seconds: float           # wall time of the solve loop (init + iterations + finalize)
    stats_log: list = field(default_factory=list)
    hist_cost: torch.Tensor | None = None   # (hist_len, B)
    hist_smax: torch.Tensor | None = None   # (hist_len, B)
    x_trajs: dict | None = None             # {lane: [x_0, x_1, ...]} of the captured lanes (capture_lanes)
    cost0: dict | None = None               # {lane: J_0} of the captured lanes
    sigmas: dict | None = None              # {lane: {iteration: sigma (T,2)}} of the captured lanes (capture_sigma)
    schedule: str = ""                      # "serial" | "pipelined" | "persistent"
    tail_lane_iterations: int = 0           # lane-iterations run by the straggler tail (gym_newton_tail)
    compactions: int = 0                    # lane compactions during the loop (BatchedNewtonSolver.compact)
    lowocc_lane_iterations: int = 0         # lane-iterations run in the low-occupancy regime (maybe_compact)
    tail_from_iteration: int | None = None  # the outer iteration the straggler tail took over at (None: no tail)
    tail_iterations: int = 0                # outer iterations the tail ran (its slowest lane's, up to the last one)
    tau_max: torch.Tensor | None = None     # (B,) per-lane torque limits of a limited solve (None: no limit)
    linearization: str = "euler"            # the sweep's linearisation: "euler" (the reference's) or "rk4"
    models: np.ndarray | None = None        # (B,11) host: the parameter set each lane was planned on (None: the engine's)
    weights: np.ndarray | None = None       # (B,10) host: Q[4], R[2], QT[4] each lane was planned under (None: the engine's)

    def save_npz(self, path, t=None, dt: float = DT):
        """Write the per-lane results as one .npz in the reference's wire format (main.py:74-79, np.savez(x=, u=,
        t=)): x (B,N,4), u (B,T,2), t (N,) = arange(N) * dt unless given, plus cost, status, n_iter, gamma,
        n_rollouts, K and sigma, which load_checkpoint / BatchedNewtonSolver.resume continue from, and
        ``linearization`` where it is not the reference's "euler" (a file without it is an Euler solve's) and
        ``models`` (B,11) where the lanes were planned on their own (a file without it: on the engine's) and likewise
        ``weights`` (B,10) where they were planned under their own.  Host I/O only: tensors on any device."""
        a = {k: getattr(self, k).detach().cpu().numpy() for k in CHECKPOINT_KEYS}
        if self.linearization != "euler":
            a["linearization"] = np.array(self.linearization)
        if self.models is not None:
            a["models"] = np.asarray(self.models, dtype=np.float64)
        if self.weights is not None:
            a["weights"] = np.asarray(self.weights, dtype=np.float64)
        N = a["x"].shape[1]
        a["t"] = np.arange(N) * float(dt) if t is None else np.asarray(t, dtype=np.float64)
        if a["t"].shape != (N,):
            raise ValueError(f"t must hold the {N} knot times, got {a['t'].shape}")
        np.savez(path, **a)

    def _track_starts(self, x0, dx0):
        """The perturbed starts of track_lqr / track_mpc: x0 itself, or x[:, 0] + dx0 with dx0 (4,), (B,4) or (B,P,4)
        (default: no perturbation)."""
        if x0 is not None and dx0 is not None:
            raise ValueError("give x0 or dx0, not both")
        if x0 is not None:
            return x0
        start = self.x[:, 0]
        if dx0 is None:
            return start
        d = torch.as_tensor(np.asarray(dx0.detach().cpu() if isinstance(dx0, torch.Tensor) else dx0, dtype=np.float64),
                            device=start.device)
        B = start.shape[0]
        if tuple(d.shape) == (4,) or tuple(d.shape) == (B, 4):
            return start + d
        if d.ndim == 3 and d.shape[0] == B and d.shape[2] == 4:
            return start[:, None, :] + d
        raise ValueError(f"dx0 must be (4,), ({B},4) or ({B},P,4), got {tuple(d.shape)}")

    def track_lqr(self, x0=None, dx0=None, **kw):
        """LQR tracking of every lane's own result (trajectory_tracking.LQR_tracking_lanes on this result's x, u):
        x0 (B,4) or (B,P,4) perturbed starts, default x[:, 0] + dx0 with dx0 (4,), (B,4) or (B,P,4) (default: no
        perturbation).  Keyword arguments go to LQR_tracking_lanes, ``plant=`` among them: a mismatched plant per closed
        loop, e.g. ``plant=trajectory_tracking.sample_plants(B, P)`` for dx0 (B,P,4).  A result planned on per-lane
        models passes them on (``models=self.models`` unless given): every lane's gains are designed on, and without
        ``plant=`` its closed loops simulated on, the model it was planned for.  Returns its LqrLanesResult."""
        from . import trajectory_tracking as tt
        kw.setdefault("models", self.models)
        return tt.LQR_tracking_lanes(self.x, self.u, self._track_starts(x0, dx0), **kw)

    def track_mpc(self, x0=None, dx0=None, **kw):
        """Receding-horizon MPC tracking of every lane's own result (trajectory_tracking.MPC_tracking_lanes on this
        result's x, u); x0 / dx0 as track_lqr.  Keyword arguments (T_pred, Q, R, trajectories, gains, tau_max,
        max_qp_iters, plant) go to MPC_tracking_lanes; ``plant=`` simulates a mismatched plant per closed loop, with
        and without a torque limit.  Returns its MpcLanesResult; with a torque limit (``tau_max=18`` is the
        reference's) every lane's closed loop keeps |u| <= tau_max and the result is an MpcBoxLanesResult.
        ``tau_max=trajectory_tracking.TorqueLimit(18.0)`` adds the projected-Newton fallback: a QP whose active set
        has not settled after max_qp_iters sweeps is finished by it, qp_iters counts both phases and unconverged only
        the QPs that neither phase finished.  The MPC trackers design on the engine's model only: on a result planned
        on per-lane models this raises NotImplementedError unless ``models=None`` is passed to say that the engine's
        model is meant."""
        from . import trajectory_tracking as tt
        if "models" in kw:
            if kw.pop("models") is not None:
                raise NotImplementedError("per-lane MPC tracking designs on the engine's model only; use track_lqr "
                                          "for a design per lane")
        elif self.models is not None:
            raise NotImplementedError(
                "this result was planned on per-lane models and the MPC trackers design on the engine's model only: "
                "use track_lqr (which designs each lane on its own model), or pass models=None to track_mpc to say "
                "that the engine's model is meant")
        return tt.MPC_tracking_lanes(self.x, self.u, self._track_starts(x0, dx0), **kw)


@dataclass
class ClosedLoopResult:
    """One closed loop per lane under receding-horizon replanning (BatchedNewtonSolver.closed_loop)."""
    x: torch.Tensor          # (B,N,4)  applied states (n_steps < T: rows 0 .. n_steps, the rest zero)
    u: torch.Tensor          # (B,T,2)  applied controls
    iters: torch.Tensor      # (B,T) int32  iterations of each step's replan
    rollouts: torch.Tensor   # (B,T) int32  rollouts of each step (Armijo trials, and the re-anchor's one)
    stop: torch.Tensor       # (B,T) int32  _lib.ACTIVE (all iterations ran) / CONVERGED / LS_FAILED per step
    cost: torch.Tensor       # (B,T)  cost-to-go after each step's replan
    err_final: torch.Tensor  # (B,)   max |x[:, -1] - x_ref[-1]|, the lane's own reference row
    u_max: torch.Tensor      # (B,)   largest |torque| applied
    tau_max: torch.Tensor | None = None     # (B,) per-lane torque limits as given (None: no limit)
    plant: np.ndarray | None = None         # (B,11) host: the plant each loop ran on (None: the design model)
    n_steps: int = 0                        # control steps taken


CHECKPOINT_KEYS = ("x", "u", "cost", "status", "n_iter", "gamma", "n_rollouts", "K", "sigma")


@dataclass
class Checkpoint:
    """Per-lane iterates to continue from (load_checkpoint): SolveResult's per-lane fields and the knot times."""
    x: torch.Tensor          # (B,N,4)
    u: torch.Tensor          # (B,T,2)
    t: torch.Tensor          # (N,)
    cost: torch.Tensor       # (B,)   NaN where the file had none
    status: torch.Tensor     # (B,)   int32
    n_iter: torch.Tensor     # (B,)   int32
    gamma: torch.Tensor      # (B,)
    n_rollouts: torch.Tensor # (B,)   int32
    K: torch.Tensor          # (B,T,2,4)
    sigma: torch.Tensor      # (B,T,2)
    linearization: str = "euler"   # the sweep the iterates come from; resume() on a solver of the other is refused
    models: np.ndarray | None = None   # (B,11) per-lane parameter sets of the solve; resume() needs the same bits
    weights: np.ndarray | None = None  # (B,10) per-lane cost weights of the solve; resume() needs the same bits


def load_checkpoint(path, device="cpu") -> Checkpoint:
    """Read a checkpoint written by SolveResult.save_npz -- or a trajectory file of the reference itself
    (acrobot_optimal_trajectory.npz: x (N,4), u (N-1 or N,2) without a lane axis, t, nothing else), which loads as a
    one-lane checkpoint with the lane ACTIVE, n_iter = 0 and no gains.  Tensors go to ``device``."""
    with np.load(path) as d:
        a = {k: d[k] for k in d.files}
    for k in ("x", "u"):
        if k not in a:
            raise ValueError(f"{path}: not a trajectory file (no '{k}')")
    x, u = np.asarray(a["x"], dtype=np.float64), np.asarray(a["u"], dtype=np.float64)
    if x.ndim == 2 and u.ndim == 2:
        x, u = x[None], u[None]
    if x.ndim != 3 or x.shape[2] != 4 or u.ndim != 3 or u.shape[2] != 2 or u.shape[0] != x.shape[0]:
        raise ValueError(f"{path}: x {x.shape} / u {u.shape} are not (B,N,4) / (B,T,2) trajectories")
    B, N = x.shape[:2]
    if u.shape[1] == N:          # a control row per knot: the last one is unused (trajectory_generation.py:301-303)
        u = u[:, :-1]
    if u.shape[1] != N - 1:
        raise ValueError(f"{path}: x has {N} knots but u has {u.shape[1]} controls (expected {N - 1})")
    T = N - 1
    full = {"x": x, "u": np.ascontiguousarray(u),
            "t": np.asarray(a["t"], dtype=np.float64) if "t" in a else np.arange(N) * DT,
            "cost": np.full(B, np.nan), "status": np.full(B, _lib.ACTIVE, np.int32), "n_iter": np.zeros(B, np.int32),
            "gamma": np.zeros(B), "n_rollouts": np.zeros(B, np.int32), "K": np.zeros((B, T, 2, 4)),
            "sigma": np.zeros((B, T, 2))}
    for k in CHECKPOINT_KEYS[2:]:
        if k in a:
            v = np.asarray(a[k], dtype=full[k].dtype)
            if v.shape != full[k].shape:
                raise ValueError(f"{path}: '{k}' has shape {v.shape}, expected {full[k].shape}")
            full[k] = v
    return Checkpoint(**{k: torch.as_tensor(v).to(device) for k, v in full.items()},
                      linearization=str(a["linearization"]) if "linearization" in a else "euler",
                      models=_ckpt_table(a, "models", (B, 11), path), weights=_ckpt_table(a, "weights", (B, 10), path))


def _ckpt_table(a, key, shape, path):
    """A per-lane host table of a checkpoint file (models, weights), or None where the file has none."""
    if key not in a:
        return None
    m = np.ascontiguousarray(a[key], dtype=np.float64)
    if m.shape != shape:
        raise ValueError(f"{path}: '{key}' has shape {m.shape}, expected {shape}")
    return m
