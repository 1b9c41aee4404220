"""Batched Newton / Armijo swing-up solver on the HIP engine (newton_Algorithm, batched).

Reference semantics, per lane (trajectory_generation.py:298-398):
  * u_ref trimmed to N-1 rows if it has N (:301-303); ValueError on other mismatches (:305-306);
  * u_0 = 0 and x_0 = open-loop rollout (:311-312); J_0 = total_cost (:319);
  * each iteration: backward sweep -> K, sigma, dJ (:332-338); Armijo gamma_0, gamma_0*beta, ...
    with the strict test J_new < J + c*gamma*dJ (:352-365), at most ``max_ls`` = 20 trials;
  * LS failure: stop without update (:367-369); otherwise update, then stop if max|sigma| < tol
    (:383-396).
The batch runs every lane in lock-step on the device.  Trial 1 is fused with its rollout; lanes
that reject it evaluate trials 2..max_ls *in parallel* (one thread per candidate) and re-run the
first accepted one -- the same decision the sequential search makes.

Schedules: ``serial`` launches the backward sweep and the trial of all lanes one after the other
(gym_newton_iteration); ``pipelined`` splits the lanes into two halves offset by one phase and runs
one half's (HBM-bound) sweep beside the other half's (fp64-VALU-bound) trial in a single launch
(gym_newton_phase); ``persistent`` runs every lane's iterations back to back inside one launch per
``chunk`` iterations (gym_newton_run): lanes are independent problems, so no grid-wide step separates
one iteration from the next.  Per lane the arithmetic is identical; only the overlap differs.

Streams per stage: the sweep reads x (2 pairs) + u (2 planes) and writes K row 1 (2 pairs) +
(c1, sigma1); the trial reads those + u0 and writes x_new, u_new.  When u_ref[:,0] == 0 (the headline
task-2 reference) the unactuated tau1 controls are identically zero and their planes are skipped.

Multi-GPU: one process per GPU, each owning a contiguous shard of lanes; the only cross-GPU
traffic is one all-reduce (SUM) of the 8 per-iteration statistics (see distributed.py).

This file holds the solver; what a solve returns and continues from is results.py, the host loops host_loop.py,
placement selection and its pool placement.py.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, placement
from .engine import AcrobotEngine, check_models, check_weights, padded, F64
from .host_loop import STAT_FIELDS, morton_order, newton_loop, run_loop, tail_loop  # noqa: F401
from .params import MAX_LINE_SEARCH_ITERS
from .placement import PlacementPool
from .results import CHECKPOINT_KEYS, Checkpoint, ClosedLoopResult, SolveResult, load_checkpoint  # noqa: F401

# _launch arguments of a size query: plain sizes in, a count out; no structure, no stream
_SIZES = dict(model=False, batch=False, stream=False)


class _Kind(NamedTuple):
    """The kind of solve a solver runs (_set_limited chooses it): ``limited`` names a limited kind in messages (None:
    the plain solve), then the entry points of its persistent run, sigma re-run, cold and warm start; ``table``:
    these take a per-lane table (and one entry point starts cold and warm): "models", the model table after the model,
    or "weights", the weight table after the weights."""
    limited: str | None = None
    run: str = "gym_newton_run"
    sigma: str = "gym_newton_sigma"
    init: str = "gym_newton_init"
    init_warm: str = "gym_newton_init_warm"
    table: str | None = None


class BatchedNewtonSolver:
    """Owns the device buffers of a batch of ``B`` lanes that share x_ref / u_ref."""

    # The pipelined schedule pays off once the batch holds two wavefronts per SIMD: with the round-2 kernels
    # serial is ahead by 2% at 73,728 and 81,920 lanes and by 1% at 98,304, the two are level (+-1%, box
    # dependent) from 131,072 to 327,680 (same-box sweeps, profiles/r02_sched_sweep_large.log; round 1's
    # kernels crossed at ~81,920, profiles/r01_batch_sweep.log).  In lanes per compute unit (4 SIMDs x 64 x 2).
    PIPELINE_MIN_LANES_PER_CU = 512
    # The persistent schedule (one launch per solve: no per-iteration launches, statistics or host round trips)
    # is ahead while the batch is latency-bound and fits in one round of its workgroups: k_nt_run2 holds 64 lanes
    # on four wavefronts and ~98 KiB of LDS, one workgroup per CU.  Round 6, same box (profiles/r06/sched/):
    # persistent 28.95 M it/s against serial 17.16 at 16,384 lanes (64 per CU), but 22.94 / 24.60 at 24,576 and
    # 29.40 / 32.19 at 32,768, where CUs take a second workgroup (round 2's threshold of 128 per CU predates the
    # kernel's LDS ring).
    PERSISTENT_MAX_LANES_PER_CU = 64
    # The straggler tail (gym_newton_tail: one workgroup per lane, every Armijo trial at once) takes over the serial /
    # pipelined loop once at most this many lanes per CU (of all ranks) are still active: one wavefront per lane, so up
    # to one per SIMD it runs each lane's iteration at the latency of one sweep pass plus one trial chain.
    TAIL_LANES_PER_CU = 4
    # Placement selection (placement.py says why and how): up to PLACEMENT_CANDIDATES stream sets are ranked at
    # construction, the PLACEMENT_TRIALS best raced in the first solve in blocks of PLACEMENT_BLOCK iterations; the
    # extra sets take at most PLACEMENT_MEM_SHARE of the device.  Eight candidates leave one selection in ~25 without
    # a fast set, four one in 5 (profiles/r06/layout/).
    PLACEMENT_CANDIDATES = 8
    PLACEMENT_TRIALS = 3
    PLACEMENT_MEM_SHARE = 0.45
    PLACEMENT_BLOCK = 12
    # Candidate slots of the post-trial Armijo search (gym_batch.cand_scratch): 32,768 (0.79 GB at T = 500) cover
    # 1,724 backtracking lanes at max_ls = 20; a hard solve's iterations mostly have 0-30 (tools/retry_counts.py).
    CAND_SLOTS = 32768

    @staticmethod
    def pipeline_min_lanes(device) -> int:
        n_cu = torch.cuda.get_device_properties(device).multi_processor_count
        return BatchedNewtonSolver.PIPELINE_MIN_LANES_PER_CU * n_cu

    @staticmethod
    def persistent_max_lanes(device) -> int:
        n_cu = torch.cuda.get_device_properties(device).multi_processor_count
        return BatchedNewtonSolver.PERSISTENT_MAX_LANES_PER_CU * n_cu

    def __init__(self, engine: AcrobotEngine, x_ref, u_ref, B: int, tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0,
                 max_ls: int = MAX_LINE_SEARCH_ITERS, hist_len: int = 0, pipeline: bool | None = None,
                 u0_zero: bool | None = None, checkpoint: bool = False, persistent: bool | None = None,
                 chunk: int = 128, reorder: bool = True, schedule_lanes: int | None = None,
                 capture_lanes=None, capture_every: int = 1, split_waves: bool = True,
                 capture_sigma=(0, 1, 2), tail_lanes: int | None = None, tail_chunk: int = 128,
                 compact: bool | None = None, world_size: int = 1, cand_slots: int | None = None,
                 arena=False, placement_trials: int | None = None, tau_max=None,
                 linearization: str = "euler", models=None, weights=None):
        if B <= 0:
            raise ValueError("batch must hold at least one lane")
        engine.weights.require_gain_solvable()
        self.eng = engine
        self._set_refs(x_ref, u_ref, B, checkpoint)
        self.armijo = _lib.GymArmijo(float(tol), float(beta), float(c), float(gamma_0), int(max_ls),
                                     1 if hist_len > 0 else 0)
        if max_ls < 1:
            raise ValueError("max_ls must be >= 1")
        self._set_u0_flag(u0_zero)
        auto_schedule = pipeline is None and persistent is None
        pipeline, persistent = self._set_limited(tau_max, linearization, models, weights, pipeline, persistent,
                                                 checkpoint)
        self._choose_schedule(pipeline, persistent, schedule_lanes, checkpoint, chunk, reorder, split_waves)
        self._set_capture(capture_lanes, capture_every, capture_sigma)
        st, placement_trials = self._alloc_streams(arena, placement_trials, auto_schedule)
        self._alloc_lane_buffers(max_ls, hist_len)
        self._fill_batch()
        self._set_streams(st)
        self._set_eligibility(auto_schedule, tail_lanes, tail_chunk, compact, world_size, cand_slots)
        self.k, self.max_iters, self.lane_order = 0, None, None
        self.lane_order_live = False   # True inside solve(), whose results follow lane_order back
        self._serial_now = self._run_now = False
        self.timeline = None    # diagnostics: a list records (iterations, active lanes, host time) per sync
        self.timing = None
        self.launches = {"phase": 0, "run": 0, "tail": 0, "iteration": 0}   # launches since reset_timing()
        self._reset_solve_counters()
        if self.placement is not None:            # a pooled set: back to the pool when this solver goes
            placement.lease(self, self._pool_key, self.placement)
        elif placement_trials > 1 and self.pipeline and not self.persistent:
            self._arm_placement(placement_trials)

    # --- the steps of __init__ -------------------------------------------------------------
    def _set_refs(self, x_ref, u_ref, B, checkpoint):
        """The references on the device and the batch's sizes B, Bp, N, T."""
        self.x_ref, self.u_ref = self.eng.refs(x_ref, u_ref, per_lane=True)
        self.B, self.Bp = int(B), padded(int(B))
        self.N = int(self.x_ref.shape[-2])
        self.T = self.N - 1
        # per-lane references (x_ref (B,N,4), u_ref (B,T,2); GYM_FLAG_REF_LANE): every schedule, no state
        # checkpointing
        self.ref_lane = self.x_ref.ndim == 3
        if self.ref_lane:
            if self.x_ref.shape[0] != self.B:
                raise ValueError(f"per-lane references must hold {self.B} lanes, got {self.x_ref.shape[0]}")
            if checkpoint:
                raise ValueError("per-lane references do not combine with state checkpointing")
            pad = self.Bp - self.B                     # padding lanes read valid rows (the last lane's)
            self._xr_in, self._ur_in = self.x_ref, self.u_ref
            self.xr_buf = torch.cat([self.x_ref, self.x_ref[-1:].expand(pad, -1, -1)]).contiguous()
            self.ur_buf = torch.cat([self.u_ref, self.u_ref[-1:].expand(pad, -1, -1)]).contiguous()

    def _set_u0_flag(self, u0_zero):
        # tau1 is unactuated (dynamics.py:205); with u_ref[:,0] == 0 its controls stay exactly 0 and the
        # kernels skip their planes (GYM_FLAG_U0_ZERO) -- bit-identical results, 24 B/stage less traffic
        ref_u0_zero = bool((self.u_ref[..., 0] == 0).all().item())
        if u0_zero and not ref_u0_zero:
            raise ValueError("u0_zero=True requires u_ref[:, 0] == 0")
        self.u0_zero = ref_u0_zero if u0_zero is None else bool(u0_zero)
        self._u0_cleared = False   # the flag is off for one warm-started solve whose u_init has tau1 != 0 (init)

    def _set_limited(self, tau_max, linearization, models, weights, pipeline, persistent, checkpoint):
        """The torque limit |tau2| <= tau_max of a limited solve (a number or (B,) per-lane limits, each positive, inf
        allowed), the sweep's linearisation: "euler" (the reference's A_d = I + dt A_c) or "rk4" (the exact
        Jacobians of the RK4 step), per-lane models (check_models' forms: lane b is planned on
        models[b]) and per-lane cost weights (check_weights' forms: lane b is planned under weights[b],
        DESIGN 4.12).  A solver with any of them runs the persistent loop on its own kernel (gym_newton_run_box /
        gym_newton_run_rk4 / gym_newton_run_models / gym_newton_run_weights) and nothing else: no pipeline, tail,
        compaction, low-occupancy switch, checkpointing or candidate scratch.  "rk4", models or weights without a
        limit pass +inf limits to that kernel and report none.  Weights combine with neither models nor "rk4" yet.
        Returns (pipeline, persistent) as _choose_schedule takes them."""
        if linearization not in ("euler", "rk4"):
            raise ValueError(f'linearization must be "euler" or "rk4", got {linearization!r}')
        self.linearization = linearization
        self.kind = _Kind()
        self._tau_in = self.tau_buf = None
        self.models = self._models_in = self.models_buf = None
        self.lane_weights = self._weights_in = self.weights_buf = None
        if weights is not None:
            if models is not None:
                raise NotImplementedError("per-lane weights (weights=) do not combine with per-lane models (models=) "
                                          "yet")
            if linearization == "rk4":
                raise NotImplementedError('per-lane weights (weights=) do not combine with linearization="rk4" yet')
            self.lane_weights = check_weights(weights, self.B, self.eng.weights)   # (B,10) host, the caller's order
            self._weights_in = self.eng.weight_table(self.lane_weights, self.B)    # (B,10) device, the caller's order
            pad = self.eng.weight_table(self.eng.weights, self.Bp - self.B)        # padding lanes: the engine's
            self.weights_buf = torch.cat([self._weights_in, pad]).contiguous()     # internal order (init)
        if models is not None:
            if linearization == "rk4":
                raise ValueError('per-lane models (models=) do not combine with linearization="rk4"')
            self.models = check_models(models, self.B, self.eng.params)        # (B,11) host, the caller's order
            self._models_in = self.eng.model_table(self.models, self.B)          # (B,8) device, the caller's order
            pad = self._models_in[-1:].expand(self.Bp - self.B, -1)              # padding lanes: a valid row
            self.models_buf = torch.cat([self._models_in, pad]).contiguous()    # internal order (init)
        if tau_max is None and linearization == "euler" and models is None and weights is None:
            return pipeline, persistent
        limit = "a torque-limited solve (tau_max)" if tau_max is not None else None
        if models is not None:
            self.kind = _Kind(limit or "per-lane models (models=)", "gym_newton_run_models", "gym_newton_sigma_models",
                              "gym_newton_init_models", "gym_newton_init_models", table="models")
        elif weights is not None:
            self.kind = _Kind(limit or "per-lane weights (weights=)", "gym_newton_run_weights",
                              "gym_newton_sigma_weights", "gym_newton_init_weights", "gym_newton_init_weights",
                              table="weights")
        elif linearization == "rk4":
            self.kind = _Kind(limit or 'linearization="rk4"', "gym_newton_run_rk4", "gym_newton_sigma_rk4")
        else:
            self.kind = _Kind(limit, "gym_newton_run_box", "gym_newton_sigma_box")
        if pipeline or checkpoint or persistent is False:
            raise ValueError(f"{self.kind.limited} runs the persistent schedule only: no pipeline=True, "
                             "persistent=False or checkpoint=True")
        if tau_max is None:
            self.tau_buf = torch.full((self.Bp,), float("inf"), dtype=F64, device=self.eng.device)
            return False, True
        t = self.eng.t(tau_max).reshape(-1)
        if t.numel() == 1:
            t = t.expand(self.B)
        if t.numel() != self.B:
            raise ValueError(f"tau_max must be a number or hold {self.B} lanes, got {t.numel()}")
        if not bool((t > 0).all().item()):      # zero, negative and NaN limits
            raise ValueError("tau_max must be positive (inf: no limit)")
        self._tau_in = t.contiguous().clone()                    # the caller's lane order
        self.tau_buf = torch.ones(self.Bp, dtype=F64, device=self.eng.device)   # internal order (init); padding: 1
        self.tau_buf[:self.B] = self._tau_in
        return False, True

    def _choose_schedule(self, pipeline, persistent, schedule_lanes, checkpoint, chunk, reorder, split_waves):
        """serial / pipelined / persistent (``schedule``), and how each runs."""
        dev = self.eng.device
        # the automatic schedule choice is made on ``schedule_lanes`` (default: this batch).  Sharded solves pass
        # the largest shard of the global batch, so that every rank picks the same schedule: the schedules
        # synchronise (all-reduce) at different points, and mixed choices would pair up the wrong collectives.
        sched_B = self.B_sched = int(schedule_lanes) if schedule_lanes is not None else self.B
        self.pipeline = (sched_B >= self.pipeline_min_lanes(dev)) if pipeline is None else bool(pipeline)
        # state checkpointing (GYM_FLAG_X_CKPT, opt-in): trials store x at every CKPT_INTERVAL-th knot only
        # and the sweep re-integrates the rest -- bit-identical results, 48 B/stage less traffic, but +0.75 RK4
        # per sweep stage: on MI355X the solver is as VALU- as HBM-limited and this measured 13% slower
        self.checkpoint = bool(checkpoint)
        # persistent schedule (gym_newton_run): not combined with checkpointing (its sweep re-integrates blocks)
        if persistent and self.checkpoint:
            raise ValueError("the persistent schedule does not support state checkpointing")
        if persistent is None:   # automatic only when the caller chose no schedule at all
            persistent = pipeline is None and sched_B <= self.persistent_max_lanes(dev)
        self.persistent = bool(persistent) and not self.checkpoint
        # iterations per persistent launch (0: all of max_iters in one).  128 keeps one launch to ~0.15 s at the
        # batch sizes that use the schedule (a non-converging batch at max_iters = 5000 would otherwise hold the
        # GPU in one multi-second kernel); the 3-4 launch boundaries of a headline solve cost nothing measurable.
        self.chunk = int(chunk)
        # solve() works on the lanes in the Morton order of their initial states (see morton_order)
        self.reorder = bool(reorder)
        # persistent schedule on two wavefronts per 64 lanes (k_nt_run2: a helper wavefront takes the Jacobians,
        # the cost and the stores off the lanes' dependency chains; same bits) unless split_waves=False
        self.split_waves = bool(split_waves)

    def _set_capture(self, capture_lanes, capture_every, capture_sigma):
        # selected-lane trajectory capture (the reference's history['x_trajs'], trajectory_generation.py:322-327,
        # 387-388): after every iteration the captured lanes' current iterates are gathered on the device; the
        # persistent schedule then runs one iteration per launch.  Not combined with checkpointing (the state
        # buffers hold checkpoints only).
        self.capture_lanes = None if capture_lanes is None else [int(i) for i in capture_lanes]
        if self.capture_lanes is not None:
            if self.checkpoint:
                raise ValueError("trajectory capture needs the full state store (checkpoint=False)")
            if any(not (0 <= i < self.B) for i in self.capture_lanes):
                raise ValueError(f"capture_lanes must lie in [0, {self.B})")
        self.capture_every = max(int(capture_every), 1)
        # sigma of the captured lanes at these iterations (the reference's report plots iterations 0, 1, 2 and the
        # last, trajectory_generation.py:341, 476-480; the last one is the solve's own sigma output)
        self.capture_sigma = tuple(sorted({int(i) for i in (capture_sigma or ())}))
        self._cap_pos, self._cap_log, self._sig_log = None, [], []

    def _alloc_streams(self, arena, placement_trials, auto_schedule):
        """The six stream buffers [x0, x1, u0, u1, K1, cs]: the PlacementPool's set of this shape, carved from one
        arena, or plain allocations.  Returns them and the number of placement trials."""
        dev = self.eng.device
        Bp, N, T = self.Bp, self.N, self.T
        shapes = [(N, 2, Bp, 2), (N, 2, Bp, 2), (T, 2, Bp, 1), (T, 2, Bp, 1), (T, 2, Bp, 2), (T, 2, Bp, 1)]
        self._stream_shapes = shapes
        # placement selection: default for the automatic schedule's pipelined solvers (the only schedule whose
        # throughput is the HBM streams'); a set chosen by an earlier solver of this shape in this process is reused
        # from the PlacementPool without a probe
        if placement_trials is None:
            placement_trials = (self.PLACEMENT_TRIALS
                                if auto_schedule and self.pipeline and not arena and not self.checkpoint else 1)
        placement_trials = int(placement_trials)
        self.placement = self._pl = None
        self._pool_key = (torch.device(dev).index, tuple(shapes))
        pooled = PlacementPool.take(self._pool_key) if placement_trials > 1 and not arena else None
        if pooled is not None:
            st, rec = pooled
            self.placement = dict(rec, reused=True)
        elif arena:
            # the six streams carved from one allocation, each 2 MiB aligned, in this order (arena: True = a torch
            # allocation, or a callable n -> fp64 device tensor of n elements that provides it)
            al = (2 << 20) // 8
            offs, n = [], 0
            for sh in shapes:
                offs.append(n)
                n += -(-int(np.prod(sh)) // al) * al
            self._arena = arena(n) if callable(arena) else torch.empty(n, dtype=F64, device=dev)
            st = [self._arena[o:o + int(np.prod(sh))].view(sh) for o, sh in zip(offs, shapes)]
        else:
            st = [torch.empty(sh, dtype=F64, device=dev) for sh in shapes]
        return st, placement_trials

    def _alloc_lane_buffers(self, max_ls, hist_len):
        dev = self.eng.device
        e = lambda *s, dt=F64: torch.empty(s, dtype=dt, device=dev)  # noqa: E731
        Bp, i32 = self.Bp, torch.int32
        self.cost, self.dJ, self.smax, self.gamma = e(Bp), e(Bp), e(Bp), e(Bp)
        self.status, self.n_iter, self.res_buf, self.n_roll = (e(Bp, dt=i32) for _ in range(4))
        self.retry_list = e(Bp, dt=i32)
        self.counters = torch.zeros(4, dtype=i32, device=dev)
        self.cand_ok = torch.zeros((max(int(max_ls), 1), Bp), dtype=torch.uint8, device=dev)
        self.partials = e(256 * 8)
        self.stats = torch.zeros(24, dtype=F64, device=dev)     # [0,8) totals, [8,16) / [16,24) halves
        self.hist_len = int(hist_len)
        self.hist_cost = torch.full((hist_len, Bp), float("nan"), dtype=F64, device=dev) if hist_len else None
        self.hist_smax = torch.full((hist_len, Bp), float("nan"), dtype=F64, device=dev) if hist_len else None

    def _fill_batch(self):
        """The gym_batch the launches take: sizes, flags and every buffer but the streams (_set_streams)."""
        b = _lib.GymBatch()
        b.B, b.Bp, b.N, b.hist_len = self.B, self.Bp, self.N, self.hist_len
        b.flags = ((_lib.FLAG_U0_ZERO if self.u0_zero else 0) | (_lib.FLAG_X_CKPT if self.checkpoint else 0) |
                   (0 if self.split_waves else _lib.FLAG_RUN_SINGLE) | (_lib.FLAG_REF_LANE if self.ref_lane else 0))
        for name in ("cost", "dJ", "smax", "gamma", "status", "n_iter", "res_buf", "n_roll",
                     "retry_list", "counters", "cand_ok", "partials", "stats"):
            setattr(b, name, getattr(self, name).data_ptr())
        if self.ref_lane:
            b.x_ref, b.u_ref = self.xr_buf.data_ptr(), self.ur_buf.data_ptr()
        else:
            b.x_ref, b.u_ref = self.x_ref.data_ptr(), self.u_ref.data_ptr()
        b.hist_cost = _lib.ptr(self.hist_cost)
        b.hist_smax = _lib.ptr(self.hist_smax)
        self.batch = b

    def _set_eligibility(self, auto_schedule, tail_lanes, tail_chunk, compact, world_size, cand_slots):
        """Which of the straggler tail, lane compaction and the candidate scratch this solver uses."""
        max_ls = int(self.armijo.max_ls)
        lockstep = not self.persistent and not self.checkpoint   # serial / pipelined with the full state store ...
        whole = lockstep and self.capture_lanes is None          # ... and whole-iteration launches (no capture)
        # straggler tail (serial / pipelined schedules; needs the full state store, whole-iteration launches: no
        # trajectory capture, at most 64 Armijo trials): switch once the global active count is <= tail_lanes.
        # Default: on with the automatic schedule choice, TAIL_LANES_PER_CU per CU of every rank (``world_size``:
        # the ranks the statistics are all-reduced over, so the switch comes at the same per-GPU occupancy at any
        # world size); a caller that picks a schedule gets it pure
        # the default also caps each rank's own active count at its per-GPU budget (tail_lanes_rank; the maximum over
        # ranks is all-reduced once the global count is under the threshold): with skewed shards one rank could
        # otherwise enter the tail with up to world x its budget of lanes, one workgroup each
        self.tail_lanes_rank = None
        if tail_lanes is None:
            n_cu = torch.cuda.get_device_properties(self.eng.device).multi_processor_count
            per_rank = self.TAIL_LANES_PER_CU * n_cu if auto_schedule else 0
            tail_lanes = per_rank * max(int(world_size), 1)
            self.tail_lanes_rank = per_rank or None
        # the tail kernel's limits: at most 64 trials, horizons up to its LDS staging, and that LDS within the
        # device's opt-in limit (checked here, so a device with less LDS turns the tail off instead of failing mid-solve)
        need, lds, lds_max = C.c_int64(), C.c_int64(), C.c_int64()
        fits = lambda name, *a: self._launch(name, *a, check=False, **_SIZES) == 0  # noqa: E731
        tail_ok = (whole and fits("gym_newton_tail_scratch", self.N, 1, max_ls, C.byref(need)) and
                   fits("gym_newton_tail_lds", self.N, C.byref(lds), C.byref(lds_max)) and
                   lds.value <= lds_max.value)
        self.tail_lanes = int(tail_lanes) if tail_ok else 0
        self.tail_chunk = max(int(tail_chunk), 1)
        self._tail_scratch = None
        # lane compaction (serial / pipelined schedules, solve(); see maybe_compact): default on with the automatic
        # schedule choice.  "force" compacts at every host synchronisation (tests)
        if compact is None:
            compact = auto_schedule
        self.compact_mode = ("force" if compact == "force" else bool(compact)) if whole else False
        # candidate scratch (gym_batch.cand_scratch, ABI 13): the post-trial Armijo candidates of the serial /
        # pipelined schedules and the low-occupancy regime record their trajectories, and the accepted one is copied
        # instead of re-run (a T-step chain per backtracking iteration).  Slots for min(lanes x (max_ls - 1),
        # cand_slots) candidates (~24 KiB each at T = 500); lanes past them are re-run.  The straggler tail borrows
        # the same buffer.  0 turns it off (the same bits either way).
        # Allocated on demand (ensure_cand_scratch): at the first host synchronisation whose iteration had lanes
        # rejecting trial 1, on entering the low-occupancy regime, or for the tail; a solve in which no lane
        # backtracks (the headline workload) never holds it.  Until then the accepted candidates are re-run (the
        # same bits).
        cand_slots = int(self.CAND_SLOTS if cand_slots is None else cand_slots)
        slots = min(self.Bp * max(max_ls - 1, 0), cand_slots) // 64 * 64
        self._cand_scratch = None
        self.cand_slots = slots if slots > 0 and lockstep and self.split_waves else 0

    def _reset_solve_counters(self):
        """What solve() counts and reports per call (SolveResult's tail / compaction / low-occupancy fields)."""
        self.tail_lane_its = 0
        self.tail_from, self.tail_iters = None, 0
        self.compactions = 0
        self._compact_prev = None
        self.serial_switch_at = None   # the iteration the low-occupancy switch happened at
        self._its_switch, self._its_tail_start = 0, None

    # --- launches and streams --------------------------------------------------------------
    def _launch(self, name, *args, pre=(), model=True, weights=None, armijo=False, batch=True, stream=True,
                check=True):
        """Call the library's ``name`` as (model[, models], weights[, lane weights][, armijo], *pre, batch, *args,
        stream) -- the keywords drop or add a part (``weights`` follows ``model`` unless given); ``models`` /
        ``lane weights``, the per-lane model / weight table, goes to the entry points of a kind that takes it
        (_Kind.table) -- and raise on a non-zero return code unless ``check`` is off.  Returns the code."""
        eng = self.eng
        a = []
        if model:
            a.append(C.byref(eng.model))
        table = self.kind.table if name in (self.kind.run, self.kind.sigma, self.kind.init,
                                            self.kind.init_warm) else None
        if table == "models":
            a.append(self.models_buf.data_ptr())
        if model if weights is None else weights:
            a.append(C.byref(eng._w))
        if table == "weights":
            a.append(self.weights_buf.data_ptr())
        if armijo:
            a.append(C.byref(self.armijo))
        a += pre
        if batch:
            a.append(C.byref(self.batch))
        a += args
        if stream:
            a.append(eng.stream)
        rc = getattr(eng.lib, name)(*a)
        if check:
            _lib.check(rc, name)
        return rc

    def _set_streams(self, st, zero: bool = True):
        """Use the stream set st = [x0, x1, u0, u1, K1, cs]; ``zero``: K1 and cs zeroed, as at construction (False: a
        set that holds the live state, copied by _move_streams)."""
        self.x = list(st[0:2])
        self.u = list(st[2:4])                         # control planes (tau1, tau2)
        self.K1 = st[4]                                # gain row 1, pairs
        self.cs = st[5]                                # planes: cg = (u1 - K1 x) + gamma0 sigma1, sigma1
        if zero:
            self.K1.zero_(); self.cs.zero_()
        b = self.batch
        b.x[0], b.x[1] = self.x[0].data_ptr(), self.x[1].data_ptr()
        b.u[0], b.u[1] = self.u[0].data_ptr(), self.u[1].data_ptr()
        b.K1, b.cs = self.K1.data_ptr(), self.cs.data_ptr()

    def _streams(self) -> list:
        return [*self.x, *self.u, self.K1, self.cs]

    def _move_streams(self, st):
        """Continue on stream set ``st``: the six streams copied into it (stream-ordered device copies, ~19 GB each way
        at 262,144 lanes), then the launches pointed at it.  Between two iterations the streams hold the whole state a
        later iteration reads (both state / control buffers, the gains and offsets of the half whose sweep already ran),
        so the solve continues bit for bit."""
        for src, dst in zip(self._streams(), st):
            dst.copy_(src)
        self._set_streams(st, zero=False)

    # --- placement selection (placement.py) ------------------------------------------------
    def _arm_placement(self, trials: int, candidates: int | None = None):
        """Set up the online selection among stream sets for the next solve (PlacementSelection.arm)."""
        B, N, T = self.B, self.N, self.T
        results_bytes = 8 * B * (4 * N + 2 * T + 8 * T + 2 * T)      # finalize's x, u, K, sigma
        # the probe kernel runs workgroups of two wavefronts: other batches race their sets unranked
        probe = (lambda cb: self._launch("gym_placement_probe", cb, model=False)) if self.Bp % 128 == 0 else None
        self._pl = placement.PlacementSelection.arm(
            self, self._pool_key, trials, candidates or self.PLACEMENT_CANDIDATES, self.PLACEMENT_BLOCK,
            self.PLACEMENT_MEM_SHARE, results_bytes, probe)
        if self._pl is not None:
            self.placement = self._pl.record

    def _end_placement(self):
        """The selection is over (its start() or tick() said so): its record stays, the object goes."""
        self.placement, self._pl = self._pl.record, None

    def ensure_cand_scratch(self) -> bool:
        """Allocate the candidate scratch (cand_slots slots, ~24 KiB each at T = 500) if this solver uses one and has
        not yet; stream-ordered, so the next launch may use it.  Returns whether it is in place."""
        if self._cand_scratch is None and self.cand_slots > 0:
            need = C.c_int64()
            self._launch("gym_newton_cand_scratch", self.N, self.cand_slots, C.byref(need), **_SIZES)
            self._cand_scratch = torch.empty(int(need.value), dtype=F64, device=self.eng.device)
            self.batch.cand_scratch, self.batch.cand_slots = self._cand_scratch.data_ptr(), self.cand_slots
        return self._cand_scratch is not None

    @property
    def schedule(self) -> str:
        return "persistent" if self.persistent else ("pipelined" if self.pipeline else "serial")

    def phase_kind(self) -> str | None:
        """The build of the phase kernel this batch's full phases launch (pipelined schedule; gym_newton_phase_kind):
        "two-wavefront" (more than 7/4 and at most 2 wavefronts per SIMD: compiled for two, prefetching two stages
        ahead) or "four-wavefront"; None for the other schedules.  Both builds give the same bits."""
        if self.schedule != "pipelined":
            return None
        lo = C.c_int32()
        self._launch("gym_newton_phase_kind", C.byref(lo), model=False, stream=False)
        return "two-wavefront" if lo.value else "four-wavefront"

    # --- optional per-kernel HIP-event timing (on the solver's stream) ---------------------
    def enable_timing(self):
        if self.timing is None:
            t = _lib.GymTiming()
            _lib.check(self.eng.lib.gym_timing_create(C.byref(t)), "gym_timing_create")
            self.timing = t
            self.batch.timing = C.pointer(t)
        return self

    def reset_timing(self):
        self.launches = {"phase": 0, "run": 0, "tail": 0, "iteration": 0}
        if self.timing is not None:
            torch.cuda.synchronize(self.eng.device)   # collect_timing reads completed event pairs only
            self.collect_timing()       # drains the pool (pairs of launches before the reset)
            for i in range(len(_lib.KERNEL_KINDS)):
                self.timing.ms[i] = 0.0
                self.timing.launches[i] = 0
            self.timing.pending = 0

    def collect_timing(self):
        """Accumulate recorded event pairs; the stream must have been synchronised."""
        if self.timing is not None:
            _lib.check(self.eng.lib.gym_timing_collect(C.byref(self.timing)), "gym_timing_collect")

    def kernel_times(self) -> dict:
        """{kind: (total_ms, launches)} for kinds _lib.KERNEL_KINDS."""
        if self.timing is None:
            return {}
        return {k: (float(self.timing.ms[i]), int(self.timing.launches[i])) for i, k in enumerate(_lib.KERNEL_KINDS)}

    def __del__(self):
        t = getattr(self, "timing", None)
        if t is not None:
            try:
                self.eng.lib.gym_timing_destroy(C.byref(t))
            except Exception:
                pass

    # --- the three stream-ordered phases (no host synchronisation inside) -----------------
    def _warm_inputs(self, u_init, status_init):
        """The warm start's inputs as the C-ABI takes them: u_init (B,T,2) fp64 and status_init (B) int32 or None,
        contiguous on the engine device, u_init 16-byte aligned.  Wrong shapes or dtypes: ValueError."""
        if isinstance(u_init, torch.Tensor) and u_init.dtype != F64:
            raise ValueError(f"u_init must be float64, got {u_init.dtype}")
        u = self.eng.t(u_init)
        if tuple(u.shape) != (self.B, self.T, 2):
            raise ValueError(f"u_init must be ({self.B},{self.T},2), got {tuple(u.shape)}")
        if u.data_ptr() % 16:
            u = u.clone()
        st = None
        if status_init is not None:
            st = status_init if isinstance(status_init, torch.Tensor) else torch.as_tensor(np.asarray(status_init))
            if st.dtype.is_floating_point or st.dtype.is_complex or st.dtype == torch.bool:
                raise ValueError(f"status_init must hold integer status codes, got {st.dtype}")
            if tuple(st.shape) != (self.B,):
                raise ValueError(f"status_init must be ({self.B},), got {tuple(st.shape)}")
            st = st.to(device=self.eng.device, dtype=torch.int32).contiguous()
        return u, st

    def _set_u0_zero(self, on: bool):
        self.u0_zero = bool(on)
        if on:
            self.batch.flags |= _lib.FLAG_U0_ZERO
        else:
            self.batch.flags &= ~_lib.FLAG_U0_ZERO

    def _restore_u0_zero(self):
        if self._u0_cleared:
            self._u0_cleared = False
            self._set_u0_zero(True)

    def init(self, x0, u_init=None, status_init=None, _ref_perm=None, _lane_map=None):
        """Start a solve from x0 (B,4): the reference's u = 0 (gym_newton_init), or, with ``u_init`` (B,T,2), from the
        caller's control iterate (gym_newton_init_warm: x rolled out from x0 under u_init with the Armijo trials'
        arithmetic, so a trial's own controls give back its states and cost bit for bit).  ``status_init`` (B)
        integer codes, with u_init only: lanes given CONVERGED or LS_FAILED keep that status and never iterate, any
        other value is an interrupted lane and iterates.  Iteration counts restart at 0 either way.
        A solver built with the tau1 planes skipped (u0_zero) whose u_init has a non-zero tau1 runs this solve on
        the general path (bit-identical by construction) and takes the flag back at the end of solve() or at the
        next init()."""
        self.lane_order = None
        self._restore_u0_zero()   # a warm start with tau1 != 0 that was not followed by solve()'s end
        x0 = self.eng.t(x0).reshape(-1, 4)
        if x0.shape[0] != self.B:
            raise ValueError(f"x0 must hold {self.B} lanes, got {x0.shape[0]}")
        if u_init is None and status_init is not None:
            raise ValueError("status_init needs u_init (a lane's status belongs to its control iterate)")
        if u_init is not None:
            u_init, status_init = self._warm_inputs(u_init, status_init)
        if self.ref_lane:   # the references in the lanes' internal order (solve()'s Morton order, or the caller's)
            self.xr_buf[:self.B] = self._xr_in if _ref_perm is None else self._xr_in[_ref_perm]
            self.ur_buf[:self.B] = self._ur_in if _ref_perm is None else self._ur_in[_ref_perm]
        if self._tau_in is not None:   # the per-lane limits likewise; a warm start must begin inside its lane's box
            self.tau_buf[:self.B] = self._tau_in if _ref_perm is None else self._tau_in[_ref_perm]
            if u_init is not None and bool((u_init[..., 1].abs() > self._tau_in[:, None]).any().item()):
                raise ValueError("u_init leaves the torque limit: |u_init[:, :, 1]| <= tau_max must hold per lane")
        if self.models_buf is not None:   # and the per-lane models
            self.models_buf[:self.B] = self._models_in if _ref_perm is None else self._models_in[_ref_perm]
        if self.weights_buf is not None:  # and the per-lane weights
            self.weights_buf[:self.B] = self._weights_in if _ref_perm is None else self._weights_in[_ref_perm]
        self._x0 = x0
        if self._pl is not None and self._pl.start(self):
            self._end_placement()
        if u_init is None:   # (a kind with one entry point for both starts: a warm start without controls)
            self._launch(self.kind.init, pre=(x0.data_ptr(),) + ((None, None) if self.kind.table else ()))
        else:
            if self.u0_zero and bool((u_init[..., 0] != 0).any().item()):
                self._set_u0_zero(False)
                self._u0_cleared = True
            # the caller's arrays go over unpermuted: internal lane i takes row lane_map[i] (the inverse direction of
            # finalize's use of the field)
            self.batch.lane_map = None if _lane_map is None else _lane_map.data_ptr()
            try:
                self._launch(self.kind.init_warm, pre=(x0.data_ptr(), u_init.data_ptr(), _lib.ptr(status_init)))
            finally:
                self.batch.lane_map = None
        self.k = 0
        self._capture_start(self.capture_lanes or [])
        self._serial_now = False   # the low-occupancy regime (maybe_compact / _enter_low_occupancy)
        self._run_now = False
        self._sigma_streamed = False
        self.batch.flags &= ~_lib.FLAG_SIGMA_STREAM
        if self.pipeline and not self.persistent and (self.max_iters is None or self.max_iters > 0):
            self._phase(0, True)                 # prologue: backward sweep of half H0, iteration 0

    def _run(self, k0: int, k1: int):
        self.launches["run"] += 1
        self._launch(self.kind.run, *self._limits(), int(k0), int(k1), armijo=True)

    _run_fn = property(lambda self: self.kind.run)   # the name a GPU test knows the run entry point by

    def _limits(self) -> tuple:
        """What a limited kind's run and sigma entry points take first: the per-lane limits."""
        return () if self.tau_buf is None else (self.tau_buf.data_ptr(),)

    def tail_run(self, k0: int, k1: int) -> torch.Tensor:
        """Iterations k0 .. k1-1 of every lane still active, on the straggler-tail kernel (gym_newton_tail: one
        workgroup per lane, every Armijo trial at once; the serial schedule's bits).  Every active lane must have
        done k0 iterations (the lock-step schedules' state after ``k0`` calls of iteration()).  Returns the 8
        statistics after iteration k1 - 1 (device)."""
        lanes = (self.status[:self.B] == _lib.ACTIVE).nonzero().flatten().to(torch.int32)
        n = int(lanes.numel())
        need = C.c_int64()
        self._launch("gym_newton_tail_scratch", self.N, n, int(self.armijo.max_ls), C.byref(need), **_SIZES)
        self.ensure_cand_scratch()
        if self._cand_scratch is not None and self._cand_scratch.numel() >= need.value:
            sc = self._cand_scratch          # the candidate scratch (the tail and the post-trial kernels never overlap)
        else:
            if self._tail_scratch is None or self._tail_scratch.numel() < need.value:
                self._tail_scratch = None
                self._tail_scratch = torch.empty(int(need.value), dtype=F64, device=self.eng.device)
            sc = self._tail_scratch
        self.launches["tail"] += 1
        self._launch("gym_newton_tail", lanes.data_ptr() if n else None, n, sc.data_ptr(), int(sc.numel()),
                     int(k0), int(k1), armijo=True)
        self.k = int(k1)
        return self.stats[:8]

    def _phase(self, p: int, do_backward: bool):
        self.launches["phase"] += 1
        self._launch("gym_newton_phase", p, int(do_backward), armijo=True)

    def iteration(self) -> torch.Tensor:
        """Enqueue outer iteration k for every active lane; returns the 8 total statistics (device)."""
        if self._pl is not None and self._pl.tick(self):
            self._end_placement()
        k = self.k
        if self.persistent or self._run_now:
            self._run(k, k + 1)
        elif self.pipeline and not self._serial_now:
            more = self.max_iters is None or k + 1 < self.max_iters
            self._phase(2 * k + 1, True)         # sweep H1 (iteration k) beside trial H0 (iteration k)
            self._phase(2 * k + 2, more)         # sweep H0 (iteration k+1) beside trial H1 (iteration k)
        else:
            self.launches["iteration"] += 1
            self._launch("gym_newton_iteration", k, armijo=True)
        self.k += 1
        self._capture()
        return self.stats[:8]

    # --- selected-lane trajectory capture -----------------------------------------------------
    def _capture_start(self, positions):
        """Begin capturing the lanes at internal positions ``positions`` (after init: the open-loop rollout)."""
        self._cap_log = []
        self._sig_log = []
        if self.capture_lanes is None:
            self._cap_pos = None
            return
        self._cap_pos = torch.as_tensor(positions, dtype=torch.int64, device=self.eng.device)
        self._capture(initial=True)

    def _capture(self, initial: bool = False):
        """Enqueue a gather of the captured lanes' current iterates, their iteration counts, statuses and costs.
        Device work only: no host synchronisation."""
        if self._cap_pos is None or (not initial and self.k % self.capture_every):
            return
        pos = self._cap_pos
        W = self.Bp // 64
        # wave-blocked pairs: (N, Bp/64, 2 rows, 64 lanes, 2) -> (n_cap, N, 2, 2) per buffer (the advanced
        # indices' dimension leads)
        # after k iterations a lane that accepted iteration k-1 holds its iterate in buffer k & 1 (iteration k-1
        # wrote its candidate there); the records of lanes that did not are discarded by captured_trajectories
        xb = self.x[self.k & 1]
        x = xb.view(self.N, W, 2, 64, 2)[:, pos // 64, :, pos % 64, :].reshape(-1, self.N, 4)
        self._cap_log.append((self.k, x.clone(), self.n_iter[pos].clone(), self.status[pos].clone(),
                              self.cost[pos].clone()))
        if not initial and (self.k - 1) in self.capture_sigma:
            # iteration k-1's sigma: gym_newton_sigma re-runs each lane's sweep at the iterate of its last
            # iteration (the same bits as that iteration's own sweep); it writes only the sigma1 plane, which every
            # schedule rewrites before reading it, so the solve is unchanged
            self._sig_log.append((self.k - 1, self.sigma()[pos].clone(), self.n_iter[pos].clone()))

    def captured_trajectories(self) -> dict:
        """{caller lane: [x_0, x after each accepted iteration ...]} as (N,4) numpy arrays -- the reference's
        history['x_trajs'] of each captured lane (entries only every ``capture_every`` iterations)."""
        if self.capture_lanes is None:
            return {}
        out = {lane: [] for lane in self.capture_lanes}
        for k, x, n_it, st, _ in self._cap_log:
            x, n_it, st = x.cpu().numpy(), n_it.cpu().numpy(), st.cpu().numpy()
            for j, lane in enumerate(self.capture_lanes):
                if k == 0:
                    out[lane].append(x[j])
                elif n_it[j] == k and st[j] != _lib.LS_FAILED:   # the lane ran iteration k-1 and accepted it
                    out[lane].append(x[j])
        return out

    def captured_sigmas(self) -> dict:
        """{caller lane: {iteration i: sigma (T,2)}} for the iterations of ``capture_sigma`` each captured lane ran
        (the reference's history['sigmas'][i])."""
        if self.capture_lanes is None:
            return {}
        out = {lane: {} for lane in self.capture_lanes}
        for it, sg, n_it in self._sig_log:
            sg, n_it = sg.cpu().numpy(), n_it.cpu().numpy()
            for j, lane in enumerate(self.capture_lanes):
                if n_it[j] == it + 1:                    # the lane ran iteration it
                    out[lane][it] = sg[j]
        return out

    def captured_initial_costs(self) -> dict:
        """{caller lane: J_0} of the captured lanes (the reference's history['cost'][0])."""
        if self.capture_lanes is None or not self._cap_log:
            return {}
        c0 = self._cap_log[0][4].cpu().numpy()
        return {lane: float(c0[j]) for j, lane in enumerate(self.capture_lanes)}

    def finalize(self):
        B, N, T, dev = self.B, self.N, self.T, self.eng.device
        x, u, K, s = (torch.empty((B, *sh), dtype=F64, device=dev) for sh in ((N, 4), (T, 2), (T, 2, 4), (T, 2)))
        if self.tau_buf is not None:   # the limited sigma: the box sweep re-run, never the unlimited one
            self._launch("gym_newton_finalize", self.k, x.data_ptr(), u.data_ptr(), K.data_ptr(), None)
            self._launch(self.kind.sigma, *self._limits(), s.data_ptr())
        else:
            self._launch("gym_newton_finalize", self.k, x.data_ptr(), u.data_ptr(), K.data_ptr(), s.data_ptr())
        return x, u, K, s

    def states(self, buf: int) -> torch.Tensor:
        """Every knot of state buffer ``buf`` (SoA (N,2,Bp,2)), rebuilt from its checkpoints if checkpointing.
        This is the solver's live stream buffer, not a copy: the next iteration overwrites it, and once this solver
        is gone the PlacementPool may hand the same memory to the next solver of the same shape.  Clone what must
        outlive either (unpack() already copies)."""
        self._launch("gym_newton_fill_states", int(buf), weights=False)
        return self.x[buf]

    def gamma_sweep(self, gammas) -> torch.Tensor:
        """Armijo line-search curve of every lane at the current iterate (the one iteration ``self.k`` starts
        from): J(gamma_g) of the trial rollout along iteration k's direction, (B, G); NaN for finished lanes.
        At the trial step sizes gamma_0 beta^i the values are the Armijo trials' costs bit for bit.  Runs
        iteration k's backward sweep, which that iteration recomputes identically, so the solve is unchanged."""
        if self.tau_buf is not None:
            raise ValueError(f"gamma_sweep() is not available on a solver with {self.kind.limited}")
        g = self.eng.t(gammas).reshape(-1)
        G = int(g.numel())
        if G < 1:
            raise ValueError("gamma_sweep needs at least one step size")
        J = torch.empty((G, self.Bp), dtype=F64, device=self.eng.device)
        self._launch("gym_newton_gamma_sweep", self.k, g.data_ptr(), G, J.data_ptr(), armijo=True)
        return J[:, :self.B].t()

    def gains(self) -> torch.Tensor:
        """K (B,T,2,4) of every lane's most recent backward sweep."""
        return self.eng.unpack_gains(self.K1, self.B)

    def controls(self, buf: int) -> torch.Tensor:
        """u (B,T,2) of control buffer ``buf``."""
        return self.eng.unpack(self.u[buf], self.B)

    def stream_sigma(self):
        """Call right after init(): run every iteration as the low-occupancy regime does (one launch of the
        four-wavefront persistent kernel per iteration, its sweep storing sigma1; _enter_low_occupancy), so that
        sigma() reads each iteration's sigma from the stored plane instead of re-running every lane's sweep.  For
        callers that want every iteration's sigma of a few lanes (the drop-in newton_Algorithm's history).  The same
        bits as any schedule."""
        if self.tau_buf is not None:
            raise ValueError(f"stream_sigma() is not available on a solver with {self.kind.limited}")
        if self.k != 0:
            raise RuntimeError("stream_sigma() must follow init() directly")
        self.pipeline = False
        self._enter_low_occupancy()
        self._sigma_streamed = True
        return self

    def sigma(self, rerun: bool = False) -> torch.Tensor:
        """sigma (B,T,2) of every lane's last completed iteration: its sweep re-run (sigma1 is not streamed), or,
        after stream_sigma() with the tau1 channel zero (u0_zero: sigma0 = -(2R0 (u0 - ur0)) / (2R0) = -0 on every
        stage), the sigma1 plane that iteration's sweep stored -- bit for bit the re-run (``rerun`` forces it)."""
        if self._sigma_streamed and self.u0_zero and not rerun:
            s = self.eng.unpack(self.cs, self.B)      # (B, T, 2): cg, sigma1
            s[..., 0] = -0.0
            return s
        s = torch.empty((self.B, self.T, 2), dtype=F64, device=self.eng.device)
        self._launch(self.kind.sigma, *self._limits(), s.data_ptr())
        return s

    # --- lane compaction ------------------------------------------------------------------
    COMPACT_MAX_SHARE = 0.25   # consider compacting once at most this share of the lanes is active ...
    COMPACT_MIN_KEEP = 0.5     # ... and the active count kept at least half its value since the last sync

    def maybe_compact(self, active: int) -> bool:
        """At a host synchronisation (iteration boundary), once at most a quarter of the lanes stay active (a stable
        population: the count kept at least half its value since the last sync), enter the low-occupancy regime:
        move the active lanes to the front (compact) and continue one iteration per launch of the persistent kernel
        with external retries (_enter_low_occupancy); later, compact again whenever the active lanes are spread over
        more than twice the wavefronts they need.  A wavefront runs its whole chains while any of its 64 lanes is
        active, so late in a hard solve (SURVEY 8(d)'s stress batch: ~22,000 of 262,144 lanes active for hundreds of
        iterations) every SIMD may still run its four wavefronts for a few lanes each; and with at most one
        wavefront per SIMD every launch is a latency-bound chain.  ``active``: this rank's count.  The trigger is
        rank-local (neither step changes a collective)."""
        if not self.compact_mode:
            return False
        prev, self._compact_prev = self._compact_prev, int(active)
        if active <= 0:
            return False
        if self.compact_mode != "force":
            if active > self.COMPACT_MAX_SHARE * self.B or prev is None or active < self.COMPACT_MIN_KEEP * prev:
                return False   # most lanes active, or a collapsing population that finishes on its own
            occupied = int((self.status.view(-1, 64) == _lib.ACTIVE).any(1).sum().item())
            if occupied < 2 * (-(-int(active) // 64) + 2) and (self._serial_now or not self.split_waves):
                if self._serial_now:
                    return False           # already dense, already switched
                self._enter_low_occupancy()
                return True
        self.compact()                     # (entering the persistent kernel's mode: always dense first)
        return True

    def _enter_low_occupancy(self):
        """Continue a pipelined or serial solve one iteration per launch of the four-wavefront persistent kernel
        (k_nt_run2: split Riccati sweep, lane-pair trial chains), its sweep storing sigma1 and the lanes that reject
        trial 1 finished by the serial schedule's parallel candidates and accepted re-run (GYM_FLAG_SIGMA_STREAM);
        with single-wavefront persistent kernels (split_waves=False), on the serial schedule (its sweep storing
        sigma1).  The same bits either way (the schedules' bitwise equality)."""
        self.ensure_cand_scratch()
        if not self._serial_now:
            self.serial_switch_at = self.k
            self._its_switch = int(self.n_iter[:self.B].sum().item())
        self._serial_now = True
        self._run_now = self.split_waves
        self.batch.flags |= _lib.FLAG_SIGMA_STREAM

    def compact(self, to_serial: bool = True):
        """Permute the lanes so that each lane range the kernels launch over (the serial schedule's batch, the
        pipelined schedule's halves H0 / H1) holds its active lanes first, in their order, and the finished ones
        behind them; waves of finished lanes then exit at once.  Every per-lane buffer moves with its lane (the
        state and trajectory buffers, gains, per-lane scalars, histories, per-lane references) and ``lane_order``
        follows, so solve() returns every lane in the caller's order: the results are the uncompacted solve's
        bit for bit (each lane's arithmetic is its own).  Only lanes that change position are moved.
        ``to_serial`` (the default): the solve then continues in the low-occupancy regime (_enter_low_occupancy;
        the next iteration re-runs H0's sweep, which the pipeline had already run: the same values), and the whole
        batch is one range.  Otherwise lanes keep their pipeline half."""
        B, Bp, dev = self.B, self.Bp, self.eng.device
        act = self.status[:B] == _lib.ACTIVE
        perm = torch.arange(Bp, device=dev)
        pipelined = self.pipeline and not self._serial_now and not to_serial
        if to_serial:
            self._enter_low_occupancy()
        if pipelined:
            Bh = C.c_int64()
            self._launch("gym_newton_pipeline_split", C.byref(Bh), model=False, stream=False)
            ranges = [(0, int(Bh.value)), (int(Bh.value), B)]
        else:
            ranges = [(0, B)]
        for lo, hi in ranges:
            if hi > lo:   # active lanes first, each group in its present order
                perm[lo:hi] = torch.argsort((~act[lo:hi]).to(torch.int8), stable=True) + lo
        moved = (perm != torch.arange(Bp, device=dev)).nonzero().flatten()
        if moved.numel() == 0:
            return
        src = perm[moved]
        gd, jd, gs, js = moved // 64, moved % 64, src // 64, src % 64
        for t in (self.x[0], self.x[1], self.K1):   # wave-blocked pairs (rows, Bp/64, 2, 64, 2)
            v = t.view(t.shape[0], Bp // 64, 2, 64, 2)
            v[:, gd, :, jd, :] = v[:, gs, :, js, :]
        for t in (self.u[0], self.u[1], self.cs):   # planes (rows, 2, Bp)
            v = t.view(t.shape[0], 2, Bp)
            v[:, :, moved] = v[:, :, src]
        for t in (self.cost, self.dJ, self.smax, self.gamma, self.status, self.n_iter, self.res_buf, self.n_roll):
            t[moved] = t[src]
        for t in (self.hist_cost, self.hist_smax):
            if t is not None:
                t[:, moved] = t[:, src]
        if self.ref_lane:
            self.xr_buf[moved] = self.xr_buf[src]
            self.ur_buf[moved] = self.ur_buf[src]
        if self.tau_buf is not None:
            self.tau_buf[moved] = self.tau_buf[src]
        if self.models_buf is not None:
            self.models_buf[moved] = self.models_buf[src]
        if self.weights_buf is not None:
            self.weights_buf[moved] = self.weights_buf[src]
        order = self.lane_order if self.lane_order is not None else torch.arange(B, device=dev)
        self.lane_order = order[perm[:B]]
        self.compactions += 1

    # --- full solve ----------------------------------------------------------------------
    def solve(self, x0, max_iters: int, reduce_stats=None, sync_every: int = 1, log_every: int = 0,
              keep_stats: bool = False, u_init=None, status_init=None) -> SolveResult:
        """Run until every lane (of every rank, if ``reduce_stats`` all-reduces) is done or max_iters.

        With ``reorder`` (default) the lanes are solved in the Morton order of their initial states
        (``morton_order``) and the results are returned in the caller's order; the device buffers then hold
        lane ``lane_order[i]`` of the input at position i.

        ``u_init`` (B,T,2) / ``status_init`` (B): warm start from the caller's control iterate (see init()); the
        arrays are handed over in the caller's order (the Morton permutation goes to the device as the init call's
        lane map, no permuted copy is made).  n_iter, n_rollouts, the histories and the captures of the result
        count from this call (resume() adds a checkpoint's)."""
        torch.cuda.synchronize(self.eng.device)
        t0 = time.perf_counter()
        self.max_iters = int(max_iters)
        perm = None
        if self.reorder and self.B > 1:
            x0 = self.eng.t(x0).reshape(-1, 4)
            perm = morton_order(x0)
            if u_init is None:
                x0 = x0[perm]
        try:
            return self._solve(x0, perm, t0, reduce_stats, sync_every, log_every, keep_stats, u_init, status_init)
        finally:
            self._restore_u0_zero()

    def _solve(self, x0, perm, t0, reduce_stats, sync_every, log_every, keep_stats, u_init, status_init):
        max_iters = self.max_iters
        if u_init is None:
            self.init(x0, status_init=status_init, _ref_perm=perm)
        else:
            self.init(x0, u_init=u_init, status_init=status_init, _ref_perm=perm, _lane_map=perm)
        self.lane_order = perm
        if perm is not None and self.capture_lanes is not None:
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(self.B, device=perm.device)
            self._capture_start(inv[torch.as_tensor(self.capture_lanes, device=perm.device)].tolist())
        self._reset_solve_counters()
        if self.persistent:
            log = run_loop(self, int(max_iters), reduce_stats, log_every, keep_stats)
        else:
            self.lane_order_live = True
            try:
                log = newton_loop(self, max_iters, reduce_stats=reduce_stats, sync_every=sync_every,
                                  log_every=log_every, keep_stats=keep_stats)
            finally:
                self.lane_order_live = False
        B = self.B
        perm = self.lane_order   # the Morton order, composed with any lane compaction of the loop
        if perm is None:
            back = slice(0, B)
        else:   # internal lane i is input lane perm[i]: finalize writes row perm[i]; gather the scalars back
            back = torch.empty_like(perm)
            back[perm] = torch.arange(B, device=perm.device)
            self.batch.lane_map = perm.data_ptr()
        try:
            x, u, K, s = self.finalize()
        finally:
            self.batch.lane_map = None
        lanes = lambda t: t[:B][back]  # noqa: E731
        n_iter = lanes(self.n_iter)
        res = dict(cost=lanes(self.cost), status=lanes(self.status), n_rollouts=lanes(self.n_roll),
                   gamma=lanes(self.gamma),
                   hist_cost=None if self.hist_cost is None else self.hist_cost[:, :B][:, back],
                   hist_smax=None if self.hist_smax is None else self.hist_smax[:, :B][:, back])
        torch.cuda.synchronize(self.eng.device)
        secs = time.perf_counter() - t0
        # persistent: the lanes' own iteration counts (no lock-step outer loop); otherwise the loop's count
        iters = int(n_iter.max().item()) if self.persistent else self.k
        if self.capture_lanes is not None:
            res.update(x_trajs=self.captured_trajectories(), cost0=self.captured_initial_costs(),
                       sigmas=self.captured_sigmas())
        lowocc = 0
        if self.serial_switch_at is not None:   # up to the tail switch, or the end of the solve
            end = self._its_tail_start if self._its_tail_start is not None else int(n_iter.sum().item())
            lowocc = end - self._its_switch
        return SolveResult(x=x, u=u, K=K, sigma=s, n_iter=n_iter, iterations=iters,
                           lane_iterations=int(n_iter.sum().item()), seconds=secs, stats_log=log,
                           schedule=self.schedule, tail_lane_iterations=int(self.tail_lane_its),
                           tail_from_iteration=self.tail_from, tail_iterations=int(self.tail_iters),
                           compactions=int(self.compactions), lowocc_lane_iterations=int(lowocc),
                           tau_max=None if self._tau_in is None else self._tau_in.clone(),
                           linearization=self.linearization,
                           models=None if self.models is None else self.models.copy(),
                           weights=None if self.lane_weights is None else self.lane_weights.copy(), **res)

    # --- closed-loop replanning -------------------------------------------------
    MPC_RUN = "gym_newton_mpc_run"

    def closed_loop(self, x0, u_init=None, *, iters: int = 1, iters_first: int | None = None, plant=None,
                    n_steps: int | None = None, steps_per_launch: int | None = None) -> ClosedLoopResult:
        """One closed loop per lane under receding-horizon replanning (shrinking horizon): init(x0, u_init), then at
        every control step t up to ``iters`` Newton iterations on the remaining horizon t .. T-1 from the measured
        state (``iters_first`` at step 0, default ``iters``), warm-started from the previous plan; stage t of the plan
        is applied to the lane's ``plant``, and where the plant leaves the plan its policy is rolled out again from
        the measured state (gym_newton_mpc_run, one persistent kernel for the whole loop or per ``steps_per_launch``
        steps: the same bits).  The stop test comes before the Armijo trials (a converged plan is kept), and either stop
        ends only its step.  ``plant``: engine.check_models' forms (a set number, a dict, (11,), (B,11), (B,1,11)) and
        refusals, default the design model on every lane; ``n_steps``: the first steps only (default all T).  A solver
        without tau_max runs with no limit.  Refused: checkpoint=True; linearization="rk4", models= and weights=
        (NotImplementedError: the kernel has no instantiation for them yet)."""
        if self.checkpoint:
            raise ValueError("closed_loop() needs the full state store: not on a solver with checkpoint=True")
        for on, what in ((self.linearization == "rk4", 'linearization="rk4"'), (self.models is not None, "models="),
                         (self.lane_weights is not None, "weights=")):
            if on:
                raise NotImplementedError(f"closed_loop() has no kernel for a solver with {what} yet: it replans on "
                                          "the engine's model, Euler sweep and weights")
        iters = int(iters)
        iters_first = iters if iters_first is None else int(iters_first)
        if iters < 0 or iters_first < 0:
            raise ValueError(f"iters and iters_first must be >= 0, got {iters} and {iters_first}")
        n_steps = self.T if n_steps is None else int(n_steps)
        if not 0 <= n_steps <= self.T:
            raise ValueError(f"n_steps must lie in 0..{self.T}, got {n_steps}")
        per = n_steps if steps_per_launch is None else int(steps_per_launch)
        if steps_per_launch is not None and per < 1:
            raise ValueError(f"steps_per_launch must be >= 1, got {steps_per_launch}")
        B, N, T, dev = self.B, self.N, self.T, self.eng.device
        par = None if plant is None else check_models(plant, B, self.eng.params)      # (B,11) host, the caller's order
        rows = self.eng.model_table({} if par is None else par, B)                    # (B,8) device, the caller's order
        x0 = self.eng.t(x0).reshape(-1, 4)
        perm = morton_order(x0) if self.reorder and B > 1 and x0.shape[0] == B else None
        # internal lane i is the caller's lane perm[i]: the limits, references and a warm start follow init()'s rules,
        # the plant rows are permuted here, and the kernel writes internal lane i's results to row perm[i]
        pad = rows[-1:].expand(self.Bp - B, -1)
        table = torch.cat([rows if perm is None else rows[perm], pad]).contiguous()
        if self.tau_buf is None:
            self._mpc_tau = torch.full((self.Bp,), float("inf"), dtype=F64, device=dev)
        tau = self.tau_buf if self.tau_buf is not None else self._mpc_tau
        keep, self.max_iters = self.max_iters, 0          # init() enqueues no solve prologue
        try:
            if u_init is None:
                self.init(x0 if perm is None else x0[perm], _ref_perm=perm)
            else:
                self.init(x0, u_init=u_init, _ref_perm=perm, _lane_map=perm)
        finally:
            self.max_iters = keep
        self.lane_order = perm
        i32 = torch.int32
        x = torch.zeros((B, N, 4), dtype=F64, device=dev)
        u = torch.zeros((B, T, 2), dtype=F64, device=dev)
        it, ro, stop = (torch.zeros((B, T), dtype=i32, device=dev) for _ in range(3))
        cost = torch.zeros((B, T), dtype=F64, device=dev)
        outs = tuple(t.data_ptr() for t in (x, u, it, ro, cost, stop))
        self.batch.lane_map = None if perm is None else perm.data_ptr()
        try:
            t = 0
            while t < n_steps:
                t1 = 1 if t == 0 else min(t + max(per, 1), n_steps)
                self._launch(self.MPC_RUN, tau.data_ptr(), table.data_ptr(), t, t1, iters_first if t == 0 else iters,
                             *outs, armijo=True)
                t = t1
        finally:
            self.batch.lane_map = None
        xr_last = self._xr_in[:, -1] if self.ref_lane else self.x_ref[-1]
        return ClosedLoopResult(x=x, u=u, iters=it, rollouts=ro, stop=stop, cost=cost,
                                err_final=(x[:, n_steps] - xr_last).abs().amax(dim=1) if n_steps == T else
                                torch.full((B,), float("nan"), dtype=F64, device=dev),
                                u_max=u.abs().amax(dim=(1, 2)) if T else torch.zeros(B, dtype=F64, device=dev),
                                tau_max=None if self._tau_in is None else self._tau_in.clone(), plant=par,
                                n_steps=n_steps)

    def resume(self, ckpt: Checkpoint, max_iters: int, **solve_kw) -> SolveResult:
        """Continue a checkpoint (load_checkpoint) for up to ``max_iters`` further iterations:
        solve(ckpt.x[:, 0], max_iters, u_init=ckpt.u, status_init=ckpt.status), merged with the checkpoint.

        A lane's bits do not depend on the schedule, its position or the launch it runs in, and the warm rollout is
        the Armijo trial's own, so a solve split at iteration k and resumed returns the uninterrupted solve's x, u,
        cost, status, n_iter, gamma and n_rollouts bit for bit (and K, sigma of every lane that iterated again).
        The merge: n_iter and n_rollouts are the checkpoint's plus this segment's; lanes the checkpoint had finished
        (CONVERGED / LS_FAILED: they do not iterate) keep its cost, gamma, K and sigma, as the device ran no sweep
        for them; so do K and sigma of lanes that ran no iteration here, and gamma of lanes that accepted no step
        here.  ``iterations``, ``lane_iterations``, the histories, the statistics log and the captures count this
        segment only."""
        dev = self.eng.device
        if ckpt.linearization != self.linearization:   # another sweep: not the same solve continued
            raise ValueError(f'the checkpoint was solved with linearization="{ckpt.linearization}", this solver has '
                             f'"{self.linearization}"')
        if (ckpt.models is None) != (self.models is None) or (
                self.models is not None and ckpt.models.tobytes() != self.models.tobytes()):
            raise ValueError("the checkpoint's per-lane models differ from this solver's (models=): another plant "
                             "per lane is not the same solve continued")
        mine, theirs = getattr(self, "lane_weights", None), getattr(ckpt, "weights", None)
        if (theirs is None) != (mine is None) or (mine is not None and theirs.tobytes() != mine.tobytes()):
            raise ValueError("the checkpoint's per-lane weights differ from this solver's (weights=): another cost "
                             "per lane is not the same solve continued")
        c = {k: getattr(ckpt, k).to(dev) for k in CHECKPOINT_KEYS}
        if c["x"].ndim != 3 or c["x"].shape[0] != self.B or c["x"].shape[1] != self.N:
            raise ValueError(f"the checkpoint holds x {tuple(c['x'].shape)}, this solver ({self.B},{self.N},4)")
        r = self.solve(c["x"][:, 0].contiguous(), max_iters, u_init=c["u"], status_init=c["status"], **solve_kw)
        done = (c["status"] == _lib.CONVERGED) | (c["status"] == _lib.LS_FAILED)
        ran = (r.n_iter > 0) & ~done
        stepped = ran & ((r.n_iter - (r.status == _lib.LS_FAILED).to(r.n_iter.dtype)) > 0)
        r.cost = torch.where(done, c["cost"].to(r.cost.dtype), r.cost)
        r.gamma = torch.where(stepped, r.gamma, c["gamma"].to(r.gamma.dtype))
        keep = (~ran).nonzero().flatten()       # rows only: K is the largest result (8 GB at 262,144 lanes)
        if keep.numel():
            r.K[keep] = c["K"][keep].to(r.K.dtype)
            r.sigma[keep] = c["sigma"][keep].to(r.sigma.dtype)
        r.n_iter = r.n_iter + c["n_iter"].to(r.n_iter.dtype)
        r.n_rollouts = r.n_rollouts + c["n_rollouts"].to(r.n_rollouts.dtype)
        return r


def newton_solve_batch(x0, x_ref, u_ref, max_iters, tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0,
                       max_ls=MAX_LINE_SEARCH_ITERS, engine: AcrobotEngine | None = None, hist_len=0,
                       reduce_stats=None, pipeline: bool | None = None,
                       persistent: bool | None = None, capture_lanes=None, u_init=None, tau_max=None,
                       linearization: str = "euler", models=None, weights=None) -> SolveResult:
    """Batched newton_Algorithm: x0 (B,4) -> SolveResult (device tensors).  ``u_init`` (B,T,2): start from these
    controls instead of u = 0 (BatchedNewtonSolver.init).  ``tau_max`` (a number or (B,)): the torque-limited solve
    (BatchedNewtonSolver's tau_max).  ``linearization``: "euler" (the reference's) or "rk4" (the exact Jacobians of
    the RK4 step, BatchedNewtonSolver's linearization).  ``models``: one parameter set per lane, lane b planned on
    models[b] (BatchedNewtonSolver's models).  ``weights``: one set of cost weights per lane, lane b planned under
    weights[b] (BatchedNewtonSolver's weights)."""
    eng = engine or AcrobotEngine()
    x0 = eng.t(x0).reshape(-1, 4)
    solver = BatchedNewtonSolver(eng, x_ref, u_ref, x0.shape[0], tol=tol, beta=beta, c=c, gamma_0=gamma_0,
                                 max_ls=max_ls, hist_len=hist_len, pipeline=pipeline, persistent=persistent,
                                 capture_lanes=capture_lanes, tau_max=tau_max, linearization=linearization,
                                 models=models, weights=weights)
    return solver.solve(x0, max_iters, reduce_stats=reduce_stats, u_init=u_init)


def newton_mpc_batch(x0, x_ref, u_ref, tol=1e-6, beta=0.7, c=0.5, gamma_0=1.0, max_ls=MAX_LINE_SEARCH_ITERS,
                     engine: AcrobotEngine | None = None, u_init=None, tau_max=None, iters: int = 1,
                     iters_first: int | None = None, plant=None, n_steps: int | None = None,
                     steps_per_launch: int | None = None) -> ClosedLoopResult:
    """Batched receding-horizon replanning: x0 (B,4) -> ClosedLoopResult (device tensors), one closed loop per lane
    (BatchedNewtonSolver.closed_loop).  The settings are newton_solve_batch's; ``iters`` / ``iters_first`` Newton
    iterations per control step / at step 0, ``plant`` the plant each loop runs on (default: the design model),
    ``n_steps`` / ``steps_per_launch`` as closed_loop takes them."""
    eng = engine or AcrobotEngine()
    x0 = eng.t(x0).reshape(-1, 4)
    solver = BatchedNewtonSolver(eng, x_ref, u_ref, x0.shape[0], tol=tol, beta=beta, c=c, gamma_0=gamma_0,
                                 max_ls=max_ls, tau_max=tau_max)
    return solver.closed_loop(x0, u_init, iters=iters, iters_first=iters_first, plant=plant, n_steps=n_steps,
                              steps_per_launch=steps_per_launch)
