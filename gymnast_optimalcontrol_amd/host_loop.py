"""The host loops of a Newton solve: launch, and every so often all-reduce and read the 8 statistics (STAT_FIELDS;
[0] = active lanes) and stop once no lane of any rank is active.  Also morton_order, the lane order solve() works in.

The loops take any stepper with these attributes (BatchedNewtonSolver; the test oracle's stepper; the tests' mocks):
  * every loop, optional (getattr): ``collect_timing()``, called after each read; ``timeline``, a list that takes
    (iterations, active lanes, host time) per read unless None.
  * run_loop (persistent schedule): ``chunk``, ``_cap_pos``, ``_run(k0, k1)``, ``_capture()``, ``stats``; sets ``k``.
  * newton_loop (lock-step schedules): ``iteration()`` -> statistics (tensor or array).  Optional: ``tail_lanes``
    (> 0: hand over to tail_loop at that global active count) with ``tail_lanes_rank``, ``maybe_compact(active)``
    (called only while ``lane_order_live``), ``ensure_cand_scratch()``.
  * tail_loop (straggler tail): ``tail_run(k0, k1)`` -> statistics, ``tail_chunk``, ``n_iter``, ``B``, ``k``; sets
    ``_its_tail_start``, ``tail_lane_its``, ``k``, ``tail_from``, ``tail_iters``.
``reduce_stats`` (None: one rank) all-reduces (SUM) a statistics tensor; its optional ``max_of(n)`` all-reduces a
number (MAX) for the tail's per-rank budget.
"""
from __future__ import annotations

import time

import numpy as np
import torch

STAT_FIELDS = ("n_active", "sum_cost", "sum_smax2", "lanes_ran", "n_retry", "n_converged", "n_failed", "n_rollouts")


def morton_order(x0: torch.Tensor, bits: int = 10) -> torch.Tensor:
    """Lane permutation along a Z-order (Morton) curve over the initial states x0 (B,4).

    A wavefront runs until the last of its 64 lanes has converged, so lanes that need different iteration
    counts waste the slots of the early finishers (on the headline workload, lanes converge after 381-404
    iterations: 97.8% of the slots do useful work in input order).  Neighbouring initial states converge in
    similar counts; grouping them along a space-filling curve raises that to 99.7% (C oracle, 8,192 lanes).
    Each coordinate is quantised to ``bits`` bits over the batch's range (non-finite values as 0) and the
    bits are interleaved; ties keep the input order."""
    x = torch.nan_to_num(x0, nan=0.0, posinf=0.0, neginf=0.0)
    lo, hi = x.min(0).values, x.max(0).values
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    q = ((x - lo) / span * (2 ** bits - 1)).clamp(0, 2 ** bits - 1).to(torch.int64)
    key = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    d = x.shape[1]
    for b in range(bits):
        for j in range(d):
            key |= ((q[:, j] >> b) & 1) << (b * d + j)
    return torch.argsort(key, stable=True)


def _read_stats(stepper, st, reduce_stats, k: int, keep_stats: bool, log: list):
    """One host synchronisation after ``k`` iterations: the statistics ``st`` all-reduced across ranks and read,
    the stepper's timing collected, the read logged (``keep_stats``) and put on the stepper's timeline.  Returns the
    host statistics and this rank's own (``st`` as given: [0] is the local active count)."""
    local = st
    if reduce_stats is not None:
        st = reduce_stats(st)
    host = st.cpu().numpy() if isinstance(st, torch.Tensor) else np.asarray(st)
    collect = getattr(stepper, "collect_timing", None)
    if collect is not None:
        collect()
    if keep_stats:
        log.append(host.copy())
    if getattr(stepper, "timeline", None) is not None:   # diagnostics: (iterations, active, host time)
        stepper.timeline.append((k, int(host[0]), time.perf_counter()))
    return host, local


def run_loop(solver, max_iters: int, reduce_stats, log_every: int, keep_stats: bool):
    """Persistent schedule: launches of ``chunk`` iterations (0: all of max_iters); after each one the
    statistics are all-reduced across ranks (``reduce_stats``) and read, and the loop stops when no lane of any
    rank is active."""
    log = []
    chunk = solver.chunk if solver.chunk > 0 else max(int(max_iters), 1)
    # trajectory capture: one iteration per launch, but the statistics are still read (and all-reduced) at the
    # same iterations as without capture, so ranks that capture and ranks that do not stay paired
    step = 1 if solver._cap_pos is not None else chunk
    k = 0
    while k < max_iters:
        k1 = min(int(max_iters), k + step)
        solver._run(k, k1)
        solver.k = k = k1
        solver._capture()
        if k % chunk and k < max_iters:
            continue
        host, _ = _read_stats(solver, solver.stats[:8], reduce_stats, k, keep_stats, log)
        if log_every:
            print(f"iter {k}: active={int(host[0])} sumJ={host[1]:.6e} ran={int(host[3])}", flush=True)
        if host[0] == 0:
            break
    return log


def newton_loop(stepper, max_iters: int, reduce_stats=None, sync_every: int = 1, log_every: int = 0,
                keep_stats: bool = False) -> list:
    """Outer Newton loop shared by every stepper (HIP solver; the test oracle stepper).

    ``stepper.iteration()`` enqueues one iteration for all of its lanes and returns the 8-entry
    statistics tensor (STAT_FIELDS).  Every ``sync_every`` iterations the statistics are
    all-reduced across ranks (``reduce_stats``, SUM) and read on the host; the loop stops when no
    lane of any rank is active.  Returns the list of host statistics if ``keep_stats``."""
    log = []
    tail = int(getattr(stepper, "tail_lanes", 0) or 0)
    compact = getattr(stepper, "maybe_compact", None) if getattr(stepper, "lane_order_live", False) else None
    for k in range(int(max_iters)):
        st = stepper.iteration()
        if (k + 1) % sync_every == 0 or k + 1 == max_iters:
            host, local = _read_stats(stepper, st, reduce_stats, k + 1, keep_stats, log)
            if log_every and (k % log_every == 0):
                print(f"iter {k}: active={int(host[0])} sumJ={host[1]:.6e} ran={int(host[3])} "
                      f"retry={int(host[4])}", flush=True)
            if host[0] == 0:
                break
            if host[4] > 0:   # lanes rejected trial 1: from now on the post-trial search records its candidates
                ensure = getattr(stepper, "ensure_cand_scratch", None)
                if ensure is not None:
                    ensure()
            # the straggler tail: decided on the (all-reduced) global active count, so every rank switches at the
            # same iteration and pairs up the same collectives afterwards; with a per-rank budget (tail_lanes_rank)
            # also on the largest rank's own count, all-reduced (MAX) by every rank at the same iteration (they all
            # see the same global count)
            if tail and host[0] <= tail and k + 1 < max_iters and _tail_rank_ok(stepper, host, local, reduce_stats):
                log += tail_loop(stepper, k + 1, int(max_iters), reduce_stats, log_every, keep_stats)
                break
            if compact is not None and k + 1 < max_iters:   # rank-local: no collective depends on it
                compact(int(local[0].item()) if reduce_stats is not None else int(host[0]))
    return log


def _tail_rank_ok(stepper, host, local, reduce_stats) -> bool:
    """The per-rank part of the straggler-tail switch: the largest rank's active count within ``tail_lanes_rank``
    (None: no per-rank budget).  Sharded, the maximum is one MAX all-reduce (``reduce_stats.max_of``) that every rank
    issues at the same iteration; with a reducer that has no ``max_of`` the budget is not applied (a warning)."""
    cap = getattr(stepper, "tail_lanes_rank", None)
    if cap is None:
        return True
    if reduce_stats is None:
        return host[0] <= cap
    max_of = getattr(reduce_stats, "max_of", None)
    if max_of is None:
        # a caller-supplied reducer without a MAX: the per-rank budget cannot be checked without a collective the
        # other ranks would not pair, so the global threshold alone decides (comparing the global count with the
        # per-rank cap would delay the tail until the whole job fits one rank's budget)
        if not getattr(stepper, "_warned_no_max_of", False):
            import warnings
            warnings.warn("reduce_stats has no max_of: the straggler tail's per-rank budget is not applied")
            stepper._warned_no_max_of = True
        return True
    n = float(local[0].item()) if isinstance(local, torch.Tensor) else float(np.asarray(local)[0])
    return max_of(n) <= cap


def tail_loop(solver, k: int, max_iters: int, reduce_stats, log_every: int, keep_stats: bool) -> list:
    """The rest of a serial / pipelined solve on the straggler-tail kernel, ``tail_chunk`` iterations per launch
    (a lane stops inside a launch when it finishes; the launch ends with its last lane); the statistics are
    all-reduced and read after each launch, and the loop stops when no lane of any rank is active."""
    log = []
    k_switch = k
    its0 = int(solver.n_iter[:solver.B].sum().item())
    solver._its_tail_start = its0
    while k < max_iters:
        k1 = min(max_iters, k + solver.tail_chunk)
        st = solver.tail_run(k, k1)
        k = k1
        host, _ = _read_stats(solver, st, reduce_stats, k, keep_stats, log)
        if log_every:
            print(f"tail iter {k}: active={int(host[0])} sumJ={host[1]:.6e}", flush=True)
        if host[0] == 0:
            break
    solver.tail_lane_its = int(solver.n_iter[:solver.B].sum().item()) - its0
    # a launch runs up to tail_chunk iterations but ends with its last lane: report the last iteration a lane ran,
    # not the end of the chunk.  Sharded (reduce_stats): the chunk end, identical on every rank, as the lock-step loop
    # reports its global count (a rank-local maximum would differ between ranks)
    if reduce_stats is None and solver.B:
        solver.k = max(k_switch, min(solver.k, int(solver.n_iter[:solver.B].max().item())))
    solver.tail_from, solver.tail_iters = k_switch, solver.k - k_switch
    return log
