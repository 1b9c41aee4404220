"""Placement selection: where a large pipelined solver's six stream buffers live.

The phase kernel's speed depends on where its stream buffers land (1.89-2.08 ms per launch for sets alive at once in
one process, each stable for its lifetime; profiles/r05/placement/, profiles/r06/README.md).  On a slow set the same
fabric requests come back later (+13..24% read latency, ~2x the L2's DRAM-credit and write stalls; no more translation
misses, no channel imbalance), and the slowness follows how the streams the same waves touch in lock step lie relative
to each other in physical memory; no allocation rule reachable from user space fixes it (contiguous VRAM at 200
layouts, record layouts), so the solver measures.  A large pipelined solver allocates up to PLACEMENT_CANDIDATES stream
sets (as free memory allows), ranks them at construction with the placement probe (gym_placement_probe: the phase
kernel's traffic without arithmetic, ~2 ms a launch; it ranks sets as the kernel does, Pearson 0.87-0.93), keeps the
PLACEMENT_TRIALS best, and races those in its first solve: blocks of PLACEMENT_BLOCK iterations of that solve on each
(the live state copied from set to set between blocks: the same bits on any set), the fastest kept and pooled for the
process's later solvers of the same shape.  In the zero-arithmetic probe about a third of the sets are fast (1.84-1.86
ms), a third middling (1.95-2.03), the rest slow: eight candidates leave one selection in ~25 without a fast set, four
one in 5 (profiles/r06/layout/).  The constants are BatchedNewtonSolver's.

PlacementSelection is host logic only.  It reaches its solver (handed to every step, never kept) through the stream
accessors ``_streams()``, ``_set_streams(st, zero=)`` and ``_move_streams(st)``, the iteration count ``k`` and the two
regime flags ``_serial_now`` / ``_run_now``, and it times with the events of ``new_event`` (a test scripts them).
"""
from __future__ import annotations

import time
import weakref
from collections import OrderedDict

import numpy as np
import torch

from .engine import F64


def new_event():
    """A timing event on the current stream: record(), synchronize(), elapsed_time(later) in ms."""
    return torch.cuda.Event(enable_timing=True)


def _mark():
    """A new event, recorded now."""
    ev = new_event()
    ev.record()
    return ev


class PlacementPool:
    """Process-wide cache of the stream-buffer sets that placement selection chose (PlacementSelection), keyed by
    (device index, stream shapes).  A solver that chose a set leases it; when the solver is garbage-collected
    the set comes back here, and the next solver of the same shape takes it without a probe or an allocation (the
    batched newton_Algorithm builds a solver per call, bench.py one per leg).  At most one free set per key; free sets
    beyond MAX_SHARE of the device's memory are dropped, oldest first.  ``clear()`` returns every free set to the
    device."""
    MAX_SHARE = 0.35
    _free: "OrderedDict" = OrderedDict()

    @staticmethod
    def _bytes(key) -> int:
        return 8 * sum(int(np.prod(sh)) for sh in key[1])

    @classmethod
    def take(cls, key):
        """(streams, record) of a free set for ``key``, now leased to the caller, or None."""
        return cls._free.pop(key, None)

    @classmethod
    def put(cls, key, streams, record):
        if key in cls._free:
            return
        cls._free[key] = (streams, record)
        try:
            cap = cls.MAX_SHARE * torch.cuda.get_device_properties(key[0]).total_memory
        except Exception:
            return
        while len(cls._free) > 1 and sum(cls._bytes(k) for k in cls._free) > cap:
            cls._free.popitem(last=False)

    @classmethod
    def clear(cls):
        cls._free.clear()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    @classmethod
    def held_bytes(cls) -> int:
        return sum(cls._bytes(k) for k in cls._free)


def lease(solver, key, record):
    """The solver's streams are the pool's set for ``key``: back to the PlacementPool when the solver goes."""
    rec = {k: v for k, v in record.items() if k != "reused"}
    f = weakref.finalize(solver, PlacementPool.put, key, solver._streams(), rec)
    f.atexit = False


class PlacementSelection:
    """The online selection among ``sets`` (stream sets of one shape; the solver is on sets[0]) over blocks of
    ``block`` iterations.  ``record`` is what the solver shows as its ``placement``; start() and tick() return True
    once the selection is over (the solver then drops this object and keeps the record)."""

    def __init__(self, sets, key, block: int, alloc_s: float = 0.0, screen=None):
        self.sets, self.key, self.block = sets, key, int(block)
        self.cur, self.attempts, self.alloc_s, self.screen = 0, 0, alloc_s, screen
        self.order, self.blocks, self.open, self.copies = None, [], None, 0
        self.record = {"trials": len(sets), "state": "pending", "alloc_s": alloc_s, "screen": screen}

    @classmethod
    def arm(cls, solver, key, trials: int, candidates: int, block: int, mem_share: float, results_bytes: int,
            probe=None):
        """Allocate up to ``candidates`` - 1 further stream sets (while the free memory allows, beside the lane-major
        results a solve allocates: ``results_bytes``), rank all of them with the placement probe (``probe(cb)``
        launches it on the solver's current streams; None: no ranking) and keep the ``trials`` best for the online
        selection of the next solve (tick); the others go back to the device.  Returns the selection, or None where
        there is nothing to select among."""
        first = solver._streams()
        dev, shapes = first[0].device, key[1]
        candidates = max(int(candidates), int(trials))
        set_bytes = 8 * sum(int(np.prod(sh)) for sh in shapes)
        free, total = torch.cuda.mem_get_info(dev)
        # beside the results a solve allocates, and at most ``mem_share`` of the device for the extra sets (so
        # that processes sharing a GPU leave each other room); an allocation that fails (another process was faster)
        # just ends the candidate list
        room = min(free - results_bytes - (4 << 30), mem_share * total)
        k = min(candidates, 1 + max(0, int(room // max(set_bytes, 1))))
        if k < 2:
            return None
        t0 = time.perf_counter()
        sets = [first]
        try:
            for _ in range(k - 1):
                sets.append([torch.empty(sh, dtype=F64, device=dev) for sh in shapes])
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
        k = len(sets)
        if k < 2:
            return None
        screen = None
        if k > trials and probe is not None:
            # rank the candidates by the placement probe (two rounds, each set's faster launch), keep the best
            ms = [float("inf")] * k
            for r in range(2):
                for i, st in enumerate(sets):
                    solver._set_streams(st, zero=False)
                    e0 = _mark()
                    probe(r & 1)
                    e1 = _mark()
                    e1.synchronize()
                    ms[i] = min(ms[i], e0.elapsed_time(e1))
            keep = sorted(range(k), key=lambda i: ms[i])[:trials]
            screen = {"candidates": k, "probe_ms": ms, "kept": keep}
            sets = [sets[i] for i in keep]
            torch.cuda.empty_cache()                # the screened-out sets go back to the device
        solver._set_streams(sets[0])                # K1, cs zeroed (the probe left garbage), as at construction
        if len(sets) < 2:
            return None
        return cls(sets, key, block, time.perf_counter() - t0, screen)

    def start(self, solver) -> bool:
        """(init) A new solve: the selection schedule restarts from the set in use, in the order c, the others, then
        the reverse (each set runs two blocks placed symmetrically, so a drift of the iterations' cost over the probe
        cancels out of the comparison)."""
        self.attempts += 1
        if self.attempts > 2:                      # two solves ended before the probe did: keep the set in use
            return self.finish(solver, abandon=True)
        seq = [self.cur] + [i for i in range(len(self.sets)) if i != self.cur]
        self.order, self.blocks, self.open, self.copies = seq + seq[::-1], [], None, 0
        return False

    def tick(self, solver) -> bool:
        """(iteration, before its launches) At the block boundaries of the schedule: close the running block with an
        event, move the state to the next block's set, open the next block.  Only on the pipelined schedule while it
        runs its phases (the low-occupancy regime and the tail end the probe for this solve)."""
        if solver._serial_now or solver._run_now or self.order is None:
            return False
        k, n = solver.k, self.block
        if k % n:
            return False
        if self.open is not None:
            self.blocks.append((*self.open, _mark()))
            self.open = None
        i = k // n
        if i >= len(self.order):
            return self.finish(solver)
        target = self.order[i]
        if target != self.cur:
            solver._move_streams(self.sets[target])
            self.cur = target
            self.copies += 1
        self.open = (target, _mark())
        return False

    def finish(self, solver, abandon: bool = False) -> bool:
        """Keep the fastest set (by the mean of its blocks' ms per iteration), release the others, and lease the kept
        one to the solver (back to the PlacementPool when the solver goes).  Returns True: the selection is over."""
        per = {}
        for s, e0, e1 in self.blocks:
            e1.synchronize()
            per.setdefault(s, []).append(e0.elapsed_time(e1) / self.block)
        best = self.cur
        if not abandon and per:
            best = min(per, key=lambda s: sum(per[s]) / len(per[s]))
            if best != self.cur:
                solver._move_streams(self.sets[best])
                self.copies += 1
        self.record = {"trials": len(self.sets), "state": "abandoned" if abandon else "chosen", "chosen": best,
                       "ms_per_iteration": {int(s): v for s, v in sorted(per.items())},
                       "probe_iterations": self.block * len(self.blocks), "copies": self.copies,
                       "alloc_s": self.alloc_s, "at_iteration": int(solver.k), "screen": self.screen}
        self.sets = self.blocks = self.open = None
        torch.cuda.empty_cache()                    # the unused sets go back to the device, not the process's cache
        lease(solver, self.key, self.record)
        return True
