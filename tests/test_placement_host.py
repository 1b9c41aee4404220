"""Placement selection as host logic (gymnast_optimalcontrol_amd.placement.PlacementSelection): the block schedule,
the event pairs, the minimum over means, abandonment and the lease -- driven with a stand-in solver and scripted events,
no device and no library.  (On the device: tests/test_gpu_parity.py::test_placement_selection_is_invisible; the pool
itself: tests/test_abi_host.py::test_placement_pool_leases_one_set_per_shape.)"""
import gc
import types

import pytest
import torch

from gymnast_optimalcontrol_amd import placement
from gymnast_optimalcontrol_amd.placement import PlacementPool, PlacementSelection

BLOCK = 12
KEY = (0, ((4,),) * 6)


class StandInSolver:
    """What the selection reaches a solver through: the stream accessors, ``k`` and the two regime flags."""

    def __init__(self, st):
        self.st, self.k, self._serial_now, self._run_now, self.moves = st, 0, False, False, []

    def _streams(self):
        return self.st

    def _set_streams(self, st, zero=True):
        self.st = st

    def _move_streams(self, st):
        self.moves.append((self.st, st))
        self.st = st


@pytest.fixture
def clock(monkeypatch):
    """Scripted events: record() reads clock.ms, which the test advances."""
    c = types.SimpleNamespace(ms=0.0, events=0)

    class Event:
        def __init__(self):
            c.events += 1
            self.t = None

        def record(self):
            self.t = c.ms

        def synchronize(self):
            assert self.t is not None

        def elapsed_time(self, later):
            return later.t - self.t

    monkeypatch.setattr(placement, "new_event", Event)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda i: types.SimpleNamespace(total_memory=1 << 30))
    PlacementPool._free.clear()
    yield c
    PlacementPool._free.clear()


def _three_sets():
    return [[f"{name}{i}" for name in ("x", "y", "u", "v", "K", "c")] for i in range(3)]


def _race(sel, solver, clock, ms_per_iteration, k_end):
    """Iterations 0 .. k_end - 1 with a tick before each (and one before iteration k_end, which nothing runs), block b
    costing ms_per_iteration[b] per iteration.  Returns [(k, set)] of the blocks opened and whether tick ended it."""
    opened, over = [], False
    for k in range(k_end + 1):
        solver.k = k
        before = sel.open
        over = sel.tick(solver)
        if over:
            break
        if sel.open is not before:
            opened.append((k, sel.open[0]))
        if k < k_end:
            clock.ms += ms_per_iteration[k // BLOCK]
    return opened, over


def test_selection_races_the_sets_and_keeps_the_fastest(clock):
    sets = _three_sets()
    solver = StandInSolver(sets[0])
    sel = PlacementSelection(sets, KEY, BLOCK)
    assert sel.record["state"] == "pending" and sel.record["trials"] == 3
    assert sel.start(solver) is False
    # sets 0, 1, 2 run 2.0 / 2.2, 1.9 / 1.9 and 2.1 / 1.8 ms per iteration in their two blocks
    opened, over = _race(sel, solver, clock, [2.0, 1.9, 2.1, 1.8, 1.9, 2.2], 6 * BLOCK)
    assert opened == [(b * BLOCK, s) for b, s in enumerate([0, 1, 2, 2, 1, 0])]
    assert over is True
    rec = sel.record
    assert rec["state"] == "chosen" and rec["chosen"] == 1 and rec["trials"] == 3
    assert rec["probe_iterations"] == 72 and rec["copies"] == 5 and rec["at_iteration"] == 72
    assert sorted(rec["ms_per_iteration"]) == [0, 1, 2]
    assert all(len(v) == 2 for v in rec["ms_per_iteration"].values())
    means = {s: sum(v) / 2 for s, v in rec["ms_per_iteration"].items()}
    assert means == pytest.approx({0: 2.1, 1: 1.9, 2: 1.95})
    # four moves along the schedule, then from set 0 (the last block's) to the chosen one
    assert [dst for _, dst in solver.moves] == [sets[1], sets[2], sets[1], sets[0], sets[1]]
    assert solver.moves[-1] == (sets[0], sets[1]) and solver.st is sets[1]


@pytest.mark.parametrize("flag", ["_serial_now", "_run_now"])
def test_tick_does_nothing_in_the_other_regimes(clock, flag):
    sets = _three_sets()
    solver = StandInSolver(sets[0])
    sel = PlacementSelection(sets, KEY, BLOCK)
    sel.start(solver)
    setattr(solver, flag, True)
    for k in (0, BLOCK, 6 * BLOCK):
        solver.k = k
        assert sel.tick(solver) is False
    assert clock.events == 0 and sel.open is None and sel.blocks == [] and solver.moves == []
    assert sel.record["state"] == "pending"


def test_third_start_without_a_finished_selection_abandons(clock):
    sets = _three_sets()
    solver = StandInSolver(sets[0])
    sel = PlacementSelection(sets, KEY, BLOCK)
    assert sel.start(solver) is False                      # a first solve that ends before the probe does
    assert sel.start(solver) is False                      # a second one, which gets as far as the second block
    opened, over = _race(sel, solver, clock, [2.0, 1.0], BLOCK + 3)
    assert opened == [(0, 0), (BLOCK, 1)] and not over and len(solver.moves) == 1
    assert sel.start(solver) is True
    rec = sel.record
    assert rec["state"] == "abandoned" and rec["chosen"] == 1       # the set in use, not the fastest measured
    assert solver.st is sets[1] and len(solver.moves) == 1          # nothing moved


def test_finished_selection_leases_the_streams_to_the_solver(clock):
    sets = _three_sets()
    solver = StandInSolver(sets[0])
    sel = PlacementSelection(sets, KEY, BLOCK)
    sel.start(solver)
    _race(sel, solver, clock, [2.0, 1.9, 2.1, 1.8, 1.9, 2.2], 6 * BLOCK)
    rec = sel.record
    assert PlacementPool.take(KEY) is None                 # leased: not free while the solver lives
    del solver
    gc.collect()
    assert PlacementPool.take(KEY) == (sets[1], rec)
    assert PlacementPool.take(KEY) is None
