"""Per-lane cost weights in the Newton solve, CPU side: the yardstick's anchors (tests/newton_weights_ref.py on the
default set is the box restatement exactly; its counts on the four sets), check_weights, the keyword's refusals, the
add-on header's binding and host checks, the engine's and the solver's call lists and the checkpoint field.  No kernel
is launched here."""
import ctypes as C
import dataclasses
import inspect
import os

import numpy as np
import pytest
import torch

import newton_box_ref as nb
import newton_weights_ref as nw
from gymnast_optimalcontrol_amd import _build, _lib, engine as en
from gymnast_optimalcontrol_amd.params import Q_DIAG, QT_DIAG, R_DIAG
from test_abi_binding_host import C_NAMES, cc, compile_only  # noqa: F401  (cc: a fixture)
from test_engine_launch_host import STREAM, rig  # noqa: F401  (rig: a fixture)

SHORT = dict(tol=1e-4, beta=0.7, c=0.5, max_ls=20)
OWN = np.array(Q_DIAG + R_DIAG + QT_DIAG, dtype=np.float64)
HEADER = "gymnast_newton_weights.h"
NAMES = ("gym_newton_init_weights", "gym_newton_run_weights", "gym_newton_sigma_weights")


@pytest.fixture(scope="module")
def short(task2_refs):
    return nw.short_setup(task2_refs[0], task2_refs[1])


# ------------------------------------------------------------------------------------------- the yardstick's anchors
@pytest.mark.parametrize("tau", [np.inf, 2.0])
def test_on_the_default_set_the_restatement_is_the_box_restatement_exactly(short, tau):
    x0, xr, ur = short
    a = nb.newton_box_solve(x0, xr, ur, 25, tau, gamma_0=0.5, **SHORT)
    b = nw.newton_weights_solve(x0, xr, ur, 25, tau, ["default"] * 5, gamma_0=0.5, **SHORT)
    for k in b:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(nw.rows_of(["default"])[0], OWN)               # the engine's defaults are the oracle's


@pytest.mark.parametrize("tau, iters, clamped, margin", [(np.inf, [20, 18, 20, 21, 20], [0, 0, 0, 0, 0], 3.8e-9),
                                                         (2.0, [17] * 5, [32, 26, 30, 32, 32], 5e-7)])
def test_the_restatements_counts_on_the_four_sets(short, tau, iters, clamped, margin):
    """What the GPU tests' cases were chosen by: every lane converges, far from a tie of any Armijo or stop decision."""
    x0, xr, ur = short
    names = nw.names_of(5)
    assert names == ["default", "stiff", "cheap", "soft_end", "default"] and nw.SETS == tuple(names[:4])
    r = nw.newton_weights_solve(x0, xr, ur, 60, tau, names, gamma_0=0.5, **SHORT)
    print("tau", tau, "n_iter", r["n_iter"], "clamped", r["clamped"].sum(1), "margin", r["margin"])
    assert (r["status"] == nb.CONVERGED).all() and r["n_iter"].tolist() == iters
    assert r["n_rollouts"].tolist() == iters and r["clamped"].sum(1).tolist() == clamped
    assert (r["margin"] >= margin).all() and margin > 1e3 * 3e-12
    # a lane depends on its own set only, and the sets are not decoration
    one = nb.newton_box_solve(x0[1:2], xr, ur, 60, tau, gamma_0=0.5, Q=np.diag(nw.diag_of("stiff")[0]), **SHORT)
    for f in ("x", "u", "K", "sigma", "cost", "n_iter", "n_rollouts", "status"):
        assert np.array_equal(r[f][1], one[f][0]), f
    base = nb.newton_box_solve(x0, xr, ur, 60, tau, gamma_0=0.5, **SHORT)
    same = [np.array_equal(r["x"][b], base["x"][b]) for b in range(5)]
    assert same[0] and same[4] and not any(same[1:4])
    rows = nw.rows_of(names)
    assert rows.shape == (5, 10) and np.array_equal(rows[1, :4], 4 * OWN[:4]) and rows[2, 5] == OWN[5] / 4
    assert np.array_equal(rows[3, 6:], 0.1 * OWN[6:]) and np.array_equal(rows[4], OWN)


# ------------------------------------------------------------------------------------------------- check_weights
def test_check_weights_forms():
    own = en.Weights()
    want = np.broadcast_to(OWN, (3, 10))
    for form in (en.Weights(), {}, dict(Q=Q_DIAG), dict(R=np.array(R_DIAG), QT=torch.as_tensor(QT_DIAG)), OWN,
                 np.tile(OWN, (3, 1)), torch.as_tensor(OWN), list(OWN)):
        got = en.check_weights(form, 3, own)
        assert got.shape == (3, 10) and got.dtype == np.float64 and got.flags.c_contiguous, form
        assert np.array_equal(got, want), form
    per_b = OWN * np.array([1.0, 2.0, 3.0])[:, None]
    assert np.array_equal(en.check_weights(per_b, 3, own), per_b)
    assert not np.shares_memory(en.check_weights(per_b, 3, own), per_b)             # never the caller's array
    assert np.array_equal(en.check_weights(per_b[:1], 1, own), per_b[:1])          # one lane
    got = en.check_weights(dict(Q=per_b[:, :4], R=(1e-3, 2.0)), 3, own)           # per lane and per batch, mixed
    assert np.array_equal(got[:, :4], per_b[:, :4]) and (got[:, 4:6] == [1e-3, 2.0]).all()
    assert np.array_equal(got[:, 6:], want[:, 6:])
    # a name left out takes the engine's value, not the default
    mine = en.Weights(Q=(1.0, 2.0, 3.0, 4.0), R=(0.5, 0.25), QT=(9.0, 8.0, 7.0, 6.0))
    got = en.check_weights(dict(R=(1.0, 1.0)), 2, mine)
    assert got.tolist() == [[1.0, 2.0, 3.0, 4.0, 1.0, 1.0, 9.0, 8.0, 7.0, 6.0]] * 2
    assert np.array_equal(en.check_weights(mine, 2, own)[1], [1.0, 2.0, 3.0, 4.0, 0.5, 0.25, 9.0, 8.0, 7.0, 6.0])
    assert np.array_equal(en.check_weights(nw.rows_of(nw.names_of(6)), 6, own), nw.rows_of(nw.names_of(6)))
    assert en.check_weights({}, 0, own).shape == (0, 10)                           # (the padding of a full batch)


def test_check_weights_refusals_in_their_words():
    own = en.Weights()
    bad_row = np.tile(OWN, (3, 1))
    for form, words in ((dict(S=Q_DIAG), "unknown weights key 'S': the keys are Q, R, QT"),
                        (dict(Q=np.ones(3)), r"weights\['Q'\] \(3,\) does not broadcast to \(3,4\)"),
                        (dict(R=np.ones((2, 2))), r"weights\['R'\] \(2, 2\) does not broadcast to \(3,2\)"),
                        (dict(QT=np.ones((3, 1, 4))), "does not broadcast"),
                        (np.zeros(9), r"weights rows must hold 10 values \(Q\[4\], R\[2\], QT\[4\]\)"),
                        (np.float64(1.0), "weights rows must hold 10 values"),
                        (np.tile(OWN, (4, 1)), r"weights \(4, 10\) does not broadcast to \(3,10\)"),
                        (np.tile(OWN, (3, 1, 1)), "does not broadcast")):
        with pytest.raises(ValueError, match=words):
            en.check_weights(form, 3, own)
    for col, value, words in ((4, 0.0, "weights of lane 1: R must be positive"),
                              (5, -1.0, "weights of lane 1: R must be positive"),
                              (5, np.inf, "weights of lane 1: R must be positive"),
                              (0, -1e-9, "weights of lane 1: Q must be non-negative"),
                              (2, np.nan, "weights of lane 1: Q must be non-negative"),
                              (9, -1.0, "weights of lane 1: Q_T must be non-negative"),
                              (7, np.inf, "weights of lane 1: Q_T must be non-negative")):
        rows = bad_row.copy()
        rows[1:, col] = value                                                       # lanes 1 and 2: the first is named
        with pytest.raises(ValueError, match=words):
            en.check_weights(rows, 3, own)
    with pytest.raises(ValueError, match="weights of lane 0: R must be positive"):
        en.check_weights(en.Weights(R=(0.0, 1.0)), 3, own)
    with pytest.raises(ValueError, match="weights of lane 2: Q must be non-negative"):
        en.check_weights(dict(Q=np.array([Q_DIAG, Q_DIAG, (1.0, 1.0, -1.0, 1.0)])), 3, own)
    zero = bad_row.copy()
    zero[:, :4] = 0.0
    zero[:, 6:] = 0.0
    assert np.array_equal(en.check_weights(zero, 3, own), zero)                     # Q = Q_T = 0 is allowed


# ------------------------------------------------------------------------------- the header and its entry points
def test_weights_header_parses_and_the_pinned_lists_are_unchanged():
    assert _lib.ADDON_HEADERS == (HEADER,) and _lib.ADDONS == {HEADER: NAMES}
    # ABI 18's lists: closed
    assert _lib.EXTENSION_HEADERS == ("gymnast_acrobot_box.h", "gymnast_acrobot_models.h", "gymnast_acrobot_rk4lin.h")
    assert tuple(_lib.EXTENSIONS) == _lib.EXTENSION_HEADERS
    assert _lib.ALL_EXPORTS == _lib.EXPORTS + sum((_lib.EXTENSIONS[h] for h in _lib.EXTENSION_HEADERS), ())
    assert len(_lib.EXPORTS) == 58 and _lib.ABI_VERSION == 18
    assert not set(NAMES) & set(_lib.ALL_EXPORTS) and not set(_lib._ADDON_SIGS) & set(_lib._EXT_SIGS)
    assert set(_lib._ADDON_SIGS) == set(NAMES)
    assert any(p.endswith(HEADER) for p in _build.DEPS) and any(p.endswith("newton_weights.hpp") for p in _build.DEPS)
    P, S = _lib._P, C.POINTER
    sig = _lib._ADDON_SIGS
    # each mirrors its entry point with the table (an address) right after the weights
    box = _lib._EXT_SIGS["gym_newton_run_box"]
    assert box[1] == S(_lib.GymWeights) and sig["gym_newton_run_weights"] == box[:2] + [P] + box[2:]
    sb = _lib._EXT_SIGS["gym_newton_sigma_box"]
    assert sig["gym_newton_sigma_weights"] == sb[:2] + [P] + sb[2:]
    warm = _lib._SIGS["gym_newton_init_warm"]
    assert sig["gym_newton_init_weights"] == warm[:2] + [P] + warm[2:]
    md = _lib._EXT_SIGS["gym_newton_init_models"]                                   # cold and warm in one, as models
    assert sig["gym_newton_init_weights"] == md[:1] + md[2:3] + [P] + md[3:]
    with open(os.path.join(_build.INCLUDE, HEADER)) as f:
        text = f.read()
    assert '#include "gymnast_acrobot.h"' in text and "typedef" not in text and "#define GYM_" not in text
    assert "enum" not in text and not HEADER.startswith("gymnast_acrobot_")
    lib = _lib.load(_build.build())
    for name in NAMES:
        assert getattr(lib, name).argtypes == sig[name] and getattr(lib, name).restype is C.c_int


def test_an_addon_header_that_declares_more_than_prototypes_is_refused(tmp_path, monkeypatch):
    """The extensions' rule, through the function both families call."""
    for name, text in (("x_struct.h", "typedef struct gym_s { double a; } gym_s;\nint gym_f(const gym_s* s);"),
                       ("x_const.h", "#define GYM_NEW 3\nint gym_f(void* s);"),
                       ("x_status.h", "enum { GYM_OOPS = 9 };\nint gym_f(void* s);")):
        (tmp_path / name).write_text(text)
    (tmp_path / "x_ok.h").write_text("int gym_f(const gym_model* m, const gym_weights rows[], void* stream);")
    monkeypatch.setattr(_build, "INCLUDE", str(tmp_path))
    sigs = {}
    assert _lib._prototypes_only(("x_ok.h",), sigs) == {"x_ok.h": ("gym_f",)}
    assert sigs == {"gym_f": [C.POINTER(_lib.GymModel), _lib._P, _lib._P]}
    for name in ("x_struct.h", "x_const.h", "x_status.h"):
        with pytest.raises(ImportError, match="declares more than prototypes"):
            _lib._prototypes_only((name,), {})


def test_the_prototypes_are_the_compilers(cc, tmp_path):  # noqa: F811
    """As tests/test_abi_binding_host.py does for the main header: a function pointer of the type the binding believes
    takes the header's function; one position widened must not compile."""
    with open(os.path.join(_build.INCLUDE, HEADER)) as f:
        protos = _lib._parse(f.read(), base=_lib._ABI).protos
    assert tuple(n for _, n, _ in protos) == NAMES and all(ret == "int" for ret, _, _ in protos)

    def source(sigs):
        lines = [f'#include "{HEADER}"']
        for i, (ret, name, args) in enumerate(protos):
            params = [text if t not in C_NAMES else C_NAMES[t] for t, (_, text) in zip(sigs[name], args)]
            lines.append(f"{ret} (*p_{i})({', '.join(params)}) = {name};")
        return "\n".join(lines) + "\n"

    sigs = dict(_lib._ADDON_SIGS)
    assert all(len(sigs[n]) == len(a) for _, n, a in protos)
    r = compile_only(cc, source(sigs), tmp_path, "wsigs")
    assert r.returncode == 0, r.stderr
    run = sigs["gym_newton_run_weights"]
    assert run[6] is C.c_int32 and [a for _, n, a in protos if n == NAMES[1]][0][2][1] == "const gym_weights weights[]"
    wrong = dict(sigs, gym_newton_run_weights=[C.c_int64 if i == 6 else t for i, t in enumerate(run)])
    r = compile_only(cc, source(wrong), tmp_path, "wwrong")
    assert r.returncode != 0 and "gym_newton_run_weights" in r.stderr, r.stderr


def _batch(B=64, Bp=64, N=41, flags=0, D=0x10000):
    b = _lib.GymBatch(B=B, Bp=Bp, N=N, flags=flags)
    for f, t in _lib.GymBatch._fields_:
        if f in ("x", "u"):
            getattr(b, f)[0] = getattr(b, f)[1] = D
        elif t is _lib._P and f not in ("hist_cost", "hist_smax", "lane_map"):
            setattr(b, f, D)
    return b


def test_every_refusal_of_the_entry_points_launches_nothing():
    """GYM_EINVAL (1) from the host-side checks, before any HIP call: this machine has no device, so a call that got
    past them would return a HIP error code, not 1."""
    lib = _lib.load(_build.build())
    R = C.byref
    D = 0x10000
    m, w, a = _lib.GymModel(dt=0.02), _lib.GymWeights(), _lib.GymArmijo(1e-4, 0.7, 0.5, 0.1, 20, 0)
    ok = _batch()
    run_ = lambda mm=R(m), ww=R(w), t=D, aa=R(a), b=ok, tau=D, k0=0, k1=1: lib.gym_newton_run_weights(  # noqa: E731
        mm, ww, t, aa, R(b) if b is not None else None, tau, k0, k1, None)
    sig_ = lambda mm=R(m), ww=R(w), t=D, b=ok, tau=D, out=D: lib.gym_newton_sigma_weights(  # noqa: E731
        mm, ww, t, R(b) if b is not None else None, tau, out, None)
    ini_ = lambda mm=R(m), ww=R(w), t=D, x0=D, u=None, st=None, b=ok: lib.gym_newton_init_weights(  # noqa: E731
        mm, ww, t, x0, u, st, R(b) if b is not None else None, None)
    # the table: NULL, and every misalignment of a 16-byte boundary
    for bad in [None] + [D + o for o in (1, 4, 8, 12, 24, 40)]:
        assert run_(t=bad) == 1 and sig_(t=bad) == 1 and ini_(t=bad) == 1 and ini_(t=bad, u=D) == 1, bad
    # the mirrored entry points' refusals
    assert run_(mm=None) == 1 and run_(ww=None) == 1 and run_(aa=None) == 1 and run_(b=None) == 1
    assert run_(tau=None) == 1 and run_(k0=5, k1=1) == 1 and run_(k0=-1) == 1
    assert run_(aa=R(_lib.GymArmijo(1e-4, 0.7, 0.5, 0.1, 0, 0))) == 1                       # max_ls < 1
    assert sig_(mm=None) == 1 and sig_(ww=None) == 1 and sig_(b=None) == 1 and sig_(tau=None) == 1
    assert sig_(out=None) == 1
    assert ini_(mm=None) == 1 and ini_(ww=None) == 1 and ini_(x0=None) == 1 and ini_(b=None) == 1
    assert ini_(u=D + 8) == 1                                                               # u_init misaligned
    for b in (_batch(B=0), _batch(B=65, Bp=64), _batch(B=60, Bp=100), _batch(N=1), _batch(Bp=_lib.MAX_BP + 64),
              _batch(flags=_lib.FLAG_REF_LANE | _lib.FLAG_X_CKPT)):
        assert run_(b=b) == 1 and sig_(b=b) == 1 and ini_(b=b) == 1 and ini_(b=b, u=D) == 1, (b.B, b.Bp, b.N, b.flags)
    # the two flags no weights entry point takes
    for flag in (_lib.FLAG_X_CKPT, _lib.FLAG_SIGMA_STREAM):
        b = _batch(flags=flag)
        assert run_(b=b) == 1 and sig_(b=b) == 1 and ini_(b=b) == 1 and ini_(b=b, u=D) == 1, flag


# ------------------------------------------------------------------------------------ what the host hands over
def test_weight_table_is_one_upload_and_no_call(rig):  # noqa: F811
    eng, lib = rig
    rows = nw.rows_of(nw.names_of(5))
    lib.calls.clear()
    table = eng.weight_table(rows, 5)
    assert lib.calls == []                                                           # host work and an upload only
    assert table.shape == (5, 10) and table.dtype == torch.float64 and table.is_contiguous()
    assert np.array_equal(table.numpy(), rows)
    eng.set_weights(en.Weights(R=(1.0, 2.0)))
    assert eng.weight_table({}, 2)[:, 4:6].tolist() == [[1.0, 2.0]] * 2              # the engine's own, as it is now
    with pytest.raises(ValueError, match="weights of lane 0: R must be positive"):
        eng.weight_table(dict(R=(0.0, 1.0)), 2)


def _calls(lib):
    return [(name, args) for name, args in lib.calls if name.startswith("gym_newton")]


def test_solver_call_lists_with_and_without_a_table(rig, short):  # noqa: F811
    """init, run, finalize and sigma of a box solve and of a weights solve: the same lists, the three entry points
    renamed and the table's address inserted after the engine's weights."""
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    eng, lib = rig
    x0, xr, ur = short
    rows = nw.rows_of(nw.names_of(5))

    def drive(**kw):
        s = BatchedNewtonSolver(eng, xr, ur, 5, gamma_0=0.5, tail_lanes=0, **SHORT, **kw)
        lib.calls.clear()
        s.init(x0)
        s._run(0, 3)
        s.finalize()
        s.sigma()
        u = torch.zeros((5, 40, 2), dtype=torch.float64)
        s.init(x0, u_init=u)
        return s, _calls(lib)

    box, plain = drive(tau_max=2.0)
    assert [c[0] for c in plain] == ["gym_newton_init", "gym_newton_run_box", "gym_newton_finalize",
                                     "gym_newton_sigma_box", "gym_newton_sigma_box", "gym_newton_init_warm"]
    assert box.weights_buf is None and box.lane_weights is None and box.kind.table is None
    for kw in (dict(weights=rows), dict(weights=rows, tau_max=2.0)):
        s, calls = drive(**kw)
        assert s.schedule == "persistent" and s.kind.table == "weights" and s._run_fn == "gym_newton_run_weights"
        assert s.weights_buf.shape == (64, 10) and s.weights_buf.data_ptr() % 16 == 0
        assert np.array_equal(s.weights_buf[:5].numpy(), rows) and np.array_equal(s.lane_weights, rows)
        assert np.array_equal(s.weights_buf[5:].numpy(), np.broadcast_to(OWN, (59, 10)))    # padding: the engine's
        assert (s._tau_in is None) == ("tau_max" not in kw)
        assert bool((s.tau_buf[:5] == (2.0 if "tau_max" in kw else np.inf)).all())
        tbl = s.weights_buf.data_ptr()
        assert [c[0] for c in calls] == ["gym_newton_init_weights", "gym_newton_run_weights", "gym_newton_finalize",
                                         "gym_newton_sigma_weights", "gym_newton_sigma_weights",
                                         "gym_newton_init_weights"]
        for (pn, pa), (wn, wa) in zip(plain, calls):
            assert pa[0]._obj is eng.model and wa[0]._obj is eng.model and wa[1]._obj is eng._w
            if wn == "gym_newton_finalize":
                assert len(wa) == len(pa) and wa[-2] is None and wa[-1] == STREAM    # sigma comes from its own entry
                continue
            assert wa[2] == tbl and wa[-1] == STREAM, wn
            rest = wa[3:]
            if pn == "gym_newton_init":                                            # cold start: no controls, no statuses
                assert rest[1:3] == (None, None)
                rest = rest[:1] + rest[3:]
            assert len(rest) == len(pa[2:])
            for x, y in zip(rest, pa[2:]):                                          # scalars equal, structs the solver's
                assert (x == y) if isinstance(x, int) and x < 1 << 20 else (type(x) is type(y)), wn
        run = calls[1][1]
        assert run[3]._obj is s.armijo and run[4]._obj is s.batch and run[5] == s.tau_buf.data_ptr()
        assert run[6:8] == (0, 3)
    # the rows follow the lanes' internal order (init's _ref_perm), the caller's copy stays
    s, _ = drive(weights=rows)
    perm = torch.as_tensor([4, 2, 0, 1, 3])
    s.init(x0[perm.numpy()], _ref_perm=perm)
    assert np.array_equal(s.weights_buf[:5].numpy(), rows[perm.numpy()]) and np.array_equal(s.lane_weights, rows)
    assert np.array_equal(s._weights_in.numpy(), rows)


def test_the_keyword_reaches_every_front_end():
    from gymnast_optimalcontrol_amd import solver, trajectory_generation as tg
    for fn in (solver.BatchedNewtonSolver.__init__, solver.newton_solve_batch, tg.newton_Algorithm_batch):
        assert inspect.signature(fn).parameters["weights"].default is None, fn
    assert "weights" not in inspect.signature(tg.newton_Algorithm).parameters


def test_what_a_weights_solver_refuses_before_any_launch(rig, short):  # noqa: F811
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    eng, lib = rig
    _, xr, ur = short
    rows = nw.rows_of(nw.names_of(5))
    lib.calls.clear()
    for kw in (dict(pipeline=True), dict(checkpoint=True), dict(persistent=False)):        # the limited solver's three
        with pytest.raises(ValueError, match=r"per-lane weights \(weights=\) runs the persistent schedule only: no "
                                             r"pipeline=True, persistent=False or checkpoint=True"):
            BatchedNewtonSolver(eng, xr, ur, 5, weights=rows, **kw)
        with pytest.raises(ValueError, match="torque-limited"):                               # the limit names itself
            BatchedNewtonSolver(eng, xr, ur, 5, weights=rows, tau_max=2.0, **kw)
    with pytest.raises(NotImplementedError, match=r"weights=\) do not combine with per-lane models \(models=\)"):
        BatchedNewtonSolver(eng, xr, ur, 5, weights=rows, models=1)
    with pytest.raises(NotImplementedError, match=r'weights=\) do not combine with linearization="rk4"'):
        BatchedNewtonSolver(eng, xr, ur, 5, weights=rows, linearization="rk4")
    with pytest.raises(NotImplementedError, match="do not combine"):
        BatchedNewtonSolver(eng, xr, ur, 5, weights=rows, linearization="rk4", tau_max=2.0)
    for bad, words in ((dict(P=Q_DIAG), "unknown weights key"), (np.tile(OWN, (4, 1)), "does not broadcast"),
                       (np.zeros(7), "must hold 10 values"), (dict(R=(0.0, 1.0)), "weights of lane 0: R must be positive"),
                       (dict(Q=np.array([Q_DIAG] * 4 + [(np.nan,) * 4])), "weights of lane 4: Q must be non-negative")):
        with pytest.raises(ValueError, match=words):
            BatchedNewtonSolver(eng, xr, ur, 5, weights=bad)
    s = BatchedNewtonSolver(eng, xr, ur, 5, weights=rows, tail_lanes=0)
    for call in (lambda: s.gamma_sweep([0.5]), s.stream_sigma):
        with pytest.raises(ValueError, match=r"not available on a solver with per-lane weights \(weights=\)"):
            call()
    assert not any(c[0].startswith("gym_newton") for c in lib.calls)


# ------------------------------------------------------------------------------------------- the checkpoint field
def _result(**extra):
    from gymnast_optimalcontrol_amd.results import SolveResult
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    i = lambda: torch.zeros(2, dtype=torch.int32)         # noqa: E731
    return SolveResult(x=z(2, 5, 4), u=z(2, 4, 2), K=z(2, 4, 2, 4), sigma=z(2, 4, 2), cost=z(2), n_iter=i(),
                       status=i(), n_rollouts=i(), gamma=z(2), iterations=0, lane_iterations=0, seconds=0.0, **extra)


def test_solve_result_and_checkpoint_carry_the_weights(tmp_path):
    from gymnast_optimalcontrol_amd.results import CHECKPOINT_KEYS, Checkpoint, SolveResult, load_checkpoint
    assert {x.name: x for x in dataclasses.fields(SolveResult)}["weights"].default is None
    assert {x.name: x for x in dataclasses.fields(Checkpoint)}["weights"].default is None
    rows = nw.rows_of(["cheap", "soft_end"])
    _result().save_npz(tmp_path / "plain.npz")
    _result(weights=rows).save_npz(tmp_path / "w.npz")
    assert set(np.load(tmp_path / "plain.npz").files) == set(CHECKPOINT_KEYS) | {"t"}        # an old file: no field
    assert set(np.load(tmp_path / "w.npz").files) == set(CHECKPOINT_KEYS) | {"t", "weights"}
    plain = load_checkpoint(tmp_path / "plain.npz")
    assert plain.weights is None and plain.models is None
    got = load_checkpoint(tmp_path / "w.npz").weights
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.tobytes() == rows.tobytes()
    a = dict(np.load(tmp_path / "w.npz"))
    a["weights"] = rows[:, :9]
    np.savez(tmp_path / "short.npz", **a)
    with pytest.raises(ValueError, match="'weights' has shape"):
        load_checkpoint(tmp_path / "short.npz")


def test_resume_needs_the_same_weights_bit_for_bit(tmp_path):
    """resume() compares before it touches the device: a stand-in solver with the attributes it reads."""
    from gymnast_optimalcontrol_amd.results import load_checkpoint
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    rows = nw.rows_of(["cheap", "soft_end"])
    _result().save_npz(tmp_path / "plain.npz")
    _result(weights=rows).save_npz(tmp_path / "w.npz")
    plain, withw = load_checkpoint(tmp_path / "plain.npz"), load_checkpoint(tmp_path / "w.npz")

    class Stop(Exception):
        pass

    class Fake:
        linearization = "euler"
        models = None
        B, N = 2, 5

        class eng:
            device = "cpu"

        def solve(self, *a, **k):
            raise Stop

    def resume(weights, ck):
        s = Fake()
        s.lane_weights = weights
        return BatchedNewtonSolver.resume(s, ck, 1)

    other = rows.copy()
    other[1, 5] = np.nextafter(other[1, 5], np.inf)       # one ulp
    for weights, ck in ((None, withw), (rows, plain), (other, withw), (rows[::-1].copy(), withw)):
        with pytest.raises(ValueError, match="per-lane weights differ"):
            resume(weights, ck)
    for weights, ck in ((None, plain), (rows.copy(), withw)):
        with pytest.raises(Stop):                         # past the check
            resume(weights, ck)
