"""Per-lane models in the Newton solve and the per-lane LQR design, CPU side: the yardstick's anchors
(tests/newton_models_ref.py on set 1 is the box restatement / the LQR oracle exactly), check_models, the keyword's
refusals, the extension header's binding and host checks, the engine's call lists and the checkpoint field.  No kernel
is launched here."""
import ctypes as C
import dataclasses
import inspect
import os

import numpy as np
import pytest
import torch

import newton_box_ref as nb
import newton_models_ref as nm
from conftest import load_golden
from gymnast_optimalcontrol_amd import _build, _lib, engine as en
from gymnast_optimalcontrol_amd import trajectory_tracking as tt
from gymnast_optimalcontrol_amd.params import PARAM_NAMES, PARAM_SETS
from oracle import tracking_np as otr
from test_engine_launch_host import B, CASES, EXPECTED, Q4, T, lanes, rig, run  # noqa: F401  (rig: a fixture)

SHORT = dict(tol=1e-4, beta=0.7, c=0.5, max_ls=20)
SET1 = np.array([PARAM_SETS[1][k] for k in PARAM_NAMES])
NAMES = ("gym_newton_init_models", "gym_newton_run_models", "gym_newton_sigma_models", "gym_lqr_lanes_gains_models")


# ------------------------------------------------------------------------------------------- the yardstick's anchors
@pytest.mark.parametrize("tau", [np.inf, 2.0])
def test_on_set_1_the_restatement_is_the_box_restatement_exactly(task2_refs, tau):
    x0, xr, ur = nm.short_setup(task2_refs[0], task2_refs[1])
    a = nb.newton_box_solve(x0, xr, ur, 25, tau, gamma_0=0.5, **SHORT)
    b = nm.newton_models_solve(x0, xr, ur, 25, tau, [1] * 5, gamma_0=0.5, **SHORT)
    for k in b:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_a_lane_of_the_restatement_depends_on_its_own_key_only(task2_refs):
    x0, xr, ur = nm.short_setup(task2_refs[0], task2_refs[1])
    keys = nm.keys_of(5)
    assert keys == [1, "heavy", "sticky", 2, 1] and nm.KEYS == (1, "heavy", "sticky", 2) and nm.NAMES == PARAM_NAMES
    mixed = nm.newton_models_solve(x0, xr, ur, 6, 2.0, keys, gamma_0=0.5, **SHORT)
    for b in (1, 3):
        one = nb.newton_box_solve(x0[b:b + 1], xr, ur, 6, 2.0, gamma_0=0.5, pset=keys[b], **SHORT)
        for f in ("x", "u", "K", "sigma", "cost", "n_iter", "n_rollouts", "status"):
            assert np.array_equal(mixed[f][b], one[f][0]), (b, f)
    base = nb.newton_box_solve(x0, xr, ur, 6, 2.0, gamma_0=0.5, **SHORT)
    same = [np.array_equal(mixed["x"][b], base["x"][b]) for b in range(5)]
    assert same == [True, False, False, False, True]                 # the keys are not decoration
    par = nm.params_of(keys)
    assert par.shape == (5, 11) and np.array_equal(par[0], SET1) and par[1, 1] == 1.1 and par[2, 9] == 1.5
    assert np.array_equal(par[3], [PARAM_SETS[2][k] for k in PARAM_NAMES])


def test_lqr_restatement_on_set_1_is_the_oracle_exactly():
    g = load_golden("lanes")
    x, u = g["x"][:2, :22], g["u"][:2, :21]
    for b in range(2):
        assert np.array_equal(nm.solve_LQR_tracking(x[b], u[b]), otr.solve_LQR_tracking(x[b], u[b]))
    K = nm.lqr_gains(x, u, ["heavy", 1])
    assert np.array_equal(K[1], otr.solve_LQR_tracking(x[1], u[1]))
    assert not np.array_equal(K[0], otr.solve_LQR_tracking(x[0], u[0]))


# ------------------------------------------------------------------------------------------------- check_models
def test_check_models_forms_and_check_plants_wording():
    own = PARAM_SETS[1]
    want = np.broadcast_to(SET1, (3, 11))
    for form in (1, {}, dict(m2=1.0), SET1, np.tile(SET1, (3, 1)), np.tile(SET1, (3, 1, 1)), torch.as_tensor(SET1),
                 tt.sample_plants(3, 1, rel=0.0)):
        got = en.check_models(form, 3, own)
        assert got.shape == (3, 11) and got.dtype == np.float64 and np.array_equal(got, want), form
    per_b = SET1 * np.array([1.0, 1.1, 1.2])[:, None]
    assert np.array_equal(en.check_models(per_b, 3, own), per_b)
    assert np.array_equal(en.check_models(per_b[:, None], 3, own), per_b)
    assert np.array_equal(en.check_models(per_b[:1], 1, own), per_b[:1])          # one lane
    got = en.check_models({"m2": np.array([1.0, 1.1, 1.2]), "f1": 2.0}, 3, own)   # (B,) arrays are per lane
    assert got[:, 1].tolist() == [1.0, 1.1, 1.2] and (got[:, 9] == 2.0).all()
    assert np.array_equal(en.check_models(2, 3, own)[1], [PARAM_SETS[2][k] for k in PARAM_NAMES])
    s = tt.sample_plants(3, 1, seed=5)
    assert np.array_equal(en.check_models(s, 3, own), s[:, 0])
    for form, words in ((dict(m3=1.0), "unknown plant parameter 'm3'"), (0, "plant set"), (4, "plant set"),
                        (np.zeros(10), "plant rows must hold 11 parameters"),
                        (np.tile(SET1, (4, 1)), "does not broadcast"), (np.tile(SET1, (3, 2, 1)), "does not broadcast"),
                        (dict(m2=np.ones(2)), "does not broadcast"), (dict(m2=np.nan), "must be finite"),
                        (SET1 * np.array([1.0] * 10 + [np.inf]), "must be finite")):
        with pytest.raises(ValueError, match=words):
            en.check_models(form, 3, own)
    en.check_model_table(torch.zeros((3, 8), dtype=torch.float64), 3)
    for bad in (torch.zeros((3, 1, 8), dtype=torch.float64), torch.zeros((3, 8), dtype=torch.float32),
                np.zeros((3, 8)), torch.zeros((2, 8), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"models must be a model_table \(3,8\) float64 tensor"):
            en.check_model_table(bad, 3)


# ------------------------------------------------------------------------------- the header and its entry points
def test_models_header_parses_and_its_exports_are_complete():
    ext = _lib.EXTENSIONS
    assert ext["gymnast_acrobot_models.h"] == NAMES
    assert _lib.EXTENSION_HEADERS == ("gymnast_acrobot_box.h", "gymnast_acrobot_models.h", "gymnast_acrobot_rk4lin.h")
    assert tuple(ext) == _lib.EXTENSION_HEADERS                      # each header's entry points, in the list's order
    assert _lib.ALL_EXPORTS == (_lib.EXPORTS + ext["gymnast_acrobot_box.h"] + ext["gymnast_acrobot_models.h"] +
                                ext["gymnast_acrobot_rk4lin.h"])
    assert ext["gymnast_acrobot_box.h"] == ("gym_newton_run_box", "gym_newton_sigma_box")
    assert ext["gymnast_acrobot_rk4lin.h"] == ("gym_linearize_rk4", "gym_newton_run_rk4", "gym_newton_sigma_rk4")
    assert not set(NAMES) & set(_lib.EXPORTS)
    assert any(p.endswith("gymnast_acrobot_models.h") for p in _build.DEPS)
    assert any(p.endswith("newton_models.hpp") for p in _build.DEPS)
    P, S = _lib._P, C.POINTER
    sig = _lib._EXT_SIGS
    # each mirrors its entry point with the table (an address, as gym_lqr_lanes_rollout_plant's) right after the model
    box = sig["gym_newton_run_box"]
    assert sig["gym_newton_run_models"] == box[:1] + [P] + box[1:]
    sb = sig["gym_newton_sigma_box"]
    assert sig["gym_newton_sigma_models"] == sb[:1] + [P] + sb[1:]
    assert sig["gym_newton_init_models"] == [S(_lib.GymModel), P, S(_lib.GymWeights), P, P, P, S(_lib.GymBatch), P]
    lq = _lib._SIGS["gym_lqr_lanes_gains"]
    assert sig["gym_lqr_lanes_gains_models"] == lq[:1] + [P] + lq[1:]
    assert _lib._SIGS["gym_lqr_lanes_rollout_plant"][1] is P
    with open(os.path.join(_build.INCLUDE, "gymnast_acrobot_models.h")) as f:
        text = f.read()
    assert '#include "gymnast_acrobot.h"' in text and "typedef" not in text and "#define GYM_" not in text
    lib = _lib.load(_build.build())
    for name in NAMES:
        assert getattr(lib, name).argtypes == sig[name]


def _batch(B=64, Bp=64, N=41, flags=0, D=0x10000):
    b = _lib.GymBatch(B=B, Bp=Bp, N=N, flags=flags)
    for f, t in _lib.GymBatch._fields_:
        if f in ("x", "u"):
            getattr(b, f)[0] = getattr(b, f)[1] = D
        elif t is _lib._P and f not in ("hist_cost", "hist_smax", "lane_map"):
            setattr(b, f, D)
    return b


def test_every_refusal_of_the_newton_entry_points_launches_nothing():
    """GYM_EINVAL (1) from the host-side checks, before any HIP call: this machine has no device, so a call that got
    past them would return a HIP error code, not 1."""
    lib = _lib.load(_build.build())
    R = C.byref
    D = 0x10000
    m, w, a = _lib.GymModel(dt=0.02), _lib.GymWeights(), _lib.GymArmijo(1e-4, 0.7, 0.5, 0.1, 20, 0)
    tbl = D
    ok = _batch()
    run_ = lambda mm=R(m), t=tbl, ww=R(w), aa=R(a), b=ok, tau=D, k0=0, k1=1: lib.gym_newton_run_models(  # noqa: E731
        mm, t, ww, aa, R(b) if b is not None else None, tau, k0, k1, None)
    sig_ = lambda mm=R(m), t=tbl, ww=R(w), b=ok, tau=D, out=D: lib.gym_newton_sigma_models(  # noqa: E731
        mm, t, ww, R(b) if b is not None else None, tau, out, None)
    ini_ = lambda mm=R(m), t=tbl, ww=R(w), x0=D, u=None, st=None, b=ok: lib.gym_newton_init_models(  # noqa: E731
        mm, t, ww, x0, u, st, R(b) if b is not None else None, None)
    # the table: NULL, and every misalignment of a 16-byte boundary
    for bad in [None] + [D + o for o in (1, 4, 8, 12, 24)]:
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
    # the two flags no models entry point takes
    for flag in (_lib.FLAG_X_CKPT, _lib.FLAG_SIGMA_STREAM):
        b = _batch(flags=flag)
        assert run_(b=b) == 1 and sig_(b=b) == 1 and ini_(b=b) == 1 and ini_(b=b, u=D) == 1, flag


def test_every_refusal_of_the_lqr_entry_point_launches_nothing():
    lib = _lib.load(_build.build())
    D = 0x10000
    m = _lib.GymModel(dt=0.02)
    Q = np.ascontiguousarray(otr.Q_REG); R = np.ascontiguousarray(otr.R_REG); QT = np.ascontiguousarray(otr.QT_REG)
    tbl = D
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(mm=C.byref(m), t=tbl, x=D, u=D, Bn=3, Nn=5, q=None, r=None, qt=None, ws=D, nb_=1 << 30):
        return lib.gym_lqr_lanes_gains_models(mm, t, x, u, Bn, Nn, p(Q) if q is None else q, p(R) if r is None else r,
                                              p(QT) if qt is None else qt, ws, nb_, None, None)

    for bad in [None] + [D + o for o in (1, 8, 24)]:
        assert call(t=bad) == 1, bad
    assert call(mm=None) == 1 and call(x=None) == 1 and call(u=None) == 1 and call(ws=None) == 1
    assert call(Bn=0) == 1 and call(Nn=1) == 1 and call(nb_=16) == 1                        # sizes, a short workspace
    Rbad = np.array([[1.0, 0.5], [0.5, 1.0]])
    Qbad = np.ascontiguousarray(otr.Q_REG + np.triu(np.ones((4, 4)), 1))
    assert call(r=p(Rbad)) == 1 and call(q=p(Qbad)) == 1 and call(qt=p(Qbad)) == 1


# ------------------------------------------------------------------------------------ what the engine hands over
def test_model_table_is_plant_tables_call_and_upload(rig):
    eng, lib = rig
    par = nm.params_of(nm.keys_of(B))
    lib.calls.clear()
    table = eng.model_table(par, B)
    assert [c[0] for c in lib.calls] == ["gym_models_from_params"]
    args = lib.calls[0][1]
    assert len(args) == 4 and args[1:3] == (B, eng.dt)                                       # no stream: a host call
    assert table.shape == (B, 8) and table.dtype == torch.float64 and table.is_contiguous()
    seen = []
    lib.gym_models_from_params = lambda p, n, dt, out: seen.append(
        np.array((C.c_double * (11 * n)).from_address(p)).reshape(n, 11)) or 0
    eng.model_table(par, B)
    assert np.array_equal(seen[0], par)
    lib.gym_models_from_params = lambda *a: 1
    with pytest.raises(ValueError, match="mass matrix is not positive definite"):
        eng.model_table(1, B)
    with pytest.raises(ValueError, match="must be finite"):
        eng.model_table(dict(m1=np.nan), B)


def test_lqr_lanes_gains_call_lists_with_and_without_a_table(rig):
    table = T(B, 8)
    for case in ("lqr_lanes_gains", "lqr_lanes_gains_ws_no_gains"):
        method, make = CASES[case]
        _, plain = run(rig, method, **make())
        assert plain == EXPECTED[case]                                                       # untouched without one
        _, calls = run(rig, method, **make(), models=table)
        want = [c if c[0] != "gym_lqr_lanes_gains" else ("gym_lqr_lanes_gains_models", c[1], "models") + c[2:]
                for c in EXPECTED[case]]
        assert calls == want and calls[-1][0] == "gym_lqr_lanes_gains_models"
    for bad in (T(B, 1, 8), T(B + 1, 8), np.zeros((B, 8))):
        with pytest.raises(ValueError, match="models must be a model_table"):
            run(rig, "lqr_lanes_gains", **lanes(QT=Q4.copy()), models=bad)
        assert not any("gains" in c[0] for c in rig[1].calls)


# --------------------------------------------------------------------------------------------- the keyword
def test_the_keyword_reaches_every_front_end():
    from gymnast_optimalcontrol_amd import solver, trajectory_generation as tg
    for fn in (solver.BatchedNewtonSolver.__init__, solver.newton_solve_batch, tg.newton_Algorithm_batch,
               en.AcrobotEngine.lqr_lanes_gains, tt.LQR_tracking_lanes):
        assert inspect.signature(fn).parameters["models"].default is None, fn
    assert "models" not in inspect.signature(tg.newton_Algorithm).parameters
    assert "models" not in inspect.signature(tt.MPC_tracking_lanes).parameters


def test_what_a_models_solver_refuses_before_any_launch(rig, task2_refs):
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    eng, lib = rig
    _, xr, ur = nm.short_setup(task2_refs[0], task2_refs[1])
    par = nm.params_of(nm.keys_of(5))
    with pytest.raises(ValueError, match='do not combine with linearization="rk4"'):
        BatchedNewtonSolver(eng, xr, ur, 5, models=par, linearization="rk4")
    with pytest.raises(ValueError, match='do not combine with linearization="rk4"'):
        BatchedNewtonSolver(eng, xr, ur, 5, models=par, linearization="rk4", tau_max=2.0)
    for kw in (dict(pipeline=True), dict(checkpoint=True), dict(persistent=False)):
        with pytest.raises(ValueError, match=r"per-lane models \(models=\) runs the persistent schedule only"):
            BatchedNewtonSolver(eng, xr, ur, 5, models=par, **kw)
        with pytest.raises(ValueError, match="torque-limited"):                               # the limit names itself
            BatchedNewtonSolver(eng, xr, ur, 5, models=par, tau_max=2.0, **kw)
    for bad, words in ((dict(mass=1.0), "unknown plant parameter"), (np.tile(SET1, (4, 1)), "does not broadcast"),
                       (dict(m1=np.inf), "must be finite"), (7, "plant set")):
        with pytest.raises(ValueError, match=words):
            BatchedNewtonSolver(eng, xr, ur, 5, models=bad)
    lib.gym_models_from_params = lambda *a: 1
    with pytest.raises(ValueError, match="mass matrix is not positive definite"):
        BatchedNewtonSolver(eng, xr, ur, 5, models=par)
    assert not any(c[0].startswith("gym_newton") for c in lib.calls)


def _result(**extra):
    from gymnast_optimalcontrol_amd.results import SolveResult
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    i = lambda: torch.zeros(2, dtype=torch.int32)         # noqa: E731
    return SolveResult(x=z(2, 5, 4), u=z(2, 4, 2), K=z(2, 4, 2, 4), sigma=z(2, 4, 2), cost=z(2), n_iter=i(),
                       status=i(), n_rollouts=i(), gamma=z(2), iterations=0, lane_iterations=0, seconds=0.0, **extra)


def test_trackers_of_a_result_planned_on_models(monkeypatch):
    seen = []
    monkeypatch.setattr(tt, "LQR_tracking_lanes", lambda *a, **k: seen.append(("lqr", k)))
    monkeypatch.setattr(tt, "MPC_tracking_lanes", lambda *a, **k: seen.append(("mpc", k)))
    par = nm.params_of(["heavy", 2])
    r, plain = _result(models=par), _result()
    r.track_lqr()
    assert seen[-1][0] == "lqr" and seen[-1][1]["models"] is par
    r.track_lqr(models=None, plant=1)
    assert seen[-1][1] == dict(models=None, plant=1)
    plain.track_lqr()
    assert seen[-1][1] == dict(models=None)
    n = len(seen)
    with pytest.raises(NotImplementedError, match="track_lqr"):
        r.track_mpc()
    with pytest.raises(NotImplementedError, match="track_lqr"):
        r.track_mpc(tau_max=18.0)
    with pytest.raises(NotImplementedError, match="track_lqr"):
        plain.track_mpc(models=par)
    assert len(seen) == n
    r.track_mpc(models=None, T_pred=5)                    # said explicitly: the engine's model is meant
    assert seen[-1] == ("mpc", dict(T_pred=5))
    plain.track_mpc(T_pred=5)
    assert seen[-1] == ("mpc", dict(T_pred=5))


def test_front_end_refuses_bad_models_before_any_device():
    x, u = np.zeros((3, 5, 4)), np.zeros((3, 4, 2))
    for bad, words in ((dict(mass=1.0), "unknown plant parameter"), (np.zeros((3, 7)), "11 parameters"),
                       (np.tile(SET1, (5, 1)), "does not broadcast"), (dict(m1=np.nan), "must be finite")):
        with pytest.raises(ValueError, match=words):
            tt.LQR_tracking_lanes(x, u, x[:, 0], models=bad)


# ------------------------------------------------------------------------------------------- the checkpoint field
def test_solve_result_and_checkpoint_carry_the_models(tmp_path):
    from gymnast_optimalcontrol_amd.results import CHECKPOINT_KEYS, Checkpoint, SolveResult, load_checkpoint
    assert {x.name: x for x in dataclasses.fields(SolveResult)}["models"].default is None
    assert {x.name: x for x in dataclasses.fields(Checkpoint)}["models"].default is None
    par = nm.params_of(["sticky", 2])
    _result().save_npz(tmp_path / "plain.npz")
    _result(models=par).save_npz(tmp_path / "m.npz")
    assert set(np.load(tmp_path / "plain.npz").files) == set(CHECKPOINT_KEYS) | {"t"}        # today's wire format
    assert set(np.load(tmp_path / "m.npz").files) == set(CHECKPOINT_KEYS) | {"t", "models"}
    assert load_checkpoint(tmp_path / "plain.npz").models is None
    got = load_checkpoint(tmp_path / "m.npz").models
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.tobytes() == par.tobytes()
    a = dict(np.load(tmp_path / "m.npz"))
    a["models"] = par[:1]
    np.savez(tmp_path / "short.npz", **a)
    with pytest.raises(ValueError, match="'models' has shape"):
        load_checkpoint(tmp_path / "short.npz")


def test_resume_needs_the_same_models_bit_for_bit(tmp_path):
    """resume() compares before it touches the device: a stand-in solver with the two attributes it reads."""
    from gymnast_optimalcontrol_amd.results import load_checkpoint
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    par = nm.params_of(["sticky", 2])
    _result().save_npz(tmp_path / "plain.npz")
    _result(models=par).save_npz(tmp_path / "m.npz")
    plain, withm = load_checkpoint(tmp_path / "plain.npz"), load_checkpoint(tmp_path / "m.npz")

    class Stop(Exception):
        pass

    class Fake:
        linearization = "euler"
        B, N = 2, 5

        class eng:
            device = "cpu"

        def solve(self, *a, **k):
            raise Stop

    def resume(models, ck):
        s = Fake()
        s.models = models
        return BatchedNewtonSolver.resume(s, ck, 1)

    other = par.copy()
    other[1, 0] = np.nextafter(other[1, 0], np.inf)      # one ulp
    for models, ck in ((None, withm), (par, plain), (other, withm), (par[::-1].copy(), withm)):
        with pytest.raises(ValueError, match="per-lane models differ"):
            resume(models, ck)
    for models, ck in ((None, plain), (par.copy(), withm)):
        with pytest.raises(Stop):                         # past the check
            resume(models, ck)
