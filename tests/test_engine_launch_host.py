"""What AcrobotEngine hands the library, call by call: CPU only, no built library, no device.

A real AcrobotEngine runs on torch.device("cpu") against a stand-in library whose every entry point records
(name, args) and returns 0 (the workspace-size entry points answer WS_BYTES).  Every recorded argument is normalised:
a byref is the class name of the struct behind it (and must be the engine's own model / weights object), the stream is
"stream", ints, floats and None stay literal, and an address is the name of the caller's argument it points into or
the dtype and shape of the engine-allocated buffer it points into ("z:" in front where the engine zero-filled it,
"+bytes" behind where it points past the start).  EXPECTED holds the call list of every public method, each flag that
changes the list both ways; the order within a list is the enqueue order on the stream.

Shapes: B = 3 lanes (Bp = 64), N = 5 knots, P = 2 starts, windows of L = 3 stages, G = 2 step sizes, 6 points.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gymnast_optimalcontrol_amd import _lib, engine as en

STREAM = 0x5EED0001
WS_BYTES = 4096
F64 = torch.float64
DTYPES = {torch.float64: "f64", torch.int32: "i32", torch.uint8: "u8"}


class RecordingLib:
    """Every attribute is an entry point that records its call and succeeds."""

    def __init__(self):
        self.calls = []
        self.model_vec = None

    def __getattr__(self, name):
        def entry(*args):
            if name.endswith("_workspace"):
                args[-1]._obj.value = WS_BYTES
            if name == "gym_model_from_params":       # the parameter vector lives only as long as the constructor
                self.model_vec = list((C.c_double * 11).from_address(args[0]))
                args = ("params",) + args[1:]
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def rig(monkeypatch):
    lib = RecordingLib()
    monkeypatch.setattr(_lib, "require_device", lambda device=None, lib_path=None: torch.device("cpu"))
    monkeypatch.setattr(_lib, "load", lambda path=None: lib)
    monkeypatch.setattr(_lib, "stream_handle", lambda device=None: STREAM)
    eng = en.AcrobotEngine()
    return eng, lib


def _span(a):
    if isinstance(a, torch.Tensor):
        return a.data_ptr(), a.numel() * a.element_size()
    return a.ctypes.data, a.nbytes


def run(rig, method, **kw):
    """eng.method(**kw) -> (result, normalised call list).  Tensor / array keywords are the named inputs."""
    eng, lib = rig
    named = {k: v for k, v in kw.items() if isinstance(v, (torch.Tensor, np.ndarray))}
    made = []

    def wrap(fn, tag):
        def alloc(*a, **k):
            out = fn(*a, **k)
            made.append((tag + DTYPES[out.dtype] + str(tuple(out.shape)).replace(" ", ""), out))
            return out
        return alloc

    def label(v):
        if v is None or isinstance(v, (float, str)):
            return v
        if hasattr(v, "_obj"):                         # a ctypes byref
            obj = v._obj
            if not isinstance(obj, C.Structure):
                return "out"                           # the int64 a workspace-size entry point answers through
            assert obj is eng.model or obj is eng._w, "a byref of a struct that is not the engine's own"
            return type(obj).__name__
        assert isinstance(v, int), v
        if v == STREAM:
            return "stream"
        for name, a in list(named.items()) + made:
            base, nbytes = _span(a)
            if base <= v < base + nbytes:
                return name if v == base else f"{name}+{v - base}"
        assert v < 1 << 32, f"address {v:#x} is neither an input nor a buffer the engine allocated"
        return v

    lib.calls.clear()
    saved = torch.empty, torch.zeros, torch.empty_like
    torch.empty, torch.zeros, torch.empty_like = wrap(saved[0], ""), wrap(saved[1], "z:"), wrap(saved[2], "")
    try:
        out = getattr(eng, method)(**kw)
    finally:
        torch.empty, torch.zeros, torch.empty_like = saved
    return out, [(name,) + tuple(label(v) for v in args) for name, args in lib.calls]


# ------------------------------------------------------------------------------------------------------ inputs
B, BP, N, P, L, G, NPTS = 3, 64, 5, 2, 3, 2, 6
Q4 = np.diag([120.0, 100.0, 1e-4, 1e-4])
R2 = np.diag([1e-6, 10.0])


def T(*shape):
    return torch.rand(shape, dtype=F64)


def A(*shape):
    return np.random.default_rng(7).uniform(size=shape)


def traj(**over):
    d = dict(x=T(B, N, 4), u=T(B, N - 1, 2), x_ref=T(N, 4), u_ref=T(N - 1, 2))
    d.update(over)
    return d


def gains(**over):
    return traj(K=T(B, N - 1, 2, 4), sigma=T(B, N - 1, 2), **over)


def stages(n=4):
    return dict(A=T(n, 4, 4), Bm=T(n, 4, 2))


def pads():
    return dict(A_pad=T(4, 4), B_pad=T(4, 2))


def points():
    return dict(x=T(NPTS, 4), u=T(NPTS, 2))


def mpc(**over):
    return dict(x_ref=T(N, 4), u_ref=T(N - 1, 2), x_f=T(4), u_f=T(2), Q=Q4.copy(), R=R2.copy(), **over)


def box_qp(**over):
    Bm = A(4, 4, 2)
    Bm[:, :, 0] = 0.0
    return dict(A=A(4, 4, 4), Bm=Bm, u_ref=A(4, 2), Q=Q4.copy(), R=R2.copy(), QT=T(4, 4), x0=T(B, 4), L=L,
                tau_max=18.0, **over)


def box_rollout(**over):
    return dict(x0=T(B, 4), QT=T(4, 4), K_all=T(N - 1, L - 1, 2, 4), tau_max=18.0, **mpc(), **over)


def lanes(**over):
    return dict(x_opt=T(B, N, 4), u_opt=T(B, N - 1, 2), Q=Q4.copy(), R=R2.copy(), **over)


def ws():
    return torch.empty(WS_BYTES, dtype=torch.uint8)


CASES = {
    "pack_pairs": ("pack", lambda: dict(a=T(B, N, 4), Bp=BP)),
    "pack_planes": ("pack", lambda: dict(a=T(B, N - 1, 2), Bp=BP, W=1)),
    "unpack": ("unpack", lambda: dict(soa=T(N, 2, BP, 2), B=B)),
    "unpack_select": ("unpack", lambda: dict(soa=T(N, 2, BP, 2), B=B, soa1=T(N, 2, BP, 2),
                                             sel=torch.ones(B, dtype=torch.int32))),
    "continuous_dynamics": ("continuous_dynamics", points),
    "rk4": ("rk4", points),
    "jacobians": ("jacobians", points),
    "stage_cost_derivs": ("stage_cost_derivs", lambda: dict(points(), x_ref=T(NPTS, 4), u_ref=T(NPTS, 2),
                                                            Q=A(4, 4), R=A(2, 2))),
    "stage_cost_derivs_terminal": ("stage_cost_derivs", lambda: dict(x=T(NPTS, 4), x_ref=T(NPTS, 4), u=None,
                                                                     u_ref=None, Q=A(4, 4), R=None, terminal=True)),
    "rollout_open_loop": ("rollout_open_loop", lambda: dict(x0=T(B, 4), u=T(B, N - 1, 2), x_ref=T(N, 4),
                                                            u_ref=T(N - 1, 2))),
    "closed_loop": ("closed_loop", lambda: gains(gamma=T(B))),
    "closed_loop_one_gamma": ("closed_loop", lambda: gains(gamma=1.0)),
    "gamma_sweep": ("gamma_sweep", lambda: gains(gammas=T(G))),
    "total_cost": ("total_cost", lambda: traj(Q=A(4, 4), R=A(2, 2), QT=A(4, 4))),
    "backward": ("backward", traj),
    "backward_lambda": ("backward", lambda: traj(want_lambda=True)),
    "linearize": ("linearize", traj),
    "riccati_general": ("riccati_general", lambda: dict(A=T(B, 4, 4, 4), Bm=T(B, 4, 4, 2), Q=T(4, 4), R=T(2, 2),
                                                        S=T(2, 4), q=T(B, 4, 4), r=T(B, 4, 2), QT=T(4, 4),
                                                        qT=T(B, 4))),
    "tv_lqr_gains_all": ("tv_lqr_gains", lambda: dict(stages(), Q=Q4.copy(), R=R2.copy(), QT=T(4, 4), L=L)),
    "tv_lqr_gains_first_padded_discretized": ("tv_lqr_gains", lambda: dict(
        stages(), Q=Q4.copy(), R=R2.copy(), QT=T(4, 4), L=L, nwin=2, all_gains=False, discretize=True, **pads())),
    "dare_fixed_point": ("dare_fixed_point", lambda: dict(A=T(4, 4), Bm=T(4, 2), Q=Q4.copy(), R=R2.copy())),
    "mpc_gains": ("mpc_gains", lambda: mpc(L=L, nwin=2)),
    "mpc_gains_all": ("mpc_gains_all", lambda: mpc(L=L, nwin=2)),
    "lq_forward": ("lq_forward", lambda: dict(stages(), K=T(L - 1, 2, 4), x0=T(4), L=L)),
    "lq_forward_padded_discretized": ("lq_forward", lambda: dict(stages(), K=T(L - 1, 2, 4), x0=T(4), L=L,
                                                                 discretize=True, **pads())),
    "track_rollout": ("track_rollout", lambda: dict(x0=T(B, 4), x_ff=T(N, 4), u_ff=T(N - 1, 2), K=T(N - 1, 2, 4))),
    "track_rollout_single": ("track_rollout", lambda: dict(x0=T(B, 4), x_ff=T(N, 4), u_ff=T(N - 1, 2),
                                                           K=T(N - 1, 2, 4), single=True)),
    "mpc_box_workspace": ("mpc_box_workspace", lambda: dict(B=B, L=L, rows=4)),
    "mpc_box_qp": ("mpc_box_qp", box_qp),
    "mpc_box_qp_ws": ("mpc_box_qp", lambda: box_qp(ws=ws())),
    "mpc_box_rollout": ("mpc_box_rollout", box_rollout),
    "mpc_box_rollout_ws": ("mpc_box_rollout", lambda: box_rollout(ws=ws())),
    "lqr_lanes_workspace": ("lqr_lanes_workspace", lambda: dict(B=B, N=N)),
    "lqr_lanes_gains": ("lqr_lanes_gains", lambda: lanes(QT=Q4.copy())),
    "lqr_lanes_gains_ws_no_gains": ("lqr_lanes_gains", lambda: lanes(QT=Q4.copy(), gains=False, ws=ws())),
    "lqr_lanes_rollout": ("lqr_lanes_rollout", lambda: dict(ws=ws(), x0=T(B, P, 4), N=N)),
    "lqr_lanes_rollout_summary": ("lqr_lanes_rollout", lambda: dict(ws=ws(), x0=T(B, P, 4), N=N,
                                                                    trajectories=False)),
    "mpc_lanes_gains": ("mpc_lanes_gains", lambda: lanes(QT=T(4, 4), L=L)),
    "mpc_lanes_gains_ws_no_gains": ("mpc_lanes_gains", lambda: lanes(QT=T(4, 4), L=L, gains=False, ws=ws())),
    "mpc_box_lanes_workspace": ("mpc_box_lanes_workspace", lambda: dict(B=B, P=P, L=L)),
    "mpc_box_lanes_rollout": ("mpc_box_lanes_rollout", lambda: lanes(x0=T(B, P, 4), QT=T(4, 4), L=L, tau_max=18.0,
                                                                     max_ws_bytes=1 << 30)),
    "mpc_box_lanes_rollout_summary": ("mpc_box_lanes_rollout", lambda: lanes(
        x0=T(B, P, 4), QT=T(4, 4), L=L, tau_max=18.0, trajectories=False, max_ws_bytes=1 << 30)),
    "mpc_box_lanes_rollout_two_chunks": ("mpc_box_lanes_rollout", lambda: lanes(
        x0=T(B, P, 4), QT=T(4, 4), L=L, tau_max=18.0, max_ws_bytes=2 * WS_BYTES)),
}

PACK_X = ("gym_pack_lanes", "x", "f64(5,2,64,2)", 3, 64, 5, 4, 2, "stream")
PACK_U = ("gym_pack_lanes", "u", "f64(4,2,64,1)", 3, 64, 4, 2, 1, "stream")
PACK_K = ("gym_pack_lanes", "K", "f64(4,4,64,2)", 3, 64, 4, 8, 2, "stream")
PACK_SIGMA = ("gym_pack_lanes", "sigma", "f64(4,2,64,1)", 3, 64, 4, 2, 1, "stream")
UNPACK_X = ("gym_unpack_lanes", "f64(5,2,64,2)", None, None, "f64(3,5,4)", 3, 64, 5, 4, 2, "stream")
UNPACK_U = ("gym_unpack_lanes", "f64(4,2,64,1)", None, None, "f64(3,4,2)", 3, 64, 4, 2, 1, "stream")
UNPACK_GAINS = ("gym_unpack_gains", "f64(4,2,64,2)", "f64(3,4,2,4)", 3, 64, 4, "stream")
CLOSED_LOOP = [
    PACK_X, PACK_U, PACK_K, PACK_SIGMA,
    ("gym_closed_loop", "GymModel", "GymWeights", "f64(5,2,64,2)", "f64(4,2,64,1)", "f64(4,4,64,2)",
     "f64(4,2,64,1)", "z:f64(64,)", "x_ref", "u_ref", "f64(5,2,64,2)", "f64(4,2,64,1)", "f64(64,)", 3, 64, 5,
     "stream"),
    UNPACK_X, UNPACK_U,
]
EXPECTED = {
    "pack_pairs": [("gym_pack_lanes", "a", "f64(5,2,64,2)", 3, 64, 5, 4, 2, "stream")],
    "pack_planes": [("gym_pack_lanes", "a", "f64(4,2,64,1)", 3, 64, 4, 2, 1, "stream")],
    "unpack": [("gym_unpack_lanes", "soa", None, None, "f64(3,5,4)", 3, 64, 5, 4, 2, "stream")],
    "unpack_select": [("gym_unpack_lanes", "soa", "soa1", "sel", "f64(3,5,4)", 3, 64, 5, 4, 2, "stream")],
    "continuous_dynamics": [("gym_continuous_dynamics", "GymModel", "x", "u", "f64(6,4)", 6, "stream")],
    "rk4": [("gym_rk4_step", "GymModel", "x", "u", "f64(6,4)", 6, "stream")],
    "jacobians": [("gym_jacobians", "GymModel", "x", "u", "f64(6,4,4)", "f64(6,4,2)", 6, "stream")],
    "stage_cost_derivs": [
        ("gym_stage_cost_derivs", "x", "x_ref", "u", "u_ref", "Q", "R", 0, "f64(6,)", "f64(6,4)", "f64(6,2)", 6,
         "stream"),
    ],
    "stage_cost_derivs_terminal": [
        ("gym_stage_cost_derivs", "x", "x_ref", None, None, "Q", None, 1, "f64(6,)", "f64(6,4)", None, 6, "stream"),
    ],
    "rollout_open_loop": [
        PACK_U,
        ("gym_rollout_open_loop", "GymModel", "GymWeights", "x0", "f64(4,2,64,1)", "x_ref", "u_ref",
         "f64(5,2,64,2)", "f64(64,)", 3, 64, 5, "stream"),
        UNPACK_X,
    ],
    "closed_loop": CLOSED_LOOP,
    "closed_loop_one_gamma": CLOSED_LOOP,
    "gamma_sweep": [
        PACK_X, PACK_U, PACK_K, PACK_SIGMA,
        ("gym_gamma_sweep", "GymModel", "GymWeights", "f64(5,2,64,2)", "f64(4,2,64,1)", "f64(4,4,64,2)",
         "f64(4,2,64,1)", "gammas", 2, "x_ref", "u_ref", "f64(2,64)", 3, 64, 5, "stream"),
    ],
    "total_cost": [
        PACK_X, PACK_U,
        ("gym_total_cost", "f64(5,2,64,2)", "f64(4,2,64,1)", "x_ref", "u_ref", "Q", "R", "QT", "f64(64,)", 3, 64, 5,
         "stream"),
    ],
    "backward": [
        PACK_X, PACK_U,
        ("gym_backward_sweep", "GymModel", "GymWeights", "f64(5,2,64,2)", "f64(4,2,64,1)", "x_ref", "u_ref",
         "f64(4,2,64,2)", "f64(4,2,64,1)", "f64(64,)", "f64(64,)", None, 3, 64, 5, "stream"),
        UNPACK_GAINS, UNPACK_U,
    ],
    "backward_lambda": [
        PACK_X, PACK_U,
        ("gym_backward_sweep", "GymModel", "GymWeights", "f64(5,2,64,2)", "f64(4,2,64,1)", "x_ref", "u_ref",
         "f64(4,2,64,2)", "f64(4,2,64,1)", "f64(64,)", "f64(64,)", "f64(5,2,64,2)", 3, 64, 5, "stream"),
        UNPACK_GAINS, UNPACK_U, UNPACK_X,
    ],
    "linearize": [
        PACK_X, PACK_U,
        ("gym_linearize", "GymModel", "GymWeights", "f64(5,2,64,2)", "f64(4,2,64,1)", "x_ref", "u_ref",
         "f64(4,16,64)", "f64(4,8,64)", "f64(4,4,64)", "f64(4,2,64)", "f64(4,64)", 3, 64, 5, "stream"),
    ],
    "riccati_general": [
        ("gym_riccati_general", "z:f64(4,16,64)", "z:f64(4,8,64)", "z:f64(4,16,64)", "z:f64(4,4,64)",
         "z:f64(4,8,64)", "z:f64(4,4,64)", "z:f64(4,2,64)", "z:f64(16,64)", "z:f64(4,64)", "f64(4,8,64)",
         "f64(4,2,64)", "f64(64,)", 3, 64, 4, "stream"),
    ],
    "tv_lqr_gains_all": [
        ("gym_tv_lqr_gains", "A", "Bm", 4, None, None, "Q", "R", "QT", 3, 1, 1, 0, 0.02, "f64(2,2,4)", "stream"),
    ],
    "tv_lqr_gains_first_padded_discretized": [
        ("gym_tv_lqr_gains", "A", "Bm", 4, "A_pad", "B_pad", "Q", "R", "QT", 3, 2, 0, 1, 0.02, "f64(2,2,4)",
         "stream"),
    ],
    "dare_fixed_point": [
        ("gym_dare_fixed_point", "A", "Bm", "Q", "R", 1000, 1e-06, "f64(4,4)", "z:i32(1,)", "stream"),
    ],
    "mpc_gains": [
        ("gym_mpc_gains", "GymModel", "x_ref", "u_ref", 4, "x_f", "u_f", "Q", "R", 3, 2, 1000, 1e-06, "f64(2,2,4)",
         "f64(4,4)", "z:i32(1,)", "stream"),
    ],
    "mpc_gains_all": [
        ("gym_mpc_gains_all", "GymModel", "x_ref", "u_ref", 4, "x_f", "u_f", "Q", "R", 3, 2, 1000, 1e-06,
         "f64(2,2,2,4)", "f64(4,4)", "z:i32(1,)", "stream"),
    ],
    "lq_forward": [
        ("gym_lq_forward", "A", "Bm", 4, None, None, 0, 0.02, "K", "x0", 3, "f64(3,4)", "f64(2,2)", "stream"),
    ],
    "lq_forward_padded_discretized": [
        ("gym_lq_forward", "A", "Bm", 4, "A_pad", "B_pad", 1, 0.02, "K", "x0", 3, "f64(3,4)", "f64(2,2)", "stream"),
    ],
    "track_rollout": [
        ("gym_track_rollout_ex", "GymModel", "x0", "x_ff", "u_ff", "K", 3, 5, 0, "f64(3,5,4)", "f64(3,4,2)",
         "stream"),
    ],
    "track_rollout_single": [
        ("gym_track_rollout_ex", "GymModel", "x0", "x_ff", "u_ff", "K", 3, 5, 1, "f64(3,5,4)", "f64(3,4,2)",
         "stream"),
    ],
    "mpc_box_workspace": [("gym_mpc_box_workspace", 3, 3, 4, "out")],
    "mpc_box_qp": [
        ("gym_mpc_box_workspace", 3, 3, 4, "out"),
        ("gym_mpc_box_qp", "A", "Bm", "u_ref", 4, "Q", "R", "QT", "x0", 3, 3, 18.0, 32, "u8(4096,)", 4096,
         "f64(3,2,2)", "f64(3,3,4)", "i32(3,)", "i32(3,)", "stream"),
    ],
    "mpc_box_qp_ws": [
        ("gym_mpc_box_qp", "A", "Bm", "u_ref", 4, "Q", "R", "QT", "x0", 3, 3, 18.0, 32, "ws", 4096, "f64(3,2,2)",
         "f64(3,3,4)", "i32(3,)", "i32(3,)", "stream"),
    ],
    "mpc_box_rollout": [
        ("gym_mpc_box_workspace", 3, 3, 5, "out"),
        ("gym_mpc_box_rollout", "GymModel", "x0", "x_ref", "u_ref", "x_f", "u_f", "Q", "R", "QT", "K_all", 3, 5, 3,
         18.0, 32, "u8(4096,)", 4096, "f64(3,5,4)", "f64(3,4,2)", "i32(3,4)", "i32(3,)", "stream"),
    ],
    "mpc_box_rollout_ws": [
        ("gym_mpc_box_rollout", "GymModel", "x0", "x_ref", "u_ref", "x_f", "u_f", "Q", "R", "QT", "K_all", 3, 5, 3,
         18.0, 32, "ws", 4096, "f64(3,5,4)", "f64(3,4,2)", "i32(3,4)", "i32(3,)", "stream"),
    ],
    "lqr_lanes_workspace": [("gym_lqr_lanes_workspace", 3, 5, "out")],
    "lqr_lanes_gains": [
        ("gym_lqr_lanes_workspace", 3, 5, "out"),
        ("gym_lqr_lanes_gains", "GymModel", "x_opt", "u_opt", 3, 5, "Q", "R", "QT", "u8(4096,)", 4096,
         "f64(3,4,2,4)", "stream"),
    ],
    "lqr_lanes_gains_ws_no_gains": [
        ("gym_lqr_lanes_gains", "GymModel", "x_opt", "u_opt", 3, 5, "Q", "R", "QT", "ws", 4096, None, "stream"),
    ],
    "lqr_lanes_rollout": [
        ("gym_lqr_lanes_rollout", "GymModel", "x0", 3, 2, 5, "ws", 4096, "f64(3,2,5,4)", "f64(3,2,4,2)",
         "f64(3,3,2)", "stream"),
    ],
    "lqr_lanes_rollout_summary": [
        ("gym_lqr_lanes_rollout", "GymModel", "x0", 3, 2, 5, "ws", 4096, None, None, "f64(3,3,2)", "stream"),
    ],
    "mpc_lanes_gains": [
        ("gym_lqr_lanes_workspace", 3, 5, "out"),
        ("gym_mpc_lanes_gains", "GymModel", "x_opt", "u_opt", 3, 5, 3, "Q", "R", "QT", "u8(4096,)", 4096,
         "f64(3,4,2,4)", "stream"),
    ],
    "mpc_lanes_gains_ws_no_gains": [
        ("gym_lqr_lanes_workspace", 3, 5, "out"),
        ("gym_mpc_lanes_gains", "GymModel", "x_opt", "u_opt", 3, 5, 3, "Q", "R", "QT", "ws", 4096, None, "stream"),
    ],
    "mpc_box_lanes_workspace": [("gym_mpc_box_lanes_workspace", 3, 2, 3, "out")],
    "mpc_box_lanes_rollout": [
        ("gym_mpc_box_lanes_workspace", 1, 2, 3, "out"),
        ("gym_mpc_box_lanes_rollout", "GymModel", "x_opt", "u_opt", "x0", 3, 2, 5, 3, "Q", "R", "QT", 18.0, 32,
         "u8(12288,)", 12288, "f64(3,2,5,4)", "f64(3,2,4,2)", "f64(3,3,2)", "i32(3,2,4)", "i32(3,2)", "stream"),
    ],
    "mpc_box_lanes_rollout_summary": [
        ("gym_mpc_box_lanes_workspace", 1, 2, 3, "out"),
        ("gym_mpc_box_lanes_rollout", "GymModel", "x_opt", "u_opt", "x0", 3, 2, 5, 3, "Q", "R", "QT", 18.0, 32,
         "u8(12288,)", 12288, None, None, "f64(3,3,2)", None, "i32(3,2)", "stream"),
    ],
    "mpc_box_lanes_rollout_two_chunks": [            # lanes 0-1, then lane 2: every per-lane address moves on
        ("gym_mpc_box_lanes_workspace", 1, 2, 3, "out"),
        ("gym_mpc_box_lanes_rollout", "GymModel", "x_opt", "u_opt", "x0", 2, 2, 5, 3, "Q", "R", "QT", 18.0, 32,
         "u8(8192,)", 8192, "f64(3,2,5,4)", "f64(3,2,4,2)", "f64(3,2,2)", "i32(3,2,4)", "i32(3,2)", "stream"),
        ("gym_mpc_box_lanes_rollout", "GymModel", "x_opt+320", "u_opt+128", "x0+128", 1, 2, 5, 3, "Q", "R", "QT",
         18.0, 32, "u8(8192,)", 8192, "f64(3,2,5,4)+640", "f64(3,2,4,2)+256", "f64(3,1,2)", "i32(3,2,4)+64",
         "i32(3,2)+16", "stream"),
    ],
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_list(rig, case):
    method, make = CASES[case]
    _, calls = run(rig, method, **make())
    assert calls == EXPECTED[case]


def test_constructor_and_methods_without_a_launch(rig):
    eng, lib = rig
    assert [(n, a[0], a[1], a[2]._obj) for n, a in lib.calls] == [("gym_model_from_params", "params", eng.dt,
                                                                   eng.model)]
    assert lib.model_vec == [eng.params[k] for k in ("m1", "m2", "l1", "lc1", "l2", "lc2", "I1", "I2", "g", "f1",
                                                     "f2")]
    assert eng.lib is lib and eng.stream == STREAM
    for method, kw in (("t", dict(a=T(2, 4))), ("refs", dict(x_ref=T(N, 4), u_ref=T(N, 2))),
                       ("set_weights", dict(weights=en.Weights(R=(1.0, 2.0))))):
        assert run(rig, method, **kw)[1] == []
    assert list(eng._w.R) == [1.0, 2.0]


def test_every_public_method_is_covered():
    public = {n for n, f in vars(en.AcrobotEngine).items() if callable(f) and not n.startswith("_")}
    assert public - {"t", "refs", "set_weights", "unpack_gains"} == {m for m, _ in CASES.values()}


# ------------------------------------------------------------------------------------- the engine's own rules
# Everything below is new with the shared preludes: the size rules they carry, _call's own invariant, unpack_gains.
def test_unpack_gains_call_list_and_its_two_users(rig, monkeypatch):
    from gymnast_optimalcontrol_amd.solver import BatchedNewtonSolver
    eng, lib = rig
    K, calls = run(rig, "unpack_gains", K1=T(N - 1, 2, BP, 2), B=B)
    assert calls == [("gym_unpack_gains", "K1", "f64(3,4,2,4)", 3, 64, 4, "stream")] and K.shape == (B, N - 1, 2, 4)
    seen = []
    inner = en.AcrobotEngine.unpack_gains
    monkeypatch.setattr(en.AcrobotEngine, "unpack_gains", lambda self, K1, B: seen.append((K1, B)) or inner(self, K1, B))
    s = object.__new__(BatchedNewtonSolver)        # gains() reads nothing but the engine, K1 and B
    s.eng, s.K1, s.B = eng, T(N - 1, 2, BP, 2), B
    lib.calls.clear()
    assert s.gains().shape == (B, N - 1, 2, 4) and seen[0][0] is s.K1 and seen[0][1] == B
    assert [c[0] for c in lib.calls] == ["gym_unpack_gains"]
    assert run(rig, "backward", **traj())[1] == EXPECTED["backward"] and len(seen) == 2
    assert tuple(seen[1][0].shape) == (N - 1, 2, BP, 2) and seen[1][1] == B


def test_call_refuses_what_the_library_would_misread(rig):
    eng, lib = rig
    lib.calls.clear()
    for bad in (T(4, 4).t(), T(B, N, 4)[:, :, :2], np.zeros((4, 4), dtype=np.float32), np.zeros((4, 4)).T,
                np.zeros((4, 4), dtype=np.int64)):
        with pytest.raises(TypeError, match="gym_rk4_step"):
            eng._call("gym_rk4_step", eng.model, bad, 1)
    assert lib.calls == []
    need = C.c_int64()
    eng._call("gym_rk4_step", eng.model, T(1, 4), np.zeros(4), None, 2, 0.5, C.byref(need))
    eng._call("gym_lqr_lanes_workspace", 1, 2, C.byref(need), stream=False)
    (_, a), (_, b) = lib.calls
    assert a[0]._obj is eng.model and a[3:6] == (None, 2, 0.5) and a[6]._obj is need and a[7] == STREAM
    assert b[:2] == (1, 2) and b[2]._obj is need and len(b) == 3 and need.value == WS_BYTES


def test_short_workspace_is_refused_on_the_host_for_mpc_lanes_gains_only(rig):
    short = torch.empty(100, dtype=torch.uint8)
    with pytest.raises(ValueError, match="the workspace holds 100 bytes, 3 lanes of 5 knots need 4096"):
        run(rig, "mpc_lanes_gains", **lanes(QT=T(4, 4), L=L, ws=short))
    assert [c[0] for c in rig[1].calls] == ["gym_lqr_lanes_workspace"]
    _, calls = run(rig, "lqr_lanes_gains", **lanes(QT=Q4.copy(), ws=short))     # the library's to refuse
    assert [c[0] for c in calls] == ["gym_lqr_lanes_gains"] and calls[0][9:11] == ("ws", 100)
    with pytest.raises(TypeError, match="workspace"):
        run(rig, "lqr_lanes_rollout", ws=None, x0=T(B, P, 4), N=N)
    assert rig[1].calls == []


def small(**over):
    """The issue's undersized trajectory call: B = 2, N = 5, and whatever ``over`` cuts short."""
    d = dict(x=T(2, 5, 4), u=T(2, 4, 2), x_ref=T(5, 4), u_ref=T(4, 2))
    d.update(over)
    return d


def small_gains(**over):
    return small(**dict(dict(K=T(2, 4, 2, 4), sigma=T(2, 4, 2)), **over))


REFUSED = {   # case -> (method, arguments, the argument the refusal names)
    "closed_loop_everything_short": ("closed_loop", lambda: small_gains(u=T(2, 2, 2), sigma=T(2, 1, 2), gamma=1.0,
                                                                        x_ref=T(3, 4), u_ref=T(2, 2)), "u"),
    "closed_loop_sigma": ("closed_loop", lambda: small_gains(sigma=T(2, 1, 2), gamma=1.0), "sigma"),
    "closed_loop_sigma_lanes": ("closed_loop", lambda: small_gains(sigma=T(1, 4, 2), gamma=1.0), "sigma"),
    "closed_loop_reference": ("closed_loop", lambda: small_gains(gamma=1.0, x_ref=T(3, 4), u_ref=T(2, 2)), "x_ref"),
    "closed_loop_one_knot": ("closed_loop", lambda: small_gains(x=T(2, 1, 4), gamma=1.0), "x"),
    "gamma_sweep_u": ("gamma_sweep", lambda: small_gains(u=T(2, 2, 2), gammas=T(G)), "u"),
    "gamma_sweep_sigma": ("gamma_sweep", lambda: small_gains(sigma=T(2, 3, 2), gammas=T(G)), "sigma"),
    "backward_u_and_reference": ("backward", lambda: small(u=T(2, 1, 2), x_ref=T(3, 4), u_ref=T(2, 2)), "u"),
    "backward_reference": ("backward", lambda: small(x_ref=T(3, 4), u_ref=T(2, 2)), "x_ref"),
    "linearize_u_lanes": ("linearize", lambda: small(u=T(1, 4, 2)), "u"),
    "linearize_u_channels": ("linearize", lambda: small(u=T(2, 4, 1)), "u"),
    "total_cost_reference": ("total_cost", lambda: small(x_ref=T(2, 4), u_ref=T(1, 2), Q=A(4, 4), R=A(2, 2),
                                                         QT=A(4, 4)), "x_ref"),
    "total_cost_u_ref": ("total_cost", lambda: small(u_ref=T(1, 2), Q=A(4, 4), R=A(2, 2), QT=A(4, 4)), "u_ref"),
    "total_cost_u": ("total_cost", lambda: small(u=T(2, 3, 2), Q=A(4, 4), R=A(2, 2), QT=A(4, 4)), "u"),
    "stage_cost_derivs_references": ("stage_cost_derivs", lambda: dict(points(), x_ref=T(1, 4), u_ref=T(1, 2),
                                                                       Q=A(4, 4), R=A(2, 2)), "x_ref"),
    "stage_cost_derivs_u_ref": ("stage_cost_derivs", lambda: dict(points(), x_ref=T(NPTS, 4), u_ref=T(1, 2),
                                                                  Q=A(4, 4), R=A(2, 2)), "u_ref"),
    "stage_cost_derivs_u": ("stage_cost_derivs", lambda: dict(x=T(NPTS, 4), u=T(NPTS - 1, 2), x_ref=T(NPTS, 4),
                                                              u_ref=T(NPTS, 2), Q=A(4, 4), R=A(2, 2)), "u"),
    "stage_cost_derivs_terminal_x_ref": ("stage_cost_derivs", lambda: dict(
        x=T(NPTS, 4), x_ref=T(1, 4), u=None, u_ref=None, Q=A(4, 4), R=None, terminal=True), "x_ref"),
    "tv_lqr_gains_stages": ("tv_lqr_gains", lambda: dict(A=T(6, 4, 4), Bm=T(2, 4, 2), Q=Q4.copy(), R=R2.copy(),
                                                         QT=T(4, 4), L=L), "Bm"),
    "lq_forward_stages": ("lq_forward", lambda: dict(A=T(6, 4, 4), Bm=T(2, 4, 2), K=T(4, 2, 4), x0=T(4), L=5), "Bm"),
    "lq_forward_gains": ("lq_forward", lambda: dict(stages(), K=T(1, 2, 4), x0=T(4), L=5), "K"),
    "unpack_select": ("unpack", lambda: dict(soa=T(N, 2, BP, 2), B=40, soa1=T(N, 2, BP, 2),
                                             sel=torch.ones(1, dtype=torch.int32)), "sel"),
    "unpack_select_dtype": ("unpack", lambda: dict(soa=T(N, 2, BP, 2), B=B, soa1=T(N, 2, BP, 2),
                                                   sel=torch.ones(B, dtype=torch.int64)), "sel"),
    "unpack_second_source": ("unpack", lambda: dict(soa=T(N, 2, BP, 2), B=B, soa1=T(N - 1, 2, BP, 2),
                                                    sel=torch.ones(B, dtype=torch.int32)), "soa1"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_undersized_call_is_refused_before_any_launch(rig, case):
    method, make, name = REFUSED[case]
    with pytest.raises(ValueError, match=rf"^{name} must be .*, got "):
        run(rig, method, **make())
    assert rig[1].calls == []


def shapeless(calls):
    """A call list without its buffer shapes: engine buffers by dtype only, the transposes' row count erased."""
    rows = {"gym_pack_lanes": 5, "gym_unpack_lanes": 7}
    out = []
    for c in calls:
        c = [v.split("(")[0] if isinstance(v, str) and "(" in v else v for v in c]
        if c[0] in rows:
            c[rows[c[0]]] = "L"
        out.append(tuple(c))
    return out


TRAJECTORY_METHODS = {
    "closed_loop": lambda **o: dict(gains(gamma=T(B)), **o), "gamma_sweep": lambda **o: dict(gains(gammas=T(G)), **o),
    "backward": lambda **o: traj(want_lambda=True, **o), "linearize": traj,
    "total_cost": lambda **o: traj(Q=A(4, 4), R=A(2, 2), QT=A(4, 4), **o),
}
SPARE = {"u_and_sigma": lambda: dict(u=T(B, N, 2), sigma=T(B, N, 2)),
         "reference": lambda: dict(x_ref=T(N + 2, 4), u_ref=T(N + 1, 2)),
         "reference_untrimmed": lambda: dict(x_ref=T(N + 2, 4), u_ref=T(N + 2, 2))}


@pytest.mark.parametrize("spare", sorted(SPARE))
@pytest.mark.parametrize("method", sorted(TRAJECTORY_METHODS))
def test_spare_rows_pass_with_the_same_call_list(rig, method, spare):
    """The in-bounds neighbours of the refusals: one spare row of u and sigma, spare rows of the reference."""
    make = TRAJECTORY_METHODS[method]
    over = SPARE[spare]()
    if "sigma" not in make():
        over.pop("sigma", None)
    _, exact = run(rig, method, **make())
    _, got = run(rig, method, **make(**over))
    assert shapeless(got) == shapeless(exact) and len(got) == len(exact) > 2
    if spare != "u_and_sigma":
        assert got == exact                          # the reference is not copied: not even a shape differs
    else:
        assert ("gym_pack_lanes", "u", "f64(5,2,64,1)", 3, 64, 5, 2, 1, "stream") in got


def test_point_and_stage_neighbours_pass(rig):
    """Spare rows next to the other refusals: references of 8 points for 6, B of 6 stages for 4, 4 gains for L = 3."""
    _, got = run(rig, "stage_cost_derivs", **dict(points(), x_ref=T(8, 4), u_ref=T(8, 2), Q=A(4, 4), R=A(2, 2)))
    assert got == EXPECTED["stage_cost_derivs"]
    _, got = run(rig, "tv_lqr_gains", **dict(A=T(4, 4, 4), Bm=T(6, 4, 2), Q=Q4.copy(), R=R2.copy(), QT=T(4, 4), L=L))
    assert got == EXPECTED["tv_lqr_gains_all"]
    _, got = run(rig, "lq_forward", **dict(A=T(4, 4, 4), Bm=T(6, 4, 2), K=T(4, 2, 4), x0=T(4), L=L))
    assert got == EXPECTED["lq_forward"]
    _, got = run(rig, "unpack", **dict(soa=T(N, 2, BP, 2), B=B, soa1=T(N, 2, BP, 2),
                                       sel=torch.ones(BP, dtype=torch.int32)))
    assert got == EXPECTED["unpack_select"]
