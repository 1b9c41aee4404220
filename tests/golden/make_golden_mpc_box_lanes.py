"""Writes tests/golden/mpc_box_lanes.npz: recorded output of the CPU reference tests/mpc_box_lanes_ref.py (NumPy only).

No reference program can produce this fixture (the reference's torque-limited QP needs casadi / IPOPT); the active set
it records is tied to the QP by the condensed solve and the KKT certificate (tests/test_mpc_box_host.py,
tests/test_mpc_box_lanes_host.py).

    python tests/golden/make_golden_mpc_box_lanes.py          (about 5 s per lane)

Contents (tau_max = 18, T_pred = 75, full length): the torque-limited closed loop of every one of the 12 lanes of
lanes.npz along its own trajectory from the three starts of mpc_box_lanes_ref.starts:
  x0 (12,3,4), x (12,3,501,4), u (12,3,500,2), qp_iters (12,3,500) int32, unconverged (12,3) int32
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import box_qp_ref as bq  # noqa: E402
from mpc_box_lanes_ref import lanes_ref, starts  # noqa: E402

L = 75


def main():
    g = np.load(os.path.join(HERE, "lanes.npz"))
    x0 = starts(g["x"])
    ref = lanes_ref(g["x"], g["u"], x0, bq.TAU_MAX, L)
    np.savez_compressed(os.path.join(HERE, "mpc_box_lanes.npz"), x0=x0, x=ref["x"], u=ref["u"],
                        qp_iters=ref["qp_iters"], unconverged=ref["unconverged"], tau_max=bq.TAU_MAX, T_pred=L)
    conv = ref["unconverged"] == 0
    print("pairs without an unconverged QP", int(conv.sum()), "of", conv.size, "unconverged", ref["unconverged"].tolist())
    print("max sweeps on those pairs", int(ref["qp_iters"][conv].max()), "steps at the limit",
          (np.abs(ref["u"][..., 1]) == bq.TAU_MAX).sum(-1)[conv].tolist())


if __name__ == "__main__":
    main()
