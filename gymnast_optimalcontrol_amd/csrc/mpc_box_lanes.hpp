// Torque-limited per-lane MPC tracking: every lane tracks its OWN trajectory with the receding-horizon MPC of
// trajectory_tracking.py:43-67 under solver_mpc's test_constraints (:87-114), |u_opt_t + u_t| <= tau_max on every
// stage of every window (main.py: task_2's result fed to task_4 with the actuator limit, per lane).  Part of the
// tracking_kernels.hip translation unit (included inside its anonymous namespace).
//
// The QP is mpc_box.hpp's "Torque-limited MPC" (box_qp_lane and its three passes, unchanged); what differs
// from k_mpc_box_rollout is where the window comes from.  There every lane shares one reference, so a stage table and
// K_all (every gain of every window) are made once.  Here they are per-lane data, and a per-lane K_all (1.2 MB at
// N = 501, L = 75) cannot be stored: the wavefront makes both on the spot.
//
// Mapping: one single-wavefront workgroup = one lane b and one block of up to 64 of its P perturbed starts, so all
// threads share the lane's stage rows: the window's rows sit in an LDS ring, read at wave-uniform addresses, as in
// k_mpc_box_rollout.  Per control step s the wavefront
//   1. linearises the ring's new row, stage s + L - 2 of the lane (lqr_lane_stage on the lane-major x_opt / u_opt,
//      or on the pad x_f = (pi, 0, 0, 0), u_f = 0 past stage N - 2: selected inputs, k_mpc_lane_gains' rule);
//   2. runs the window's unconstrained recursion over the ring from P = Q_T (lqr_lane_step, k_mpc_lane_gains'
//      operations: its last gain is that kernel's K0_s bit for bit) and keeps every stage's gain in LDS: the QP's
//      first iterate Kw, which does not depend on the start;
//   3. solves each start's QP from e = x - x_opt[s] (box_qp_lane<false>), applies u_opt[s] + u_0, one RK4 step.
// Steps 1 and 2 are wave-uniform work (every thread computes the same values, thread 0 stores them).  The per-start
// sweep data (k, d, x, u, state) lives in a caller-allocated workspace, per lane in (slot, stage, start) layout: a
// full wavefront's accesses to one stage coalesce, and a lane with P < 64 starts pays for P, not for 64.
// With no bound active at any step this is k_mpc_lane_gains + k_lqr_lane_rollout bit for bit (tested).
// k_mpc_box_lane_rollout_fb is the same kernel text with box_qp_lane's projected-Newton fallback (mpc_box.hpp).
// No atomics; every loop is bounded (max_it sweeps, L - 1 stages, N - 1 steps); the only data-dependent exit is
// box_qp_lane's wave vote.  A lane's results depend on that lane's inputs and that start only.
#pragma once

#include "mpc_box.hpp"     // M44, BoxWin, BoxWs, box_qp_lane, box_apply, kBoxRow, kBoxSlots, wave_lds_order
#include "mpc_lanes.hpp"   // ML_ROWS; Sym4, lqr_lane_stage, lqr_lane_step of lqr_lanes.hpp

// workspace of B lanes x P starts, windows of L stages: the doubles of every (lane, start), then the stage states
struct BoxLanesLayout {
    int64_t per_d, off_st, bytes;   // doubles per (lane, start); byte offset of the states
};
inline BoxLanesLayout box_lanes_layout(int64_t B, int64_t P, int L) {
    BoxLanesLayout o;
    o.per_d = (int64_t)kBoxSlots * (L - 1) + 4;
    o.off_st = 8 * B * P * o.per_d;
    o.bytes = o.off_st + 4 * B * P * (L - 1);
    return o;
}

// Row `dst` (kBoxRow doubles of LDS) of the lane's stage gs: A_d, b = B_d[:, 1], u_opt[gs]; the pad at or past T
__device__ __forceinline__ void box_lane_row(const Dyn& m, const double2* __restrict__ xl,
                                             const double2* __restrict__ ul, int gs, int T, bool store, double* dst) {
    const bool own = gs < T;                                // the lane's own stage; else the pad (x_f, u_f)
    const int gi = own ? gs : 0;
    double2 xa = xl[2 * gi], xb = xl[2 * gi + 1], uu = ul[gi];
    xa = own ? xa : make_double2(3.14159265358979323846, 0.0);
    xb = own ? xb : make_double2(0.0, 0.0);
    uu = own ? uu : make_double2(0.0, 0.0);
    double a2[4], a3[4], b2, b3;
    lqr_lane_stage(m, xa, xb, uu.y, a2, a3, b2, b3);
    if (!store) return;
    dst[0] = 1.0; dst[1] = 0.0; dst[2] = m.h; dst[3] = 0.0;
    dst[4] = 0.0; dst[5] = 1.0; dst[6] = 0.0; dst[7] = m.h;
#pragma unroll
    for (int j = 0; j < 4; ++j) { dst[8 + j] = a2[j]; dst[12 + j] = a3[j]; }
    dst[16] = 0.0; dst[17] = 0.0; dst[18] = b2; dst[19] = b3;
    dst[20] = uu.x; dst[21] = uu.y;
}

// k_mpc_box_lane_rollout and its fallback twin k_mpc_box_lane_rollout_fb: one text, two passes (as in mpc_box.hpp)
#define GYM_BOX_K(name) name
#define GYM_BOX_FB false
#define GYM_BOX_FB_PARAM
#define GYM_BOX_FB_ARG
#include "mpc_box_lanes_kernel.def.hpp"
#undef GYM_BOX_K
#undef GYM_BOX_FB
#undef GYM_BOX_FB_PARAM
#undef GYM_BOX_FB_ARG
#define GYM_BOX_K(name) name##_fb
#define GYM_BOX_FB true
#define GYM_BOX_FB_PARAM int fb_it,
#define GYM_BOX_FB_ARG , fb_it
#include "mpc_box_lanes_kernel.def.hpp"
#undef GYM_BOX_K
#undef GYM_BOX_FB
#undef GYM_BOX_FB_PARAM
#undef GYM_BOX_FB_ARG
