// Per-lane MPC tracking: every lane tracks its OWN trajectory with the receding-horizon MPC of
// trajectory_tracking.py:8-69 (main.py: task_2's result fed to task_4, per lane).  Part of the tracking_kernels.hip
// translation unit (included inside its anonymous namespace).
//
// Without a torque limit the QP of control step t is solved exactly by the first gain of window t's finite-horizon
// recursion (mpc_gains.hpp, "Fused MPC gains"): stages t .. t+L-2 of the lane's own linearisation, the pad
// (A_f, B_f) at x_f = (pi, 0, 0, 0), u_f = 0 past stage S = N-1, from P = Q_T = compute_P_inf on the pad.  The pad and
// Q_T do not depend on the lane; the stages do.  The closed loop u_t = u_opt_t + K0_t (x_t - x_opt_t) is exactly
// k_lqr_lane_rollout on a K1 stream, so only the gains are new: this file fills lqr_lanes.hpp's workspace.
//
// Unlike the streaming per-lane kernels this one is arithmetic: a lane reads its 24 KB once and runs T windows x (L-1)
// Riccati maps (37,000 maps at N = 501, L = 75).  A workgroup owns one lane and ML_W consecutive windows, one window
// per thread (B T windows in all: no need for k_mpc_gains' 16-lanes-per-map layout, which exists because that kernel
// has T windows in total).  It first linearises the ML_W + L - 2 stages its windows touch, one stage per thread, from
// the lane-major x_opt (B,N,4) / u_opt (B,N-1,2) (consecutive stages of one lane are contiguous there), into LDS as
// [component][stage]: thread w reading stage w + s is a run of consecutive doubles, conflict-free.  Rows at or past S
// hold the pad's values, so the window loop has no branch.  Each thread then runs its L-1 dependent maps
// (lqr_lane_step, P in 10 registers) and keeps the last k.  Row 0 of every gain is exactly zero (lqr_lanes.hpp).
#pragma once

#include "lqr_lanes.hpp"   // Sym4, lqr_lane_stage, lqr_lane_step, wix

constexpr int ML_W = 256;            // windows (threads) per workgroup: 64 and 128 were 4.6 % and 3.4 % slower
constexpr int ML_ROWS = 10;          // doubles per stage: a2[4], a3[4], b2, b3

// First gain of every window of every lane, written straight into the K1 stream (T, Bp/64, 2, 64) double2 with one
// 16-byte store per pair: a coalesced lane-major (B, T, 4) intermediate followed by k_lqr_pack<4> was 2.9 - 3.5 %
// slower at every block size and needs 32 T B more workspace bytes.  Workgroups are dealt to the XCDs as
// k_lqr_lane_rollout's (round-robin over 8; gridDim.x is a multiple of 8): one XCD runs consecutive lanes of the same
// window block back to back, so the stores of 8 neighbouring lanes to one 128-byte line of a K1 row meet in that
// XCD's L2.  The grid covers Bp lanes; padding lanes (>= B) store zeros, which the rollout runs on.
// LDS: ML_ROWS (W + L - 2) doubles, dynamic (at most 40,640 B: L + 2 <= kMpcMaxStages, k_mpc_gains' bound, which the
// entry point enforces).  nwork = Bp ceil(T / W) workgroups do work.
template <int W>
__global__ __launch_bounds__(W) void k_mpc_lane_gains(Dyn m, Sym4 Q, const double* __restrict__ QT, double r11,
                                                      const double2* __restrict__ x_opt,
                                                      const double2* __restrict__ u_opt, double2* __restrict__ kout,
                                                      int64_t B, int64_t Bp, int N, int L, int64_t nwork) {
#pragma clang fp contract(on)
    extern __shared__ double ml_tab[];
    const int64_t per = gridDim.x / 8;
    const int64_t bi = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;
    if (bi >= nwork) return;
    const int64_t blk = bi / Bp;
    const int64_t b = bi - blk * Bp;
    const int T = N - 1;
    const int w = threadIdx.x, t0 = (int)blk * W, t = t0 + w;
    if (b >= B) {                                          // a padding lane: finite (zero) gains for the rollout
        if (t < T) {
            kout[wix(t, 0, 2, b, Bp)] = make_double2(0.0, 0.0);
            kout[wix(t, 1, 2, b, Bp)] = make_double2(0.0, 0.0);
        }
        return;
    }
    const int nst = W + L - 2;                              // stages t0 .. t0 + W - 1 + L - 2
    const double2* xl = x_opt + 2 * (b * N);
    const double2* ul = u_opt + b * T;
    for (int s = w; s < nst; s += W) {
        const int gs = t0 + s;
        const bool own = gs < T;                            // the lane's own stage; else the pad (x_f, u_f)
        const int gi = own ? gs : 0;
        double2 xa = xl[2 * gi], xb = xl[2 * gi + 1];
        double tau = ul[gi].y;
        xa = own ? xa : make_double2(3.14159265358979323846, 0.0);
        xb = own ? xb : make_double2(0.0, 0.0);
        tau = own ? tau : 0.0;
        double a2[4], a3[4], b2, b3;
        lqr_lane_stage(m, xa, xb, tau, a2, a3, b2, b3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ml_tab[j * nst + s] = a2[j];
            ml_tab[(4 + j) * nst + s] = a3[j];
        }
        ml_tab[8 * nst + s] = b2;
        ml_tab[9 * nst + s] = b3;
    }
    __syncthreads();
    if (t >= T) return;
    Sym4 P = sym4(QT);
    const double* row = ml_tab + w;                         // stage s of this window: row[c nst + s]
    double k[4];
    for (int s = L - 2; s >= 0; --s) {                      // the workgroup's other wavefronts cover the LDS latency:
        double cur[ML_ROWS];                                // reading a step ahead cost 9 register copies per step
#pragma unroll
        for (int c = 0; c < ML_ROWS; ++c) cur[c] = row[c * nst + s];
        lqr_lane_step(cur, cur + 4, cur[8], cur[9], m.h, r11, Q, P, k);
    }
    kout[wix(t, 0, 2, b, Bp)] = make_double2(k[0], k[1]);
    kout[wix(t, 1, 2, b, Bp)] = make_double2(k[2], k[3]);
}
