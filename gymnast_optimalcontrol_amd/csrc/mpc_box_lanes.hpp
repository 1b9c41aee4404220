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
// k_mpc_box_lane_rollout<true, int> is the instantiation with box_qp_lane's projected-Newton fallback (mpc_box.hpp).
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

// k_mpc_box_lane_rollout's optional parameters after max_it, the pack Ex = [int fb_it] [const gym_model* plant]: the
// fallback's iteration cap (0 without it: box_qp_lane's default, never read) and the plant's model (lane_plant)
__device__ __forceinline__ int box_ex_fb_it() { return 0; }
__device__ __forceinline__ int box_ex_fb_it(const gym_model*) { return 0; }
template <class... Pl> __device__ __forceinline__ int box_ex_fb_it(int fb_it, Pl...) { return fb_it; }
template <class... Pl>
__device__ __forceinline__ decltype(auto) box_ex_plant(const Dyn& m, int64_t row, bool valid, Pl... plant) {
    return lane_plant(m, row, valid, plant...);
}
template <class... Pl>
__device__ __forceinline__ decltype(auto) box_ex_plant(const Dyn& m, int64_t row, bool valid, int, Pl... plant) {
    return lane_plant(m, row, valid, plant...);
}

// x0 (B,P,4); lane-major x_opt (B,N,4), u_opt (B,N-1,2).  Outputs lane-major: xo (B,P,N,4), uo (B,P,N-1,2) (both or
// neither), summary (3,B,P) = err_final, err_max, u_max as k_lqr_lane_rollout, it_out (B,P,N-1) or null, unconv_out
// (B,P).  grid B nblk (nblk = ceil(P / 64)), 64 threads; LDS dynamic: (kBoxRow + 4) (L - 1) doubles.
// <false>: the active set alone; <true, int>: fb_it after max_it, handed to box_qp_lane's projected-Newton fallback
// (qp_iters then counts both phases, unconverged only the QPs that neither phase finished), as mpc_box.hpp's kernels.
// <FB, [int,] const gym_model*>: a mismatched plant, the (B,P) table last in the pack; closed loop (b, p) integrates
// its row b P + p (lane_plant, lqr_lanes.hpp).  The linearisation, the windows, the QP and m.h stay the
// design model's.
template <bool FB, class... Ex>
__global__ __launch_bounds__(64) void k_mpc_box_lane_rollout(Dyn m, M44 Q, double r, const double* __restrict__ QT,
                                                             double tau, int max_it, Ex... ex,
                                                             const double2* __restrict__ x_opt,
                                                             const double2* __restrict__ u_opt,
                                                             const double* __restrict__ x0, int P, int N, int L,
                                                             int nblk, double* wsd, int32_t* wst,
                                                             double* __restrict__ xo, double* __restrict__ uo,
                                                             double* __restrict__ summary,
                                                             int32_t* __restrict__ it_out,
                                                             int32_t* __restrict__ unconv_out) {
    extern __shared__ double bl_lds[];
    const int T = N - 1, Lm = L - 1;
    double* rows = bl_lds;
    double* kw = bl_lds + kBoxRow * Lm;
    const int ln = threadIdx.x;
    const int64_t b = blockIdx.x / nblk;
    const int p = (int)(blockIdx.x % nblk) * 64 + ln;
    const bool valid = p < P;
    const int64_t row = b * P + (valid ? p : 0);
    const int64_t BP = (int64_t)gridDim.x / nblk * P;
    decltype(auto) pm = box_ex_plant(m, row, valid, ex...);   // a block's padding threads (p >= P): the design model
    const double2* xlo = x_opt + 2 * (b * N);
    const double2* ulo = u_opt + b * T;
    const BoxWs ws{wsd + b * ((int64_t)kBoxSlots * Lm + 4) * P, wst + b * Lm * P, P, p};
    double2* xl = reinterpret_cast<double2*>(xo) + 2 * (int64_t)N * row;
    double2* ul = reinterpret_cast<double2*>(uo) + (int64_t)T * row;
    double n0 = x0[4 * row], n1 = x0[4 * row + 1], n2 = x0[4 * row + 2], n3 = x0[4 * row + 3];
    if (valid && xo) {
        xl[0] = make_double2(n0, n1);
        xl[1] = make_double2(n2, n3);
    }
    const Sym4 Qs = sym4(Q.v), QTs = sym4(QT);
    const gym::PolyRegs pk = gym::poly_vgprs();
    int unconv = 0;
    double emax = 0.0, umax = 0.0;
    BoxWin w{rows, kw, 0, Lm};
    for (int s = 0; s < T; ++s) {
        wave_lds_order();                               // the previous step's LDS reads are done
        if (s == 0) {
            for (int st = ln; st < Lm; st += 64) box_lane_row(m, xlo, ulo, st, T, true, rows + kBoxRow * st);
        } else {                                        // stage s + Lm - 1 replaces stage s - 1 in the ring
            box_lane_row(m, xlo, ulo, s + Lm - 1, T, ln == 0, rows + kBoxRow * w.base);
            w.base = w.base + 1 == Lm ? 0 : w.base + 1;
        }
        wave_lds_order();
        {                                               // Kw: the window's unconstrained gains (k_mpc_lane_gains' maps)
            Sym4 Pm = QTs;
            for (int t = Lm - 1; t >= 0; --t) {
                const double* A = w.row(t);
                double cur[ML_ROWS], k[4];
#pragma unroll
                for (int c = 0; c < 8; ++c) cur[c] = A[8 + c];
                cur[8] = A[18];
                cur[9] = A[19];
                lqr_lane_step(cur, cur + 4, cur[8], cur[9], m.h, r, Qs, Pm, k);
                if (ln == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) kw[4 * t + j] = k[j];
                }
            }
        }
        wave_lds_order();
        const double2 ra = xlo[2 * s], rb = xlo[2 * s + 1];
        const double d0 = n0 - ra.x, d1 = n1 - ra.y, d2 = n2 - rb.x, d3 = n3 - rb.y;
        const double* f = w.row(0) + 20;                // u_opt[s]
        double u1;
        int iters;
        bool conv;
        box_qp_lane<false, FB>(w, Lm, Q, r, QT, tau, max_it, ws, valid, d0, d1, d2, d3, u1, iters, conv,
                               box_ex_fb_it(ex...));
        if (valid) {
            const double v0 = box_apply(f[0], box_clip0(f[0], tau), tau), v1 = box_apply(f[1], u1, tau);
            emax = gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(emax, d0), d1), d2), d3);
            umax = gym::nanmax_abs(umax, v1);
            unconv += conv ? 0 : 1;
            gym::rk4(pm, n0, n1, n2, n3, v1, pk);
            if (it_out) it_out[(int64_t)T * row + s] = iters;
            if (xo) {
                ul[s] = make_double2(v0, v1);
                xl[2 * (s + 1)] = make_double2(n0, n1);
                xl[2 * (s + 1) + 1] = make_double2(n2, n3);
            }
        }
    }
    if (!valid) return;
    const double2 ra = xlo[2 * T], rb = xlo[2 * T + 1];
    const double d0 = n0 - ra.x, d1 = n1 - ra.y, d2 = n2 - rb.x, d3 = n3 - rb.y;
    const double efin = gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(0.0, d0), d1), d2), d3);
    emax = gym::nanmax_abs(emax, efin);
    summary[row] = efin;
    summary[BP + row] = emax;
    summary[2 * BP + row] = umax;
    unconv_out[row] = unconv;
}
