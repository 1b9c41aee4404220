// MI355X (gfx950) LQR / receding-horizon MPC trackers (trajectory_tracking.py), C-ABI part 2: the launch layer.
// The kernels live in the headers included below, one family each.
//
// The shared-reference trackers follow ONE reference trajectory that every lane shares (main.py task_3 / task_4), so
// their feedback gains are lane-independent:
//   * LQR (solve_LQR_tracking :170-203): one backward recursion along the reference (tracking_dense.hpp);
//   * MPC (solve_mpc_tracking :8-69 with solver_mpc :73-140): at control step t the QP over the window
//     [t, t + T_pred - 1] of the shifted reference (padded with (A_f, B_f)) has only equality constraints
//     (test_constraints = False, :87), so its exact solution is u_0 = K_0(t) x_0 with K_0(t) the first gain of
//     the window's finite-horizon LQ recursion.  All T windows are solved in parallel (mpc_gains.hpp); with the
//     torque limit every control step is a box-constrained QP per lane (mpc_box.hpp).
// The batched part is the closed-loop RK4 simulation of B perturbed initial states under the shared
// feed-forward / feedback sequence (simulate_tracking :206-216 and the MPC loop :43-60, track_rollout.hpp).
// Per-lane LQR tracking (every lane follows its OWN trajectory, so the gains are per-lane streams) is lqr_lanes.hpp;
// per-lane MPC tracking (every window of every lane has its own first gain) is mpc_lanes.hpp; with the torque limit
// (every lane's own QPs) it is mpc_box_lanes.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#ifndef GYM_HORNER_VOP3
#define GYM_HORNER_VOP3 1   // three-address Horner steps (acrobot_device.hpp): no per-step constant copies
#endif
#include "acrobot_device.hpp"
#include "gymnast_acrobot.h"
#include "gymnast_acrobot_models.h"

using gym::Dyn;

namespace {

// every header includes the project headers whose names it uses, so the order here is for the reader only
#include "tracking_dense.hpp"   // M44 / M22, the dense recursion, compute_P_inf as a fixed point, the LQ forward pass
#include "mpc_gains.hpp"        // fused MPC gains of the shared reference: every window's first (or every) gain
#include "track_rollout.hpp"    // closed-loop rollouts on the shared reference
#include "mpc_box.hpp"          // torque-limited MPC on the shared reference: the box QP and its closed loop
#include "lqr_lanes.hpp"   // per-lane LQR tracking: every lane follows its own trajectory
#include "mpc_lanes.hpp"   // per-lane MPC tracking: the first gain of every window of every lane
#include "mpc_box_lanes.hpp"   // per-lane torque-limited MPC tracking: each lane's QPs along its own trajectory

// ---- launch layer: each argument rule and each workspace carve is written once ----
inline M44 m44(const double* p) { M44 m; for (int i = 0; i < 16; ++i) m.v[i] = p[i]; return m; }
inline M22 m22(const double* p) { M22 m; for (int i = 0; i < 4; ++i) m.v[i] = p[i]; return m; }
inline int launch_status() { return (int)hipGetLastError(); }
template <class T> T* ws_at(void* ws, int64_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

inline bool finite_pos(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }      // not NaN, not inf
inline bool window_ok(int L) { return !(L < 2 || L + 2 > kMpcMaxStages); }               // k_mpc_gains' LDS table
inline bool batch_ok(int64_t B) { return B >= 1 && B <= ((int64_t)1 << 30); }             // shared-reference lanes
inline bool box_sizes_ok(int64_t B, int L, double tau_max, int max_qp_iters) {
    return batch_ok(B) && window_ok(L) && finite_pos(tau_max) && max_qp_iters >= 1;
}
// the channel split needs a diagonal R with r = R[1][1] > 0
inline bool box_weights_ok(const double* R) { return R[1] == 0.0 && R[2] == 0.0 && finite_pos(R[3]); }
inline bool lanes_sizes_ok(int64_t B, int32_t N) { return B >= 1 && N >= 2 && (B + 63) / 64 * 64 <= GYM_MAX_BP; }
inline bool box_lanes_sizes_ok(int64_t B, int32_t P, int32_t N, int32_t L) {
    return B >= 1 && P >= 1 && N >= 2 && window_ok(L) && B <= GYM_MAX_BP / P;
}
// a plant table: its 64-byte rows are read with 16-byte loads
inline bool plant_ok(const gym_model* plant) { return plant && reinterpret_cast<uintptr_t>(plant) % 16 == 0; }

template <bool ALL>   // K_out: every gain of every window (ALL) or each window's first gain
int mpc_gains_launch(const gym_model* m, const double* x_ref, const double* u_ref, int32_t S, const double* x_f,
                     const double* u_f, const double* Q, const double* R, int32_t L, int32_t nwin, int32_t max_iter,
                     double tol, double* K_out, double* QT_out, int32_t* iters_out, void* s) {
    if (!m || !x_ref || !u_ref || !x_f || !u_f || !Q || !R || !K_out || !QT_out || !iters_out || S <= 0 ||
        !window_ok(L) || nwin <= 0 || max_iter <= 0)
        return GYM_EINVAL;
    hipLaunchKernelGGL(k_mpc_gains<ALL>, dim3((unsigned)((nwin + 3) / 4)), dim3(64), 0, (hipStream_t)s, Dyn(*m),
                       x_ref, u_ref, S, x_f, u_f, m44(Q), m22(R), L, nwin, max_iter, tol, K_out, QT_out, iters_out);
    return launch_status();
}

// The box workspace (box_layout): the stage table, then the per-lane sweep doubles, then the stage states
struct BoxWsView {
    BoxLayout lo;
    double *A, *Bm, *ur, *d; int32_t* st;   // table A_d, B_d, u_ref; sweep doubles; stage states
};
inline BoxWsView box_ws(void* ws, int64_t B, int L, int64_t rows) {
    const BoxLayout lo = box_layout(B, L, rows);
    return {lo, ws_at<double>(ws, 0), ws_at<double>(ws, lo.off_B), ws_at<double>(ws, lo.off_ur),
            ws_at<double>(ws, lo.off_d), ws_at<int32_t>(ws, lo.off_st)};
}

// The per-lane LQR workspace (lanes_layout: x_opt pairs, u_opt planes, K1 pairs) with the tile grids of the kernels
// that fill and empty it.  ntx >= ntk >= ntu, so groups * ntx is the largest of the three grids.
struct LanesWs {
    LanesLayout lo;
    double2* xs; double* us; double2* ks;
    int64_t groups;             // 64-lane groups
    int T, ntx, ntu, ntk;       // stages; knot tiles per group: k_lqr_pack<4>, k_lqr_pack<2>, k_lqr_unpack_gains
};
inline LanesWs lanes_ws(void* ws, int64_t B, int N) {
    const LanesLayout lo = lanes_layout(B, N);
    const int T = N - 1;
    return {lo, ws_at<double2>(ws, 0), ws_at<double>(ws, lo.off_u), ws_at<double2>(ws, lo.off_k), lo.Bp / BLK, T,
            (N + 15) / 16, (T + 31) / 32, (T + 15) / 16};
}
// lane-major x_opt (B,N,4), u_opt (B,N-1,2) into the workspace
inline void lanes_pack(const LanesWs& w, const double* x_opt, const double* u_opt, int64_t B, hipStream_t st) {
    hipLaunchKernelGGL(k_lqr_pack<4>, dim3((unsigned)(w.groups * w.ntx)), dim3(LL_THREADS), 0, st,
                       reinterpret_cast<const double2*>(x_opt), reinterpret_cast<double*>(w.xs), B, w.lo.Bp, w.T + 1,
                       w.ntx);
    hipLaunchKernelGGL(k_lqr_pack<2>, dim3((unsigned)(w.groups * w.ntu)), dim3(LL_THREADS), 0, st,
                       reinterpret_cast<const double2*>(u_opt), w.us, B, w.lo.Bp, w.T, w.ntu);
}
// the workspace's K1 stream as lane-major full gains (B,N-1,2,4), if the caller wants them
inline void lanes_unpack_gains(const LanesWs& w, double* K_out, int64_t B, hipStream_t st) {
    if (K_out)
        hipLaunchKernelGGL(k_lqr_unpack_gains, dim3((unsigned)(w.groups * w.ntk)), dim3(LL_THREADS), 0, st, w.ks,
                           reinterpret_cast<double2*>(K_out), B, w.lo.Bp, w.T, w.ntk);
}

}  // namespace

extern "C" {

int gym_tv_lqr_gains(const double* A, const double* Bm, int32_t S, const double* A_pad, const double* B_pad,
                     const double Q[16], const double R[4], const double QT[16], int32_t L, int32_t nwin,
                     int32_t all_gains, int32_t discretize, double dt, double* K_out, void* s) {
    if (!A || !Bm || !Q || !R || !QT || !K_out || S <= 0 || L < 2 || nwin <= 0 || (all_gains && nwin != 1))
        return GYM_EINVAL;
    if ((nwin - 1) + (L - 2) >= S && (!A_pad || !B_pad)) return GYM_EINVAL;   // a window runs past the stages
    hipLaunchKernelGGL(k_tv_lqr_gains, dim3((nwin + 63) / 64), dim3(64), 0, (hipStream_t)s, A, Bm, S, A_pad, B_pad,
                       m44(Q), m22(R), QT, L, nwin, all_gains, discretize, dt, K_out);
    return launch_status();
}

int gym_dare_fixed_point(const double* A, const double* Bm, const double Q[16], const double R[4], int32_t max_iter,
                         double tol, double* P_out, int32_t* iters_out, void* s) {
    if (!A || !Bm || !Q || !R || !P_out || !iters_out || max_iter <= 0) return GYM_EINVAL;
    hipLaunchKernelGGL(k_dare_fixed_point, dim3(1), dim3(64), 0, (hipStream_t)s, A, Bm, m44(Q), m22(R), max_iter, tol,
                       P_out, iters_out);
    return launch_status();
}

int gym_mpc_gains(const gym_model* m, const double* x_ref, const double* u_ref, int32_t S, const double* x_f,
                  const double* u_f, const double Q[16], const double R[4], int32_t L, int32_t nwin, int32_t max_iter,
                  double tol, double* K_out, double* QT_out, int32_t* iters_out, void* s) {
    return mpc_gains_launch<false>(m, x_ref, u_ref, S, x_f, u_f, Q, R, L, nwin, max_iter, tol, K_out, QT_out,
                                   iters_out, s);
}

int gym_mpc_gains_all(const gym_model* m, const double* x_ref, const double* u_ref, int32_t S, const double* x_f,
                      const double* u_f, const double Q[16], const double R[4], int32_t L, int32_t nwin,
                      int32_t max_iter, double tol, double* K_all, double* QT_out, int32_t* iters_out, void* s) {
    return mpc_gains_launch<true>(m, x_ref, u_ref, S, x_f, u_f, Q, R, L, nwin, max_iter, tol, K_all, QT_out,
                                  iters_out, s);
}

int gym_mpc_box_workspace(int64_t B, int32_t L, int32_t rows, int64_t* bytes_out) {
    if (!bytes_out || !batch_ok(B) || !window_ok(L) || rows < 1) return GYM_EINVAL;
    *bytes_out = box_layout(B, L, rows).bytes;
    return 0;
}

// fallback_iters = 0: the active set alone, k_mpc_box_qp<false>; >= 1: with the projected-Newton fallback, <true, int>
static int box_qp_launch(const double* A, const double* Bm, const double* u_ref, int32_t S, const double Q[16],
                         const double R[4], const double* QT, const double* x0, int64_t B, int32_t L, double tau_max,
                         int32_t max_qp_iters, int32_t fallback_iters, void* ws, int64_t ws_bytes, double* U, double* X,
                         int32_t* iters_out, int32_t* converged_out, void* s) {
    if (!A || !Bm || !u_ref || !Q || !R || !QT || !x0 || !ws || !U || !X || !iters_out || !converged_out ||
        !box_sizes_ok(B, L, tau_max, max_qp_iters) || S < L - 1 || !box_weights_ok(R))
        return GYM_EINVAL;
    for (int64_t q = 0; q < 4 * (int64_t)S; ++q)
        if (Bm[2 * q] != 0.0) return GYM_EINVAL;       // the channel split needs B[:, 0] = 0 at every stage
    const BoxWsView w = box_ws(ws, B, L, S);
    if (ws_bytes < w.lo.bytes) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    hipError_t e = hipMemcpyAsync(w.A, A, 16 * sizeof(double) * S, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.Bm, Bm, 8 * sizeof(double) * S, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(w.ur, u_ref, 2 * sizeof(double) * S, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)(w.lo.Bp / 64));
    const BoxTable tb{w.A, w.Bm, w.ur, S - 1};
    if (fallback_iters)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mpc_box_qp<true, int>), grid, dim3(64), 0, st, tb, L, m44(Q), R[3], QT,
                           tau_max, max_qp_iters, fallback_iters, x0, B, w.d, w.st, w.lo.Bp, U, X, iters_out,
                           converged_out);
    else
        hipLaunchKernelGGL(k_mpc_box_qp<false>, grid, dim3(64), 0, st, tb, L, m44(Q), R[3], QT, tau_max, max_qp_iters,
                           x0, B, w.d, w.st, w.lo.Bp, U, X, iters_out, converged_out);
    return launch_status();
}

int gym_mpc_box_qp(const double* A, const double* Bm, const double* u_ref, int32_t S, const double Q[16],
                   const double R[4], const double* QT, const double* x0, int64_t B, int32_t L, double tau_max,
                   int32_t max_qp_iters, void* ws, int64_t ws_bytes, double* U, double* X, int32_t* iters_out,
                   int32_t* converged_out, void* s) {
    return box_qp_launch(A, Bm, u_ref, S, Q, R, QT, x0, B, L, tau_max, max_qp_iters, 0, ws, ws_bytes, U, X, iters_out,
                         converged_out, s);
}

int gym_mpc_box_qp_fallback(const double* A, const double* Bm, const double* u_ref, int32_t S, const double Q[16],
                            const double R[4], const double* QT, const double* x0, int64_t B, int32_t L,
                            double tau_max, int32_t max_qp_iters, int32_t fallback_iters, void* ws, int64_t ws_bytes,
                            double* U, double* X, int32_t* iters_out, int32_t* converged_out, void* s) {
    if (fallback_iters < 1) return GYM_EINVAL;
    return box_qp_launch(A, Bm, u_ref, S, Q, R, QT, x0, B, L, tau_max, max_qp_iters, fallback_iters, ws, ws_bytes, U,
                         X, iters_out, converged_out, s);
}

static int box_rollout_launch(const gym_model* m, const double* x0, const double* x_ref, const double* u_ref,
                              const double* x_f, const double* u_f, const double Q[16], const double R[4],
                              const double* QT, const double* K_all, int64_t B, int32_t N, int32_t L, double tau_max,
                              int32_t max_qp_iters, int32_t fallback_iters, void* ws, int64_t ws_bytes, double* x_out,
                              double* u_out, int32_t* qp_iters_out, int32_t* unconverged_out, void* s) {
    if (!m || !x0 || !x_ref || !u_ref || !x_f || !u_f || !Q || !R || !QT || !K_all || !ws || !x_out || !u_out ||
        !qp_iters_out || !unconverged_out || !box_sizes_ok(B, L, tau_max, max_qp_iters) || N < 2 ||
        !box_weights_ok(R))
        return GYM_EINVAL;
    const int S = N - 1;
    const BoxWsView w = box_ws(ws, B, L, S + 1);
    if (ws_bytes < w.lo.bytes) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(k_mpc_box_stages, dim3((unsigned)((S + 1 + 63) / 64)), dim3(64), 0, st, Dyn(*m), x_ref, u_ref,
                       S, x_f, u_f, w.A, w.Bm, w.ur);
    const dim3 grid((unsigned)(w.lo.Bp / 64));
    const BoxTable tb{w.A, w.Bm, w.ur, S};
    if (fallback_iters)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mpc_box_rollout<true, int>), grid, dim3(64), 0, st, Dyn(*m), tb, L,
                           m44(Q), R[3], QT, tau_max, max_qp_iters, fallback_iters, x0, x_ref, K_all, B, N, w.d, w.st,
                           w.lo.Bp, x_out, u_out, qp_iters_out, unconverged_out);
    else
        hipLaunchKernelGGL(k_mpc_box_rollout<false>, grid, dim3(64), 0, st, Dyn(*m), tb, L, m44(Q), R[3], QT, tau_max,
                           max_qp_iters, x0, x_ref, K_all, B, N, w.d, w.st, w.lo.Bp, x_out, u_out, qp_iters_out,
                           unconverged_out);
    return launch_status();
}

int gym_mpc_box_rollout(const gym_model* m, const double* x0, const double* x_ref, const double* u_ref,
                        const double* x_f, const double* u_f, const double Q[16], const double R[4], const double* QT,
                        const double* K_all, int64_t B, int32_t N, int32_t L, double tau_max, int32_t max_qp_iters,
                        void* ws, int64_t ws_bytes, double* x_out, double* u_out, int32_t* qp_iters_out,
                        int32_t* unconverged_out, void* s) {
    return box_rollout_launch(m, x0, x_ref, u_ref, x_f, u_f, Q, R, QT, K_all, B, N, L, tau_max, max_qp_iters, 0, ws,
                              ws_bytes, x_out, u_out, qp_iters_out, unconverged_out, s);
}

int gym_mpc_box_rollout_fallback(const gym_model* m, const double* x0, const double* x_ref, const double* u_ref,
                                 const double* x_f, const double* u_f, const double Q[16], const double R[4],
                                 const double* QT, const double* K_all, int64_t B, int32_t N, int32_t L,
                                 double tau_max, int32_t max_qp_iters, int32_t fallback_iters, void* ws,
                                 int64_t ws_bytes, double* x_out, double* u_out, int32_t* qp_iters_out,
                                 int32_t* unconverged_out, void* s) {
    if (fallback_iters < 1) return GYM_EINVAL;
    return box_rollout_launch(m, x0, x_ref, u_ref, x_f, u_f, Q, R, QT, K_all, B, N, L, tau_max, max_qp_iters,
                              fallback_iters, ws, ws_bytes, x_out, u_out, qp_iters_out, unconverged_out, s);
}

int gym_lq_forward(const double* A, const double* Bm, int32_t S, const double* A_pad, const double* B_pad,
                   int32_t discretize, double dt, const double* K, const double* x0, int32_t L, double* X, double* U,
                   void* s) {
    if (!A || !Bm || !K || !x0 || !X || !U || S <= 0 || L < 2) return GYM_EINVAL;
    if (L - 2 >= S && (!A_pad || !B_pad)) return GYM_EINVAL;
    hipLaunchKernelGGL(k_lq_forward, dim3(1), dim3(64), 0, (hipStream_t)s, A, Bm, S, A_pad, B_pad, discretize, dt, K,
                       x0, L, X, U);
    return launch_status();
}

int gym_track_rollout_ex(const gym_model* m, const double* x0, const double* x_ff, const double* u_ff,
                         const double* K, int64_t B, int32_t N, int32_t flags, double* x_out, double* u_out, void* s) {
    if (!m || !x0 || !x_ff || !u_ff || !K || !x_out || !u_out || !batch_ok(B) || N < 2 || (flags & ~GYM_TRACK_SINGLE))
        return GYM_EINVAL;
    const int64_t per = (flags & GYM_TRACK_SINGLE) ? 1 : 2;   // threads per trajectory: one lane, or a lane pair
    hipLaunchKernelGGL(per == 1 ? k_track_rollout : k_track_rollout_pair, dim3((unsigned)((per * B + 63) / 64)), dim3(64),
                       0, (hipStream_t)s, Dyn(*m), x0, x_ff, u_ff, K, B, N, x_out, u_out);
    return launch_status();
}

int gym_track_rollout(const gym_model* m, const double* x0, const double* x_ff, const double* u_ff, const double* K,
                      int64_t B, int32_t N, double* x_out, double* u_out, void* s) {
    return gym_track_rollout_ex(m, x0, x_ff, u_ff, K, B, N, 0, x_out, u_out, s);
}

// ---- per-lane LQR tracking (lqr_lanes.hpp) ----
int gym_lqr_lanes_workspace(int64_t B, int32_t N, int64_t* bytes_out) {
    if (!bytes_out || !lanes_sizes_ok(B, N)) return GYM_EINVAL;
    *bytes_out = lanes_layout(B, N).bytes;
    return 0;
}

// solve_LQR_tracking (trajectory_tracking.py:170-203) per lane; models: the (B) table of per-lane design models, or
// null for m on every lane
static int lanes_gains_launch(const gym_model* m, const gym_model* models, const double* x_opt, const double* u_opt,
                              int64_t B, int32_t N, const double Q[16], const double R[4], const double QT[16], void* ws,
                              int64_t ws_bytes, double* K_out, void* s) {
    if (!m || !x_opt || !u_opt || !Q || !R || !QT || !ws || !lanes_sizes_ok(B, N) || !box_weights_ok(R) ||
        !lanes_sym(Q) || !lanes_sym(QT))
        return GYM_EINVAL;
    const LanesWs w = lanes_ws(ws, B, N);
    if (ws_bytes < w.lo.bytes || w.groups * w.ntx > ((int64_t)1 << 31) - 1) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    lanes_pack(w, x_opt, u_opt, B, st);
    if (models)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lqr_lane_gains<const gym_model*, int64_t>), dim3((unsigned)w.groups),
                           dim3(BLK), 0, st, Dyn(*m), models, B, sym4(Q), sym4(QT), R[3], w.xs, w.us, w.ks, w.lo.Bp,
                           (int)N);
    else
        hipLaunchKernelGGL(k_lqr_lane_gains<>, dim3((unsigned)w.groups), dim3(BLK), 0, st, Dyn(*m), sym4(Q), sym4(QT),
                           R[3], w.xs, w.us, w.ks, w.lo.Bp, (int)N);
    lanes_unpack_gains(w, K_out, B, st);
    return launch_status();
}

int gym_lqr_lanes_gains(const gym_model* m, const double* x_opt, const double* u_opt, int64_t B, int32_t N,
                        const double Q[16], const double R[4], const double QT[16], void* ws, int64_t ws_bytes,
                        double* K_out, void* s) {
    return lanes_gains_launch(m, nullptr, x_opt, u_opt, B, N, Q, R, QT, ws, ws_bytes, K_out, s);
}

// the same with lane l linearised on models[l] (gymnast_acrobot_models.h)
int gym_lqr_lanes_gains_models(const gym_model* m, const gym_model* models, const double* x_opt, const double* u_opt,
                               int64_t B, int32_t N, const double Q[16], const double R[4], const double QT[16],
                               void* ws, int64_t ws_bytes, double* K_out, void* s) {
    if (!plant_ok(models)) return GYM_EINVAL;
    return lanes_gains_launch(m, models, x_opt, u_opt, B, N, Q, R, QT, ws, ws_bytes, K_out, s);
}

// simulate_tracking (trajectory_tracking.py:206-216) per lane and perturbed start; plant: the (B,P) table of the
// mismatched-plant kernels, or null for the design model itself
static int lanes_rollout_launch(const gym_model* m, const gym_model* plant, const double* x0, int64_t B, int32_t P,
                                int32_t N, const void* ws, int64_t ws_bytes, double* x_out, double* u_out,
                                double* summary_out, void* s) {
    if (!m || !x0 || !ws || !summary_out || !lanes_sizes_ok(B, N) || P < 1 || B > GYM_MAX_BP / P ||
        (x_out == nullptr) != (u_out == nullptr))
        return GYM_EINVAL;
    const LanesWs w = lanes_ws(const_cast<void*>(ws), B, N);   // read only: the kernels take it as const
    if (ws_bytes < w.lo.bytes) return GYM_EINVAL;
    const int64_t nb = w.groups * P;                       // <= 2^20 + 2^26 / 64: far below the grid limit
    const dim3 grid((unsigned)((nb + 7) / 8 * 8));
    if (plant)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(x_out ? k_lqr_lane_rollout<true, const gym_model*>
                                                 : k_lqr_lane_rollout<false, const gym_model*>),
                           grid, dim3(BLK), 0, (hipStream_t)s, Dyn(*m), plant, x0, w.xs, w.us, w.ks, B, w.lo.Bp, (int)P,
                           (int)N, x_out, u_out, summary_out);
    else
        hipLaunchKernelGGL(x_out ? k_lqr_lane_rollout<true> : k_lqr_lane_rollout<false>, grid, dim3(BLK), 0,
                           (hipStream_t)s, Dyn(*m), x0, w.xs, w.us, w.ks, B, w.lo.Bp, (int)P, (int)N, x_out, u_out,
                           summary_out);
    return launch_status();
}

int gym_lqr_lanes_rollout(const gym_model* m, const double* x0, int64_t B, int32_t P, int32_t N, const void* ws,
                          int64_t ws_bytes, double* x_out, double* u_out, double* summary_out, void* s) {
    return lanes_rollout_launch(m, nullptr, x0, B, P, N, ws, ws_bytes, x_out, u_out, summary_out, s);
}

// simulate_tracking (:206-216) with the plant step of closed loop (b, p) on plant[b][p] (dynamics.py:15-61)
int gym_lqr_lanes_rollout_plant(const gym_model* m, const gym_model* plant, const double* x0, int64_t B, int32_t P,
                                int32_t N, const void* ws, int64_t ws_bytes, double* x_out, double* u_out,
                                double* summary_out, void* s) {
    if (!plant_ok(plant)) return GYM_EINVAL;
    return lanes_rollout_launch(m, plant, x0, B, P, N, ws, ws_bytes, x_out, u_out, summary_out, s);
}

// ---- per-lane MPC tracking (mpc_lanes.hpp) ----
// solve_mpc_tracking's gains (trajectory_tracking.py:8-69) per lane: fills a gym_lqr_lanes_rollout workspace
int gym_mpc_lanes_gains(const gym_model* m, const double* x_opt, const double* u_opt, int64_t B, int32_t N, int32_t L,
                        const double Q[16], const double R[4], const double* QT_dev, void* ws, int64_t ws_bytes,
                        double* K_out, void* s) {
    if (!m || !x_opt || !u_opt || !Q || !R || !QT_dev || !ws || !lanes_sizes_ok(B, N) || !window_ok(L) ||
        !box_weights_ok(R) || !lanes_sym(Q))
        return GYM_EINVAL;
    const LanesWs w = lanes_ws(ws, B, N);
    const int64_t nwork = w.lo.Bp * ((w.T + ML_W - 1) / ML_W);   // (lane, window block) workgroups
    const int64_t gmax = ((int64_t)1 << 31) - 8;                 // the gains grid is rounded up to a multiple of 8
    if (ws_bytes < w.lo.bytes || w.groups * w.ntx > gmax || nwork > gmax) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    lanes_pack(w, x_opt, u_opt, B, st);
    const size_t lds = sizeof(double) * ML_ROWS * (ML_W + L - 2);
    hipLaunchKernelGGL(k_mpc_lane_gains<ML_W>, dim3((unsigned)((nwork + 7) / 8 * 8)), dim3(ML_W), lds, st, Dyn(*m),
                       sym4(Q), QT_dev, R[3], reinterpret_cast<const double2*>(x_opt),
                       reinterpret_cast<const double2*>(u_opt), w.ks, B, w.lo.Bp, (int)N, (int)L, nwork);
    lanes_unpack_gains(w, K_out, B, st);
    return launch_status();
}

// ---- per-lane torque-limited MPC tracking (mpc_box_lanes.hpp) ----
int gym_mpc_box_lanes_workspace(int64_t B, int32_t P, int32_t L, int64_t* bytes_out) {
    if (!bytes_out || !box_lanes_sizes_ok(B, P, 2, L)) return GYM_EINVAL;
    *bytes_out = box_lanes_layout(B, P, L).bytes;
    return 0;
}

// solve_mpc_tracking's closed loop (trajectory_tracking.py:43-67) with solver_mpc's test_constraints (:87-114) per lane
// plant: the (B,P) table of the mismatched-plant kernels, or null for the design model itself
static int box_lanes_launch(const gym_model* m, const gym_model* plant, const double* x_opt, const double* u_opt,
                            const double* x0, int64_t B, int32_t P, int32_t N, int32_t L, const double Q[16],
                            const double R[4], const double* QT_dev, double tau_max, int32_t max_qp_iters,
                            int32_t fallback_iters, void* ws, int64_t ws_bytes, double* x_out, double* u_out,
                            double* summary_out, int32_t* qp_iters_out, int32_t* unconverged_out, void* s) {
    if (!m || !x_opt || !u_opt || !x0 || !Q || !R || !QT_dev || !ws || !summary_out || !unconverged_out ||
        !box_lanes_sizes_ok(B, P, N, L) || !finite_pos(tau_max) || max_qp_iters < 1 || !box_weights_ok(R) ||
        !lanes_sym(Q) || (x_out == nullptr) != (u_out == nullptr))
        return GYM_EINVAL;
    const BoxLanesLayout lo = box_lanes_layout(B, P, L);
    if (ws_bytes < lo.bytes) return GYM_EINVAL;
    const int nblk = (P + 63) / 64;                        // B nblk <= B P <= GYM_MAX_BP: far below the grid limit
    const size_t lds = sizeof(double) * (kBoxRow + 4) * (L - 1);
    const dim3 grid((unsigned)(B * nblk));
    const double2 *xo2 = reinterpret_cast<const double2*>(x_opt), *uo2 = reinterpret_cast<const double2*>(u_opt);
    if (plant && fallback_iters)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mpc_box_lane_rollout<true, int, const gym_model*>), grid, dim3(64), lds,
                           (hipStream_t)s, Dyn(*m), m44(Q), R[3], QT_dev, tau_max, max_qp_iters, fallback_iters, plant,
                           xo2, uo2, x0, (int)P, (int)N, (int)L, nblk, ws_at<double>(ws, 0),
                           ws_at<int32_t>(ws, lo.off_st), x_out, u_out, summary_out, qp_iters_out, unconverged_out);
    else if (plant)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mpc_box_lane_rollout<false, const gym_model*>), grid, dim3(64), lds,
                           (hipStream_t)s, Dyn(*m), m44(Q), R[3], QT_dev, tau_max, max_qp_iters, plant, xo2, uo2, x0,
                           (int)P, (int)N, (int)L, nblk, ws_at<double>(ws, 0), ws_at<int32_t>(ws, lo.off_st), x_out,
                           u_out, summary_out, qp_iters_out, unconverged_out);
    else if (fallback_iters)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mpc_box_lane_rollout<true, int>), grid, dim3(64), lds, (hipStream_t)s,
                           Dyn(*m), m44(Q), R[3], QT_dev, tau_max, max_qp_iters, fallback_iters, xo2, uo2, x0, (int)P,
                           (int)N, (int)L, nblk, ws_at<double>(ws, 0), ws_at<int32_t>(ws, lo.off_st), x_out, u_out,
                           summary_out, qp_iters_out, unconverged_out);
    else
        hipLaunchKernelGGL(k_mpc_box_lane_rollout<false>, grid, dim3(64), lds, (hipStream_t)s, Dyn(*m), m44(Q), R[3],
                           QT_dev, tau_max, max_qp_iters, xo2, uo2, x0, (int)P, (int)N, (int)L, nblk,
                           ws_at<double>(ws, 0), ws_at<int32_t>(ws, lo.off_st), x_out, u_out, summary_out,
                           qp_iters_out, unconverged_out);
    return launch_status();
}

int gym_mpc_box_lanes_rollout(const gym_model* m, const double* x_opt, const double* u_opt, const double* x0, int64_t B,
                              int32_t P, int32_t N, int32_t L, const double Q[16], const double R[4],
                              const double* QT_dev, double tau_max, int32_t max_qp_iters, void* ws, int64_t ws_bytes,
                              double* x_out, double* u_out, double* summary_out, int32_t* qp_iters_out,
                              int32_t* unconverged_out, void* s) {
    return box_lanes_launch(m, nullptr, x_opt, u_opt, x0, B, P, N, L, Q, R, QT_dev, tau_max, max_qp_iters, 0, ws,
                            ws_bytes, x_out, u_out, summary_out, qp_iters_out, unconverged_out, s);
}

int gym_mpc_box_lanes_rollout_fallback(const gym_model* m, const double* x_opt, const double* u_opt, const double* x0,
                                       int64_t B, int32_t P, int32_t N, int32_t L, const double Q[16],
                                       const double R[4], const double* QT_dev, double tau_max, int32_t max_qp_iters,
                                       int32_t fallback_iters, void* ws, int64_t ws_bytes, double* x_out,
                                       double* u_out, double* summary_out, int32_t* qp_iters_out,
                                       int32_t* unconverged_out, void* s) {
    if (fallback_iters < 1) return GYM_EINVAL;
    return box_lanes_launch(m, nullptr, x_opt, u_opt, x0, B, P, N, L, Q, R, QT_dev, tau_max, max_qp_iters,
                            fallback_iters, ws, ws_bytes, x_out, u_out, summary_out, qp_iters_out, unconverged_out, s);
}

// the closed loop (trajectory_tracking.py:43-67) with the plant step of (b, p) on plant[b][p] (dynamics.py:15-61);
// fallback_iters = 0: the active set alone
int gym_mpc_box_lanes_rollout_plant(const gym_model* m, const gym_model* plant, const double* x_opt,
                                    const double* u_opt, const double* x0, int64_t B, int32_t P, int32_t N, int32_t L,
                                    const double Q[16], const double R[4], const double* QT_dev, double tau_max,
                                    int32_t max_qp_iters, int32_t fallback_iters, void* ws, int64_t ws_bytes,
                                    double* x_out, double* u_out, double* summary_out, int32_t* qp_iters_out,
                                    int32_t* unconverged_out, void* s) {
    if (!plant_ok(plant) || fallback_iters < 0) return GYM_EINVAL;
    return box_lanes_launch(m, plant, x_opt, u_opt, x0, B, P, N, L, Q, R, QT_dev, tau_max, max_qp_iters,
                            fallback_iters, ws, ws_bytes, x_out, u_out, summary_out, qp_iters_out, unconverged_out, s);
}

}  // extern "C"
