// MI355X (gfx950) kernels + C-ABI of the batched acrobot Newton/Armijo engine.
//
// One trajectory ("lane") per GPU thread, 64-thread workgroups (one wavefront), time-major SoA
// streams with the lane innermost.  States and gains are stored as 16-byte pairs (one 1 KiB
// transaction per wavefront load), controls and sigma as 8-byte planes.  The shared references
// x_ref (N,4), u_ref (T,2) are read with wave-uniform addresses (scalar loads).  The whole
// per-lane recursion (Jacobians, Riccati state P/p, RK4 state, running cost) is register-resident;
// no LDS is needed because lanes never exchange data.
//
// The solver's two HBM streams per Newton iteration:
//   backward sweep : read x (2 pairs) + u (2 planes), write K row 1 (2 pairs) + cg (1 plane)
//   Armijo trial   : read K row 1 + cg + u0, write x_new (2 pairs) + u_new (2 planes)
// where cg = (u1 - K1 x) + gamma0 sigma1 folds the reference's u1 + K1 (x_new - x) + gamma0 sigma1 into
// cg + K1 x_new, so the first trial never re-reads the old trajectory x nor sigma1; sigma0 = -r0 / (2R0) is
// recomputed from u0 bit-identically.  sigma1 itself is not streamed: the rare consumers (trials 2..20 of
// lanes that backtrack, the final sigma output, gamma sweeps) re-run the lane's sweep, which reproduces it
// bit for bit, into the sigma1 plane.  Streamed once per pass, these use non-temporal loads/stores.
//
// Reference: the original project's trajectory_generation.py (newton_Algorithm :298-398 and the
// primitives it calls) and dynamics.py.  See include/gymnast_acrobot.h for the ABI.
//
// One translation unit; the device code lives in headers included below, inside the anonymous namespace and in
// dependency order:
//   newton_streams.hpp   kernel-argument constants (Dyn / KW, kw()), load / store wrappers, index helpers
//   newton_stages.hpp    per-lane building blocks: stage cost, rollouts, trial controls, the backward sweeps
//   newton_lockstep.hpp  serial and pipelined-phase kernels, post-trial Armijo search
//   newton_run.hpp       the persistent kernels k_nt_run / k_nt_run2
//   newton_limited.hpp   the torque-limited persistent solve, once for its variants: k_nt_run_limited and the sigma1
//                        re-run k_nt_sigma_limited
//   newton_box.hpp       its plain variant (BoxVariant)
//   newton_mpc.hpp       closed-loop replanning on that loop body: k_nt_mpc_run
//   newton_models.hpp    its variant on per-lane models (ModelsVariant)
//   newton_weights.hpp   its variant on per-lane cost weights (WeightsVariant)
//   rk4_lin.hpp          the RK4-exact linearisation: its variant (Rk4Variant), and k_linearize_rk4
//   newton_tail.hpp      the straggler tail k_nt_tail
//   newton_util.hpp      API / point kernels, pack / unpack / gather, init, placement probe
// This file keeps the batch-wide auxiliary kernels (gamma sweeps, statistics, sigma1 re-run, finalize, fill-states),
// the launch helpers and the extern "C" entry points.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "acrobot_device.hpp"
#include "gymnast_acrobot.h"
#include "gymnast_acrobot_box.h"
#include "gymnast_acrobot_rk4lin.h"
#include "gymnast_acrobot_models.h"
#include "gymnast_newton_weights.h"
#include "gymnast/newton_mpc.h"

using gym::Dyn;

namespace {

#include "newton_streams.hpp"
#include "newton_stages.hpp"
#include "newton_lockstep.hpp"
#include "newton_run.hpp"
#include "newton_limited.hpp"
#include "newton_box.hpp"
#include "newton_mpc.hpp"
#include "newton_models.hpp"
#include "newton_weights.hpp"
#include "rk4_lin.hpp"
#include "newton_tail.hpp"
#include "newton_util.hpp"

inline int grid_for(int64_t n, int block, int64_t cap = (int64_t)1 << 30) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// ------------------------------------------------------------------------------------------
// Armijo gamma sweeps (plot_armijo_line_search :254-265): J(gamma_g) of the candidate rollout for G step
// sizes per lane, cost only, one thread per (lane, g).  The G blocks of one lane group re-read the same
// streams, so a group's blocks are mapped onto one XCD (blocks are dealt round-robin over the 8 XCDs) and
// run back to back there: the re-reads hit that XCD's L2.  gridDim.x is a multiple of 8.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sweep_block(int G, int64_t groups, int64_t& grp, int& g) {
    const int64_t per = gridDim.x / 8;
    const int64_t i = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;
    grp = i / G;
    g = (int)(i % G);
    return grp < groups;
}

// reference form: full gains Kf (T,4,Bp), sigma planes, u_new = u + K (x_new - x) + gamma sigma
__global__ __launch_bounds__(BLK) void k_gamma_sweep(Dyn m, KW w, const double2* __restrict__ x,
                                                     const double* __restrict__ u, const double2* __restrict__ Kf,
                                                     const double* __restrict__ sig, const double* __restrict__ gammas,
                                                     int G, const double* __restrict__ xr,
                                                     const double* __restrict__ ur, double* __restrict__ cost_out,
                                                     int64_t B, int64_t Bp, int N) {
    int64_t grp;
    int g;
    if (!sweep_block(G, Bp / BLK, grp, g)) return;
    const int64_t l = grp * BLK + threadIdx.x;
    if (l >= B) {
        cost_out[(int64_t)g * Bp + l] = __builtin_nan("");
        return;
    }
    const double2 a = x[wix(0, 0, 2, l, Bp)], b = x[wix(0, 1, 2, l, Bp)];
    cost_out[(int64_t)g * Bp + l] = rollout_ref<true, false>(m, w, x, u, Kf, sig, xr, ur, nullptr, nullptr, gammas[g],
                                                             l, Bp, N, a.x, a.y, b.x, b.y);
}

// solver form: the Armijo trial's own rollout (offset form) on a batch's iteration-k streams; at the
// trial's step sizes the costs are bit-identical to the trial's.  Non-active lanes get NaN.
template <bool U0Z, bool RL>
__global__ __launch_bounds__(BLK) void k_nt_gamma_sweep(Dyn m, KW w, const double2* __restrict__ x,
                                                        const double* __restrict__ u, const double2* __restrict__ K1,
                                                        const double* __restrict__ cs, double g0,
                                                        const double* __restrict__ gammas, int G,
                                                        const double* __restrict__ xr, const double* __restrict__ ur,
                                                        const int32_t* __restrict__ status,
                                                        double* __restrict__ cost_out, int64_t B, int64_t Bp, int N) {
    int64_t grp;
    int g;
    if (!sweep_block(G, Bp / BLK, grp, g)) return;
    const int64_t l = grp * BLK + threadIdx.x;
    if (l >= B || status[l] != GYM_ACTIVE) {
        cost_out[(int64_t)g * Bp + l] = __builtin_nan("");
        return;
    }
    const double2 a = x[wix(0, 0, 2, l, Bp)], b = x[wix(0, 1, 2, l, Bp)];
    cost_out[(int64_t)g * Bp + l] = rollout_cform<false, U0Z, true, false, 0>(
        m, w, u, K1, cs, lane_ref<RL>(xr, l, 4 * (int64_t)N), lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), nullptr,
        nullptr, gammas[g], g0, l, Bp, N, a.x, a.y, b.x, b.y);
}

// Deterministic two-stage statistics reduction (fixed lane->thread map, fixed trees).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(STAT_THREADS) void k_stats_partial(const int32_t* __restrict__ status,
                                                                const double* __restrict__ cost,
                                                                const double* __restrict__ smax,
                                                                const int32_t* __restrict__ n_iter,
                                                                const int32_t* __restrict__ n_roll,
                                                                double* __restrict__ partials, Range rg, int k) {
    __shared__ double red[STAT_THREADS / 64][NSTAT];
    double acc[NSTAT] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t n = rg.hi - rg.lo;
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t lo = rg.lo + (int64_t)blockIdx.x * chunk;
    const int64_t hi = (lo + chunk < rg.hi) ? lo + chunk : rg.hi;
    for (int64_t l = lo + threadIdx.x; l < hi; l += STAT_THREADS) {
        const int st = status[l];
        const bool ran = n_iter[l] == k + 1;
        acc[0] += (st == GYM_ACTIVE) ? 1.0 : 0.0;
        acc[1] += cost[l];
        acc[2] += ran ? smax[l] * smax[l] : 0.0;
        acc[3] += ran ? 1.0 : 0.0;
        acc[5] += (st == GYM_CONVERGED) ? 1.0 : 0.0;
        acc[6] += (st == GYM_LS_FAILED) ? 1.0 : 0.0;
        acc[7] += (double)n_roll[l];
    }
    const int wv = threadIdx.x / 64, ln = threadIdx.x % 64;
#pragma unroll
    for (int s = 0; s < NSTAT; ++s) {
        const double v = wave_sum(acc[s]);
        if (ln == 0) red[wv][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSTAT) {
        double v = 0.0;
        for (int q = 0; q < STAT_THREADS / 64; ++q) v += red[q][threadIdx.x];
        partials[(int64_t)blockIdx.x * NSTAT + threadIdx.x] = v;
    }
}

// stats_out[0..7] = this range's statistics; if other != NULL, total[s] = other[s] + stats_out[s].
// One wavefront per statistic: lane i adds partials i, i+64, ... in order, then a fixed shuffle tree.
__global__ __launch_bounds__(64 * NSTAT) void k_stats_final(const double* __restrict__ partials,
                                                            int32_t* __restrict__ counter,
                                                            double* __restrict__ stats_out,
                                                            const double* __restrict__ other,
                                                            double* __restrict__ total, int nblocks) {
    const int s = threadIdx.x / 64, ln = threadIdx.x % 64;
    double v = 0.0;
    for (int b = ln; b < nblocks; b += 64) v += partials[(int64_t)b * NSTAT + s];
    v = wave_sum(v);
    if (ln == 0) {
        if (s == 4) v = (double)(*counter);
        stats_out[s] = v;
        if (other) total[s] = other[s] + v;
    }
    __syncthreads();
    if (threadIdx.x == 0) *counter = 0;  // the retry list is rebuilt every iteration
}

// sigma1 re-run: the sweep of an earlier pass, recomputed (same inputs, same code: the same bits) into the
// sigma1 plane.  retry mode (list != nullptr): the lanes list[0 .. *count) at the iterate (x, u); final mode:
// the lanes whose last iteration started from this buffer, (n_iter - 1) & 1 == parity (one launch per
// buffer, so the streams' base addresses stay wave-uniform).
template <bool U0Z, bool CK, bool RL = false>
__global__ __launch_bounds__(BLK, 4) void k_nt_sigma(Dyn m, KW w, const double2* __restrict__ x,
                                                     const double* __restrict__ u, const double* __restrict__ xr,
                                                     const double* __restrict__ ur, double* __restrict__ cs,
                                                     const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                     const int32_t* __restrict__ n_iter, int parity, int64_t B,
                                                     int64_t Bp, int N) {
    GYM_CK_LDS(CK, U0Z);
    const int64_t n = list ? (int64_t)*count : B;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLK) {
        const int64_t l = list ? (int64_t)list[i] : i;
        if (!list) {
            const int it = n_iter[l];
            if (it <= 0 || ((it - 1) & 1) != parity) continue;
        }
        backward_solver<U0Z, CK, OUT_SIGMA>(m, w, x, u, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                            lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), nullptr, cs, 0.0, nullptr,
                                            nullptr, nullptr, l, Bp, N, 0, 0, ck_lds);
    }
}

__global__ void k_finalize_status(int32_t* __restrict__ status, int32_t* __restrict__ res_buf, int64_t B, int k_done) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= B) return;
    if (status[l] == GYM_ACTIVE) {
        status[l] = GYM_MAX_ITERS;
        res_buf[l] = k_done & 1;
    }
}


// GYM_FLAG_X_CKPT: rebuild every knot of a state buffer from x_0 and the tau2 controls, x_{t+1} =
// RK4(x_t, u1_t) -- the same recursion (and code) the trial ran, so the rebuilt knots equal the bits it
// would have stored and the checkpoints are rewritten unchanged.  sel_buf < 0: lane l's res_buf.
__global__ __launch_bounds__(BLK) void k_fill_states(Dyn m, double2* __restrict__ x0b, double2* __restrict__ x1b,
                                                     const double* __restrict__ u0b, const double* __restrict__ u1b,
                                                     const int32_t* __restrict__ res_buf, int sel_buf, int64_t B,
                                                     int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const int sel = sel_buf >= 0 ? sel_buf : res_buf[l];
    double2* xs = sel ? x1b : x0b;
    const double* us = sel ? u1b : u0b;
    const double2 a = xs[wix(0, 0, 2, l, Bp)], b = xs[wix(0, 1, 2, l, Bp)];
    double n0 = a.x, n1 = a.y, n2 = b.x, n3 = b.y;
    for (int t = 0; t < N - 1; ++t) {
        gym::rk4(m, n0, n1, n2, n3, us[pix(t, 1, 2, l, Bp)]);
        st_nt(xs + wix(t + 1, 0, 2, l, Bp), n0, n1);
        st_nt(xs + wix(t + 1, 1, 2, l, Bp), n2, n3);
    }
}

// The kinds timed at every launch (pool pairs): the solver's main kernels (sweep, trial, phase, run, tail), whose
// average duration is the roofline's denominator.  The short post-trial kernels (candidates, retry, statistics,
// sigma1 re-run: five per phase) keep one sampled pair per kind and collect: an event pair around each of them
// lengthened the phase-to-phase gap from ~28 to ~73 us in the rocprofv3 trace (+1-2% per solve).
constexpr int TIMING_POOL_KINDS = (1 << 0) | (1 << 1) | (1 << 5) | (1 << 6) | (1 << 8) | (1 << 9);
struct TimedLaunch {  // records a start/stop event pair around one launch: a pool pair, else the kind's free slot
    gym_timing* t;
    int kind;
    hipStream_t s;
    int slot;            // pool index, -1: the kind's sampled pair, -2: not timed
    TimedLaunch(gym_timing* t_, int kind_, hipStream_t s_) : t(t_), kind(kind_), s(s_), slot(-2) {
        if (!t) return;
        if (((TIMING_POOL_KINDS >> kind) & 1) && t->pool_used < GYM_TIMING_POOL && t->pool_ev[0]) {
            slot = t->pool_used++;
            t->pool_kind[slot] = kind;
            (void)hipEventRecord((hipEvent_t)t->pool_ev[2 * slot], s);
        } else if (!(t->pending & (1 << kind))) {
            slot = -1;
            (void)hipEventRecord((hipEvent_t)t->ev[2 * kind], s);
        }
    }
    ~TimedLaunch() {
        if (slot >= 0) {
            (void)hipEventRecord((hipEvent_t)t->pool_ev[2 * slot + 1], s);
        } else if (slot == -1) {
            (void)hipEventRecord((hipEvent_t)t->ev[2 * kind + 1], s);
            t->pending |= 1 << kind;
        }
    }
};

// Kernel-variant selection.  The batch flags reach a generic lambda as compile-time booleans (U0Z:
// GYM_FLAG_U0_ZERO, CK: GYM_FLAG_X_CKPT, RL: GYM_FLAG_REF_LANE), and the lambda names the instantiation:
//     with_variant(b, [](auto U0Z, auto CK, auto RL) { return k_nt_trial<U0Z(), CK(), RL()>; })
// Every launch selects through here, so the two rules on which instantiations exist are stated once:
//   * X_CKPT and REF_LANE never combine (bad_batch rejects the pair): per-lane references win, no <CK, RL> kernel;
//   * an extra boolean that excludes checkpointing (k_nt_phase's LO) is false whenever CK is set.
template <bool V>
using flag_c = std::integral_constant<bool, V>;

template <class F>
auto with_variant(const gym_batch* b, F&& f) {   // <U0Z, CK, RL> kernels
    const auto rest = [&](auto U0Z) {
        if (b->flags & GYM_FLAG_REF_LANE) return f(U0Z, flag_c<false>{}, flag_c<true>{});
        if (b->flags & GYM_FLAG_X_CKPT) return f(U0Z, flag_c<true>{}, flag_c<false>{});
        return f(U0Z, flag_c<false>{}, flag_c<false>{});
    };
    return (b->flags & GYM_FLAG_U0_ZERO) ? rest(flag_c<true>{}) : rest(flag_c<false>{});
}
template <class F>
auto with_variant_no_ck(const gym_batch* b, bool extra, F&& f) {   // <U0Z, CK, RL, X> kernels, X never with CK
    return with_variant(b, [&](auto U0Z, auto CK, auto RL) {
        if constexpr (decltype(CK)::value) return f(U0Z, CK, RL, flag_c<false>{});
        else return extra ? f(U0Z, CK, RL, flag_c<true>{}) : f(U0Z, CK, RL, flag_c<false>{});
    });
}
template <class F>
auto with_variant2(const gym_batch* b, F&& f) {   // <U0Z, RL> kernels (no checkpointed form)
    return with_variant(b, [&](auto U0Z, auto, auto RL) { return f(U0Z, RL); });
}
template <class F>
auto with_variant2(const gym_batch* b, bool extra, F&& f) {   // <U0Z, RL, X> kernels
    return with_variant2(b, [&](auto U0Z, auto RL) {
        return extra ? f(U0Z, RL, flag_c<true>{}) : f(U0Z, RL, flag_c<false>{});
    });
}

inline bool bad_dims(int64_t B, int64_t Bp, int N) {
    return B <= 0 || Bp < B || (Bp % 64) != 0 || Bp > GYM_MAX_BP || N < 2;
}

inline int launch_status() { return (int)hipGetLastError(); }

template <class Src>
int launch_unpack_tiled(const Src& src, double* dst, int64_t B, int64_t Bp, int L, int C, hipStream_t st,
                        const int64_t* map = nullptr) {
    const int ts = tile_knots(C);
    if (C * TILE_PITCH > TILE_DOUBLES) return GYM_EINVAL;
    const dim3 grid((unsigned)(Bp / BLK), (unsigned)((L + ts - 1) / ts));
    const size_t lds = sizeof(double) * ts * C * TILE_PITCH;
    if (C == 2)
        hipLaunchKernelGGL((k_unpack_tiled<Src, 2>), grid, dim3(TILE_THREADS), lds, st, src, dst, map, B, Bp, L, C, ts);
    else if (C == 4)
        hipLaunchKernelGGL((k_unpack_tiled<Src, 4>), grid, dim3(TILE_THREADS), lds, st, src, dst, map, B, Bp, L, C, ts);
    else if (C == 8)
        hipLaunchKernelGGL((k_unpack_tiled<Src, 8>), grid, dim3(TILE_THREADS), lds, st, src, dst, map, B, Bp, L, C, ts);
    else
        hipLaunchKernelGGL((k_unpack_tiled<Src, 0>), grid, dim3(TILE_THREADS), lds, st, src, dst, map, B, Bp, L, C, ts);
    return launch_status();
}

inline Mat4 mat4(const double* p) { Mat4 m; for (int i = 0; i < 16; ++i) m.v[i] = p[i]; return m; }
inline Mat2 mat2(const double* p) { Mat2 m; for (int i = 0; i < 4; ++i) m.v[i] = p[i]; return m; }

inline SolverCtl solver_ctl(const gym_armijo* a, const gym_batch* b, int k) {
    return SolverCtl{a->tol, a->beta, a->c, a->gamma0, a->max_ls, k, b->hist_len, 0};
}

// The fields every by-value argument struct (PhaseArgs, RunArgs, TailArgs) has under the same names, from
// (m, w, a, b) and the iteration k ...
template <class Args>
void shared_args(Args& r, const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b, int k) {
    const bool hist = a->record_history != 0;
    r.m = Dyn(*m);
    r.w = kw(*w);
    r.a = solver_ctl(a, b, k);
    r.K1 = (double2*)b->K1; r.cs = b->cs; r.xr = b->x_ref; r.ur = b->u_ref;
    r.cost = b->cost; r.dJ = b->dJ; r.smax = b->smax; r.gamma = b->gamma;
    r.status = b->status; r.n_iter = b->n_iter; r.res_buf = b->res_buf; r.n_roll = b->n_roll;
    r.hist_cost = hist ? b->hist_cost : nullptr; r.hist_smax = hist ? b->hist_smax : nullptr;
}
// ... and with both state / control buffers, the part RunArgs and TailArgs embed
inline void lane_args(LaneArgs& r, const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                      int k0) {
    shared_args(r, m, w, a, b, k0);
    for (int i = 0; i < 2; ++i) { r.x[i] = (double2*)b->x[i]; r.u[i] = b->u[i]; }
}

// the kernels that more than one entry point launches
inline auto sigma_kernel(const gym_batch* b) {
    return with_variant(b, [](auto U0Z, auto CK, auto RL) { return k_nt_sigma<U0Z(), CK(), RL()>; });
}
inline auto backward_all_kernel(const gym_batch* b) {
    return with_variant(b, [](auto U0Z, auto CK, auto RL) { return k_nt_backward_all<U0Z(), CK(), RL()>; });
}

// The statistics of the lanes in rg after iteration k (deterministic partial + final reduction): stats_out[0..7],
// and, if other != NULL, total[s] = other[s] + stats_out[s]; *counter (the retry count, statistic 4) is reset.
inline void launch_stats(const gym_batch* b, Range rg, int k, int32_t* counter, double* stats_out, const double* other,
                         double* total, hipStream_t st) {
    hipLaunchKernelGGL(k_stats_partial, dim3(STAT_BLOCKS), dim3(STAT_THREADS), 0, st, b->status, b->cost, b->smax,
                       b->n_iter, b->n_roll, b->partials, rg, k);
    hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(64 * NSTAT), 0, st, b->partials, counter, stats_out, other, total,
                       STAT_BLOCKS);
}

// what a limited solve's sigma is unpacked from: sigma0 recomputed on the batch's weights, or with a per-lane weight
// table (the entry point's extra argument) on the lane's
template <class... X>
SrcSigma sigma_src(const gym_weights* w, const gym_batch* b, X...) {
    return SrcSigma{kw(*w), b->cs, b->u[0], b->u[1], b->u_ref, b->n_iter,
                    (b->flags & GYM_FLAG_REF_LANE) ? 2 * (int64_t)(b->N - 1) : 0};
}
inline SrcSigmaRows sigma_src(const gym_weights*, const gym_batch* b, const gym_weights* rows) {
    return SrcSigmaRows{rows, b->cs, b->u[0], b->u[1], b->u_ref, b->n_iter,
                        (b->flags & GYM_FLAG_REF_LANE) ? 2 * (int64_t)(b->N - 1) : 0};
}

}  // namespace

// ==========================================================================================
// C-ABI
// ==========================================================================================
extern "C" {

int gym_abi_version(void) { return GYM_ABI_VERSION; }

// _build.source_hash() of the sources this library was compiled from (-DGYM_BUILD_ID); the tag lets the build
// script read it from the file without loading the library
#ifndef GYM_BUILD_ID
#define GYM_BUILD_ID "unversioned"
#endif
static const char gym_build_id_tagged[] = "gym-build-id:" GYM_BUILD_ID;
const char* gym_build_id(void) { return gym_build_id_tagged + sizeof("gym-build-id:") - 1; }

int gym_model_from_params(const double p[11], double dt, gym_model* out) {
    if (!p || !out) return GYM_EINVAL;
    const double m1 = p[0], m2 = p[1], l1 = p[2], lc1 = p[3], lc2 = p[5], I1 = p[6], I2 = p[7], g = p[8];
    out->a = I1 + I2 + lc1 * lc1 * m1 + m2 * (l1 * l1 + lc2 * lc2);
    out->b = m2 * l1 * lc2;
    out->d = I2 + lc2 * lc2 * m2;
    out->g1 = g * (lc1 * m1 + m2 * l1);
    out->g2 = g * m2 * lc2;
    out->f1 = p[9];
    out->f2 = p[10];
    out->dt = dt;
    return 0;
}

// n parameter sets (n,11) -> n models, each gym_model_from_params' own; refused unless every entry is finite and the
// mass matrix is positive definite at every theta2: d > 0 and d (a - d) > b^2, gym::accel's denominator dad - bb cos^2
int gym_models_from_params(const double* params, int64_t n, double dt, gym_model* out) {
    if (!params || !out || n < 1) return GYM_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        const double* p = params + 11 * i;
        for (int j = 0; j < 11; ++j)
            if (!(p[j] - p[j] == 0.0)) return GYM_EINVAL;   // inf - inf and NaN - NaN are NaN
        gym_model* o = out + i;
        gym_model_from_params(p, dt, o);
        if (!(o->d > 0.0 && o->d * (o->a - o->d) > o->b * o->b)) return GYM_EINVAL;
    }
    return 0;
}

static int point_op(const gym_model* m, const double* x, const double* u, double* o1, double* o2, int64_t n, void* s,
                    int what) {
    if (!m || !x || !u || !o1 || n < 0 || (what == 2 && !o2)) return GYM_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_point, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, Dyn(*m), x, u, o1, o2, n, what);
    return launch_status();
}

int gym_continuous_dynamics(const gym_model* m, const double* x, const double* u, double* xdot, int64_t n, void* s) {
    return point_op(m, x, u, xdot, nullptr, n, s, 0);
}
int gym_rk4_step(const gym_model* m, const double* x, const double* u, double* xnext, int64_t n, void* s) {
    return point_op(m, x, u, xnext, nullptr, n, s, 1);
}
int gym_jacobians(const gym_model* m, const double* x, const double* u, double* A, double* Bc, int64_t n, void* s) {
    return point_op(m, x, u, A, Bc, n, s, 2);
}

int gym_stage_cost_derivs(const double* x, const double* xr, const double* u, const double* ur, const double Q[16],
                          const double R[4], int32_t terminal, double* l, double* gx, double* gu, int64_t n,
                          void* s) {
    if (!x || !xr || !Q || !l || !gx || n < 0) return GYM_EINVAL;
    if (!terminal && (!u || !ur || !R || !gu)) return GYM_EINVAL;
    if (n == 0) return 0;
    const double zero4[4] = {0, 0, 0, 0};
    hipLaunchKernelGGL(k_stage_cost_derivs, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, x, xr, u, ur,
                       mat4(Q), mat2(R ? R : zero4), (int)terminal, l, gx, gu, n);
    return launch_status();
}

int gym_pack_lanes(const double* src, double* dst, int64_t B, int64_t Bp, int32_t L, int32_t C, int32_t W, void* s) {
    if (!src || !dst || bad_dims(B, Bp, 2) || L <= 0 || C <= 0 || (W != 1 && W != 2) || (C % W)) return GYM_EINVAL;
    const int64_t n = (int64_t)L * (C / W) * Bp;
    hipLaunchKernelGGL(k_pack, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)s, src, dst, B, Bp, L, C, W);
    return launch_status();
}

int gym_unpack_lanes(const double* s0, const double* s1, const int32_t* sel, double* dst, int64_t B, int64_t Bp,
                     int32_t L, int32_t C, int32_t W, void* s) {
    if (!s0 || !dst || bad_dims(B, Bp, 2) || L <= 0 || C <= 0 || (W != 1 && W != 2) || (C % W) || (sel && !s1))
        return GYM_EINVAL;
    if (W == 2)
        return launch_unpack_tiled(SrcPairs{(const double2*)s0, (const double2*)(s1 ? s1 : s0), sel, C / 2}, dst, B,
                                   Bp, L, C, (hipStream_t)s);
    return launch_unpack_tiled(SrcPlanes{s0, s1 ? s1 : s0, sel, C}, dst, B, Bp, L, C, (hipStream_t)s);
}

int gym_unpack_gains(const double* K1, double* K, int64_t B, int64_t Bp, int32_t T, void* s) {
    if (!K1 || !K || bad_dims(B, Bp, 2) || T <= 0) return GYM_EINVAL;
    return launch_unpack_tiled(SrcGains{(const double2*)K1}, K, B, Bp, T, 8, (hipStream_t)s);
}

int gym_rollout_open_loop(const gym_model* m, const gym_weights* w, const double* x0, const double* u,
                          const double* xr, const double* ur, double* x, double* cost, int64_t B, int64_t Bp,
                          int32_t N, void* s) {
    if (!m || !w || !x0 || !u || !xr || !ur || !x || bad_dims(B, Bp, N)) return GYM_EINVAL;
    hipLaunchKernelGGL(k_open_loop, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), kw(*w), x0, u, xr, ur,
                       (double2*)x, cost, B, Bp, N);
    return launch_status();
}

int gym_closed_loop(const gym_model* m, const gym_weights* w, const double* x, const double* u, const double* Kf,
                    const double* sigma, const double* gamma, const double* xr, const double* ur, double* xn,
                    double* un, double* cost, int64_t B, int64_t Bp, int32_t N, void* s) {
    if (!m || !w || !x || !u || !Kf || !sigma || !gamma || !xr || !ur || !xn || !un || bad_dims(B, Bp, N))
        return GYM_EINVAL;
    hipLaunchKernelGGL(k_closed_loop, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), kw(*w),
                       (const double2*)x, u, (const double2*)Kf, sigma, gamma, xr, ur, (double2*)xn, un, cost, B, Bp,
                       N);
    return launch_status();
}

int gym_total_cost(const double* x, const double* u, const double* xr, const double* ur, const double Q[16],
                   const double R[4], const double QT[16], double* cost, int64_t B, int64_t Bp, int32_t N, void* s) {
    if (!x || !u || !xr || !ur || !Q || !R || !QT || !cost || bad_dims(B, Bp, N)) return GYM_EINVAL;
    hipLaunchKernelGGL(k_total_cost, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, (const double2*)x, u, xr,
                       ur, mat4(Q), mat2(R), mat4(QT), cost, B, Bp, N);
    return launch_status();
}

int gym_backward_sweep(const gym_model* m, const gym_weights* w, const double* x, const double* u, const double* xr,
                       const double* ur, double* K1, double* sigma, double* dJ, double* smax, double* lambda, int64_t B,
                       int64_t Bp, int32_t N, void* s) {
    if (!m || !w || !x || !u || !xr || !ur || !K1 || !sigma || bad_dims(B, Bp, N)) return GYM_EINVAL;
    hipLaunchKernelGGL(k_backward_api, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), kw(*w),
                       (const double2*)x, u, xr, ur, (double2*)K1, sigma, dJ, smax, (double2*)lambda, B, Bp, N);
    return launch_status();
}

int gym_linearize(const gym_model* m, const gym_weights* w, const double* x, const double* u, const double* xr,
                  const double* ur, double* Ad, double* Bd, double* q, double* r, double* qT, int64_t B, int64_t Bp,
                  int32_t N, void* s) {
    if (!m || !w || !x || !u || !xr || !ur || !Ad || !Bd || !q || !r || !qT || bad_dims(B, Bp, N)) return GYM_EINVAL;
    hipLaunchKernelGGL(k_linearize, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), kw(*w), (const double2*)x, u,
                       xr, ur, Ad, Bd, q, r, qT, B, Bp, N);
    return launch_status();
}

int gym_linearize_rk4(const gym_model* m, const gym_weights* w, const double* x, const double* u, const double* xr,
                      const double* ur, double* Ad, double* Bd, double* q, double* r, double* qT, int64_t B, int64_t Bp,
                      int32_t N, void* s) {
    if (!m || !w || !x || !u || !xr || !ur || !Ad || !Bd || !q || !r || !qT || bad_dims(B, Bp, N)) return GYM_EINVAL;
    hipLaunchKernelGGL(k_linearize_rk4, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), kw(*w),
                       (const double2*)x, u, xr, ur, Ad, Bd, q, r, qT, B, Bp, N);
    return launch_status();
}

int gym_riccati_general(const double* A, const double* Bm, const double* Q, const double* R, const double* S,
                        const double* q, const double* r, const double* QT, const double* qT, double* K, double* sigma,
                        double* dJ, int64_t B, int64_t Bp, int32_t T, void* s) {
    if (!A || !Bm || !Q || !R || !S || !q || !r || !QT || !qT || !K || !sigma || !dJ || bad_dims(B, Bp, T + 1))
        return GYM_EINVAL;
    hipLaunchKernelGGL(k_riccati_general, dim3(grid_for(B, BLK)), dim3(BLK), 0, (hipStream_t)s, A, Bm, Q, R, S, q, r,
                       QT, qT, K, sigma, dJ, B, Bp, T);
    return launch_status();
}

// every batch entry point: the buffers, the sizes and the flag combination (per-lane references are never
// combined with state checkpointing: no kernel instantiates both)
static bool bad_batch(const gym_batch* b) {
    return !b || bad_dims(b->B, b->Bp, b->N) || (b->cand_scratch && (b->cand_slots < 0 || b->cand_slots % BLK != 0 ||
                                                                    b->cand_slots > GYM_MAX_BP)) || !b->x[0] || !b->x[1] || !b->u[0] || !b->u[1] || !b->K1 || !b->cs ||
           !b->x_ref || !b->u_ref || !b->cost || !b->dJ || !b->smax || !b->gamma || !b->status || !b->n_iter ||
           !b->res_buf || !b->n_roll || !b->retry_list || !b->counters || !b->partials || !b->stats ||
           ((b->flags & GYM_FLAG_REF_LANE) && (b->flags & GYM_FLAG_X_CKPT));
}

// What both init entry points clear: the control planes (zero_u0: u[0] too; u[1] only with GYM_FLAG_U0_ZERO, whose
// trials never write the u0 planes, so both buffers' stay zero), the counters and the statistics.
static hipError_t reset_batch(const gym_batch* b, bool zero_u0, hipStream_t st) {
    const size_t u_bytes = sizeof(double) * 2 * (size_t)(b->N - 1) * b->Bp;
    hipError_t e = zero_u0 ? hipMemsetAsync(b->u[0], 0, u_bytes, st) : hipSuccess;
    if (e == hipSuccess && (b->flags & GYM_FLAG_U0_ZERO)) e = hipMemsetAsync(b->u[1], 0, u_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(b->counters, 0, sizeof(int32_t) * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(b->stats, 0, sizeof(double) * 24, st);
    return e;
}

// gym_newton_init / gym_newton_init_warm; table: none, or the (Bp) table of gym_newton_init_models (per-lane models)
// or gym_newton_init_weights (per-lane weights), which the init kernels take after w
extern "C++" template <class... Tb>
static int init_cold(const gym_model* m, const gym_weights* w, const double* x0, const gym_batch* b, void* s,
                     Tb... table) {
    if (!m || !w || !x0 || bad_batch(b)) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const hipError_t e = reset_batch(b, true, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(with_variant2(b, [](auto, auto RL) { return k_init<RL(), Tb...>; }), dim3(grid_for(b->Bp, BLK)),
                       dim3(BLK), 0, st, Dyn(*m), kw(*w), table..., x0, b->u[0], b->x_ref, b->u_ref,
                       (double2*)b->x[0], b->cost, b->status, b->n_iter, b->res_buf, b->n_roll, b->gamma, b->smax,
                       b->dJ, b->B, b->Bp, b->N);
    return launch_status();
}

extern "C++" template <class... Tb>
static int init_warm(const gym_model* m, const gym_weights* w, const double* x0, const double* u_init,
                     const int32_t* status_init, const gym_batch* b, void* s, Tb... table) {
    if (!m || !w || !x0 || !u_init || bad_batch(b) || ((uintptr_t)u_init & 15)) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const int T = b->N - 1;
    if ((T + GP_TS - 1) / GP_TS > 65535) return GYM_EINVAL;   // the gather-pack's grid.y
    const hipError_t e = reset_batch(b, false, st);
    if (e != hipSuccess) return (int)e;
    // u[0] <- the caller's controls (every element of the planes is written: padding lanes zero)
    hipLaunchKernelGGL(k_gather_pack_u, dim3((unsigned)(b->Bp / BLK), (unsigned)((T + GP_TS - 1) / GP_TS)),
                       dim3(TILE_THREADS), 0, st, (const double2*)u_init, b->u[0], b->lane_map, b->B, b->Bp, T);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_init_warm<U0Z(), RL(), Tb...>; }),
                       dim3(grid_for(b->Bp, BLK)), dim3(BLK), 0, st, Dyn(*m), kw(*w), table..., x0, status_init,
                       b->lane_map, b->u[0], b->x_ref, b->u_ref, (double2*)b->x[0], b->cost, b->status, b->n_iter,
                       b->res_buf, b->n_roll, b->gamma, b->smax, b->dJ, b->B, b->Bp, b->N);
    return launch_status();
}

int gym_newton_init(const gym_model* m, const gym_weights* w, const double* x0, const gym_batch* b, void* s) {
    return init_cold(m, w, x0, b, s);
}

int gym_newton_init_warm(const gym_model* m, const gym_weights* w, const double* x0, const double* u_init,
                         const int32_t* status_init, const gym_batch* b, void* s) {
    return init_warm(m, w, x0, u_init, status_init, b, s);
}

// a per-lane table (gymnast_acrobot_models.h, gymnast_newton_weights.h): present and 16-byte aligned (the rows are
// read as 16-byte pairs)
static bool bad_table(const void* rows) { return !rows || ((uintptr_t)rows & 15); }
// the flags no Newton entry point with a per-lane table takes (as the box solve)
static bool table_flags(const gym_batch* b) { return b && (b->flags & (GYM_FLAG_X_CKPT | GYM_FLAG_SIGMA_STREAM)); }

int gym_newton_init_models(const gym_model* m, const gym_model* models, const gym_weights* w, const double* x0,
                           const double* u_init, const int32_t* status_init, const gym_batch* b, void* s) {
    if (bad_table(models) || table_flags(b)) return GYM_EINVAL;
    return u_init ? init_warm(m, w, x0, u_init, status_init, b, s, models) : init_cold(m, w, x0, b, s, models);
}

int gym_newton_init_weights(const gym_model* m, const gym_weights* w, const gym_weights* weights, const double* x0,
                            const double* u_init, const int32_t* status_init, const gym_batch* b, void* s) {
    if (bad_table(weights) || table_flags(b)) return GYM_EINVAL;
    return u_init ? init_warm(m, w, x0, u_init, status_init, b, s, weights) : init_cold(m, w, x0, b, s, weights);
}

// Grid caps of the post-trial kernels (grid-stride over the retry list; any cap is correct).  They launch every
// phase, also when no lane rejected trial 1 (the device-side count is not known to the host).  Lower caps (256 /
// 64) measured the same at 262,144 lanes and 2% slower on the stress start: the gap between phases is
// launch latency, not workgroup dispatch.
constexpr int64_t POST_CAP = 2048;
constexpr int64_t CAND_CAP = 4096;
// the candidate scratch of the batch (gym_batch.cand_scratch): none without lane-pair candidates or with state
// checkpointing (whose accepted re-run stores the checkpoint knots only)
static CandScratch cand_scratch(const gym_batch* b, bool pair) {
    CandScratch c{nullptr, nullptr, nullptr, 0};
    if (!pair || !b->cand_scratch || b->cand_slots <= 0 || (b->flags & GYM_FLAG_X_CKPT)) return c;
    const int64_t V = b->cand_slots, N = b->N;
    c.sx = (double2*)b->cand_scratch;
    c.su = b->cand_scratch + 4 * N * V;
    c.sJ = c.su + 2 * (N - 1) * V;
    c.V = V;
    return c;
}
static void launch_post_trial(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                              const SolverCtl& c, const TrialIO& io, Range rg, int32_t* counter, double* stats_out,
                              const double* other, double* total, hipStream_t st, bool sigma_streamed = false) {
    const int64_t n = rg.hi - rg.lo;
    const double2* K1 = (const double2*)b->K1;
    const double* cs = b->cs;
    double* hc = a->record_history ? b->hist_cost : nullptr;
    if (a->max_ls > 1 && n > 0) {
        if (!sigma_streamed) {   // the lanes that reject trial 1 need sigma1: re-run their sweep into its plane
            TimedLaunch tl(b->timing, 7, st);
            hipLaunchKernelGGL(sigma_kernel(b), dim3(grid_for(n, BLK, POST_CAP)), dim3(BLK), 0, st, Dyn(*m), kw(*w),
                               io.x, io.u, b->x_ref, b->u_ref, b->cs, b->retry_list + rg.lo, counter,
                               (const int32_t*)nullptr, -1, b->B, b->Bp, b->N);
        }
        // candidates on lane pairs (recorded in the scratch slots, if any) unless single-lane chains were asked for
        const bool pair = !(b->flags & GYM_FLAG_RUN_SINGLE);
        const CandScratch sc = cand_scratch(b, pair);
        const int64_t ncand = n * (int64_t)(a->max_ls - 1);
        {
            TimedLaunch tl(b->timing, 2, st);
            if (pair)
                hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_cand_pair<U0Z(), RL()>; }),
                                   dim3(grid_for(2 * ncand, BLK, CAND_CAP)), dim3(BLK), 0, st, Dyn(*m), kw(*w), c, io,
                                   K1, cs, b->x_ref, b->u_ref, b->cost, b->dJ, b->retry_list + rg.lo, counter,
                                   b->cand_ok, sc, b->Bp, b->N);
            else
                hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_candidates<U0Z(), RL()>; }),
                                   dim3(grid_for(ncand, BLK, CAND_CAP)), dim3(BLK), 0, st, Dyn(*m), kw(*w), c, io, K1,
                                   cs, b->x_ref, b->u_ref, b->cost, b->dJ, b->retry_list + rg.lo, counter, b->cand_ok,
                                   b->Bp, b->N);
        }
        const int64_t items = sc.V > 0 ? n * (1 + (b->N + CPK - 1) / CPK) : n;
        TimedLaunch tl(b->timing, 3, st);
        hipLaunchKernelGGL(with_variant(b, [](auto U0Z, auto CK, auto RL) { return k_nt_retry<U0Z(), CK(), RL()>; }),
                           dim3(grid_for(items, BLK, POST_CAP)), dim3(BLK), 0, st, Dyn(*m), kw(*w), c, io, K1, cs,
                           b->x_ref, b->u_ref, b->cost, b->smax, b->gamma, b->status, b->n_iter, b->res_buf, b->n_roll,
                           b->retry_list + rg.lo, counter, b->cand_ok, hc, sc, b->Bp, b->N);
    }
    TimedLaunch tl(b->timing, 4, st);
    launch_stats(b, rg, c.k, counter, stats_out, other, total, st);
}

static TrialIO trial_io(const gym_batch* b, int k) {
    return TrialIO{(const double2*)b->x[k & 1], b->u[k & 1], (double2*)b->x[(k + 1) & 1], b->u[(k + 1) & 1]};
}

static bool bad_iter_args(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b) {
    return !m || !w || !a || bad_batch(b) || a->max_ls < 1 || (a->max_ls > 1 && !b->cand_ok);
}

int gym_newton_iteration(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b, int32_t k,
                         void* s) {
    if (bad_iter_args(m, w, a, b) || k < 0) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const Range all{0, b->B};
    const TrialIO io = trial_io(b, k);
    const int grid = grid_for(b->B, BLK);
    const bool hist = a->record_history != 0;
    // GYM_FLAG_SIGMA_STREAM: the sweep also stores sigma1 (8 B per stage), so the lanes that reject trial 1 need no
    // re-run of it (a chain as long as the sweep's, for however few lanes)
    const bool sig = (b->flags & GYM_FLAG_SIGMA_STREAM) != 0;
    {
        TimedLaunch tl(b->timing, 0, st);
        const auto sweep =
            with_variant(b, [](auto U0Z, auto CK, auto RL) { return k_nt_backward<U0Z(), CK(), RL()>; });
        hipLaunchKernelGGL(sig ? backward_all_kernel(b) : sweep, dim3(grid), dim3(BLK), 0, st, Dyn(*m), kw(*w), io.x,
                           io.u, b->x_ref, b->u_ref, (double2*)b->K1, b->cs, a->gamma0, b->dJ, b->smax, b->status,
                           hist ? b->hist_smax : nullptr, all, b->Bp, b->N, k, b->hist_len);
    }
    const SolverCtl c = solver_ctl(a, b, k);
    {
        TimedLaunch tl(b->timing, 1, st);
        hipLaunchKernelGGL(with_variant(b, [](auto U0Z, auto CK, auto RL) { return k_nt_trial<U0Z(), CK(), RL()>; }),
                           dim3(grid), dim3(BLK), 0, st, Dyn(*m), kw(*w), c, io, (const double2*)b->K1,
                           (const double*)b->cs, b->x_ref, b->u_ref, b->cost, b->dJ, b->smax, b->gamma, b->status,
                           b->n_iter, b->res_buf, b->n_roll, b->retry_list, b->counters, hist ? b->hist_cost : nullptr,
                           all, b->Bp, b->N);
    }
    launch_post_trial(m, w, a, b, c, io, all, b->counters, b->stats, nullptr, nullptr, st, sig);
    return launch_status();
}

// compute units of the current device (cached per device index; 0 if the query fails)
static int device_cus() {
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!cache[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cache[dev] = n;
    }
    return cache[dev];
}

// The phase kernel for a launch of `waves` wavefronts: the two-wavefront build (k_nt_phase<..., LO>) when the
// launch fills the SIMDs with more than LO_MIN_EIGHTHS/8 = 7/4 and at most 2 wavefronts each (profiles/r06/README.md "pd2":
// same-buffer A/B over batch sizes), the four-wavefront build otherwise.
constexpr int LO_MIN_EIGHTHS = 14;
static bool phase_low_occupancy(const gym_batch* b, int64_t waves) {
    if (b->flags & GYM_FLAG_X_CKPT) return false;
    const int64_t simds = 4 * (int64_t)device_cus();
    return simds > 0 && 8 * waves > LO_MIN_EIGHTHS * simds && waves <= 2 * simds;
}

int gym_newton_phase_kind(const gym_batch* b, int32_t* low_out) {
    if (bad_batch(b) || !low_out) return GYM_EINVAL;
    int64_t Bh;
    gym_newton_pipeline_split(b, &Bh);
    const int64_t waves = (Bh + BLK - 1) / BLK + (b->B - Bh + BLK - 1) / BLK;
    *low_out = phase_low_occupancy(b, waves) ? 1 : 0;
    return 0;
}

int gym_newton_pipeline_split(const gym_batch* b, int64_t* Bh) {
    if (!b || !Bh || b->B <= 0) return GYM_EINVAL;
    int64_t h = ((b->B + 1) / 2 + 63) / 64 * 64;
    *Bh = h < b->B ? h : b->B;
    return 0;
}

int gym_newton_phase(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b, int32_t p,
                     int32_t do_backward, void* s) {
    if (bad_iter_args(m, w, a, b) || p < 0) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    int64_t Bh;
    gym_newton_pipeline_split(b, &Bh);
    const Range half[2] = {{0, Bh}, {Bh, b->B}};
    // backward half: H0 on even phases (iteration p/2), H1 on odd phases (iteration (p-1)/2)
    const int hb = p & 1, kb = p >> 1;
    const Range rb = do_backward ? half[hb] : Range{0, 0};
    // trial half: H0 on odd phases (iteration (p-1)/2), H1 on even phases >= 2 (iteration (p-2)/2)
    const int ht = (p & 1) ? 0 : 1;
    const int kt = (p & 1) ? (p - 1) >> 1 : (p - 2) >> 1;
    const Range rt = (p >= 1) ? half[ht] : Range{0, 0};
    const int nb_b = (int)((rb.hi - rb.lo + BLK - 1) / BLK), nb_t = (int)((rt.hi - rt.lo + BLK - 1) / BLK);
    const SolverCtl c = solver_ctl(a, b, kt < 0 ? 0 : kt);
    const TrialIO io = trial_io(b, c.k);
    if (nb_b + nb_t > 0) {
        TimedLaunch tl(b->timing, (p & 1) ? 5 : 6, st);
        PhaseArgs pa;
        shared_args(pa, m, w, a, b, c.k);
        pa.io = io;
        pa.xb_in = (const double2*)b->x[kb & 1]; pa.ub_in = b->u[kb & 1];
        pa.retry_list = b->retry_list; pa.counter = b->counters + ht;
        pa.rb = rb; pa.rt = rt; pa.Bp = b->Bp; pa.N = b->N; pa.kb = kb; pa.nb_b = nb_b; pa.pad = 0;
        // the two-wavefront build (LO) by the launch's size; never with X_CKPT
        hipLaunchKernelGGL(with_variant_no_ck(b, phase_low_occupancy(b, nb_b + nb_t),
                                              [](auto U0Z, auto CK, auto RL, auto LO) {
                                                  return k_nt_phase<U0Z(), CK(), RL(), LO()>;
                                              }),
                           dim3(nb_b + nb_t), dim3(BLK), 0, st, pa);
    }
    if (p >= 1)  // the trial half's retries and statistics; H1 closes the iteration: total = H0 + H1
        launch_post_trial(m, w, a, b, c, io, rt, b->counters + ht, b->stats + 8 + 8 * ht,
                          ht ? b->stats + 8 : nullptr, ht ? b->stats : nullptr, st);
    return launch_status();
}

int gym_newton_run(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b, int32_t k0,
                   int32_t k1, void* s) {
    // GYM_FLAG_SIGMA_STREAM with the four-wavefront kernel: one iteration per launch, its sweep storing sigma1, the
    // lanes that reject trial 1 finished by the serial schedule's parallel candidates and accepted re-run
    const bool ext = (b->flags & GYM_FLAG_SIGMA_STREAM) && !(b->flags & GYM_FLAG_RUN_SINGLE);
    if (bad_iter_args(m, w, a, b) || k0 < 0 || k1 < k0 || (b->flags & GYM_FLAG_X_CKPT) || (ext && k1 > k0 + 1))
        return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const Range all{0, b->B};
    if (k1 > k0) {
        TimedLaunch tl(b->timing, 8, st);
        RunArgs ra;
        lane_args(ra, m, w, a, b, k0);
        ra.retry_list = b->retry_list; ra.counter = b->counters;
        ra.B = b->B; ra.Bp = b->Bp; ra.N = b->N; ra.k0 = k0; ra.k1 = k1; ra.ext = ext ? 1 : 0;
        if (b->flags & GYM_FLAG_RUN_SINGLE)
            hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_run<U0Z(), RL()>; }),
                               dim3(grid_for(b->B, BLK)), dim3(BLK), 0, st, ra);
        else   // two wavefronts per 64 lanes; every lane of the padded batch takes part (padding: GYM_PAD)
            hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_run2<U0Z(), RL()>; }),
                               dim3((unsigned)(b->Bp / BLK)), dim3(R2WAVES * BLK), 0, st, ra);
        if (ext) {   // iteration k0's retries (the kernel listed the lanes that reject trial 1) and its statistics
            launch_post_trial(m, w, a, b, ra.a, trial_io(b, k0), all, b->counters, b->stats, nullptr, nullptr, st, true);
            return launch_status();
        }
    }
    // the statistics after iteration k1 - 1 ("lanes that ran" = the lanes that executed it; [4] = 0: this
    // schedule keeps no retry list)
    launch_stats(b, all, (int)k1 - 1, b->counters, b->stats, nullptr, nullptr, st);
    return launch_status();
}

// gym_newton_run_box / _rk4 / _models / _weights: variant V's persistent kernel over the iterations k0 .. k1-1, then the
// statistics after iteration k1 - 1, as gym_newton_run
// (extra: the entry point's arguments that V::extra puts into V::Args, the per-lane table of ModelsVariant or
// WeightsVariant)
extern "C++" template <class V, class... X>
static int run_limited(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                       const double* tau_max, int32_t k0, int32_t k1, void* s, X... extra) {
    if (!tau_max || bad_iter_args(m, w, a, b) || k0 < 0 || k1 < k0 ||
        (b->flags & (GYM_FLAG_X_CKPT | GYM_FLAG_SIGMA_STREAM)))
        return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    if (k1 > k0) {
        TimedLaunch tl(b->timing, 8, st);
        typename V::Args ra;
        lane_args(ra, m, w, a, b, k0);
        ra.retry_list = b->retry_list; ra.counter = b->counters;
        ra.B = b->B; ra.Bp = b->Bp; ra.N = b->N; ra.k0 = k0; ra.k1 = k1; ra.ext = 0;
        ra.tau = tau_max;
        V::extra(ra, extra...);
        hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_run_limited<V, U0Z(), RL()>; }),
                           dim3(grid_for(b->B, BLK)), dim3(BLK), 0, st, ra);
    }
    launch_stats(b, Range{0, b->B}, (int)k1 - 1, b->counters, b->stats, nullptr, nullptr, st);
    return launch_status();
}

int gym_newton_run_box(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                       const double* tau_max, int32_t k0, int32_t k1, void* s) {
    return run_limited<BoxVariant>(m, w, a, b, tau_max, k0, k1, s);
}

int gym_newton_run_rk4(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                       const double* tau_max, int32_t k0, int32_t k1, void* s) {
    return run_limited<Rk4Variant>(m, w, a, b, tau_max, k0, k1, s);
}

int gym_newton_run_models(const gym_model* m, const gym_model* models, const gym_weights* w, const gym_armijo* a,
                          const gym_batch* b, const double* tau_max, int32_t k0, int32_t k1, void* s) {
    if (bad_table(models)) return GYM_EINVAL;
    return run_limited<ModelsVariant>(m, w, a, b, tau_max, k0, k1, s, models);
}

int gym_newton_run_weights(const gym_model* m, const gym_weights* w, const gym_weights* weights, const gym_armijo* a,
                           const gym_batch* b, const double* tau_max, int32_t k0, int32_t k1, void* s) {
    if (bad_table(weights)) return GYM_EINVAL;
    return run_limited<WeightsVariant>(m, w, a, b, tau_max, k0, k1, s, weights);
}

// gym_newton_mpc_run: the closed loops' control steps t0 .. t1-1 in one launch of k_nt_mpc_run (newton_mpc.hpp), on the
// arguments of gym_newton_run_box plus the plant table and the outputs; results go to the caller's rows (lane_map)
int gym_newton_mpc_run(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                       const double* tau_max, const gym_model* plant, int32_t t0, int32_t t1, int32_t iters,
                       double* x_cl, double* u_cl, int32_t* step_iters, int32_t* step_rolls, double* step_cost,
                       int32_t* step_stop, void* s) {
    if (!tau_max || bad_table(plant) || bad_iter_args(m, w, a, b) || table_flags(b) || !x_cl || !u_cl ||
        !step_iters || !step_rolls || !step_cost || !step_stop || t0 < 0 || t1 > b->N - 1 || t0 > t1 || iters < 0)
        return GYM_EINVAL;
    if (t1 == t0) return 0;
    MpcRunArgs ra;
    lane_args(ra, m, w, a, b, 0);
    ra.retry_list = b->retry_list; ra.counter = b->counters;
    ra.B = b->B; ra.Bp = b->Bp; ra.N = b->N; ra.k0 = 0; ra.k1 = 0; ra.ext = 0;
    ra.tau = tau_max;
    ra.plant = plant; ra.map = b->lane_map;
    ra.x_cl = x_cl; ra.u_cl = u_cl; ra.s_iter = step_iters; ra.s_roll = step_rolls; ra.s_cost = step_cost;
    ra.s_stop = step_stop;
    ra.t0 = t0; ra.t1 = t1; ra.iters = iters; ra.pad = 0;
    TimedLaunch tl(b->timing, 8, (hipStream_t)s);
    hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_mpc_run<BoxVariant, U0Z(), RL()>; }),
                       dim3(grid_for(b->B, BLK)), dim3(BLK), 0, (hipStream_t)s, ra);
    return launch_status();
}

int gym_newton_tail_scratch(int32_t N, int32_t n_lanes, int32_t max_ls, int64_t* doubles_out) {
    if (!doubles_out || N < 2 || N - 1 > TL_MAX_T || n_lanes < 0 || max_ls < 1 || max_ls > BLK) return GYM_EINVAL;
    const int64_t v = (int64_t)n_lanes * max_ls;
    const int64_t Vp = v > 0 ? (v + BLK - 1) / BLK * BLK : BLK;
    *doubles_out = Vp * (4 * (int64_t)N + 2 * (int64_t)(N - 1));
    return 0;
}

int gym_newton_cand_scratch(int32_t N, int64_t slots, int64_t* doubles_out) {
    if (!doubles_out || N < 2 || slots < 0 || slots % BLK != 0 || slots > GYM_MAX_BP) return GYM_EINVAL;
    *doubles_out = slots * (4 * (int64_t)N + 2 * (int64_t)(N - 1) + 1);
    return 0;
}

int gym_newton_tail_lds(int32_t N, int64_t* bytes_out, int64_t* limit_out) {
    if (!bytes_out || N < 2 || N - 1 > TL_MAX_T) return GYM_EINVAL;
    *bytes_out = (int64_t)tail_lds_bytes(N - 1);
    if (limit_out) {   // the current device's opt-in LDS per workgroup
        int dev = 0, lim = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&lim, hipDeviceAttributeSharedMemPerBlockOptin, dev);
        if (e != hipSuccess) return (int)e;
        *limit_out = lim;
    }
    return 0;
}

int gym_newton_tail(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                    const int32_t* lanes, int32_t n_lanes, double* scratch, int64_t scratch_doubles, int32_t k0,
                    int32_t k1, void* s) {
    int64_t need = 0;
    if (bad_iter_args(m, w, a, b) || k0 < 0 || k1 < k0 || n_lanes < 0 || (n_lanes > 0 && (!lanes || !scratch)) ||
        (b->flags & GYM_FLAG_X_CKPT) || gym_newton_tail_scratch(b->N, n_lanes, a->max_ls, &need) ||
        scratch_doubles < need || (int64_t)n_lanes > b->B)
        return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    if (k1 > k0 && n_lanes > 0) {
        TimedLaunch tl(b->timing, 9, st);
        TailArgs ta;
        lane_args(ta, m, w, a, b, k0);
        ta.list = lanes;
        const int64_t v = (int64_t)n_lanes * a->max_ls;
        ta.Vp = (v + BLK - 1) / BLK * BLK;
        ta.sx = (double2*)scratch;
        ta.su = scratch + 4 * (int64_t)b->N * ta.Vp;
        ta.Bp = b->Bp; ta.N = b->N; ta.k0 = k0; ta.k1 = k1; ta.pad = 0;
        // trials on lane pairs while they fit one wavefront (gym::rk4_pair: the same bits, a shorter chain)
        const bool pair = a->max_ls <= BLK / 2 && !(b->flags & GYM_FLAG_RUN_SINGLE);
        const auto kern =
            with_variant2(b, pair, [](auto U0Z, auto RL, auto PAIR) { return k_nt_tail<U0Z(), RL(), PAIR()>; });
        const size_t lds = tail_lds_bytes(b->N - 1);
        if (lds > 65536) {   // above the default dynamic-LDS limit (gfx950: 160 KiB per workgroup)
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)n_lanes), dim3(TL_THREADS), lds, st, ta);
    }
    // the statistics after iteration k1 - 1, over the whole batch (as gym_newton_run)
    launch_stats(b, Range{0, b->B}, (int)k1 - 1, b->counters, b->stats, nullptr, nullptr, st);
    return launch_status();
}

int gym_newton_fill_states(const gym_model* m, const gym_batch* b, int32_t buf, void* s) {
    if (!m || bad_batch(b) || buf < -1 || buf > 1) return GYM_EINVAL;
    if (!(b->flags & GYM_FLAG_X_CKPT)) return 0;
    hipLaunchKernelGGL(k_fill_states, dim3(grid_for(b->B, BLK)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), (double2*)b->x[0],
                       (double2*)b->x[1], b->u[0], b->u[1], b->res_buf, (int)buf, b->B, b->Bp, b->N);
    return launch_status();
}

int gym_newton_finalize(const gym_model* m, const gym_weights* w, const gym_batch* b, int32_t k_done, double* x_out,
                        double* u_out, double* K_out, double* sig_out, void* s) {
    if (!m || !w || bad_batch(b) || k_done < 0) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(k_finalize_status, dim3(grid_for(b->B, 256)), dim3(256), 0, st, b->status, b->res_buf, b->B,
                       (int)k_done);
    int e = launch_status();
    if (e) return e;
    const int T = b->N - 1;
    if (x_out && (e = gym_newton_fill_states(m, b, -1, s))) return e;
    const int64_t* map = b->lane_map;   // results straight into the caller's lane order
    if (x_out && (e = launch_unpack_tiled(SrcPairs{(const double2*)b->x[0], (const double2*)b->x[1], b->res_buf, 2},
                                          x_out, b->B, b->Bp, b->N, 4, st, map)))
        return e;
    if (u_out && (e = launch_unpack_tiled(SrcPlanes{b->u[0], b->u[1], b->res_buf, 2}, u_out, b->B, b->Bp, T, 2, st,
                                          map)))
        return e;
    if (K_out && (e = launch_unpack_tiled(SrcGains{(const double2*)b->K1}, K_out, b->B, b->Bp, T, 8, st, map)))
        return e;
    if (sig_out && (e = gym_newton_sigma(m, w, b, sig_out, s))) return e;
    return 0;
}

int gym_placement_probe(const gym_batch* b, int32_t cb, void* s) {
    if (bad_batch(b) || cb < 0 || cb > 1 || b->Bp % (2 * BLK) != 0) return GYM_EINVAL;
    hipLaunchKernelGGL(k_placement_probe, dim3((unsigned)(b->Bp / BLK)), dim3(BLK), 0, (hipStream_t)s,
                       (double2*)b->x[cb], (double2*)b->x[cb ^ 1], b->u[cb], b->u[cb ^ 1], (double2*)b->K1, b->cs,
                       b->Bp, b->N - 1);
    return launch_status();
}

int gym_newton_sigma(const gym_model* m, const gym_weights* w, const gym_batch* b, double* sig_out, void* s) {
    if (!m || !w || bad_batch(b) || !sig_out) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const int T = b->N - 1;
    for (int parity = 0; parity < 2; ++parity) {   // sigma1 of each lane's last sweep, one launch per buffer
        hipLaunchKernelGGL(sigma_kernel(b), dim3(grid_for(b->B, BLK)), dim3(BLK), 0, st, Dyn(*m), kw(*w),
                           (const double2*)b->x[parity], b->u[parity], b->x_ref, b->u_ref, b->cs,
                           (const int32_t*)nullptr, (const int32_t*)nullptr, b->n_iter, parity, b->B, b->Bp, b->N);
        const int e = launch_status();
        if (e) return e;
    }
    return launch_unpack_tiled(SrcSigma{kw(*w), b->cs, b->u[0], b->u[1], b->u_ref, b->n_iter,
                                        (b->flags & GYM_FLAG_REF_LANE) ? 2 * (int64_t)(b->N - 1) : 0}, sig_out, b->B, b->Bp,
                               T, 2, st, b->lane_map);
}

// gym_newton_sigma_box / _rk4 / _models / _weights: sigma1 of each lane's last limited sweep by variant V's re-run kernel, one
// launch per buffer, then sigma unpacked
// (extra: the kernel's arguments after N: the per-lane table of ModelsVariant or WeightsVariant)
extern "C++" template <class V, class... X>
static int sigma_limited(const gym_model* m, const gym_weights* w, const gym_batch* b, const double* tau_max,
                         double* sig_out, void* s, X... extra) {
    if (!m || !w || bad_batch(b) || !tau_max || !sig_out || (b->flags & GYM_FLAG_X_CKPT)) return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const auto kern = with_variant2(b, [](auto U0Z, auto RL) { return k_nt_sigma_limited<V, U0Z(), RL(), X...>; });
    for (int parity = 0; parity < 2; ++parity) {
        hipLaunchKernelGGL(kern, dim3(grid_for(b->B, BLK)), dim3(BLK), 0, st, Dyn(*m), kw(*w),
                           (const double2*)b->x[parity], b->u[parity], b->x_ref, b->u_ref, b->cs, tau_max, b->n_iter,
                           parity, b->B, b->Bp, b->N, extra...);
        const int e = launch_status();
        if (e) return e;
    }
    return launch_unpack_tiled(sigma_src(w, b, extra...), sig_out, b->B, b->Bp, b->N - 1, 2, st, b->lane_map);
}

int gym_newton_sigma_box(const gym_model* m, const gym_weights* w, const gym_batch* b, const double* tau_max,
                         double* sig_out, void* s) {
    return sigma_limited<BoxVariant>(m, w, b, tau_max, sig_out, s);
}

int gym_newton_sigma_rk4(const gym_model* m, const gym_weights* w, const gym_batch* b, const double* tau_max,
                         double* sig_out, void* s) {
    return sigma_limited<Rk4Variant>(m, w, b, tau_max, sig_out, s);
}

int gym_newton_sigma_models(const gym_model* m, const gym_model* models, const gym_weights* w, const gym_batch* b,
                            const double* tau_max, double* sig_out, void* s) {
    if (bad_table(models) || table_flags(b)) return GYM_EINVAL;
    return sigma_limited<ModelsVariant>(m, w, b, tau_max, sig_out, s, models);
}

int gym_newton_sigma_weights(const gym_model* m, const gym_weights* w, const gym_weights* weights, const gym_batch* b,
                             const double* tau_max, double* sig_out, void* s) {
    if (bad_table(weights) || table_flags(b)) return GYM_EINVAL;
    return sigma_limited<WeightsVariant>(m, w, b, tau_max, sig_out, s, weights);
}

static int sweep_grid(int64_t Bp, int G) {
    const int64_t nb = (Bp / BLK) * (int64_t)G;
    return (int)((nb + 7) / 8 * 8);
}

int gym_gamma_sweep(const gym_model* m, const gym_weights* w, const double* x, const double* u, const double* Kf,
                    const double* sigma, const double* gammas, int32_t G, const double* xr, const double* ur,
                    double* cost_out, int64_t B, int64_t Bp, int32_t N, void* s) {
    if (!m || !w || !x || !u || !Kf || !sigma || !gammas || !xr || !ur || !cost_out || G < 1 || bad_dims(B, Bp, N) ||
        (Bp / BLK) * (int64_t)G > ((int64_t)1 << 31) - 8)
        return GYM_EINVAL;
    hipLaunchKernelGGL(k_gamma_sweep, dim3(sweep_grid(Bp, G)), dim3(BLK), 0, (hipStream_t)s, Dyn(*m), kw(*w),
                       (const double2*)x, u, (const double2*)Kf, sigma, gammas, (int)G, xr, ur, cost_out, B, Bp, N);
    return launch_status();
}

int gym_newton_gamma_sweep(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* b,
                           int32_t k, const double* gammas, int32_t G, double* cost_out, void* s) {
    if (!m || !w || !a || bad_batch(b) || k < 0 || !gammas || !cost_out || G < 1 ||
        (b->Bp / BLK) * (int64_t)G > ((int64_t)1 << 31) - 8)
        return GYM_EINVAL;
    hipStream_t st = (hipStream_t)s;
    const TrialIO io = trial_io(b, k);
    // iteration k's backward sweep (K1, cg, dJ, smax: the values iteration k itself computes) plus sigma1
    hipLaunchKernelGGL(backward_all_kernel(b), dim3(grid_for(b->B, BLK)), dim3(BLK), 0, st, Dyn(*m), kw(*w),
                       io.x, io.u, b->x_ref, b->u_ref, (double2*)b->K1, b->cs, a->gamma0, b->dJ, b->smax, b->status,
                       (double*)nullptr, Range{0, b->B}, b->Bp, b->N, (int)k, 0);
    int e = launch_status();
    if (e) return e;
    hipLaunchKernelGGL(with_variant2(b, [](auto U0Z, auto RL) { return k_nt_gamma_sweep<U0Z(), RL()>; }),
                       dim3(sweep_grid(b->Bp, G)), dim3(BLK), 0, st, Dyn(*m), kw(*w), io.x, io.u,
                       (const double2*)b->K1, (const double*)b->cs, a->gamma0, gammas, (int)G, b->x_ref, b->u_ref,
                       b->status, cost_out, b->B, b->Bp, b->N);
    return launch_status();
}

#ifdef GYM_TAIL_TRACE
int gym_debug_tail_trace(void* host_out, int reset) {   // diagnostic build only: 4096 x 4 uint64
    if (reset) {
        static unsigned long long zero[4096][4];
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_tail_trace), zero, sizeof(zero));
    }
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tail_trace), sizeof(g_tail_trace));
}
#endif
#ifdef GYM_RUN2_TRACE
int gym_debug_run2_trace(void* host_out, int reset) {   // diagnostic build only: 8192 x 2 x 6 uint64
    if (reset) {
        static unsigned long long zero[8192][2][6];
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_run2_trace), zero, sizeof(zero));
    }
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_run2_trace), sizeof(g_run2_trace));
}
#endif
#ifdef GYM_WAVE_TRACE
int gym_debug_wave_trace(void* host_out) {   // diagnostic build only: 2 x 8192 x 4 uint64
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_wave_trace), sizeof(g_wave_trace));
}
#endif

int gym_timing_create(gym_timing* t) {
    if (!t) return GYM_EINVAL;
    for (int i = 0; i < 2 * GYM_NK; ++i) {
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return (int)r;
        t->ev[i] = (void*)e;
    }
    for (int i = 0; i < 2 * GYM_TIMING_POOL; ++i) {
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return (int)r;
        t->pool_ev[i] = (void*)e;
    }
    for (int i = 0; i < GYM_NK; ++i) { t->ms[i] = 0.0; t->launches[i] = 0; }
    t->pending = 0;
    t->pool_used = 0;
    return 0;
}

int gym_timing_destroy(gym_timing* t) {
    if (!t) return GYM_EINVAL;
    for (int i = 0; i < 2 * GYM_NK; ++i)
        if (t->ev[i]) { (void)hipEventDestroy((hipEvent_t)t->ev[i]); t->ev[i] = nullptr; }
    for (int i = 0; i < 2 * GYM_TIMING_POOL; ++i)
        if (t->pool_ev[i]) { (void)hipEventDestroy((hipEvent_t)t->pool_ev[i]); t->pool_ev[i] = nullptr; }
    t->pool_used = 0;
    return 0;
}

int gym_timing_collect(gym_timing* t) {
    if (!t) return GYM_EINVAL;
    // every recorded pair is read first and committed only when all of them succeeded: on an error (e.g.
    // hipErrorNotReady, the stream not synchronised) the record is unchanged and a later collect counts each pair once
    double ms_add[GYM_NK] = {};
    int n_add[GYM_NK] = {};
    for (int i = 0; i < GYM_NK; ++i) {
        if (!(t->pending & (1 << i))) continue;
        float ms = 0.f;
        hipError_t r = hipEventElapsedTime(&ms, (hipEvent_t)t->ev[2 * i], (hipEvent_t)t->ev[2 * i + 1]);
        if (r != hipSuccess) return (int)r;
        ms_add[i] += ms;
        n_add[i] += 1;
    }
    for (int j = 0; j < t->pool_used; ++j) {
        float ms = 0.f;
        hipError_t r = hipEventElapsedTime(&ms, (hipEvent_t)t->pool_ev[2 * j], (hipEvent_t)t->pool_ev[2 * j + 1]);
        if (r != hipSuccess) return (int)r;
        ms_add[t->pool_kind[j]] += ms;
        n_add[t->pool_kind[j]] += 1;
    }
    for (int i = 0; i < GYM_NK; ++i) {
        t->ms[i] += ms_add[i];
        t->launches[i] += n_add[i];
    }
    t->pending = 0;
    t->pool_used = 0;
    return 0;
}

}  // extern "C"
