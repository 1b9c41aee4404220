// MI355X (gfx950) kernels of the LQR / receding-horizon MPC trackers (trajectory_tracking.py), C-ABI part 2.
//
// Both trackers follow ONE reference trajectory that every lane shares (main.py task_3 / task_4), so their
// feedback gains are lane-independent:
//   * LQR (solve_LQR_tracking :170-203): one backward recursion along the reference;
//   * MPC (solve_mpc_tracking :8-69 with solver_mpc :73-140): at control step t the QP over the window
//     [t, t + T_pred - 1] of the shifted reference (padded with (A_f, B_f)) has only equality constraints
//     (test_constraints = False, :87), so its exact solution is u_0 = K_0(t) x_0 with K_0(t) the first gain of
//     the window's finite-horizon LQ recursion.  All T windows are solved in parallel, one thread each.
// The batched part is the closed-loop RK4 simulation of B perturbed initial states under the shared
// feed-forward / feedback sequence (simulate_tracking :206-216 and the MPC loop :43-60), one lane per thread
// with the gains, reference and feed-forward read through wave-uniform (scalar) loads.
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

using gym::Dyn;

namespace {

struct M44 { double v[16]; };
struct M22 { double v[4]; };

// one step of the reference's recursion (trajectory_tracking.py:158-160 / :195-200):
//   aux1 = R + B'PB, aux2 = B'PA, K = -inv(aux1) aux2, P <- Q + A'PA + (A'PB) K
__device__ __forceinline__ void lqr_step(const double* A, const double* Bm, double* P, const M44& Q, const M22& R,
                                         double* K) {
    double PA[16], PB[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            PA[4 * i + j] = ((P[4 * i] * A[j] + P[4 * i + 1] * A[4 + j]) + P[4 * i + 2] * A[8 + j]) + P[4 * i + 3] * A[12 + j];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            PB[2 * i + j] = ((P[4 * i] * Bm[j] + P[4 * i + 1] * Bm[2 + j]) + P[4 * i + 2] * Bm[4 + j]) + P[4 * i + 3] * Bm[6 + j];
    }
    double a1[4], a2[8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            a1[2 * i + j] = R.v[2 * i + j] + (((Bm[i] * PB[j] + Bm[2 + i] * PB[2 + j]) + Bm[4 + i] * PB[4 + j]) + Bm[6 + i] * PB[6 + j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            a2[4 * i + j] = ((Bm[i] * PA[j] + Bm[2 + i] * PA[4 + j]) + Bm[4 + i] * PA[8 + j]) + Bm[6 + i] * PA[12 + j];
    }
    const double idet = 1.0 / (a1[0] * a1[3] - a1[1] * a1[2]);
    const double i00 = a1[3] * idet, i01 = -a1[1] * idet, i10 = -a1[2] * idet, i11 = a1[0] * idet;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        K[j] = -(i00 * a2[j] + i01 * a2[4 + j]);
        K[4 + j] = -(i10 * a2[j] + i11 * a2[4 + j]);
    }
    double nP[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double apa = ((A[i] * PA[j] + A[4 + i] * PA[4 + j]) + A[8 + i] * PA[8 + j]) + A[12 + i] * PA[12 + j];
            const double apb0 = ((A[i] * PB[0] + A[4 + i] * PB[2]) + A[8 + i] * PB[4]) + A[12 + i] * PB[6];
            const double apb1 = ((A[i] * PB[1] + A[4 + i] * PB[3]) + A[8 + i] * PB[5]) + A[12 + i] * PB[7];
            nP[4 * i + j] = (Q.v[4 * i + j] + apa) + (apb0 * K[j] + apb1 * K[4 + j]);
        }
#pragma unroll
    for (int k = 0; k < 16; ++k) P[k] = nP[k];
}

// stage s of a stage array (continuous Jacobians if disc: A_d = I + dt A_c, B_d = dt B_c, :161-164)
__device__ __forceinline__ void load_stage(const double* A, const double* Bm, int s, int S, const double* Ap,
                                           const double* Bp, int disc, double dt, double* Ad, double* Bd) {
    const double* a = s < S ? A + 16 * (int64_t)s : Ap;
    const double* b = s < S ? Bm + 8 * (int64_t)s : Bp;
#pragma unroll
    for (int k = 0; k < 16; ++k) Ad[k] = disc ? ((k % 5 == 0 ? 1.0 : 0.0) + dt * a[k]) : a[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) Bd[k] = disc ? dt * b[k] : b[k];
}

// window w: recursion over stages w + L-2 .. w (stage index >= S -> pad), terminal P = QT.
// all_gains: K_out (L-1, 2, 4) of window 0;  else K_out (nwin, 2, 4) = the first gain of every window.
__global__ __launch_bounds__(64) void k_tv_lqr_gains(const double* __restrict__ A, const double* __restrict__ Bm,
                                                     int S, const double* __restrict__ Ap,
                                                     const double* __restrict__ Bp, M44 Q, M22 R,
                                                     const double* __restrict__ QT, int L,
                                                     int nwin, int all_gains, int disc, double dt,
                                                     double* __restrict__ K_out) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwin) return;
    double P[16], K[8], Ad[16], Bd[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) P[k] = QT[k];
    for (int s = L - 2; s >= 0; --s) {
        load_stage(A, Bm, w + s, S, Ap, Bp, disc, dt, Ad, Bd);
        lqr_step(Ad, Bd, P, Q, R, K);
        if (all_gains) {
#pragma unroll
            for (int k = 0; k < 8; ++k) K_out[8 * (int64_t)s + k] = K[k];
        }
    }
    if (!all_gains) {
#pragma unroll
        for (int k = 0; k < 8; ++k) K_out[8 * (int64_t)w + k] = K[k];
    }
}

// compute_P_inf (:144-165): P <- Riccati map of (A, B, Q, R) from P = Q until max|dP| < tol.  One wavefront;
// lane 4i+j (< 16) owns P[i][j] and evaluates that entry of every product of the map (the same sums, in
// the same order, as one lane would), exchanging rows/columns through LDS: each iteration is a few
// dependent steps instead of ~400 dependent flops of a single lane.  max|dP| is a wave reduction.
__global__ __launch_bounds__(64) void k_dare_fixed_point(const double* __restrict__ A, const double* __restrict__ Bm,
                                                         M44 Q, M22 R, int max_iter, double tol,
                                                         double* __restrict__ P_out, int32_t* __restrict__ iters) {
    __shared__ double sP[16], sPA[16], sPB[8];
    const int ln = threadIdx.x, i = (ln >> 2) & 3, j = ln & 3;
    const bool own = ln < 16;
    double a[16], b[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = A[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = Bm[k];
    double P = Q.v[4 * i + j];
    int it = max_iter + 1;                 // max_iter + 1: the tolerance was never met
    for (int n = 0; n < max_iter; ++n) {
        if (own) sP[ln] = P;
        __syncthreads();
        const double* Pi = sP + 4 * i;   // row i of P
        const double PA = ((Pi[0] * a[j] + Pi[1] * a[4 + j]) + Pi[2] * a[8 + j]) + Pi[3] * a[12 + j];
        const double PB0 = ((Pi[0] * b[0] + Pi[1] * b[2]) + Pi[2] * b[4]) + Pi[3] * b[6];
        const double PB1 = ((Pi[0] * b[1] + Pi[1] * b[3]) + Pi[2] * b[5]) + Pi[3] * b[7];
        if (own) {
            sPA[ln] = PA;
            if (j == 0) { sPB[2 * i] = PB0; sPB[2 * i + 1] = PB1; }
        }
        __syncthreads();
        double a1[4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                a1[2 * r + c] = R.v[2 * r + c] + (((b[r] * sPB[c] + b[2 + r] * sPB[2 + c]) + b[4 + r] * sPB[4 + c]) +
                                                  b[6 + r] * sPB[6 + c]);
        const double a20 = ((b[0] * sPA[j] + b[2] * sPA[4 + j]) + b[4] * sPA[8 + j]) + b[6] * sPA[12 + j];
        const double a21 = ((b[1] * sPA[j] + b[3] * sPA[4 + j]) + b[5] * sPA[8 + j]) + b[7] * sPA[12 + j];
        const double idet = 1.0 / (a1[0] * a1[3] - a1[1] * a1[2]);
        const double i00 = a1[3] * idet, i01 = -a1[1] * idet, i10 = -a1[2] * idet, i11 = a1[0] * idet;
        const double K0 = -(i00 * a20 + i01 * a21), K1 = -(i10 * a20 + i11 * a21);
        const double apa = ((a[i] * sPA[j] + a[4 + i] * sPA[4 + j]) + a[8 + i] * sPA[8 + j]) + a[12 + i] * sPA[12 + j];
        const double apb0 = ((a[i] * sPB[0] + a[4 + i] * sPB[2]) + a[8 + i] * sPB[4]) + a[12 + i] * sPB[6];
        const double apb1 = ((a[i] * sPB[1] + a[4 + i] * sPB[3]) + a[8 + i] * sPB[5]) + a[12 + i] * sPB[7];
        const double nP = (Q.v[4 * i + j] + apa) + (apb0 * K0 + apb1 * K1);
        // np.max(np.abs(P_next - P)) < tol (:160-163) as a wave vote: every entry below tol (a NaN entry is not,
        // as np.max would return NaN); no cross-lane data movement on the iteration's critical path
        const bool conv = __all(!own || fabs(nP - P) < tol);
        P = nP;
        __syncthreads();   // every lane has read sP / sPA / sPB before the next iteration rewrites them
        if (conv) { it = n + 1; break; }
    }
    if (own) P_out[ln] = P;
    if (ln == 0) *iters = it;
}

// ------------------------------------------------------------------------------------------
// Fused MPC gains (solve_mpc_tracking :14-38 + the exact solution of every control step's QP): one launch.
//
// Every stage matrix the MPC uses is the acrobot's discretised linearisation (:18-23, the pad (A_f, B_f) :31-33),
// so it has a fixed structure: A_d rows 0,1 = [1,0,h,0], [0,1,0,h] (I + dt A_c with A_c rows e3', e4'),
// B_d = [0, b] with b = (0, 0, b2, b3)' (tau1 unactuated, dynamics.py:205).  The Riccati map
//   aux1 = R + B'PB, aux2 = B'PA, K = -inv(aux1) aux2, P <- Q + A'PA + (A'PB) K            (:158-160)
// then needs, per entry, only the terms those zeros leave (the skipped products are exact zeros / ones in the
// dense form; rounding of the rest is the reference's up to sum order, checked against the oracle at 1e-9).
//
// Lane-parallel map: a 16-lane group evaluates one map; lane 4i+j owns P[i][j] and the (i, j) entry of every
// product.  Row i of P comes from the lane's own quad (DPP quad broadcasts); rows 2, 3 and i&1 of PA and PB
// come from the group's other quads: the PB rows (uniform in a quad, on the gain's critical path) through
// row broadcasts (one v_mov_b64_dpp each), the PA rows through ds_swizzle (no LDS storage, no barrier).  A map is then ~35 fp64
// instructions per lane and a handful of exchanges on the critical path, instead of ~400 dependent flops of one
// lane (k_tv_lqr_gains) or three LDS round trips with barriers (k_dare_fixed_point).
// ------------------------------------------------------------------------------------------
struct StageLin {
    double a2[4], a3[4], b2, b3;   // rows 2, 3 of A_d; B_d[2][1], B_d[3][1]
};

// Calculate_A_B_matrixes + discretize_linearization (dynamics.py:217-226, trajectory_generation.py:161-164):
// A_d = I + dt A_c, B_d = dt B_c, with the same operations as load_stage() on k_point's Jacobians
__device__ __forceinline__ void disc_stage(const Dyn& m, double x0, double x1, double x2, double x3, double tau2,
                                           StageLin& s) {
    const gym::Jac J = gym::jacobian(m, x0, x1, x2, x3, tau2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s.a2[j] = (j == 2 ? 1.0 : 0.0) + m.h * J.a2[j];
        s.a3[j] = (j == 3 ? 1.0 : 0.0) + m.h * J.a3[j];
    }
    s.b2 = m.h * J.bc2;
    s.b3 = m.h * J.bc3;
}

using gym::dpp_d;
template <int N>   // v_mov_b64_dpp row_newbcast:N -- lane N of each 16-lane row to the whole row (gfx90a+ DPP64)
__device__ __forceinline__ double bcast_d(double v) {
    return __longlong_as_double(
        __builtin_amdgcn_update_dpp(0ll, __double_as_longlong(v), 0x150 + N, 0xF, 0xF, false));
}
template <int AND, int OR>   // ds_swizzle bit mode inside 32-lane halves: lane' = (lane & AND) | OR
__device__ __forceinline__ double swz_d(double v) {
    constexpr int pat = (AND & 31) | ((OR & 31) << 5);
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_swizzle((int)b, pat);
    const int hi = __builtin_amdgcn_ds_swizzle((int)(b >> 32), pat);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// per-lane constants of the map: lane 4i+j of its group
struct MapLane {
    bool hi;           // i & 1
    double c0j, c1j;   // A_d[0][j], A_d[1][j]
    double ci;         // A_d[0][i] + A_d[1][i] (exactly one of the two is nonzero): 1, 1, h, h
    double Qij, R00, R01, R10, R11;
};
__device__ __forceinline__ MapLane map_lane(int i, int j, double h, const M44& Q, const M22& R) {
    MapLane c;
    c.hi = i & 1;
    c.c0j = j == 0 ? 1.0 : (j == 2 ? h : 0.0);
    c.c1j = j == 1 ? 1.0 : (j == 3 ? h : 0.0);
    c.ci = i < 2 ? 1.0 : h;
    c.Qij = Q.v[4 * i + j];
    c.R00 = R.v[0]; c.R01 = R.v[1]; c.R10 = R.v[2]; c.R11 = R.v[3];
    return c;
}

// One Riccati map on the structured stage (a2j = A_d[2][j], a3j = A_d[3][j], a2i = A_d[2][i], a3i = A_d[3][i]);
// returns P_next[i][j] and this lane's column j of the gain K (K0j, K1j).
__device__ __forceinline__ double riccati_map_lane(double P, const MapLane& c, double a2j, double a3j, double a2i,
                                                   double a3i, double b2, double b3, double& K0j, double& K1j) {
#pragma clang fp contract(on)
    // the gain's critical path is P -> PB -> aux1 -> 1/det -> K: PB and its exchanges are issued first
    const double P2 = dpp_d<0xAA>(P), P3 = dpp_d<0xFF>(P);                    // P[i][2], P[i][3]
    const double PB = P2 * b2 + P3 * b3;                                      // (PB)[i][1]; (PB)[i][0] = 0
    const double PB2 = bcast_d<8>(PB), PB3 = bcast_d<12>(PB);                 // (PB)[2][1], (PB)[3][1]
    const double P0 = dpp_d<0x00>(P), P1 = dpp_d<0x55>(P);
    const double PA = ((P0 * c.c0j + P1 * c.c1j) + P2 * a2j) + P3 * a3j;     // (PA)[i][j]
    const double a1 = c.R11 + (b2 * PB2 + b3 * PB3);                           // aux1[1][1]; aux1[0][*] = R[0][*]
    const double idet = gym::recip(c.R00 * a1 - c.R01 * c.R10);              // rcp + 2 Newton steps
    const double PA2 = swz_d<0x13, 0x08>(PA), PA3 = swz_d<0x13, 0x0C>(PA), PAh = swz_d<0x17, 0x00>(PA);
    const double B0 = bcast_d<0>(PB), B4 = bcast_d<4>(PB);
    const double PBh = c.hi ? B4 : B0;                                        // (PB)[i&1][1]
    const double a2 = b2 * PA2 + b3 * PA3;                                    // aux2[1][j]; aux2[0][j] = 0
    K0j = -((-c.R01 * idet) * a2);                                            // -(inv(aux1) aux2)[0][j]
    K1j = -((c.R00 * idet) * a2);                                             // -(inv(aux1) aux2)[1][j]
    const double APA = (c.ci * PAh + a2i * PA2) + a3i * PA3;                  // (A'PA)[i][j]
    const double APB = (c.ci * PBh + a2i * PB2) + a3i * PB3;                  // (A'PB)[i][1]; [i][0] = 0
    return (c.Qij + APA) + APB * K1j;
}

constexpr int kMpcMaxStages = 256;   // LDS stage table of one workgroup: its 4 windows' stages (L + 2 <= 256)

// ------------------------------------------------------------------------------------------
// compute_P_inf (:144-165) with doubling jumps.  The reference iterates the Riccati map F from P_0 = Q and stops at
// the first n with max|P_{n+1} - P_n| < tol, returning P_{n+1}.  The structure-preserving doubling algorithm
//   A_0 = A, G_0 = B R^-1 B', H_0 = Q;  W = (I + G_k H_k)^-1,
//   A_{k+1} = A_k W A_k,   G_{k+1} = G_k + A_k W G_k A_k',   H_{k+1} = H_k + A_k' H_k W A_k
// gives H_k = F^(2^k)(0) = P_{2^k - 1}, the reference's own iterate (up to rounding), in k steps.  k_mpc_gains jumps
// with it while the map still moves H_k by >= tol (the reference has not stopped there yet) and then runs the
// reference's loop, with its own test, from the last such H_k: the same stop iterate as the reference, ~2^(k-1)
// maps instead of ~2^k (the cfg 5 pad: 434 maps -> 9 doublings + 179 maps).  Doubling all the way to the limit
// (round 5) overshoots the reference's stop by ~tol rho^2 / (1 - rho^2) absolute, which is invisible at the cfg 5
// pad's scale (P ~ 2e7) but not for smaller Q / R.
// On a 16-lane group as the Riccati map below: lane 4i+j owns entry (i, j) of every 4x4 matrix; each product is one
// round through a per-group LDS scratch (one wavefront: its LDS accesses are in order, so no barrier), W by
// Gauss-Jordan elimination with partial pivoting (every lane finds the same pivot row).  Every group of every
// workgroup computes the same bits.
// ------------------------------------------------------------------------------------------
constexpr int kSdaMaxSteps = 30;   // 2^30 - 1 maps: beyond any max_iter an int holds

__device__ __forceinline__ void wave_lds_order() {   // LDS writes of this wavefront visible to its later reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// (X Y)[i][j], (X Y')[i][j], (X' Y)[i][j] from 16-double LDS matrices (row-major)
__device__ __forceinline__ double dot_xy(const double* X, const double* Y, int i, int j) {
    return ((X[4 * i] * Y[j] + X[4 * i + 1] * Y[4 + j]) + X[4 * i + 2] * Y[8 + j]) + X[4 * i + 3] * Y[12 + j];
}
__device__ __forceinline__ double dot_xyt(const double* X, const double* Y, int i, int j) {
    return ((X[4 * i] * Y[4 * j] + X[4 * i + 1] * Y[4 * j + 1]) + X[4 * i + 2] * Y[4 * j + 2]) + X[4 * i + 3] * Y[4 * j + 3];
}
__device__ __forceinline__ double dot_xty(const double* X, const double* Y, int i, int j) {
    return ((X[i] * Y[j] + X[4 + i] * Y[4 + j]) + X[8 + i] * Y[8 + j]) + X[12 + i] * Y[12 + j];
}

// The doubling's initial triple on the pad (lane 4i+j: entry (i, j) of A_0, G_0, H_0)
__device__ __forceinline__ void sda16_init(double h, const StageLin& pad, const M44& Q, const M22& R, int i, int j,
                                           double& a, double& g, double& hh) {
    // A_f: rows 0, 1 = [1 0 h 0], [0 1 0 h]; rows 2, 3 the StageLin's.  G_0 = (R^-1)[1][1] b b', b = (0, 0, b2, b3)'
    a = i == 0 ? (j == 0 ? 1.0 : (j == 2 ? h : 0.0)) : i == 1 ? (j == 1 ? 1.0 : (j == 3 ? h : 0.0))
                                                   : (i == 2 ? pad.a2[j] : pad.a3[j]);
    const double r11 = R.v[0] / (R.v[0] * R.v[3] - R.v[1] * R.v[2]);
    const double bi = i == 2 ? pad.b2 : (i == 3 ? pad.b3 : 0.0), bj = j == 2 ? pad.b2 : (j == 3 ? pad.b3 : 0.0);
    g = r11 * bi * bj;
    hh = Q.v[4 * i + j];
}

// One doubling step of (a, g, hh) in place; sm = this group's 8 x 16 doubles of LDS.  Returns false (for every lane of
// the wavefront) on a zero / non-finite pivot or a non-finite H.  Every lane of the wavefront must call it.
__device__ bool sda16_step(int i, int j, double* sm, double& a, double& g, double& hh) {
    double* sA = sm;        double* sG = sm + 16;  double* sH = sm + 32;  double* sM = sm + 48;
    double* sV = sm + 64;   double* sW = sm + 80;  double* sT = sm + 96;  double* sU = sm + 112;
    const int l = 4 * i + j;
    wave_lds_order();                                               // reads of the previous step before these writes
    sA[l] = a; sG[l] = g; sH[l] = hh;
    wave_lds_order();
    double m = dot_xy(sG, sH, i, j) + (i == j ? 1.0 : 0.0);        // I + G H
    double v = i == j ? 1.0 : 0.0;                                  // its inverse, built alongside
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        wave_lds_order();                                           // earlier reads of sM / sV are done
        sM[l] = m; sV[l] = v;
        wave_lds_order();
        int p = c;                                                  // the largest |M[r][c]|, r >= c
        double best = fabs(sM[4 * c + c]);
#pragma unroll
        for (int r = c + 1; r < 4; ++r) {
            const double t = fabs(sM[4 * r + c]);
            p = t > best ? r : p;
            best = t > best ? t : best;
        }
        const int row = i == c ? p : (i == p ? c : i);            // this lane's row after swapping rows c, p
        const double piv = sM[4 * p + c];
        ok &= (piv != 0.0) & (fabs(piv) <= 1.7976931348623157e308);
        const double ip = 1.0 / piv;
        const double mm = sM[4 * row + j], vv = sV[4 * row + j];
        const double f = sM[4 * row + c];
        const double mc = sM[4 * p + j] * ip, vc = sV[4 * p + j] * ip;
        m = i == c ? mc : fma(-f, mc, mm);
        v = i == c ? vc : fma(-f, vc, vv);
    }
    wave_lds_order();
    sW[l] = v;
    wave_lds_order();
    const double wa = dot_xy(sW, sA, i, j), wg = dot_xy(sW, sG, i, j);
    sM[l] = wa; sV[l] = wg;                                         // W A, W G
    wave_lds_order();
    const double awg = dot_xy(sA, sV, i, j), hwa = dot_xy(sH, sM, i, j), awa = dot_xy(sA, sM, i, j);
    sT[l] = awg; sU[l] = hwa;
    wave_lds_order();
    const double gn = g + dot_xyt(sT, sA, i, j);                   // G + A W G A'
    const double hn = hh + dot_xty(sA, sU, i, j);                  // H + A' H W A
    const bool bad = !ok || !(fabs(hn) <= 1.7976931348623157e308);
    a = awa; g = gn; hh = hn;
    return !__any(bad);
}

// Workgroup = 4 windows (16 lanes each).  1) every stage the 4 windows use, discretised, into LDS (one lane per
// stage), and the pad (A_f, B_f) at x_f, u_f;  2) compute_P_inf (:144-165) on the pad (doubling jumps, then the
// reference's loop to its stop iterate), in every workgroup (the same bits everywhere: no grid-wide dependency);  3) each window's recursion from P = P_inf over stages
// w+L-2 .. w;  its first gain is the QP's solution u0 = K x0 at control step w.
// ALL: K_out (nwin, L-1, 2, 4) holds every stage's gain of every window (the shared first iterate of the torque-
// limited QP, k_mpc_box_rollout); else K_out (nwin, 2, 4), each window's first gain.  Same recursion, same bits.
template <bool ALL>
__global__ __launch_bounds__(64) void k_mpc_gains(Dyn m, const double* __restrict__ x_ref,
                                                  const double* __restrict__ u_ref, int S,
                                                  const double* __restrict__ xf, const double* __restrict__ uf,
                                                  M44 Q, M22 R, int L, int nwin, int max_iter, double tol,
                                                  double* __restrict__ K_out, double* __restrict__ QT_out,
                                                  int32_t* __restrict__ iters_out) {
    __shared__ StageLin st[kMpcMaxStages];
    __shared__ StageLin pad;
    const int ln = threadIdx.x, g = ln >> 4, i = (ln >> 2) & 3, j = ln & 3;
    const int w0 = blockIdx.x * 4;
    const int nst = min(3 + L - 1, kMpcMaxStages);      // local stages 0 .. 3 + L - 2
    if (ln == 0) disc_stage(m, xf[0], xf[1], xf[2], xf[3], uf[1], pad);
    for (int s = ln; s < nst; s += 64) {
        const int gs = w0 + s;
        if (gs < S) {
            disc_stage(m, x_ref[4 * (int64_t)gs], x_ref[4 * (int64_t)gs + 1], x_ref[4 * (int64_t)gs + 2],
                       x_ref[4 * (int64_t)gs + 3], u_ref[2 * (int64_t)gs + 1], st[s]);
        }
    }
    __syncthreads();
    // compute_P_inf (:144-165) on the pad stage, the same bits in every group: doubling jumps while the map still
    // moves the iterate by >= tol, then the reference's loop and test from the last such iterate (see sda16_step)
    __shared__ double sm[4][128];
    const MapLane c = map_lane(i, j, m.h, Q, R);
    const double fa2j = pad.a2[j], fa3j = pad.a3[j], fa2i = pad.a2[i], fa3i = pad.a3[i], fb2 = pad.b2, fb3 = pad.b3;
    double P, K0j, K1j;
    double Pst = c.Qij;                                   // P_{n0}: the loop below resumes from it
    int n0 = 0;
    {
        double da, dg, dh;
        sda16_init(m.h, pad, Q, R, i, j, da, dg, dh);
        for (int s = 1; s <= kSdaMaxSteps; ++s) {
            if (!sda16_step(i, j, sm[g], da, dg, dh)) break;      // (not a stabilisable pad: the loop from P_{n0})
            const int idx = (1 << s) - 1;                          // dh = P_idx
            if (idx >= max_iter) break;                            // the reference never gets past max_iter maps
            const double nP = riccati_map_lane(dh, c, fa2j, fa3j, fa2i, fa3i, fb2, fb3, K0j, K1j);
            if (__all(fabs(nP - dh) < tol)) break;                 // the reference stops at or before map idx + 1
            Pst = dh;
            n0 = idx;
        }
    }
    P = Pst;
    int it = max_iter + 1;                                // the reference's count; max_iter + 1: never converged
    for (int n = n0; n < max_iter; ++n) {
        const double nP = riccati_map_lane(P, c, fa2j, fa3j, fa2i, fa3i, fb2, fb3, K0j, K1j);
        const bool conv = __all(fabs(nP - P) < tol);      // np.abs(P - P_prev).max() < tol (a NaN entry fails)
        P = nP;
        if (conv) { it = n + 1; break; }
    }
    if (blockIdx.x == 0 && ln < 16) {
        QT_out[ln] = P;
        if (ln == 0) *iters_out = it;
    }
    // window w0 + g: stages w + L - 2 .. w (local g + L - 2 .. g), pad past S
    const int w = w0 + g;
    for (int s = L - 2; s >= 0; --s) {
        const StageLin* q = (w + s < S) ? &st[g + s] : &pad;
        P = riccati_map_lane(P, c, q->a2[j], q->a3[j], q->a2[i], q->a3[i], q->b2, q->b3, K0j, K1j);
        if constexpr (ALL) {
            if (w < nwin && i == 0) {
                double* ks = K_out + 8 * ((int64_t)w * (L - 1) + s);
                ks[j] = K0j;
                ks[4 + j] = K1j;
            }
        }
    }
    if constexpr (!ALL) {
        if (w < nwin && i == 0) {
            K_out[8 * (int64_t)w + j] = K0j;
            K_out[8 * (int64_t)w + 4 + j] = K1j;
        }
    }
}

// LQ forward pass of one window (solver_mpc's X_opt, U_opt): x_{s+1} = A_s x_s + B_s u_s, u_s = K_s x_s
__global__ void k_lq_forward(const double* __restrict__ A, const double* __restrict__ Bm, int S,
                             const double* __restrict__ Ap, const double* __restrict__ Bp, int disc, double dt,
                             const double* __restrict__ K, const double* __restrict__ x0, int L,
                             double* __restrict__ X, double* __restrict__ U) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double x[4] = {x0[0], x0[1], x0[2], x0[3]}, Ad[16], Bd[8];
    for (int s = 0; s < L - 1; ++s) {
        const double* k = K + 8 * s;
        const double u0 = ((k[0] * x[0] + k[1] * x[1]) + k[2] * x[2]) + k[3] * x[3];
        const double u1 = ((k[4] * x[0] + k[5] * x[1]) + k[6] * x[2]) + k[7] * x[3];
        X[4 * s] = x[0]; X[4 * s + 1] = x[1]; X[4 * s + 2] = x[2]; X[4 * s + 3] = x[3];
        U[2 * s] = u0; U[2 * s + 1] = u1;
        load_stage(A, Bm, s, S, Ap, Bp, disc, dt, Ad, Bd);
        double n[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            n[i] = (((Ad[4 * i] * x[0] + Ad[4 * i + 1] * x[1]) + Ad[4 * i + 2] * x[2]) + Ad[4 * i + 3] * x[3]) +
                   (Bd[2 * i] * u0 + Bd[2 * i + 1] * u1);
        x[0] = n[0]; x[1] = n[1]; x[2] = n[2]; x[3] = n[3];
    }
    X[4 * (L - 1)] = x[0]; X[4 * (L - 1) + 1] = x[1]; X[4 * (L - 1) + 2] = x[2]; X[4 * (L - 1) + 3] = x[3];
}

// The tracking feedback u = u_ff + K (x - x_ff) (simulate_tracking :210, the MPC loop's u = K x0 + u_ref :50) with
// FMA contraction inside the expression only: the frontend then fuses the same product of every sum in every kernel
// and code context.  Under the file's default -ffp-contract=fast the backend chose per context: a pair rollout
// unrolled by two with double-buffered rows (round 3) fused k1 d1 instead of k0 d0 in its second step and lost
// bitwise equality with the single-lane kernel (tools/mpc_rowbuf_probe.py, profiles/r04/mpc_rowbuf/).
__device__ __forceinline__ void track_feedback(const double* k, const double* f, double d0, double d1, double d2,
                                               double d3, double& v0, double& v1) {
#pragma clang fp contract(on)
    v0 = f[0] + (((k[0] * d0 + k[1] * d1) + k[2] * d2) + k[3] * d3);
    v1 = f[1] + (((k[4] * d0 + k[5] * d1) + k[6] * d2) + k[7] * d3);
}

// Batched closed-loop tracking simulation (simulate_tracking :206-216; MPC loop :43-60):
//   u_t = u_ff[t] + K[t] (x_t - x_ff[t]),  x_{t+1} = RK4(x_t, u_t)
// x0 (B,4); shared x_ff (N,4), u_ff (T,2), K (T,2,4); outputs lane-major x (B,N,4), u (B,T,2).  Each lane is a
// chain of T dependent RK4 steps (B/64 wavefronts: latency-bound), so the step's shared operands are loaded
// one step ahead (wave-uniform, scalar) and the lane writes its own rows directly: consecutive steps fill
// its 128-B lines in L2, no transpose pass afterwards.
__global__ __launch_bounds__(64) void k_track_rollout(Dyn m, const double* __restrict__ x0,
                                                      const double* __restrict__ x_ff, const double* __restrict__ u_ff,
                                                      const double* __restrict__ K, int64_t B, int N,
                                                      double* __restrict__ xo, double* __restrict__ uo) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= B) return;
    const int T = N - 1;
    double2* xl = reinterpret_cast<double2*>(xo + 4 * (int64_t)N * l);
    double2* ul = reinterpret_cast<double2*>(uo + 2 * (int64_t)T * l);
    double n0 = x0[4 * l], n1 = x0[4 * l + 1], n2 = x0[4 * l + 2], n3 = x0[4 * l + 3];
    xl[0] = make_double2(n0, n1);
    xl[1] = make_double2(n2, n3);
    double k[8], r[4], f[2];
#pragma unroll
    for (int q = 0; q < 8; ++q) k[q] = K[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = x_ff[q];
    f[0] = u_ff[0]; f[1] = u_ff[1];
    const gym::PolyRegs pk = gym::poly_vgprs();   // minimax coefficients held in VGPRs (acrobot_device.hpp)
    for (int t = 0; t < T; ++t) {
        const double d0 = n0 - r[0], d1 = n1 - r[1], d2 = n2 - r[2], d3 = n3 - r[3];
        double v0, v1;
        track_feedback(k, f, d0, d1, d2, d3, v0, v1);
        if (t + 1 < T) {   // next step's shared operands, in flight during this step's RK4
            const double* kn = K + 8 * (t + 1);
#pragma unroll
            for (int q = 0; q < 8; ++q) k[q] = kn[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = x_ff[4 * (t + 1) + q];
            f[0] = u_ff[2 * (t + 1)]; f[1] = u_ff[2 * (t + 1) + 1];
        }
        ul[t] = make_double2(v0, v1);
        gym::rk4(m, n0, n1, n2, n3, v1, pk);
        xl[2 * (t + 1)] = make_double2(n0, n1);
        xl[2 * (t + 1) + 1] = make_double2(n2, n3);
    }
}

// 16-B non-temporal store: the trajectories are written once and not read back by this kernel.  The per-step
// stores land in rows 16 KB apart (the reference's lane-major arrays); streamed past the caches they cost the
// latency-bound rollout less (cfg 5: 426 -> 412 us, tools/rollout_probe.py; staging the steps in LDS to write
// whole-trajectory runs was slower, 458 us: LDS traffic shares lgkmcnt with the per-step scalar loads)
__device__ __forceinline__ void st_nt2(double2* p, double a, double b) {
    typedef double d2v __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(d2v{a, b}, reinterpret_cast<d2v*>(p));
}

// k_track_rollout with each trajectory on a lane pair (gym::rk4_pair): 2B threads, 128 B... of one lane's rows
// split between the pair (even lane: (th1, th2) and u; odd lane: (w1, w2)).  The chain of 500 dependent RK4 steps
// is the whole cost of this latency-bound kernel (B/32 wavefronts, one per SIMD), and the split shortens each
// step's instruction stream by ~1/3.  Bit-identical to k_track_rollout (tested).
__global__ __launch_bounds__(64) void k_track_rollout_pair(Dyn m, const double* __restrict__ x0,
                                                           const double* __restrict__ x_ff,
                                                           const double* __restrict__ u_ff,
                                                           const double* __restrict__ K, int64_t B, int N,
                                                           double* __restrict__ xo, double* __restrict__ uo) {
    const int64_t th = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t l = th >> 1;
    const bool odd = th & 1;
    if (l >= B) return;                    // both lanes of a pair, so the pair's DPP partners are always active
    const int T = N - 1;
    double2* xl = reinterpret_cast<double2*>(xo + 4 * (int64_t)N * l) + (odd ? 1 : 0);
    double2* ul = reinterpret_cast<double2*>(uo + 2 * (int64_t)T * l);
    double n0 = x0[4 * l], n1 = x0[4 * l + 1], n2 = x0[4 * l + 2], n3 = x0[4 * l + 3];
    xl[0] = odd ? make_double2(n2, n3) : make_double2(n0, n1);
    double k[8], r[4], f[2];
#pragma unroll
    for (int q = 0; q < 8; ++q) k[q] = K[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = x_ff[q];
    f[0] = u_ff[0]; f[1] = u_ff[1];
    const gym::PolyRegs pk = gym::poly_vgprs_all();   // every Horner coefficient in VGPRs
    Dyn dm = m;                            // the model in VGPRs across the step loop
    gym::in_vgpr(dm.b); gym::in_vgpr(dm.d); gym::in_vgpr(dm.a2b); gym::in_vgpr(dm.bb); gym::in_vgpr(dm.dad);
    gym::in_vgpr(dm.g1); gym::in_vgpr(dm.g2); gym::in_vgpr(dm.f1); gym::in_vgpr(dm.f2); gym::in_vgpr(dm.h);
    gym::in_vgpr(dm.h2); gym::in_vgpr(dm.h6);
    for (int t = 0; t < T; ++t) {
        const double d0 = n0 - r[0], d1 = n1 - r[1], d2 = n2 - r[2], d3 = n3 - r[3];
        double v0, v1;
        track_feedback(k, f, d0, d1, d2, d3, v0, v1);
        if (t + 1 < T) {
            const double* kn = K + 8 * (t + 1);
#pragma unroll
            for (int q = 0; q < 8; ++q) k[q] = kn[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = x_ff[4 * (t + 1) + q];
            f[0] = u_ff[2 * (t + 1)]; f[1] = u_ff[2 * (t + 1) + 1];
        }
        if (!odd) st_nt2(ul + t, v0, v1);
        gym::rk4_pair_fast(dm, odd, n0, n1, n2, n3, v1, pk);   // branch-free near path (gym::rk4_pair_fast)
        if (odd) st_nt2(xl + 2 * (t + 1), n2, n3);
        else st_nt2(xl + 2 * (t + 1), n0, n1);
    }
}

// ------------------------------------------------------------------------------------------
// Torque-limited MPC (solver_mpc with test_constraints on, :87-114): every stage of the window obeys
//   -tau_max <= u_t + u_ref_t <= tau_max.
// B_d's column 0 is zero (tau1 unactuated), so channel 0 separates (u_t[0] = clip(0, lo, hi)) and channel 1 is a
// scalar-input LQ problem with a box, b = B_t[:, 1], r = R[1][1].  One lane solves one QP with a primal-dual
// active set over a clamped Riccati sweep (each stage free, at hi or at lo; all free at the start):
//   backward   P = Q_T, p = 0;  free: g = r + b'Pb, k = -(b'PA)/g, d = -(b'p)/g;  clamped: k = 0, d = the bound;
//              Acl = A + b k,  p <- r k'd + Acl'(P b d + p),  P <- Q + r k'k + Acl' P Acl
//   forward    u_t = k_t x_t + d_t,  x_{t+1} = A_t x_t + b u_t
//   costate    lam = 2 Q_T x_{L-1};  q_t = 2 r u_t + b'lam,  lam <- 2 Q x_t + A_t'lam  (the reduced-cost gradient)
//   update     free and u_t > hi -> hi, < lo -> lo;  at hi stays while q_t < 0, at lo while q_t > 0, else free
// until no stage changes (u is then the exact minimiser) or the sweep count reaches max_it (unconverged: clip(u, lo,
// hi) of the last iterate, flagged; so a QP is unconverged exactly when its count is max_it -- a last sweep that
// happens to settle is still flagged, and its clipped iterate is then the minimiser itself).  Iteration 1 has every stage free, so its gains do not depend on the lane: with Kw
// (k_mpc_gains<true>'s table of the window) it is one linear forward pass and no per-lane Riccati sweep.
//
// Shared operands: the window's stage rows and Kw sit in the workgroup's LDS (one wavefront per workgroup), read at
// wave-uniform addresses (broadcast).  Every sweep stage needs ~26 shared doubles; as scalar loads from the global
// table each stage waited a full L2 round trip with nothing to overlap it (one wavefront per CU), 4x the stage's
// arithmetic (tools/mpc_box_probe.py, profiles/mpc_box/).  The closed loop keeps the rows in a ring: the window
// slides by one stage per control step, so a step loads one new row and the window's Kw.  The per-lane sweep data, a
// few KB per lane, lives in a caller-allocated workspace in lane-fastest layout (slot, stage, lane), so a wavefront's
// accesses to one stage coalesce.
// ------------------------------------------------------------------------------------------
constexpr int kBoxRow = 22;   // one stage row: A_d (16), b = B_d[:, 1] (4), u_ref (2)
struct BoxTable {             // global stage table: stage t of window `first` reads row min(first + t, last)
    const double* A;          // A_d (rows, 4, 4)
    const double* Bm;         // B_d (rows, 4, 2)
    const double* ur;         // u_ref (rows, 2)
    int last;
};
struct BoxWin {
    const double* rows;       // LDS: stage t at rows + kBoxRow slot(t)
    const double* Kw;         // LDS: row 1 of the window's unconstrained gains, 4 per stage; or null
    int base, Lm;             // ring: slot(t) = (base + t) mod Lm
    __device__ __forceinline__ const double* row(int t) const {
        const int i = base + t;
        return rows + kBoxRow * (i >= Lm ? i - Lm : i);
    }
};
// element e of global stage row r (clamped to the table's last row) in the LDS row format
__device__ __forceinline__ double box_row_elem(const BoxTable& tb, int r, int e) {
    const int64_t row = min(r, tb.last);
    return e < 16 ? tb.A[16 * row + e] : (e < 20 ? tb.Bm[8 * row + 2 * (e - 16) + 1] : tb.ur[2 * row + (e - 20)]);
}
struct BoxWs {
    double* d;          // slots 0-3 k, 4 d, 5-8 x, 9 u of stage t at ((10 t + slot) Bp + lane); x_{L-1} after them
    int32_t* st;        // stage state (0 free, 1 at hi, -1 at lo) at (t Bp + lane)
    int64_t Bp, lane;
    __device__ __forceinline__ double& at(int t, int slot) const { return d[(10 * (int64_t)t + slot) * Bp + lane]; }
    __device__ __forceinline__ int32_t& state(int t) const { return st[(int64_t)t * Bp + lane]; }
};
constexpr int kBoxSlots = 10;

__device__ __forceinline__ double box_gain_dot(const double* k, double x0, double x1, double x2, double x3) {
#pragma clang fp contract(on)   // the chain of track_feedback(): the same bits as the unconstrained rollout
    return ((k[0] * x0 + k[1] * x1) + k[2] * x2) + k[3] * x3;
}

// clamped Riccati sweep of the lane's current stage states -> (k, d) of every stage in the workspace
__device__ __forceinline__ void box_backward(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                             double tau, const BoxWs& ws, bool all_free) {
    double P[16], p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 16; ++q) P[q] = QT[q];
    // the lane's workspace reads of a sweep do not depend on its arithmetic: each is issued one stage ahead, so the
    // stage's own work covers the memory latency (one wavefront per CU: nothing else would)
    int sn = all_free ? 0 : ws.state(Lm - 1);
    for (int t = Lm - 1; t >= 0; --t) {
        const double* A = w.row(t);
        const double b[4] = {A[16], A[17], A[18], A[19]};
        const int s = sn;
        sn = all_free ? 0 : ws.state(t > 0 ? t - 1 : 0);
        double Pb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) Pb[i] = ((P[4 * i] * b[0] + P[4 * i + 1] * b[1]) + P[4 * i + 2] * b[2]) + P[4 * i + 3] * b[3];
        const double g = r + (((Pb[0] * b[0] + Pb[1] * b[1]) + Pb[2] * b[2]) + Pb[3] * b[3]);
        const double ig = 1.0 / g;
        double k[4], d;
        if (s == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                k[j] = -((((Pb[0] * A[j] + Pb[1] * A[4 + j]) + Pb[2] * A[8 + j]) + Pb[3] * A[12 + j]) * ig);
            d = -((((p[0] * b[0] + p[1] * b[1]) + p[2] * b[2]) + p[3] * b[3]) * ig);
        } else {
            k[0] = k[1] = k[2] = k[3] = 0.0;
            d = (s > 0 ? tau : -tau) - A[21];
        }
        double Acl[16], v[4], pn[4], M[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) Acl[4 * i + j] = A[4 * i + j] + b[i] * k[j];
            v[i] = Pb[i] * d + p[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pn[i] = (r * k[i]) * d + (((Acl[i] * v[0] + Acl[4 + i] * v[1]) + Acl[8 + i] * v[2]) + Acl[12 + i] * v[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                M[4 * i + j] = ((P[4 * i] * Acl[j] + P[4 * i + 1] * Acl[4 + j]) + P[4 * i + 2] * Acl[8 + j]) + P[4 * i + 3] * Acl[12 + j];
        }
        double Pn[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                Pn[4 * i + j] = (Q.v[4 * i + j] + (r * k[i]) * k[j]) +
                                (((Acl[i] * M[j] + Acl[4 + i] * M[4 + j]) + Acl[8 + i] * M[8 + j]) + Acl[12 + i] * M[12 + j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = pn[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) P[4 * i + j] = 0.5 * (Pn[4 * i + j] + Pn[4 * j + i]);   // P stays symmetric
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ws.at(t, j) = k[j];
        ws.at(t, 4) = d;
    }
}

// forward pass from e; STORE: x_t, u_t of every stage and x_{L-1} go to the workspace.  shared: the window's
// unconstrained gains (every stage free, d = 0).  Returns whether a free stage's u_t lies outside its bounds.
template <bool STORE>
__device__ __forceinline__ bool box_forward(const BoxWin& w, int Lm, const BoxWs& ws, bool shared, bool all_free,
                                            double tau, double x0, double x1, double x2, double x3, double& u_first) {
    bool viol = false;
    double kn[4] = {0.0, 0.0, 0.0, 0.0}, dn = 0.0;
    int sn = 0;
    if (!shared) {                                       // (k, d, state) one stage ahead, as in box_backward
#pragma unroll
        for (int q = 0; q < 4; ++q) kn[q] = ws.at(0, q);
        dn = ws.at(0, 4);
        sn = all_free ? 0 : ws.state(0);
    }
    for (int t = 0; t < Lm; ++t) {
        const double* A = w.row(t);
        double u;
        if (shared) {
            u = box_gain_dot(w.Kw + 4 * t, x0, x1, x2, x3);
            viol |= (u > tau - A[21]) | (u < -tau - A[21]);
        } else {
            const int s = sn;
            const double k[4] = {kn[0], kn[1], kn[2], kn[3]};
            const double d = dn;
            const int tn = t + 1 < Lm ? t + 1 : t;
#pragma unroll
            for (int q = 0; q < 4; ++q) kn[q] = ws.at(tn, q);
            dn = ws.at(tn, 4);
            sn = all_free ? 0 : ws.state(tn);
            u = s == 0 ? box_gain_dot(k, x0, x1, x2, x3) + d : d;
            viol |= (s == 0) & ((u > tau - A[21]) | (u < -tau - A[21]));
        }
        if (t == 0) u_first = u;
        if constexpr (STORE) {
            ws.at(t, 5) = x0; ws.at(t, 6) = x1; ws.at(t, 7) = x2; ws.at(t, 8) = x3;
            ws.at(t, 9) = u;
        }
        const double n0 = (((A[0] * x0 + A[1] * x1) + A[2] * x2) + A[3] * x3) + A[16] * u;
        const double n1 = (((A[4] * x0 + A[5] * x1) + A[6] * x2) + A[7] * x3) + A[17] * u;
        const double n2 = (((A[8] * x0 + A[9] * x1) + A[10] * x2) + A[11] * x3) + A[18] * u;
        const double n3 = (((A[12] * x0 + A[13] * x1) + A[14] * x2) + A[15] * x3) + A[19] * u;
        x0 = n0; x1 = n1; x2 = n2; x3 = n3;
    }
    if constexpr (STORE) { ws.at(Lm, 0) = x0; ws.at(Lm, 1) = x1; ws.at(Lm, 2) = x2; ws.at(Lm, 3) = x3; }
    return viol;
}

// costate pass over the stored (x, u) and the stage-state update; returns whether any stage changed
__device__ __forceinline__ bool box_update(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                           double tau, const BoxWs& ws, bool all_free) {
    double lam[4];
    {
        const double x[4] = {ws.at(Lm, 0), ws.at(Lm, 1), ws.at(Lm, 2), ws.at(Lm, 3)};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            lam[i] = 2.0 * (((QT[4 * i] * x[0] + QT[4 * i + 1] * x[1]) + QT[4 * i + 2] * x[2]) + QT[4 * i + 3] * x[3]);
    }
    bool changed = false;
    double un = ws.at(Lm - 1, 9), xn[4] = {ws.at(Lm - 1, 5), ws.at(Lm - 1, 6), ws.at(Lm - 1, 7), ws.at(Lm - 1, 8)};
    int sn = all_free ? 0 : ws.state(Lm - 1);               // (x, u, state) one stage ahead, as in box_backward
    for (int t = Lm - 1; t >= 0; --t) {
        const double* A = w.row(t);
        const double f = A[21];
        const double hi = tau - f, lo = -tau - f;
        const double u = un;
        const double x[4] = {xn[0], xn[1], xn[2], xn[3]};
        const int s = sn;
        const int tn = t > 0 ? t - 1 : 0;
        un = ws.at(tn, 9);
#pragma unroll
        for (int q = 0; q < 4; ++q) xn[q] = ws.at(tn, 5 + q);
        sn = all_free ? 0 : ws.state(tn);
        const double q = 2.0 * r * u + (((lam[0] * A[16] + lam[1] * A[17]) + lam[2] * A[18]) + lam[3] * A[19]);
        const int ns = s == 0 ? (u > hi ? 1 : (u < lo ? -1 : 0)) : (s > 0 ? (q < 0.0 ? 1 : 0) : (q > 0.0 ? -1 : 0));
        changed |= ns != s;
        ws.state(t) = ns;
        double nl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            nl[i] = 2.0 * (((Q.v[4 * i] * x[0] + Q.v[4 * i + 1] * x[1]) + Q.v[4 * i + 2] * x[2]) + Q.v[4 * i + 3] * x[3]) +
                    (((A[i] * lam[0] + A[4 + i] * lam[1]) + A[8 + i] * lam[2]) + A[12 + i] * lam[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) lam[i] = nl[i];
    }
    return changed;
}

// One lane's QP from e = x0; u_first = u_0 of channel 1.  WS_RESULT: (x_t, u_t) of the result are always left in the
// workspace (the batch kernel's outputs); without it a first iterate (shared gains) that violates no bound -- the
// exact minimiser: no free stage changes state -- ends the QP after a forward pass that stores nothing.
// The loop runs until every lane of the wavefront is done; lanes that are done (or not valid) sit out.
template <bool WS_RESULT>
__device__ __forceinline__ void box_qp_lane(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                            double tau, int max_it, const BoxWs& ws, bool valid, double e0, double e1,
                                            double e2, double e3, double& u_first, int& iters, bool& conv) {
    bool active = valid;
    conv = false;
    iters = 0;
    for (int it = 0; it < max_it; ++it) {
        if (!__any(active)) break;
        if (active) {
            const bool all_free = it == 0;
            const bool shared = all_free && w.Kw != nullptr;
            bool changed = true;
            iters = it + 1;
            if (!WS_RESULT && shared && max_it > 1 &&
                !box_forward<false>(w, Lm, ws, true, true, tau, e0, e1, e2, e3, u_first)) {
                changed = false;
            } else {
                if (!shared) box_backward(w, Lm, Q, r, QT, tau, ws, all_free);
                box_forward<true>(w, Lm, ws, shared, all_free, tau, e0, e1, e2, e3, u_first);
                changed = box_update(w, Lm, Q, r, QT, tau, ws, all_free);
            }
            if (!changed && it + 1 < max_it) { conv = true; active = false; }
        }
    }
    if (valid && !conv) {
        for (int t = 0; t < Lm; ++t) {
            const double f = w.row(t)[21];
            const double hi = tau - f, lo = -tau - f;
            const double u = ws.at(t, 9);
            const double c = u > hi ? hi : (u < lo ? lo : u);
            ws.at(t, 9) = c;
            if (t == 0) u_first = c;
        }
    }
}

// the applied torque u_ref + u_0 of one channel: a first control on its bound is the limit itself (hi + u_ref is
// tau_max only up to rounding), and the sum stays inside the limit (NaN passes through)
__device__ __forceinline__ double box_apply(double f, double u0, double tau) {
    const double hi = tau - f, lo = -tau - f;
    const double v = u0 >= hi ? tau : (u0 <= lo ? -tau : f + u0);
    return v > tau ? tau : (v < -tau ? -tau : v);
}
__device__ __forceinline__ double box_clip0(double f, double tau) {   // channel 0: clip(0, lo, hi)
    const double hi = tau - f, lo = -tau - f;
    return 0.0 > hi ? hi : (0.0 < lo ? lo : 0.0);
}

// Stage table of the closed loop: rows 0..S-1 the reference's discretised linearisations, row S the pad (x_f, u_f),
// dense A_d (4,4), B_d (4,2) with disc_stage()'s operations (k_mpc_gains' own stages), and u_ref with u_f appended.
__global__ __launch_bounds__(64) void k_mpc_box_stages(Dyn m, const double* __restrict__ x_ref,
                                                       const double* __restrict__ u_ref, int S,
                                                       const double* __restrict__ xf, const double* __restrict__ uf,
                                                       double* __restrict__ A, double* __restrict__ Bm,
                                                       double* __restrict__ ur) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    const double* x = s < S ? x_ref + 4 * (int64_t)s : xf;
    const double* u = s < S ? u_ref + 2 * (int64_t)s : uf;
    StageLin q;
    disc_stage(m, x[0], x[1], x[2], x[3], u[1], q);
    double* a = A + 16 * (int64_t)s;
    double* b = Bm + 8 * (int64_t)s;
    a[0] = 1.0; a[1] = 0.0; a[2] = m.h; a[3] = 0.0;
    a[4] = 0.0; a[5] = 1.0; a[6] = 0.0; a[7] = m.h;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[8 + j] = q.a2[j]; a[12 + j] = q.a3[j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = 0.0;
    b[5] = q.b2; b[7] = q.b3;
    ur[2 * (int64_t)s] = u[0]; ur[2 * (int64_t)s + 1] = u[1];
}

constexpr int kBoxMaxLm = kMpcMaxStages - 3;   // L - 1 <= 253 stages per window (L + 2 <= 256)

// A batch of QPs on one window: x0 (B,4) -> U (B,L-1,2), X (B,L,4), iterations and converged flag per QP
__global__ __launch_bounds__(64) void k_mpc_box_qp(BoxTable tb, int L, M44 Q, double r, const double* __restrict__ QT,
                                                   double tau, int max_it, const double* __restrict__ x0, int64_t B,
                                                   double* wsd, int32_t* wst, int64_t Bp, double* __restrict__ U,
                                                   double* __restrict__ X, int32_t* __restrict__ iters_out,
                                                   int32_t* __restrict__ conv_out) {
    __shared__ double rows[kBoxMaxLm * kBoxRow];
    const int ln = threadIdx.x;
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + ln;
    const bool valid = l < B;
    const int Lm = L - 1;
    for (int idx = ln; idx < Lm * kBoxRow; idx += 64) rows[idx] = box_row_elem(tb, idx / kBoxRow, idx % kBoxRow);
    wave_lds_order();
    const BoxWin w{rows, nullptr, 0, Lm};
    const BoxWs ws{wsd, wst, Bp, l};
    const int64_t lr = valid ? l : 0;
    double u_first;
    int iters;
    bool conv;
    box_qp_lane<true>(w, Lm, Q, r, QT, tau, max_it, ws, valid, x0[4 * lr], x0[4 * lr + 1], x0[4 * lr + 2],
                      x0[4 * lr + 3], u_first, iters, conv);
    if (!valid) return;
    double* Ul = U + 2 * (int64_t)Lm * l;
    double* Xl = X + 4 * (int64_t)L * l;
    for (int t = 0; t < Lm; ++t) {
        Ul[2 * t] = box_clip0(w.row(t)[20], tau);
        Ul[2 * t + 1] = ws.at(t, 9);
#pragma unroll
        for (int q = 0; q < 4; ++q) Xl[4 * t + q] = ws.at(t, 5 + q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Xl[4 * Lm + q] = ws.at(Lm, q);
    iters_out[l] = iters;
    conv_out[l] = conv ? 1 : 0;
}

// The torque-limited closed loop (solve_mpc_tracking :43-67), one trajectory per lane.  Per control step s: e = x -
// x_ref[s], the window's QP (rows s .. s+L-2 of the stage table, the pad past its end; first iterate from K_all's
// window s), u_real[s] = u_ref[s] + u_0, one RK4 step.  Lane-major x (B,N,4), u (B,N-1,2), qp_iters (B,N-1) and the
// lane's count of unconverged QPs.  The wavefront keeps the window's rows in an LDS ring (one new row per step) and
// loads the window's Kw (row 1 of each gain) at the top of the step.
__global__ __launch_bounds__(64) void k_mpc_box_rollout(Dyn m, BoxTable tb, int L, M44 Q, double r,
                                                        const double* __restrict__ QT, double tau, int max_it,
                                                        const double* __restrict__ x0,
                                                        const double* __restrict__ x_ref,
                                                        const double* __restrict__ K_all, int64_t B, int N,
                                                        double* wsd, int32_t* wst, int64_t Bp,
                                                        double* __restrict__ xo, double* __restrict__ uo,
                                                        int32_t* __restrict__ it_out, int32_t* __restrict__ unconv_out) {
    __shared__ double rows[kBoxMaxLm * kBoxRow];
    __shared__ double kw[kBoxMaxLm * 4];
    const int ln = threadIdx.x;
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + ln;
    const bool valid = l < B;
    const int64_t lr = valid ? l : 0;
    const int T = N - 1, Lm = L - 1;
    const BoxWs ws{wsd, wst, Bp, l};
    double2* xl = reinterpret_cast<double2*>(xo + 4 * (int64_t)N * lr);
    double2* ul = reinterpret_cast<double2*>(uo + 2 * (int64_t)T * lr);
    int32_t* il = it_out + (int64_t)T * lr;
    double n0 = x0[4 * lr], n1 = x0[4 * lr + 1], n2 = x0[4 * lr + 2], n3 = x0[4 * lr + 3];
    if (valid) {
        xl[0] = make_double2(n0, n1);
        xl[1] = make_double2(n2, n3);
    }
    const gym::PolyRegs pk = gym::poly_vgprs();
    int unconv = 0;
    BoxWin w{rows, kw, 0, Lm};
    for (int s = 0; s < T; ++s) {
        wave_lds_order();                               // the previous step's LDS reads are done
        if (s == 0) {
            for (int idx = ln; idx < Lm * kBoxRow; idx += 64) rows[idx] = box_row_elem(tb, idx / kBoxRow, idx % kBoxRow);
        } else {                                        // stage s + Lm - 1 replaces stage s - 1 in the ring
            if (ln < kBoxRow) rows[kBoxRow * w.base + ln] = box_row_elem(tb, s + Lm - 1, ln);
            w.base = w.base + 1 == Lm ? 0 : w.base + 1;
        }
        const double* Ks = K_all + 8 * (int64_t)s * Lm;
        for (int idx = ln; idx < 4 * Lm; idx += 64) kw[idx] = Ks[8 * (idx >> 2) + 4 + (idx & 3)];
        wave_lds_order();
        const double* r4 = x_ref + 4 * (int64_t)s;
        const double* f = w.row(0) + 20;                // u_ref[s]
        double u1;
        int iters;
        bool conv;
        box_qp_lane<false>(w, Lm, Q, r, QT, tau, max_it, ws, valid, n0 - r4[0], n1 - r4[1], n2 - r4[2], n3 - r4[3], u1,
                           iters, conv);
        if (valid) {
            const double v0 = box_apply(f[0], box_clip0(f[0], tau), tau), v1 = box_apply(f[1], u1, tau);
            ul[s] = make_double2(v0, v1);
            il[s] = iters;
            unconv += conv ? 0 : 1;
            gym::rk4(m, n0, n1, n2, n3, v1, pk);
            xl[2 * (s + 1)] = make_double2(n0, n1);
            xl[2 * (s + 1) + 1] = make_double2(n2, n3);
        }
    }
    if (valid) unconv_out[l] = unconv;
}

// workspace of B lanes, windows of L stages, a stage table of `rows` rows: table, then per-lane doubles, then states
struct BoxLayout {
    int64_t Bp, off_B, off_ur, off_d, off_st, bytes;
};
inline BoxLayout box_layout(int64_t B, int L, int64_t rows) {
    BoxLayout o;
    o.Bp = (B + 63) / 64 * 64;
    o.off_B = 16 * rows * 8;
    o.off_ur = o.off_B + 8 * rows * 8;
    o.off_d = o.off_ur + 2 * rows * 8;
    o.off_st = o.off_d + ((int64_t)kBoxSlots * (L - 1) + 4) * o.Bp * 8;
    o.bytes = o.off_st + (int64_t)(L - 1) * o.Bp * 4;
    return o;
}
inline bool box_sizes_ok(int64_t B, int L, double tau_max, int max_qp_iters) {
    return B >= 1 && B <= ((int64_t)1 << 30) && L >= 2 && L + 2 <= kMpcMaxStages && tau_max > 0.0 &&
           tau_max <= 1.7976931348623157e308 && max_qp_iters >= 1;
}
inline bool box_weights_ok(const double* R) {   // the channel split needs a diagonal R with r = R[1][1] > 0
    return R[1] == 0.0 && R[2] == 0.0 && R[3] > 0.0 && R[3] <= 1.7976931348623157e308;
}

#include "lqr_lanes.hpp"   // per-lane LQR tracking: every lane follows its own trajectory
#include "mpc_lanes.hpp"   // per-lane MPC tracking: the first gain of every window of every lane
#include "mpc_box_lanes.hpp"   // per-lane torque-limited MPC tracking: each lane's QPs along its own trajectory

inline M44 m44(const double* p) { M44 m; for (int i = 0; i < 16; ++i) m.v[i] = p[i]; return m; }
inline M22 m22(const double* p) { M22 m; for (int i = 0; i < 4; ++i) m.v[i] = p[i]; return m; }
inline int launch_status() { return (int)hipGetLastError(); }

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
    if (!m || !x_ref || !u_ref || !x_f || !u_f || !Q || !R || !K_out || !QT_out || !iters_out || S <= 0 || L < 2 ||
        L + 2 > kMpcMaxStages || nwin <= 0 || max_iter <= 0)
        return GYM_EINVAL;
    hipLaunchKernelGGL(k_mpc_gains<false>, dim3((unsigned)((nwin + 3) / 4)), dim3(64), 0, (hipStream_t)s, Dyn(*m),
                       x_ref, u_ref, S, x_f, u_f, m44(Q), m22(R), L, nwin, max_iter, tol, K_out, QT_out, iters_out);
    return launch_status();
}

int gym_mpc_gains_all(const gym_model* m, const double* x_ref, const double* u_ref, int32_t S, const double* x_f,
                      const double* u_f, const double Q[16], const double R[4], int32_t L, int32_t nwin,
                      int32_t max_iter, double tol, double* K_all, double* QT_out, int32_t* iters_out, void* s) {
    if (!m || !x_ref || !u_ref || !x_f || !u_f || !Q || !R || !K_all || !QT_out || !iters_out || S <= 0 || L < 2 ||
        L + 2 > kMpcMaxStages || nwin <= 0 || max_iter <= 0)
        return GYM_EINVAL;
    hipLaunchKernelGGL(k_mpc_gains<true>, dim3((unsigned)((nwin + 3) / 4)), dim3(64), 0, (hipStream_t)s, Dyn(*m),
                       x_ref, u_ref, S, x_f, u_f, m44(Q), m22(R), L, nwin, max_iter, tol, K_all, QT_out, iters_out);
    return launch_status();
}

int gym_mpc_box_workspace(int64_t B, int32_t L, int32_t rows, int64_t* bytes_out) {
    if (!bytes_out || B < 1 || B > ((int64_t)1 << 30) || L < 2 || L + 2 > kMpcMaxStages || rows < 1)
        return GYM_EINVAL;
    *bytes_out = box_layout(B, L, rows).bytes;
    return 0;
}

int gym_mpc_box_qp(const double* A, const double* Bm, const double* u_ref, int32_t S, const double Q[16],
                   const double R[4], const double* QT, const double* x0, int64_t B, int32_t L, double tau_max,
                   int32_t max_qp_iters, void* ws, int64_t ws_bytes, double* U, double* X, int32_t* iters_out,
                   int32_t* converged_out, void* s) {
    if (!A || !Bm || !u_ref || !Q || !R || !QT || !x0 || !ws || !U || !X || !iters_out || !converged_out ||
        !box_sizes_ok(B, L, tau_max, max_qp_iters) || S < L - 1 || !box_weights_ok(R))
        return GYM_EINVAL;
    for (int64_t q = 0; q < 4 * (int64_t)S; ++q)
        if (Bm[2 * q] != 0.0) return GYM_EINVAL;       // the channel split needs B[:, 0] = 0 at every stage
    const BoxLayout lo = box_layout(B, L, S);
    if (ws_bytes < lo.bytes) return GYM_EINVAL;
    char* base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)s;
    hipError_t e = hipMemcpyAsync(base, A, 16 * sizeof(double) * S, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(base + lo.off_B, Bm, 8 * sizeof(double) * S, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(base + lo.off_ur, u_ref, 2 * sizeof(double) * S, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    const BoxTable w{reinterpret_cast<const double*>(base), reinterpret_cast<const double*>(base + lo.off_B),
                     reinterpret_cast<const double*>(base + lo.off_ur), S - 1};
    hipLaunchKernelGGL(k_mpc_box_qp, dim3((unsigned)(lo.Bp / 64)), dim3(64), 0, st, w, L, m44(Q), R[3], QT, tau_max,
                       max_qp_iters, x0, B, reinterpret_cast<double*>(base + lo.off_d),
                       reinterpret_cast<int32_t*>(base + lo.off_st), lo.Bp, U, X, iters_out, converged_out);
    return launch_status();
}

int gym_mpc_box_rollout(const gym_model* m, const double* x0, const double* x_ref, const double* u_ref,
                        const double* x_f, const double* u_f, const double Q[16], const double R[4], const double* QT,
                        const double* K_all, int64_t B, int32_t N, int32_t L, double tau_max, int32_t max_qp_iters,
                        void* ws, int64_t ws_bytes, double* x_out, double* u_out, int32_t* qp_iters_out,
                        int32_t* unconverged_out, void* s) {
    if (!m || !x0 || !x_ref || !u_ref || !x_f || !u_f || !Q || !R || !QT || !K_all || !ws || !x_out || !u_out ||
        !qp_iters_out || !unconverged_out || !box_sizes_ok(B, L, tau_max, max_qp_iters) || N < 2 ||
        !box_weights_ok(R))
        return GYM_EINVAL;
    const int S = N - 1;
    const BoxLayout lo = box_layout(B, L, S + 1);
    if (ws_bytes < lo.bytes) return GYM_EINVAL;
    char* base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)s;
    double* tA = reinterpret_cast<double*>(base);
    double* tB = reinterpret_cast<double*>(base + lo.off_B);
    double* tu = reinterpret_cast<double*>(base + lo.off_ur);
    hipLaunchKernelGGL(k_mpc_box_stages, dim3((unsigned)((S + 1 + 63) / 64)), dim3(64), 0, st, Dyn(*m), x_ref, u_ref,
                       S, x_f, u_f, tA, tB, tu);
    const BoxTable w{tA, tB, tu, S};
    hipLaunchKernelGGL(k_mpc_box_rollout, dim3((unsigned)(lo.Bp / 64)), dim3(64), 0, st, Dyn(*m), w, L, m44(Q), R[3],
                       QT, tau_max, max_qp_iters, x0, x_ref, K_all, B, N, reinterpret_cast<double*>(base + lo.off_d),
                       reinterpret_cast<int32_t*>(base + lo.off_st), lo.Bp, x_out, u_out, qp_iters_out,
                       unconverged_out);
    return launch_status();
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
    if (!m || !x0 || !x_ff || !u_ff || !K || !x_out || !u_out || B <= 0 || B > ((int64_t)1 << 30) || N < 2 ||
        (flags & ~GYM_TRACK_SINGLE))
        return GYM_EINVAL;
    if (flags & GYM_TRACK_SINGLE)
        hipLaunchKernelGGL(k_track_rollout, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)s, Dyn(*m), x0,
                           x_ff, u_ff, K, B, N, x_out, u_out);
    else
        hipLaunchKernelGGL(k_track_rollout_pair, dim3((unsigned)((2 * B + 63) / 64)), dim3(64), 0, (hipStream_t)s,
                           Dyn(*m), x0, x_ff, u_ff, K, B, N, x_out, u_out);
    return launch_status();
}

int gym_track_rollout(const gym_model* m, const double* x0, const double* x_ff, const double* u_ff, const double* K,
                      int64_t B, int32_t N, double* x_out, double* u_out, void* s) {
    return gym_track_rollout_ex(m, x0, x_ff, u_ff, K, B, N, 0, x_out, u_out, s);
}

// ---- per-lane LQR tracking (lqr_lanes.hpp) ----
static bool lanes_sizes_ok(int64_t B, int32_t N) {
    return B >= 1 && N >= 2 && (B + 63) / 64 * 64 <= GYM_MAX_BP;
}

int gym_lqr_lanes_workspace(int64_t B, int32_t N, int64_t* bytes_out) {
    if (!bytes_out || !lanes_sizes_ok(B, N)) return GYM_EINVAL;
    *bytes_out = lanes_layout(B, N).bytes;
    return 0;
}

// solve_LQR_tracking (trajectory_tracking.py:170-203) per lane
int gym_lqr_lanes_gains(const gym_model* m, const double* x_opt, const double* u_opt, int64_t B, int32_t N,
                        const double Q[16], const double R[4], const double QT[16], void* ws, int64_t ws_bytes,
                        double* K_out, void* s) {
    if (!m || !x_opt || !u_opt || !Q || !R || !QT || !ws || !lanes_sizes_ok(B, N) || !box_weights_ok(R) ||
        !lanes_sym(Q) || !lanes_sym(QT))
        return GYM_EINVAL;
    const LanesLayout lo = lanes_layout(B, N);
    const int T = N - 1;
    const int64_t groups = lo.Bp / BLK;
    const int ntx = (N + 15) / 16, ntu = (T + 31) / 32, ntk = (T + 15) / 16;
    if (ws_bytes < lo.bytes || groups * ntx > ((int64_t)1 << 31) - 1) return GYM_EINVAL;
    char* base = static_cast<char*>(ws);
    double2* xs = reinterpret_cast<double2*>(base);
    double* us = reinterpret_cast<double*>(base + lo.off_u);
    double2* ks = reinterpret_cast<double2*>(base + lo.off_k);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(k_lqr_pack<4>, dim3((unsigned)(groups * ntx)), dim3(LL_THREADS), 0, st,
                       reinterpret_cast<const double2*>(x_opt), reinterpret_cast<double*>(xs), B, lo.Bp, (int)N, ntx);
    hipLaunchKernelGGL(k_lqr_pack<2>, dim3((unsigned)(groups * ntu)), dim3(LL_THREADS), 0, st,
                       reinterpret_cast<const double2*>(u_opt), us, B, lo.Bp, T, ntu);
    hipLaunchKernelGGL(k_lqr_lane_gains, dim3((unsigned)groups), dim3(BLK), 0, st, Dyn(*m), sym4(Q), sym4(QT), R[3], xs,
                       us, ks, lo.Bp, (int)N);
    if (K_out)
        hipLaunchKernelGGL(k_lqr_unpack_gains, dim3((unsigned)(groups * ntk)), dim3(LL_THREADS), 0, st, ks,
                           reinterpret_cast<double2*>(K_out), B, lo.Bp, T, ntk);
    return launch_status();
}

// simulate_tracking (trajectory_tracking.py:206-216) per lane and perturbed start
int gym_lqr_lanes_rollout(const gym_model* m, const double* x0, int64_t B, int32_t P, int32_t N, const void* ws,
                          int64_t ws_bytes, double* x_out, double* u_out, double* summary_out, void* s) {
    if (!m || !x0 || !ws || !summary_out || !lanes_sizes_ok(B, N) || P < 1 || B > GYM_MAX_BP / P ||
        (x_out == nullptr) != (u_out == nullptr))
        return GYM_EINVAL;
    const LanesLayout lo = lanes_layout(B, N);
    if (ws_bytes < lo.bytes) return GYM_EINVAL;
    const char* base = static_cast<const char*>(ws);
    const double2* xs = reinterpret_cast<const double2*>(base);
    const double* us = reinterpret_cast<const double*>(base + lo.off_u);
    const double2* ks = reinterpret_cast<const double2*>(base + lo.off_k);
    const int64_t nb = (lo.Bp / BLK) * P;                  // <= 2^20 + 2^26 / 64: far below the grid limit
    const dim3 grid((unsigned)((nb + 7) / 8 * 8));
    if (x_out)
        hipLaunchKernelGGL(k_lqr_lane_rollout<true>, grid, dim3(BLK), 0, (hipStream_t)s, Dyn(*m), x0, xs, us, ks, B,
                           lo.Bp, (int)P, (int)N, x_out, u_out, summary_out);
    else
        hipLaunchKernelGGL(k_lqr_lane_rollout<false>, grid, dim3(BLK), 0, (hipStream_t)s, Dyn(*m), x0, xs, us, ks, B,
                           lo.Bp, (int)P, (int)N, x_out, u_out, summary_out);
    return launch_status();
}

// ---- per-lane MPC tracking (mpc_lanes.hpp) ----
// solve_mpc_tracking's gains (trajectory_tracking.py:8-69) per lane: fills a gym_lqr_lanes_rollout workspace
int gym_mpc_lanes_gains(const gym_model* m, const double* x_opt, const double* u_opt, int64_t B, int32_t N, int32_t L,
                        const double Q[16], const double R[4], const double* QT_dev, void* ws, int64_t ws_bytes,
                        double* K_out, void* s) {
    if (!m || !x_opt || !u_opt || !Q || !R || !QT_dev || !ws || !lanes_sizes_ok(B, N) || L < 2 ||
        L + 2 > kMpcMaxStages || !box_weights_ok(R) || !lanes_sym(Q))
        return GYM_EINVAL;
    const LanesLayout lo = lanes_layout(B, N);
    const int T = N - 1;
    const int64_t groups = lo.Bp / BLK;
    const int ntx = (N + 15) / 16, ntu = (T + 31) / 32, ntk = (T + 15) / 16;
    const int64_t nwork = lo.Bp * ((T + ML_W - 1) / ML_W);   // (lane, window block) workgroups
    const int64_t gmax = ((int64_t)1 << 31) - 8;
    if (ws_bytes < lo.bytes || groups * ntx > gmax || nwork > gmax) return GYM_EINVAL;
    char* base = static_cast<char*>(ws);
    double2* xs = reinterpret_cast<double2*>(base);
    double* us = reinterpret_cast<double*>(base + lo.off_u);
    double2* ks = reinterpret_cast<double2*>(base + lo.off_k);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(k_lqr_pack<4>, dim3((unsigned)(groups * ntx)), dim3(LL_THREADS), 0, st,
                       reinterpret_cast<const double2*>(x_opt), reinterpret_cast<double*>(xs), B, lo.Bp, (int)N, ntx);
    hipLaunchKernelGGL(k_lqr_pack<2>, dim3((unsigned)(groups * ntu)), dim3(LL_THREADS), 0, st,
                       reinterpret_cast<const double2*>(u_opt), us, B, lo.Bp, T, ntu);
    const size_t lds = sizeof(double) * ML_ROWS * (ML_W + L - 2);
    hipLaunchKernelGGL(k_mpc_lane_gains<ML_W>, dim3((unsigned)((nwork + 7) / 8 * 8)), dim3(ML_W), lds, st, Dyn(*m),
                       sym4(Q), QT_dev, R[3], reinterpret_cast<const double2*>(x_opt),
                       reinterpret_cast<const double2*>(u_opt), ks, B, lo.Bp, (int)N, (int)L, nwork);
    if (K_out)
        hipLaunchKernelGGL(k_lqr_unpack_gains, dim3((unsigned)(groups * ntk)), dim3(LL_THREADS), 0, st, ks,
                           reinterpret_cast<double2*>(K_out), B, lo.Bp, T, ntk);
    return launch_status();
}


// ---- per-lane torque-limited MPC tracking (mpc_box_lanes.hpp) ----
static bool box_lanes_sizes_ok(int64_t B, int32_t P, int32_t N, int32_t L) {
    return B >= 1 && P >= 1 && N >= 2 && L >= 2 && L + 2 <= kMpcMaxStages && B <= GYM_MAX_BP / P;
}

int gym_mpc_box_lanes_workspace(int64_t B, int32_t P, int32_t L, int64_t* bytes_out) {
    if (!bytes_out || !box_lanes_sizes_ok(B, P, 2, L)) return GYM_EINVAL;
    *bytes_out = box_lanes_layout(B, P, L).bytes;
    return 0;
}

// solve_mpc_tracking's closed loop (trajectory_tracking.py:43-67) with solver_mpc's test_constraints (:87-114) per lane
int gym_mpc_box_lanes_rollout(const gym_model* m, const double* x_opt, const double* u_opt, const double* x0, int64_t B,
                              int32_t P, int32_t N, int32_t L, const double Q[16], const double R[4],
                              const double* QT_dev, double tau_max, int32_t max_qp_iters, void* ws, int64_t ws_bytes,
                              double* x_out, double* u_out, double* summary_out, int32_t* qp_iters_out,
                              int32_t* unconverged_out, void* s) {
    if (!m || !x_opt || !u_opt || !x0 || !Q || !R || !QT_dev || !ws || !summary_out || !unconverged_out ||
        !box_lanes_sizes_ok(B, P, N, L) || !(tau_max > 0.0 && tau_max <= 1.7976931348623157e308) || max_qp_iters < 1 ||
        !box_weights_ok(R) || !lanes_sym(Q) || (x_out == nullptr) != (u_out == nullptr))
        return GYM_EINVAL;
    const BoxLanesLayout lo = box_lanes_layout(B, P, L);
    if (ws_bytes < lo.bytes) return GYM_EINVAL;
    char* base = static_cast<char*>(ws);
    const int nblk = (P + 63) / 64;                        // B nblk <= B P <= GYM_MAX_BP: far below the grid limit
    const size_t lds = sizeof(double) * (kBoxRow + 4) * (L - 1);
    hipLaunchKernelGGL(k_mpc_box_lane_rollout, dim3((unsigned)(B * nblk)), dim3(64), lds, (hipStream_t)s, Dyn(*m),
                       m44(Q), R[3], QT_dev, tau_max, max_qp_iters, reinterpret_cast<const double2*>(x_opt),
                       reinterpret_cast<const double2*>(u_opt), x0, (int)P, (int)N, (int)L, nblk,
                       reinterpret_cast<double*>(base), reinterpret_cast<int32_t*>(base + lo.off_st), x_out, u_out,
                       summary_out, qp_iters_out, unconverged_out);
    return launch_status();
}

}  // extern "C"
