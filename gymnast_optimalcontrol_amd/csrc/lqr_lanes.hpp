// Per-lane LQR tracking: every lane tracks its OWN trajectory (x_opt, u_opt), e.g. the swing-up the batched Newton
// solver produced for it (main.py: task_2's result fed to task_3, per lane).  Part of the tracking_kernels.hip
// translation unit (included inside its anonymous namespace; gym:: and Dyn come from acrobot_device.hpp, which the .hip
// includes ahead of the namespace).
//
//   gains    solve_LQR_tracking (trajectory_tracking.py:170-203) per lane: linearise along the lane's trajectory,
//            backward recursion K = -inv(R + B'PB) B'PA, P <- Q + A'PA + (A'PB) K from P = QT;
//   rollout  simulate_tracking (:206-216) per lane and perturbed start: u_t = u_opt_t + K_t (x_t - x_opt_t),
//            x_{t+1} = RK4(x_t, u_t).
//
// The gains are per-lane data here (4 doubles per stage and lane: with B_c[:, 0] = 0 and a diagonal R, row 0 of K_t
// is exactly zero and is never computed or stored), so both kernels stream: one lane per thread, one wavefront per
// workgroup, the solver's time-major SoA with the lane innermost.  Workspace (caller-allocated, Bp = B rounded up to
// 64, padding lanes zero):
//   x_opt  wave-blocked pairs (N, Bp/64, 2, 64) double2      32 N Bp bytes
//   u_opt  planes             (T, 2, Bp)                     16 T Bp bytes
//   K1     wave-blocked pairs (T, Bp/64, 2, 64) double2      32 T Bp bytes   (row 1 of K_t)
// so a wavefront's access to one stage is contiguous (2 KiB for pairs, 512 B per plane).
#pragma once

#include "mpc_gains.hpp"        // wave_lds_order
#include "newton_streams.hpp"   // BLK, wix / pix, ld_nt / st_nt

constexpr int LL_THREADS = 256;   // the LDS-tiled transposes: 4 wavefronts per workgroup
constexpr int LL_PITCH = 65;      // LDS row pitch in doubles (64 lanes + 1: conflict-free transposed reads)
constexpr int LL_RUN = 64;        // doubles of one lane's contiguous run per tile (512 B)
constexpr int LL_STEPS = 8;       // rollout steps a wavefront stages in LDS before it writes them out (24 KiB)

struct LanesLayout {
    int64_t Bp, off_u, off_k, bytes;
};
inline LanesLayout lanes_layout(int64_t B, int N) {
    LanesLayout o;
    o.Bp = (B + 63) / 64 * 64;
    o.off_u = 32 * (int64_t)N * o.Bp;
    o.off_k = o.off_u + 16 * (int64_t)(N - 1) * o.Bp;
    o.bytes = o.off_k + 32 * (int64_t)(N - 1) * o.Bp;
    return o;
}

// Lane-major (B, L, C) -> the working layout, C = 4: wave-blocked pairs (L, Bp/64, 2, 64) double2; C = 2: planes
// (L, 2, Bp).  k_gather_pack_u's scheme for both widths: one workgroup moves the tile of one 64-lane group x KN
// knots (KN C = 64 doubles: a 512-B contiguous run per lane, read by consecutive threads with 16-byte loads), staged
// in LDS as [component][knot][lane] with the 65-double pitch, and written out as whole coalesced rows of 64 lanes
// (1 KiB per pair row, 512 B per plane row).  Padding lanes (>= B) read nothing and are zero-filled.
// grid: (Bp / 64) * ceil(L / KN) workgroups, the knot tiles of one group adjacent.
template <int C>
__global__ __launch_bounds__(LL_THREADS) void k_lqr_pack(const double2* __restrict__ src, double* __restrict__ dst,
                                                         int64_t B, int64_t Bp, int L, int ntiles) {
    constexpr int KN = LL_RUN / C, H = C / 2;              // knots per tile; double2 per knot
    __shared__ double tile[C * KN * LL_PITCH];
    const int64_t g0 = (int64_t)(blockIdx.x / ntiles) * BLK;
    const int t0 = (int)(blockIdx.x % ntiles) * KN;
    const int ts = (L - t0 < KN) ? L - t0 : KN;
    const int run = ts * H;                                 // double2 per lane in this tile
    for (int i = threadIdx.x; i < run * BLK; i += LL_THREADS) {
        const int ln = i / run, e = i - ln * run;
        const int k = e / H, h = e - k * H;
        const int64_t row = g0 + ln;
        const double2 v = row < B ? ld_nt(src + (row * L + t0) * H + e) : make_double2(0.0, 0.0);
        tile[((2 * h) * KN + k) * LL_PITCH + ln] = v.x;
        tile[((2 * h + 1) * KN + k) * LL_PITCH + ln] = v.y;
    }
    __syncthreads();
    if constexpr (C == 4) {
        double2* d2 = reinterpret_cast<double2*>(dst);
        for (int i = threadIdx.x; i < 2 * ts * BLK; i += LL_THREADS) {
            const int ln = i & (BLK - 1), r = i >> 6;      // r = knot * 2 + pair row
            const int k = r >> 1, p = r & 1;
            st_nt(d2 + wix(t0 + k, p, 2, g0 + ln, Bp), tile[((2 * p) * KN + k) * LL_PITCH + ln],
                  tile[((2 * p + 1) * KN + k) * LL_PITCH + ln]);
        }
    } else {
        for (int i = threadIdx.x; i < 2 * ts * BLK; i += LL_THREADS) {
            const int ln = i & (BLK - 1), r = i >> 6;      // r = knot * 2 + plane
            const int k = r >> 1, p = r & 1;
            st_nt(dst + pix(t0 + k, p, 2, g0 + ln, Bp), tile[(p * KN + k) * LL_PITCH + ln]);
        }
    }
}

// K1 pairs (T, Bp/64, 2, 64) -> lane-major full gains (B, T, 2, 4), row 0 = 0: the mirror image of k_lqr_pack<4>
// (coalesced rows in, 1-KiB runs per lane out with 16-byte stores).
__global__ __launch_bounds__(LL_THREADS) void k_lqr_unpack_gains(const double2* __restrict__ K1,
                                                                 double2* __restrict__ dst, int64_t B, int64_t Bp,
                                                                 int T, int ntiles) {
    constexpr int KN = 16;
    __shared__ double tile[4 * KN * LL_PITCH];
    const int64_t g0 = (int64_t)(blockIdx.x / ntiles) * BLK;
    const int t0 = (int)(blockIdx.x % ntiles) * KN;
    const int ts = (T - t0 < KN) ? T - t0 : KN;
    for (int i = threadIdx.x; i < 2 * ts * BLK; i += LL_THREADS) {
        const int ln = i & (BLK - 1), r = i >> 6;
        const int k = r >> 1, p = r & 1;
        const double2 v = K1[wix(t0 + k, p, 2, g0 + ln, Bp)];
        tile[((2 * p) * KN + k) * LL_PITCH + ln] = v.x;
        tile[((2 * p + 1) * KN + k) * LL_PITCH + ln] = v.y;
    }
    __syncthreads();
    const int64_t nl = (B - g0 < BLK) ? B - g0 : BLK;      // real lanes of the group
    const int run = ts * 4;                                 // double2 per lane: (0,0) (0,0) (K10,K11) (K12,K13)
    for (int i = threadIdx.x; i < nl * run; i += LL_THREADS) {
        const int ln = i / run, e = i - ln * run;
        const int k = e >> 2, q = e & 3;
        double2 v = make_double2(0.0, 0.0);
        if (q >= 2) v = make_double2(tile[((2 * (q - 2)) * KN + k) * LL_PITCH + ln],
                                     tile[((2 * (q - 2) + 1) * KN + k) * LL_PITCH + ln]);
        st_nt(dst + ((g0 + ln) * T + t0) * 4 + e, v.x, v.y);
    }
}

// Symmetric 4x4 in 10 registers: the upper triangle, row by row
struct Sym4 { double v[10]; };   // (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
__host__ __device__ inline Sym4 sym4(const double* M) {   // of a symmetric row-major 4x4
    return Sym4{{M[0], M[1], M[2], M[3], M[5], M[6], M[7], M[10], M[11], M[15]}};
}

// One step of the reference's recursion (trajectory_tracking.py:195-200) on the acrobot's discretised stage
//   A_d = I + dt A_c: rows 0, 1 = [1 0 h 0], [0 1 0 h], rows 2, 3 = a2, a3;   B_d = [0, b], b = (0, 0, b2, b3)'
// with a diagonal R.  B_d's zero column leaves aux1 = diag(R00, g), g = R11 + b'Pb, and aux2's row 0 = 0, so row 0 of
// K is zero and row 1 is k = -(b'PA) / g;  P <- Q + A'PA + (A'Pb) k stays symmetric (A'Pb = (b'PA)' for a symmetric
// P) and only its upper triangle is formed.  The products with A_d's rows 0, 1 are the terms their zeros and ones
// leave.  Q: upper triangle of the (symmetric) stage weight.
__device__ __forceinline__ void lqr_lane_step(const double* a2, const double* a3, double b2, double b3, double h,
                                              double r11, const Sym4& Q, Sym4& P, double* k) {
#pragma clang fp contract(on)   // context-independent bits: FMA contraction inside an expression only
    // the full matrices from their upper triangles (register renames: every index is a literal)
    const double* v = P.v;
    const double p[16] = {v[0], v[1], v[2], v[3], v[1], v[4], v[5], v[6], v[2], v[5], v[7], v[8], v[3], v[6], v[8], v[9]};
    const double* w = Q.v;
    const double q[16] = {w[0], w[1], w[2], w[3], w[1], w[4], w[5], w[6], w[2], w[5], w[7], w[8], w[3], w[6], w[8], w[9]};
    double Pb[4], M[16], c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        Pb[i] = p[4 * i + 2] * b2 + p[4 * i + 3] * b3;                                  // P b
        M[4 * i + 0] = (p[4 * i + 0] + p[4 * i + 2] * a2[0]) + p[4 * i + 3] * a3[0];    // P A_d
        M[4 * i + 1] = (p[4 * i + 1] + p[4 * i + 2] * a2[1]) + p[4 * i + 3] * a3[1];
        M[4 * i + 2] = (h * p[4 * i + 0] + p[4 * i + 2] * a2[2]) + p[4 * i + 3] * a3[2];
        M[4 * i + 3] = (h * p[4 * i + 1] + p[4 * i + 2] * a2[3]) + p[4 * i + 3] * a3[3];
    }
    const double g = r11 + (b2 * Pb[2] + b3 * Pb[3]);                          // aux1[1][1]
    c[0] = (Pb[0] + Pb[2] * a2[0]) + Pb[3] * a3[0];                            // b'P A_d = (A_d' P b)'
    c[1] = (Pb[1] + Pb[2] * a2[1]) + Pb[3] * a3[1];
    c[2] = (h * Pb[0] + Pb[2] * a2[2]) + Pb[3] * a3[2];
    c[3] = (h * Pb[1] + Pb[2] * a2[3]) + Pb[3] * a3[3];
    const double ig = gym::recip(g);                                           // g >= R11 > 0 (P stays PSD)
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = -(c[j] * ig);
    double n[16];                                                              // rows i <= j are used
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                              // Q + A_d' M + c k'
        n[j] = (q[j] + ((M[j] + a2[0] * M[8 + j]) + a3[0] * M[12 + j])) + c[0] * k[j];
        n[4 + j] = (q[4 + j] + ((M[4 + j] + a2[1] * M[8 + j]) + a3[1] * M[12 + j])) + c[1] * k[j];
        n[8 + j] = (q[8 + j] + ((h * M[j] + a2[2] * M[8 + j]) + a3[2] * M[12 + j])) + c[2] * k[j];
        n[12 + j] = (q[12 + j] + ((h * M[4 + j] + a2[3] * M[8 + j]) + a3[3] * M[12 + j])) + c[3] * k[j];
    }
    P = Sym4{{n[0], n[1], n[2], n[3], n[5], n[6], n[7], n[10], n[11], n[15]}};
}

// A_d's rows 2, 3 and b of the stage at (x, tau2): discretize_linearization (trajectory_generation.py:161-164) of
// gym::jacobian, with disc_stage()'s operations
__device__ __forceinline__ void lqr_lane_stage(const Dyn& m, double2 xa, double2 xb, double tau2, double* a2,
                                               double* a3, double& b2, double& b3) {
#pragma clang fp contract(on)
    const gym::Jac J = gym::jacobian(m, xa.x, xa.y, xb.x, xb.y, tau2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a2[j] = (j == 2 ? 1.0 : 0.0) + m.h * J.a2[j];
        a3[j] = (j == 3 ? 1.0 : 0.0) + m.h * J.a3[j];
    }
    b2 = m.h * J.bc2;
    b3 = m.h * J.bc3;
}

// The model of a closed loop's plant step x_{t+1} = RK4(x_t, u_t).  Without a table it is the design
// model m itself, by reference, so a kernel instantiated without one is the kernel it was before tables existed.  With
// one it is row `row` of a table of gym_model (gym::model_row, read once per thread before the time loop); dt is the
// design model's.  A thread that is not `valid` (padding) reads nothing and gets the design model.  The per-lane gain
// sweep (k_lqr_lane_gains) takes its design model the same way from a (B) table.
__device__ __forceinline__ const Dyn& lane_plant(const Dyn& m, int64_t, bool) { return m; }
__device__ __forceinline__ Dyn lane_plant(const Dyn& m, int64_t row, bool valid, const gym_model* rows) {
    if (!valid) return m;
    return gym::model_row(m, rows, row);
}
// the design model of lane l in k_lqr_lane_gains: m itself, or with a (B) table row l (padding lanes: m)
__device__ __forceinline__ const Dyn& lane_design(const Dyn& m, int64_t) { return m; }
__device__ __forceinline__ Dyn lane_design(const Dyn& m, int64_t l, const gym_model* rows, int64_t B) {
    return lane_plant(m, l, l < B, rows);
}

// solve_LQR_tracking per lane: reverse time over the packed trajectory, row 1 of every K_t to the K1 stream.
// Stage t - 1's operands are loaded (non-temporal: read once) while stage t is computed.  Padding lanes run on
// their zero trajectory (finite everywhere) and fill their own slots of K1.  grid Bp / 64.
// k<>: every lane is designed on m; k<const gym_model*, int64_t>: the pack Md is the two parameters after m, a (B)
// table of design models in the caller's lane order and B: lane l linearises on row l (lane_plant), padding lanes of a
// ragged group on m.  m.h stays m's.
template <class... Md>
__global__ __launch_bounds__(BLK) void k_lqr_lane_gains(Dyn m, Md... models, Sym4 Q, Sym4 QT, double r11,
                                                        const double2* __restrict__ xs, const double* __restrict__ us,
                                                        double2* __restrict__ ks, int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int T = N - 1;
    decltype(auto) dm = lane_design(m, l, models...);
    Sym4 P = QT;
    double2 xa = ld_nt(xs + wix(T - 1, 0, 2, l, Bp)), xb = ld_nt(xs + wix(T - 1, 1, 2, l, Bp));
    double u1 = ld_nt(us + pix(T - 1, 1, 2, l, Bp));
    for (int t = T - 1; t >= 0; --t) {
        const double2 ca = xa, cb = xb;
        const double cu = u1;
        const int tn = t > 0 ? t - 1 : 0;
        xa = ld_nt(xs + wix(tn, 0, 2, l, Bp));
        xb = ld_nt(xs + wix(tn, 1, 2, l, Bp));
        u1 = ld_nt(us + pix(tn, 1, 2, l, Bp));
        double a2[4], a3[4], b2, b3, k[4];
        lqr_lane_stage(dm, ca, cb, cu, a2, a3, b2, b3);
        lqr_lane_step(a2, a3, b2, b3, m.h, r11, Q, P, k);
        st_nt(ks + wix(t, 0, 2, l, Bp), k[0], k[1]);
        st_nt(ks + wix(t, 1, 2, l, Bp), k[2], k[3]);
    }
}

// u_t[1] of simulate_tracking (:210) with track_feedback()'s operation order (row 1 of K_t; row 0 is zero, so
// channel 0 is u_opt_t[0] itself)
__device__ __forceinline__ double lqr_lane_feedback(double2 ka, double2 kb, double f1, double d0, double d1, double d2,
                                                    double d3) {
#pragma clang fp contract(on)
    return f1 + (((ka.x * d0 + ka.y * d1) + kb.x * d2) + kb.y * d3);
}

// simulate_tracking per lane and perturbed start: B P threads, a wavefront = 64 consecutive lanes at one start index
// p, so its reads of x_opt, u_opt and K1 are the gain sweep's coalesced rows.  The P wavefronts of one lane group are
// dealt to the same XCD (workgroups go round-robin over the 8 XCDs; gridDim.x is a multiple of 8) and run back to
// back there, as k_gamma_sweep's G blocks: the group's streams come from HBM once and from that XCD's L2 for the
// other P - 1.  x0 (B,P,4); summary (3,B,P) = err_final, err_max, u_max.  Stage t + 1's operands are loaded during
// step t's RK4.
// TRAJ: lane-major x_out (B,P,N,4), u_out (B,P,T,2).  The wavefront stages LL_STEPS steps of its 64 lanes in LDS
// ([component][step][lane], 65-double pitch) and writes them as one contiguous run per lane (256 B of x, 128 B of u)
// with 16-byte stores from consecutive threads.  Per-step 16-byte stores from each lane to its own row, as
// k_track_rollout_pair does for its few hundred wavefronts, reach rows 16 KB apart and were 3.3x (non-temporal) and
// 1.5x (plain) slower at 262,144 lanes; 4 staged steps were 2-17 % slower than 8.  Padding lanes of a
// ragged group run on their zero trajectory (the staging is a whole-wavefront step) and write nothing.
// k<TRAJ>: plant and design model are one; k<TRAJ, const gym_model*>: the pack Pl is the one parameter after m, the
// (B,P) table whose row l P + p closed loop (l, p) integrates (lane_plant).  The feedback, the streams and m.h stay
// the design model's.
template <bool TRAJ, class... Pl>
__global__ __launch_bounds__(BLK) void k_lqr_lane_rollout(Dyn m, Pl... plant, const double* __restrict__ x0,
                                                          const double2* __restrict__ xs, const double* __restrict__ us,
                                                          const double2* __restrict__ ks, int64_t B, int64_t Bp, int P,
                                                          int N, double* __restrict__ xo, double* __restrict__ uo,
                                                          double* __restrict__ summary) {
    constexpr int S = LL_STEPS;
    __shared__ double stage[TRAJ ? 6 * S * LL_PITCH : 1];
    const int64_t per = gridDim.x / 8;
    const int64_t bi = (int64_t)(blockIdx.x % 8) * per + blockIdx.x / 8;
    const int64_t grp = bi / P;
    const int p = (int)(bi - grp * P);
    const int ln = threadIdx.x;
    const int64_t l = grp * BLK + ln;
    if (grp >= Bp / BLK) return;
    const bool valid = l < B;
    if (!TRAJ && !valid) return;
    const int T = N - 1;
    const int64_t row = l * P + p;
    decltype(auto) pm = lane_plant(m, row, valid, plant...);   // padding lanes of a ragged group: the design model
    double2* xl = reinterpret_cast<double2*>(xo + 4 * (int64_t)N * row);
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0;
    if (valid) {
        const double2* x0l = reinterpret_cast<const double2*>(x0) + 2 * row;
        const double2 s0 = x0l[0], s1 = x0l[1];
        n0 = s0.x; n1 = s0.y; n2 = s1.x; n3 = s1.y;
        if (TRAJ) {
            st_nt(xl, n0, n1);
            st_nt(xl + 1, n2, n3);
        }
    }
    double2 ra = xs[wix(0, 0, 2, l, Bp)], rb = xs[wix(0, 1, 2, l, Bp)];
    double2 ka = ks[wix(0, 0, 2, l, Bp)], kb = ks[wix(0, 1, 2, l, Bp)];
    double f0 = us[pix(0, 0, 2, l, Bp)], f1 = us[pix(0, 1, 2, l, Bp)];
    const gym::PolyRegs pk = gym::poly_vgprs();
    double emax = 0.0, umax = 0.0;
    const int64_t nl = (B - grp * BLK < BLK) ? B - grp * BLK : BLK;
    for (int t = 0; t < T; ++t) {
        const double d0 = n0 - ra.x, d1 = n1 - ra.y, d2 = n2 - rb.x, d3 = n3 - rb.y;
        const double v0 = f0;
        const double v1 = lqr_lane_feedback(ka, kb, f1, d0, d1, d2, d3);
        ra = xs[wix(t + 1, 0, 2, l, Bp)];                  // x_opt has N = T + 1 stages
        rb = xs[wix(t + 1, 1, 2, l, Bp)];
        const int tn = t + 1 < T ? t + 1 : t;
        ka = ks[wix(tn, 0, 2, l, Bp)];
        kb = ks[wix(tn, 1, 2, l, Bp)];
        f0 = us[pix(tn, 0, 2, l, Bp)];
        f1 = us[pix(tn, 1, 2, l, Bp)];
        emax = gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(emax, d0), d1), d2), d3);
        umax = gym::nanmax_abs(umax, v1);
        gym::rk4(pm, n0, n1, n2, n3, v1, pk);
        if (TRAJ) {
            const int s = t % S;
            stage[(0 * S + s) * LL_PITCH + ln] = n0;
            stage[(1 * S + s) * LL_PITCH + ln] = n1;
            stage[(2 * S + s) * LL_PITCH + ln] = n2;
            stage[(3 * S + s) * LL_PITCH + ln] = n3;
            stage[(4 * S + s) * LL_PITCH + ln] = v0;
            stage[(5 * S + s) * LL_PITCH + ln] = v1;
            if (s == S - 1 || t == T - 1) {                // steps t0 .. t of the 64 lanes, as runs per lane
                const int cnt = s + 1, t0 = t - s;
                wave_lds_order();
                double2* x2 = reinterpret_cast<double2*>(xo);
                double2* u2 = reinterpret_cast<double2*>(uo);
                for (int i = ln; i < nl * 2 * cnt; i += BLK) {
                    const int lo = i / (2 * cnt), e = i - lo * 2 * cnt;
                    const int q = e >> 1, h = e & 1;
                    const int64_t r = (grp * BLK + lo) * P + p;
                    st_nt(x2 + (r * N + t0 + 1) * 2 + e, stage[((2 * h) * S + q) * LL_PITCH + lo],
                          stage[((2 * h + 1) * S + q) * LL_PITCH + lo]);
                }
                for (int i = ln; i < nl * cnt; i += BLK) {
                    const int lo = i / cnt, q = i - lo * cnt;
                    const int64_t r = (grp * BLK + lo) * P + p;
                    st_nt(u2 + r * T + t0 + q, stage[(4 * S + q) * LL_PITCH + lo], stage[(5 * S + q) * LL_PITCH + lo]);
                }
                wave_lds_order();
            }
        }
    }
    if (!valid) return;
    const double d0 = n0 - ra.x, d1 = n1 - ra.y, d2 = n2 - rb.x, d3 = n3 - rb.y;
    const double efin = gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(0.0, d0), d1), d2), d3);
    emax = gym::nanmax_abs(emax, efin);
    const int64_t BP = B * P;
    summary[row] = efin;
    summary[BP + row] = emax;
    summary[2 * BP + row] = umax;
}

inline bool lanes_sym(const double* M) {
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (!(M[4 * i + j] == M[4 * j + i])) return false;
    return true;
}
