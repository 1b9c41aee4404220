// Fused MPC gains of the shared-reference tracker (gym_mpc_gains / gym_mpc_gains_all): the structured stage
// (StageLin, disc_stage), the lane-parallel Riccati map, compute_P_inf with doubling jumps and k_mpc_gains.  Also the
// two things the other tracking headers take from here: kMpcMaxStages (the window bound) and wave_lds_order().
// Part of the tracking_kernels.hip translation unit: included inside its anonymous namespace; gym:: and Dyn come from
// acrobot_device.hpp, which the .hip includes ahead of the namespace (under its GYM_HORNER_VOP3 policy).
#pragma once

#include "tracking_dense.hpp"   // M44, M22, chain4

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

constexpr int kMpcMaxStages = GYM_MPC_MAX_STAGES;   // LDS stage table of one workgroup: its 4 windows' stages (L + 2 <= 256)

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
    return chain4(X + 4 * i, 1, Y + j, 4);
}
__device__ __forceinline__ double dot_xyt(const double* X, const double* Y, int i, int j) {
    return chain4(X + 4 * i, 1, Y + 4 * j, 1);
}
__device__ __forceinline__ double dot_xty(const double* X, const double* Y, int i, int j) {
    return chain4(X + i, 4, Y + j, 4);
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
