// Dense Riccati primitives of the trackers: the 4x4 / 2x2 matrix arguments every tracking kernel takes (M44, M22),
// the reference's recursion on dense stage arrays (gym_tv_lqr_gains), compute_P_inf as a fixed-point loop
// (gym_dare_fixed_point) and one window's LQ forward pass (gym_lq_forward).  Part of the tracking_kernels.hip
// translation unit: included inside its anonymous namespace, after <hip/hip_runtime.h> and <cstdint>.
#pragma once

struct M44 { double v[16]; };
struct M22 { double v[4]; };

// The 4-term sum of every dense product in this translation unit, a and b read at strides sa and sb (1 along a row,
// 4 or 2 down a column): ((a0 b0 + a1 b1) + a2 b2) + a3 b3, left to right.  The bit-for-bit contracts between the
// kernels rest on this order, so it is written here and nowhere else.
__device__ __forceinline__ double chain4(const double* a, int sa, const double* b, int sb) {
    return ((a[0] * b[0] + a[sa] * b[sb]) + a[2 * sa] * b[2 * sb]) + a[3 * sa] * b[3 * sb];
}

// one step of the reference's recursion (trajectory_tracking.py:158-160 / :195-200):
//   aux1 = R + B'PB, aux2 = B'PA, K = -inv(aux1) aux2, P <- Q + A'PA + (A'PB) K
__device__ __forceinline__ void lqr_step(const double* A, const double* Bm, double* P, const M44& Q, const M22& R,
                                         double* K) {
    double PA[16], PB[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) PA[4 * i + j] = chain4(P + 4 * i, 1, A + j, 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) PB[2 * i + j] = chain4(P + 4 * i, 1, Bm + j, 2);
    }
    double a1[4], a2[8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) a1[2 * i + j] = R.v[2 * i + j] + chain4(Bm + i, 2, PB + j, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) a2[4 * i + j] = chain4(Bm + i, 2, PA + j, 4);
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
            const double apa = chain4(A + i, 4, PA + j, 4);
            const double apb0 = chain4(A + i, 4, PB, 2), apb1 = chain4(A + i, 4, PB + 1, 2);
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
        // chain4's sum, written out where a lane-dependent i or j picks the operands (and for PB beside PA): through
        // the helper this kernel gets other register allocation (tools/kernel_isa_diff.py), so these six stay
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
            for (int c = 0; c < 2; ++c) a1[2 * r + c] = R.v[2 * r + c] + chain4(b + r, 2, sPB + c, 2);
        const double a20 = chain4(b, 2, sPA + j, 4), a21 = chain4(b + 1, 2, sPA + j, 4);
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

// LQ forward pass of one window (solver_mpc's X_opt, U_opt): x_{s+1} = A_s x_s + B_s u_s, u_s = K_s x_s
__global__ void k_lq_forward(const double* __restrict__ A, const double* __restrict__ Bm, int S,
                             const double* __restrict__ Ap, const double* __restrict__ Bp, int disc, double dt,
                             const double* __restrict__ K, const double* __restrict__ x0, int L,
                             double* __restrict__ X, double* __restrict__ U) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double x[4] = {x0[0], x0[1], x0[2], x0[3]}, Ad[16], Bd[8];
    for (int s = 0; s < L - 1; ++s) {
        const double* k = K + 8 * s;
        const double u0 = chain4(k, 1, x, 1), u1 = chain4(k + 4, 1, x, 1);
        X[4 * s] = x[0]; X[4 * s + 1] = x[1]; X[4 * s + 2] = x[2]; X[4 * s + 3] = x[3];
        U[2 * s] = u0; U[2 * s + 1] = u1;
        load_stage(A, Bm, s, S, Ap, Bp, disc, dt, Ad, Bd);
        double n[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            n[i] = chain4(Ad + 4 * i, 1, x, 1) + (Bd[2 * i] * u0 + Bd[2 * i + 1] * u1);
        x[0] = n[0]; x[1] = n[1]; x[2] = n[2]; x[3] = n[3];
    }
    X[4 * (L - 1)] = x[0]; X[4 * (L - 1) + 1] = x[1]; X[4 * (L - 1) + 2] = x[2]; X[4 * (L - 1) + 3] = x[3];
}
