// API primitives and point kernels, layout (pack / unpack / gather), solver init, placement probe.
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// kernels: API primitives
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK) void k_backward_api(Dyn m, KW w, const double2* __restrict__ x,
                                                      const double* __restrict__ u, const double* __restrict__ xr,
                                                      const double* __restrict__ ur, double2* __restrict__ K1,
                                                      double* __restrict__ sig, double* __restrict__ dJ,
                                                      double* __restrict__ smax, double2* __restrict__ lam, int64_t B,
                                                      int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    double d, s;
    if (lam)
        backward_lane<true>(m, w, x, u, xr, ur, K1, sig, lam, l, Bp, N, d, s);
    else
        backward_lane<false>(m, w, x, u, xr, ur, K1, sig, nullptr, l, Bp, N, d, s);
    if (dJ) dJ[l] = d;
    if (smax) smax[l] = s;
}

__global__ __launch_bounds__(BLK) void k_open_loop(Dyn m, KW w, const double* __restrict__ x0,
                                                   const double* __restrict__ u, const double* __restrict__ xr,
                                                   const double* __restrict__ ur, double2* __restrict__ xn,
                                                   double* __restrict__ cost, int64_t B, int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const double J = rollout_ref<false>(m, w, nullptr, u, nullptr, nullptr, xr, ur, xn, nullptr, 0.0, l, Bp, N,
                                        x0[4 * l + 0], x0[4 * l + 1], x0[4 * l + 2], x0[4 * l + 3]);
    if (cost) cost[l] = J;
}

__global__ __launch_bounds__(BLK) void k_closed_loop(Dyn m, KW w, const double2* __restrict__ x,
                                                     const double* __restrict__ u, const double2* __restrict__ Kf,
                                                     const double* __restrict__ s, const double* __restrict__ gamma,
                                                     const double* __restrict__ xr, const double* __restrict__ ur,
                                                     double2* __restrict__ xn, double* __restrict__ un,
                                                     double* __restrict__ cost, int64_t B, int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const double2 a = x[wix(0, 0, 2, l, Bp)], b = x[wix(0, 1, 2, l, Bp)];
    const double J = rollout_ref<true>(m, w, x, u, Kf, s, xr, ur, xn, un, gamma[l], l, Bp, N, a.x, a.y, b.x, b.y);
    if (cost) cost[l] = J;
}

__global__ void k_point(Dyn m, const double* __restrict__ x, const double* __restrict__ u,
                        double* __restrict__ out, double* __restrict__ out2, int64_t n, int what) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x0 = x[4 * i], x1 = x[4 * i + 1], x2 = x[4 * i + 2], x3 = x[4 * i + 3];
    const double tau2 = u[2 * i + 1];  // tau1 is not an acrobot input (dynamics.py:205, :153)
    if (what == 0) {                   // continuous_dynamics
        double q1, q2;
        gym::accel(m, x0, x1, x2, x3, tau2, q1, q2);
        out[4 * i] = x2; out[4 * i + 1] = x3; out[4 * i + 2] = q1; out[4 * i + 3] = q2;
    } else if (what == 1) {            // dynamics (RK4)
        gym::rk4(m, x0, x1, x2, x3, tau2);
        out[4 * i] = x0; out[4 * i + 1] = x1; out[4 * i + 2] = x2; out[4 * i + 3] = x3;
    } else {                           // Calculate_A_B_matrixes
        const gym::Jac J = gym::jacobian(m, x0, x1, x2, x3, tau2);
        double* A = out + 16 * i;
        double* Bc = out2 + 8 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) { A[j] = 0.0; A[4 + j] = 0.0; A[8 + j] = J.a2[j]; A[12 + j] = J.a3[j]; }
        A[2] = 1.0; A[7] = 1.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) Bc[j] = 0.0;
        Bc[5] = J.bc2; Bc[7] = J.bc3;
    }
}

struct Mat4 { double v[16]; };
struct Mat2 { double v[4]; };

__device__ __forceinline__ double quad4(const double* M, const double e[4]) {
    double l = 0.0;  // (e^T M) e
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += e[k] * M[4 * k + c];
        l += s * e[c];
    }
    return l;
}

__device__ __forceinline__ double quad2(const double* M, double f0, double f1) {
    return (f0 * M[0] + f1 * M[2]) * f0 + (f0 * M[1] + f1 * M[3]) * f1;
}

__global__ void k_stage_cost_derivs(const double* __restrict__ x, const double* __restrict__ xr,
                                    const double* __restrict__ u, const double* __restrict__ ur, Mat4 Q, Mat2 R,
                                    int terminal, double* __restrict__ lo, double* __restrict__ gx,
                                    double* __restrict__ gu, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = x[4 * i + k] - xr[4 * i + k];
    double l = quad4(Q.v, e);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += Q.v[4 * r + k] * e[k];
        gx[4 * i + r] = 2.0 * s;
    }
    if (!terminal) {
        const double f0 = u[2 * i] - ur[2 * i], f1 = u[2 * i + 1] - ur[2 * i + 1];
        l += quad2(R.v, f0, f1);
        gu[2 * i] = 2.0 * (R.v[0] * f0 + R.v[1] * f1);
        gu[2 * i + 1] = 2.0 * (R.v[2] * f0 + R.v[3] * f1);
    }
    lo[i] = l;
}

__global__ __launch_bounds__(BLK) void k_total_cost(const double2* __restrict__ x, const double* __restrict__ u,
                                                    const double* __restrict__ xr, const double* __restrict__ ur,
                                                    Mat4 Q, Mat2 R, Mat4 QT, double* __restrict__ cost, int64_t B,
                                                    int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    double J = 0.0;
    for (int t = 0; t < N - 1; ++t) {
        const double2 a = x[wix(t, 0, 2, l, Bp)], b = x[wix(t, 1, 2, l, Bp)];
        const double e[4] = {a.x - xr[4 * t], a.y - xr[4 * t + 1], b.x - xr[4 * t + 2], b.y - xr[4 * t + 3]};
        J += quad4(Q.v, e);
        J += quad2(R.v, u[pix(t, 0, 2, l, Bp)] - ur[2 * t], u[pix(t, 1, 2, l, Bp)] - ur[2 * t + 1]);
    }
    const int T = N - 1;
    const double2 a = x[wix(T, 0, 2, l, Bp)], b = x[wix(T, 1, 2, l, Bp)];
    const double e[4] = {a.x - xr[4 * T], a.y - xr[4 * T + 1], b.x - xr[4 * T + 2], b.y - xr[4 * T + 3]};
    cost[l] = J + quad4(QT.v, e);
}

// build_stage_lists (:166-181) as plain-double SoA for the generic Riccati path
__global__ __launch_bounds__(BLK) void k_linearize(Dyn m, KW w, const double2* __restrict__ x,
                                                   const double* __restrict__ u, const double* __restrict__ xr,
                                                   const double* __restrict__ ur, double* __restrict__ Ad,
                                                   double* __restrict__ Bd, double* __restrict__ q,
                                                   double* __restrict__ r, double* __restrict__ qT, int64_t B,
                                                   int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const double dt = m.h;
    const int T = N - 1;
    for (int t = 0; t < T; ++t) {
        const double2 a = x[wix(t, 0, 2, l, Bp)], b = x[wix(t, 1, 2, l, Bp)];
        const double v0 = u[pix(t, 0, 2, l, Bp)], v1 = u[pix(t, 1, 2, l, Bp)];
        const gym::Jac J = gym::jacobian(m, a.x, a.y, b.x, b.y, v1);
        double A[16] = {1.0, 0.0, dt, 0.0, 0.0, 1.0, 0.0, dt};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            A[8 + j] = (j == 2 ? 1.0 : 0.0) + dt * J.a2[j];
            A[12 + j] = (j == 3 ? 1.0 : 0.0) + dt * J.a3[j];
        }
        double Bv[8] = {0, 0, 0, 0, 0, dt * J.bc2, 0, dt * J.bc3};
#pragma unroll
        for (int c = 0; c < 16; ++c) Ad[((int64_t)t * 16 + c) * Bp + l] = A[c];
#pragma unroll
        for (int c = 0; c < 8; ++c) Bd[((int64_t)t * 8 + c) * Bp + l] = Bv[c];
        const double xe[4] = {a.x - xr[4 * t], a.y - xr[4 * t + 1], b.x - xr[4 * t + 2], b.y - xr[4 * t + 3]};
#pragma unroll
        for (int c = 0; c < 4; ++c) q[((int64_t)t * 4 + c) * Bp + l] = (2.0 * w.Q[c]) * xe[c];
        r[((int64_t)t * 2) * Bp + l] = (2.0 * w.R[0]) * (v0 - ur[2 * t]);
        r[((int64_t)t * 2 + 1) * Bp + l] = (2.0 * w.R[1]) * (v1 - ur[2 * t + 1]);
    }
    const double2 a = x[wix(T, 0, 2, l, Bp)], b = x[wix(T, 1, 2, l, Bp)];
    const double xe[4] = {a.x - xr[4 * T], a.y - xr[4 * T + 1], b.x - xr[4 * T + 2], b.y - xr[4 * T + 3]};
#pragma unroll
    for (int c = 0; c < 4; ++c) qT[(int64_t)c * Bp + l] = (2.0 * w.QT[c]) * xe[c];
}

// 2x2 solve G X = Y (X, Y 2 x ncol) by LU with partial pivoting, as LAPACK dgesv orders it.
template <int NC>
__device__ __forceinline__ void solve2(double g00, double g01, double g10, double g11, double (&y)[2][NC]) {
    if (fabs(g10) > fabs(g00)) {
        double t;
        t = g00; g00 = g10; g10 = t;
        t = g01; g01 = g11; g11 = t;
#pragma unroll
        for (int c = 0; c < NC; ++c) { t = y[0][c]; y[0][c] = y[1][c]; y[1][c] = t; }
    }
    const double l10 = g10 / g00;
    const double u11 = g11 - l10 * g01;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double z1 = y[1][c] - l10 * y[0][c];
        const double x1 = z1 / u11;
        y[1][c] = x1;
        y[0][c] = (y[0][c] - g01 * x1) / g00;
    }
}

// calculate_K_and_sigma (:183-216) on general dense stage data (plain-double SoA).
__global__ __launch_bounds__(BLK) void k_riccati_general(
    const double* __restrict__ A, const double* __restrict__ Bm, const double* __restrict__ Q,
    const double* __restrict__ R, const double* __restrict__ S, const double* __restrict__ q,
    const double* __restrict__ r, const double* __restrict__ QT, const double* __restrict__ qT,
    double* __restrict__ K, double* __restrict__ sigma, double* __restrict__ dJo, int64_t B, int64_t Bp, int T) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    double P[16], p[4];
#pragma unroll
    for (int c = 0; c < 16; ++c) P[c] = QT[(int64_t)c * Bp + l];
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] = qT[(int64_t)c * Bp + l];
    double dJ = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        double a[16], b[8];
#pragma unroll
        for (int c = 0; c < 16; ++c) a[c] = A[((int64_t)t * 16 + c) * Bp + l];
#pragma unroll
        for (int c = 0; c < 8; ++c) b[c] = Bm[((int64_t)t * 8 + c) * Bp + l];
        double PB[8], PA[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += P[4 * i + k] * b[2 * k + j];
                PB[2 * i + j] = s;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += P[4 * i + k] * a[4 * k + j];
                PA[4 * i + j] = s;
            }
        }
        double G[4], Y[2][5];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += b[2 * k + i] * PB[2 * k + j];
                G[2 * i + j] = R[((int64_t)t * 4 + 2 * i + j) * Bp + l] + s;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += b[2 * k + i] * PA[4 * k + j];
                Y[i][j] = S[((int64_t)t * 8 + 4 * i + j) * Bp + l] + s;   // F
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += b[2 * k + i] * p[k];
            Y[i][4] = r[((int64_t)t * 2 + i) * Bp + l] + s;                // g
        }
        const double g0 = Y[0][4], g1 = Y[1][4];
        solve2<5>(G[0], G[1], G[2], G[3], Y);
        double Kt[8], st[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) Kt[4 * i + j] = -Y[i][j];
            st[i] = -Y[i][4];
        }
        dJ += g0 * st[0] + g1 * st[1];
        double GK[8], Gs[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) GK[4 * i + j] = G[2 * i] * Kt[j] + G[2 * i + 1] * Kt[4 + j];
            Gs[i] = G[2 * i] * st[0] + G[2 * i + 1] * st[1];
        }
        double Pn[16], pn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += a[4 * k + i] * PA[4 * k + j];
                Pn[4 * i + j] = Q[((int64_t)t * 16 + 4 * i + j) * Bp + l] + s - (Kt[i] * GK[j] + Kt[4 + i] * GK[4 + j]);
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a[4 * k + i] * p[k];
            pn[i] = q[((int64_t)t * 4 + i) * Bp + l] + s - (Kt[i] * Gs[0] + Kt[4 + i] * Gs[1]);
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) P[c] = Pn[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) p[c] = pn[c];
#pragma unroll
        for (int c = 0; c < 8; ++c) K[((int64_t)t * 8 + c) * Bp + l] = Kt[c];
        sigma[((int64_t)t * 2) * Bp + l] = st[0];
        sigma[((int64_t)t * 2 + 1) * Bp + l] = st[1];
    }
    dJo[l] = dJ;
}

// ------------------------------------------------------------------------------------------
// kernels: layout.  Lane-major (B, L, C) <-> SoA (L, C/W, Bp, W), W = 1 (planes) or 2 (pairs).
// ------------------------------------------------------------------------------------------
__global__ void k_pack(const double* __restrict__ src, double* __restrict__ dst, int64_t B, int64_t Bp, int L,
                       int C, int W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // element (of W doubles) index
    const int P = C / W;
    if (i >= (int64_t)L * P * Bp) return;
    const int64_t lane = i % Bp;
    const int64_t rest = i / Bp;
    const int p = (int)(rest % P);
    const int64_t t = rest / P;
    const double* s = src + (lane * L + t) * C + W * p;
    const int64_t d = W == 2 ? wix(t, p, P, lane, Bp) : i;   // pairs: wave-blocked
    for (int k = 0; k < W; ++k) dst[W * d + k] = (lane < B) ? s[k] : 0.0;
}

// SoA -> lane-major transposes through LDS.  One workgroup (256 threads) moves the tile of one 64-lane group x
// TS knots: the SoA rows are read coalesced (a 64-lane row is 512 B or 1 KiB contiguous), the tile is staged in
// LDS as [knot][component][lane] with a 65-double row pitch (a lane's column is read conflict-free), and each
// lane's TS x C output doubles -- contiguous in the lane-major array -- are written by consecutive threads.
// Src supplies component c of knot t of a lane (which may be derived, e.g. sigma0, or a constant 0).
constexpr int TILE_PITCH = BLK + 1;
constexpr int TILE_THREADS = 256;
constexpr int TILE_DOUBLES = 4096;   // 32 KiB of LDS per workgroup (5 per CU): TS * C * TILE_PITCH <= TILE_DOUBLES
inline int tile_knots(int C) {
    int ts = TILE_DOUBLES / (C * TILE_PITCH);
    return ts < 1 ? 1 : (ts > 32 ? 32 : ts);
}

struct SrcPairs {   // wave-blocked pairs (L, P, Bp) double2, per-lane buffer select
    const double2 *s0, *s1;
    const int32_t* sel;
    int P;
    __device__ __forceinline__ double operator()(int64_t t, int c, int64_t lane, int64_t Bp) const {
        const double2* b = (sel && sel[lane]) ? s1 : s0;
        const double2 v = b[wix(t, c >> 1, P, lane, Bp)];
        return (c & 1) ? v.y : v.x;
    }
};
struct SrcPlanes {  // planes (L, C, Bp) double, per-lane buffer select
    const double *s0, *s1;
    const int32_t* sel;
    int C;
    __device__ __forceinline__ double operator()(int64_t t, int c, int64_t lane, int64_t Bp) const {
        const double* b = (sel && sel[lane]) ? s1 : s0;
        return b[(t * C + c) * Bp + lane];
    }
};
struct SrcGains {   // full K_t (2,4) from its row 1 (K1 pairs); row 0 is identically 0
    const double2* K1;
    __device__ __forceinline__ double operator()(int64_t t, int c, int64_t lane, int64_t Bp) const {
        if (c < 4) return 0.0;
        const double2 v = K1[wix(t, (c - 4) >> 1, 2, lane, Bp)];
        return (c & 1) ? v.y : v.x;
    }
};
struct SrcSigma {   // sigma of each lane's last iteration: sigma0 recomputed from that iteration's u0, sigma1 plane
    KW w;
    const double *cs, *u0b, *u1b, *ur;
    const int32_t* n_iter;
    int64_t ur_lane;   // per-lane references: doubles per lane of u_ref (0: shared)
    __device__ __forceinline__ double operator()(int64_t t, int c, int64_t lane, int64_t Bp) const {
        const int it = n_iter[lane];
        if (it <= 0) return 0.0;
        if (c == 1) return cs[pix((int)t, 1, 2, lane, Bp)];
        const double* u = ((it - 1) & 1) ? u1b : u0b;
        return -(w.G00 * (u[pix((int)t, 0, 2, lane, Bp)] - ur[lane * ur_lane + 2 * t])) * w.iG00;
    }
};

// dst (B, L, C) lane-major; grid (Bp / 64) x ceil(L / TS); dynamic LDS TS * C * TILE_PITCH doubles.
// CT: C at compile time (the solver's outputs: 2, 4, 8 -- the divisions by C become shifts and the stores 16 B
// wide), 0 = C at run time (gym_unpack_lanes' general form).
template <class Src, int CT>
__global__ __launch_bounds__(TILE_THREADS) void k_unpack_tiled(Src src, double* __restrict__ dst,
                                                               const int64_t* __restrict__ map, int64_t B,
                                                               int64_t Bp, int L, int C_rt, int TS) {
    extern __shared__ double tile[];
    __shared__ int64_t rows_of[BLK];                        // output row of each lane of the group
    const int C = CT ? CT : C_rt;
    const int64_t g0 = (int64_t)blockIdx.x * BLK;          // first lane of the group
    const int t0 = (int)blockIdx.y * TS;
    const int ts = (L - t0 < TS) ? L - t0 : TS;
    const int rows = ts * C;
    if (threadIdx.x < BLK) {
        const int64_t l = g0 + threadIdx.x;
        rows_of[threadIdx.x] = map ? (l < B ? map[l] : 0) : l;
    }
    for (int i = threadIdx.x; i < rows * BLK; i += TILE_THREADS) {
        const int ln = i & (BLK - 1), r = i >> 6;          // r = knot * C + component
        tile[r * TILE_PITCH + ln] = src(t0 + r / C, r % C, g0 + ln, Bp);
    }
    __syncthreads();
    const int64_t nl = (B - g0 < BLK) ? B - g0 : BLK;      // real lanes of the group
    if (CT > 0 && CT % 2 == 0) {   // component pairs: 16-byte stores
        const int half = rows / 2;
        double2* d2 = reinterpret_cast<double2*>(dst);
        for (int i = threadIdx.x; i < nl * half; i += TILE_THREADS) {
            const int ln = i / half, r2 = i - ln * half;
            d2[((rows_of[ln] * L + t0) * C) / 2 + r2] =
                make_double2(tile[(2 * r2) * TILE_PITCH + ln], tile[(2 * r2 + 1) * TILE_PITCH + ln]);
        }
    } else {
        for (int i = threadIdx.x; i < nl * rows; i += TILE_THREADS) {
            const int ln = i / rows, r = i - ln * rows;
            dst[(rows_of[ln] * L + t0) * C + r] = tile[r * TILE_PITCH + ln];
        }
    }
}

// Lane-major controls (B, T, 2), rows selected through a lane map, -> planes (T, 2, Bp): the warm start's input
// side (gym_newton_init_warm).  The mirror image of k_unpack_tiled: one workgroup moves the tile of one 64-lane
// group x GP_TS knots.  Each lane's GP_TS (tau1, tau2) pairs -- contiguous in the lane-major array -- are read by
// consecutive threads with 16-byte loads (512 B runs per lane), staged in LDS as [plane][knot][lane] with the
// 65-double row pitch (consecutive knots of one lane land 65 doubles apart: conflict-free), and every plane row is
// written as one coalesced 512 B row of 64 lanes.  Internal lane l takes row map[l] (NULL: l); padding lanes
// (l >= B) read nothing and are zero-filled.  grid (Bp / 64) x ceil(T / GP_TS).
constexpr int GP_TS = 32;
__global__ __launch_bounds__(TILE_THREADS) void k_gather_pack_u(const double2* __restrict__ src,
                                                                double* __restrict__ dst,
                                                                const int64_t* __restrict__ map, int64_t B,
                                                                int64_t Bp, int T) {
    __shared__ double tile[2 * GP_TS * TILE_PITCH];
    __shared__ int64_t rows_of[BLK];                        // input row of each lane of the group
    const int64_t g0 = (int64_t)blockIdx.x * BLK;          // first lane of the group
    const int t0 = (int)blockIdx.y * GP_TS;
    const int ts = (T - t0 < GP_TS) ? T - t0 : GP_TS;
    if (threadIdx.x < BLK) {
        const int64_t l = g0 + threadIdx.x;
        rows_of[threadIdx.x] = (l < B) ? (map ? map[l] : l) : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ts * BLK; i += TILE_THREADS) {
        const int ln = i / ts, k = i - ln * ts;
        const int64_t row = rows_of[ln];
        const double2 v = row >= 0 ? ld_nt(src + row * T + t0 + k) : make_double2(0.0, 0.0);
        tile[k * TILE_PITCH + ln] = v.x;
        tile[(GP_TS + k) * TILE_PITCH + ln] = v.y;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * ts * BLK; i += TILE_THREADS) {
        const int ln = i & (BLK - 1), r = i >> 6;          // r = plane * ts + knot
        const int p = r >= ts, k = r - p * ts;
        st_nt(dst + pix(t0 + k, p, 2, g0 + ln, Bp), tile[(p * GP_TS + k) * TILE_PITCH + ln]);
    }
}

// Warm start (gym_newton_init_warm): k_init's reset, with x[0] rolled out from x0 under the caller's controls
// (already packed into u[0]) and each lane's status taken from status_init.  Internal lane l takes row map[l] of x0
// and status_init (NULL: l); per-lane references are indexed by the internal lane, as everywhere.
// Both init kernels: k<...>: every lane rolls out on m; k<..., const gym_model*>: the pack Md is the one parameter
// after w, the (Bp) table of per-lane models in internal lane order (gym_newton_init_models): lane l rolls out on row
// l (gym::model_row), dt staying m's; k<..., const gym_weights*>: the pack is the (Bp) table of per-lane weights
// (gym_newton_init_weights): lane l's cost is on row l (weights_row, kw()).
__device__ __forceinline__ const Dyn& init_model(const Dyn& m, int64_t) { return m; }
__device__ __forceinline__ Dyn init_model(const Dyn& m, int64_t l, const gym_model* rows) {
    return gym::model_row(m, rows, l);
}
__device__ __forceinline__ const Dyn& init_model(const Dyn& m, int64_t, const gym_weights*) { return m; }
__device__ __forceinline__ const KW& init_weights(const KW& w, int64_t) { return w; }
__device__ __forceinline__ const KW& init_weights(const KW& w, int64_t, const gym_model*) { return w; }
__device__ __forceinline__ KW init_weights(const KW&, int64_t l, const gym_weights* rows) {
    return kw(weights_row(rows, l));
}
template <bool U0Z, bool RL, class... Md>
__global__ __launch_bounds__(BLK) void k_init_warm(Dyn m, KW w, Md... models, const double* __restrict__ x0,
                                                   const int32_t* __restrict__ status_init,
                                                   const int64_t* __restrict__ map, const double* __restrict__ u,
                                                   const double* __restrict__ xr, const double* __restrict__ ur,
                                                   double2* __restrict__ xn, double* __restrict__ cost,
                                                   int32_t* __restrict__ status, int32_t* __restrict__ n_iter,
                                                   int32_t* __restrict__ res_buf, int32_t* __restrict__ n_roll,
                                                   double* __restrict__ gamma, double* __restrict__ smax,
                                                   double* __restrict__ dJ, int64_t B, int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= Bp) return;
    n_iter[l] = 0; res_buf[l] = 0; n_roll[l] = 0; gamma[l] = 0.0; smax[l] = 0.0; dJ[l] = 0.0;
    if (l >= B) {
        status[l] = GYM_PAD;
        cost[l] = 0.0;
        return;
    }
    const int64_t row = map ? map[l] : l;
    // a finished lane keeps its status and never iterates (its result: buffer 0); anything else is an interrupted
    // lane (GYM_ACTIVE, GYM_MAX_ITERS) or out of contract, and iterates
    const int32_t s_in = status_init ? status_init[row] : (int32_t)GYM_ACTIVE;
    status[l] = (s_in == GYM_CONVERGED || s_in == GYM_LS_FAILED) ? s_in : (int32_t)GYM_ACTIVE;
    decltype(auto) lm = init_model(m, l, models...);
    decltype(auto) lw = init_weights(w, l, models...);
    cost[l] = rollout_warm<U0Z>(lm, lw, u, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), xn, l, Bp, N, x0[4 * row + 0],
                                x0[4 * row + 1], x0[4 * row + 2], x0[4 * row + 3]);
}

template <bool RL = false, class... Md>
__global__ __launch_bounds__(BLK) void k_init(Dyn m, KW w, Md... models, const double* __restrict__ x0,
                                              const double* __restrict__ u, const double* __restrict__ xr,
                                              const double* __restrict__ ur, double2* __restrict__ xn,
                                              double* __restrict__ cost, int32_t* __restrict__ status,
                                              int32_t* __restrict__ n_iter, int32_t* __restrict__ res_buf,
                                              int32_t* __restrict__ n_roll, double* __restrict__ gamma,
                                              double* __restrict__ smax, double* __restrict__ dJ, int64_t B,
                                              int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= Bp) return;
    n_iter[l] = 0; res_buf[l] = 0; n_roll[l] = 0; gamma[l] = 0.0; smax[l] = 0.0; dJ[l] = 0.0;
    if (l >= B) {
        status[l] = GYM_PAD;
        cost[l] = 0.0;
        return;
    }
    status[l] = GYM_ACTIVE;
    decltype(auto) lm = init_model(m, l, models...);
    decltype(auto) lw = init_weights(w, l, models...);
    cost[l] = rollout_ref<false>(lm, lw, nullptr, u, nullptr, nullptr, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                 lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), xn, nullptr, 0.0, l, Bp, N,
                                 x0[4 * l + 0], x0[4 * l + 1], x0[4 * l + 2], x0[4 * l + 3]);
}

// Placement probe (gym_placement_probe): the pipelined phase kernel's stream traffic with no arithmetic.  The first
// half of the workgroups runs the sweep's pattern on lanes [0, Bp/2) (stage T-1 .. 0: read the 2 KiB x_cb block and
// the 512 B tau2 row of u_cb, write the K1 block and the cg row), the rest the trial's on [Bp/2, Bp) (stage 0 .. T-1:
// read K1 and cg, write x_cb' at t + 1 and u_cb'), one stage prefetched, non-temporal, four wavefronts per SIMD -- the
// phase kernel's bytes per launch.  How fast this moves depends on where the driver placed the six streams the same
// way the phase kernel's speed does (profiles/r06/README.md: 1.84-2.13 ms on eight sets of one process, Pearson
// 0.87-0.93 against the kernel's own phase times), so a solver ranks candidate stream sets with it in a few ms each.
// It overwrites the streams (garbage; no NaN traps on the GPU): only before gym_newton_init.
extern "C" __global__ __launch_bounds__(BLK, 4) void k_placement_probe(double2* __restrict__ xc, double2* __restrict__ xn,
                                                            double* __restrict__ uc, double* __restrict__ un,
                                                            double2* __restrict__ K1, double* __restrict__ cs,
                                                            int64_t Bp, int T) {
    const int64_t w = blockIdx.x, j = threadIdx.x;
    const bool sweep = w < (Bp / BLK) / 2;
    const int64_t px = w * 2 * BLK + j, pl = w * BLK + j;
    const int64_t row = 2 * Bp;                  // double2 per knot row of a pair stream; doubles per stage of planes
    if (sweep) {
        double2 a = ld_nt(xc + (int64_t)(T - 1) * row + px), b = ld_nt(xc + (int64_t)(T - 1) * row + px + BLK);
        double c = ld_nt(uc + (int64_t)(T - 1) * row + Bp + pl);
        for (int t = T - 1; t >= 0; --t) {
            double2 na = a, nb = b;
            double nc = c;
            if (t > 0) {
                na = ld_nt(xc + (int64_t)(t - 1) * row + px); nb = ld_nt(xc + (int64_t)(t - 1) * row + px + BLK);
                nc = ld_nt(uc + (int64_t)(t - 1) * row + Bp + pl);
            }
            st_nt(K1 + (int64_t)t * row + px, a.x + c, a.y); st_nt(K1 + (int64_t)t * row + px + BLK, b.x, b.y);
            st_nt(cs + (int64_t)t * row + pl, c);
            a = na; b = nb; c = nc;
        }
    } else {
        double2 a = ld_nt(K1 + px), b = ld_nt(K1 + px + BLK);
        double c = ld_nt(cs + pl);
        for (int t = 0; t < T; ++t) {
            double2 na = a, nb = b;
            double nc = c;
            if (t + 1 < T) {
                na = ld_nt(K1 + (int64_t)(t + 1) * row + px); nb = ld_nt(K1 + (int64_t)(t + 1) * row + px + BLK);
                nc = ld_nt(cs + (int64_t)(t + 1) * row + pl);
            }
            st_nt(xn + (int64_t)(t + 1) * row + px, a.x + c, a.y); st_nt(xn + (int64_t)(t + 1) * row + px + BLK, b.x, b.y);
            st_nt(un + (int64_t)t * row + Bp + pl, c);
            a = na; b = nb; c = nc;
        }
    }
}
