// Closed-loop rollouts on ONE shared reference (gym_track_rollout / gym_track_rollout_ex): the tracking feedback, the
// single-lane kernel and the lane-pair kernel.  Part of the tracking_kernels.hip translation unit: included inside its
// anonymous namespace; gym:: and Dyn come from acrobot_device.hpp, which the .hip includes ahead of the namespace.
#pragma once

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
