// Newton solver kernels: the lock-step schedules (serial sweep / trial, pipelined phase) and the post-trial Armijo
// search.
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// kernels: batched Newton / Armijo solver (newton_Algorithm :298-398)
// ------------------------------------------------------------------------------------------
// Diagnostic build only (-DGYM_WAVE_TRACE, tools/wave_trace.py): per-wavefront start/end time and
// hardware placement of the serial schedule's sweep (kind 0) and trial (kind 1) launches.
#ifdef GYM_WAVE_TRACE
__device__ unsigned long long g_wave_trace[2][8192][4];
struct WaveTrace {
    int kind;
    unsigned long long t0;
    __device__ explicit WaveTrace(int k) : kind(k), t0(__builtin_amdgcn_s_memrealtime()) {}
    __device__ ~WaveTrace() {
        if (threadIdx.x == 0 && blockIdx.x < 8192) {
            unsigned long long* r = g_wave_trace[kind][blockIdx.x];
            r[0] = t0;
            r[1] = __builtin_amdgcn_s_memrealtime();
            r[2] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
            r[3] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
        }
    }
};
#define GYM_TRACE_WAVE(k) WaveTrace wave_trace_(k)
#else
#define GYM_TRACE_WAVE(k)
#endif

// lane-private LDS of the checkpointed sweep: CKI knots x 2 pairs + CKI controls (tau2; and tau1 unless
// U0Z) x 64 lanes: 10 KiB per wave with U0Z, so 16 waves fill one CU's 160 KiB exactly.
constexpr int ck_lds_doubles(bool ck, bool u0z) { return ck ? (4 + (u0z ? 1 : 2)) * CKI * BLK : 2; }
#define GYM_CK_LDS(CK, U0Z) __shared__ double2 ck_lds[ck_lds_doubles(CK, U0Z) / 2]

// Lane ranges: the serial schedule runs every lane [0, B); the pipelined schedule splits the batch
// into two halves H0 = [0, Bh), H1 = [Bh, B) whose iterations are offset by one phase.
struct Range {
    int64_t lo, hi;
};

template <bool U0Z, bool CK, int OUT = OUT_SOLVER>
__device__ __forceinline__ void backward_solver(const Dyn& m, const KW& w, const double2* __restrict__ x,
                                                const double* __restrict__ u, const double* __restrict__ xr,
                                                const double* __restrict__ ur, double2* __restrict__ K1,
                                                double* __restrict__ cs, double g0, double* __restrict__ dJ,
                                                double* __restrict__ smax, double* __restrict__ hist_smax, int64_t l,
                                                int64_t Bp, int N, int k, int hist_len, double2* __restrict__ lds) {
    double d, s;
    if (CK)
        backward_solver_lane_ck<U0Z, OUT>(m, w, x, u, xr, ur, K1, cs, g0, lds, l, Bp, N, d, s);
    else
        backward_solver_lane<U0Z, OUT>(m, w, x, u, xr, ur, K1, cs, g0, l, Bp, N, d, s);
    if (OUT == OUT_SIGMA) return;   // a re-run: the lane's dJ / smax are those of the original sweep
    dJ[l] = d;
    smax[l] = s;
    if (hist_smax && k < hist_len) hist_smax[(int64_t)k * Bp + l] = s;
}

#define GYM_NT_BACKWARD_PARAMS                                                                                  \
    Dyn m, KW w, const double2 *__restrict__ x, const double *__restrict__ u, const double *__restrict__ xr,   \
        const double *__restrict__ ur, double2 *__restrict__ K1, double *__restrict__ cs, double g0,           \
        double *__restrict__ dJ, double *__restrict__ smax, const int32_t *__restrict__ status,               \
        double *__restrict__ hist_smax, Range rg, int64_t Bp, int N, int k, int hist_len
#define GYM_NT_BACKWARD_BODY(OUT)                                                                               \
    GYM_TRACE_WAVE(0);                                                                                          \
    const int64_t l = rg.lo + (int64_t)blockIdx.x * BLK + threadIdx.x;                                          \
    GYM_CK_LDS(CK, U0Z);                                                                                        \
    if (l >= rg.hi || status[l] != GYM_ACTIVE) return;                                                          \
    backward_solver<U0Z, CK, OUT>(m, w, x, u, lane_ref<RL>(xr, l, 4 * (int64_t)N),                               \
                                  lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), K1, cs, g0, dJ, smax, hist_smax, l, Bp, \
                                  N, k, hist_len, ck_lds);

// the solver's serial-schedule sweep (K1, cg) ...
template <bool U0Z, bool CK, bool RL = false>
__global__ __launch_bounds__(BLK, 4) void k_nt_backward(GYM_NT_BACKWARD_PARAMS) { GYM_NT_BACKWARD_BODY(OUT_SOLVER) }
// ... and the same sweep also storing sigma1, for the gamma sweeps of gym_newton_gamma_sweep
template <bool U0Z, bool CK, bool RL = false>
__global__ __launch_bounds__(BLK, 4) void k_nt_backward_all(GYM_NT_BACKWARD_PARAMS) { GYM_NT_BACKWARD_BODY(OUT_ALL) }

struct SolverCtl {
    double tol, beta, c, gamma0;
    int max_ls, k, hist_len, pad;
};

__device__ __forceinline__ void accept_lane(const SolverCtl& a, int64_t l, double Jn, double g, double smax,
                                            double* cost, double* gamma, int32_t* status, int32_t* res_buf,
                                            double* hist_cost, int64_t Bp) {
    cost[l] = Jn;
    gamma[l] = g;
    if (smax < a.tol) {  // convergence is tested after the update (:383-396)
        status[l] = GYM_CONVERGED;
        res_buf[l] = (a.k + 1) & 1;
    }
    if (hist_cost && a.k < a.hist_len) hist_cost[(int64_t)a.k * Bp + l] = Jn;
}

__device__ __forceinline__ void fail_lane(const SolverCtl& a, int64_t l, int32_t* status, int32_t* res_buf) {
    status[l] = GYM_LS_FAILED;  // no update (:367-369): the result is the current trajectory
    res_buf[l] = a.k & 1;
}

// The per-lane state and streams one Armijo trial touches.
struct TrialIO {
    const double2* x;   // current trajectory (only x_0 is read)
    const double* u;    // current control planes (u0 is read)
    double2* xn;        // candidate trajectory (written)
    double* un;         // candidate controls (written)
};

// Armijo trial 1 (gamma0) fused with the candidate rollout and its cost (:352-365, first pass).
template <bool U0Z, bool CK>
__device__ __forceinline__ void trial_solver(const Dyn& m, const KW& w, const SolverCtl& a, const TrialIO& io,
                                             const double2* __restrict__ K1, const double* __restrict__ cs,
                                             const double* __restrict__ xr, const double* __restrict__ ur,
                                             double* __restrict__ cost, const double* __restrict__ dJ,
                                             const double* __restrict__ smax, double* __restrict__ gamma,
                                             int32_t* __restrict__ status, int32_t* __restrict__ n_iter,
                                             int32_t* __restrict__ res_buf, int32_t* __restrict__ n_roll,
                                             int32_t* __restrict__ retry_list, int32_t* __restrict__ counter,
                                             double* __restrict__ hist_cost, int64_t l, int64_t Bp, int N) {
    const double2 xa = io.x[wix(0, 0, 2, l, Bp)], xb = io.x[wix(0, 1, 2, l, Bp)];
    const double g = a.gamma0;
    const double Jn = rollout_cform<true, U0Z, false, CK>(m, w, io.u, K1, cs, xr, ur, io.xn, io.un, g, g, l, Bp, N,
                                                          xa.x, xa.y, xb.x, xb.y);
    // trial 1's outcome; k_nt_phase holds a second copy (a shared function changes that kernel's machine code)
    n_roll[l] += 1;
    if (Jn < cost[l] + a.c * g * dJ[l]) {  // strict Armijo test (:361)
        n_iter[l] += 1;
        accept_lane(a, l, Jn, g, smax[l], cost, gamma, status, res_buf, hist_cost, Bp);
    } else if (a.max_ls > 1) {
        retry_list[atomicAdd(counter, 1)] = (int32_t)l;
    } else {
        n_iter[l] += 1;
        fail_lane(a, l, status, res_buf);
    }
}

template <bool U0Z, bool CK, bool RL = false>
__global__ __launch_bounds__(BLK, 4) void k_nt_trial(Dyn m, KW w, SolverCtl a, TrialIO io,
                                                     const double2* __restrict__ K1, const double* __restrict__ cs,
                                                     const double* __restrict__ xr, const double* __restrict__ ur,
                                                     double* __restrict__ cost, const double* __restrict__ dJ,
                                                     const double* __restrict__ smax, double* __restrict__ gamma,
                                                     int32_t* __restrict__ status, int32_t* __restrict__ n_iter,
                                                     int32_t* __restrict__ res_buf, int32_t* __restrict__ n_roll,
                                                     int32_t* __restrict__ retry_list, int32_t* __restrict__ counter,
                                                     double* __restrict__ hist_cost, Range rg, int64_t Bp, int N) {
    const int64_t l = rg.lo + (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= rg.hi || status[l] != GYM_ACTIVE) return;
    GYM_TRACE_WAVE(1);
    trial_solver<U0Z, CK>(m, w, a, io, K1, cs, lane_ref<RL>(xr, l, 4 * (int64_t)N), lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)),
                          cost, dJ, smax, gamma, status, n_iter, res_buf, n_roll,
                      retry_list + rg.lo, counter, hist_cost, l, Bp, N);
}

// One pipeline phase: the first nb_b workgroups run the backward sweep of one half, the rest run the
// Armijo trial of the other half.  The sweep is HBM-bound and the trial fp64-VALU-bound, so co-resident
// waves of the two kinds overlap memory and arithmetic on every CU.  The two halves' lanes are disjoint.
// Every operand is in one by-value argument struct, re-read from the kernel-argument segment at each use
// (kernarg<PhaseArgs>(), as the persistent kernels do): no pointer or control value is held in SGPRs across
// the stage loops, where their spills cost v_readlane VALU slots (13 per trial stage before; 1 now;
// same-box A/B +0.3%).
struct PhaseArgs {
    Dyn m;
    KW w;
    SolverCtl a;
    TrialIO io;
    const double2* xb_in;
    const double* ub_in;
    double2* K1;
    double* cs;
    const double* xr;
    const double* ur;
    double *cost, *dJ, *smax, *gamma;
    int32_t *status, *n_iter, *res_buf, *n_roll, *retry_list, *counter;
    double *hist_cost, *hist_smax;
    Range rb, rt;
    int64_t Bp;
    int32_t N, kb, nb_b, pad;
};
static_assert(offsetof(PhaseArgs, w) == 96, "kernarg layout: KW at byte 96 (kernarg_consts)");
typedef const PhaseArgs* pargs_t;

// LO: the phase for at most two wavefronts per SIMD (gym_newton_phase's choice by the launch's size), compiled for
// two (up to 256 VGPRs) with both stage loops prefetching two stages ahead (three stream sets in rotation): with
// half the headline's waves a stage's loads must be issued further ahead to keep as many bytes in flight.  The same
// arithmetic in the same order (the same bits; tests/test_gpu_workloads.py).  Not with CK.
template <bool U0Z, bool CK, bool RL = false, bool LO = false>
__global__ __launch_bounds__(BLK, LO ? 2 : 4) void k_nt_phase(PhaseArgs args) {
    constexpr int PD = LO && !CK ? 2 : 1;
    GYM_CK_LDS(CK, U0Z);
    if ((int)blockIdx.x < args.nb_b) {
        const int64_t l = args.rb.lo + (int64_t)blockIdx.x * BLK + threadIdx.x;
        if (l >= args.rb.hi || args.status[l] != GYM_ACTIVE) return;
        double d, s;
        {
            const pargs_t R = kernarg<PhaseArgs>();
            const double* xr = lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N);
            const double* ur = lane_ref<RL>(R->ur, l, 2 * (int64_t)(R->N - 1));
            if (CK)
                backward_solver_lane_ck<U0Z, OUT_SOLVER>(R->m, R->w, R->xb_in, R->ub_in, xr, ur, R->K1, R->cs,
                                                         R->a.gamma0, ck_lds, l, R->Bp, R->N, d, s);
            else
                backward_solver_lane<U0Z, OUT_SOLVER, true, PD>(R->m, R->w, R->xb_in, R->ub_in, xr, ur, R->K1,
                                                                R->cs, R->a.gamma0, l, R->Bp, R->N, d, s);
        }
        const pargs_t Q = kernarg<PhaseArgs>();
        Q->dJ[l] = d;
        Q->smax[l] = s;
        if (Q->hist_smax && Q->kb < Q->a.hist_len) Q->hist_smax[(int64_t)Q->kb * Q->Bp + l] = s;
    } else {
        const int64_t l = args.rt.lo + (int64_t)(blockIdx.x - args.nb_b) * BLK + threadIdx.x;
        if (l >= args.rt.hi || args.status[l] != GYM_ACTIVE) return;
        double Jn;
        {   // Armijo trial 1 (gamma0) fused with the candidate rollout and its cost (:352-365, first pass)
            const pargs_t R = kernarg<PhaseArgs>();
            const double2 xa = R->io.x[wix(0, 0, 2, l, R->Bp)], xb = R->io.x[wix(0, 1, 2, l, R->Bp)];
            Jn = rollout_cform<true, U0Z, false, CK, kNT, true, PD>(
                R->m, R->w, R->io.u, R->K1, R->cs, lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N),
                lane_ref<RL>(R->ur, l, 2 * (int64_t)(R->N - 1)), R->io.xn, R->io.un, R->a.gamma0, R->a.gamma0, l,
                R->Bp, R->N, xa.x, xa.y, xb.x, xb.y);
        }
        const pargs_t R = kernarg<PhaseArgs>();
        const SolverCtl a = R->a;
        const double g = a.gamma0;
        // trial 1's outcome, as in trial_solver (operands re-read from the kernarg segment: kept as its own copy)
        R->n_roll[l] += 1;
        if (Jn < R->cost[l] + a.c * g * R->dJ[l]) {  // strict Armijo test (:361)
            R->n_iter[l] += 1;
            accept_lane(a, l, Jn, g, R->smax[l], R->cost, R->gamma, R->status, R->res_buf, R->hist_cost, R->Bp);
        } else if (a.max_ls > 1) {
            R->retry_list[R->rt.lo + atomicAdd(R->counter, 1)] = (int32_t)l;
        } else {
            R->n_iter[l] += 1;
            fail_lane(a, l, R->status, R->res_buf);
        }
    }
}

// Armijo trials 2..max_ls evaluated in parallel: one thread per (lane, j), cost only.
template <bool U0Z, bool RL = false>
__global__ __launch_bounds__(BLK) void k_nt_candidates(Dyn m, KW w, SolverCtl a, TrialIO io,
                                                       const double2* __restrict__ K1, const double* __restrict__ cs,
                                                       const double* __restrict__ xr, const double* __restrict__ ur,
                                                       const double* __restrict__ cost, const double* __restrict__ dJ,
                                                       const int32_t* __restrict__ retry_list,
                                                       const int32_t* __restrict__ counter,
                                                       uint8_t* __restrict__ cand_ok, int64_t Bp, int N) {
    const int nj = a.max_ls - 1;
    const int64_t total = (int64_t)(*counter) * nj;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLK) {
        const int64_t r = i / nj;
        const int j = 1 + (int)(i % nj);
        const int64_t l = retry_list[r];
        double g = a.gamma0;
        for (int q = 0; q < j; ++q) g *= a.beta;  // gamma_i *= beta, sequentially (:365)
        const double2 xa = io.x[wix(0, 0, 2, l, Bp)], xb = io.x[wix(0, 1, 2, l, Bp)];
        const double Jn = rollout_cform<false, U0Z, true>(m, w, io.u, K1, cs, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                                          lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), nullptr, nullptr,
                                                          g, a.gamma0, l, Bp, N, xa.x, xa.y, xb.x, xb.y);
        cand_ok[(int64_t)j * Bp + l] = (Jn < cost[l] + a.c * g * dJ[l]) ? 1 : 0;
    }
}

// Candidate scratch (gym_batch.cand_scratch, ABI 13): slot v holds candidate v's trajectory x (N, V/64, 2, 64) double2,
// controls u (T, 2, V) planes and cost J (V); V = 0: no scratch (every accepted candidate is re-run).
struct CandScratch {
    double2* sx;
    double* su;
    double* sJ;
    int64_t V;
};

// Armijo trials 2..max_ls on lane PAIRS: candidate i = r (max_ls - 1) + j - 1 (retry-list entry r, step gamma0 beta^j)
// on lanes (2q, 2q + 1) of a wavefront, the offset-form feedback and gym::rk4_pair_fast -- the chain of
// k_nt_candidates' single-lane rollout_cform<false, U0Z, true> with the joint-angle trigonometry split over the pair
// (the same operations, the same bits).  Candidate i's trajectory, controls and cost also go to scratch slot i while
// i < V, so that k_nt_retry copies the accepted one instead of re-running its chain.  The candidates of a launch
// are few lanes' (most iterations of a hard solve have 0-30 lanes backtracking), so each launch is one chain long:
// this halves the post-trial chains (candidates, then a copy instead of a second chain).  Stress workload, same
// process (tools/cand_ab.py, profiles/r04/cand/): +6.3% against re-running the accepted candidate; the candidates
// launch 42.5 ms per 193 sampled launches on pairs with the stores, 47.5 on single lanes with the stores, 39.1 for the
// former single-lane cost-only chain.
template <bool U0Z, bool RL = false>
__global__ __launch_bounds__(BLK) void k_nt_cand_pair(Dyn m, KW w, SolverCtl a, TrialIO io,
                                                      const double2* __restrict__ K1, const double* __restrict__ cs,
                                                      const double* __restrict__ xr, const double* __restrict__ ur,
                                                      const double* __restrict__ cost, const double* __restrict__ dJ,
                                                      const int32_t* __restrict__ retry_list,
                                                      const int32_t* __restrict__ counter,
                                                      uint8_t* __restrict__ cand_ok, CandScratch sc, int64_t Bp, int N) {
    const int nj = a.max_ls - 1;
    const int64_t total = (int64_t)(*counter) * nj;
    const int T = N - 1;
    const bool odd = threadIdx.x & 1;
    const uint32_t srow = (uint32_t)sc.V * 16u, splane = (uint32_t)sc.V * 8u;
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Kb = reinterpret_cast<const char*>(K1);
    const char* Cb = reinterpret_cast<const char*>(cs);
    const char* Ub = reinterpret_cast<const char*>(io.u);
    const char* Xs = reinterpret_cast<const char*>(sc.sx);
    const char* Us = reinterpret_cast<const char*>(sc.su);
    const gym::PolyRegs pk = gym::poly_vgprs_all();
    Dyn dm = m;
    gym::in_vgpr(dm.b); gym::in_vgpr(dm.d); gym::in_vgpr(dm.a2b); gym::in_vgpr(dm.bb); gym::in_vgpr(dm.dad);
    gym::in_vgpr(dm.g1); gym::in_vgpr(dm.g2); gym::in_vgpr(dm.f1); gym::in_vgpr(dm.f2); gym::in_vgpr(dm.h);
    gym::in_vgpr(dm.h2); gym::in_vgpr(dm.h6);
    // wave-uniform trip count: every lane of the wavefront runs the pair step (DPP partners, its ballot)
    for (int64_t base = (int64_t)blockIdx.x * (BLK / 2); base < total; base += (int64_t)gridDim.x * (BLK / 2)) {
        const int64_t i0 = base + (threadIdx.x >> 1);
        const bool act = i0 < total;
        const int64_t i = act ? i0 : total - 1;          // a padding pair repeats the last candidate, unrecorded
        const int64_t r = i / nj;
        const int j = 1 + (int)(i % nj);
        const int64_t l = retry_list[r];
        double g = a.gamma0;
        for (int q = 0; q < j; ++q) g *= a.beta;         // gamma_i *= beta, sequentially (:365)
        const double dg = g - a.gamma0;
        // this candidate's trajectory into slot i: the even lane stores (th1, th2) and the controls, the odd lane
        // (w1, w2).  A store that must not land gets an offset past the buffer resource's range, which the
        // hardware drops -- no branch around the stores, so the loop's wait counts stay exact (a store under a
        // divergent branch would make the compiler wait for every store before the next stage's operands).
        const bool keep = act && i < sc.V;
        constexpr uint32_t OOB = 0x80000000u;            // > the resources' num_records (0x7fffffff)
        const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
        const uint32_t v2 = keep ? wbo(i, 2) + (odd ? WROW : 0u) : OOB;
        const uint32_t v1o = keep && !odd ? (uint32_t)i * 8u : OOB;
        const double* xrl = lane_ref<RL>(xr, l, 4 * (int64_t)N);
        const double* url = lane_ref<RL>(ur, l, 2 * (int64_t)T);
        const double2 xa = io.x[wix(0, 0, 2, l, Bp)], xb = io.x[wix(0, 1, 2, l, Bp)];
        double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
        bst2(rsrc(Xs), v2, 0, odd ? n2 : n0, odd ? n3 : n1);
        auto fetch = [&](TrialStage& q, int t) {
            const auto rK = rsrc(Kb + (int64_t)t * (2 * (int64_t)row));
            q.k0 = bld2(rK, o2, 0);
            q.k1 = bld2(rK, o2, WROW);
            const auto rC = rsrc(Cb + (int64_t)t * row);
            q.cg = bld1(rC, o1, 0);
            q.s1 = bld1(rC, o1, plane);
            q.u0 = U0Z ? 0.0 : bld1(rsrc(Ub + (int64_t)t * row), o1, 0);
        };
        const double G00 = w.G00, iG00 = w.iG00;
        double J = 0.0;
        TrialStage pre;
        fetch(pre, 0);
        for (int t = 0; t < T; ++t) {
            const TrialStage q = pre;
            if (t + 1 < T) fetch(pre, t + 1);
            const double* urt = url + 2 * t;
            const double v0 = U0Z ? 0.0 : trial_u0(q.u0, urt[0], g, G00, iG00);   // U0Z: +0 exactly
            const double v1 = trial_u1_sig(q.k0, q.k1, q.cg, q.s1, dg, n0, n1, n2, n3);
            const double f0 = U0Z ? 0.0 : v0 - urt[0], f1 = v1 - urt[1];
            J = stage_cost<U0Z>(J, w.Q, w.R, n0, n1, n2, n3, xrl + 4 * t, f0, f1);
            {
                const auto rO = rsrc(Us + (int64_t)t * srow);
                if (!U0Z) bst1(rO, v1o, 0, v0);
                bst1(rO, v1o, splane, v1);
            }
            gym::rk4_pair_fast<true>(dm, odd, n0, n1, n2, n3, v1, pk);
            bst2(rsrc(Xs + (int64_t)(t + 1) * (2 * (int64_t)srow)), v2, 0, odd ? n2 : n0, odd ? n3 : n1);
        }
        const double Jn = J + xcost(w.QT, n0, n1, n2, n3, xrl + 4 * T);
        if (act && !odd) {
            cand_ok[(int64_t)j * Bp + l] = (Jn < cost[l] + a.c * g * dJ[l]) ? 1 : 0;
            if (keep) sc.sJ[i] = Jn;
        }
    }
}

// First accepted candidate per retry lane: its trajectory into the lane's next iterate (io.xn / io.un), the lane
// updated.  Work items: first one head item per retry-list entry r (its bookkeeping; without a scratch slot for its
// accepted candidate -- V = 0, or a slot index past V -- the re-run of that candidate writing the trajectory, its
// rollout_cform: the same bits as the copy), then, with scratch, one copy item per entry and knot chunk (CPK knots).
// Head items on consecutive threads: the re-runs of a launch with more backtracking lanes than slots run side by
// side, one chain each (with the copy items interleaved, a thread could draw several: stress trace, launches of
// up to 2.2 ms).
constexpr int CPK = 8;   // knots per copy item
template <bool U0Z, bool CK, bool RL = false>
__global__ __launch_bounds__(BLK) void k_nt_retry(Dyn m, KW w, SolverCtl a, TrialIO io,
                                                  const double2* __restrict__ K1, const double* __restrict__ cs,
                                                  const double* __restrict__ xr, const double* __restrict__ ur,
                                                  double* __restrict__ cost, const double* __restrict__ smax,
                                                  double* __restrict__ gamma, int32_t* __restrict__ status,
                                                  int32_t* __restrict__ n_iter, int32_t* __restrict__ res_buf,
                                                  int32_t* __restrict__ n_roll, const int32_t* __restrict__ retry_list,
                                                  const int32_t* __restrict__ counter,
                                                  const uint8_t* __restrict__ cand_ok, double* __restrict__ hist_cost,
                                                  CandScratch sc, int64_t Bp, int N) {
    const int nr = *counter;
    const int nj = a.max_ls - 1;
    const int T = N - 1;
    const int nc = sc.V > 0 ? (N + CPK - 1) / CPK : 0;   // copy items per retry lane
    const int64_t total = (int64_t)nr * (1 + nc);
    for (int64_t it = (int64_t)blockIdx.x * BLK + threadIdx.x; it < total; it += (int64_t)gridDim.x * BLK) {
        const bool head = it < nr;
        const int64_t ri = head ? it : (it - nr) / nc;
        const int c = head ? 0 : (int)((it - nr) % nc);
        const int64_t l = retry_list[ri];
        int jacc = 0;                                    // the first accepted candidate (0: none)
        for (int j0 = 1; j0 <= nj && jacc == 0; j0 += 8) {   // eight independent byte loads per round
            uint8_t ok[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) ok[q] = j0 + q <= nj ? cand_ok[(int64_t)(j0 + q) * Bp + l] : 0;
#pragma unroll
            for (int q = 7; q >= 0; --q)
                if (ok[q]) jacc = j0 + q;
        }
        const int64_t v = ri * nj + jacc - 1;
        const bool copy = jacc > 0 && v < sc.V;
        if (!head) {
            if (copy) {
#pragma unroll
                for (int q = 0; q < CPK; ++q) {
                    const int t = c * CPK + q;
                    if (t < N) {
                        io.xn[wix(t, 0, 2, l, Bp)] = sc.sx[wix(t, 0, 2, v, sc.V)];
                        io.xn[wix(t, 1, 2, l, Bp)] = sc.sx[wix(t, 1, 2, v, sc.V)];
                    }
                    if (t < T) {
                        if (!U0Z) io.un[pix(t, 0, 2, l, Bp)] = sc.su[pix(t, 0, 2, v, sc.V)];
                        io.un[pix(t, 1, 2, l, Bp)] = sc.su[pix(t, 1, 2, v, sc.V)];
                    }
                }
            }
            continue;
        }
        n_iter[l] += 1;
        if (jacc == 0) {
            n_roll[l] += nj;
            fail_lane(a, l, status, res_buf);
            continue;
        }
        n_roll[l] += jacc;
        double g = a.gamma0;
        for (int q = 0; q < jacc; ++q) g *= a.beta;
        double Jn;
        if (copy) {
            Jn = sc.sJ[v];
        } else {
            const double2 xa = io.x[wix(0, 0, 2, l, Bp)], xb = io.x[wix(0, 1, 2, l, Bp)];
            Jn = rollout_cform<true, U0Z, true, CK>(m, w, io.u, K1, cs, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                                    lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), io.xn, io.un, g,
                                                    a.gamma0, l, Bp, N, xa.x, xa.y, xb.x, xb.y);
        }
        accept_lane(a, l, Jn, g, smax[l], cost, gamma, status, res_buf, hist_cost, Bp);
    }
}
