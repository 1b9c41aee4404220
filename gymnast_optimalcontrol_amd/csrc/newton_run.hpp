// Newton solver kernels: the persistent schedule (k_nt_run, k_nt_run2).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// Persistent schedule (gym_newton_run): every lane runs its own outer iterations k0 .. k1-1 of
// newton_Algorithm (:329-396) back to back inside ONE launch -- sweep, Armijo trial 1, and only for a lane
// that rejects it the sigma1 re-run and trials 2..max_ls one after another (:352-365), exactly the
// sequential search of the reference.  Lanes are independent problems, so nothing orders one lane's
// iteration against another's: the only dependences are the lane's own stores -> loads through K1 / cs
// (sweep -> trial) and x / u (trial -> next sweep), ordered by a fence per pass.  The waves of a SIMD drift
// apart and mix sweep (HBM-heavy) and trial (fp64-heavy) passes by themselves, with no launch boundary, tail
// or host round trip per iteration.  Per lane the arithmetic is the other schedules' (same device functions):
// bit-identical results.  No wave priority bands (measured: the phase kernels' per-pass bands 4-8% slower here,
// each pass restarting at priority 3 undoes them; cyclic bands of the iteration count no faster than none).
// The kernel serves batches of at most 128 lanes per CU (the solver's default: 64), i.e. at most one wavefront per
// SIMD, so it is compiled for one (__launch_bounds__(BLK, 1)), and its sweep interleaves stage t-1's Jacobian with
// stage t's Riccati update (backward_solver_lane_ilp).
// ------------------------------------------------------------------------------------------
// Everything the kernel needs beyond the stage loops' own operands is one by-value struct whose fields are
// re-read from the kernel-argument segment at each use (kernarg<RunArgs>(): scalar loads behind an opaque pointer),
// so that none of its ~20 pointers is held in SGPRs across the stage loops (spilled, they cost v_readlane
// VALU slots in every stage).  Dyn and KW come first: kernarg_consts() reads them at offsets 0 and 96.
// LaneArgs: the part RunArgs and TailArgs share (their leading bytes), filled by one host function (lane_args).
struct LaneArgs {
    Dyn m;
    KW w;
    SolverCtl a;
    double2* x[2];
    double* u[2];
    double2* K1;
    double* cs;
    const double* xr;
    const double* ur;
    double *cost, *dJ, *smax, *gamma;
    int32_t *status, *n_iter, *res_buf, *n_roll;
    double *hist_cost, *hist_smax;
};
static_assert(offsetof(LaneArgs, w) == 96, "kernarg layout: KW at byte 96 (kernarg_consts)");
struct RunArgs : LaneArgs {
    int32_t *retry_list, *counter;   // ext: the lanes that reject trial 1 (GYM_FLAG_SIGMA_STREAM)
    int64_t B, Bp;
    int32_t N, k0, k1, ext;
};
static_assert(sizeof(RunArgs) == sizeof(LaneArgs) + 48, "kernarg layout: LaneArgs, then RunArgs' own fields");
typedef const RunArgs* rargs_t;

// the lane's reference rows in the persistent kernels (per-lane references: GYM_FLAG_REF_LANE)
template <bool RL>
__device__ __forceinline__ const double* run_xr(rargs_t R, int64_t l) {
    return lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N);
}
template <bool RL>
__device__ __forceinline__ const double* run_ur(rargs_t R, int64_t l) {
    return lane_ref<RL>(R->ur, l, 2 * (int64_t)(R->N - 1));
}

__device__ __forceinline__ void lane_fence() {   // this lane's stores visible to its own later loads
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}

#ifdef GYM_RUN2_TRACE
// Diagnostic build only (tools/run2_trace.py): per workgroup and wavefront role, cycles (s_memtime) spent in the
// sweep, the trial and the post-trial part, accumulated in registers and written once at the kernel's end.
__device__ unsigned long long g_run2_trace[8192][2][6];
#endif
#if defined(GYM_RUN2_TRACE) || defined(GYM_TAIL_TRACE)
#define R2T_NOW() __builtin_amdgcn_s_memtime()
#else
#define R2T_NOW() 0ull
#endif
template <bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_run(RunArgs args) {
    constexpr bool BAND = false;
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= args.B) return;
    // Nothing but the lane index, the iteration counter and the lane's status stays live across a pass: J, dJ,
    // max|sigma| and x_0 are re-read from memory where needed (once per iteration).
    int st = kernarg<RunArgs>()->status[l];
    unsigned long long acc[4] = {0, 0, 0, 0};   // GYM_RUN2_TRACE only: sweep / trial / post cycles, iterations
    for (int k = kernarg<RunArgs>()->k0; st == GYM_ACTIVE && k < kernarg<RunArgs>()->k1; ++k) {
        unsigned long long tt = R2T_NOW();
        ++acc[3];
        const int cb = k & 1;
        {
            const rargs_t R = kernarg<RunArgs>();
            double d, s;
            backward_solver_lane_ilp<U0Z, OUT_SOLVER>(R->m, R->w, R->x[cb], R->u[cb], run_xr<RL>(R, l),
                                                      run_ur<RL>(R, l), R->K1,
                                                      R->cs, R->a.gamma0, l, R->Bp, R->N, d, s);
            const rargs_t Q = kernarg<RunArgs>();
            Q->dJ[l] = d;
            Q->smax[l] = s;
            if (Q->hist_smax && k < Q->a.hist_len) Q->hist_smax[(int64_t)k * Q->Bp + l] = s;
        }
        lane_fence();
        acc[0] += R2T_NOW() - tt;
        tt = R2T_NOW();
        double Jn;
        {
            const rargs_t R = kernarg<RunArgs>();
            const double2 xa = R->x[cb][wix(0, 0, 2, l, R->Bp)], xb = R->x[cb][wix(0, 1, 2, l, R->Bp)];
            Jn = rollout_cform<true, U0Z, false, false, kNT, BAND>(R->m, R->w, R->u[cb], R->K1, R->cs,
                                                                   run_xr<RL>(R, l), run_ur<RL>(R, l),
                                                                   R->x[cb ^ 1], R->u[cb ^ 1], R->a.gamma0,
                                                                   R->a.gamma0, l, R->Bp, R->N, xa.x, xa.y, xb.x, xb.y);
        }
        acc[1] += R2T_NOW() - tt;
        const rargs_t R = kernarg<RunArgs>();
        double g = R->a.gamma0;
        int nr = 1;
        bool ok = Jn < R->cost[l] + R->a.c * g * R->dJ[l];   // strict Armijo test (:361)
        if (!ok && R->a.max_ls > 1) {
            // sigma1 of this sweep (not streamed): the sweep re-run, same code and inputs -> the same bits
            {
                const rargs_t P = kernarg<RunArgs>();
                double d2, s2;
                backward_solver_lane<U0Z, OUT_SIGMA, BAND>(P->m, P->w, P->x[cb], P->u[cb], run_xr<RL>(P, l),
                                                           run_ur<RL>(P, l), P->K1,
                                                           P->cs, 0.0, l, P->Bp, P->N, d2, s2);
            }
            lane_fence();
            for (int j = 1; !ok && j < kernarg<RunArgs>()->a.max_ls; ++j) {
                const rargs_t P = kernarg<RunArgs>();
                g *= P->a.beta;   // gamma_i *= beta, sequentially (:365)
                const double2 xa = P->x[cb][wix(0, 0, 2, l, P->Bp)], xb = P->x[cb][wix(0, 1, 2, l, P->Bp)];
                Jn = rollout_cform<true, U0Z, true, false, kNT, BAND>(P->m, P->w, P->u[cb], P->K1, P->cs,
                                                                      run_xr<RL>(P, l), run_ur<RL>(P, l), P->x[cb ^ 1], P->u[cb ^ 1], g,
                                                                      P->a.gamma0, l, P->Bp, P->N, xa.x, xa.y, xb.x,
                                                                      xb.y);
                ++nr;
                const rargs_t Q = kernarg<RunArgs>();
                ok = Jn < Q->cost[l] + Q->a.c * g * Q->dJ[l];
            }
        }
        const rargs_t F = kernarg<RunArgs>();
        F->n_roll[l] += nr;
        F->n_iter[l] += 1;
        SolverCtl c = F->a;
        c.k = k;
        if (ok) {
            const double s = F->smax[l];
            accept_lane(c, l, Jn, g, s, F->cost, F->gamma, F->status, F->res_buf, F->hist_cost, F->Bp);
            if (s < c.tol) st = GYM_CONVERGED;
        } else {
            fail_lane(c, l, F->status, F->res_buf);
            st = GYM_LS_FAILED;
        }
        lane_fence();   // the candidate buffer is the next sweep's input
    }
#ifdef GYM_RUN2_TRACE
    if (threadIdx.x == 0 && blockIdx.x < 8192)
        for (int i = 0; i < 4; ++i) g_run2_trace[blockIdx.x][0][i] = acc[i];
#endif
}

// ------------------------------------------------------------------------------------------
// Persistent schedule on TWO wavefronts per 64 lanes (k_nt_run2, the default persistent kernel).
// In the latency-bound regime (BASELINE cfg 2: 4,096 lanes = 64 wavefronts on 1,024 SIMDs) every wavefront is
// alone on its SIMD and issues about one fp64 instruction per 4.4-5 cycles (profiles/r02_probe/README.md), so a
// stage costs its instruction count.  A second wavefront per 64 lanes, on another SIMD, takes every instruction
// that is not on the lane's dependency chain:
//   sweep : the helper evaluates stage t's Jacobian and linearisation (stage_lin: a function of x_t, u_t only)
//           and hands them, with x_t and u_t, to the main wavefront through an LDS ring; the main wavefront runs
//           only the Riccati recursion (step_lin) and stores K row 1 / cg;
//   trial : the main wavefront runs the feedback + RK4 chain and hands (x_{t+1}, u1_t) to the helper, which
//           forms u0, accumulates the cost and stores the candidate trajectory.
// The two advance in chunks of R2C stages, the producer one chunk ahead (two chunks of ring slots), separated by
// workgroup barriers; a chunk's ring slots hold R2W pairs per lane ([slot][pair][lane]: one 1 KiB row per wave
// instruction).  Per lane the arithmetic is the single-wavefront kernel's -- the same functions (jacobian,
// stage_lin, step_lin, trial_u0 / trial_u1, stage_cost, rk4), each contracting FMAs inside its expressions only
// -- so the results are the same bits.  The rare Armijo retries (sigma1 re-run, trials 2..20) run on the main
// wavefront alone, with the single-wavefront code, while the helper waits at the end-of-iteration barrier.
// Lanes that are not active (finished, padding) run along without storing anything: every barrier is reached by
// every thread, and the iteration loop ends when no lane of the workgroup is active.
// ------------------------------------------------------------------------------------------
constexpr int R2C = 2;            // stages per chunk (even)
constexpr int R2S = 3 * R2C;      // ring slots (the trial uses two chunks of them, the split sweep three)
constexpr int R2W = 11;           // pairs per lane and slot: sweep x_t (2), u_t, Lin (8); trial x_{t+1} (2), u1_t
// The sweep's Riccati update is split over two wavefronts: the main one runs only the matrix half (Sweep::step_P:
// gain row, P) and hands k, G11, 1/G11 to the pair wavefront, which runs the vector half (step_p: sigma, dJ, p,
// ||sigma||) and the K1 / cg stores one chunk behind.  Nothing flows back, so the main wavefront's chain loses the
// vector half, the stores and 6 of its 11 ring reads per stage.  The helpers' ring is three chunks deep (the pair
// wavefront reads chunk c - 1 while the main one reads c and the helpers write c + 1).
constexpr int R2RD = 3;           // helper ring depth in chunks (sweep)
// Prefetch distance of the producers' stream loads, in stages (= register sets in rotation).  A stage of either
// wavefront is ~2x shorter than the single-wavefront kernel's, and the loads of data the previous pass wrote
// take ~1 us: with one stage of prefetch both passes ran at the load latency (~2,400 cycles per stage measured,
// whatever the instruction count, tools/run2_trace.py).
constexpr int R2PD = 4;
static_assert(R2PD % R2C == 0, "the prefetch distance is a whole number of chunks");
// chunks per pass, rounded up to whole register-set rotations: producer and consumer both run this many chunk
// phases (the consumer skips the stages past T), so their barrier counts match
// a stage index the compiler may compute on the VALU (e.g. a clamp as v_sub_u32 ... clamp) made wave-uniform
// again: a buffer resource built from a VGPR value becomes a waterfall loop of v_readfirstlane
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// x_ref / u_ref rows through the constant address space: the compiler then reads a stage's row with scalar loads
// (it cannot prove that no store of the kernel clobbers a plain global pointer, and falls back to vector loads
// that count in vmcnt -- and the stage then waits for them behind its prefetches)
typedef const __attribute__((address_space(4))) double* cptr_t;
template <int NV>
struct Row {
    double v[NV];
};
template <int NV>
__device__ __forceinline__ Row<NV> const_row(const double* base, int t) {
    const cptr_t p = (cptr_t)base + (int64_t)NV * t;
    Row<NV> r;
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = p[i];
    return r;
}
// ... or, for per-lane references, the lane's own row (vector loads)
template <int NV, bool RL>
__device__ __forceinline__ Row<NV> ref_row(const double* base, int t) {
    if (!RL) return const_row<NV>(base, t);
    Row<NV> r;
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = base[(int64_t)NV * t + i];
    return r;
}
__device__ __forceinline__ void in_vgpr2(double2& v) { asm volatile("" : "+v"(v.x), "+v"(v.y)); }
__device__ __forceinline__ int run2_chunks(int T) {
    constexpr int per = R2PD / R2C;
    return ((T + R2C - 1) / R2C + per - 1) / per * per;
}
typedef double2 (*ring_t)[R2W][BLK];

// The chunk hand-off: this wavefront's LDS writes complete, then the workgroup barrier.  Not __syncthreads(): its
// workgroup-scope release also drains every outstanding global load and store (s_waitcnt vmcnt(0)), i.e. the
// next stages' prefetches and the last stores' round trip at every chunk.  Only LDS crosses between the two
// wavefronts inside a pass; global memory is handed over at the iteration's end (lane_fence + __syncthreads).
// The "memory" clobber keeps the compiler from moving LDS accesses across it.
__device__ __forceinline__ void lds_barrier(unsigned long long& wait) {
    const unsigned long long t0 = R2T_NOW();
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    wait += R2T_NOW() - t0;   // GYM_RUN2_TRACE only (otherwise 0 + 0: removed)
}

// helper wavefront HID of NH, sweep: the stages i = HID, HID + NH, ... of the reverse pass (t = T-1-i) into slot
// (chunk & 1) * R2C + (i % R2C)
template <bool U0Z, int HID, int NH, bool RL>
__device__ __forceinline__ void run2_sweep_helper(ring_t ring, int lane, int64_t l, int cb, const double* __restrict__ xr,
                                                  const double* __restrict__ ur, unsigned long long& bw) {
    const rargs_t R = kernarg<RunArgs>();
    const int T = R->N - 1;
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t row = (uint32_t)R->Bp * 16u, plane = (uint32_t)R->Bp * 8u;
    const char* Xb = reinterpret_cast<const char*>(R->x[cb]);
    const char* Ub = reinterpret_cast<const char*>(R->u[cb]);
    // x_ref / u_ref rows: wave-uniform scalar loads (restrict parameters: no store can alias them); per-lane
    // references (RL): the lane's own rows
    // the model, the weights stage_lin reads and every Horner coefficient held in VGPRs across the stage loop: no
    // per-stage kernel-argument loads (and their lgkmcnt(0) waits) and no per-use copies of scalar operands
    const gym::PolyRegs pk = gym::poly_vgprs_all();
    Dyn dm = R->m;
    KW wv = R->w;
    gym::in_vgpr(dm.b); gym::in_vgpr(dm.d); gym::in_vgpr(dm.a2b); gym::in_vgpr(dm.bb); gym::in_vgpr(dm.dad);
    gym::in_vgpr(dm.g1); gym::in_vgpr(dm.g2); gym::in_vgpr(dm.f1); gym::in_vgpr(dm.f2); gym::in_vgpr(dm.h);
    gym::in_vgpr(dm.h2); gym::in_vgpr(dm.h6);
    gym::in_vgpr(wv.twoQ[0]); gym::in_vgpr(wv.twoQ[1]); gym::in_vgpr(wv.twoQ[2]); gym::in_vgpr(wv.twoQ[3]);
    gym::in_vgpr(wv.G00); gym::in_vgpr(wv.twoR1);
    auto fetch = [&](SweepStage& q, int t) {
        const auto rX = rsrc(Xb + (int64_t)t * (2 * (int64_t)row)), rU = rsrc(Ub + (int64_t)t * row);
        q.xa = bld2(rX, o2, 0);
        q.xb = bld2(rX, o2, WROW);
        q.u0 = U0Z ? 0.0 : bld1(rU, o1, 0);
        q.u1 = bld1(rU, o1, plane);
    };
    auto produce = [&](const SweepStage& q, int t, int slot) {
        const gym::Jac J = gym::jacobian(dm, q.xa.x, q.xa.y, q.xb.x, q.xb.y, q.u1, pk);
        const Row<4> xrt = ref_row<4, RL>(xr, t);
        const Row<2> urt = ref_row<2, RL>(ur, t);
        const Lin L = stage_lin<U0Z>(dm, wv, J, q.xa, q.xb, q.u0, q.u1, xrt.v, urt.v);
        double2(*s)[BLK] = ring[slot];
        s[0][lane] = q.xa;                          s[1][lane] = q.xb;
        s[2][lane] = make_double2(q.u0, q.u1);      s[3][lane] = make_double2(L.A20, L.A21);
        s[4][lane] = make_double2(L.A22, L.A23);    s[5][lane] = make_double2(L.A30, L.A31);
        s[6][lane] = make_double2(L.A32, L.A33);    s[7][lane] = make_double2(L.bd2, L.bd3);
        s[8][lane] = make_double2(L.q0, L.q1);      s[9][lane] = make_double2(L.q2, L.q3);
        s[10][lane] = make_double2(L.r0, L.r1);
    };
    // Branch-free stream loads: every producer stage loads (a clamped stage index past the end), so the
    // compiler's wait-count tracking stays exact and a stage waits only for its own loads, R2PD stages old
    // (with loads on conditional paths it fell back to vmcnt(0) at every stage: the prefetch was void).
    static_assert(R2C % NH == 0, "every helper takes the same number of stages per chunk");
    const int nch = run2_chunks(T);
    SweepStage P[R2PD / NH];               // stage i's streams in set (i % R2PD) / NH, loaded R2PD stages ahead
#pragma unroll
    for (int j = HID; j < R2PD; j += NH) fetch(P[j / NH], uni(max(T - 1 - j, 0)));
    for (int c0 = 0; c0 < nch; c0 += R2PD / R2C) {
#pragma unroll
        for (int cc = 0; cc < R2PD / R2C; ++cc) {
            const int c = c0 + cc;
#pragma unroll
            for (int j = HID; j < R2C; j += NH) {
                const int i = c * R2C + j, set = (cc * R2C + j) / NH;
                // the stage's streams moved out of the loading registers first (the only wait: for this set, R2PD
                // stages old), so that the set is re-armed at once and every later use reads the copy
                SweepStage w = P[set];
                in_vgpr2(w.xa); in_vgpr2(w.xb); gym::in_vgpr(w.u0); gym::in_vgpr(w.u1);
                fetch(P[set], uni(max(T - 1 - (i + R2PD), 0)));
                produce(w, uni(max(T - 1 - i, 0)), (c % R2RD) * R2C + j);   // past the end: not consumed
            }
            lds_barrier(bw);
        }
    }
    lds_barrier(bw);
    lds_barrier(bw);                       // the vector half's last chunk
}

// main wavefront, sweep: the matrix half of the Riccati recursion (Sweep::step_P) from the ring's
// A_d rows and b; stage i's gain row, G11 and 1/G11 into the gain ring (slot (c & 1) * R2C + j) for the pair
// wavefront.  Chunk c between barriers c and c + 1, as run2_sweep_main.
typedef double2 (*gring_t)[3][BLK];
template <bool U0Z, bool RL>
__device__ __forceinline__ void run2_sweep_gain(ring_t ring, gring_t gring, int lane, int64_t l, int cb,
                                                unsigned long long& bw) {
    const rargs_t R = kernarg<RunArgs>();
    const int T = R->N - 1;
    const double2* x = R->x[cb];
    Sweep<false> S(R->w, x[wix(T, 0, 2, l, R->Bp)], x[wix(T, 1, 2, l, R->Bp)], run_xr<RL>(R, l) + 4 * T);
    const int nch = run2_chunks(T);
    KW wv = R->w;                          // step_P's weights and dt in VGPRs: no per-stage kernel-argument loads
    double dtv = R->m.h;
    gym::in_vgpr(wv.twoQ[0]); gym::in_vgpr(wv.twoQ[1]); gym::in_vgpr(wv.twoQ[2]); gym::in_vgpr(wv.twoQ[3]);
    gym::in_vgpr(wv.twoR1); gym::in_vgpr(dtv);
    lds_barrier(bw);                       // the helpers' chunk 0
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int j = 0; j < R2C; ++j) {
            const int i = c * R2C + j;
            if (i < T) {
                const double2(*s)[BLK] = ring[(c % R2RD) * R2C + j];
                const double2 a0 = s[3][lane], a1 = s[4][lane], a2 = s[5][lane], a3 = s[6][lane];
                const double2 bd = s[7][lane];
                const Lin L{a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y, bd.x, bd.y,
                            0.0, 0.0, 0.0, 0.0, 0.0, 0.0, dtv};      // q, r: the vector half's
                double k0, k1, k2, k3, G11, iG;
                S.step_P(wv, L, k0, k1, k2, k3, G11, iG);
                double2(*g)[BLK] = gring[(c & 1) * R2C + j];
                g[0][lane] = make_double2(k0, k1);
                g[1][lane] = make_double2(k2, k3);
                g[2][lane] = make_double2(G11, iG);
            }
        }
        lds_barrier(bw);
    }
    lds_barrier(bw);                       // the vector half's last chunk
}

// pair wavefront, sweep: the vector half (Sweep::step_p) of stage i from the helpers' ring (chunk
// c, still in its slot: three chunks deep) and the main wavefront's gain ring; K row 1 / cg stored for active lanes.
// Chunk c between barriers c + 1 and c + 2.
template <bool U0Z, bool RL>
__device__ __forceinline__ void run2_sweep_vec(ring_t ring, gring_t gring, int lane, int64_t l, int cb, bool act,
                                               double& dJ_out, double& smax_out, unsigned long long& bw) {
    const rargs_t R = kernarg<RunArgs>();
    const bool ext = R->ext != 0;
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t so2 = act ? o2 : 0x80000000u, so1 = act ? o1 : 0x80000000u;   // inactive: dropped (OOB)
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Kb = reinterpret_cast<const char*>(R->K1);
    const char* Cb = reinterpret_cast<const char*>(R->cs);
    const double g0 = R->a.gamma0;
    const double2* x = R->x[cb];
    Sweep<false> S(R->w, x[wix(T, 0, 2, l, Bp)], x[wix(T, 1, 2, l, Bp)], run_xr<RL>(R, l) + 4 * T);
    const int nch = run2_chunks(T);
    KW wv = R->w;                          // step_p's weights and dt in VGPRs: no per-stage kernel-argument loads
    double dtv = R->m.h;
    gym::in_vgpr(wv.iG00); gym::in_vgpr(dtv);
    lds_barrier(bw);                       // the helpers' chunk 0
    lds_barrier(bw);                       // the main wavefront's chunk 0
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int j = 0; j < R2C; ++j) {
            const int i = c * R2C + j;
            if (i < T) {
                const double2(*s)[BLK] = ring[(c % R2RD) * R2C + j];
                const double2 xa = s[0][lane], xb = s[1][lane], uu = s[2][lane];
                const double2 a0 = s[3][lane], a1 = s[4][lane], a2 = s[5][lane], a3 = s[6][lane];
                const double2 bd = s[7][lane], qa = s[8][lane], qb = s[9][lane], rr = s[10][lane];
                const double2(*g)[BLK] = gring[(c & 1) * R2C + j];
                const double2 ka01 = g[0][lane], ka23 = g[1][lane], gi = g[2][lane];
                const Lin L{a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y, bd.x, bd.y,
                            qa.x, qa.y, qb.x, qb.y, rr.x, rr.y, dtv};
                double s0, s1;
                S.step_p<U0Z>(wv, L, ka01.x, ka01.y, ka23.x, ka23.y, gi.x, gi.y, s0, s1);
                // an inactive lane's stores take an offset past the resources' range (dropped): no exec-mask branch
                if (ext)   // external retries: sigma1 stored too (the candidates read it; no re-run)
                    store_stage<OUT_ALL>(Kb, Cb, T - 1 - i, row, plane, so2, so1, xa, xb, uu.y, g0, ka01.x,
                                         ka01.y, ka23.x, ka23.y, s1);
                else
                    store_stage<OUT_SOLVER>(Kb, Cb, T - 1 - i, row, plane, so2, so1, xa, xb, uu.y, g0, ka01.x,
                                            ka01.y, ka23.x, ka23.y, s1);
            }
        }
        lds_barrier(bw);
    }
    dJ_out = S.dJ;
    smax_out = S.smax;
}

// The first Armijo trial's chain runs on lane pairs: two wavefronts share the 64 lanes' RK4 chains, trajectory
// tl (< 64) of the workgroup on lanes (2q, 2q+1) of wavefront tl / 32 with q = tl % 32; the even lane reduces /
// rotates th1, the odd lane th2 (gym::rk4_pair_fast, bit-identical to rk4).  The second sweep helper, idle in the
// trial, is the chains' loader.  It reads K row 1 and cg of the stages two chunks ahead from global memory and writes them into
// an LDS ring three chunks deep ([slot][k0, k1, cg][trajectory]); the two RK4-chain wavefronts read each stage's row
// from LDS one stage ahead and issue no global loads at all.  With the global loads on the chains the compiler's
// wait-count placement (loop rotation around the branchy RK4 step) waited for the most recent prefetches once per
// unrolled body: a load round trip on the chain.  The loader waits for its own loads, off every chain.
typedef double2 (*kring_t)[3][BLK];

// loader wavefront: chunks 0, 1 before the pass's leading barrier, chunk c + 2 during phase c
template <bool U0Z>
__device__ __forceinline__ void run2_trial_kload(kring_t kr, int lane, int64_t l, unsigned long long& bw) {
    const rargs_t R = kernarg<RunArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t row = (uint32_t)Bp * 16u;
    const char* Kb = reinterpret_cast<const char*>(R->K1);
    const char* Cb = reinterpret_cast<const char*>(R->cs);
    auto fetch = [&](TrialStage& q, int t) {
        const auto rK = rsrc(Kb + (int64_t)t * (2 * (int64_t)row));
        q.k0 = bld2(rK, o2, 0);
        q.k1 = bld2(rK, o2, WROW);
        q.cg = bld1(rsrc(Cb + (int64_t)t * row), o1, 0);
    };
    auto put = [&](const TrialStage& q, int slot) {
        kr[slot][0][lane] = q.k0;
        kr[slot][1][lane] = q.k1;
        kr[slot][2][lane] = make_double2(q.cg, 0.0);
    };
    const int nch = run2_chunks(T);
    {
        TrialStage P0[2 * R2C];
#pragma unroll
        for (int j = 0; j < 2 * R2C; ++j) fetch(P0[j], uni(min(j, T - 1)));
#pragma unroll
        for (int j = 0; j < 2 * R2C; ++j) put(P0[j], j);
    }
    TrialStage P[R2C];                     // chunk c + 2's rows, loaded during phase c - 1
#pragma unroll
    for (int j = 0; j < R2C; ++j) fetch(P[j], uni(min(2 * R2C + j, T - 1)));
    lds_barrier(bw);                       // the pass's leading barrier: chunks 0, 1 in the ring
    int s2 = 2;                            // (c + 2) % 3
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int j = 0; j < R2C; ++j) {
            put(P[j], s2 * R2C + j);
            fetch(P[j], uni(min((c + 3) * R2C + j, T - 1)));
        }
        s2 = s2 == 2 ? 0 : s2 + 1;
        lds_barrier(bw);
    }
    lds_barrier(bw);
}

// the pair trial's chain fed from the loader's LDS ring: stage t's row is read during stage
// t - 1 (chunk c + 1's first row during chunk c's last stage: written in phase c - 1)
template <bool U0Z>
__device__ __forceinline__ void run2_trial_pair_lds(ring_t ring, kring_t kr, int tl, int64_t l, bool odd, int cb,
                                                    unsigned long long& bw) {
    const rargs_t R = kernarg<RunArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const double2 xa = R->x[cb][wix(0, 0, 2, l, Bp)], xb = R->x[cb][wix(0, 1, 2, l, Bp)];
    double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
    auto get = [&](TrialStage& q, int slot) {
        q.k0 = kr[slot][0][tl];
        q.k1 = kr[slot][1][tl];
        q.cg = kr[slot][2][tl].x;
    };
    // every Horner coefficient of the minimax kernels and the model held in VGPRs across the stage loop: no scalar
    // loads in it (the LDS reads' lgkmcnt waits are not merged with kernarg loads) and no per-stage copies of second
    // scalar operands
    const gym::PolyRegs pk = gym::poly_vgprs_all();
    Dyn dm = R->m;
    gym::in_vgpr(dm.b); gym::in_vgpr(dm.d); gym::in_vgpr(dm.a2b); gym::in_vgpr(dm.bb); gym::in_vgpr(dm.dad);
    gym::in_vgpr(dm.g1); gym::in_vgpr(dm.g2); gym::in_vgpr(dm.f1); gym::in_vgpr(dm.f2); gym::in_vgpr(dm.h);
    gym::in_vgpr(dm.h2); gym::in_vgpr(dm.h6);
    auto step = [&](const TrialStage& q, int slot) {
        const double v1 = trial_u1(q.k0, q.k1, q.cg, n0, n1, n2, n3);
        // branch-free near-path step (a wave-uniform fallback to the full reduction inside); three-address Horner
        gym::rk4_pair_fast<true>(dm, odd, n0, n1, n2, n3, v1, pk);
        double2(*s)[BLK] = ring[slot];
        s[0][tl] = make_double2(n0, n1);    // both lanes of the pair: the same values, no per-lane select
        s[1][tl] = make_double2(n2, n3);
        s[2][tl] = make_double2(v1, 0.0);   // both lanes of the pair: the same value
    };
    const int nch = run2_chunks(T);
    lds_barrier(bw);                       // the loader's chunks 0, 1
    TrialStage cur;
    get(cur, 0);
    int s0 = 0, s1 = 1;                    // c % 3, (c + 1) % 3
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int j = 0; j < R2C; ++j) {
            TrialStage nxt;
            get(nxt, j + 1 < R2C ? s0 * R2C + j + 1 : s1 * R2C);
            step(cur, (c & 1) * R2C + j);   // past the end: harmless, not consumed
            cur = nxt;
        }
        s0 = s1;
        s1 = s1 == 2 ? 0 : s1 + 1;
        lds_barrier(bw);
    }
    lds_barrier(bw);
}

// helper wavefront, first Armijo trial: u0, the running cost and the candidate's stores; returns J
template <bool U0Z, bool RL>
__device__ __forceinline__ double run2_trial_helper(ring_t ring, int lane, int64_t l, int cb, bool act,
                                                  const double* __restrict__ xr, const double* __restrict__ ur,
                                                  unsigned long long& bw) {
    const rargs_t R = kernarg<RunArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t so2 = act ? o2 : 0x80000000u, so1 = act ? o1 : 0x80000000u;   // inactive: dropped (OOB)
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Ub = reinterpret_cast<const char*>(R->u[cb]);
    const char* Xb = reinterpret_cast<const char*>(R->x[cb ^ 1]);
    const char* Ob = reinterpret_cast<const char*>(R->u[cb ^ 1]);
    // x_ref / u_ref rows: wave-uniform scalar loads (restrict parameters: no store can alias them); per-lane
    // references (RL): the lane's own rows
    const double gamma = R->a.gamma0;
    const double2 xa = R->x[cb][wix(0, 0, 2, l, Bp)], xb = R->x[cb][wix(0, 1, 2, l, Bp)];
    double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
    if (act) {
        const auto rX = rsrc(Xb);
        bst2(rX, o2, 0, n0, n1);
        bst2(rX, o2, WROW, n2, n3);
    }
    double J = 0.0;
    const int nch = run2_chunks(T);
    lds_barrier(bw);                       // the loader's leading barrier
    lds_barrier(bw);                       // the main wavefront's chunk 0
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int j = 0; j < R2C; ++j) {
            const int t = c * R2C + j;
            if (t < T) {
                const double2(*s)[BLK] = ring[(c & 1) * R2C + j];
                const double2 na = s[0][lane], nb = s[1][lane], vv = s[2][lane];
                const Row<2> urt = ref_row<2, RL>(ur, t);
                const Row<4> xrt = ref_row<4, RL>(xr, t);
                const KArgs ka = kernarg_consts();
                const double u0 = U0Z ? 0.0 : bld1(rsrc(Ub + (int64_t)t * row), o1, 0);
                const double v0 = U0Z ? 0.0 : trial_u0(u0, urt.v[0], gamma, ka.w.G00, ka.w.iG00);
                const double v1 = vv.x;
                const double f0 = U0Z ? 0.0 : v0 - urt.v[0], f1 = v1 - urt.v[1];
                J = stage_cost<U0Z>(J, ka.w.Q, ka.w.R, n0, n1, n2, n3, xrt.v, f0, f1);
                {   // an inactive lane's stores fall outside the resources' range (dropped): no exec-mask branch
                    const auto rO = rsrc(Ob + (int64_t)t * row);
                    if (!U0Z) bst1(rO, so1, 0, v0);
                    bst1(rO, so1, plane, v1);
                    const auto rX = rsrc(Xb + (int64_t)(t + 1) * (2 * (int64_t)row));
                    bst2(rX, so2, 0, na.x, na.y);
                    bst2(rX, so2, WROW, nb.x, nb.y);
                }
                n0 = na.x; n1 = na.y; n2 = nb.x; n3 = nb.y;
            }
        }
        lds_barrier(bw);
    }
    const Row<4> xrT = ref_row<4, RL>(xr, T);
    return J + xcost(R->w.QT, n0, n1, n2, n3, xrT.v);
}

// Four wavefronts per 64 lanes.  Sweep: 0 the matrix half of the Riccati update, 1 and 2 the stage linearisations
// (dealt round-robin), 3 the vector half and the stores.  Trial: 0 and 3 the RK4 chains on lane pairs, 1 the cost
// and the candidate's stores, 2 the chains' loader.
constexpr int R2H = 2;            // sweep helper wavefronts
constexpr int R2WAVES = 4;

template <bool U0Z, bool RL>
__global__ __launch_bounds__(R2WAVES * BLK, 1) void k_nt_run2(RunArgs args) {
    __shared__ double2 ring[R2S][R2W][BLK];
    __shared__ double2 gring[2 * R2C][3][BLK];   // the split sweep's gain rows, G11, 1/G11
    __shared__ double2 kring[3 * R2C][3][BLK];   // the trial's K row 1 / cg (loader wavefront)
    __shared__ double shJ[BLK];
    __shared__ int shst[BLK];
    const int lane = threadIdx.x & (BLK - 1);
    const int wave = threadIdx.x / BLK;          // 0: main; 1 .. R2H: helpers
    const bool helper = wave > 0;
    const int64_t l = (int64_t)blockIdx.x * BLK + lane;   // < Bp: padding lanes hold GYM_PAD
    int st = kernarg<RunArgs>()->status[l];
    // GYM_RUN2_TRACE only: sweep / trial / post cycles, iterations, barrier waits in the sweep / the trial
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    for (int k = kernarg<RunArgs>()->k0; k < kernarg<RunArgs>()->k1; ++k) {
        if (!__syncthreads_or(st == GYM_ACTIVE)) break;    // workgroup-uniform
        const bool act = st == GYM_ACTIVE;
        const int cb = k & 1;
        unsigned long long tt = R2T_NOW();
        ++acc[3];
        if (wave == 1) {
            run2_sweep_helper<U0Z, 0, R2H, RL>(ring, lane, l, cb, run_xr<RL>(kernarg<RunArgs>(), l), run_ur<RL>(kernarg<RunArgs>(), l),
                                               acc[4]);
        } else if (wave == 2) {
            run2_sweep_helper<U0Z, 1, R2H, RL>(ring, lane, l, cb, run_xr<RL>(kernarg<RunArgs>(), l),
                                               run_ur<RL>(kernarg<RunArgs>(), l), acc[4]);
        } else if (wave == 0) {
            run2_sweep_gain<U0Z, RL>(ring, gring, lane, l, cb, acc[4]);
        } else {   // the pair wavefront: the vector half, the stores
            double d, s;
            run2_sweep_vec<U0Z, RL>(ring, gring, lane, l, cb, act, d, s, acc[4]);
            const rargs_t Q = kernarg<RunArgs>();
            if (act) {
                Q->dJ[l] = d;
                Q->smax[l] = s;
                if (Q->hist_smax && k < Q->a.hist_len) Q->hist_smax[(int64_t)k * Q->Bp + l] = s;
            }
            lane_fence();                                  // K1 / cg visible to this wavefront's trial loads
        }
        __syncthreads();                                   // K1 / cg stored by the pair wavefront, read by the loader
        acc[0] += R2T_NOW() - tt;
        tt = R2T_NOW();
        if (wave == 1) {
            shJ[lane] = run2_trial_helper<U0Z, RL>(ring, lane, l, cb, act, run_xr<RL>(kernarg<RunArgs>(), l),
                                                   run_ur<RL>(kernarg<RunArgs>(), l), acc[5]);
        } else if (wave == 2) {
            run2_trial_kload<U0Z>(kring, lane, l, acc[5]);
        } else {                                           // waves 0 and 3: lane pairs, rows from LDS
            const int tl = (wave == 0 ? 0 : BLK / 2) + (lane >> 1);
            run2_trial_pair_lds<U0Z>(ring, kring, tl, (int64_t)blockIdx.x * BLK + tl, lane & 1, cb, acc[5]);
        }
        __syncthreads();                                   // shJ written; the helper's stores are complete
        acc[1] += R2T_NOW() - tt;
        tt = R2T_NOW();
        if (!helper && act) {
            const rargs_t R = kernarg<RunArgs>();
            double Jn = shJ[lane];
            double g = R->a.gamma0;
            int nr = 1;
            bool ok = Jn < R->cost[l] + R->a.c * g * R->dJ[l];   // strict Armijo test (:361)
            const bool deferred = !ok && R->a.max_ls > 1 && R->ext;
            if (deferred) {
                // external retries (one iteration per launch): the lane joins the retry list, as after the serial
                // schedule's trial (k_nt_trial); the candidates / accepted re-run kernels finish its iteration
                R->n_roll[l] += 1;
                R->retry_list[atomicAdd(R->counter, 1)] = (int32_t)l;
            } else if (!ok && R->a.max_ls > 1) {
                lane_fence();                              // the helper's candidate stores, before they are rewritten
                {
                    const rargs_t P = kernarg<RunArgs>();
                    double d2, s2;
                    backward_solver_lane<U0Z, OUT_SIGMA, false>(P->m, P->w, P->x[cb], P->u[cb], run_xr<RL>(P, l),
                                                                run_ur<RL>(P, l), P->K1,
                                                                P->cs, 0.0, l, P->Bp, P->N, d2, s2);
                }
                lane_fence();
                for (int j = 1; !ok && j < kernarg<RunArgs>()->a.max_ls; ++j) {
                    const rargs_t P = kernarg<RunArgs>();
                    g *= P->a.beta;                        // gamma_i *= beta, sequentially (:365)
                    const double2 xa = P->x[cb][wix(0, 0, 2, l, P->Bp)], xb = P->x[cb][wix(0, 1, 2, l, P->Bp)];
                    Jn = rollout_cform<true, U0Z, true, false, kNT, false>(P->m, P->w, P->u[cb], P->K1, P->cs,
                                                                          run_xr<RL>(P, l), run_ur<RL>(P, l),
                                                                          P->x[cb ^ 1], P->u[cb ^ 1], g,
                                                                          P->a.gamma0, l, P->Bp, P->N, xa.x, xa.y,
                                                                          xb.x, xb.y);
                    ++nr;
                    const rargs_t Q = kernarg<RunArgs>();
                    ok = Jn < Q->cost[l] + Q->a.c * g * Q->dJ[l];
                }
            }
            if (!deferred) {
                const rargs_t F = kernarg<RunArgs>();
                F->n_roll[l] += nr;
                F->n_iter[l] += 1;
                SolverCtl c = F->a;
                c.k = k;
                if (ok) {
                    const double sm = F->smax[l];
                    accept_lane(c, l, Jn, g, sm, F->cost, F->gamma, F->status, F->res_buf, F->hist_cost, F->Bp);
                    if (sm < c.tol) st = GYM_CONVERGED;
                } else {
                    fail_lane(c, l, F->status, F->res_buf);
                    st = GYM_LS_FAILED;
                }
            }
        }
        if (!helper) shst[lane] = st;
        lane_fence();                                      // every store of this iteration visible to both wavefronts
        __syncthreads();
        if (helper) st = shst[lane];
        acc[2] += R2T_NOW() - tt;
    }
#ifdef GYM_RUN2_TRACE
    if (lane == 0 && blockIdx.x < 8192 && wave <= 1)
        for (int i = 0; i < 6; ++i) g_run2_trace[blockIdx.x][wave][i] = acc[i];
#endif
}
