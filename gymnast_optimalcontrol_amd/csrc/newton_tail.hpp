// Newton solver kernels: the straggler tail (k_nt_tail).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// Straggler tail (gym_newton_tail).  Late in a hard solve a handful of lanes keep iterating for thousands of
// outer iterations, many of them backtracking (SURVEY 8(d)'s stress variant: one lane to 5,000 iterations, the
// last ~4,000 serving a few lanes).  The lock-step schedules then pay, per iteration and lane, one sweep chain
// and one trial chain on one thread each, plus for a backtracking lane the sigma1 re-run, the candidate pass and
// the accepted candidate's re-run.  Here one workgroup (one wavefront) owns one listed lane and runs its own
// iterations k0 .. k1-1 back to back (lanes are independent problems; the persistent schedule's argument):
//   sweep  : the 64 threads evaluate the Jacobians / linearisations of 64 stages at once (stage_lin, a function
//            of x_t, u_t only) into LDS, then run the Riccati recursion (step_lin) over those stages, reading
//            them back; K row 1, cg and sigma1 are stored in the same pass (no sigma1 re-run);
//   trials : thread c evaluates Armijo trial c (gamma_0 beta^c, formed sequentially as the reference does) --
//            all max_ls of them at once, each writing its candidate into a scratch slot -- and the first
//            accepted one (ballot) is copied into the lane's next state buffer.
// Every value is the one the serial schedule computes (the same device functions: jacobian, stage_lin, step_lin,
// store_stage, trial_u0 / trial_u1, stage_cost, rk4): trial 1 is the offset form cg + K1 x_new, trial c > 0
// fma(gamma_c - gamma_0, sigma1, cg + K1 x_new), so decisions, rollout counts and trajectories are the same bits.
// ------------------------------------------------------------------------------------------
constexpr int TL_STAGES = BLK;   // stages per linearisation pass (one per thread)
constexpr int TL_PITCH = 22;     // doubles per stage in LDS: Lin (16), x_t (4), u1_t; padded to an even count
struct TailArgs : LaneArgs {   // re-read from the kernel-argument segment at each use (kernarg<TailArgs>())
    const int32_t* list;   // the lanes, one workgroup each
    double2* sx;           // candidate scratch: x (N, Vp/64, 2, 64) double2 over virtual lanes (slot * max_ls + c)
    double* su;            // ... and u planes (T, 2, Vp)
    int64_t Bp, Vp;
    int32_t N, k0, k1, pad;
};
static_assert(sizeof(TailArgs) == sizeof(LaneArgs) + 56, "kernarg layout: LaneArgs, then TailArgs' own fields");
typedef const TailArgs* targs_t;

// The trials' per-stage inputs are staged in LDS by the sweep (K row 1, cg, sigma1 and u0: 8 doubles per stage), so
// the trial loop issues no global loads: its scratch stores are never waited on (the GFX9 vmcnt counts both)
constexpr int TL_TST = 8;
constexpr int TL_MAX_T = 640;    // T * 64 B of trial staging (40 KiB) + the linearisation / gain / exchange areas: tail_lds_bytes(T),
                                 // ~72 KiB at T = 500, ~87 KiB at T = 640: above the 64 KiB default, so every launch raises
                                 // the kernel's dynamic-LDS limit (gfx950: 160 KiB); gym_newton_tail_lds reports both
// Two wavefronts per tail lane: the sweep's Riccati update split as in k_nt_run2 (Sweep::step_P on wavefront 0,
// Sweep::step_p, the stores and the next pass's linearisations on wavefront 1, one 64-stage pass behind;
// linearisations triple-buffered, the gain rows double-buffered)
constexpr int TL_THREADS = 2 * BLK;
constexpr int TL_GK = 6;         // doubles per stage in the gain ring: k row 1 (4), G11, 1/G11
// Trials on lane pairs: wavefront 0 runs the candidates' RK4 chains and hands each stage's (x_{t+1}, u1_t) to
// wavefront 1 through a ring of 2 chunks x TL_RC stages x 32 trials x 3 pairs; wavefront 1 (lane c: trial c)
// accumulates the cost and stores the candidate.  (Single-thread trials, GYM_FLAG_RUN_SINGLE or more than 32
// trials: wavefront 0 alone, tail_candidate.)
constexpr int TL_RC = 2;
constexpr int TL_RING = 2 * TL_RC * (BLK / 2) * 3 * 2;   // doubles
constexpr size_t tail_lds_bytes(int T) {
    return sizeof(double) * ((size_t)3 * TL_STAGES * TL_PITCH + (size_t)2 * TL_STAGES * TL_GK + 4 +
                             (size_t)TL_RING + (size_t)T * TL_TST);
}
// The sweep of lane l at iterate cb on two wavefronts: K row 1, cg and sigma1 of every stage (global, and staged in
// tst).  Pass j covers stages T-1-64j down to T-64-64j.  Between
// workgroup barriers j and j+1, wavefront 0 runs the matrix half over pass j (linearisations lin3[j % 3], gain rows
// into gk2[j & 1]) while wavefront 1 runs the vector half over pass j - 1 (its linearisations and gain rows, K row
// 1 / cg / sigma1 stored and staged in tst) and then evaluates pass j + 1's linearisations.  Every thread of a
// wavefront runs the same recursion (the same bits); its lane 0 writes.  dJ and max|sigma| land in shd[0..1].
template <bool U0Z, bool RL>
__device__ __forceinline__ void tail_sweep_split(double* lin3, double* gk2, double* shd, double* tst, int wave,
                                                 int lane, int64_t l, int cb) {
    const targs_t R = kernarg<TailArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const double2* x = R->x[cb];
    const double* u = R->u[cb];
    const double* xr = lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N);
    const double* ur = lane_ref<RL>(R->ur, l, 2 * (int64_t)T);
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t so2 = lane == 0 ? o2 : 0x80000000u, so1 = lane == 0 ? o1 : 0x80000000u;   // OOB: dropped
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Kb = reinterpret_cast<const char*>(R->K1);
    const char* Cb = reinterpret_cast<const char*>(R->cs);
    const double g0 = R->a.gamma0;
    const double dt = R->m.h;
    Sweep<false> S(R->w, x[wix(T, 0, 2, l, Bp)], x[wix(T, 1, 2, l, Bp)], xr + 4 * T);
    const int np = (T + TL_STAGES - 1) / TL_STAGES;
    auto linearise = [&](int j) {   // wavefront 1: pass j's linearisations, thread i stage T-1-64j-i
        const int t = T - 1 - j * TL_STAGES - lane;
        if (t >= 0) {
            const double2 xa = x[wix(t, 0, 2, l, Bp)], xb = x[wix(t, 1, 2, l, Bp)];
            const double u0 = U0Z ? 0.0 : u[pix(t, 0, 2, l, Bp)], u1 = u[pix(t, 1, 2, l, Bp)];
            const KArgs ka = kernarg_consts();
            const gym::Jac J = gym::jacobian(ka.m, xa.x, xa.y, xb.x, xb.y, u1);
            const Lin L = stage_lin<U0Z>(ka.m, ka.w, J, xa, xb, u0, u1, xr + 4 * t, ur + 2 * t);
            double* s = lin3 + ((j % 3) * TL_STAGES + lane) * TL_PITCH;
            s[0] = L.A20; s[1] = L.A21; s[2] = L.A22; s[3] = L.A23;
            s[4] = L.A30; s[5] = L.A31; s[6] = L.A32; s[7] = L.A33;
            s[8] = L.bd2; s[9] = L.bd3; s[10] = L.q0; s[11] = L.q1;
            s[12] = L.q2; s[13] = L.q3; s[14] = L.r0; s[15] = L.r1;
            s[16] = xa.x; s[17] = xa.y; s[18] = xb.x; s[19] = xb.y; s[20] = u1;
            tst[t * TL_TST + 6] = u0;
        }
    };
    KW wv = R->w;                          // the Riccati halves' weights in VGPRs: no per-stage kernel-argument loads
    gym::in_vgpr(wv.twoQ[0]); gym::in_vgpr(wv.twoQ[1]); gym::in_vgpr(wv.twoQ[2]); gym::in_vgpr(wv.twoQ[3]);
    gym::in_vgpr(wv.twoR1); gym::in_vgpr(wv.iG00);
    if (wave == 1) linearise(0);
    __syncthreads();
    for (int j = 0; j <= np; ++j) {
        if (wave == 0) {
            if (j < np) {
                const int tb = T - 1 - j * TL_STAGES;
                const int n = tb + 1 < TL_STAGES ? tb + 1 : TL_STAGES;
                const double* L3 = lin3 + (j % 3) * TL_STAGES * TL_PITCH;
                double* G = gk2 + (j & 1) * TL_STAGES * TL_GK;
                for (int i = 0; i < n; ++i) {
                    const double* s = L3 + i * TL_PITCH;
                    const KW& kw = wv;
                    const Lin L{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9],
                                0.0, 0.0, 0.0, 0.0, 0.0, 0.0, dt};   // q, r: the vector half's
                    double k0, k1, k2, k3, G11, iG;
                    S.step_P(kw, L, k0, k1, k2, k3, G11, iG);
                    double* g = G + i * TL_GK;     // every thread: the same values at the same addresses
                    g[0] = k0; g[1] = k1; g[2] = k2; g[3] = k3; g[4] = G11; g[5] = iG;
                }
            }
        } else {
            if (j >= 1) {
                const int jj = j - 1;
                const int tb = T - 1 - jj * TL_STAGES;
                const int n = tb + 1 < TL_STAGES ? tb + 1 : TL_STAGES;
                const double* L3 = lin3 + (jj % 3) * TL_STAGES * TL_PITCH;
                const double* G = gk2 + (jj & 1) * TL_STAGES * TL_GK;
                for (int i = 0; i < n; ++i) {
                    const double* s = L3 + i * TL_PITCH;
                    const double* g = G + i * TL_GK;
                    const double k0 = g[0], k1 = g[1], k2 = g[2], k3 = g[3];
                    const KW& kw = wv;
                    const Lin L{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9],
                                s[10], s[11], s[12], s[13], s[14], s[15], dt};
                    double s0, s1;
                    S.step_p<U0Z>(kw, L, k0, k1, k2, k3, g[4], g[5], s0, s1);
                    {   // every thread: the same values; lane 0's global stores land, the others' fall outside the
                        // resources' range (dropped by the hardware) -- no exec-mask branch on the pass
                        const int ts = tb - i;
                        const double2 xa = make_double2(s[16], s[17]), xb = make_double2(s[18], s[19]);
                        const double cg = stage_cg(xa, xb, s[20], g0, k0, k1, k2, k3, s1);
                        double* q = tst + ts * TL_TST;
                        q[0] = k0; q[1] = k1; q[2] = k2; q[3] = k3; q[4] = cg; q[5] = s1;
                        const auto rC = rsrc(Cb + (int64_t)ts * row);
                        const auto rK = rsrc(Kb + (int64_t)ts * (2 * (int64_t)row));
                        bst2(rK, so2, 0, k0, k1);
                        bst2(rK, so2, WROW, k2, k3);
                        bst1(rC, so1, 0, cg);
                        bst1(rC, so1, plane, s1);
                    }
                }
            }
            if (j + 1 < np) linearise(j + 1);
            if (j == np && lane == 0) { shd[0] = S.dJ; shd[1] = S.smax; }
        }
        __syncthreads();
    }
}

// Armijo trial c of lane l (step size g; c = 0: the first trial's offset form) on one thread into virtual lane v of
// the scratch, its streams from the staging tst; returns the candidate's cost
template <bool U0Z, bool RL>
__device__ __forceinline__ double tail_candidate(const double* tst, int64_t l, int cb, int c, double g, int64_t v) {
    const targs_t R = kernarg<TailArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const double* xr = lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N);
    const double* ur = lane_ref<RL>(R->ur, l, 2 * (int64_t)T);
    const uint32_t v2 = wbo(v, 2), v1o = (uint32_t)v * 8u;
    const uint32_t srow = (uint32_t)R->Vp * 16u, splane = (uint32_t)R->Vp * 8u;
    const char* Xs = reinterpret_cast<const char*>(R->sx);
    const char* Us = reinterpret_cast<const char*>(R->su);
    const double gamma0 = R->a.gamma0, dg = g - gamma0;
    const double2 xa = R->x[cb][wix(0, 0, 2, l, Bp)], xb = R->x[cb][wix(0, 1, 2, l, Bp)];
    double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
    {
        const auto rX = rsrc(Xs);
        bst2(rX, v2, 0, n0, n1);
        bst2(rX, v2, WROW, n2, n3);
    }
    double J = 0.0;
    const gym::PolyRegs pk = gym::poly_vgprs();
    const KArgs ka = kernarg_consts();
    const Dyn m = ka.m;
    const double G00 = ka.w.G00, iG00 = ka.w.iG00;
    for (int t = 0; t < T; ++t) {
        const double* q = tst + t * TL_TST;
        const double2 k0 = make_double2(q[0], q[1]), k1 = make_double2(q[2], q[3]);
        const double cg = q[4], s1 = q[5];
        const Row<2> urt = ref_row<2, RL>(ur, t);
        const Row<4> xrt = ref_row<4, RL>(xr, t);
        const double v0 = U0Z ? 0.0 : trial_u0(q[6], urt.v[0], g, G00, iG00);
        const double y = trial_u1(k0, k1, cg, n0, n1, n2, n3);   // cg + K1 x_new: trial 1's value
        const double ysig = __builtin_fma(dg, s1, y);            // trial_u1_sig's value
        const double u1 = c == 0 ? y : ysig;
        const double f0 = U0Z ? 0.0 : v0 - urt.v[0], f1 = u1 - urt.v[1];
        const KArgs kc = kernarg_consts();
        J = stage_cost<U0Z>(J, kc.w.Q, kc.w.R, n0, n1, n2, n3, xrt.v, f0, f1);
        {
            const auto rO = rsrc(Us + (int64_t)t * srow);
            if (!U0Z) bst1(rO, v1o, 0, v0);
            bst1(rO, v1o, splane, u1);
        }
        gym::rk4(m, n0, n1, n2, n3, u1, pk);
        const auto rX = rsrc(Xs + (int64_t)(t + 1) * (2 * (int64_t)srow));
        bst2(rX, v2, 0, n0, n1);
        bst2(rX, v2, WROW, n2, n3);
    }
    const Row<4> xrT = ref_row<4, RL>(xr, T);
    return J + xcost(ka.w.QT, n0, n1, n2, n3, xrT.v);
}

// Wavefront 0: the RK4 chain of Armijo trial c on the lane pair (2c, 2c + 1) -- the offset-form feedback
// and gym::rk4_pair, exactly tail_candidate's chain -- handing each stage's state and control to wavefront 1 (ring
// [chunk & 1][stage in chunk][trial][(th1, th2) | (w1, w2) | (u1, -)]).  Chunk cc between barriers cc and cc + 1.
typedef double2 (*tring_t)[TL_RC][BLK / 2][3];
template <bool U0Z, bool RL>
__device__ __forceinline__ void tail_trial_chain(const double* tst, tring_t ring, int64_t l, int cb, int c, double g,
                                                 bool odd) {
    const targs_t R = kernarg<TailArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const double dg = g - R->a.gamma0;
    const double2 xa = R->x[cb][wix(0, 0, 2, l, Bp)], xb = R->x[cb][wix(0, 1, 2, l, Bp)];
    double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
    // every Horner coefficient and the model in VGPRs across the chain's loop (as k_nt_run2's trial chain)
    const gym::PolyRegs pk = gym::poly_vgprs_all();
    Dyn m = kernarg_consts().m;
    gym::in_vgpr(m.b); gym::in_vgpr(m.d); gym::in_vgpr(m.a2b); gym::in_vgpr(m.bb); gym::in_vgpr(m.dad);
    gym::in_vgpr(m.g1); gym::in_vgpr(m.g2); gym::in_vgpr(m.f1); gym::in_vgpr(m.f2); gym::in_vgpr(m.h);
    gym::in_vgpr(m.h2); gym::in_vgpr(m.h6);
    const int nch = (T + TL_RC - 1) / TL_RC;
    const int tc = c < BLK / 2 ? c : 0;
    for (int cc = 0; cc < nch; ++cc) {
#pragma unroll
        for (int j = 0; j < TL_RC; ++j) {
            const int t = cc * TL_RC + j;
            if (t < T) {
                const double* q = tst + t * TL_TST;
                const double2 k0 = make_double2(q[0], q[1]), k1 = make_double2(q[2], q[3]);
                const double y = trial_u1(k0, k1, q[4], n0, n1, n2, n3);   // cg + K1 x_new: trial 1's value
                const double ysig = __builtin_fma(dg, q[5], y);             // trial_u1_sig's value
                const double u1 = c == 0 ? y : ysig;
                gym::rk4_pair_fast<true>(m, odd, n0, n1, n2, n3, u1, pk);   // branch-free near path, as k_nt_run2
                double2* r = ring[cc & 1][j][tc];   // both lanes of the pair: the same values, no per-lane select
                r[0] = make_double2(n0, n1);
                r[1] = make_double2(n2, n3);
                r[2] = make_double2(u1, 0.0);
            }
        }
        __syncthreads();
    }
    __syncthreads();                       // the helper's last chunk
}

// Wavefront 1, lane c (< max_ls): trial c's cost (stage costs in stage order, as tail_candidate) and its
// candidate trajectory into virtual lane v of the scratch; returns J.  Chunk cc between barriers cc + 1 and cc + 2.
template <bool U0Z, bool RL>
__device__ __forceinline__ double tail_trial_helper(const double* tst, tring_t ring, int64_t l, int cb, int c, double g,
                                                    int64_t v, bool act) {
    const targs_t R = kernarg<TailArgs>();
    const int T = R->N - 1;
    const int64_t Bp = R->Bp;
    const double* xr = lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N);
    const double* ur = lane_ref<RL>(R->ur, l, 2 * (int64_t)T);
    const uint32_t v2 = wbo(v, 2), v1o = (uint32_t)v * 8u;
    const uint32_t srow = (uint32_t)R->Vp * 16u, splane = (uint32_t)R->Vp * 8u;
    const char* Xs = reinterpret_cast<const char*>(R->sx);
    const char* Us = reinterpret_cast<const char*>(R->su);
    const double2 xa = R->x[cb][wix(0, 0, 2, l, Bp)], xb = R->x[cb][wix(0, 1, 2, l, Bp)];
    double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
    if (act) {
        const auto rX = rsrc(Xs);
        bst2(rX, v2, 0, n0, n1);
        bst2(rX, v2, WROW, n2, n3);
    }
    double J = 0.0;
    const KArgs ka = kernarg_consts();
    const double G00 = ka.w.G00, iG00 = ka.w.iG00;
    const int nch = (T + TL_RC - 1) / TL_RC;
    const int tc = c < BLK / 2 ? c : 0;
    __syncthreads();                       // the chain's chunk 0
    for (int cc = 0; cc < nch; ++cc) {
#pragma unroll
        for (int j = 0; j < TL_RC; ++j) {
            const int t = cc * TL_RC + j;
            if (t < T) {
                const double2* r = ring[cc & 1][j][tc];
                const double2 na = r[0], nb = r[1], uu = r[2];
                const Row<2> urt = ref_row<2, RL>(ur, t);
                const Row<4> xrt = ref_row<4, RL>(xr, t);
                const double v0 = U0Z ? 0.0 : trial_u0(tst[t * TL_TST + 6], urt.v[0], g, G00, iG00);
                const double u1 = uu.x;
                const double f0 = U0Z ? 0.0 : v0 - urt.v[0], f1 = u1 - urt.v[1];
                const KArgs kc = kernarg_consts();
                J = stage_cost<U0Z>(J, kc.w.Q, kc.w.R, n0, n1, n2, n3, xrt.v, f0, f1);
                if (act) {
                    const auto rO = rsrc(Us + (int64_t)t * srow);
                    if (!U0Z) bst1(rO, v1o, 0, v0);
                    bst1(rO, v1o, splane, u1);
                    const auto rX = rsrc(Xs + (int64_t)(t + 1) * (2 * (int64_t)srow));
                    bst2(rX, v2, 0, na.x, na.y);
                    bst2(rX, v2, WROW, nb.x, nb.y);
                }
                n0 = na.x; n1 = na.y; n2 = nb.x; n3 = nb.y;
            }
        }
        __syncthreads();
    }
    const Row<4> xrT = ref_row<4, RL>(xr, T);
    return J + xcost(ka.w.QT, n0, n1, n2, n3, xrT.v);
}

#ifdef GYM_TAIL_TRACE
// Diagnostic build only (tools/tail_trace.py): per workgroup, cycles (s_memtime) in the sweep, the trials, the rest
// of the iteration, and the iterations run
__device__ unsigned long long g_tail_trace[4096][4];
#endif
template <bool U0Z, bool RL, bool PAIR>
__global__ __launch_bounds__(TL_THREADS, 1) void k_nt_tail(TailArgs args) {
    extern __shared__ double tail_lds[];          // tail_lds_bytes(T)
    // lin3 (3 passes) | gk2 (2 passes of gain rows) | shd (dJ, max|sigma|, the decision) | ring | tst
    double* lin = tail_lds;
    double* gk2 = lin + 3 * TL_STAGES * TL_PITCH;
    double* shd = gk2 + 2 * TL_STAGES * TL_GK;
    const tring_t ring = reinterpret_cast<tring_t>(shd + 4);   // PAIR: the trials' hand-off
    double* tst = shd + 4 + TL_RING;
    const int lane = threadIdx.x & (BLK - 1);
    const int wave = threadIdx.x / BLK;           // 0 the matrix half and the trials, 1 the vector half
    const int64_t l = kernarg<TailArgs>()->list[blockIdx.x];
    int st = kernarg<TailArgs>()->status[l];
    unsigned long long acc[4] = {0, 0, 0, 0};   // GYM_TAIL_TRACE only
    for (int k = kernarg<TailArgs>()->k0; st == GYM_ACTIVE && k < kernarg<TailArgs>()->k1; ++k) {
        const int cb = k & 1;
        double dJ, sm;
        unsigned long long tt = R2T_NOW();
        ++acc[3];
        tail_sweep_split<U0Z, RL>(lin, gk2, shd, tst, wave, lane, l, cb);   // ends at a workgroup barrier
        dJ = shd[0];
        sm = shd[1];
        acc[0] += R2T_NOW() - tt;
        tt = R2T_NOW();
        {
            const targs_t Q = kernarg<TailArgs>();
            if (lane == 0 && wave == 0) {
                Q->dJ[l] = dJ;
                Q->smax[l] = sm;
                if (Q->hist_smax && k < Q->a.hist_len) Q->hist_smax[(int64_t)k * Q->Bp + l] = sm;
            }
        }
        __syncthreads();   // the staged trial inputs (LDS) complete
        const int max_ls = kernarg<TailArgs>()->a.max_ls;
        // PAIR: wavefront 0 runs the trials' chains (trial c on lanes 2c, 2c + 1), wavefront 1 (lane c: trial c) their
        // costs, stores and Armijo tests; otherwise wavefront 0 does all of it, one trial per thread
        const int dec = PAIR ? 1 : 0;               // the wavefront holding the decisions
        const bool helper_wave = PAIR && wave == 1;  // lane c: trial c's cost
        const int cand = (PAIR && !helper_wave) ? lane >> 1 : lane;   // this thread's trial
        const int64_t v = (int64_t)blockIdx.x * max_ls + cand;
        double g = kernarg<TailArgs>()->a.gamma0;
        for (int q = 0; q < cand && q < max_ls; ++q) g *= kernarg<TailArgs>()->a.beta;   // gamma_i *= beta (:365)
        bool ok = false;
        double Jn = 0.0;
        if (PAIR) {
            if (wave == 0) {
                tail_trial_chain<U0Z, RL>(tst, ring, l, cb, cand, g, lane & 1);
            } else {
                Jn = tail_trial_helper<U0Z, RL>(tst, ring, l, cb, cand, g, v, cand < max_ls);
                const targs_t R = kernarg<TailArgs>();
                ok = cand < max_ls && Jn < R->cost[l] + R->a.c * g * dJ;   // strict Armijo test (:361)
            }
        } else if (cand < max_ls && wave == 0) {
            Jn = tail_candidate<U0Z, RL>(tst, l, cb, cand, g, v);
            const targs_t R = kernarg<TailArgs>();
            ok = Jn < R->cost[l] + R->a.c * g * dJ;   // strict Armijo test (:361)
        }
        const unsigned long long okm = __ballot(ok);
        acc[1] += R2T_NOW() - tt;
        tt = R2T_NOW();
        // the first accepted trial, in order, handed from the deciding wavefront to the other so that both leave the
        // iteration loop together
        int first = okm ? __ffsll((long long)okm) - 1 : -1;
        lane_fence();   // the candidates' scratch stores, before the copy reads them
        if (wave == dec && lane == 0) shd[2] = (double)first;
        __syncthreads();
        first = (int)shd[2];
        const int nr = first >= 0 ? first + 1 : max_ls;
        if (first >= 0 && wave == 0) {   // the accepted candidate becomes the lane's next iterate (buffer cb ^ 1)
            const targs_t R = kernarg<TailArgs>();
            const int T = R->N - 1;
            const int64_t vf = (int64_t)blockIdx.x * max_ls + first;
            for (int t0 = 0; t0 <= T; t0 += 4 * BLK) {   // four knots per thread in flight
                double2 a[4], b[4];
                double c0[4], c1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = t0 + j * BLK + lane;
                    if (t <= T) {
                        a[j] = R->sx[wix(t, 0, 2, vf, R->Vp)];
                        b[j] = R->sx[wix(t, 1, 2, vf, R->Vp)];
                    }
                    if (t < T) {
                        c0[j] = U0Z ? 0.0 : R->su[pix(t, 0, 2, vf, R->Vp)];
                        c1[j] = R->su[pix(t, 1, 2, vf, R->Vp)];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = t0 + j * BLK + lane;
                    if (t <= T) {
                        R->x[cb ^ 1][wix(t, 0, 2, l, R->Bp)] = a[j];
                        R->x[cb ^ 1][wix(t, 1, 2, l, R->Bp)] = b[j];
                    }
                    if (t < T) {
                        if (!U0Z) R->u[cb ^ 1][pix(t, 0, 2, l, R->Bp)] = c0[j];
                        R->u[cb ^ 1][pix(t, 1, 2, l, R->Bp)] = c1[j];
                    }
                }
            }
        }
        const int src = first >= 0 ? first : 0;
        const double Jf = __shfl(Jn, src);
        const double gf = __shfl(g, src);
        if (lane == 0 && wave == dec) {
            const targs_t F = kernarg<TailArgs>();
            F->n_roll[l] += nr;
            F->n_iter[l] += 1;
            SolverCtl c = F->a;
            c.k = k;
            if (first >= 0)
                accept_lane(c, l, Jf, gf, sm, F->cost, F->gamma, F->status, F->res_buf, F->hist_cost, F->Bp);
            else
                fail_lane(c, l, F->status, F->res_buf);
        }
        st = first < 0 ? GYM_LS_FAILED : (sm < kernarg<TailArgs>()->a.tol ? GYM_CONVERGED : GYM_ACTIVE);
        lane_fence();   // the next iterate and the lane's state visible to the next iteration
        __syncthreads();
        acc[2] += R2T_NOW() - tt;
    }
#ifdef GYM_TAIL_TRACE
    if (threadIdx.x == 0 && blockIdx.x < 4096)
        for (int i = 0; i < 4; ++i) g_tail_trace[blockIdx.x][i] += acc[i];
#endif
}
