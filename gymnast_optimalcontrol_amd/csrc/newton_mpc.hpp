// Newton solver kernels: closed-loop replanning (shrinking-horizon nonlinear MPC) on the limited solve's loop body,
// k_nt_mpc_run (gym_newton_mpc_run, include/gymnast/newton_mpc.h).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// One closed loop per lane.  Lane l holds a consistent plan over the knots 0 .. N-1 and its cost J
// (gym_newton_init / _init_warm); control step t, t0 <= t < t1 <= T = N - 1, works on the horizon of stages t .. T-1:
// every stream at row t with N - t knots (x, u, K1, cs: a base-pointer offset of t stage strides; the lane's reference
// rows xr + 4t, ur + 2t, with per-lane references behind the full horizon's lane stride 4N / 2(N-1)).
//   1. replan: up to `iters` iterations of k_nt_run_limited's body on horizon t: sweep (V::sweep<U0Z, OUT_ALL>, the
//      lane's tau), Armijo trials rollout_cform<.., BOX> at gamma0, gamma0 beta, ... (at most max_ls, the strict test).
//      The stop test comes after the sweep and BEFORE the trials: max|sigma| < tol keeps the plan, runs no trial and
//      ends the step as GYM_CONVERGED (after the update, as in a single solve, every later step of a converged lane
//      would spend max_ls trials on rounding-level ties).  An Armijo failure keeps the plan and ends the step as
//      GYM_LS_FAILED.  Either stop ends this step only.  An iteration is counted when its trials ran.
//   2. act: u_t = stage t of the plan, x_t = its knot t (both recorded), x_{t+1} = rk4_fast(plant row l, x_t, u_t),
//      the trials' step on the thread's own Dyn (the row read once, h / h2 / h6 from the kernel arguments, as
//      ModelsVariant); the cost-to-go becomes J - l_t, l_t = stage_cost(0, ...) of stage t.
//   3. re-anchor, only if t + 1 < T and x_{t+1} differs in any bit from the plan's knot t + 1: sweep horizon t + 1 of
//      the plan, roll its policy out at step size 0 from x_{t+1} (the SIG trial with gamma = 0, clipped as every trial)
//      into the other buffer and accept it unconditionally: its cost is the new J.  One rollout, no iteration.  A lane
//      whose plant row is the design model never re-anchors.
// Buffer parity: the stage loops take their stream bases as buffer resources (SGPRs), so the buffer a pass addresses
// must be the wavefront's, while the lanes of a wavefront accept different numbers of steps (early stops, failed line
// searches, re-anchors).  Each lane's parity is a register (across launches: res_buf[l]); every pass runs for p = 0, 1
// with p wave-uniform, executed by the lanes whose parity is p, and an empty side is skipped (no lane enters the
// branch).  A unanimous wavefront runs each pass once.  The buffers are indexed by mpc_pass(p), never by p itself.
// Every loop is bounded (t1 - t0, iters, max_ls, N - t stages); no atomics, no spinning.  A lane_fence() separates a
// pass's stores from the next pass's loads of the same rows, and the arguments are re-read through kernarg<Args>() at
// each use, as in k_nt_run_limited.
// Outputs, written lane-major straight into the caller's lane order (row map[l], NULL: l; one row per step is no hot
// path): x_cl rows t and t + 1, u_cl row t, and per step the iterations, the rollouts (the re-anchor's included), the
// cost-to-go after the replan and the stop code (GYM_ACTIVE: all `iters` ran).
// ------------------------------------------------------------------------------------------
struct MpcRunArgs : BoxArgs {
    const gym_model* plant;       // (Bp) per-lane plants, internal lane order (padding lanes: any valid row)
    const int64_t* map;           // the output row of internal lane l (NULL: l)
    double *x_cl, *u_cl;          // (B,N,4), (B,T,2) applied states and controls
    int32_t *s_iter, *s_roll;     // (B,T)
    double* s_cost;               // (B,T)
    int32_t* s_stop;              // (B,T)
    int32_t t0, t1, iters, pad;
};
static_assert(sizeof(MpcRunArgs) == sizeof(BoxArgs) + 8 * 8 + 16,
              "kernarg layout: BoxArgs, then the loop's own fields");

// the lane's reference rows of horizon t (per-lane references: the full horizon's lane stride)
template <bool RL>
__device__ __forceinline__ const double* mpc_xr(const MpcRunArgs* R, int64_t l, int t) {
    return lane_ref<RL>(R->xr, l, 4 * (int64_t)R->N) + 4 * t;
}
template <bool RL>
__device__ __forceinline__ const double* mpc_ur(const MpcRunArgs* R, int64_t l, int t) {
    return lane_ref<RL>(R->ur, l, 2 * (int64_t)(R->N - 1)) + 2 * t;
}
// row t of a pair stream (x, K1) / a plane stream (u, cs): t stage strides of 2 Bp elements
template <class P>
__device__ __forceinline__ P* mpc_row(P* base, const MpcRunArgs* R, int t) {
    return base + (int64_t)t * 2 * R->Bp;
}
__device__ __forceinline__ bool mpc_any(bool v) { return __builtin_amdgcn_ballot_w64(v) != 0; }   // wave vote
// The pass index as the stage loops see it: an SGPR the compiler knows nothing about.  Inside "if (par == p)" it would
// otherwise replace p by the lane's parity (equal there, but a VGPR): every x[p] / u[p] base would become a per-lane
// value and every buffer access a waterfall loop of v_readfirstlane.
__device__ __forceinline__ int mpc_pass(int p) {
    asm volatile("" : "+s"(p));
    return p;
}

template <class V, bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_mpc_run(MpcRunArgs args) {
    typedef MpcRunArgs Args;
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= args.B) return;
    const V v(l);
    const Dyn pm = gym::model_row(kernarg_consts().m, kernarg<Args>()->plant, l);   // this thread's plant, read once
    int par = kernarg<Args>()->res_buf[l] & 1;
    for (int t = kernarg<Args>()->t0; t < kernarg<Args>()->t1; ++t) {
        int stop = GYM_ACTIVE, ni = 0, nr = 0;
        // ---- 1. replan on horizon t
        for (int k = 0; k < kernarg<Args>()->iters; ++k) {
            const bool act = stop == GYM_ACTIVE;
            if (!mpc_any(act)) break;
#pragma unroll 1
            for (int p = 0; p < 2; ++p) {
                const int q = mpc_pass(p);
                if (act && par == p) {
                    const Args* R = kernarg<Args>();
                    double d, s;
                    V::template sweep<U0Z, OUT_ALL>(v.model(R->m), v.weights(R->w), mpc_row(R->x[q], R, t),
                                                    mpc_row(R->u[q], R, t), mpc_xr<RL>(R, l, t), mpc_ur<RL>(R, l, t),
                                                    mpc_row(R->K1, R, t), mpc_row(R->cs, R, t), R->a.gamma0, l, R->Bp,
                                                    R->N - t, d, s, R->tau[l]);
                    const Args* Q = kernarg<Args>();
                    Q->dJ[l] = d;
                    Q->smax[l] = s;
                }
            }
            lane_fence();
            if (act && kernarg<Args>()->smax[l] < kernarg<Args>()->a.tol) stop = GYM_CONVERGED;   // before the trials
            const bool go = act && stop == GYM_ACTIVE;
            double Jn = 0.0, g = kernarg<Args>()->a.gamma0;
            bool ok = false;
            if (mpc_any(go)) {
#pragma unroll 1
                for (int p = 0; p < 2; ++p) {
                    const int q = mpc_pass(p);
                    if (go && par == p) {
                        const Args* R = kernarg<Args>();
                        const double2* xs = mpc_row(R->x[q], R, t);
                        const double2 xa = xs[wix(0, 0, 2, l, R->Bp)], xb = xs[wix(0, 1, 2, l, R->Bp)];
                        Jn = rollout_cform<true, U0Z, false, false, kNT, false, 1, true, V::LW>(
                            v.model(R->m), v.weights(R->w), mpc_row(R->u[q], R, t), mpc_row(R->K1, R, t),
                            mpc_row(R->cs, R, t), mpc_xr<RL>(R, l, t), mpc_ur<RL>(R, l, t), mpc_row(R->x[q ^ 1], R, t),
                            mpc_row(R->u[q ^ 1], R, t), R->a.gamma0, R->a.gamma0, l, R->Bp, R->N - t, xa.x, xa.y, xb.x,
                            xb.y, R->tau[l]);
                    }
                }
            }
            int nk = 0;
            if (go) {
                const Args* R = kernarg<Args>();
                nk = 1;
                ok = Jn < R->cost[l] + R->a.c * g * R->dJ[l];   // strict Armijo test (:361)
            }
            for (int j = 1; j < kernarg<Args>()->a.max_ls; ++j) {
                const bool again = go && !ok;
                if (!mpc_any(again)) break;
                if (again) g *= kernarg<Args>()->a.beta;   // gamma_i *= beta, sequentially (:365)
#pragma unroll 1
                for (int p = 0; p < 2; ++p) {
                    const int q = mpc_pass(p);
                    if (again && par == p) {
                        const Args* P = kernarg<Args>();
                        const double2* xs = mpc_row(P->x[q], P, t);
                        const double2 xa = xs[wix(0, 0, 2, l, P->Bp)], xb = xs[wix(0, 1, 2, l, P->Bp)];
                        Jn = rollout_cform<true, U0Z, true, false, kNT, false, 1, true, V::LW>(
                            v.model(P->m), v.weights(P->w), mpc_row(P->u[q], P, t), mpc_row(P->K1, P, t),
                            mpc_row(P->cs, P, t), mpc_xr<RL>(P, l, t), mpc_ur<RL>(P, l, t), mpc_row(P->x[q ^ 1], P, t),
                            mpc_row(P->u[q ^ 1], P, t), g, P->a.gamma0, l, P->Bp, P->N - t, xa.x, xa.y, xb.x, xb.y,
                            P->tau[l]);
                    }
                }
                if (again) {
                    const Args* Q = kernarg<Args>();
                    ++nk;
                    ok = Jn < Q->cost[l] + Q->a.c * g * Q->dJ[l];
                }
            }
            if (go) {
                const Args* F = kernarg<Args>();
                nr += nk;
                ni += 1;
                if (ok) {
                    F->cost[l] = Jn;
                    F->gamma[l] = g;
                    par ^= 1;
                } else {
                    stop = GYM_LS_FAILED;   // no update (:367-369): the plan stays
                }
            }
            lane_fence();   // the candidate buffer is the next sweep's input
        }
        // ---- 2. act: stage t of the plan on the lane's plant
        bool re;
        {
            const Args* R = kernarg<Args>();
            const int T = R->N - 1;
            const int64_t Bp = R->Bp;
            const int64_t row = R->map ? R->map[l] : l;
            const double2* xs = par ? R->x[1] : R->x[0];   // per-lane buffer select: plain loads, no buffer resource
            const double* us = par ? R->u[1] : R->u[0];
            const double2 xa = xs[wix(t, 0, 2, l, Bp)], xb = xs[wix(t, 1, 2, l, Bp)];
            const double u0 = U0Z ? 0.0 : us[pix(t, 0, 2, l, Bp)], u1 = us[pix(t, 1, 2, l, Bp)];
            const double* xrt = mpc_xr<RL>(R, l, t);
            const double* urt = mpc_ur<RL>(R, l, t);
            const double f0 = U0Z ? 0.0 : u0 - urt[0], f1 = u1 - urt[1];
            const KArgs ka = kernarg_consts();
            const double lt = stage_cost<U0Z>(0.0, ka.w.Q, ka.w.R, xa.x, xa.y, xb.x, xb.y, xrt, f0, f1);
            const double J = R->cost[l];
            R->cost[l] = J - lt;   // the cost-to-go of horizon t + 1
            double n0 = xa.x, n1 = xa.y, n2 = xb.x, n3 = xb.y;
            Dyn pl = pm;           // the plant's coefficients with the step sizes re-read from the kernel arguments
            pl.h = ka.m.h; pl.h2 = ka.m.h2; pl.h6 = ka.m.h6;
            gym::rk4_fast(pl, n0, n1, n2, n3, u1, gym::poly_vgprs());
            double* xo = R->x_cl + (row * R->N + t) * 4;
            xo[0] = xa.x; xo[1] = xa.y; xo[2] = xb.x; xo[3] = xb.y;
            xo[4] = n0; xo[5] = n1; xo[6] = n2; xo[7] = n3;   // row t + 1 (the last step's: x_T)
            double* uo = R->u_cl + (row * T + t) * 2;
            uo[0] = u0; uo[1] = u1;
            const int64_t si = row * T + t;
            R->s_iter[si] = ni;
            R->s_cost[si] = J;
            R->s_stop[si] = stop;
            re = false;
            if (t + 1 < T) {
                const double2 pa = xs[wix(t + 1, 0, 2, l, Bp)], pb = xs[wix(t + 1, 1, 2, l, Bp)];
                re = __double_as_longlong(pa.x) != __double_as_longlong(n0) ||
                     __double_as_longlong(pa.y) != __double_as_longlong(n1) ||
                     __double_as_longlong(pb.x) != __double_as_longlong(n2) ||
                     __double_as_longlong(pb.y) != __double_as_longlong(n3);
            }
        }
        // ---- 3. re-anchor the plan at the measured state (read back from x_cl row t + 1: not held across the sweep)
        if (mpc_any(re)) {
            lane_fence();
#pragma unroll 1
            for (int p = 0; p < 2; ++p) {
                const int q = mpc_pass(p);
                if (re && par == p) {
                    const Args* R = kernarg<Args>();
                    double d, s;
                    V::template sweep<U0Z, OUT_ALL>(v.model(R->m), v.weights(R->w), mpc_row(R->x[q], R, t + 1),
                                                    mpc_row(R->u[q], R, t + 1), mpc_xr<RL>(R, l, t + 1),
                                                    mpc_ur<RL>(R, l, t + 1), mpc_row(R->K1, R, t + 1),
                                                    mpc_row(R->cs, R, t + 1), R->a.gamma0, l, R->Bp, R->N - t - 1, d, s,
                                                    R->tau[l]);
                }
            }
            lane_fence();
#pragma unroll 1
            for (int p = 0; p < 2; ++p) {
                const int q = mpc_pass(p);
                if (re && par == p) {
                    const Args* R = kernarg<Args>();
                    const int64_t row = R->map ? R->map[l] : l;
                    const double* xn = R->x_cl + (row * R->N + t + 1) * 4;
                    const double Jn = rollout_cform<true, U0Z, true, false, kNT, false, 1, true, V::LW>(
                        v.model(R->m), v.weights(R->w), mpc_row(R->u[q], R, t + 1), mpc_row(R->K1, R, t + 1),
                        mpc_row(R->cs, R, t + 1), mpc_xr<RL>(R, l, t + 1), mpc_ur<RL>(R, l, t + 1),
                        mpc_row(R->x[q ^ 1], R, t + 1), mpc_row(R->u[q ^ 1], R, t + 1), 0.0, R->a.gamma0, l, R->Bp,
                        R->N - t - 1, xn[0], xn[1], xn[2], xn[3], R->tau[l]);
                    kernarg<Args>()->cost[l] = Jn;   // accepted unconditionally
                }
            }
            if (re) {
                par ^= 1;
                nr += 1;
            }
            lane_fence();
        }
        {
            const Args* R = kernarg<Args>();
            const int64_t row = R->map ? R->map[l] : l;
            R->s_roll[row * (R->N - 1) + t] = nr;
            R->n_iter[l] += ni;
            R->n_roll[l] += nr;
        }
    }
    kernarg<Args>()->res_buf[l] = par;
}
