// Newton solver kernels: the torque-limited (box-constrained) persistent solve k_nt_run_limited and its sigma1 re-run
// k_nt_sigma_limited, written once for every variant (BoxVariant in newton_box.hpp, Rk4Variant in rk4_lin.hpp,
// ModelsVariant in newton_models.hpp, WeightsVariant in newton_weights.hpp).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// Control-limited form of newton_Algorithm (:329-396; control-limited DDP, Tassa, Mansard and Todorov 2014) for
// this model: only tau2 enters the dynamics, so each stage's box QP is a scalar clip.  Per lane a limit
// tau = tau_max[lane], 0 < tau <= +inf, and the invariant |u1_t| <= tau on every stage of every iterate (u = 0 at
// init satisfies it).
//   sweep (calculate_K_and_sigma :183-216), stage t: G11, F = row 1 of B^T P A_d, g1 = r1 + b^T p and the unlimited
//     step s1u = -g1 / G11 as Sweep::step_P / step_p compute them; lo = -tau - u1_t, hi = tau - u1_t; the stage is
//     clamped iff s1u < lo or s1u > hi.  Not clamped (a NaN s1u included): the unlimited stage, bit for bit.
//     Clamped: sigma1 = the bound, K row 1 = 0 (stored as zeros), P <- 2Q + A_d^T P A_d, p <- q + A_d^T p + F sigma1.
//     Either way dJ += r0 s0 + g1 s1, max|sigma| takes |s1|, cg = (u1 - k x) + gamma0 s1 with these values.
//   trials (forward_closed_loop_update :218-229): u1_new = clip(trial_u1 / trial_u1_sig, -tau, tau) (box_clip: a NaN
//     stays NaN) before the cost, the store and the RK4 step.
// The Armijo test, gamma <- beta gamma, the update, the stop test, LS failure, statuses, counters and histories are
// k_nt_run's.  With tau = +inf no comparison is ever true and every value is k_nt_run's: the same bits.
// The sweep always stores sigma1 (OUT_ALL), so a lane that backtracks needs no sigma1 re-run.
//
// A variant V says what differs between the limited solves, and nothing else:
//   V::Args                      the run kernel's argument struct, BoxArgs or derived from it
//   V::extra(Args&, table...)    host: fills the fields Args adds to BoxArgs from the entry point's extra arguments
//   V(l) / V(m, l, table...)     what a thread reads once, before the iteration loop / in the sigma1 re-run
//   v.model(m)                   the model of one pass, from the batch's (re-read from the kernel arguments per pass)
//   v.weights(w)                 the cost weights of one pass, from the batch's: w untouched, or this thread's own
//   V::LW                        whether v.weights(w) is the thread's own, so that the trials take them as handed
//                                (rollout_cform's LW) instead of re-reading the batch's per stage
//   V::sweep<U0Z, OUT>(m, ...)   the lane's backward sweep, called with backward_solver_lane_ilp's operands.  Where it
//                                is that function, V names it (a constexpr alias) rather than wrapping it: through
//                                one more inlined call the compiler numbers the kernel's registers differently
// ------------------------------------------------------------------------------------------
struct BoxArgs : RunArgs {
    const double* tau;   // (Bp) per-lane limits, internal lane order (padding lanes: any positive value)
};
static_assert(sizeof(BoxArgs) == sizeof(RunArgs) + 8, "kernarg layout: RunArgs, then the limits");

// The persistent kernel of gym_newton_run_box / _rk4 / _models / _weights: lane l's outer iterations k0 .. k1-1, as k_nt_run.
// The arguments are re-read through kernarg<Args>() at each use (newton_run.hpp: no pointer held across a stage loop).
template <class V, bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_run_limited(typename V::Args args) {
    typedef typename V::Args Args;
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= args.B) return;
    const V v(l);
    int st = kernarg<Args>()->status[l];
    for (int k = kernarg<Args>()->k0; st == GYM_ACTIVE && k < kernarg<Args>()->k1; ++k) {
        const int cb = k & 1;
        {
            const Args* R = kernarg<Args>();
            double d, s;
            V::template sweep<U0Z, OUT_ALL>(v.model(R->m), v.weights(R->w), R->x[cb], R->u[cb], run_xr<RL>(R, l), run_ur<RL>(R, l),
                                            R->K1, R->cs, R->a.gamma0, l, R->Bp, R->N, d, s, R->tau[l]);
            const Args* Q = kernarg<Args>();
            Q->dJ[l] = d;
            Q->smax[l] = s;
            if (Q->hist_smax && k < Q->a.hist_len) Q->hist_smax[(int64_t)k * Q->Bp + l] = s;
        }
        lane_fence();
        double Jn;
        {
            const Args* R = kernarg<Args>();
            const double2 xa = R->x[cb][wix(0, 0, 2, l, R->Bp)], xb = R->x[cb][wix(0, 1, 2, l, R->Bp)];
            Jn = rollout_cform<true, U0Z, false, false, kNT, false, 1, true, V::LW>(
                v.model(R->m), v.weights(R->w), R->u[cb], R->K1, R->cs, run_xr<RL>(R, l), run_ur<RL>(R, l), R->x[cb ^ 1],
                R->u[cb ^ 1], R->a.gamma0, R->a.gamma0, l, R->Bp, R->N, xa.x, xa.y, xb.x, xb.y, R->tau[l]);
        }
        const Args* R = kernarg<Args>();
        double g = R->a.gamma0;
        int nr = 1;
        bool ok = Jn < R->cost[l] + R->a.c * g * R->dJ[l];   // strict Armijo test (:361)
        for (int j = 1; !ok && j < kernarg<Args>()->a.max_ls; ++j) {
            const Args* P = kernarg<Args>();
            g *= P->a.beta;   // gamma_i *= beta, sequentially (:365)
            const double2 xa = P->x[cb][wix(0, 0, 2, l, P->Bp)], xb = P->x[cb][wix(0, 1, 2, l, P->Bp)];
            Jn = rollout_cform<true, U0Z, true, false, kNT, false, 1, true, V::LW>(
                v.model(P->m), v.weights(P->w), P->u[cb], P->K1, P->cs, run_xr<RL>(P, l), run_ur<RL>(P, l), P->x[cb ^ 1],
                P->u[cb ^ 1], g, P->a.gamma0, l, P->Bp, P->N, xa.x, xa.y, xb.x, xb.y, P->tau[l]);
            ++nr;
            const Args* Q = kernarg<Args>();
            ok = Jn < Q->cost[l] + Q->a.c * g * Q->dJ[l];
        }
        const Args* F = kernarg<Args>();
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
}

// sigma1 of each lane's last completed iteration of a limited solve: that iteration's sweep re-run (same inputs, same
// code: the same bits) into the sigma1 plane.  One launch per buffer parity, as k_nt_sigma's final mode.  table: the
// entry point's extra arguments (ModelsVariant: the per-lane models, WeightsVariant: the per-lane weights), none for
// the other variants.
template <class V, bool U0Z, bool RL, class... T>
__global__ __launch_bounds__(BLK, 1) void k_nt_sigma_limited(Dyn m, KW w, const double2* __restrict__ x,
                                                             const double* __restrict__ u,
                                                             const double* __restrict__ xr,
                                                             const double* __restrict__ ur, double* __restrict__ cs,
                                                             const double* __restrict__ tau,
                                                             const int32_t* __restrict__ n_iter, int parity, int64_t B,
                                                             int64_t Bp, int N, T __restrict__... table) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const int it = n_iter[l];
    if (it <= 0 || ((it - 1) & 1) != parity) return;
    const V v(m, l, table...);
    double d, s;
    V::template sweep<U0Z, OUT_SIGMA>(v.model(m), v.weights(w), x, u, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                      lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), nullptr, cs, 0.0, l, Bp, N, d, s,
                                      tau[l]);
}
