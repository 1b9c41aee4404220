// Newton solver kernels: the torque-limited (box-constrained) persistent solve, k_nt_run_box / k_nt_sigma_box.
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
// ------------------------------------------------------------------------------------------
struct BoxArgs : RunArgs {
    const double* tau;   // (Bp) per-lane limits, internal lane order (padding lanes: any positive value)
};
static_assert(sizeof(BoxArgs) == sizeof(RunArgs) + 8, "kernarg layout: RunArgs, then the limits");

template <bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_run_box(BoxArgs args) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= args.B) return;
    int st = kernarg<BoxArgs>()->status[l];
    for (int k = kernarg<BoxArgs>()->k0; st == GYM_ACTIVE && k < kernarg<BoxArgs>()->k1; ++k) {
        const int cb = k & 1;
        {
            const BoxArgs* R = kernarg<BoxArgs>();
            double d, s;
            backward_solver_lane_ilp<U0Z, OUT_ALL, true>(R->m, R->w, R->x[cb], R->u[cb], run_xr<RL>(R, l),
                                                         run_ur<RL>(R, l), R->K1, R->cs, R->a.gamma0, l, R->Bp, R->N,
                                                         d, s, R->tau[l]);
            const BoxArgs* Q = kernarg<BoxArgs>();
            Q->dJ[l] = d;
            Q->smax[l] = s;
            if (Q->hist_smax && k < Q->a.hist_len) Q->hist_smax[(int64_t)k * Q->Bp + l] = s;
        }
        lane_fence();
        double Jn;
        {
            const BoxArgs* R = kernarg<BoxArgs>();
            const double2 xa = R->x[cb][wix(0, 0, 2, l, R->Bp)], xb = R->x[cb][wix(0, 1, 2, l, R->Bp)];
            Jn = rollout_cform<true, U0Z, false, false, kNT, false, 1, true>(
                R->m, R->w, R->u[cb], R->K1, R->cs, run_xr<RL>(R, l), run_ur<RL>(R, l), R->x[cb ^ 1], R->u[cb ^ 1],
                R->a.gamma0, R->a.gamma0, l, R->Bp, R->N, xa.x, xa.y, xb.x, xb.y, R->tau[l]);
        }
        const BoxArgs* R = kernarg<BoxArgs>();
        double g = R->a.gamma0;
        int nr = 1;
        bool ok = Jn < R->cost[l] + R->a.c * g * R->dJ[l];   // strict Armijo test (:361)
        for (int j = 1; !ok && j < kernarg<BoxArgs>()->a.max_ls; ++j) {
            const BoxArgs* P = kernarg<BoxArgs>();
            g *= P->a.beta;   // gamma_i *= beta, sequentially (:365)
            const double2 xa = P->x[cb][wix(0, 0, 2, l, P->Bp)], xb = P->x[cb][wix(0, 1, 2, l, P->Bp)];
            Jn = rollout_cform<true, U0Z, true, false, kNT, false, 1, true>(
                P->m, P->w, P->u[cb], P->K1, P->cs, run_xr<RL>(P, l), run_ur<RL>(P, l), P->x[cb ^ 1], P->u[cb ^ 1], g,
                P->a.gamma0, l, P->Bp, P->N, xa.x, xa.y, xb.x, xb.y, P->tau[l]);
            ++nr;
            const BoxArgs* Q = kernarg<BoxArgs>();
            ok = Jn < Q->cost[l] + Q->a.c * g * Q->dJ[l];
        }
        const BoxArgs* F = kernarg<BoxArgs>();
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

// sigma1 of each lane's last completed iteration with the limit: that iteration's box sweep re-run (same inputs,
// same code: the same bits) into the sigma1 plane.  One launch per buffer parity, as k_nt_sigma's final mode.
template <bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_sigma_box(Dyn m, KW w, const double2* __restrict__ x,
                                                         const double* __restrict__ u, const double* __restrict__ xr,
                                                         const double* __restrict__ ur, double* __restrict__ cs,
                                                         const double* __restrict__ tau,
                                                         const int32_t* __restrict__ n_iter, int parity, int64_t B,
                                                         int64_t Bp, int N) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const int it = n_iter[l];
    if (it <= 0 || ((it - 1) & 1) != parity) return;
    double d, s;
    backward_solver_lane_ilp<U0Z, OUT_SIGMA, true>(m, w, x, u, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                                   lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), nullptr, cs, 0.0, l, Bp, N,
                                                   d, s, tau[l]);
}
