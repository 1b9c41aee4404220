// Newton solver kernels: the persistent solve on per-lane models, k_nt_run_models / k_nt_sigma_models.
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// newton_Algorithm (:329-396) with every lane planned on its own acrobot (dynamics.py:15-61 per lane): the box
// solver (newton_box.hpp) with a table of gym_model rows, one per lane in internal lane order.  Lane l's sweep takes
// its Jacobians (dynamics.py:157-170) and every Armijo trial its RK4 steps (:177-195) on row l; dt, the weights and the
// Armijo settings stay the batch's.  The thread reads its row once, before the iteration loop (gym::model_row: four
// 16-byte loads), and keeps the nine coefficients in VGPRs across the passes; h, h2, h6 and the whole KW are re-read
// from the kernel-argument segment at each pass (kernarg_consts), as in every persistent kernel.  Where the row is the
// batch model's the operands have the same bits and so has every result: k_nt_run_box's, and at tau = +inf
// k_nt_run's.  The loop below repeats k_nt_run_box's text (as k_nt_run_rk4 does): only the model operand of the sweep
// and of the trials differs.
// ------------------------------------------------------------------------------------------
struct ModelArgs : BoxArgs {
    const gym_model* models;   // (Bp) per-lane models, internal lane order (padding lanes: any valid row)
};
static_assert(sizeof(ModelArgs) == sizeof(BoxArgs) + 8, "kernarg layout: BoxArgs, then the table");

// this thread's model for one pass: its own coefficients with the step sizes re-read from the kernel arguments
__device__ __forceinline__ Dyn lane_model(Dyn pm) {
    const KArgs ka = kernarg_consts();
    pm.h = ka.m.h; pm.h2 = ka.m.h2; pm.h6 = ka.m.h6;
    return pm;
}

template <bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_run_models(ModelArgs args) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= args.B) return;
    const Dyn pm = gym::model_row(kernarg_consts().m, kernarg<ModelArgs>()->models, l);
    int st = kernarg<ModelArgs>()->status[l];
    for (int k = kernarg<ModelArgs>()->k0; st == GYM_ACTIVE && k < kernarg<ModelArgs>()->k1; ++k) {
        const int cb = k & 1;
        {
            const ModelArgs* R = kernarg<ModelArgs>();
            double d, s;
            backward_solver_lane_ilp<U0Z, OUT_ALL, true, true>(lane_model(pm), R->w, R->x[cb], R->u[cb],
                                                               run_xr<RL>(R, l), run_ur<RL>(R, l), R->K1, R->cs,
                                                               R->a.gamma0, l, R->Bp, R->N, d, s, R->tau[l]);
            const ModelArgs* Q = kernarg<ModelArgs>();
            Q->dJ[l] = d;
            Q->smax[l] = s;
            if (Q->hist_smax && k < Q->a.hist_len) Q->hist_smax[(int64_t)k * Q->Bp + l] = s;
        }
        lane_fence();
        double Jn;
        {
            const ModelArgs* R = kernarg<ModelArgs>();
            const double2 xa = R->x[cb][wix(0, 0, 2, l, R->Bp)], xb = R->x[cb][wix(0, 1, 2, l, R->Bp)];
            Jn = rollout_cform<true, U0Z, false, false, kNT, false, 1, true>(
                lane_model(pm), R->w, R->u[cb], R->K1, R->cs, run_xr<RL>(R, l), run_ur<RL>(R, l), R->x[cb ^ 1],
                R->u[cb ^ 1], R->a.gamma0, R->a.gamma0, l, R->Bp, R->N, xa.x, xa.y, xb.x, xb.y, R->tau[l]);
        }
        const ModelArgs* R = kernarg<ModelArgs>();
        double g = R->a.gamma0;
        int nr = 1;
        bool ok = Jn < R->cost[l] + R->a.c * g * R->dJ[l];   // strict Armijo test (:361)
        for (int j = 1; !ok && j < kernarg<ModelArgs>()->a.max_ls; ++j) {
            const ModelArgs* P = kernarg<ModelArgs>();
            g *= P->a.beta;   // gamma_i *= beta, sequentially (:365)
            const double2 xa = P->x[cb][wix(0, 0, 2, l, P->Bp)], xb = P->x[cb][wix(0, 1, 2, l, P->Bp)];
            Jn = rollout_cform<true, U0Z, true, false, kNT, false, 1, true>(
                lane_model(pm), P->w, P->u[cb], P->K1, P->cs, run_xr<RL>(P, l), run_ur<RL>(P, l), P->x[cb ^ 1],
                P->u[cb ^ 1], g, P->a.gamma0, l, P->Bp, P->N, xa.x, xa.y, xb.x, xb.y, P->tau[l]);
            ++nr;
            const ModelArgs* Q = kernarg<ModelArgs>();
            ok = Jn < Q->cost[l] + Q->a.c * g * Q->dJ[l];
        }
        const ModelArgs* F = kernarg<ModelArgs>();
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

// sigma1 of each lane's last completed iteration on its own model: k_nt_sigma_box with the table (that iteration's
// sweep re-run: same inputs, same code, the same bits).  One launch per buffer parity.
template <bool U0Z, bool RL>
__global__ __launch_bounds__(BLK, 1) void k_nt_sigma_models(Dyn m, KW w, const double2* __restrict__ x,
                                                            const double* __restrict__ u,
                                                            const double* __restrict__ xr,
                                                            const double* __restrict__ ur, double* __restrict__ cs,
                                                            const double* __restrict__ tau,
                                                            const int32_t* __restrict__ n_iter, int parity, int64_t B,
                                                            int64_t Bp, int N, const gym_model* __restrict__ models) {
    const int64_t l = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (l >= B) return;
    const int it = n_iter[l];
    if (it <= 0 || ((it - 1) & 1) != parity) return;
    const Dyn pm = gym::model_row(m, models, l);
    double d, s;
    backward_solver_lane_ilp<U0Z, OUT_SIGMA, true, true>(pm, w, x, u, lane_ref<RL>(xr, l, 4 * (int64_t)N),
                                                         lane_ref<RL>(ur, l, 2 * (int64_t)(N - 1)), nullptr, cs, 0.0,
                                                         l, Bp, N, d, s, tau[l]);
}
