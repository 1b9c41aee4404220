// Newton solver kernels: the persistent solve on per-lane models (ModelsVariant; gym_newton_run_models, _sigma_models).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// newton_Algorithm (:329-396) with every lane planned on its own acrobot (dynamics.py:15-61 per lane): the limited
// solve (newton_limited.hpp) with a table of gym_model rows, one per lane in internal lane order.  Lane l's sweep takes
// its Jacobians (dynamics.py:157-170) and every Armijo trial its RK4 steps (:177-195) on row l; dt, the weights and the
// Armijo settings stay the batch's.  The thread reads its row once, before the iteration loop (gym::model_row: four
// 16-byte loads), and keeps the nine coefficients in VGPRs across the passes; h, h2, h6 and the whole KW are re-read
// from the kernel-argument segment at each pass, as in every persistent kernel.  Where the row is the batch model's
// the operands have the same bits and so has every result: the box solve's, and at tau = +inf k_nt_run's.
// ------------------------------------------------------------------------------------------
struct ModelArgs : BoxArgs {
    const gym_model* models;   // (Bp) per-lane models, internal lane order (padding lanes: any valid row)
};
static_assert(sizeof(ModelArgs) == sizeof(BoxArgs) + 8, "kernarg layout: BoxArgs, then the table");

struct ModelsVariant {
    typedef ModelArgs Args;
    static void extra(ModelArgs& a, const gym_model* rows) { a.models = rows; }
    Dyn pm;   // this thread's row, read once
    __device__ __forceinline__ ModelsVariant(int64_t l)
        : pm(gym::model_row(kernarg_consts().m, kernarg<ModelArgs>()->models, l)) {}
    __device__ __forceinline__ ModelsVariant(const Dyn& m, int64_t l, const gym_model* rows)
        : pm(gym::model_row(m, rows, l)) {}
    // this thread's model for one pass: its own coefficients with the step sizes re-read from the kernel arguments
    __device__ __forceinline__ Dyn model(const Dyn&) const {
        const KArgs ka = kernarg_consts();
        Dyn r = pm;
        r.h = ka.m.h; r.h2 = ka.m.h2; r.h6 = ka.m.h6;
        return r;
    }
    static constexpr bool LW = false;
    __device__ __forceinline__ const KW& weights(const KW& w) const { return w; }
    template <bool U0Z, int OUT>
    static constexpr auto sweep = backward_solver_lane_ilp<U0Z, OUT, true, true>;
};
