// Newton solver kernels: the plain variant of newton_limited.hpp's torque-limited (box-constrained) persistent solve
// (gym_newton_run_box / gym_newton_sigma_box): the batch's model, the forward-Euler sweep.
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

struct BoxVariant {
    typedef BoxArgs Args;
    static void extra(BoxArgs&) {}
    __device__ __forceinline__ BoxVariant(int64_t) {}
    __device__ __forceinline__ BoxVariant(const Dyn&, int64_t) {}
    __device__ __forceinline__ const Dyn& model(const Dyn& m) const { return m; }
    static constexpr bool LW = false;
    __device__ __forceinline__ const KW& weights(const KW& w) const { return w; }
    template <bool U0Z, int OUT>
    static constexpr auto sweep = backward_solver_lane_ilp<U0Z, OUT, true>;
};
