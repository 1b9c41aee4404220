// Newton solver kernels: the persistent solve on per-lane cost weights (WeightsVariant; gym_newton_run_weights,
// _sigma_weights).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// ------------------------------------------------------------------------------------------
// newton_Algorithm (:329-396) with every lane planned under its own Q, R, Q_T (total_cost :231-252 and the stage
// blocks Q_t = 2Q, R_t = 2R of build_stage_lists :166-181 per lane): the limited solve (newton_limited.hpp) with a
// table of gym_weights rows, one per lane in internal lane order.  Lane l's sweep takes its stage and terminal blocks,
// G and sigma0, and every Armijo trial its cost, from row l; the model, dt and the Armijo settings stay the batch's.
// The thread reads its row once, before the iteration loop (weights_row: five 16-byte loads), forms the KW of it with
// kw() -- the function the host forms the batch's with -- and keeps the 17 doubles in VGPRs across the passes; the
// model with h, h2, h6 is re-read from the kernel-argument segment at each pass, as in every persistent kernel.  Where
// the row is the batch's weights the operands have the same bits and so has every result: the box solve's, and at
// tau = +inf k_nt_run's.
// ------------------------------------------------------------------------------------------
struct WeightArgs : BoxArgs {
    const gym_weights* weights;   // (Bp) per-lane weights, internal lane order (padding lanes: any valid row)
};
static_assert(sizeof(WeightArgs) == sizeof(BoxArgs) + 8, "kernarg layout: BoxArgs, then the table");
static_assert(sizeof(gym_weights) == 80, "a table row is five 16-byte pairs");

// Row `row` of a device table of gym_weights (80 bytes a row, 16-byte aligned: five 16-byte loads).
__device__ __forceinline__ gym_weights weights_row(const gym_weights* rows, int64_t row) {
    const double2* r = reinterpret_cast<const double2*>(rows + row);
    const double2 q0 = r[0], q1 = r[1], rr = r[2], t0 = r[3], t1 = r[4];
    return gym_weights{{q0.x, q0.y, q1.x, q1.y}, {rr.x, rr.y}, {t0.x, t0.y, t1.x, t1.y}};
}

struct WeightsVariant {
    typedef WeightArgs Args;
    static void extra(WeightArgs& a, const gym_weights* rows) { a.weights = rows; }
    KW pw;   // this thread's weights, read and derived once
    __device__ __forceinline__ WeightsVariant(int64_t l) : pw(kw(weights_row(kernarg<WeightArgs>()->weights, l))) {}
    __device__ __forceinline__ WeightsVariant(const Dyn&, int64_t l, const gym_weights* rows)
        : pw(kw(weights_row(rows, l))) {}
    __device__ __forceinline__ const Dyn& model(const Dyn& m) const { return m; }
    static constexpr bool LW = true;
    __device__ __forceinline__ const KW& weights(const KW&) const { return pw; }
    template <bool U0Z, int OUT>
    static constexpr auto sweep = backward_solver_lane_ilp<U0Z, OUT, true, false, true>;
};

// sigma of each lane's last iteration as SrcSigma unpacks it, with sigma0 = -(2R0 (u0 - ur0)) / (2R0) on the lane's
// own R0 (kw() of its row: the sweep's G00 and 1/G00, the same bits)
struct SrcSigmaRows {
    const gym_weights* rows;
    const double *cs, *u0b, *u1b, *ur;
    const int32_t* n_iter;
    int64_t ur_lane;   // per-lane references: doubles per lane of u_ref (0: shared)
    __device__ __forceinline__ double operator()(int64_t t, int c, int64_t lane, int64_t Bp) const {
        const int it = n_iter[lane];
        if (it <= 0) return 0.0;
        if (c == 1) return cs[pix((int)t, 1, 2, lane, Bp)];
        const double* u = ((it - 1) & 1) ? u1b : u0b;
        const KW w = kw(rows[lane]);   // (only G00 and 1/G00 survive)
        return -(w.G00 * (u[pix((int)t, 0, 2, lane, Bp)] - ur[lane * ur_lane + 2 * t])) * w.iG00;
    }
};
