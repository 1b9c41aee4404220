/*
 * gymnast_newton_weights.h -- C-ABI of the Newton solve on per-lane cost weights, an add-on to gymnast_acrobot.h.
 *
 * Additive to ABI 18: the structures, flags, status codes and conventions are gymnast_acrobot.h's (included below), no
 * entry point or structure of it changes, and all headers' entry points live in the same library.  The lists of ABI 18
 * (the main header's prototypes and its gymnast_acrobot_*.h extensions) are closed; this header stands beside them.  A
 * caller whose lanes share one set of weights does not need it.
 */
#ifndef GYMNAST_NEWTON_WEIGHTS_H
#define GYMNAST_NEWTON_WEIGHTS_H

#include "gymnast_acrobot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- Per-lane weights: every lane is planned under its own Q, R, Q_T ----------------
 * weights [device] (an array parameter, as gym_newton_run_models' models[]): one gym_weights row per lane (80 bytes a
 * row, 16-byte aligned), Bp rows in internal lane order like tau_max (padding lanes: any valid row).  Lane l's whole
 * computation uses weights[l] where the mirrored entry point uses w: the cost of the start (total_cost,
 * trajectory_generation.py:231-252), the sweep's stage and terminal blocks Q_t = 2Q, R_t = 2R, P_N = 2Q_T
 * (build_stage_lists :166-181, calculate_K_and_sigma :183-216) and every Armijo trial's cost (:352-365).  2Q, 2R and
 * 1 / (2 R0) are formed on the device by the single-rounded operations the host forms them with for w (the reciprocal
 * by IEEE division).  Every row needs R > 0 and Q, Q_T >= 0, all finite; the library does not check the rows.  m, a and
 * dt stay per batch; w is still required (it is what a lane without a row of its own would use, and no lane is).
 * Where every row equals w, every output is the mirrored entry point's bit for bit; lane l's outputs are those of the
 * mirrored entry point called with w = weights[l], whatever the other rows hold.
 * GYM_EINVAL with nothing launched: weights NULL or not 16-byte aligned, any refusal of the mirrored entry point,
 * GYM_FLAG_X_CKPT or GYM_FLAG_SIGMA_STREAM. */
/* gym_newton_init (u_init NULL; simulate_open_loop + total_cost, trajectory_generation.py:74-87, 231-252, of u = 0) or
 * gym_newton_init_warm (u_init (B,T,2), status_init (B) or NULL) with each lane's first cost on its own row. */
int gym_newton_init_weights(const gym_model* m, const gym_weights* w, const gym_weights weights[], const double* x0,
                            const double* u_init, const int32_t* status_init, const gym_batch* bt, void* stream);
/* gym_newton_run_box (gymnast_acrobot_box.h; newton_Algorithm's loop, trajectory_generation.py:329-396, sweep
 * :183-229) with lane l's sweep and every Armijo trial's cost on weights[l].  tau_max [device]: (Bp) doubles in internal
 * lane order, 0 < tau_max <= +inf, required: an unlimited solve passes +inf in every lane.  Statistics of iteration
 * k1-1 into stats[0,8); timing kind 8. */
int gym_newton_run_weights(const gym_model* m, const gym_weights* w, const gym_weights weights[], const gym_armijo* a,
                           const gym_batch* bt, const double* tau_max, int32_t k0, int32_t k1, void* stream);
/* gym_newton_sigma_box on the table: sigma (B,T,2) of each lane's last completed iteration by re-running that
 * iteration's sweep (calculate_K_and_sigma, trajectory_generation.py:183-229) on the lane's row; sigma0 =
 * -(2 R0 (u0 - ur0)) / (2 R0) with the row's R0.  gym_newton_finalize is then called with sigma_out = NULL. */
int gym_newton_sigma_weights(const gym_model* m, const gym_weights* w, const gym_weights weights[],
                             const gym_batch* bt, const double* tau_max, double* sigma_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMNAST_NEWTON_WEIGHTS_H */
