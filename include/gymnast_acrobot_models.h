/*
 * gymnast_acrobot_models.h -- C-ABI of the Newton solve and the per-lane LQR design on per-lane models, an extension
 * of gymnast_acrobot.h.
 *
 * Additive to ABI 18: the structures, flags, status codes and conventions are gymnast_acrobot.h's (included below), no
 * entry point or structure of it changes, and all headers' entry points live in the same library.  A caller whose
 * lanes share one model does not need this header.
 */
#ifndef GYMNAST_ACROBOT_MODELS_H
#define GYMNAST_ACROBOT_MODELS_H

#include "gymnast_acrobot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- Per-lane models: every lane is planned on, or designed for, its own acrobot ----------------
 * models [device] (an array parameter, as gym_lqr_lanes_rollout_plant's plant[]): one gym_model row per lane (64 bytes
 * a row, 16-byte aligned), as gym_models_from_params makes them (dynamics.py:15-61 per row).  Lane l's whole computation uses models[l] where the mirrored entry point uses m: the
 * coefficients a, b, d, g1, g2, f1, f2 of dynamics.py:63-90, with b^2 and d (a - d) formed on the device by the same
 * single-rounded operations the host forms them with for m.  A row's dt is ignored: m supplies dt, and w and a stay per
 * batch.  Where every row equals m, every output is the mirrored entry point's bit for bit; lane l's outputs are those
 * of the mirrored entry point called with m = models[l], whatever the other rows hold.
 * For the three Newton entry points the table has Bp rows in internal lane order, like tau_max (padding lanes: any
 * valid row).  GYM_EINVAL with nothing launched: models NULL or not 16-byte aligned, any refusal of the mirrored entry
 * point, and for the Newton entry points GYM_FLAG_X_CKPT or GYM_FLAG_SIGMA_STREAM.
 * Additive to ABI 18: no existing entry point or structure changed. */
/* gym_newton_init (u_init NULL; simulate_open_loop + total_cost, trajectory_generation.py:74-87, 231-252, of u = 0) or
 * gym_newton_init_warm (u_init (B,T,2), status_init (B) or NULL) with each lane rolled out on its own row. */
int gym_newton_init_models(const gym_model* m, const gym_model models[], const gym_weights* w, const double* x0,
                           const double* u_init, const int32_t* status_init, const gym_batch* bt, void* stream);
/* gym_newton_run_box (gymnast_acrobot_box.h; newton_Algorithm's loop, trajectory_generation.py:329-396, sweep
 * :183-229) with the sweep's Jacobians (dynamics.py:157-170) and every Armijo rollout (:177-195) of lane l on
 * models[l].  tau_max [device]: (Bp) doubles in internal lane order, 0 < tau_max <= +inf, required: an unlimited solve
 * passes +inf in every lane.  Statistics of iteration k1-1 into stats[0,8); timing kind 8. */
int gym_newton_run_models(const gym_model* m, const gym_model models[], const gym_weights* w, const gym_armijo* a,
                          const gym_batch* bt, const double* tau_max, int32_t k0, int32_t k1, void* stream);
/* gym_newton_sigma_box on the table: sigma (B,T,2) of each lane's last completed iteration by re-running that
 * iteration's sweep (calculate_K_and_sigma, trajectory_generation.py:183-229) on the lane's row.  gym_newton_finalize
 * is then called with sigma_out = NULL. */
int gym_newton_sigma_models(const gym_model* m, const gym_model models[], const gym_weights* w, const gym_batch* bt,
                            const double* tau_max, double* sigma_out, void* stream);
/* gym_lqr_lanes_gains (solve_LQR_tracking, trajectory_tracking.py:170-203, per lane) with lane l linearised on
 * models[l]: (B) rows in the CALLER's lane order (this tracker has no internal order).  The workspace it fills is the
 * one gym_lqr_lanes_rollout / gym_lqr_lanes_rollout_plant take. */
int gym_lqr_lanes_gains_models(const gym_model* m, const gym_model models[], const double* x_opt, const double* u_opt,
                               int64_t B, int32_t N, const double Q[16], const double R[4], const double QT[16],
                               void* ws, int64_t ws_bytes, double* K_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMNAST_ACROBOT_MODELS_H */
