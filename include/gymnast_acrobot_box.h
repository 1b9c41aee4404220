/*
 * gymnast_acrobot_box.h -- C-ABI of the torque-limited Newton solve, an extension of gymnast_acrobot.h.
 *
 * Additive to ABI 18: the structures, flags, status codes and conventions are gymnast_acrobot.h's (included below), no
 * entry point or structure of it changes, and both headers' entry points live in the same library.  A caller that
 * plans without an actuator limit does not need this header.
 */
#ifndef GYMNAST_ACROBOT_BOX_H
#define GYMNAST_ACROBOT_BOX_H

#include "gymnast_acrobot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- Torque-limited Newton solve: |tau2| <= tau_max[lane] on every stage of every iterate ----------------
 * The control-limited form of newton_Algorithm (control-limited DDP, Tassa, Mansard and Todorov 2014), specialised to
 * this model: only tau2 enters the dynamics (dynamics.py:205), so each stage's box QP is a scalar clip.  tau_max
 * [device]: (Bp) doubles in internal lane order, 0 < tau_max <= +inf (padding lanes: any positive value); the
 * caller's contract is |u[:, 1]| <= tau_max at init (u = 0 of gym_newton_init always; a u_init of gym_newton_init_warm
 * inside its lane's box).
 *   Backward sweep (calculate_K_and_sigma, trajectory_generation.py:183-229 with forward_closed_loop_update), stage t:
 *     G11, F = row 1 of B^T P A_d, g1 = r1 + b^T p and the unlimited step s1u = -g1 / G11 as the unlimited sweep has
 *     them; lo = -tau_max - u1_t, hi = tau_max - u1_t.  The stage is clamped iff s1u < lo or s1u > hi.  Not clamped
 *     (a NaN s1u included): the unlimited stage.  Clamped: sigma1 = the bound it crossed, K_t row 1 = 0,
 *     P <- 2Q + A_d^T P A_d, p <- q + A_d^T p + F sigma1.  dJ and max|sigma| take the clamped sigma1.
 *   Armijo trials (:218-229): u1_new clipped to [-tau_max, tau_max] (a NaN stays NaN) before the cost and the RK4 step.
 * Everything else is newton_Algorithm's loop (:329-396) as gym_newton_run runs it.  With tau_max = +inf, or any
 * limit that never binds, every output is gym_newton_run's bit for bit.
 * Additive to ABI 18: no existing entry point or structure changed. */
/* gym_newton_run with the limit (trajectory_generation.py:329-396; sweep :183-229): every ACTIVE lane's iterations
 * k0 .. k1-1 in ONE launch of the single-wavefront persistent kernel, its sweep storing sigma1 (no re-run for lanes
 * that backtrack), then the statistics of iteration k1-1 into stats[0,8); timing kind 8.  GYM_EINVAL: tau_max NULL,
 * gym_newton_run's own checks, GYM_FLAG_X_CKPT, GYM_FLAG_SIGMA_STREAM. */
int gym_newton_run_box(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* bt,
                       const double* tau_max, int32_t k0, int32_t k1, void* stream);
/* gym_newton_sigma with the limit (trajectory_generation.py:183-229): sigma (B,T,2) of each lane's last completed
 * iteration by re-running that iteration's box sweep, so a limited solve's sigma is never the unlimited one.
 * gym_newton_finalize is then called with sigma_out = NULL; its K_out comes from the stored K row 1, where clamped
 * stages are zero rows.  GYM_EINVAL: a NULL pointer, a bad batch, GYM_FLAG_X_CKPT. */
int gym_newton_sigma_box(const gym_model* m, const gym_weights* w, const gym_batch* bt, const double* tau_max,
                         double* sigma_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMNAST_ACROBOT_BOX_H */
