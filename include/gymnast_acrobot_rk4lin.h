/*
 * gymnast_acrobot_rk4lin.h -- C-ABI of the Newton solve on the RK4-exact linearisation, an extension of
 * gymnast_acrobot.h.
 *
 * Additive to ABI 18: the structures, flags, status codes and conventions are gymnast_acrobot.h's (included below), no
 * entry point or structure of it changes, and all headers' entry points live in the same library.  A caller that
 * plans on the reference's forward-Euler linearisation does not need this header.
 */
#ifndef GYMNAST_ACROBOT_RK4LIN_H
#define GYMNAST_ACROBOT_RK4LIN_H

#include "gymnast_acrobot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- RK4-exact linearisation: the stage matrices are the Jacobians of the RK4 step itself ----------------
 * newton_Algorithm's sweep linearises by forward Euler (A_d = I + dt A_c, trajectory_generation.py:161-164) while
 * every rollout is RK4 (dynamics.py:177-195), so its dJ is not the directional derivative of the cost the Armijo test
 * (:361) measures and the search stalls short of a small tol.  Here A_d = d rk4(x, u) / dx and B_d = d rk4(x, u) / du at
 * (x_t, u_t), by the chain rule through the step's four stage points X1 = x, X2 = x + h/2 k1, X3 = x + h/2 k2,
 * X4 = x + h k3 with J_i, B_i the continuous Jacobians (dynamics.py:157-170) at (X_i, u):
 *   d1 = J1, d2 = J2 (I + h/2 d1), d3 = J3 (I + h/2 d2), d4 = J4 (I + h d3), A_d = I + h/6 (d1 + 2 d2 + 2 d3 + d4)
 *   e1 = B1, e2 = J2 (h/2 e1) + B2, e3 = J3 (h/2 e2) + B3, e4 = J4 (h e3) + B4, B_d = h/6 (e1 + 2 e2 + 2 e3 + e4)
 * Column 0 of B_d is exactly zero (tau1 never enters the dynamics, dynamics.py:205): K row 0 stays zero and the
 * solver's streams (K row 1, cg, sigma1) are gym_newton_run's.
 * Additive to ABI 18: no existing entry point or structure changed. */
/* gym_linearize (build_stage_lists, trajectory_generation.py:166-181) with these Jacobians: the same arguments and
 * output planes A_d (T,16,Bp), B_d (T,8,Bp), q (T,4,Bp), r (T,2,Bp), qT (4,Bp); q, r, qT are gym_linearize's bits.
 * GYM_EINVAL: a NULL pointer, bad sizes. */
int gym_linearize_rk4(const gym_model* m, const gym_weights* w, const double* x, const double* u, const double* x_ref,
                      const double* u_ref, double* Ad, double* Bd, double* q, double* r, double* qT, int64_t B,
                      int64_t Bp, int32_t N, void* stream);
/* gym_newton_run_box (gymnast_acrobot_box.h) with the sweep on this linearisation: the single-wavefront persistent
 * kernel, the control-limited stage and the clipped trials of the box solve, the loop of trajectory_generation.py
 * :329-396.  tau_max [device]: (Bp) doubles in internal lane order, 0 < tau_max <= +inf, required: an unlimited solve
 * passes +inf in every lane.  Statistics of iteration k1-1 into stats[0,8); timing kind 8.  GYM_EINVAL: tau_max NULL,
 * gym_newton_run's own checks, GYM_FLAG_X_CKPT, GYM_FLAG_SIGMA_STREAM. */
int gym_newton_run_rk4(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* bt,
                       const double* tau_max, int32_t k0, int32_t k1, void* stream);
/* gym_newton_sigma_box with this linearisation: sigma (B,T,2) of each lane's last completed iteration by re-running
 * that iteration's sweep.  gym_newton_finalize is then called with sigma_out = NULL.  GYM_EINVAL: a NULL pointer, a
 * bad batch, GYM_FLAG_X_CKPT. */
int gym_newton_sigma_rk4(const gym_model* m, const gym_weights* w, const gym_batch* bt, const double* tau_max,
                         double* sigma_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMNAST_ACROBOT_RK4LIN_H */
