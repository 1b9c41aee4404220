/*
 * gymnast/newton_mpc.h -- C-ABI of closed-loop replanning (shrinking-horizon nonlinear MPC) on the batched Newton
 * solver, a module of gymnast_acrobot.h.
 *
 * Additive to ABI 18: the structures, flags, status codes and conventions are gymnast_acrobot.h's (included below), no
 * entry point or structure of it changes, and all headers' entry points live in the same library.  A module declares
 * prototypes only.  A caller that only plans does not need this header.
 */
#ifndef GYMNAST_NEWTON_MPC_H
#define GYMNAST_NEWTON_MPC_H

#include "gymnast_acrobot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- One closed loop per lane: replan, act, re-anchor at every control step ----------------
 * After gym_newton_init / gym_newton_init_warm lane l holds a plan over the knots 0 .. N-1 and its cost.  Control
 * steps t0 .. t1-1 (0 <= t0 <= t1 <= T = N-1) of every lane run back to back in one launch; step t works on the
 * horizon of stages t .. T-1:
 *   1. replan: up to `iters` iterations of gym_newton_run_box's loop body (gymnast_acrobot_box.h: box sweep with the
 *      lane's tau_max, Armijo trials gamma0, gamma0 beta, ... up to max_ls, the strict test).  The stop test comes
 *      after the sweep and BEFORE the trials: max|sigma| < tol keeps the plan, runs no trial and ends the step as
 *      GYM_CONVERGED; an Armijo failure keeps the plan and ends the step as GYM_LS_FAILED.  Either ends this step only.
 *   2. act: u_t = stage t of the plan, x_t = its knot t; x_{t+1} = RK4(plant[l], x_t, u_t) (dynamics.py:177-195 on
 *      the lane's own plant row); the cost-to-go becomes J - l_t, l_t the stage cost of stage t.
 *   3. re-anchor, only if t+1 < T and x_{t+1} differs in any bit from the plan's knot t+1: the sweep of horizon t+1,
 *      its policy rolled out at step size 0 from x_{t+1}, accepted unconditionally (one rollout, no iteration).
 * tau_max [device]: (Bp) doubles in internal lane order, 0 < tau_max <= +inf, required (+inf: no limit).
 * plant [device]: (Bp) gym_model rows in internal lane order (64 bytes a row, 16-byte aligned; a row's dt is ignored,
 * m supplies dt; padding lanes: any valid row).  A row equal to m reproduces the plan's knots bit for bit.
 * Outputs [device], lane-major, internal lane i in row bt->lane_map[i] (NULL: i): x_cl (B,N,4) rows t0 .. t1 and
 * u_cl (B,T,2) rows t0 .. t1-1, the applied states and controls; per step t0 .. t1-1 step_iters, step_rolls (the
 * re-anchor's rollout included), step_stop (B,T) int32 and step_cost (B,T), the cost-to-go after the replan.
 * step_stop: GYM_ACTIVE (all `iters` ran), GYM_CONVERGED or GYM_LS_FAILED.  Each lane's buffer parity is kept in
 * bt->res_buf between launches, so consecutive step ranges continue one another bit for bit; n_iter and n_roll
 * accumulate the steps' counts.
 * GYM_EINVAL with nothing launched: plant NULL or not 16-byte aligned, a NULL output, t0 < 0, t1 > T, t0 > t1,
 * iters < 0, GYM_FLAG_X_CKPT or GYM_FLAG_SIGMA_STREAM, and any refusal of gym_newton_run_box. */
int gym_newton_mpc_run(const gym_model* m, const gym_weights* w, const gym_armijo* a, const gym_batch* bt,
                       const double* tau_max, const gym_model plant[], int32_t t0, int32_t t1, int32_t iters,
                       double* x_cl, double* u_cl, int32_t* step_iters, int32_t* step_rolls, double* step_cost,
                       int32_t* step_stop, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GYMNAST_NEWTON_MPC_H */
