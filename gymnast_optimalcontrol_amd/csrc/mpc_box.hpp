// Torque-limited MPC on ONE shared reference (gym_mpc_box_qp / gym_mpc_box_rollout): the box-QP active set
// (box_qp_lane and its three passes, which mpc_box_lanes.hpp runs per lane as well), its opt-in projected-Newton
// fallback (box_pn_lane; the ..._fallback entry points), the stage table, the kernel templates and the workspace
// layout.  Part of the tracking_kernels.hip translation unit: included inside its anonymous
// namespace; gym:: and Dyn come from acrobot_device.hpp, which the .hip includes ahead of the namespace.
#pragma once

#include "mpc_gains.hpp"   // M44, chain4, StageLin, disc_stage, kMpcMaxStages, wave_lds_order

// ------------------------------------------------------------------------------------------
// Torque-limited MPC (solver_mpc with test_constraints on, :87-114): every stage of the window obeys
//   -tau_max <= u_t + u_ref_t <= tau_max.
// B_d's column 0 is zero (tau1 unactuated), so channel 0 separates (u_t[0] = clip(0, lo, hi)) and channel 1 is a
// scalar-input LQ problem with a box, b = B_t[:, 1], r = R[1][1].  One lane solves one QP with a primal-dual
// active set over a clamped Riccati sweep (each stage free, at hi or at lo; all free at the start):
//   backward   P = Q_T, p = 0;  free: g = r + b'Pb, k = -(b'PA)/g, d = -(b'p)/g;  clamped: k = 0, d = the bound;
//              Acl = A + b k,  p <- r k'd + Acl'(P b d + p),  P <- Q + r k'k + Acl' P Acl
//   forward    u_t = k_t x_t + d_t,  x_{t+1} = A_t x_t + b u_t
//   costate    lam = 2 Q_T x_{L-1};  q_t = 2 r u_t + b'lam,  lam <- 2 Q x_t + A_t'lam  (the reduced-cost gradient)
//   update     free and u_t > hi -> hi, < lo -> lo;  at hi stays while q_t < 0, at lo while q_t > 0, else free
// until no stage changes (u is then the exact minimiser) or the sweep count reaches max_it (unconverged: clip(u, lo,
// hi) of the last iterate, flagged; so a QP is unconverged exactly when its count is max_it -- a last sweep that
// happens to settle is still flagged, and its clipped iterate is then the minimiser itself).  Iteration 1 has every stage free, so its gains do not depend on the lane: with Kw
// (k_mpc_gains<true>'s table of the window) it is one linear forward pass and no per-lane Riccati sweep.
//
// Shared operands: the window's stage rows and Kw sit in the workgroup's LDS (one wavefront per workgroup), read at
// wave-uniform addresses (broadcast).  Every sweep stage needs ~26 shared doubles; as scalar loads from the global
// table each stage waited a full L2 round trip with nothing to overlap it (one wavefront per CU), 4x the stage's
// arithmetic (tools/mpc_box_probe.py, profiles/mpc_box/).  The closed loop keeps the rows in a ring: the window
// slides by one stage per control step, so a step loads one new row and the window's Kw.  The per-lane sweep data, a
// few KB per lane, lives in a caller-allocated workspace in lane-fastest layout (slot, stage, lane), so a wavefront's
// accesses to one stage coalesce.
// ------------------------------------------------------------------------------------------
constexpr int kBoxRow = 22;   // one stage row: A_d (16), b = B_d[:, 1] (4), u_ref (2)
struct BoxTable {             // global stage table: stage t of window `first` reads row min(first + t, last)
    const double* A;          // A_d (rows, 4, 4)
    const double* Bm;         // B_d (rows, 4, 2)
    const double* ur;         // u_ref (rows, 2)
    int last;
};
struct BoxWin {
    const double* rows;       // LDS: stage t at rows + kBoxRow slot(t)
    const double* Kw;         // LDS: row 1 of the window's unconstrained gains, 4 per stage; or null
    int base, Lm;             // ring: slot(t) = (base + t) mod Lm
    __device__ __forceinline__ const double* row(int t) const {
        const int i = base + t;
        return rows + kBoxRow * (i >= Lm ? i - Lm : i);
    }
};
// element e of global stage row r (clamped to the table's last row) in the LDS row format
__device__ __forceinline__ double box_row_elem(const BoxTable& tb, int r, int e) {
    const int64_t row = min(r, tb.last);
    return e < 16 ? tb.A[16 * row + e] : (e < 20 ? tb.Bm[8 * row + 2 * (e - 16) + 1] : tb.ur[2 * row + (e - 20)]);
}
struct BoxWs {
    double* d;          // slots 0-3 k, 4 d, 5-8 x, 9 u of stage t at ((10 t + slot) Bp + lane); x_{L-1} after them
    int32_t* st;        // stage state (0 free, 1 at hi, -1 at lo) at (t Bp + lane)
    int64_t Bp, lane;
    __device__ __forceinline__ double& at(int t, int slot) const { return d[(10 * (int64_t)t + slot) * Bp + lane]; }
    __device__ __forceinline__ int32_t& state(int t) const { return st[(int64_t)t * Bp + lane]; }
};
constexpr int kBoxSlots = 10;

__device__ __forceinline__ double box_gain_dot(const double* k, double x0, double x1, double x2, double x3) {
#pragma clang fp contract(on)   // the chain of track_feedback(): the same bits as the unconstrained rollout
    return ((k[0] * x0 + k[1] * x1) + k[2] * x2) + k[3] * x3;
}

// the state step x <- A x + b u on stage row A (A_d, then b), by value: as in/out references the passes' kernels change
struct BoxX { double x0, x1, x2, x3; };
__device__ __forceinline__ BoxX box_step(const double* A, double x0, double x1, double x2, double x3, double u) {
    const double x[4] = {x0, x1, x2, x3};
    return {chain4(A, 1, x, 1) + A[16] * u, chain4(A + 4, 1, x, 1) + A[17] * u, chain4(A + 8, 1, x, 1) + A[18] * u,
            chain4(A + 12, 1, x, 1) + A[19] * u};
}

// clamped Riccati sweep of the lane's current stage states -> (k, d) of every stage in the workspace
__device__ __forceinline__ void box_backward(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                             double tau, const BoxWs& ws, bool all_free) {
    double P[16], p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 16; ++q) P[q] = QT[q];
    // the lane's workspace reads of a sweep do not depend on its arithmetic: each is issued one stage ahead, so the
    // stage's own work covers the memory latency (one wavefront per CU: nothing else would)
    int sn = all_free ? 0 : ws.state(Lm - 1);
    for (int t = Lm - 1; t >= 0; --t) {
        const double* A = w.row(t);
        const double b[4] = {A[16], A[17], A[18], A[19]};
        const int s = sn;
        sn = all_free ? 0 : ws.state(t > 0 ? t - 1 : 0);
        double Pb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) Pb[i] = chain4(P + 4 * i, 1, b, 1);
        const double g = r + chain4(Pb, 1, b, 1);
        const double ig = 1.0 / g;
        double k[4], d;
        if (s == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) k[j] = -(chain4(Pb, 1, A + j, 4) * ig);
            d = -(chain4(p, 1, b, 1) * ig);
        } else {
            k[0] = k[1] = k[2] = k[3] = 0.0;
            d = (s > 0 ? tau : -tau) - A[21];
        }
        double Acl[16], v[4], pn[4], M[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) Acl[4 * i + j] = A[4 * i + j] + b[i] * k[j];
            v[i] = Pb[i] * d + p[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pn[i] = (r * k[i]) * d + chain4(Acl + i, 4, v, 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) M[4 * i + j] = chain4(P + 4 * i, 1, Acl + j, 4);
        }
        double Pn[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                Pn[4 * i + j] = (Q.v[4 * i + j] + (r * k[i]) * k[j]) + chain4(Acl + i, 4, M + j, 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = pn[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) P[4 * i + j] = 0.5 * (Pn[4 * i + j] + Pn[4 * j + i]);   // P stays symmetric
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ws.at(t, j) = k[j];
        ws.at(t, 4) = d;
    }
}

// forward pass from e; STORE: x_t, u_t of every stage and x_{L-1} go to the workspace.  shared: the window's
// unconstrained gains (every stage free, d = 0).  Returns whether a free stage's u_t lies outside its bounds.
template <bool STORE>
__device__ __forceinline__ bool box_forward(const BoxWin& w, int Lm, const BoxWs& ws, bool shared, bool all_free,
                                            double tau, double x0, double x1, double x2, double x3, double& u_first) {
    bool viol = false;
    double kn[4] = {0.0, 0.0, 0.0, 0.0}, dn = 0.0;
    int sn = 0;
    if (!shared) {                                       // (k, d, state) one stage ahead, as in box_backward
#pragma unroll
        for (int q = 0; q < 4; ++q) kn[q] = ws.at(0, q);
        dn = ws.at(0, 4);
        sn = all_free ? 0 : ws.state(0);
    }
    for (int t = 0; t < Lm; ++t) {
        const double* A = w.row(t);
        double u;
        if (shared) {
            u = box_gain_dot(w.Kw + 4 * t, x0, x1, x2, x3);
            viol |= (u > tau - A[21]) | (u < -tau - A[21]);
        } else {
            const int s = sn;
            const double k[4] = {kn[0], kn[1], kn[2], kn[3]};
            const double d = dn;
            const int tn = t + 1 < Lm ? t + 1 : t;
#pragma unroll
            for (int q = 0; q < 4; ++q) kn[q] = ws.at(tn, q);
            dn = ws.at(tn, 4);
            sn = all_free ? 0 : ws.state(tn);
            u = s == 0 ? box_gain_dot(k, x0, x1, x2, x3) + d : d;
            viol |= (s == 0) & ((u > tau - A[21]) | (u < -tau - A[21]));
        }
        if (t == 0) u_first = u;
        if constexpr (STORE) {
            ws.at(t, 5) = x0; ws.at(t, 6) = x1; ws.at(t, 7) = x2; ws.at(t, 8) = x3;
            ws.at(t, 9) = u;
        }
        const BoxX n = box_step(A, x0, x1, x2, x3, u);
        x0 = n.x0; x1 = n.x1; x2 = n.x2; x3 = n.x3;
    }
    if constexpr (STORE) { ws.at(Lm, 0) = x0; ws.at(Lm, 1) = x1; ws.at(Lm, 2) = x2; ws.at(Lm, 3) = x3; }
    return viol;
}

// costate pass over the stored (x, u) and the stage-state update; returns whether any stage changed.  PN: the
// fallback's gradient pass (all_free = false): its state rule, the active set of (u, q), and q_t -> slot 5
template <bool PN = false>
__device__ __forceinline__ bool box_update(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                           double tau, const BoxWs& ws, bool all_free) {
    double lam[4];
    {
        const double x[4] = {ws.at(Lm, 0), ws.at(Lm, 1), ws.at(Lm, 2), ws.at(Lm, 3)};
#pragma unroll
        for (int i = 0; i < 4; ++i) lam[i] = 2.0 * chain4(QT + 4 * i, 1, x, 1);
    }
    bool changed = false;
    double un = ws.at(Lm - 1, 9), xn[4] = {ws.at(Lm - 1, 5), ws.at(Lm - 1, 6), ws.at(Lm - 1, 7), ws.at(Lm - 1, 8)};
    int sn = all_free ? 0 : ws.state(Lm - 1);               // (x, u, state) one stage ahead, as in box_backward
    for (int t = Lm - 1; t >= 0; --t) {
        const double* A = w.row(t);
        const double f = A[21];
        const double hi = tau - f, lo = -tau - f;
        const double u = un;
        const double x[4] = {xn[0], xn[1], xn[2], xn[3]};
        const int s = sn;
        const int tn = t > 0 ? t - 1 : 0;
        un = ws.at(tn, 9);
#pragma unroll
        for (int q = 0; q < 4; ++q) xn[q] = ws.at(tn, 5 + q);
        sn = all_free ? 0 : ws.state(tn);
        const double q = 2.0 * r * u + chain4(lam, 1, A + 16, 1);
        const int ns = PN       ? ((u <= lo && q > 0.0) ? -1 : ((u >= hi && q < 0.0) ? 1 : 0))
                       : s == 0 ? (u > hi ? 1 : (u < lo ? -1 : 0))
                                : (s > 0 ? (q < 0.0 ? 1 : 0) : (q > 0.0 ? -1 : 0));
        changed |= ns != s;
        ws.state(t) = ns;
        if constexpr (PN) ws.at(t, 5) = q;                  // x_t is in registers; stage t - 1 is read already
        double nl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) nl[i] = 2.0 * chain4(Q.v + 4 * i, 1, x, 1) + chain4(A + i, 4, lam, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) lam[i] = nl[i];
    }
    return changed;
}

// ------------------------------------------------------------------------------------------
// The fallback (FALLBACK instantiations only): a QP whose active set has not settled after max_it sweeps is continued
// by projected Newton (Bertsekas) from its clipped iterate u, which is feasible.  One iteration:
//   gradient   box_update<true>: the active set's own costate pass over the stored (x, u), one loop for both, with
//              this phase's state rule -- stage t is at lo when u_t <= lo_t and q_t > 0, at hi when u_t >= hi_t and
//              q_t < 0, free otherwise -- and q_t kept; returns whether any state changed
//   target     box_backward on these states, unchanged; ubar_t = k_t x_t + d_t along its own states (box_pn_target:
//              whether a free stage of ubar lies outside its bounds)
//   search     a = 1, 1/2, ... (kBoxPnTrials at most): u(a) = clip(u + a (ubar - u), lo, hi); the first a with
//              J(u(a)) <= J(u) + kBoxPnSigma q'(u(a) - u) is taken, the difference of the two costs coming from one
//              linear rollout (box_pn_trial), and stored with its states (box_pn_store); none: the QP stays
//              unconverged and returns u
//   stop       a = 1 taken, no violation, and the next gradient's active set is the one just used: ubar is
//              stationary on its face with correctly signed multipliers, the active set's own certificate.
// Slots: q lives in slot 5 and ubar in slot 6 from the gradient to the store (x is dead there: the store rolls the
// states out again, and every exit ends with a store), so the layout and the workspace sizes do not change.
// ------------------------------------------------------------------------------------------
constexpr int kBoxPnTrials = 30;
constexpr double kBoxPnSigma = 1e-4;

// forward pass of box_backward's (k, d) along its own states: ubar_t -> slot 6; whether a free ubar_t is out of bounds
__device__ __forceinline__ bool box_pn_target(const BoxWin& w, int Lm, const BoxWs& ws, double tau, double x0,
                                              double x1, double x2, double x3) {
    bool viol = false;
    double kn[4], dn = ws.at(0, 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) kn[q] = ws.at(0, q);
    int sn = ws.state(0);
    for (int t = 0; t < Lm; ++t) {
        const double* A = w.row(t);
        const int s = sn;
        const double k[4] = {kn[0], kn[1], kn[2], kn[3]};
        const double d = dn;
        const int tn = t + 1 < Lm ? t + 1 : t;
#pragma unroll
        for (int q = 0; q < 4; ++q) kn[q] = ws.at(tn, q);
        dn = ws.at(tn, 4);
        sn = ws.state(tn);
        const double u = s == 0 ? box_gain_dot(k, x0, x1, x2, x3) + d : d;
        viol |= (s == 0) & ((u > tau - A[21]) | (u < -tau - A[21]));
        ws.at(t, 6) = u;
        const BoxX n = box_step(A, x0, x1, x2, x3, u);
        x0 = n.x0; x1 = n.x1; x2 = n.x2; x3 = n.x3;
    }
    return viol;
}

// the step of one stage: v = u(a) = clip(u + a (ubar - u), lo, hi); a = 0 or a NaN target moves nothing
__device__ __forceinline__ double box_pn_step(double u, double ub, double a, double lo, double hi) {
    if (a == 0.0) return u;
    const double c = u + a * (ub - u);
    const double v = c > hi ? hi : (c < lo ? lo : c);
    return v == v ? v : u;
}

// One trial of the search: the decrease J(u(a)) - J(u) = slope + quad, with slope = q'D the Armijo slope, D = u(a) - u
// and quad = 1/2 D'H D the cost of the linear rollout of D from a zero state.  J is quadratic, so this is the
// difference itself, without its cancellation: on a diverged closed loop J is 2e9 while the decrease of a last step
// can be 0 exactly (every stage on its bound: nothing moves, and the step must be accepted), which a difference of
// two separately rounded costs cannot resolve.
__device__ __forceinline__ void box_pn_trial(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                             double tau, const BoxWs& ws, double a, double& slope, double& quad) {
    double un = ws.at(0, 9), bn = ws.at(0, 6), qn = ws.at(0, 5);   // (u, ubar, q) one stage ahead
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, cost = 0.0, sl = 0.0;
    for (int t = 0; t < Lm; ++t) {
        const double* A = w.row(t);
        const double f = A[21];
        const double u = un, ub = bn, q = qn;
        const int tn = t + 1 < Lm ? t + 1 : t;
        un = ws.at(tn, 9); bn = ws.at(tn, 6); qn = ws.at(tn, 5);
        const double dl = box_pn_step(u, ub, a, -tau - f, tau - f) - u;
        sl += q * dl;
        const double x[4] = {x0, x1, x2, x3};
        double xq = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) xq += x[i] * chain4(Q.v + 4 * i, 1, x, 1);
        cost += xq + (r * dl) * dl;
        const BoxX n = box_step(A, x0, x1, x2, x3, dl);
        x0 = n.x0; x1 = n.x1; x2 = n.x2; x3 = n.x3;
    }
    const double x[4] = {x0, x1, x2, x3};
    double xq = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) xq += x[i] * chain4(QT + 4 * i, 1, x, 1);
    slope = sl;
    quad = cost + xq;
}

// the step taken: v = u(a) and its states from e -> x_t slots 5-8, v_t slot 9, x_{L-1}.  a = 0: v = u, nothing of
// ubar or q enters the result (the slots may hold anything); this is also how a leaving lane gets its states back.
__device__ __forceinline__ void box_pn_store(const BoxWin& w, int Lm, double tau, const BoxWs& ws, double a, double x0,
                                             double x1, double x2, double x3, double& u_first) {
    double un = ws.at(0, 9), bn = ws.at(0, 6);                     // (u, ubar) one stage ahead
    for (int t = 0; t < Lm; ++t) {
        const double* A = w.row(t);
        const double f = A[21];
        const double u = un, ub = bn;
        const int tn = t + 1 < Lm ? t + 1 : t;
        un = ws.at(tn, 9); bn = ws.at(tn, 6);
        const double v = box_pn_step(u, ub, a, -tau - f, tau - f);
        if (t == 0) u_first = v;
        ws.at(t, 5) = x0; ws.at(t, 6) = x1; ws.at(t, 7) = x2; ws.at(t, 8) = x3;
        ws.at(t, 9) = v;
        const BoxX n = box_step(A, x0, x1, x2, x3, v);
        x0 = n.x0; x1 = n.x1; x2 = n.x2; x3 = n.x3;
    }
    ws.at(Lm, 0) = x0; ws.at(Lm, 1) = x1; ws.at(Lm, 2) = x2; ws.at(Lm, 3) = x3;
}

// The second phase of one lane's QP, from the clipped iterate in slot 9 (feasible; x of slots 5-8 is the unclipped
// iterate's and is not used).  Adds its Newton iterations (one Riccati sweep each) to iters.  The loop runs to a wave
// vote, as box_qp_lane's does; lanes that are done (or did not enter) sit out.  Every exit leaves (x, u) of the
// result in the workspace.
__device__ __forceinline__ void box_pn_lane(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                            double tau, int fb_it, const BoxWs& ws, bool enter, double e0, double e1,
                                            double e2, double e3, double& u_first, int& iters, bool& conv) {
    bool active = enter, full = false;
    double uf;
    if (active) box_pn_store(w, Lm, tau, ws, 0.0, e0, e1, e2, e3, uf);
    for (int n = 0; n <= fb_it; ++n) {
        if (!__any(active)) break;
        if (active) {
            const bool changed = box_update<true>(w, Lm, Q, r, QT, tau, ws, false);
            if (n > 0 && full && !changed) {
                conv = true;
                active = false;
            } else if (n == fb_it) {
                active = false;
            } else {
                iters += 1;
                box_backward(w, Lm, Q, r, QT, tau, ws, false);
                const bool viol = box_pn_target(w, Lm, ws, tau, e0, e1, e2, e3);
                double a = 1.0, slope, quad;
                bool took = false;
                for (int j = 0; j < kBoxPnTrials; ++j) {
                    box_pn_trial(w, Lm, Q, r, QT, tau, ws, a, slope, quad);
                    if (slope + quad <= kBoxPnSigma * slope) { took = true; break; }
                    a *= 0.5;
                }
                if (took) {
                    box_pn_store(w, Lm, tau, ws, a, e0, e1, e2, e3, uf);
                    full = a == 1.0 && !viol;
                } else {
                    active = false;                         // no step found: unconverged, returns u
                }
            }
            // q overwrote slot 5: a lane that leaves here rolls its states out again
            if (!active) box_pn_store(w, Lm, tau, ws, 0.0, e0, e1, e2, e3, u_first);
        }
    }
}

// One lane's QP from e = x0; u_first = u_0 of channel 1.  WS_RESULT: (x_t, u_t) of the result are always left in the
// workspace (the batch kernel's outputs); without it a first iterate (shared gains) that violates no bound -- the
// exact minimiser: no free stage changes state -- ends the QP after a forward pass that stores nothing.
// The loop runs until every lane of the wavefront is done; lanes that are done (or not valid) sit out.
// FALLBACK: a QP that reaches max_it goes on in box_pn_lane for at most fb_it Newton iterations (iters counts both
// phases, so iters > max_it exactly when the fallback ran; conv: either phase finished); without it fb_it is not read.
template <bool WS_RESULT, bool FALLBACK = false>
__device__ __forceinline__ void box_qp_lane(const BoxWin& w, int Lm, const M44& Q, double r, const double* QT,
                                            double tau, int max_it, const BoxWs& ws, bool valid, double e0, double e1,
                                            double e2, double e3, double& u_first, int& iters, bool& conv,
                                            int fb_it = 0) {
    bool active = valid;
    conv = false;
    iters = 0;
    for (int it = 0; it < max_it; ++it) {
        if (!__any(active)) break;
        if (active) {
            const bool all_free = it == 0;
            const bool shared = all_free && w.Kw != nullptr;
            bool changed = true;
            iters = it + 1;
            if (!WS_RESULT && shared && max_it > 1 &&
                !box_forward<false>(w, Lm, ws, true, true, tau, e0, e1, e2, e3, u_first)) {
                changed = false;
            } else {
                if (!shared) box_backward(w, Lm, Q, r, QT, tau, ws, all_free);
                box_forward<true>(w, Lm, ws, shared, all_free, tau, e0, e1, e2, e3, u_first);
                changed = box_update(w, Lm, Q, r, QT, tau, ws, all_free);
            }
            if (!changed && it + 1 < max_it) { conv = true; active = false; }
        }
    }
    if (valid && !conv) {
        for (int t = 0; t < Lm; ++t) {
            const double f = w.row(t)[21];
            const double hi = tau - f, lo = -tau - f;
            const double u = ws.at(t, 9);
            const double c = u > hi ? hi : (u < lo ? lo : u);
            ws.at(t, 9) = c;
            if (t == 0) u_first = c;
        }
    }
    if constexpr (FALLBACK)
        box_pn_lane(w, Lm, Q, r, QT, tau, fb_it, ws, valid && !conv, e0, e1, e2, e3, u_first, iters, conv);
}

// the applied torque u_ref + u_0 of one channel: a first control on its bound is the limit itself (hi + u_ref is
// tau_max only up to rounding), and the sum stays inside the limit (NaN passes through)
__device__ __forceinline__ double box_apply(double f, double u0, double tau) {
    const double hi = tau - f, lo = -tau - f;
    const double v = u0 >= hi ? tau : (u0 <= lo ? -tau : f + u0);
    return v > tau ? tau : (v < -tau ? -tau : v);
}
__device__ __forceinline__ double box_clip0(double f, double tau) {   // channel 0: clip(0, lo, hi)
    const double hi = tau - f, lo = -tau - f;
    return 0.0 > hi ? hi : (0.0 < lo ? lo : 0.0);
}

// Stage table of the closed loop: rows 0..S-1 the reference's discretised linearisations, row S the pad (x_f, u_f),
// dense A_d (4,4), B_d (4,2) with disc_stage()'s operations (k_mpc_gains' own stages), and u_ref with u_f appended.
__global__ __launch_bounds__(64) void k_mpc_box_stages(Dyn m, const double* __restrict__ x_ref,
                                                       const double* __restrict__ u_ref, int S,
                                                       const double* __restrict__ xf, const double* __restrict__ uf,
                                                       double* __restrict__ A, double* __restrict__ Bm,
                                                       double* __restrict__ ur) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    const double* x = s < S ? x_ref + 4 * (int64_t)s : xf;
    const double* u = s < S ? u_ref + 2 * (int64_t)s : uf;
    StageLin q;
    disc_stage(m, x[0], x[1], x[2], x[3], u[1], q);
    double* a = A + 16 * (int64_t)s;
    double* b = Bm + 8 * (int64_t)s;
    a[0] = 1.0; a[1] = 0.0; a[2] = m.h; a[3] = 0.0;
    a[4] = 0.0; a[5] = 1.0; a[6] = 0.0; a[7] = m.h;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[8 + j] = q.a2[j]; a[12 + j] = q.a3[j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = 0.0;
    b[5] = q.b2; b[7] = q.b3;
    ur[2 * (int64_t)s] = u[0]; ur[2 * (int64_t)s + 1] = u[1];
}

constexpr int kBoxMaxLm = kMpcMaxStages - 3;   // L - 1 <= 253 stages per window (L + 2 <= 256)

// The kernels below and k_mpc_box_lane_rollout (mpc_box_lanes.hpp) are kernel templates with two instantiations:
// k<false>, the active set alone, and k<true, int>, whose pack Fb is the one parameter fb_it after max_it, handed to
// box_qp_lane's fallback.  The kernel itself is the template: thin __global__ wrappers around a shared body gave the
// fallback-off kernels other register allocation; instantiations do not (tools/kernel_isa_diff.py).

// A batch of QPs on one window: x0 (B,4) -> U (B,L-1,2), X (B,L,4), iterations and converged flag per QP
template <bool FB, class... Fb>
__global__ __launch_bounds__(64) void k_mpc_box_qp(BoxTable tb, int L, M44 Q, double r,
                                                   const double* __restrict__ QT, double tau, int max_it,
                                                   Fb... fb_it, const double* __restrict__ x0, int64_t B,
                                                   double* wsd, int32_t* wst, int64_t Bp, double* __restrict__ U,
                                                   double* __restrict__ X, int32_t* __restrict__ iters_out,
                                                   int32_t* __restrict__ conv_out) {
    __shared__ double rows[kBoxMaxLm * kBoxRow];
    const int ln = threadIdx.x;
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + ln;
    const bool valid = l < B;
    const int Lm = L - 1;
    for (int idx = ln; idx < Lm * kBoxRow; idx += 64) rows[idx] = box_row_elem(tb, idx / kBoxRow, idx % kBoxRow);
    wave_lds_order();
    const BoxWin w{rows, nullptr, 0, Lm};
    const BoxWs ws{wsd, wst, Bp, l};
    const int64_t lr = valid ? l : 0;
    double u_first;
    int iters;
    bool conv;
    box_qp_lane<true, FB>(w, Lm, Q, r, QT, tau, max_it, ws, valid, x0[4 * lr], x0[4 * lr + 1], x0[4 * lr + 2],
                          x0[4 * lr + 3], u_first, iters, conv, fb_it...);
    if (!valid) return;
    double* Ul = U + 2 * (int64_t)Lm * l;
    double* Xl = X + 4 * (int64_t)L * l;
    for (int t = 0; t < Lm; ++t) {
        Ul[2 * t] = box_clip0(w.row(t)[20], tau);
        Ul[2 * t + 1] = ws.at(t, 9);
#pragma unroll
        for (int q = 0; q < 4; ++q) Xl[4 * t + q] = ws.at(t, 5 + q);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Xl[4 * Lm + q] = ws.at(Lm, q);
    iters_out[l] = iters;
    conv_out[l] = conv ? 1 : 0;
}

// The torque-limited closed loop (solve_mpc_tracking :43-67), one trajectory per lane.  Per control step s: e = x -
// x_ref[s], the window's QP (rows s .. s+L-2 of the stage table, the pad past its end; first iterate from K_all's
// window s), u_real[s] = u_ref[s] + u_0, one RK4 step.  Lane-major x (B,N,4), u (B,N-1,2), qp_iters (B,N-1) and the
// lane's count of unconverged QPs.  The wavefront keeps the window's rows in an LDS ring (one new row per step) and
// loads the window's Kw (row 1 of each gain) at the top of the step.  With the fallback qp_iters counts both phases
// and unconverged only the QPs that neither phase finished.
template <bool FB, class... Fb>
__global__ __launch_bounds__(64) void k_mpc_box_rollout(Dyn m, BoxTable tb, int L, M44 Q, double r,
                                                        const double* __restrict__ QT, double tau, int max_it,
                                                        Fb... fb_it, const double* __restrict__ x0,
                                                        const double* __restrict__ x_ref,
                                                        const double* __restrict__ K_all, int64_t B, int N,
                                                        double* wsd, int32_t* wst, int64_t Bp,
                                                        double* __restrict__ xo, double* __restrict__ uo,
                                                        int32_t* __restrict__ it_out, int32_t* __restrict__ unconv_out) {
    __shared__ double rows[kBoxMaxLm * kBoxRow];
    __shared__ double kw[kBoxMaxLm * 4];
    const int ln = threadIdx.x;
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + ln;
    const bool valid = l < B;
    const int64_t lr = valid ? l : 0;
    const int T = N - 1, Lm = L - 1;
    const BoxWs ws{wsd, wst, Bp, l};
    double2* xl = reinterpret_cast<double2*>(xo + 4 * (int64_t)N * lr);
    double2* ul = reinterpret_cast<double2*>(uo + 2 * (int64_t)T * lr);
    int32_t* il = it_out + (int64_t)T * lr;
    double n0 = x0[4 * lr], n1 = x0[4 * lr + 1], n2 = x0[4 * lr + 2], n3 = x0[4 * lr + 3];
    if (valid) {
        xl[0] = make_double2(n0, n1);
        xl[1] = make_double2(n2, n3);
    }
    const gym::PolyRegs pk = gym::poly_vgprs();
    int unconv = 0;
    BoxWin w{rows, kw, 0, Lm};
    for (int s = 0; s < T; ++s) {
        wave_lds_order();                               // the previous step's LDS reads are done
        if (s == 0) {
            for (int idx = ln; idx < Lm * kBoxRow; idx += 64) rows[idx] = box_row_elem(tb, idx / kBoxRow, idx % kBoxRow);
        } else {                                        // stage s + Lm - 1 replaces stage s - 1 in the ring
            if (ln < kBoxRow) rows[kBoxRow * w.base + ln] = box_row_elem(tb, s + Lm - 1, ln);
            w.base = w.base + 1 == Lm ? 0 : w.base + 1;
        }
        const double* Ks = K_all + 8 * (int64_t)s * Lm;
        for (int idx = ln; idx < 4 * Lm; idx += 64) kw[idx] = Ks[8 * (idx >> 2) + 4 + (idx & 3)];
        wave_lds_order();
        const double* r4 = x_ref + 4 * (int64_t)s;
        const double* f = w.row(0) + 20;                // u_ref[s]
        double u1;
        int iters;
        bool conv;
        box_qp_lane<false, FB>(w, Lm, Q, r, QT, tau, max_it, ws, valid, n0 - r4[0], n1 - r4[1], n2 - r4[2],
                               n3 - r4[3], u1, iters, conv, fb_it...);
        if (valid) {
            const double v0 = box_apply(f[0], box_clip0(f[0], tau), tau), v1 = box_apply(f[1], u1, tau);
            ul[s] = make_double2(v0, v1);
            il[s] = iters;
            unconv += conv ? 0 : 1;
            gym::rk4(m, n0, n1, n2, n3, v1, pk);
            xl[2 * (s + 1)] = make_double2(n0, n1);
            xl[2 * (s + 1) + 1] = make_double2(n2, n3);
        }
    }
    if (valid) unconv_out[l] = unconv;
}

// workspace of B lanes, windows of L stages, a stage table of `rows` rows: table, then per-lane doubles, then states
struct BoxLayout {
    int64_t Bp, off_B, off_ur, off_d, off_st, bytes;
};
inline BoxLayout box_layout(int64_t B, int L, int64_t rows) {
    BoxLayout o;
    o.Bp = (B + 63) / 64 * 64;
    o.off_B = 16 * rows * 8;
    o.off_ur = o.off_B + 8 * rows * 8;
    o.off_d = o.off_ur + 2 * rows * 8;
    o.off_st = o.off_d + ((int64_t)kBoxSlots * (L - 1) + 4) * o.Bp * 8;
    o.bytes = o.off_st + (int64_t)(L - 1) * o.Bp * 4;
    return o;
}
