// Newton solver kernels: the per-lane building blocks (stage cost, rollouts, trial controls, backward sweeps).
// Part of the acrobot_kernels.hip translation unit (included inside its anonymous namespace, in dependency order).
#pragma once

// stage cost exactly as total_cost accumulates it (:244-245): J += dx^T Q dx ; J += du^T R du
__device__ __forceinline__ double xcost(const double* w, double n0, double n1, double n2, double n3,
                                        const double* xr) {
#pragma clang fp contract(on)   // context-independent bits (the cost of k_nt_run2's helper wavefront)
    const double e0 = n0 - xr[0], e1 = n1 - xr[1], e2 = n2 - xr[2], e3 = n3 - xr[3];
    return ((e0 * (w[0] * e0) + e1 * (w[1] * e1)) + e2 * (w[2] * e2)) + e3 * (w[3] * e3);
}
// one stage of total_cost (:244-245) added to the running J, with FMA contraction inside each expression only:
// the same bits in every kernel that accumulates a trial's cost.  U0Z: f0 = +0, so f0 (R0 f0) + f1 (R1 f1) is
// f1 (R1 f1) exactly (both contractions of the general expression round to it)
template <bool U0Z = false>
__device__ __forceinline__ double stage_cost(double J, const double* Q, const double* R, double n0, double n1,
                                            double n2, double n3, const double* xrt, double f0, double f1) {
#pragma clang fp contract(on)
    J += xcost(Q, n0, n1, n2, n3, xrt);
    if (U0Z) {
        const double c1 = f1 * (R[1] * f1);
        J += c1;
    } else {
        J += f0 * (R[0] * f0) + f1 * (R[1] * f1);
    }
    return J;
}

// ------------------------------------------------------------------------------------------
// Reference-form rollouts (forward_closed_loop_update :218-229 + total_cost :231-252;
// simulate_open_loop :74-87) for the API entry points:
//   u_new_t = u_t + K_t (x_new_t - x_t) + gamma sigma_t ;  x_new_{t+1} = RK4(x_new_t, u_new_t)
// FULLK = false: open loop, u_new_t = u_t.  x pairs (N,2,Bp); u, sigma planes (T,2,Bp); K pairs (T,4,Bp).
// ------------------------------------------------------------------------------------------
template <bool FULLK, bool WRITE = true>
__device__ __forceinline__ double rollout_ref(const Dyn& m, const KW& w, const double2* __restrict__ x,
                                              const double* __restrict__ u, const double2* __restrict__ K,
                                              const double* __restrict__ s, const double* __restrict__ xr,
                                              const double* __restrict__ ur, double2* __restrict__ xn,
                                              double* __restrict__ un, double gamma, int64_t l, int64_t Bp, int N,
                                              double n0, double n1, double n2, double n3) {
    const int T = N - 1;
    double J = 0.0;
    if (WRITE) {
        xn[wix(0, 0, 2, l, Bp)] = make_double2(n0, n1);
        xn[wix(0, 1, 2, l, Bp)] = make_double2(n2, n3);
    }
    for (int t = 0; t < T; ++t) {
        double v0 = u[pix(t, 0, 2, l, Bp)], v1 = u[pix(t, 1, 2, l, Bp)];
        if (FULLK) {
            const double2 a = x[wix(t, 0, 2, l, Bp)], b = x[wix(t, 1, 2, l, Bp)];
            const double2 k0 = K[wix(t, 0, 4, l, Bp)], k1 = K[wix(t, 1, 4, l, Bp)];
            const double2 k2 = K[wix(t, 2, 4, l, Bp)], k3 = K[wix(t, 3, 4, l, Bp)];
            const double d0 = n0 - a.x, d1 = n1 - a.y, d2 = n2 - b.x, d3 = n3 - b.y;
            const double kd0 = ((k0.x * d0 + k0.y * d1) + k1.x * d2) + k1.y * d3;
            const double kd1 = ((k2.x * d0 + k2.y * d1) + k3.x * d2) + k3.y * d3;
            v0 = (v0 + kd0) + gamma * s[pix(t, 0, 2, l, Bp)];
            v1 = (v1 + kd1) + gamma * s[pix(t, 1, 2, l, Bp)];
            if (WRITE) {
                un[pix(t, 0, 2, l, Bp)] = v0;
                un[pix(t, 1, 2, l, Bp)] = v1;
            }
        }
        const double* urt = ur + 2 * t;
        const double f0 = v0 - urt[0], f1 = v1 - urt[1];
        J = stage_cost(J, w.Q, w.R, n0, n1, n2, n3, xr + 4 * t, f0, f1);
        gym::rk4(m, n0, n1, n2, n3, v1);
        if (WRITE) {
            xn[wix(t + 1, 0, 2, l, Bp)] = make_double2(n0, n1);
            xn[wix(t + 1, 1, 2, l, Bp)] = make_double2(n2, n3);
        }
    }
    return J + xcost(w.QT, n0, n1, n2, n3, xr + 4 * T);
}

// ------------------------------------------------------------------------------------------
// Solver rollout (Armijo trial / candidate / accepted-candidate re-run), offset form:
//   u_new0 = u0 + gamma sigma0,  sigma0 = -(2R0 (u0 - ur0)) / (2R0)     (bit-identical to the sweep)
//   u_new1 = cg + K1 x_new,  cg = (u1 - K1 x) + gamma0 sigma1  (the sweep's offset)          first trial
//   u_new1 = fma(gamma - gamma0, sigma1, cg + K1 x_new)                          SIG: any other step size
// (at gamma = gamma0 the SIG form returns the first trial's value exactly).
// Streams per stage: K1 (2 pairs) + cg (plane) [+ sigma1 (plane) if SIG] + u0 (plane) in; x_new, u_new out.
// cs: (T, 2, Bp) planes, plane 0 = cg, plane 1 = sigma1.
// ------------------------------------------------------------------------------------------
// Streams of one stage of the offset-form rollout, prefetched into registers one stage ahead.
struct TrialStage {
    double2 k0, k1;      // K row 1 (two pairs)
    double cg, s1;       // offset cg, sigma1 (SIG only)
    double u0;           // tau1 control (0 when U0Z)
};

// The trial's controls of one stage, each with FMA contraction inside its expression only (the same bits in
// every kernel, including k_nt_run2 where the helper wavefront forms u0 and the cost):
//   u0_new = u0 + gamma sigma0,  sigma0 = -(2R0 (u0 - ur0)) / (2R0)  == the sweep's sigma0, bit for bit
//   (U0Z: u0 = ur0 = 0  =>  u0_new = +0 exactly)
__device__ __forceinline__ double trial_u0(double u0, double ur0, double gamma, double G00, double iG00) {
#pragma clang fp contract(on)
    const double s0 = -(G00 * (u0 - ur0)) * iG00;
    return u0 + gamma * s0;
}
//   u1_new = cg + K1 x_new  (the first trial, gamma = gamma0)
__device__ __forceinline__ double trial_u1(double2 k0, double2 k1, double cg, double n0, double n1, double n2,
                                          double n3) {
#pragma clang fp contract(on)
    const double kx = ((k0.x * n0 + k0.y * n1) + k1.x * n2) + k1.y * n3;
    return cg + kx;
}
//   u1_new = fma(gamma - gamma0, sigma1, cg + K1 x_new)  (any other step size)
__device__ __forceinline__ double trial_u1_sig(double2 k0, double2 k1, double cg, double s1, double dg, double n0,
                                              double n1, double n2, double n3) {
#pragma clang fp contract(on)
    const double kx = ((k0.x * n0 + k0.y * n1) + k1.x * n2) + k1.y * n3;
    return __builtin_fma(dg, s1, cg + kx);
}

// Torque limit of the box solver (newton_box.hpp): the trial's tau2 control clipped to [-tau, tau].  A NaN control
// stays NaN (no comparison with it is true; fmin / fmax alone would turn it into a bound); tau = +inf returns v.
__device__ __forceinline__ double box_clip(double v, double tau) {
    const double lo = -tau;
    return v < lo ? lo : (v > tau ? tau : v);
}

// BOX (newton_box.hpp): u1_new clipped to [-tau, tau] before the cost, the store and the RK4 step.
// LW (newton_weights.hpp): the stage cost on w, this thread's own weights (held in VGPRs); without it the stage cost's
// Q, R are kernarg_consts()'s, re-read per stage.
template <bool WRITE, bool U0Z, bool SIG, bool CK = false, int CP = kNT, bool BAND = true, int PD = 1,
          bool BOX = false, bool LW = false>
__device__ __forceinline__ double rollout_cform(const Dyn& m, const KW& w, const double* __restrict__ u,
                                                const double2* __restrict__ K1, const double* __restrict__ cs,
                                                const double* __restrict__ xr, const double* __restrict__ ur,
                                                double2* __restrict__ xn, double* __restrict__ un, double gamma,
                                                double gamma0, int64_t l, int64_t Bp, int N, double n0, double n1,
                                                double n2, double n3, double tau = 0.0) {
    const int T = N - 1;
    const double G00 = w.G00, iG00 = w.iG00;
    // lane byte offsets: 2-row wave-blocked pairs (K1, x), planes (cs, u)
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const double dg = gamma - gamma0;                     // SIG: step size relative to the first trial's
    const char* Kb = reinterpret_cast<const char*>(K1);   // stage stride 2 rows
    const char* Cb = reinterpret_cast<const char*>(cs);   // stage stride 2 planes = 1 row
    const char* Ub = reinterpret_cast<const char*>(u);    // stage stride 2 planes = 1 row
    const char* Xb = reinterpret_cast<const char*>(xn);   // stage stride 2 rows
    const char* Ob = reinterpret_cast<const char*>(un);   // stage stride 1 row
    double J = 0.0;
    if (WRITE) {
        const auto rX = rsrc(Xb);
        bst2(rX, o2, 0, n0, n1);
        bst2(rX, o2, WROW, n2, n3);
    }
    auto fetch = [&](TrialStage& q, int t) {   // stage t's streams into register set q
        const auto rK = rsrc(Kb + (int64_t)t * (2 * (int64_t)row));
        q.k0 = bld2<CP>(rK, o2, 0);
        q.k1 = bld2<CP>(rK, o2, WROW);
        const auto rC = rsrc(Cb + (int64_t)t * row);
        q.cg = bld1<CP>(rC, o1, 0);
        q.s1 = SIG ? bld1<CP>(rC, o1, plane) : 0.0;
        q.u0 = U0Z ? 0.0 : bld1<CP>(rsrc(Ub + (int64_t)t * row), o1, 0);
    };
    const gym::PolyRegs pk = gym::poly_vgprs();   // loop-invariant coefficients held in VGPRs
    // stage t with its streams in q (prefetched earlier)
    auto body = [&](const TrialStage& q, int t) {
        prio_band<BAND ? 1 : PRIO_NONE>(t, T);
        const double* urt = ur + 2 * t;
        const double v0 = U0Z ? 0.0 : trial_u0(q.u0, urt[0], gamma, G00, iG00);   // U0Z: +0 exactly
        const double v1u = SIG ? trial_u1_sig(q.k0, q.k1, q.cg, q.s1, dg, n0, n1, n2, n3)
                               : trial_u1(q.k0, q.k1, q.cg, n0, n1, n2, n3);
        double v1 = v1u;
        if constexpr (BOX) v1 = box_clip(v1u, tau);
        const double f0 = U0Z ? 0.0 : v0 - urt[0], f1 = v1 - urt[1];
        if constexpr (LW) {
            J = stage_cost<U0Z>(J, w.Q, w.R, n0, n1, n2, n3, xr + 4 * t, f0, f1);
        } else {
            const KArgs ka = kernarg_consts();   // cost weights re-read per stage (no SGPR spills)
            J = stage_cost<U0Z>(J, ka.w.Q, ka.w.R, n0, n1, n2, n3, xr + 4 * t, f0, f1);
        }
        if (WRITE) {
            const auto rO = rsrc(Ob + (int64_t)t * row);
            if (!U0Z) bst1(rO, o1, 0, v0);             // U0Z: the u0 planes stay zero
            bst1(rO, o1, plane, v1);
        }
        gym::rk4_fast(m, n0, n1, n2, n3, v1, pk);      // near path without sub-step branches
        if (WRITE && (!CK || (t + 1) % CKI == 0 || t + 1 == T)) {   // CK: checkpoint knots only
            const auto rX = rsrc(Xb + (int64_t)(t + 1) * (2 * (int64_t)row));
            bst2(rX, o2, 0, n0, n1);
            bst2(rX, o2, WROW, n2, n3);
        }
    };
    if constexpr (PD == 1) {
        TrialStage pre;   // software prefetch of stage t+1's streams while stage t computes
        fetch(pre, 0);
        pin(pre.k0); pin(pre.k1); pin(pre.cg); pin(pre.s1); pin(pre.u0);
        prio_start<BAND ? 1 : PRIO_NONE>();
        for (int t = 0; t < T; ++t) {
            const TrialStage q = pre;
            fetch(pre, t + 1 < T ? t + 1 : t);   // unconditional (the last stage's copy unused): no phi, no copies
            body(q, t);
        }
    } else {
        // prefetch distance 2 (few wavefronts per SIMD: two stages of loads in flight behind each stage's compute):
        // three register sets in rotation, unrolled by 3 so that no set is copied (a copy waits for its load)
        static_assert(PD == 2, "prefetch distance 1 or 2");
        auto clampT = [&](int v) { return __builtin_amdgcn_readfirstlane(v < T ? v : T - 1); };
        TrialStage s0, s1, s2;
        fetch(s0, 0);
        fetch(s1, clampT(1));
        prio_start<BAND ? 1 : PRIO_NONE>();
        int t = 0;
        for (; t + 3 <= T; t += 3) {
            fetch(s2, clampT(t + 2));
            body(s0, t);
            fetch(s0, clampT(t + 3));
            body(s1, t + 1);
            fetch(s1, clampT(t + 4));
            body(s2, t + 2);
        }
        if (t < T) body(s0, t);
        if (t + 1 < T) body(s1, t + 1);
    }
    return J + xcost(w.QT, n0, n1, n2, n3, xr + 4 * T);
}

// ------------------------------------------------------------------------------------------
// Fused backward sweep of one lane (compute_costate_trajectory :138-159, build_stage_lists
// :166-181, calculate_K_and_sigma :183-216) exploiting the model structure:
//   A_d = I + dt A_c with A_c rows 0,1 = e3^T, e4^T ; B_d = dt B_c with only column 1 non-zero
//   Q_t = 2Q, R_t = 2R (diagonal), S_t = 0  =>  G = diag(2R0, 2R1 + b^T P b), K_t row 0 = 0.
// P is kept symmetric (10 registers), p and (optionally) the costate lambda in registers.
// ------------------------------------------------------------------------------------------
// Stage t's linearisation (build_stage_lists :166-181 with discretize_linearization :161-164): rows 2, 3 of
// A_d = I + dt A_c (rows 0, 1 are [1 0 dt 0], [0 1 0 dt]), column 1 of B_d = dt B_c, q_t = 2Q dx_t, r_t = 2R du_t.
// A function of x_t, u_t only (not of P), so it can be evaluated apart from the Riccati chain.
// U0Z (GYM_FLAG_U0_ZERO: u0 = ur0 = 0): r0 = 2R0 (u0 - ur0) is +0 (the bits the general expression gives), and the
// Riccati step drops the terms it zeroes (sigma0 = -0, its dJ and max|sigma| contributions): the same bits.
struct Lin {
    double A20, A21, A22, A23, A30, A31, A32, A33, bd2, bd3, q0, q1, q2, q3, r0, r1, dt;
};
template <bool U0Z = false>
__device__ __forceinline__ Lin stage_lin(const Dyn& m, const KW& w, const gym::Jac& J, double2 xa, double2 xb,
                                         double ut0, double ut1, const double* xrt, const double* urt) {
#pragma clang fp contract(on)
    const double dt = m.h;
    Lin L;
    L.A20 = dt * J.a2[0]; L.A21 = dt * J.a2[1]; L.A22 = 1.0 + dt * J.a2[2]; L.A23 = dt * J.a2[3];
    L.A30 = dt * J.a3[0]; L.A31 = dt * J.a3[1]; L.A32 = dt * J.a3[2]; L.A33 = 1.0 + dt * J.a3[3];
    L.bd2 = dt * J.bc2; L.bd3 = dt * J.bc3;
    L.q0 = w.twoQ[0] * (xa.x - xrt[0]); L.q1 = w.twoQ[1] * (xa.y - xrt[1]);
    L.q2 = w.twoQ[2] * (xb.x - xrt[2]); L.q3 = w.twoQ[3] * (xb.y - xrt[3]);
    L.r0 = U0Z ? 0.0 : w.G00 * (ut0 - urt[0]);
    L.r1 = w.twoR1 * (ut1 - urt[1]);
    L.dt = dt;
    return L;
}

// One stage of the box solver's sweep (newton_box.hpp; BOX = true below): the caller sets the step's bounds
// lo = -tau - u1_t, hi = tau - u1_t; step_P decides whether the stage is clamped (the unlimited step
// s1u = -g1 / G11 leaves [lo, hi]; a NaN s1u does not) and hands step_p the bound it stops at and F = row 1 of
// B^T P A_d.  A stage that is not clamped is the stage without BOX, bit for bit.
struct BoxStage {
    double lo, hi;
    bool clamped;
    double s1, F0, F1, F2, F3;
};

template <bool LAMBDA>
struct Sweep {
    double P00, P01, P02, P03, P11, P12, P13, P22, P23, P33, p0, p1, p2, p3;
    double l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    double dJ = 0.0, smax = 0.0;

    // terminal conditions from x_N (P = 2 Q_T, p = 2 Q_T dx_N; lambda_N = p)
    __device__ __forceinline__ Sweep(const KW& w, double2 xa, double2 xb, const double* xrT) {
        P00 = 2.0 * w.QT[0]; P11 = 2.0 * w.QT[1]; P22 = 2.0 * w.QT[2]; P33 = 2.0 * w.QT[3];
        P01 = P02 = P03 = P12 = P13 = P23 = 0.0;
        p0 = P00 * (xa.x - xrT[0]); p1 = P11 * (xa.y - xrT[1]);
        p2 = P22 * (xb.x - xrT[2]); p3 = P33 * (xb.y - xrT[3]);
        if (LAMBDA) { l0 = p0; l1 = p1; l2 = p2; l3 = p3; }
    }

    // stage t (x_t = (xa, xb), u_t = (ut0, ut1)): gain row 1 k[0..3], sigma (s0, s1); updates P, p, dJ, smax
    template <bool U0Z = false>
    __device__ __forceinline__ void step(const Dyn& m, const KW& w, double2 xa, double2 xb, double ut0, double ut1,
                                         const double* xrt, const double* urt, double& k0, double& k1,
                                         double& k2, double& k3, double& s0, double& s1,
                                         const gym::PolyRegs& pk = gym::poly_lits()) {
        step_j<U0Z>(m, w, gym::jacobian(m, xa.x, xa.y, xb.x, xb.y, ut1, pk), xa, xb, ut0, ut1, xrt, urt, k0, k1, k2,
                    k3, s0, s1);
    }
    // the same with the stage's Jacobian already evaluated (it depends on x_t, u_t only, not on P)
    template <bool U0Z = false, bool BOX = false>
    __device__ __forceinline__ void step_j(const Dyn& m, const KW& w, const gym::Jac& J, double2 xa, double2 xb,
                                           double ut0, double ut1, const double* xrt, const double* urt, double& k0,
                                           double& k1, double& k2, double& k3, double& s0, double& s1,
                                           BoxStage* bx = nullptr) {
        step_lin<U0Z, BOX>(w, stage_lin<U0Z>(m, w, J, xa, xb, ut0, ut1, xrt, urt), k0, k1, k2, k3, s0, s1, bx);
    }
    // the Riccati update of stage t from its linearisation (stage_lin: a function of x_t, u_t only): the matrix half
    // (gain row 1, P) and then the vector half (sigma, dJ, p, ||sigma||_inf)
    template <bool U0Z = false, bool BOX = false>
    __device__ __forceinline__ void step_lin(const KW& w, const Lin& L, double& k0, double& k1, double& k2,
                                             double& k3, double& s0, double& s1, BoxStage* bx = nullptr) {
        double G11, iG;
        step_P<BOX>(w, L, k0, k1, k2, k3, G11, iG, bx);
        step_p<U0Z, BOX>(w, L, k0, k1, k2, k3, G11, iG, s0, s1, bx);
    }
    // The matrix half of step_lin: gain row 1 k = -(P b)^T A_d / G11, G11 = 2R1 + b^T P b and its reciprocal, and
    // P <- 2Q + A_d^T P A_d - G11 k k^T.  A function of P and the stage's A_d, b only (not of p), so k_nt_run2
    // runs it alone on its main wavefront and hands k, G11, 1/G11 to another wavefront for the vector half.
    // FMA contraction within each expression only, never across statements: the bits then do not depend on the
    // context the stage is compiled into (the interleaved sweep of backward_solver_lane_ilp, the sigma1 re-runs,
    // the split sweep of k_nt_run2) -- with cross-statement fusion they did
    // BOX: a clamped stage (BoxStage) has k = 0, so that G11 k k^T drops out of P: P <- 2Q + A_d^T P A_d
    template <bool BOX = false>
    __device__ __forceinline__ void step_P(const KW& w, const Lin& L, double& k0, double& k1, double& k2, double& k3,
                                           double& G11, double& iG, BoxStage* bx = nullptr) {
#pragma clang fp contract(on)
        const double dt = L.dt;
        const double A20 = L.A20, A21 = L.A21, A22 = L.A22, A23 = L.A23;
        const double A30 = L.A30, A31 = L.A31, A32 = L.A32, A33 = L.A33;
        const double bd2 = L.bd2, bd3 = L.bd3;
        // Pb = P B_d[:,1]
        const double Pb0 = P02 * bd2 + P03 * bd3, Pb1 = P12 * bd2 + P13 * bd3;
        const double Pb2 = P22 * bd2 + P23 * bd3, Pb3 = P23 * bd2 + P33 * bd3;
        G11 = w.twoR1 + (bd2 * Pb2 + bd3 * Pb3);
        // F row 1 = (P b)^T A_d
        const double F0 = Pb0 + A20 * Pb2 + A30 * Pb3;
        const double F1 = Pb1 + A21 * Pb2 + A31 * Pb3;
        const double F2 = dt * Pb0 + A22 * Pb2 + A32 * Pb3;
        const double F3 = dt * Pb1 + A23 * Pb2 + A33 * Pb3;
        iG = gym::recip(G11);   // G11 = 2 R1 + b^T P b >= 2 R1 > 0: rcp + two Newton steps
        k0 = -F0 * iG; k1 = -F1 * iG; k2 = -F2 * iG; k3 = -F3 * iG;
        if constexpr (BOX) {
            // the unlimited step of this stage: step_p's g1 and sigma1, the same expressions
            const double g1 = L.r1 + (bd2 * p2 + bd3 * p3);
            const double s1u = -g1 * iG;
            bx->clamped = s1u < bx->lo || s1u > bx->hi;
            bx->s1 = s1u < bx->lo ? bx->lo : bx->hi;
            bx->F0 = F0; bx->F1 = F1; bx->F2 = F2; bx->F3 = F3;
            if (bx->clamped) { k0 = 0.0; k1 = 0.0; k2 = 0.0; k3 = 0.0; }
        }
        // W = P A_d
        const double W00 = P00 + P02 * A20 + P03 * A30, W01 = P01 + P02 * A21 + P03 * A31;
        const double W02 = dt * P00 + P02 * A22 + P03 * A32, W03 = dt * P01 + P02 * A23 + P03 * A33;
        const double W10 = P01 + P12 * A20 + P13 * A30, W11 = P11 + P12 * A21 + P13 * A31;
        const double W12 = dt * P01 + P12 * A22 + P13 * A32, W13 = dt * P11 + P12 * A23 + P13 * A33;
        const double W20 = P02 + P22 * A20 + P23 * A30, W21 = P12 + P22 * A21 + P23 * A31;
        const double W22 = dt * P02 + P22 * A22 + P23 * A32, W23 = dt * P12 + P22 * A23 + P23 * A33;
        const double W30 = P03 + P23 * A20 + P33 * A30, W31 = P13 + P23 * A21 + P33 * A31;
        const double W32 = dt * P03 + P23 * A22 + P33 * A32, W33 = dt * P13 + P23 * A23 + P33 * A33;
        // P <- 2Q + A_d^T W - K^T G K   (K^T G K = G11 k k^T)
        const double gk0 = G11 * k0, gk1 = G11 * k1, gk2 = G11 * k2, gk3 = G11 * k3;
        const double nP00 = w.twoQ[0] + (W00 + A20 * W20 + A30 * W30) - gk0 * k0;
        const double nP01 = (W01 + A20 * W21 + A30 * W31) - gk0 * k1;
        const double nP02 = (W02 + A20 * W22 + A30 * W32) - gk0 * k2;
        const double nP03 = (W03 + A20 * W23 + A30 * W33) - gk0 * k3;
        const double nP11 = w.twoQ[1] + (W11 + A21 * W21 + A31 * W31) - gk1 * k1;
        const double nP12 = (W12 + A21 * W22 + A31 * W32) - gk1 * k2;
        const double nP13 = (W13 + A21 * W23 + A31 * W33) - gk1 * k3;
        const double nP22 = w.twoQ[2] + (dt * W02 + A22 * W22 + A32 * W32) - gk2 * k2;
        const double nP23 = (dt * W03 + A22 * W23 + A32 * W33) - gk2 * k3;
        const double nP33 = w.twoQ[3] + (dt * W13 + A23 * W23 + A33 * W33) - gk3 * k3;
        P00 = nP00; P01 = nP01; P02 = nP02; P03 = nP03; P11 = nP11; P12 = nP12; P13 = nP13;
        P22 = nP22; P23 = nP23; P33 = nP33;
    }
    // The vector half of step_lin from the stage's gain row, G11 and 1/G11 (step_P): the costate (LAMBDA), sigma,
    // dJ, p <- q + A_d^T p - K^T G sigma and the running ||sigma||_inf.  Not a function of P.
    // BOX: a clamped stage (BoxStage) takes sigma1 = the bound it stops at and p <- q + A_d^T p + F sigma1
    template <bool U0Z = false, bool BOX = false>
    __device__ __forceinline__ void step_p(const KW& w, const Lin& L, double k0, double k1, double k2, double k3,
                                           double G11, double iG, double& s0, double& s1, const BoxStage* bx = nullptr) {
#pragma clang fp contract(on)
        const double dt = L.dt;
        const double A20 = L.A20, A21 = L.A21, A22 = L.A22, A23 = L.A23;
        const double A30 = L.A30, A31 = L.A31, A32 = L.A32, A33 = L.A33;
        const double bd2 = L.bd2, bd3 = L.bd3;
        const double q0 = L.q0, q1 = L.q1, q2 = L.q2, q3 = L.q3, r0 = L.r0, r1 = L.r1;
        if (LAMBDA) {  // lambda_t = 2Q dx_t + A_d^T lambda_{t+1}
            const double n0 = q0 + (l0 + A20 * l2 + A30 * l3);
            const double n1 = q1 + (l1 + A21 * l2 + A31 * l3);
            const double n2 = q2 + (dt * l0 + A22 * l2 + A32 * l3);
            const double n3 = q3 + (dt * l1 + A23 * l2 + A33 * l3);
            l0 = n0; l1 = n1; l2 = n2; l3 = n3;
        }
        const double g1 = r1 + (bd2 * p2 + bd3 * p3);
        s1 = -g1 * iG;
        if constexpr (BOX) {
            if (bx->clamped) s1 = bx->s1;
        }
        if (U0Z) {   // r0 = +0: sigma0 = -0, and r0 sigma0 + g1 sigma1 = g1 sigma1 exactly
            s0 = -0.0;
            const double d1 = g1 * s1;
            dJ += d1;
        } else {
            s0 = -r0 * w.iG00;
            dJ += r0 * s0 + g1 * s1;
        }
        // p <- q + A_d^T p - K^T G sigma
        const double pp0 = p0, pp1 = p1, pp2 = p2, pp3 = p3;   // BOX: p_{t+1} for the clamped form
        const double gs = G11 * s1;
        const double np0 = q0 + (p0 + A20 * p2 + A30 * p3) - k0 * gs;
        const double np1 = q1 + (p1 + A21 * p2 + A31 * p3) - k1 * gs;
        const double np2 = q2 + (dt * p0 + A22 * p2 + A32 * p3) - k2 * gs;
        const double np3 = q3 + (dt * p1 + A23 * p2 + A33 * p3) - k3 * gs;
        p0 = np0; p1 = np1; p2 = np2; p3 = np3;
        if constexpr (BOX) {
            const double c0 = q0 + (pp0 + A20 * pp2 + A30 * pp3) + bx->F0 * s1;
            const double c1 = q1 + (pp1 + A21 * pp2 + A31 * pp3) + bx->F1 * s1;
            const double c2 = q2 + (dt * pp0 + A22 * pp2 + A32 * pp3) + bx->F2 * s1;
            const double c3 = q3 + (dt * pp1 + A23 * pp2 + A33 * pp3) + bx->F3 * s1;
            if (bx->clamped) { p0 = c0; p1 = c1; p2 = c2; p3 = c3; }
        }
        // U0Z: |sigma0| = 0 never raises smax (>= 0 or NaN)
        smax = U0Z ? gym::nanmax_abs(smax, s1) : gym::nanmax_abs(gym::nanmax_abs(smax, s0), s1);
    }
};

// API form: writes K row 1 (pairs), sigma planes and optionally lambda; register prefetch of stage t-1.
template <bool LAMBDA>
__device__ __forceinline__ void backward_lane(const Dyn& m, const KW& w, const double2* __restrict__ x,
                                              const double* __restrict__ u, const double* __restrict__ xr,
                                              const double* __restrict__ ur, double2* __restrict__ K1,
                                              double* __restrict__ sig, double2* __restrict__ lam, int64_t l,
                                              int64_t Bp, int N, double& dJ_out, double& smax_out) {
    const int T = N - 1;
    Sweep<LAMBDA> S(w, x[wix(T, 0, 2, l, Bp)], x[wix(T, 1, 2, l, Bp)], xr + 4 * T);
    if (LAMBDA) {
        lam[wix(T, 0, 2, l, Bp)] = make_double2(S.l0, S.l1);
        lam[wix(T, 1, 2, l, Bp)] = make_double2(S.l2, S.l3);
    }
    double2 pa = x[wix(T - 1, 0, 2, l, Bp)], pb = x[wix(T - 1, 1, 2, l, Bp)];
    double pu0 = u[pix(T - 1, 0, 2, l, Bp)], pu1 = u[pix(T - 1, 1, 2, l, Bp)];
    for (int t = T - 1; t >= 0; --t) {
        const double2 xa = pa, xb = pb;
        const double ut0 = pu0, ut1 = pu1;
        if (t > 0) {
            pa = x[wix(t - 1, 0, 2, l, Bp)];
            pb = x[wix(t - 1, 1, 2, l, Bp)];
            pu0 = u[pix(t - 1, 0, 2, l, Bp)];
            pu1 = u[pix(t - 1, 1, 2, l, Bp)];
        }
        double k0, k1, k2, k3, s0, s1;
        S.step(m, w, xa, xb, ut0, ut1, xr + 4 * t, ur + 2 * t, k0, k1, k2, k3, s0, s1);
        if (LAMBDA) {
            lam[wix(t, 0, 2, l, Bp)] = make_double2(S.l0, S.l1);
            lam[wix(t, 1, 2, l, Bp)] = make_double2(S.l2, S.l3);
        }
        K1[wix(t, 0, 2, l, Bp)] = make_double2(k0, k1);
        K1[wix(t, 1, 2, l, Bp)] = make_double2(k2, k3);
        sig[pix(t, 0, 2, l, Bp)] = s0;
        sig[pix(t, 1, 2, l, Bp)] = s1;
    }
    dJ_out = S.dJ;
    smax_out = S.smax;
}

// Streams of one sweep stage (x_t pairs, u_t planes), prefetched into registers ahead of the stage.
struct SweepStage {
    double2 xa, xb;
    double u0, u1;
};

// What a solver sweep stores: K row 1 + cg (every iteration), sigma1 only (re-run for the trials 2..20 and
// the final sigma), or all three (gamma sweeps).
enum SweepOut { OUT_SOLVER = 0, OUT_SIGMA = 1, OUT_ALL = 2 };

// stage t's sweep outputs: K row 1 (wave-blocked pairs), cg (plane 0 of cs), sigma1 (plane 1)
// the stage's offset cg = (u1 - K1 x) + gamma0 sigma1 (FMA contraction inside the expression only)
__device__ __forceinline__ double stage_cg(double2 xa, double2 xb, double ut1, double g0, double k0, double k1,
                                           double k2, double k3, double s1) {
#pragma clang fp contract(on)
    const double c1 = ut1 - (((k0 * xa.x + k1 * xa.y) + k2 * xb.x) + k3 * xb.y);
    return __builtin_fma(g0, s1, c1);
}
template <int OUT>
__device__ __forceinline__ void store_stage(const char* Kb, const char* Cb, int t, uint32_t row, uint32_t plane,
                                            uint32_t o2, uint32_t o1, double2 xa, double2 xb, double ut1, double g0,
                                            double k0, double k1, double k2, double k3, double s1) {
    const auto rC = rsrc(Cb + (int64_t)t * row);
    if (OUT != OUT_SIGMA) {
        const auto rK = rsrc(Kb + (int64_t)t * (2 * (int64_t)row));
        bst2(rK, o2, 0, k0, k1);
        bst2(rK, o2, WROW, k2, k3);
        bst1(rC, o1, 0, stage_cg(xa, xb, ut1, g0, k0, k1, k2, k3, s1));
    }
    if (OUT != OUT_SOLVER) bst1(rC, o1, plane, s1);
}

// Solver sweep of one lane: writes K row 1 and cg = (u1 - K1 x) + gamma0 sigma1 (and / or sigma1, OUT),
// prefetching stage t-1's streams while stage t computes.  U0Z: the tau1 channel is identically zero
// (u0 = ur0 = 0, GYM_FLAG_U0_ZERO) and its plane is not read.
template <bool U0Z, int OUT, bool BAND = true, int PD = 1>
__device__ __forceinline__ void backward_solver_lane(const Dyn& m, const KW& w,
                                                     const double2* __restrict__ x, const double* __restrict__ u,
                                                     const double* __restrict__ xr, const double* __restrict__ ur,
                                                     double2* __restrict__ K1, double* __restrict__ cs, double g0,
                                                     int64_t l, int64_t Bp, int N, double& dJ_out, double& smax_out) {
    const int T = N - 1;
    // lane byte offsets: 2-row wave-blocked pairs (x, K1), planes (cs, u)
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Xb = reinterpret_cast<const char*>(x);    // stage stride 2 rows
    const char* Ub = reinterpret_cast<const char*>(u);    // stage stride 1 row
    const char* Kb = reinterpret_cast<const char*>(K1);
    const char* Cb = reinterpret_cast<const char*>(cs);
    Sweep<false> S(w, x[wix(T, 0, 2, l, Bp)], x[wix(T, 1, 2, l, Bp)], xr + 4 * T);
    const gym::PolyRegs pk = gym::poly_vgprs();
    if constexpr (PD == 2) {
        // prefetch distance 2: three stream sets in rotation, unrolled by 3 (see rollout_cform)
        auto fetch = [&](SweepStage& q, int t) {
            const int tp = __builtin_amdgcn_readfirstlane(t > 0 ? t : 0);
            const auto rX = rsrc(Xb + (int64_t)tp * (2 * (int64_t)row));
            const auto rU = rsrc(Ub + (int64_t)tp * row);
            q.xa = bld2(rX, o2, 0);
            q.xb = bld2(rX, o2, WROW);
            q.u0 = U0Z ? 0.0 : bld1(rU, o1, 0);
            q.u1 = bld1(rU, o1, plane);
        };
        auto body = [&](const SweepStage& q, int t) {
            prio_band<BAND ? 0 : PRIO_NONE>(T - 1 - t, T);
            double k0, k1, k2, k3, s0, s1;
            const KArgs ka = kernarg_consts();
            S.template step<U0Z>(ka.m, ka.w, q.xa, q.xb, q.u0, q.u1, xr + 4 * t, ur + 2 * t, k0, k1, k2, k3, s0, s1,
                                 pk);
            store_stage<OUT>(Kb, Cb, t, row, plane, o2, o1, q.xa, q.xb, q.u1, g0, k0, k1, k2, k3, s1);
        };
        SweepStage s0, s1, s2;
        fetch(s0, T - 1);
        fetch(s1, T - 2);
        prio_start<BAND ? 0 : PRIO_NONE>();
        int t = T - 1;
        for (; t >= 2; t -= 3) {
            fetch(s2, t - 2);
            body(s0, t);
            fetch(s0, t - 3);
            body(s1, t - 1);
            fetch(s1, t - 4);
            body(s2, t - 2);
        }
        if (t >= 0) body(s0, t);
        if (t >= 1) body(s1, t - 1);
        dJ_out = S.dJ;
        smax_out = S.smax;
        return;
    }
    double2 pa, pb;
    double pu0 = 0.0, pu1;
    {
        const auto rX = rsrc(Xb + (int64_t)(T - 1) * (2 * (int64_t)row)), rU = rsrc(Ub + (int64_t)(T - 1) * row);
        pa = bld2(rX, o2, 0); pb = bld2(rX, o2, WROW); pu1 = bld1(rU, o1, plane);
        if (!U0Z) pu0 = bld1(rU, o1, 0);
    }
    pin(pa); pin(pb); pin(pu0); pin(pu1);
    prio_start<BAND ? 0 : PRIO_NONE>();
    for (int t = T - 1; t >= 0; --t) {
        prio_band<BAND ? 0 : PRIO_NONE>(T - 1 - t, T);
        const double2 xa = pa, xb = pb;
        const double ut0 = pu0, ut1 = pu1;
        {   // unconditional (at t = 0 stage 0 again, unused): no phi, no copies of the prefetch registers
            const int tp = __builtin_amdgcn_readfirstlane(t > 0 ? t - 1 : 0);   // wave-uniform
            const auto rX = rsrc(Xb + (int64_t)tp * (2 * (int64_t)row));
            const auto rU = rsrc(Ub + (int64_t)tp * row);
            pa = bld2(rX, o2, 0);
            pb = bld2(rX, o2, WROW);
            if (!U0Z) pu0 = bld1(rU, o1, 0);
            pu1 = bld1(rU, o1, plane);
        }
        double k0, k1, k2, k3, s0, s1;
        const KArgs ka = kernarg_consts();   // the kernel's (Dyn, KW) arguments, re-read: no SGPR spills
        S.step<U0Z>(ka.m, ka.w, xa, xb, ut0, ut1, xr + 4 * t, ur + 2 * t, k0, k1, k2, k3, s0, s1, pk);
        store_stage<OUT>(Kb, Cb, t, row, plane, o2, o1, xa, xb, ut1, g0, k0, k1, k2, k3, s1);
    }
    dJ_out = S.dJ;
    smax_out = S.smax;
}

// The solver sweep for ONE wavefront per SIMD (the persistent kernel at its batch sizes), where a stage's time is
// its dependency chain, not the SIMD's issue rate: stage t-1's Jacobian (a function of x_{t-1}, u_{t-1} only) is
// evaluated beside stage t's Riccati update, so the two chains interleave.  That needs stage t-1's streams in
// registers one stage early: prefetch distance 2, three stream sets and two Jacobians in rotation (unrolled by
// 6, so that no set is copied -- a copy of a loading register waits for its load).  Same per-stage arithmetic
// as backward_solver_lane (step = jacobian + step_j): the same bits.
// BOX (newton_box.hpp): the sweep of the box solver with the lane's torque limit tau, |u1_t| <= tau on every stage.
// LM (newton_models.hpp): the stage Jacobians on m, this thread's own model (its nine coefficients in VGPRs); without
// it m is not read and every constant is kernarg_consts()'s.  dt is kernarg_consts()'s either way.
// LW (newton_weights.hpp): the stages' weights are w, this thread's own (held in VGPRs); without it w gives the terminal
// conditions only and the stages re-read kernarg_consts()'s.
template <bool U0Z, int OUT, bool BOX = false, bool LM = false, bool LW = false>
__device__ __forceinline__ void backward_solver_lane_ilp(const Dyn& m, const KW& w,
                                                         const double2* __restrict__ x, const double* __restrict__ u,
                                                         const double* __restrict__ xr, const double* __restrict__ ur,
                                                         double2* __restrict__ K1, double* __restrict__ cs, double g0,
                                                         int64_t l, int64_t Bp, int N, double& dJ_out,
                                                         double& smax_out, double tau = 0.0) {
    const int T = N - 1;
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Xb = reinterpret_cast<const char*>(x);
    const char* Ub = reinterpret_cast<const char*>(u);
    const char* Kb = reinterpret_cast<const char*>(K1);
    const char* Cb = reinterpret_cast<const char*>(cs);
    Sweep<false> S(w, x[wix(T, 0, 2, l, Bp)], x[wix(T, 1, 2, l, Bp)], xr + 4 * T);
    const gym::PolyRegs pk = gym::poly_vgprs();
    auto fetch = [&](SweepStage& q, int t) {
        const auto rX = rsrc(Xb + (int64_t)t * (2 * (int64_t)row)), rU = rsrc(Ub + (int64_t)t * row);
        q.xa = bld2(rX, o2, 0);
        q.xb = bld2(rX, o2, WROW);
        q.u0 = U0Z ? 0.0 : bld1(rU, o1, 0);
        q.u1 = bld1(rU, o1, plane);
    };
    auto jac = [&](const SweepStage& q) {
        if constexpr (LM) {
            return gym::jacobian(m, q.xa.x, q.xa.y, q.xb.x, q.xb.y, q.u1, pk);
        } else {
            const KArgs ka = kernarg_consts();
            return gym::jacobian(ka.m, q.xa.x, q.xa.y, q.xb.x, q.xb.y, q.u1, pk);
        }
    };
    // stage t: c = its streams, Jc = its Jacobian; n = stage t-1's streams (landed), f <- stage t-2's
    auto stage = [&](const SweepStage& c, const SweepStage& n, SweepStage& f, const gym::Jac& Jc, gym::Jac& Jn,
                     int t) {
        if (t < 0) return;
        if (t >= 2) fetch(f, t - 2);
        if (t >= 1) Jn = jac(n);
        double k0, k1, k2, k3, s0, s1;
        const KArgs ka = kernarg_consts();
        const KW& sw = LW ? w : ka.w;
        if constexpr (BOX) {
            BoxStage bx;
            bx.lo = -tau - c.u1;
            bx.hi = tau - c.u1;
            S.step_j<U0Z, true>(ka.m, sw, Jc, c.xa, c.xb, c.u0, c.u1, xr + 4 * t, ur + 2 * t, k0, k1, k2, k3, s0, s1,
                                &bx);
        } else {
            S.step_j<U0Z>(ka.m, sw, Jc, c.xa, c.xb, c.u0, c.u1, xr + 4 * t, ur + 2 * t, k0, k1, k2, k3, s0, s1);
        }
        store_stage<OUT>(Kb, Cb, t, row, plane, o2, o1, c.xa, c.xb, c.u1, g0, k0, k1, k2, k3, s1);
    };
    SweepStage A, B, C;
    gym::Jac J0, J1;
    fetch(A, T - 1);
    if (T >= 2) fetch(B, T - 2);
    J0 = jac(A);
    for (int t = T - 1; t >= 0; t -= 6) {
        stage(A, B, C, J0, J1, t);
        stage(B, C, A, J1, J0, t - 1);
        stage(C, A, B, J0, J1, t - 2);
        stage(A, B, C, J1, J0, t - 3);
        stage(B, C, A, J0, J1, t - 4);
        stage(C, A, B, J1, J0, t - 5);
    }
    dJ_out = S.dJ;
    smax_out = S.smax;
}

// Checkpointed solver sweep (GYM_FLAG_X_CKPT): the trial stored x only at the knots c0 = 0, CKI, 2 CKI, ...
// and T.  Going backward one block [c0, c0 + len) at a time, the sweep takes the block's checkpoint x_c0
// and controls, re-integrates x_{c0+1} .. x_{c0+len-1} with the trial's RK4 (same inputs, same code: the
// same bits) into a lane-private LDS slot, then runs the block's stages t = c0+len-1 .. c0 from it.  The
// earlier block's streams are requested after the re-integration, so they land while the block's
// Riccati stages compute and the prefetch registers are not live across the RK4 (128-VGPR budget).
// lds: this wavefront's CKI x 2 rows of 64 double2 (knot c0 + j in rows 2j, 2j+1), then CKI rows of 64
// tau2 controls and (unless U0Z) CKI rows of tau1 controls.
struct CkBlock {
    double2 a, b;          // checkpoint x_c0
    double u0[CKI], u1[CKI];
};

template <bool U0Z, int OUT>
__device__ __forceinline__ void backward_solver_lane_ck(const Dyn& m, const KW& w,
                                                        const double2* __restrict__ x, const double* __restrict__ u,
                                                        const double* __restrict__ xr, const double* __restrict__ ur,
                                                        double2* __restrict__ K1, double* __restrict__ cs, double g0,
                                                        double2* __restrict__ lds, int64_t l, int64_t Bp, int N,
                                                        double& dJ_out, double& smax_out) {
    const int T = N - 1;
    const uint32_t o2 = wbo(l, 2), o1 = (uint32_t)l * 8u;
    const uint32_t row = (uint32_t)Bp * 16u, plane = (uint32_t)Bp * 8u;
    const char* Xb = reinterpret_cast<const char*>(x);
    const char* Ub = reinterpret_cast<const char*>(u);
    const char* Kb = reinterpret_cast<const char*>(K1);
    const char* Cb = reinterpret_cast<const char*>(cs);
    const int ln = threadIdx.x;
    double* lu1 = reinterpret_cast<double*>(lds + 2 * CKI * BLK);   // (CKI, 64) tau2 controls
    double* lu0 = lu1 + CKI * BLK;                                   // (CKI, 64) tau1 controls (!U0Z)
    Sweep<false> S(w, x[wix(T, 0, 2, l, Bp)], x[wix(T, 1, 2, l, Bp)], xr + 4 * T);
    auto fetch = [&](CkBlock& q, int c0, int len) {
        const auto rX = rsrc(Xb + (int64_t)c0 * (2 * (int64_t)row));
        q.a = bld2(rX, o2, 0);
        q.b = bld2(rX, o2, WROW);
#pragma unroll
        for (int j = 0; j < CKI; ++j) {
            q.u0[j] = 0.0;
            q.u1[j] = 0.0;
            if (j < len) {
                const auto rU = rsrc(Ub + (int64_t)(c0 + j) * row);
                if (!U0Z) q.u0[j] = bld1(rU, o1, 0);
                q.u1[j] = bld1(rU, o1, plane);
            }
        }
    };
    const int nblk = (T + CKI - 1) / CKI;
    CkBlock q;
    {
        const int c0 = (nblk - 1) * CKI;
        fetch(q, c0, T - c0);
    }
    prio_start<0>();
    for (int bk = nblk - 1; bk >= 0; --bk) {
        const int c0 = bk * CKI;
        const int len = (T - c0 < CKI) ? T - c0 : CKI;
        prio_band<0>(T - c0 - len, T);
        // knots c0 .. c0+len-1 into LDS: the checkpoint, then the trial's x_{t+1} = RK4(x_t, u1_t); the
        // block's controls too, so that no register holds them across the stages
        {
            double n0 = q.a.x, n1 = q.a.y, n2 = q.b.x, n3 = q.b.y;
            lds[ln] = q.a;
            lds[BLK + ln] = q.b;
#pragma unroll
            for (int j = 0; j < CKI; ++j) {
                lu1[j * BLK + ln] = q.u1[j];
                if (!U0Z) lu0[j * BLK + ln] = q.u0[j];
            }
#pragma unroll
            for (int j = 0; j < CKI - 1; ++j) {
                if (j < len - 1) {
                    gym::rk4(m, n0, n1, n2, n3, q.u1[j]);
                    lds[(2 * j + 2) * BLK + ln] = make_double2(n0, n1);
                    lds[(2 * j + 3) * BLK + ln] = make_double2(n2, n3);
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the unrolled steps apart (register pressure)
            }
        }
        if (bk > 0) fetch(q, c0 - CKI, CKI);   // the earlier block (always full) lands during the stages below
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = CKI - 1; j >= 0; --j) {
            if (j < len) {
                const int t = c0 + j;
                const double2 xa = lds[(2 * j) * BLK + ln], xb = lds[(2 * j + 1) * BLK + ln];
                const double ut1 = lu1[j * BLK + ln], ut0 = U0Z ? 0.0 : lu0[j * BLK + ln];
                double k0, k1, k2, k3, s0, s1;
                const KArgs ka = kernarg_consts();
                S.step<U0Z>(ka.m, ka.w, xa, xb, ut0, ut1, xr + 4 * t, ur + 2 * t, k0, k1, k2, k3, s0, s1);
                store_stage<OUT>(Kb, Cb, t, row, plane, o2, o1, xa, xb, ut1, g0, k0, k1, k2, k3, s1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    dJ_out = S.dJ;
    smax_out = S.smax;
}

// Open-loop rollout of the control planes u with its cost, as an Armijo trial forms them (rollout_cform): per stage
// the cost of (x_t, u_t) through stage_cost<U0Z>, then x_{t+1} = rk4_fast(x_t, tau2_t), the terminal cost last.  The
// trial's controls are the values it stored, so the rollout of a control sequence a trial produced returns that
// trial's states and cost bit for bit (gym_newton_init_warm).  Every knot of xn is stored (valid with
// GYM_FLAG_X_CKPT, as k_init's).
template <bool U0Z>
__device__ __forceinline__ double rollout_warm(const Dyn& m, const KW& w, const double* __restrict__ u,
                                               const double* __restrict__ xr, const double* __restrict__ ur,
                                               double2* __restrict__ xn, int64_t l, int64_t Bp, int N, double n0,
                                               double n1, double n2, double n3) {
    const int T = N - 1;
    const gym::PolyRegs pk = gym::poly_vgprs();
    double J = 0.0;
    xn[wix(0, 0, 2, l, Bp)] = make_double2(n0, n1);
    xn[wix(0, 1, 2, l, Bp)] = make_double2(n2, n3);
    for (int t = 0; t < T; ++t) {
        const double* urt = ur + 2 * t;
        const double v1 = u[pix(t, 1, 2, l, Bp)];
        const double f0 = U0Z ? 0.0 : u[pix(t, 0, 2, l, Bp)] - urt[0], f1 = v1 - urt[1];
        J = stage_cost<U0Z>(J, w.Q, w.R, n0, n1, n2, n3, xr + 4 * t, f0, f1);
        gym::rk4_fast(m, n0, n1, n2, n3, v1, pk);
        xn[wix(t + 1, 0, 2, l, Bp)] = make_double2(n0, n1);
        xn[wix(t + 1, 1, 2, l, Bp)] = make_double2(n2, n3);
    }
    return J + xcost(w.QT, n0, n1, n2, n3, xr + 4 * T);
}
