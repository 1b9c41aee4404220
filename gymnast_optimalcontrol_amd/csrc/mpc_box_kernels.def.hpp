// The two kernels of mpc_box.hpp, which includes this text twice and sets four macros for each pass (no conditional
// here: both passes are in the one shipped build).  Pass 1 defines k_mpc_box_qp and k_mpc_box_rollout, the active set
// alone; pass 2 k_mpc_box_qp_fb and k_mpc_box_rollout_fb, which take fb_it after max_it and hand it to box_qp_lane's
// projected-Newton fallback:
//   GYM_BOX_K(name)   name            | name##_fb          the kernel's name
//   GYM_BOX_FB        false           | true               box_qp_lane's FALLBACK
//   GYM_BOX_FB_PARAM  (empty)         | int fb_it,         the kernel parameter after max_it
//   GYM_BOX_FB_ARG    (empty)         | , fb_it            box_qp_lane's last argument
// One text, so the two pairs cannot drift apart; kernels and not wrappers of a shared body, so the fallback-off pair
// stays the machine code it was (tools/kernel_isa_diff.py).  With AMD clang 22.0.0git (ROCm 7.2.0, -O3, gfx950) thin
// __global__ wrappers around a __forceinline__ template body, with or without __restrict__ on its parameters, gave
// the three old kernels other register allocation and SGPR spill counts (k_mpc_box_qp: 14 -> 19): worth trying
// again with a later compiler.  No include guard.

// A batch of QPs on one window: x0 (B,4) -> U (B,L-1,2), X (B,L,4), iterations and converged flag per QP
__global__ __launch_bounds__(64) void GYM_BOX_K(k_mpc_box_qp)(BoxTable tb, int L, M44 Q, double r,
                                                              const double* __restrict__ QT, double tau, int max_it,
                                                              GYM_BOX_FB_PARAM const double* __restrict__ x0, int64_t B,
                                                              double* wsd, int32_t* wst, int64_t Bp,
                                                              double* __restrict__ U, double* __restrict__ X,
                                                              int32_t* __restrict__ iters_out,
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
    box_qp_lane<true, GYM_BOX_FB>(w, Lm, Q, r, QT, tau, max_it, ws, valid, x0[4 * lr], x0[4 * lr + 1], x0[4 * lr + 2],
                                  x0[4 * lr + 3], u_first, iters, conv GYM_BOX_FB_ARG);
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
__global__ __launch_bounds__(64) void GYM_BOX_K(k_mpc_box_rollout)(Dyn m, BoxTable tb, int L, M44 Q, double r,
                                                                   const double* __restrict__ QT, double tau,
                                                                   int max_it, GYM_BOX_FB_PARAM
                                                                   const double* __restrict__ x0,
                                                                   const double* __restrict__ x_ref,
                                                                   const double* __restrict__ K_all, int64_t B, int N,
                                                                   double* wsd, int32_t* wst, int64_t Bp,
                                                                   double* __restrict__ xo, double* __restrict__ uo,
                                                                   int32_t* __restrict__ it_out,
                                                                   int32_t* __restrict__ unconv_out) {
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
        box_qp_lane<false, GYM_BOX_FB>(w, Lm, Q, r, QT, tau, max_it, ws, valid, n0 - r4[0], n1 - r4[1], n2 - r4[2],
                                       n3 - r4[3], u1, iters, conv GYM_BOX_FB_ARG);
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
