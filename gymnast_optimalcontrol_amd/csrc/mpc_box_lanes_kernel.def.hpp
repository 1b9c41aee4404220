// The kernel of mpc_box_lanes.hpp, which includes this text twice with mpc_box_kernels.def.hpp's four macros: pass 1
// defines k_mpc_box_lane_rollout (the active set alone, the machine code it was), pass 2 k_mpc_box_lane_rollout_fb,
// which takes fb_it after max_it and hands it to box_qp_lane's projected-Newton fallback (qp_iters then counts both
// phases, unconverged only the QPs that neither phase finished).  No include guard.

// x0 (B,P,4); lane-major x_opt (B,N,4), u_opt (B,N-1,2).  Outputs lane-major: xo (B,P,N,4), uo (B,P,N-1,2) (both or
// neither), summary (3,B,P) = err_final, err_max, u_max as k_lqr_lane_rollout, it_out (B,P,N-1) or null, unconv_out
// (B,P).  grid B nblk (nblk = ceil(P / 64)), 64 threads; LDS dynamic: (kBoxRow + 4) (L - 1) doubles.
__global__ __launch_bounds__(64) void GYM_BOX_K(k_mpc_box_lane_rollout)(Dyn m, M44 Q, double r,
                                                                        const double* __restrict__ QT, double tau,
                                                                        int max_it, GYM_BOX_FB_PARAM
                                                                        const double2* __restrict__ x_opt,
                                                                        const double2* __restrict__ u_opt,
                                                                        const double* __restrict__ x0, int P, int N,
                                                                        int L, int nblk, double* wsd, int32_t* wst,
                                                                        double* __restrict__ xo, double* __restrict__ uo,
                                                                        double* __restrict__ summary,
                                                                        int32_t* __restrict__ it_out,
                                                                        int32_t* __restrict__ unconv_out) {
    extern __shared__ double bl_lds[];
    const int T = N - 1, Lm = L - 1;
    double* rows = bl_lds;
    double* kw = bl_lds + kBoxRow * Lm;
    const int ln = threadIdx.x;
    const int64_t b = blockIdx.x / nblk;
    const int p = (int)(blockIdx.x % nblk) * 64 + ln;
    const bool valid = p < P;
    const int64_t row = b * P + (valid ? p : 0);
    const int64_t BP = (int64_t)gridDim.x / nblk * P;
    const double2* xlo = x_opt + 2 * (b * N);
    const double2* ulo = u_opt + b * T;
    const BoxWs ws{wsd + b * ((int64_t)kBoxSlots * Lm + 4) * P, wst + b * Lm * P, P, p};
    double2* xl = reinterpret_cast<double2*>(xo) + 2 * (int64_t)N * row;
    double2* ul = reinterpret_cast<double2*>(uo) + (int64_t)T * row;
    double n0 = x0[4 * row], n1 = x0[4 * row + 1], n2 = x0[4 * row + 2], n3 = x0[4 * row + 3];
    if (valid && xo) {
        xl[0] = make_double2(n0, n1);
        xl[1] = make_double2(n2, n3);
    }
    const Sym4 Qs = sym4(Q.v), QTs = sym4(QT);
    const gym::PolyRegs pk = gym::poly_vgprs();
    int unconv = 0;
    double emax = 0.0, umax = 0.0;
    BoxWin w{rows, kw, 0, Lm};
    for (int s = 0; s < T; ++s) {
        wave_lds_order();                               // the previous step's LDS reads are done
        if (s == 0) {
            for (int st = ln; st < Lm; st += 64) box_lane_row(m, xlo, ulo, st, T, true, rows + kBoxRow * st);
        } else {                                        // stage s + Lm - 1 replaces stage s - 1 in the ring
            box_lane_row(m, xlo, ulo, s + Lm - 1, T, ln == 0, rows + kBoxRow * w.base);
            w.base = w.base + 1 == Lm ? 0 : w.base + 1;
        }
        wave_lds_order();
        {                                               // Kw: the window's unconstrained gains (k_mpc_lane_gains' maps)
            Sym4 Pm = QTs;
            for (int t = Lm - 1; t >= 0; --t) {
                const double* A = w.row(t);
                double cur[ML_ROWS], k[4];
#pragma unroll
                for (int c = 0; c < 8; ++c) cur[c] = A[8 + c];
                cur[8] = A[18];
                cur[9] = A[19];
                lqr_lane_step(cur, cur + 4, cur[8], cur[9], m.h, r, Qs, Pm, k);
                if (ln == 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) kw[4 * t + j] = k[j];
                }
            }
        }
        wave_lds_order();
        const double2 ra = xlo[2 * s], rb = xlo[2 * s + 1];
        const double d0 = n0 - ra.x, d1 = n1 - ra.y, d2 = n2 - rb.x, d3 = n3 - rb.y;
        const double* f = w.row(0) + 20;                // u_opt[s]
        double u1;
        int iters;
        bool conv;
        box_qp_lane<false, GYM_BOX_FB>(w, Lm, Q, r, QT, tau, max_it, ws, valid, d0, d1, d2, d3, u1, iters, conv
                                       GYM_BOX_FB_ARG);
        if (valid) {
            const double v0 = box_apply(f[0], box_clip0(f[0], tau), tau), v1 = box_apply(f[1], u1, tau);
            emax = gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(emax, d0), d1), d2), d3);
            umax = gym::nanmax_abs(umax, v1);
            unconv += conv ? 0 : 1;
            gym::rk4(m, n0, n1, n2, n3, v1, pk);
            if (it_out) it_out[(int64_t)T * row + s] = iters;
            if (xo) {
                ul[s] = make_double2(v0, v1);
                xl[2 * (s + 1)] = make_double2(n0, n1);
                xl[2 * (s + 1) + 1] = make_double2(n2, n3);
            }
        }
    }
    if (!valid) return;
    const double2 ra = xlo[2 * T], rb = xlo[2 * T + 1];
    const double d0 = n0 - ra.x, d1 = n1 - ra.y, d2 = n2 - rb.x, d3 = n3 - rb.y;
    const double efin = gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(gym::nanmax_abs(0.0, d0), d1), d2), d3);
    emax = gym::nanmax_abs(emax, efin);
    summary[row] = efin;
    summary[BP + row] = emax;
    summary[2 * BP + row] = umax;
    unconv_out[row] = unconv;
}
