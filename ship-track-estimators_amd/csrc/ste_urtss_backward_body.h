// ste_urtss_backward_body.h -- the body of the stand-alone smoother kernels (ste_kernels.hip: urtss_backward_l1 and its
// per-track-noise twin urtss_backward_tn), included once into each.  It is text, not a function, on purpose: both kernels
// must run the same arithmetic source (their results are compared bit for bit), and urtss_backward_l1 must compile to
// exactly the code it had as a plain kernel -- moved into an inline function its body is optimised before it meets the
// kernel's arguments and comes out differently.  No include guard.
//   in scope: `const KParams p`; STE_BWD_Q(r, c) = entry (r, c) of the process noise of track t (t is defined below, so
//   the macro may name it).
    const size_t B = (size_t)p.ld;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const int ns = p.nsteps ? p.nsteps[t] : p.Nmax;
    const double* srp = p.sog_rate_rts ? p.sog_rate_rts : p.sog_rate;
    const double* crp = p.cog_rate_rts ? p.cog_rate_rts : p.cog_rate;

    // row ns: smoothed = filtered
    double xs[4], Ps[4][4];
    load_vec(p.fwd_mean, (size_t)ns, B, t, xs);
    const bool packed = (p.flags & STE_FLAG_PACKED_COV) != 0;
    load_cov_m(p.fwd_cov, packed, (size_t)ns, B, t, Ps);
    store_vec(p.sm_mean, (size_t)ns, B, t, xs);
    store_cov_m(p.sm_cov, packed, (size_t)ns, B, t, Ps);
    store_pos(p, (size_t)ns, B, t, xs);

    // filtered row of the first step to process, prefetched
    double xn[4] = {0, 0, 0, 0}, Pn[4][4] = {};
    double dt_n = 0.0, sr_n = 0.0, cr_n = 0.0;
    if (ns > 0) {
        load_vec(p.fwd_mean, (size_t)ns - 1, B, t, xn);
        load_cov_m(p.fwd_cov, packed, (size_t)ns - 1, B, t, Pn);
        const size_t o = (size_t)(ns - 1) * B + t;
        dt_n = p.dt[o];
        sr_n = srp[o];
        cr_n = crp[o];
    }
    int st = 0;
    EigBasis fan_basis, pb_basis;
    fan_basis.valid = false;
    pb_basis.valid = false;
    for (int k = p.Nmax - 1; k >= 0; --k) {
        if (!__any(k < ns)) continue;  // ragged batch: nobody in this wave has reached its last step yet
        if (k < ns) {
            double xk[4], Pk[4][4];
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                xk[r] = xn[r];
                STE_UNROLL
                for (int c = 0; c < 4; ++c) Pk[r][c] = Pn[r][c];
            }
            const double dt = dt_n, sr = sr_n, cr = cr_n;
            if (k > 0) {
                load_vec(p.fwd_mean, (size_t)k - 1, B, t, xn);
                load_cov_m(p.fwd_cov, packed, (size_t)k - 1, B, t, Pn);
                const size_t o = (size_t)(k - 1) * B + t;
                dt_n = p.dt[o];
                sr_n = srp[o];
                cr_n = crp[o];
            }
            double sig0[9][4], sig[9][4];
            if ((k & (kColdEvery - 1)) == kColdEvery - 1) {
                fan_basis.valid = false;
                pb_basis.valid = false;
            }
            st |= propagate_fan<true>(xk, Pk, p.m.fan_scale, dt, sr, cr, sig0, sig, fan_basis);
            double xb[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) {
                double acc = 0.0;
                STE_UNROLL
                for (int j = 1; j < 9; ++j) acc += sig[j][c];
                xb[c] = fma(p.m.w0, sig[0][c], p.m.wi * acc);
            }
            if (p.noise_rts) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) xb[c] += p.noise_rts[((size_t)k * 4 + c) * B + t];
            }
            // P_b is centred on the filtered mean x_k, not on x_b (unscented.py:324-325)
            double dk[9][4], db[9][4];
            STE_UNROLL
            for (int j = 0; j < 9; ++j) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) {
                    dk[j][c] = sig[j][c] - xk[c];
                    db[j][c] = sig[j][c] - xb[c];
                    sig0[j][c] -= xk[c];
                }
            }
            double Pb[4][4], D[4][4], Pbi[4][4], K[4][4];
            weighted_outer<true>(dk, dk, p.m.w0, p.m.wi, Pb);
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) Pb[r][c] += STE_BWD_Q(r, c);
            }
            weighted_outer<false>(sig0, db, p.m.w0, p.m.wi, D);  // unscented.py:328-330
            st |= sym_pinv4<true>(Pb, Pbi, pb_basis);
            pb_basis.valid = true;
            mm(D, Pbi, K);  // unscented.py:333
            double y[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) y[c] = xs[c] - xb[c];
            y[3] = wrap180(y[3]);
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                double acc = xk[r];
                STE_UNROLL
                for (int c = 0; c < 4; ++c) acc = fma(K[r][c], y[c], acc);
                xs[r] = acc;
            }
            xs[3] = floored_mod(xs[3], 360.0);
            double dP[4][4], KdP[4][4], U[4][4];
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) dP[r][c] = Ps[r][c] - Pb[r][c];
            }
            mm(K, dP, KdP);
            mmt_sym(KdP, K, U);
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) Ps[r][c] = Pk[r][c] + U[r][c];
            }
            store_vec(p.sm_mean, (size_t)k, B, t, xs);
            store_cov_m(p.sm_cov, packed, (size_t)k, B, t, Ps);
            store_pos(p, (size_t)k, B, t, xs);
        }
    }
    if (!all_finite(xs, Ps)) st |= STE_STATUS_NAN;
    if (st) atomicOr(&p.status[t], st);
