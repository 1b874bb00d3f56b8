// ste_forward_quad.hip — the UKF forward pass with one DPP quad per track (ste_quad.h) for gfx950 (MI355X), and the choice
// between it and the lane-per-track pass of ste_kernels.hip.  fp64 throughout; no MFMA (4x4 contractions); the whole per-track
// state lives in VGPRs.  The kernel declares no LDS and does not synchronise through it (it exchanges rows by DPP); its
// instantiations with the smoother's rows or the robust loop do carry 4 096 B of compiler-allocated LDS each -- hipcc promotes
// a small dynamically indexed private array (the q-dependent row stores) to LDS instead of scratch (SQ_INSTS_LDS in
// profiles/r03_pmc_counters_per_launch.csv).
//
// Kernels:
//   ukf_forward_q4                       forward filter, one DPP quad per track (chosen by batch size or by flag); with
//                                        rts_work it also leaves the smoother's cross-covariance D and, where it does not
//                                        follow from the history, its x_b and P_b
//
// Reference semantics (paths relative to the reference's src/track_estimators/kalman_filters/):
//   forward  : kalman_filter.py:61-117 (driver), unscented.py:178-207 (predict), :219-265 (update)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_ukf.h"
#include "ste_quad.h"

namespace ste {

// ---------------------------------------------------------------------------------------------------------------
// forward pass, one DPP quad per track (ste_quad.h)
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tri_index(int r, int c) { return r * 4 - (r * (r - 1)) / 2 + (c - r); }  // r <= c

// Predict for a quad (unscented.py:178-207) and, when `work` is given, the smoother's x_b, P_b, D of this step.
// With T = sqrtm(scale P) the cross-covariance is D = wi sum_i T_i (chi'_{i+} - chi'_{i-})^T (the centre's deviation is
// zero and x_b cancels in the difference), and P_b, which is centred on x_k instead of on the predicted mean, follows
// from the predicted covariance by P_b = P^- + e b^T + b e^T + b b^T with b = x^- - x_k and e = (weighted mean) - x^-
// (= minus the injected predict noise; zero in noise-free runs), because the weights sum to one.
template <class KT, class KG>
__device__ __forceinline__ int quad_predict(const Mats& p, const QuadCtx& cx, double (&x)[4], double (&Px)[4],
                                            QuadBasis& basis, double dt, double sr, double cr, const double* noise,
                                            const double* noise_rts, double* work, size_t nrow, size_t B, size_t t,
                                            bool full_row, bool noise_mode, bool& flagged, double* first_bad,
                                            const KT& tk, const KG& gk) {
    double Tn[4], s0[4], sp[4], sm[4], m[4], xp[4];
    int st = quad_sym_sqrt(Px, p.fan_scale, cx, basis, Tn);
    quad_propagate<KT, KG>(x, Tn, dt, sr, cr, s0, sp, sm, tk, gk);
    STE_UNROLL
    for (int c = 0; c < 4; ++c) m[c] = fma(p.w0, s0[c], p.wi * quad_sum(sp[c] + sm[c]));
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xp[c] = m[c];
    if (noise) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) xp[c] += noise[(nrow * 4 + c) * B + t];
    }
    double Pn[4];
    quad_scatter(s0, sp, sm, xp, p.w0, p.wi, cx, Pn);
    if (work) {
        const int q = cx.q;
        double xb[4], D[2], bv[4], bx[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            xb[c] = m[c];
            bv[c] = xp[c] - x[c];
        }
        if (noise_rts) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) xb[c] += noise_rts[(nrow * 4 + c) * B + t];
        }
        STE_UNROLL
        for (int c = 0; c < 2; ++c) {  // columns 0-1 of D (row q): sum_l T[q][l] (chi'_{l+} - chi'_{l-})[c]
            const double dlt = sp[c] - sm[c];
            double acc = Tn[0] * bcast<0>(dlt);
            acc = fma(Tn[1], bcast<1>(dlt), acc);
            acc = fma(Tn[2], bcast<2>(dlt), acc);
            acc = fma(Tn[3], bcast<3>(dlt), acc);
            D[c] = acc;
        }
        xorperm(bv, q, bx);
        double Pb[4];
        STE_UNROLL
        for (int s = 0; s < 4; ++s) Pb[s] = fma(bx[0], bx[s], Pn[s]);
        if (noise) {
            double ev[4], ex[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) ev[c] = m[c] - xp[c];
            xorperm(ev, q, ex);
            STE_UNROLL
            for (int s = 0; s < 4; ++s) Pb[s] += fma(ex[0], bx[s], bx[0] * ex[s]);
        }
        double* w = work + (nrow * kWorkElems) * B + t;
        if (q < 2 || noise_mode) {  // rows 2-3: only with recorded noise, else the smoother takes them from P_b (see kWorkD)
            STE_UNROLL
            for (int c = 0; c < 2; ++c) w[(kWorkD + q * 2 + c) * B] = p.wi * D[c];  // row q of D, columns 0-1
        }
        if (full_row) {  // elsewhere the smoother rebuilds x_b and P_b from history rows k and k + 1 (see kWorkD)
            w[(kWorkXb + q) * B] = sel4(xb, q);
            STE_UNROLL
            for (int s = 0; s < 4; ++s) {
                const int c = q ^ s;
                if (c >= q) w[(kWorkPb + tri_index(q, c)) * B] = Pb[s];
            }
        }
        int stq = st & (STE_STATUS_CLAMPED | STE_STATUS_NOCONV);  // each lane saw its own eigenvalue: combine over the quad
        stq |= dpp_move_i<0xB1>(stq);
        stq |= dpp_move_i<0x4E>(stq);
        const bool bad_now = stq != 0;
        if (bad_now && !flagged && q == 0) *first_bad = (double)((long long)nrow + late_k0());  // absolute step index
        flagged = flagged || bad_now;
        if (flagged) {
            // columns 2-3 of D (row q): 2 wi (T T)[q][2:4] -- (2 wi scale) P_k[q][2:4] only for an exact square root
            STE_UNROLL
            for (int c = 2; c < 4; ++c) {
                double acc = Tn[0] * bcast<0>(Tn[c]);
                acc = fma(Tn[1], bcast<1>(Tn[c]), acc);
                acc = fma(Tn[2], bcast<2>(Tn[c]), acc);
                acc = fma(Tn[3], bcast<3>(Tn[c]), acc);
                w[(kWorkD23 + q * 2 + (c - 2)) * B] = (p.wi + p.wi) * acc;
            }
        }
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) {
        x[c] = xp[c];
        Px[c] = Pn[c];
    }
    return st;
}

// Measurement update for a quad (unscented.py:219-265): every 4x4 product is one row per lane, rows of the other
// operand arrive by quad broadcasts.
template <bool kRobust>
__device__ __forceinline__ int quad_update(const Mats& p, const QuadCtx& cx, double (&x)[4], double (&Px)[4],
                                           const double (&zin)[4], const double* noise, size_t nrow, size_t B,
                                           size_t t) {
    const int q = cx.q;
    double z[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) z[c] = zin[c];
    if (noise) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) z[c] += noise[(nrow * 4 + c) * B + t];
    }
    // G = P H^T (row q): G[c] = sum_k P[q][q^k] H[c][q^k]
    double G[4], Sn[4], Sin[4], K[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) {
        double acc = Px[0] * cx.HTx[c][0];
        STE_UNROLL
        for (int k = 1; k < 4; ++k) acc = fma(Px[k], cx.HTx[c][k], acc);
        G[c] = acc;
    }
    quad_mm_rows(cx.Hrow, G, Sn);  // H G = H P H^T (row q)
    double Rrow[4];                // row q of the measurement covariance this update runs with
    STE_UNROLL
    for (int c = 0; c < 4; ++c) Rrow[c] = cx.Rrow[c];
    int rst = 0;
    if (kRobust) {
        // Opt-in robustification (check_robustness, unscented.py:353-387) on the un-noised observation with the
        // reference's y = z - x: while gamma = |y^T S^+ y| exceeds chi_alpha, lambda += (gamma - chi)/(y^T S^+ R S^+ y) and
        // R <- lambda R (compounding, as written there).  A quad's four lanes see the same gamma; tracks that are done
        // keep their values while others in the wave iterate.
        double y0[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) y0[c] = zin[c] - x[c];
        const double yq = sel4(y0, q);
        auto terms = [&](double& gamma, double& denom) -> int {
            double S[4], Si[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) S[c] = Sn[c] + Rrow[c];
            const int pst = quad_sym_pinv(S, cx, Si);
            double uq = 0.0;  // (S^+ y)[q]
            STE_UNROLL
            for (int c = 0; c < 4; ++c) uq = fma(Si[c], y0[c], uq);
            gamma = fabs(quad_sum(yq * uq));
            double vq = 0.0;  // (R S^+ y)[q]
            vq = fma(Rrow[0], bcast<0>(uq), vq);
            vq = fma(Rrow[1], bcast<1>(uq), vq);
            vq = fma(Rrow[2], bcast<2>(uq), vq);
            vq = fma(Rrow[3], bcast<3>(uq), vq);
            denom = quad_sum(uq * vq);
            return pst;
        };
        double gamma, denom, lambda = 1.0;
        rst |= terms(gamma, denom);
        for (int it = 0; it < p.robust_iters; ++it) {
            const bool active = gamma > p.chi_alpha;
            if (!__any(active)) break;
            lambda = active ? lambda + (gamma - p.chi_alpha) / denom : lambda;
            STE_UNROLL
            for (int c = 0; c < 4; ++c) Rrow[c] = active ? Rrow[c] * lambda : Rrow[c];
            double g2, d2;
            const int pst = terms(g2, d2);
            if (active) {
                rst |= pst;
                gamma = g2;
                denom = d2;
            }
        }
        if (gamma > p.chi_alpha) rst |= STE_STATUS_ROBUST_CAP;
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) Sn[c] += Rrow[c];  // S = H P H^T + R
    const int st = quad_sym_pinv(Sn, cx, Sin) | rst;
    quad_mm_rows(G, Sin, K);  // K = G S^+  (row q)
    double y[4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        double hx = p.H[r * 4 + 0] * x[0];
        STE_UNROLL
        for (int c = 1; c < 4; ++c) hx = fma(p.H[r * 4 + c], x[c], hx);
        y[r] = z[r] - hx;
    }
    y[3] = wrap180(y[3]);
    double xq = sel4(x, q);
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xq = fma(K[c], y[c], xq);
    x[0] = bcast<0>(xq);
    x[1] = bcast<1>(xq);
    x[2] = bcast<2>(xq);
    x[3] = floored_mod(bcast<3>(xq), 360.0);
    // Joseph form: A = I - K H, P = A P A^T + K R K^T
    double A[4], KR[4], Pnat[4], AP[4], P1[4], P2[4], Pnew[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) {
        double kh = K[0] * p.H[0 * 4 + c], kr = K[0] * p.R[0 * 4 + c];
        STE_UNROLL
        for (int l = 1; l < 4; ++l) {
            kh = fma(K[l], p.H[l * 4 + c], kh);
            kr = fma(K[l], p.R[l * 4 + c], kr);
        }
        A[c] = ((c == q) ? 1.0 : 0.0) - kh;
        KR[c] = kr;
    }
    if (kRobust) quad_mm_rows(K, Rrow, KR);  // K R with this update's rescaled R (rows live one per lane)
    xorperm(Px, q, Pnat);
    quad_mm_rows(A, Pnat, AP);
    quad_mm_rows_t(AP, A, P1);
    quad_mm_rows_t(KR, K, P2);
    STE_UNROLL
    for (int c = 0; c < 4; ++c) Pnew[c] = P1[c] + P2[c];
    xorperm(Pnew, q, Px);
    return st;
}

// The same update for H = diag(1, 1, 0, 0) and an R confined to that block (every example and the CLI of the reference), in
// closed form like lane_update_sel2: S = H P H^T + R is 2 x 2, K = P[:, 0:2] S^+ has two columns, and the Joseph form needs the
// products with those two columns only.  Row q of every matrix in lane q; rows 0 and 1 of P and the two columns of K reach
// the other lanes by quad broadcasts.  ~150 instead of ~600 instructions per update; with kRobust the rescaling loop in closed
// form too (robust_rescale_sel2 on the three entries of the block, the same on every lane of the quad).
template <bool kRobust>
__device__ __forceinline__ int quad_update_sel2(const Mats& p, const QuadCtx& cx, double (&x)[4], double (&Px)[4],
                                                const double (&zin)[4], const double* noise, size_t nrow, size_t B,
                                                size_t t) {
#pragma clang fp contract(off)  // explicit fma() only
    const int q = cx.q;
    double z[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) z[c] = zin[c];
    double Pn[4];  // row q of P, natural order
    xorperm(Px, q, Pn);
    const double p00 = bcast<0>(Pn[0]), p11 = bcast<1>(Pn[1]);
    const double p01 = 0.5 * (bcast<0>(Pn[1]) + bcast<1>(Pn[0]));  // the quad keeps both triangles: symmetrised like quad_sym_pinv
    double r00 = p.R[0], r01 = p.R[1], r11 = p.R[5];
    int st = 0;
    if (kRobust) {
        double Pblk[10];
        STE_UNROLL
        for (int e = 0; e < 10; ++e) Pblk[e] = 0.0;
        Pblk[tix(0, 0)] = p00;
        Pblk[tix(0, 1)] = p01;
        Pblk[tix(1, 1)] = p11;
        st = robust_rescale_sel2(p, x, Pblk, z, r00, r01, r11);  // on the un-noised observation (unscented.py:228)
    }
    if (noise) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) z[c] += noise[(nrow * 4 + c) * B + t];
    }
    double Sm[4][4], Si[4][4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) Sm[r][c] = 0.0;
    }
    Sm[0][0] = p00 + r00;
    Sm[0][1] = p01 + r01;
    Sm[1][0] = Sm[0][1];
    Sm[1][1] = p11 + r11;
    sym_pinv4_block2(Sm, Si);
    const double i00 = Si[0][0], i01 = Si[0][1], i11 = Si[1][1];
    const double k0 = fma(Pn[1], i01, Pn[0] * i00), k1 = fma(Pn[1], i11, Pn[0] * i01);  // K[q][0], K[q][1]
    const double y0 = z[0] - x[0], y1 = z[1] - x[1];
    const double poison = fma(0.0, z[2], 0.0 * z[3]);  // K[:, 2:4] y[2:4] with K[:, 2:4] = 0: NaN iff z[2] or z[3] is not finite
    const double xq = fma(k1, y1, fma(k0, y0, sel4(x, q))) + poison;
    x[0] = bcast<0>(xq);
    x[1] = bcast<1>(xq);
    x[2] = bcast<2>(xq);
    x[3] = floored_mod(bcast<3>(xq), 360.0);
    // AP = (I - K H) P, row q:  P[q][c] - K[q][0] P[0][c] - K[q][1] P[1][c]
    double AP[4], K0c[4], K1c[4], Pnew[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) {
        AP[c] = fma(-k1, bcast<1>(Pn[c]), fma(-k0, bcast<0>(Pn[c]), Pn[c]));
    }
    K0c[0] = bcast<0>(k0);
    K0c[1] = bcast<1>(k0);
    K0c[2] = bcast<2>(k0);
    K0c[3] = bcast<3>(k0);
    K1c[0] = bcast<0>(k1);
    K1c[1] = bcast<1>(k1);
    K1c[2] = bcast<2>(k1);
    K1c[3] = bcast<3>(k1);
    const double kr0 = fma(k1, r01, k0 * r00), kr1 = fma(k1, r11, k0 * r01);  // (K R)[q][0:2]
    STE_UNROLL
    for (int c = 0; c < 4; ++c) {
        const double p1 = fma(-AP[1], K1c[c], fma(-AP[0], K0c[c], AP[c]));  // (A P A^T)[q][c]
        const double p2 = fma(kr1, K1c[c], kr0 * K0c[c]);                    // (K R K^T)[q][c]
        Pnew[c] = p1 + p2;
    }
    xorperm(Pnew, q, Px);
    return st;
}

// kSel: H = diag(1, 1, 0, 0) with R in the same block (chosen by launch_forward from the matrices): closed-form update.
template <bool kGains, bool kRobust, bool kSel>
// __launch_bounds__(64, 2): at most 256 VGPRs, so that two waves fit on a SIMD.  What no longer fits is needed only by the
// branching fallback of the propagation (its library-call constants go to scratch); the step loop itself has no scratch
// access.  Alone the kernel is 5 % faster than the 362-VGPR build (no AGPR traffic), and two forward passes on the same
// compute units take 3.5 ms together instead of 2 x 2.36: a lone wave leaves half of the fp64 pipe's issue slots unused.
__global__ __launch_bounds__(64, 2) void ukf_forward_q4(const KParams p) {
    const size_t B = (size_t)p.ld;  // row pitch of every per-track array
    // p.qpw quads per wave (16 fill it).  A wave pays for the slowest of its tracks at every step -- another Jacobi sweep, another
    // robust rescaling, the device-library fallback of the fan whenever ANY of its lanes asks -- so when there are fewer tracks than
    // the chip has SIMDs to spare, each gets a wave of its own (launch_forward): BASELINE configs[3]'s seven ships take 41 .. 89 ms
    // each on their own and 128 ms sharing one wave.
    const int quad = (int)(threadIdx.x >> 2);
    if (quad >= p.qpw) return;
    const size_t t = (size_t)blockIdx.x * (size_t)p.qpw + (size_t)quad;
    const int q = (int)(threadIdx.x & 3);
    if (t >= (size_t)p.B) return;  // whole quads leave together
    const bool cont = (p.flags & kFlagContinue) != 0;  // a later time slice (see ukf_forward_l1; full covariances only)
    const int ns = (p.nsteps ? p.nsteps[t] - p.k0 : p.Nmax);
    if (cont && ns <= 0) return;
    QuadCtx cx;
    quad_ctx_init(p.m, q, cx);
    // the sin / cos and arctangent polynomial coefficients in VGPRs for the whole kernel: a wave that has its SIMD to itself
    // pays an issue slot for every s_mov_b32 that brings half a literal into a register (92 of them in the step's main block,
    // 46 with these 23 coefficients resident).  The closed-form update (kSel) leaves the 46 registers free; the general one
    // (246-256 registers already) keeps the literals.
    typename std::conditional<kSel, TrigReg, TrigLit>::type tk;
    typename std::conditional<kSel, GeoReg, GeoLit>::type gk;
    trig_reg_init(tk);
    geo_reg_init(gk);

    double x[4], Px[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) x[c] = p.x0[c * B + t];
    STE_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int e = q * 4 + (q ^ k);
        Px[k] = (p.flags & STE_FLAG_SHARED_P0) ? p.P0[e] : p.P0[(size_t)e * B + t];
    }
    auto store_row = [&](size_t row) {
        p.fwd_mean[(row * 4 + q) * B + t] = sel4(x, q);
        STE_UNROLL
        for (int k = 0; k < 4; ++k) {
            const int c = q ^ k;
            if (!(p.flags & STE_FLAG_PACKED_COV))
                p.fwd_cov[(row * 16 + q * 4 + c) * B + t] = Px[k];
            else if (c >= q)
                p.fwd_cov[(row * 10 + tri_index(q, c)) * B + t] = Px[k];
        }
    };
    store_row(0);  // slot 0 = prior (kalman_filter.py:76-77)

    int st = cont ? (p.status[t] & ~STE_STATUS_NAN) : 0;
    bool flagged = false;
    double* first_bad = (kGains && p.rts_work) ? p.first_bad + t : nullptr;
    if (first_bad) {
        if (cont)
            flagged = *first_bad != kNeverBad;
        else if (q == 0)
            *first_bad = kNeverBad;
    }
    const bool noise_mode = p.noise_pred || p.noise_upd || p.noise_rts;
    const bool initial_update = !(p.flags & STE_FLAG_NO_INITIAL_UPDATE);
    if (kGains && initial_update && ns > 0) {
        // smoother step 0 reads history row 0 = the prior, not the state the first predict starts from
        double xc[4], Pc[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            xc[c] = x[c];
            Pc[c] = Px[c];
        }
        QuadBasis cold;
        cold.valid = false;
        st |= quad_predict(p.m, cx, xc, Pc, cold, p.dt[t], p.sog_rate[t], p.cog_rate[t], nullptr, p.noise_rts,
                           p.rts_work, 0, B, t, true, noise_mode, flagged, first_bad, tk, gk);
    }
    if (initial_update) {
        double z0[4];
        load_vec(p.z, 0, B, t, z0);
        st |= kSel ? quad_update_sel2<kRobust>(p.m, cx, x, Px, z0, p.noise_upd, 0, B, t)
                   : quad_update<kRobust>(p.m, cx, x, Px, z0, p.noise_upd, 0, B, t);  // kalman_filter.py:81
    }
    QuadBasis basis;
    basis.valid = false;
    double dt_n = 0.0, sr_n = 0.0, cr_n = 0.0;
    int ui_n = -1;
    if (ns > 0) {
        dt_n = p.dt[t];
        sr_n = p.sog_rate[t];
        cr_n = p.cog_rate[t];
        ui_n = p.upd_idx[t];
    }
    for (int k = 0; k < p.Nmax; ++k) {
        const bool live = k < ns;
        if (!__any(live)) break;
        if (live) {
            const double dt = dt_n, sr = sr_n, cr = cr_n;
            const int ui = ui_n;
            // Unconditional loads with clamped indices: a load inside an `if` makes hipcc drain the queue with
            // s_waitcnt vmcnt(0) where the branch rejoins, i.e. right after issuing it -- a full HBM round trip per step.
            double zk[4];
            const bool ui_ok = ui < p.Tmax;  // an observation column past the padded batch: flagged, update skipped
            load_vec(p.z, (size_t)((ui >= 0 && ui_ok) ? ui : 0), B, t, zk);
            {
                const size_t o = (size_t)(k + 1 < ns ? k + 1 : k) * B + t;
                dt_n = p.dt[o];
                sr_n = p.sog_rate[o];
                cr_n = p.cog_rate[o];
                ui_n = p.upd_idx[o];
            }
            if ((k & (kColdEvery - 1)) == 0) basis.valid = false;
            double* work = (kGains && !(k == 0 && initial_update)) ? p.rts_work : nullptr;
            st |= quad_predict(p.m, cx, x, Px, basis, dt, sr, cr, p.noise_pred, p.noise_rts, work, (size_t)k, B, t,
                               (ui >= 0 && ui_ok) || noise_mode, noise_mode, flagged, first_bad, tk, gk);
            if (ui >= 0 && ui_ok)
                st |= kSel ? quad_update_sel2<kRobust>(p.m, cx, x, Px, zk, p.noise_upd, (size_t)k + 1, B, t)
                           : quad_update<kRobust>(p.m, cx, x, Px, zk, p.noise_upd, (size_t)k + 1, B, t);
            if (!ui_ok) st |= STE_STATUS_BAD_INDEX;
            store_row((size_t)k + 1);
        }
    }
    double chk = 0.0;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) chk += x[c] * 0.0 + Px[c] * 0.0;
    if (!(chk == 0.0)) st |= STE_STATUS_NAN;
    st |= dpp_move_i<0xB1>(st);
    st |= dpp_move_i<0x4E>(st);
    if (q == 0) p.status[t] = st;
}

}  // namespace ste

// Lane mapping of the forward kernel.  A quad per track shortens the per-wave instruction stream ~1.7x and puts 4x as
// many waves on the chip, but replicates work across its lanes.  The quad forward kernel fits two waves on a SIMD
// (<= 256 VGPRs), so it stays a single round up to 32 768 tracks (2 048 waves), after which one lane per track wins
// (measured on MI355X).  STE_FLAG_LANES_1 / STE_FLAG_LANES_4 in the batch's flags override the choice for
// that call.
namespace {
constexpr int kQuadMaxTracks = 32768;
constexpr size_t kQuadSpreadWaves = 1024;  // SIMDs of an MI355X: up to this many tracks, one quad (track) per wave
}  // namespace
int ste::choose_lanes(int B, unsigned flags) {
    if (flags & STE_FLAG_LANES_1) return 1;
    if (flags & STE_FLAG_LANES_4) return 4;
    return B <= kQuadMaxTracks ? 4 : 1;
}

// The quad launch of launch_forward (ste_kernels.hip), which has looked at choose_lanes.
int ste::launch_forward_q4(const ste::KParams& kp, hipStream_t s) {
    // quads per wave: 16 fill a wave; with fewer tracks than SIMDs to spare every track gets a wave (and a SIMD) of its own,
    // so that no track waits for another's extra sweep, rescaling or slow-path fan (see ukf_forward_q4)
    ste::KParams kq = kp;
    kq.qpw = (int)std::min<size_t>(16, std::max<size_t>(1, ((size_t)kp.B + kQuadSpreadWaves - 1) / kQuadSpreadWaves));
    const unsigned gridq = (unsigned)(((size_t)kp.B + kq.qpw - 1) / kq.qpw);
    const int which = (kp.m.robust_iters > 0 ? 4 : 0) | (kp.rts_work ? 2 : 0) | (kp.fast_upd ? 1 : 0);
    switch (which) {
#define STE_Q4(n, g, r, f) \
    case n: hipLaunchKernelGGL((ste::ukf_forward_q4<g, r, f>), dim3(gridq), dim3(64), 0, s, kq); break;
        STE_Q4(0, false, false, false) STE_Q4(1, false, false, true) STE_Q4(2, true, false, false) STE_Q4(3, true, false, true)
        STE_Q4(4, false, true, false) STE_Q4(5, false, true, true) STE_Q4(6, true, true, false) STE_Q4(7, true, true, true)
#undef STE_Q4
    }
    return abi_check_hip(hipGetLastError(), "ukf_forward_q4 launch");
}
