// ste_kernels.hip — batched UKF forward pass, lane per track, the stand-alone unscented RTS smoother and the single-step
// kernels for gfx950 (MI355X), plus the C ABI of include/ste.h.  fp64 throughout; no MFMA (4x4 contractions); the whole
// per-track state lives in VGPRs.  The only LDS a kernel of this file declares is g_sched_word, two words in which
// ukf_forward_sched parks its slice offset; nothing synchronises through LDS.  Three kernel families are in files of their
// own, each with its launches: the quad forward kernel in ste_forward_quad.hip, the smoothers that read the forward pass's work
// rows in ste_smooth.hip, the posterior-track sampler in ste_sample.hip.  What the four share on the device is in ste_ukf.h
// (and ste_smooth.h), the host functions that cross a file in ste_err.h.  The families of this file stay one code object:
// hipcc shapes ukf_update, propagate_points and propagate_fan_branching by all their callers (profiles/kernels_split.md).
//
// Kernels:
//   ukf_forward_l1                       forward filter, one lane per track (the quad form is chosen by batch size or by
//                                        flag); with rts_work it also leaves the smoother's cross-covariance D and,
//                                        where it does not follow from the history, its x_b and P_b
//   ukf_forward_sched + sched_gate       the forward passes of MANY batches / fleet windows as one launch of resident waves
//     + sched_upload                     working through a host-made schedule of (64-track tile, time slice) items -- the
//                                        body is ukf_forward_l1's --, the one-wave gate a smoother's stream waits behind,
//                                        and the upload of the schedule's table from page-locked memory
//   ukf_forward_l1_plain,                ukf_forward_l1 / ukf_forward_sched <true, true, false> for plain batches (ste_ukf.h:
//     ukf_forward_sched_plain            plain_batch): packed layout and no recorded noise compiled into the step loop
//   urtss_backward_l1                    stand-alone smoother that recomputes everything (rts_work == NULL)
//   ukf_forward_lik, ukf_forward_tn,     the lane-per-track forward pass with the likelihood, and it and the stand-alone
//     urtss_backward_l1<true>            smoother with per-track Q / R (ste_ukf_noise_f64): instantiations of the same
//                                        device functions and kernels, the track's matrices loaded from NoiseParams
//   predict / update / robust_terms / geodetic / sigma_points kernels   single-step API parity
// All per-step inputs/outputs are SoA with the track index fastest, so a wave's accesses are contiguous runs.
//
// Reference semantics (paths relative to the reference's src/track_estimators/kalman_filters/):
//   forward  : kalman_filter.py:61-117 (driver), unscented.py:178-207 (predict), :219-265 (update)
//   backward : unscented.py:285-351 (rts_step)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_ukf.h"

namespace ste {

// The scheduled forward kernel (ukf_forward_sched) has no KParams in its argument segment: the work item's slice offset is
// parked in a word of LDS (one wave per workgroup) and read back where it is used, for the same reason.
__shared__ int g_sched_word[2];  // [0] the slice offset k0 of the item being run, [1] the wave's position in its item list
__device__ __forceinline__ int sched_k0() { return *(volatile int*)&g_sched_word[0]; }

// Sigma fan of (x, P): dev[i] = column i of sqrtm(scale*P) (unscented.py:95-105).  chi_{i+1} = x + dev[i],
// chi_{i+1+n} = x - dev[i], chi_0 = x.  T is symmetric, so column i == row i.
template <bool kWarm>
__device__ __forceinline__ int sigma_fan(const double (&x)[4], const double (&P)[4][4], double scale,
                                         double (&sig)[9][4], EigBasis& basis);

__device__ __forceinline__ int sigma_fan(const double (&x)[4], const double (&P)[4][4], double scale,
                                         double (&sig)[9][4]) {
    EigBasis none;
    return sigma_fan<false>(x, P, scale, sig, none);
}

template <bool kWarm>
__device__ __forceinline__ int sigma_fan(const double (&x)[4], const double (&P)[4][4], double scale,
                                         double (&sig)[9][4], EigBasis& basis) {
    double T[4][4];
    const int st = sym_sqrt4<kWarm>(P, scale, T, basis);
    if (kWarm) basis.valid = true;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) sig[0][c] = x[c];
    STE_UNROLL
    for (int i = 0; i < 4; ++i) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            sig[1 + i][c] = x[c] + T[c][i];
            sig[5 + i][c] = x[c] - T[c][i];
        }
    }
    return st;
}

// Sigma fan of (x, P) pushed through the process model (unscented.py:183-191 = :301-312):
//   sig0[j]  the fan itself: x, x + col_i(T), x - col_i(T) with T = sqrtm(scale * P)
//   sig[j]   geodetic_dynamics(sig0[j], dt, sog_rate, cog_rate)
// The 2n points come in +- pairs around the centre, so their angles are (centre angle) +- (small increment) and
// sin/cos of all of them follow from the centre's three sincos and one sincos per increment by the angle-addition
// formulas: 15 sincos evaluations instead of 27, 12 of them on small arguments that need no range reduction.
__device__ __noinline__ void propagate_fan_branching(const double (&x)[4], const double (&T)[4][4], double dt, double sr,
                                                        double cr, double (&sig0)[9][4], double (&sig)[9][4]) {
    const double dt_r = dt / kEarthRadius;
    const double du = sr * dt, da = cr * dt;
    // centre
    const double lat0 = x[1] * kDeg2Rad, alpha0 = x[3] * kDeg2Rad, delta0 = x[2] * dt_r;
    double sp0, cp0, sa0, ca0, sd0, cd0;
    sincos_fast(lat0, sp0, cp0);
    sincos_fast(alpha0, sa0, ca0);
    sincos_fast(delta0, sd0, cd0);
    STE_UNROLL
    for (int c = 0; c < 4; ++c) sig0[0][c] = x[c];
    geodetic_finish(x[0] * kDeg2Rad, lat0, sp0, cp0, sa0, ca0, sd0, cd0, sig[0][0], sig[0][1]);
    sig[0][2] = x[2] + du;
    sig[0][3] = alpha0 * kRad2Deg + da;
    STE_UNROLL
    for (int i = 0; i < 4; ++i) {
        // increments of the three angles along column i of T (T symmetric: T[c][i] == T[i][c])
        double sdp, cdp, sda, cda, sdd, cdd;
        sincos_delta(T[1][i] * kDeg2Rad, sdp, cdp);
        sincos_delta(T[3][i] * kDeg2Rad, sda, cda);
        sincos_delta(T[2][i] * dt_r, sdd, cdd);
        const double p1 = sp0 * cdp, p2 = cp0 * sdp, p3 = cp0 * cdp, p4 = sp0 * sdp;
        const double a1 = sa0 * cda, a2 = ca0 * sda, a3 = ca0 * cda, a4 = sa0 * sda;
        const double d1 = sd0 * cdd, d2 = cd0 * sdd, d3 = cd0 * cdd, d4 = sd0 * sdd;
        STE_UNROLL
        for (int sgn = 0; sgn < 2; ++sgn) {
            const int j = 1 + i + 4 * sgn;
            double pt[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) pt[c] = sgn ? x[c] - T[c][i] : x[c] + T[c][i];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) sig0[j][c] = pt[c];
            const double sp = sgn ? p1 - p2 : p1 + p2, cp = sgn ? p3 + p4 : p3 - p4;
            const double sa = sgn ? a1 - a2 : a1 + a2, ca = sgn ? a3 + a4 : a3 - a4;
            const double sd = sgn ? d1 - d2 : d1 + d2, cd = sgn ? d3 + d4 : d3 - d4;
            geodetic_finish(pt[0] * kDeg2Rad, pt[1] * kDeg2Rad, sp, cp, sa, ca, sd, cd, sig[j][0], sig[j][1]);
            sig[j][2] = pt[2] + du;
            sig[j][3] = (pt[3] * kDeg2Rad) * kRad2Deg + da;
        }
    }
}

// The same fan with the several-at-a-time, branch-free helpers of ste_math.h (each polynomial coefficient is fetched once
// for the three angles of the centre, once per direction for its three increments, and once per direction for its +/-
// pair); a wave in which some lane leaves their validity range redoes the step with the branching version above.
__device__ __forceinline__ void propagate_points(const double (&x)[4], const double (&T)[4][4], double dt, double sr,
                                                 double cr, double (&sig0)[9][4], double (&sig)[9][4]) {
#pragma clang fp contract(off)  // explicit fma() only: the same bits in every kernel this is inlined into
    const double dt_r = div_earth_radius(dt);

    const double du = sr * dt, da = cr * dt;
    bool ok = true;
    const double lat0 = x[1] * kDeg2Rad, alpha0 = x[3] * kDeg2Rad, delta0 = x[2] * dt_r;
    const double a0[3] = {lat0, alpha0, delta0};
    double s_0[3], c_0[3];
    sincos_fast_n<3>(a0, s_0, c_0, ok);
    const double sp0 = s_0[0], cp0 = c_0[0], sa0 = s_0[1], ca0 = c_0[1], sd0 = s_0[2], cd0 = c_0[2];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) sig0[0][c] = x[c];
    {
        const double lo[1] = {x[0] * kDeg2Rad}, la[1] = {lat0}, vsp[1] = {sp0}, vcp[1] = {cp0}, vsa[1] = {sa0},
                     vca[1] = {ca0}, vsd[1] = {sd0}, vcd[1] = {cd0};
        double lon_o[1], lat_o[1];
        geodetic_finish_n<1>(lo, la, vsp, vcp, vsa, vca, vsd, vcd, lon_o, lat_o, ok);
        sig[0][0] = lon_o[0];
        sig[0][1] = lat_o[0];
    }
    sig[0][2] = x[2] + du;
    sig[0][3] = fma(alpha0, kRad2Deg, da);
    STE_UNROLL
    for (int i = 0; i < 4; ++i) {
        const double dl[3] = {T[1][i] * kDeg2Rad, T[3][i] * kDeg2Rad, T[2][i] * dt_r};
        double s_d[3], c_d[3];
        sincos_delta_n<3>(dl, s_d, c_d, ok);
        const double p2 = cp0 * s_d[0], p4 = sp0 * s_d[0], a2 = ca0 * s_d[1], a4 = sa0 * s_d[1], d2 = cd0 * s_d[2],
                     d4 = sd0 * s_d[2];
        double ptp[4], ptm[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            ptp[c] = x[c] + T[c][i];
            ptm[c] = x[c] - T[c][i];
            sig0[1 + i][c] = ptp[c];
            sig0[5 + i][c] = ptm[c];
        }
        const double lo[2] = {ptp[0] * kDeg2Rad, ptm[0] * kDeg2Rad}, la[2] = {ptp[1] * kDeg2Rad, ptm[1] * kDeg2Rad};
        const double vsp[2] = {fma(sp0, c_d[0], p2), fma(sp0, c_d[0], -p2)};
        const double vcp[2] = {fma(cp0, c_d[0], -p4), fma(cp0, c_d[0], p4)};
        const double vsa[2] = {fma(sa0, c_d[1], a2), fma(sa0, c_d[1], -a2)};
        const double vca[2] = {fma(ca0, c_d[1], -a4), fma(ca0, c_d[1], a4)};
        const double vsd[2] = {fma(sd0, c_d[2], d2), fma(sd0, c_d[2], -d2)};
        const double vcd[2] = {fma(cd0, c_d[2], -d4), fma(cd0, c_d[2], d4)};
        double lon_o[2], lat_o[2];
        geodetic_finish_n<2>(lo, la, vsp, vcp, vsa, vca, vsd, vcd, lon_o, lat_o, ok);
        sig[1 + i][0] = lon_o[0];
        sig[1 + i][1] = lat_o[0];
        sig[1 + i][2] = ptp[2] + du;
        sig[1 + i][3] = fma(ptp[3] * kDeg2Rad, kRad2Deg, da);
        sig[5 + i][0] = lon_o[1];
        sig[5 + i][1] = lat_o[1];
        sig[5 + i][2] = ptm[2] + du;
        sig[5 + i][3] = fma(ptm[3] * kDeg2Rad, kRad2Deg, da);
    }
    double fin = dt + sr + cr;  // non-finite lanes end in NaN on either path: they do not ask for the slow one
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        fin += x[r];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) fin += T[r][c];
    }
    if (__builtin_expect(__any(!ok && fin * 0.0 == 0.0), 0)) {
        // Out of line, through copies: the branching version calls the device library (Payne-Hanek sincos, atan2, asin) and
        // is ~55 KB of code; inlined it tripled this kernel's size and register pressure.  Its arguments are address-taken,
        // so they are private copies here and the hot path's arrays stay in registers.
        double xc[4], Tc[4][4], s0c[9][4], sc[9][4];
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            xc[r] = x[r];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) Tc[r][c] = T[r][c];
        }
        propagate_fan_branching(xc, Tc, dt, sr, cr, s0c, sc);
        STE_UNROLL
        for (int j = 0; j < 9; ++j) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) {
                sig0[j][c] = s0c[j][c];
                sig[j][c] = sc[j][c];
            }
        }
    }
}


template <bool kWarm>
__device__ __forceinline__ int propagate_fan(const double (&x)[4], const double (&P)[4][4], double scale, double dt,
                                             double sr, double cr, double (&sig0)[9][4], double (&sig)[9][4],
                                             EigBasis& basis) {
    double T[4][4];
    const int st = sym_sqrt4<kWarm>(P, scale, T, basis);
    if (kWarm) basis.valid = true;
    propagate_points(x, T, dt, sr, cr, sig0, sig);
    return st;
}

// sum_j W_j a_j b_j^T  for two sets of 9 deviation vectors.
template <bool kSym>
__device__ __forceinline__ void weighted_outer(const double (&a)[9][4], const double (&b)[9][4], double w0, double wi,
                                               double (&out)[4][4]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = kSym ? r : 0; c < 4; ++c) {
            double acc = 0.0;
            STE_UNROLL
            for (int j = 1; j < 9; ++j) acc = fma(a[j][r], b[j][c], acc);
            acc = fma(w0 * a[0][r], b[0][c], wi * acc);
            out[r][c] = acc;
            if (kSym) out[c][r] = acc;
        }
    }
}

// UKF predict (unscented.py:178-207), the literal form: the whole fan, the weighted mean, the weighted outer products.
// x, P updated in place.  Used by the single-step entry point (ste_ukf_predict_f64); the forward kernels run the streamed
// form of the same arithmetic (lane_predict / quad_predict).
__device__ __forceinline__ int ukf_predict(const Mats& p, double (&x)[4], double (&P)[4][4], double dt, double sr,
                                           double cr, const double* noise, size_t nrow, size_t B, size_t t) {
    double sig[9][4], sig0[9][4], T[4][4];
    EigBasis none;
    const int st = sym_sqrt4<false>(P, p.fan_scale, T, none);
    propagate_points(x, T, dt, sr, cr, sig0, sig);
    double xp[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) {
        double acc = 0.0;
        STE_UNROLL
        for (int j = 1; j < 9; ++j) acc += sig[j][c];
        xp[c] = fma(p.w0, sig[0][c], p.wi * acc);
    }
    if (noise) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) xp[c] += noise[(nrow * 4 + c) * B + t];
    }
    STE_UNROLL
    for (int j = 0; j < 9; ++j) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) sig[j][c] -= xp[c];
    }
    double Pn[4][4];
    weighted_outer<true>(sig, sig, p.w0, p.wi, Pn);
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        x[r] = xp[r];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) P[r][c] = Pn[r][c] + p.Q[r * 4 + c];
    }
    return st;
}

// Chang (2014) Mahalanobis terms of the robustification helpers (unscented.py:389-483), with the reference's y = z - x:
//   gamma = | y^T (H P H^T + R)^+ y |          criterion_index, :420-426
//   denom =   y^T (S^+ R S^+) y                  denominator of update_lambda_factor, :468-478
__device__ __forceinline__ int robust_terms(const double (&H)[4][4], const double (&R)[4][4], const double (&x)[4],
                                            const double (&P)[4][4], const double (&z)[4], double& gamma,
                                            double& denom) {
    double HP[4][4], S[4][4], Si[4][4], y[4], u[4], v[4];
    mm(H, P, HP);
    mmt(HP, H, S);
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        y[r] = z[r] - x[r];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) S[r][c] += R[r][c];
    }
    const int st = sym_pinv4(S, Si);
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        double acc = 0.0;
        STE_UNROLL
        for (int c = 0; c < 4; ++c) acc = fma(Si[r][c], y[c], acc);
        u[r] = acc;  // S^+ y
    }
    double g = 0.0, d = 0.0;
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        g = fma(y[r], u[r], g);
        double acc = 0.0;
        STE_UNROLL
        for (int c = 0; c < 4; ++c) acc = fma(R[r][c], u[c], acc);
        v[r] = acc;  // R S^+ y
    }
    STE_UNROLL
    for (int r = 0; r < 4; ++r) d = fma(u[r], v[r], d);  // (S^+ y)^T R (S^+ y) = y^T S^+ R S^+ y  (S^+ symmetric)
    gamma = fabs(g);
    denom = d;
    return st;
}

// Linear Kalman update with pseudo-inverse gain and Joseph-form covariance (unscented.py:219-265).
// kLik: also the update's log-likelihood terms into *lik (UpdLik, ste_math.h), from the eigenvalues the pseudo-inverse
// already has and the innovation it already forms.
// kTrackR: per-track noise (ste_ukf_forward_noise_f64): with `Rt` the track's own R, read here from its upper triangle
// Rt[e * B] (the order of STE_FLAG_PACKED_COV) -- per-track constants that stay in L2, loaded where they are used instead
// of held in registers across the step loop; Rt == nullptr: the shared R.  The arithmetic below is the same source either
// way.  One difference in control flow: the 2 x 2 shortcut of the pseudo-inverse is taken per lane instead of per wave, and
// only where the lane's own S is exactly confined to the block (no waiver for a non-finite S), so that a track's result
// does not depend on its neighbours' matrices (with a shared R the test is uniform anyway).
template <bool kLik = false, bool kTrackR = false>
__device__ __forceinline__ int ukf_update(const Mats& p, double (&x)[4], double (&P)[4][4], const double (&zin)[4],
                                          const double* noise, size_t nrow, size_t B, size_t t, UpdLik* lik = nullptr,
                                          const double* Rt = nullptr) {
    double H[4][4], R[4][4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            H[r][c] = p.H[r * 4 + c];
            R[r][c] = p.R[r * 4 + c];
        }
    }
    if constexpr (kTrackR) {
        if (Rt) {
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = r; c < 4; ++c) {
                    const double v = Rt[(size_t)tix(r, c) * B];
                    R[r][c] = v;
                    R[c][r] = v;
                }
            }
        }
    }
    double z[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) z[c] = zin[c];
    int rst = 0;
    if (p.robust_iters > 0) {
        // Opt-in robustification (check_robustness, unscented.py:353-387) on the un-noised observation: while the
        // criterion exceeds chi_alpha, lambda += (gamma - chi)/denom and R <- lambda R (compounding, as written there).
        double gamma, denom, lambda = 1.0;
        rst |= robust_terms(H, R, x, P, z, gamma, denom);
        for (int it = 0; it < p.robust_iters && gamma > p.chi_alpha; ++it) {
            lambda += (gamma - p.chi_alpha) / denom;
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) R[r][c] *= lambda;
            }
            rst |= robust_terms(H, R, x, P, z, gamma, denom);
        }
        if (gamma > p.chi_alpha) rst |= STE_STATUS_ROBUST_CAP;
    }
    if (noise) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) z[c] += noise[(nrow * 4 + c) * B + t];
    }
    double HP[4][4], S[4][4], Si[4][4], PHt[4][4], K[4][4];
    mm(H, P, HP);
    mmt(HP, H, S);
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) S[r][c] += R[r][c];
    }
    int st = rst;
    {
        bool blk = true;  // S confined to its leading 2 x 2 block (exact zeros elsewhere), for every track of the wave
        double fin = 0.0;
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) {
                if (r >= 2 || c >= 2) blk = blk && (S[r][c] == 0.0);
                fin += S[r][c];
            }
        }
        // a non-finite S is NaN on either route: no veto against the fast one.  (Per lane -- kTrackR -- there is no one to
        // veto: the lane takes the route its shared launch takes, which with a general R is sym_pinv4 whatever S holds, so
        // that the status bits of an already non-finite track are the shared launch's too.)
        if constexpr (!kTrackR) blk = blk || !(fin * 0.0 == 0.0);
        const bool take_blk = kTrackR ? blk : (bool)__all(blk);
        if constexpr (kLik) {
            if (take_blk) {
                double w[2];
                sym_pinv4_block2(S, Si, w);
                pinv_loglik_terms(w, *lik);
            } else {
                double w[4];
                st |= sym_pinv4(S, Si, w);
                pinv_loglik_terms(w, *lik);
            }
        } else {
            if (take_blk)
                sym_pinv4_block2(S, Si);
            else
                st |= sym_pinv4(S, Si);
        }
    }
    mmt(P, H, PHt);
    mm(PHt, Si, K);
    double y[4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        double hx = H[r][0] * x[0];
        STE_UNROLL
        for (int c = 1; c < 4; ++c) hx = fma(H[r][c], x[c], hx);
        y[r] = z[r] - hx;
    }
    y[3] = wrap180(y[3]);
    if constexpr (kLik) {
        double nis = 0.0;
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            double acc = 0.0;
            STE_UNROLL
            for (int c = 0; c < 4; ++c) acc = fma(Si[r][c], y[c], acc);
            nis = fma(y[r], acc, nis);  // y^T S^+ y
        }
        lik->nis = nis;
    }
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        double acc = x[r];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) acc = fma(K[r][c], y[c], acc);
        x[r] = acc;
    }
    x[3] = floored_mod(x[3], 360.0);
    double A[4][4], AP[4][4], KR[4][4], P1[4][4], P2[4][4];
    mm(K, H, A);
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) A[r][c] = ((r == c) ? 1.0 : 0.0) - A[r][c];
    }
    mm(A, P, AP);
    mmt_sym(AP, A, P1);
    mm(K, R, KR);
    mmt_sym(KR, K, P2);
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) P[r][c] = P1[r][c] + P2[r][c];
    }
    return st;
}

// ---------------------------------------------------------------------------------------------------------------
// forward pass, one lane per track (ste_lane.h)
// ---------------------------------------------------------------------------------------------------------------
// UKF predict (unscented.py:178-207) on packed (x, P), the sigma pairs streamed through running moments; with `work` it
// also leaves the smoother's row of this step (see kWorkD).  x, P are replaced by the predicted mean (+ recorded noise)
// and covariance.  `flagged` is sticky: set once a square root of this track was clamped or did not converge; from that
// step on columns 2-3 of D are stored as well.
// kPlain: inlined into a plain batch's step loop (forward_tile_l1), whose callers pass noise = noise_rts = nullptr.
// `before_stores` is called once, after the moment arithmetic and in front of the first store: the plain step loop consumes
// there what it loaded at the top of the step (every other caller passes nothing).
struct NoHook {
    __device__ __forceinline__ void operator()() const {}
};
template <bool kGains, bool kSched = false, bool kPlain = false, class Hook = NoHook>
__device__ __forceinline__ int lane_predict(const Mats& p, double (&x)[4], double (&P)[10], double (&V)[4][4], bool warm,
                                            double dt, double sr, double cr, const double* noise,
                                            const double* noise_rts, size_t nrow, size_t B, size_t t, double* work,
                                            bool full_row, bool noise_mode, bool& flagged, double* first_bad,
                                            const TrigReg& tk, const double (&Qv)[10], const Hook& before_stores = Hook()) {
#pragma clang fp contract(off)  // explicit fma() only: the same bits in every kernel this is inlined into
    double T[10];
    const int st = sym_sqrt_p(P, p.fan_scale, T, V, warm);
    bool ok = true;
    FanCentre g;
    fan_centre(x, dt, sr, cr, g, ok, tk);
    FanMoments f;
    moments_clear(f);
    {
        double lonp, latp, lonm, latm;
        fan_pair<0>(x, T, g, lonp, latp, lonm, latm, ok, tk);
        moments_add<0, kGains>(f, T, g.c[0], g.c[1], lonp, latp, lonm, latm);
        fan_pair<1>(x, T, g, lonp, latp, lonm, latm, ok, tk);
        moments_add<1, kGains>(f, T, g.c[0], g.c[1], lonp, latp, lonm, latm);
        fan_pair<2>(x, T, g, lonp, latp, lonm, latm, ok, tk);
        moments_add<2, kGains>(f, T, g.c[0], g.c[1], lonp, latp, lonm, latm);
        fan_pair<3>(x, T, g, lonp, latp, lonm, latm, ok, tk);
        moments_add<3, kGains>(f, T, g.c[0], g.c[1], lonp, latp, lonm, latm);
    }
    // A lane whose inputs are already non-finite fails every range test, but its outcome is NaN on either path: it must not
    // send its whole wave through the slow one (BASELINE configs[3]: five of seven ships go non-finite early -- duplicate
    // timestamps -- and dragged the two healthy ones along at a tenth of the speed, step after step).
    double fin = dt + sr + cr;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) fin += x[c];
    STE_UNROLL
    for (int e = 0; e < 10; ++e) fin += T[e];
    const bool finite_in = fin * 0.0 == 0.0;
    if (__builtin_expect(__any(!ok && finite_in), 0)) {
        // Some lane left the validity range of the branch-free transcendentals (a pole, a step of tens of degrees):
        // the whole fan again with the branching version (device-library sincos / atan2 / asin, out
        // of line, through copies so that the hot path's arrays stay in registers), same formulas for the lanes that
        // were fine, then the same moment sums.  (Same formulas, not the same bits: the branching version's centre point
        // and pairs go through one-at-a-time code whose last bits differ in places, so an ordinary track that shares a
        // wave with a lane out of range gets the fallback's bits for that step -- a known dependence on wave neighbours,
        // DESIGN.md section 5.)
        double xc[4], Tc[4][4], s0c[9][4], sc[9][4];
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            xc[r] = x[r];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) Tc[r][c] = T[tix(r, c)];
        }
        propagate_fan_branching(xc, Tc, dt, sr, cr, s0c, sc);
        STE_UNROLL
        for (int c = 0; c < 4; ++c) g.c[c] = sc[0][c];
        if constexpr (kPlain) {
            // Waited for in this cold branch: without recorded noise nothing reads the centre's speed and heading before
            // the work-row and history stores do, and a reload left pending where the branch rejoins puts a wait behind the
            // first of those stores on every step -- for the step's earlier stores too ("Store drain").
            g.c[2] = in_vgpr(g.c[2]);
            g.c[3] = in_vgpr(g.c[3]);
        }
        moments_clear(f);
        moments_add<0, kGains>(f, T, g.c[0], g.c[1], sc[1][0], sc[1][1], sc[5][0], sc[5][1]);
        moments_add<1, kGains>(f, T, g.c[0], g.c[1], sc[2][0], sc[2][1], sc[6][0], sc[6][1]);
        moments_add<2, kGains>(f, T, g.c[0], g.c[1], sc[3][0], sc[3][1], sc[7][0], sc[7][1]);
        moments_add<3, kGains>(f, T, g.c[0], g.c[1], sc[4][0], sc[4][1], sc[8][0], sc[8][1]);
    }
    // weighted mean and covariance about it: the weights sum to one (make_params refuses anything else), the centre's
    // deviation is zero, so mean = c' + wi s and cov = wi S - (wi s)(wi s)^T
    const double d0 = p.wi * f.s0, d1 = p.wi * f.s1;
    const double m[4] = {g.c[0] + d0, g.c[1] + d1, g.c[2], g.c[3]};
    double xp[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xp[c] = m[c];
    if (noise) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) xp[c] += noise[(nrow * 4 + c) * B + t];
    }
    const double two_wi = p.wi + p.wi;
    double Pn[10];
    Pn[tix(0, 0)] = fma(-d0, d0, p.wi * f.S[tix(0, 0)]);
    Pn[tix(0, 1)] = fma(-d0, d1, p.wi * f.S[tix(0, 1)]);
    Pn[tix(1, 1)] = fma(-d1, d1, p.wi * f.S[tix(1, 1)]);
    Pn[tix(0, 2)] = p.wi * f.S[tix(0, 2)];
    Pn[tix(0, 3)] = p.wi * f.S[tix(0, 3)];
    Pn[tix(1, 2)] = p.wi * f.S[tix(1, 2)];
    Pn[tix(1, 3)] = p.wi * f.S[tix(1, 3)];
    Pn[tix(2, 2)] = two_wi * f.S[tix(2, 2)];
    Pn[tix(2, 3)] = two_wi * f.S[tix(2, 3)];
    Pn[tix(3, 3)] = two_wi * f.S[tix(3, 3)];
    before_stores();
    if (kGains && work) {
        // The smoother's cross-covariance D = wi sum_i T_i (chi'_{i+} - chi'_{i-})^T (the centre's deviation from x_k is
        // zero and x_b cancels in the difference): rows 2-3 of its columns 0-1 are the cross moments S[c][2], S[c][3] just
        // formed, i.e. Pn before Q is added.
        double* w = work + (nrow * kWorkElems) * B + t;
        st_stream(&w[(kWorkD + 0) * B], p.wi * f.Dn[0][0]);
        st_stream(&w[(kWorkD + 1) * B], p.wi * f.Dn[0][1]);
        st_stream(&w[(kWorkD + 2) * B], p.wi * f.Dn[1][0]);
        st_stream(&w[(kWorkD + 3) * B], p.wi * f.Dn[1][1]);
        if (noise_mode) {  // otherwise the smoother takes rows 2-3 from P_b: D[2:4, 0:2] = (P_b - b b^T - Q)[0:2, 2:4]^T
            st_stream(&w[(kWorkD + 4) * B], Pn[tix(0, 2)]);
            st_stream(&w[(kWorkD + 5) * B], Pn[tix(1, 2)]);
            st_stream(&w[(kWorkD + 6) * B], Pn[tix(0, 3)]);
            st_stream(&w[(kWorkD + 7) * B], Pn[tix(1, 3)]);
        }
        const bool bad_now = (st & (STE_STATUS_CLAMPED | STE_STATUS_NOCONV)) != 0;
        if (bad_now && !flagged) *first_bad = (double)((long long)nrow + (kSched ? sched_k0() : late_k0()));  // absolute step index
        flagged = flagged || bad_now;
        if (flagged) {  // columns 2-3 of D = 2 wi (T T)[:, 2:4]: (2 wi scale) P_k[:, 2:4] only for an exact square root
            st_stream(&w[(kWorkD23 + 0) * B], two_wi * f.TT[0][0]);
            st_stream(&w[(kWorkD23 + 1) * B], two_wi * f.TT[0][1]);
            st_stream(&w[(kWorkD23 + 2) * B], two_wi * f.TT[1][0]);
            st_stream(&w[(kWorkD23 + 3) * B], two_wi * f.TT[1][1]);
            st_stream(&w[(kWorkD23 + 4) * B], Pn[tix(2, 2)]);
            st_stream(&w[(kWorkD23 + 5) * B], Pn[tix(2, 3)]);
            st_stream(&w[(kWorkD23 + 6) * B], Pn[tix(2, 3)]);
            st_stream(&w[(kWorkD23 + 7) * B], Pn[tix(3, 3)]);
        }
    }
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) Pn[tix(r, c)] += Qv[tix(r, c)];
    }
    if (noise) {  // the covariance is taken about the noised mean (unscented.py:203-205): + e e^T, e = mean - x^-
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = r; c < 4; ++c) Pn[tix(r, c)] = fma(m[r] - xp[r], m[c] - xp[c], Pn[tix(r, c)]);
        }
    }
    if (kGains && work && full_row) {
        // P_b is centred on the filtered mean x_k, not on the predicted one (unscented.py:324-325): with b = x^- - x_k,
        // e = (weighted mean) - x^-,  P_b = P^- + e b^T + b e^T + b b^T
        double* w = work + (nrow * kWorkElems) * B + t;
        double bv[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) bv[c] = xp[c] - x[c];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            double xb = m[c];
            if (noise_rts) xb += noise_rts[(nrow * 4 + c) * B + t];
            st_stream(&w[(kWorkXb + c) * B], xb);
        }
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = r; c < 4; ++c) {
                double v = fma(bv[r], bv[c], Pn[tix(r, c)]);
                if (noise) v += fma(m[r] - xp[r], bv[c], bv[r] * (m[c] - xp[c]));
                st_stream(&w[(kWorkPb + tix(r, c)) * B], v);
            }
        }
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) x[c] = xp[c];
    STE_UNROLL
    for (int e = 0; e < 10; ++e) P[e] = Pn[e];
    return st;
}

// Measurement update on packed (x, P): the closed form for H = diag(1, 1, 0, 0) (kFastUpd, chosen by launch_forward from
// the matrices), otherwise the general 4x4 route (any H, R; the opt-in robust rescaling).
// kLik: also the update's log-likelihood terms into *lik (either route).
// kTrackR: the track's own R from Rt[e * B] when Rt is given (see ukf_update); the closed form reads entries 00, 01, 11.
template <bool kFastUpd, bool kRobust = false, bool kLik = false, bool kTrackR = false>
__device__ __forceinline__ int lane_update(const Mats& p, double (&x)[4], double (&P)[10], const double (&zin)[4],
                                           const double* noise, size_t nrow, size_t B, size_t t, UpdLik* lik = nullptr,
                                           const double* Rt = nullptr) {
    if (kFastUpd) {
        double z[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) z[c] = zin[c];
        double r00 = p.R[0], r01 = p.R[1], r11 = p.R[5];
        if constexpr (kTrackR) {
            if (Rt) {
                r00 = Rt[(size_t)tix(0, 0) * B];
                r01 = Rt[(size_t)tix(0, 1) * B];
                r11 = Rt[(size_t)tix(1, 1) * B];
            }
        }
        int st = 0;
        if (kRobust) st = robust_rescale_sel2(p, x, P, z, r00, r01, r11);  // on the un-noised observation (unscented.py:228)
        if (noise) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) z[c] += noise[(nrow * 4 + c) * B + t];
        }
        lane_update_sel2<kLik>(r00, r01, r11, x, P, z, lik);
        return st;
    } else {
        double Pf[4][4];
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) Pf[r][c] = P[tix(r, c)];
        }
        const int st = ukf_update<kLik, kTrackR>(p, x, Pf, zin, noise, nrow, B, t, lik, Rt);
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = r; c < 4; ++c) P[tix(r, c)] = Pf[r][c];
        }
        return st;
    }
}

__device__ __forceinline__ void store_hist(const KParams& p, size_t row, size_t B, size_t t, const double (&x)[4],
                                           const double (&P)[10]) {
    STE_UNROLL
    for (int c = 0; c < 4; ++c) st_stream(&p.fwd_mean[(row * 4 + c) * B + t], x[c]);
    store_cov_p(p.fwd_cov, (p.flags & STE_FLAG_PACKED_COV) != 0, row, B, t, P);
}
// ... of a plain batch (ste_ukf.h: plain_batch): the packed layout compiled in
__device__ __forceinline__ void store_hist_packed(const KParams& p, size_t row, size_t B, size_t t, const double (&x)[4],
                                                  const double (&P)[10]) {
    STE_UNROLL
    for (int c = 0; c < 4; ++c) st_stream(&p.fwd_mean[(row * 4 + c) * B + t], x[c]);
    store_cov_p<true>(p.fwd_cov, row, B, t, P);
}

// One wave per SIMD, on purpose: the step loop issues a vector instruction in ~80 % of its cycles, so a second forward
// wave on the same SIMD gains next to nothing (measured: two per SIMD run 1.55x slower each), while waves of several
// passes that the dispatcher doubles up on some SIMDs leave others empty.  The kernel holds 254 registers (its state,
// plus the sin / cos coefficients and Q kept in VGPRs) and amdgpu_waves_per_eu(1, 1) pads the allocation to 264: a second
// forward wave never fits on a SIMD, a smoother wave (234, allocation 240) does (264 + 240 <= 512).
// kRobust: the closed-form update with the closed-form robust rescaling in front of it (a template parameter, so that the
// default instantiation's step loop is exactly the one measured without it); with kFastUpd false the general route reads
// robust_iters itself.
// kLik: the innovation log-likelihood (ste_ukf_forward_loglik_f64): kLikOff (every existing kernel), kLikHist (the pass
// as it is, plus the likelihood) or kLikOnly (no histories: store_hist skipped, kGains false, rts_work NULL).  l_u, the
// ranks and the update count add up in registers and are written once per track; `lk->nis`, if given, gets one row per
// history row (NaN where no update fired).
enum { kLikOff = 0, kLikHist = 1, kLikOnly = 2 };
struct LikParams {
    double* loglik;  // [ld] (indexed like status)
    int32_t* dof;    // [ld] or nullptr
    int32_t* nupd;   // [ld] or nullptr
    double* nis;     // [Nmax+1][ld] or nullptr
};

// a recorded-noise array of the batch, or -- kPlain -- the literal nullptr
template <bool kPlain>
__device__ __forceinline__ const double* noise_ptr(const double* q) {
    if constexpr (kPlain)
        return nullptr;
    else
        return q;
}
// kPlain: a plain batch (ste_ukf.h: plain_batch) -- packed histories, no recorded noise: `noise_mode` is false, the noise
// pointers handed to lane_predict / lane_update are literal nullptr and store_hist has the layout compiled in, so the step
// loop neither tests nor keeps live what cannot change during a launch.  Same arithmetic, same bits.
template <bool kGains, bool kFastUpd, bool kRobust, bool kSched, int kLik = kLikOff, bool kTrackNoise = false, bool kPlain = false>
__device__ __forceinline__ void forward_tile_l1(const KParams& p, const size_t t, const LikParams* lk = nullptr,
                                                const NoiseParams* nz = nullptr) {
    static_assert(kLik != kLikOnly || (!kGains && !kSched), "the likelihood-only pass writes no histories and no work rows");
    static_assert(!kPlain || (kLik == kLikOff && !kTrackNoise), "plain batches: the default entry points only");
    const size_t B = (size_t)p.ld;  // row pitch of every per-track array (= the batch's own width unless it is a window)
    if (t >= (size_t)p.B) return;
    // A later time slice of a forward pass (slice_params): x0 / P0 name history row k0 -- the state the previous launch
    // left, bit for bit -- and every per-step pointer row k0; the slice boundary is a multiple of kColdEvery, where the
    // eigenvector basis restarts from the identity anyway, so nothing else has to be carried.
    const bool cont = (p.flags & kFlagContinue) != 0;
    const int ns = (p.nsteps ? p.nsteps[t] - p.k0 : p.Nmax);
    if (cont && ns <= 0) return;  // this track ended in an earlier slice: its rows and its status are final

    double x[4], P[10];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) x[c] = p.x0[c * B + t];
    if (cont && (kPlain || (p.flags & STE_FLAG_PACKED_COV))) {
        load_cov_p(p.P0, true, 0, B, t, P);
    } else {
        // the prior enters as (P0 + P0^T) / 2: the host refuses a P0 that is not symmetric (batch._as44)
        double Pf[4][4];
        if (p.flags & STE_FLAG_SHARED_P0) {
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) Pf[r][c] = p.P0[r * 4 + c];
            }
        } else {
            load_mat(p.P0, 0, B, t, Pf);
        }
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = r; c < 4; ++c) P[tix(r, c)] = 0.5 * (Pf[r][c] + Pf[c][r]);
        }
    }
    if constexpr (kPlain)
        store_hist_packed(p, 0, B, t, x, P);
    else if (kLik != kLikOnly) store_hist(p, 0, B, t, x, P);  // slot 0 = prior (kalman_filter.py:76-77); a later slice rewrites row k0 with its own bits

    // (a later slice may run in the same launch, on the same wave, as the one that wrote these two words -- the scheduled
    //  kernel -- without a cache invalidate in between: read them past the CU's L1)
    int st = cont ? (__hip_atomic_load(&p.status[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~STE_STATUS_NAN) : 0;  // the NaN bit is taken from the final state, as in a whole pass
    const bool initial_update = !(p.flags & STE_FLAG_NO_INITIAL_UPDATE);
    const bool noise_mode = kPlain ? false : (p.noise_pred || p.noise_upd || p.noise_rts);
    bool flagged = false;  // sticky: a square root of this track was clamped or did not converge
    double* first_bad = (kGains && p.rts_work) ? p.first_bad + t : nullptr;
    if (first_bad) {
        if (cont)
            flagged = __hip_atomic_load(first_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kNeverBad;
        else
            *first_bad = kNeverBad;
    }
    TrigReg tk;  // sin / cos polynomial coefficients, in VGPRs for the whole kernel (ste_math.h)
    trig_reg_init(tk);
    double Qv[10];  // Q in VGPRs too: as kernel arguments its 20 words were spilled to VGPR lanes and read back every step
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) Qv[tix(r, c)] = in_vgpr(p.m.Q[r * 4 + c]);
    }
    const double* Rt = nullptr;  // kTrackNoise: this track's R triangle, or nullptr = the shared R
    if constexpr (kTrackNoise) {
        if (nz->Q) {
            STE_UNROLL
            for (int e = 0; e < 10; ++e) Qv[e] = nz->Q[(size_t)e * B + t];
        }
        if (nz->R) Rt = nz->R + t;
    }
    double V[4][4];
    if (kGains && initial_update && ns > 0) {
        // History row 0 is the PRIOR (kalman_filter.py:76-77) while the first predict starts from the state after the
        // initial update, so the smoother's step 0 (which reads row 0, unscented.py:301) needs its own fan: run the
        // predict arithmetic once on a copy of the prior, keep only the smoother's rows.
        double xc[4], Pc[10];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) xc[c] = x[c];
        STE_UNROLL
        for (int e = 0; e < 10; ++e) Pc[e] = P[e];
        st |= lane_predict<true, kSched, kPlain>(p.m, xc, Pc, V, false, p.dt[t], p.sog_rate[t], p.cog_rate[t], nullptr, noise_ptr<kPlain>(p.noise_rts), 0, B, t,
                                         p.rts_work, true, noise_mode, flagged, first_bad, tk, Qv);
    }
    double lik_sum = 0.0;  // kLik: sum of l_u, of the ranks, and the number of updates
    int lik_dof = 0, lik_nupd = 0;
    if (initial_update) {
        double z0[4];
        load_vec(p.z, 0, B, t, z0);
        if constexpr (kLik != kLikOff) {
            UpdLik u;
            st |= lane_update<kFastUpd, kRobust, true, kTrackNoise>(p.m, x, P, z0, p.noise_upd, 0, B, t, &u, Rt);
            lik_sum += update_loglik(u);
            lik_dof += u.rank;
            lik_nupd += 1;
            if (lk->nis) st_stream(&lk->nis[t], u.nis);
        } else {
            st |= lane_update<kFastUpd, kRobust, false, kTrackNoise>(p.m, x, P, z0, noise_ptr<kPlain>(p.noise_upd), 0, B, t, nullptr, Rt);  // kalman_filter.py:81
        }
    } else if (kLik != kLikOff && lk->nis) {
        st_stream(&lk->nis[t], __builtin_nan(""));
    }

    // The eigenvectors of the fan matrix carry over from step to step (warm start); restarted from the identity every
    // kColdEvery steps so that rounding in the accumulated rotations cannot build up over a long track.
    double dt_n = 0.0, sr_n = 0.0, cr_n = 0.0;
    int ui_n = -1;
    if (ns > 0) {
        dt_n = p.dt[t];
        sr_n = p.sog_rate[t];
        cr_n = p.cog_rate[t];
        ui_n = p.upd_idx[t];
    }
    // Consumed here, once: nothing pending from the prologue reaches the loop header, so the wait for a step's inputs (loaded
    // a whole step ahead) does not also cover the history and work-row stores of the step before (in_vgpr, ste_math.h).
    dt_n = in_vgpr(dt_n);
    sr_n = in_vgpr(sr_n);
    cr_n = in_vgpr(cr_n);
    ui_n = in_vgpr(ui_n);
    for (int k = 0; k < p.Nmax; ++k) {
        const bool live = k < ns;
        if (!__any(live)) break;
        if (live) {
            const double dt = dt_n, sr = sr_n, cr = cr_n;
            const int ui = ui_n;
            // Unconditional loads with clamped indices: a load inside an `if` makes hipcc drain the queue with
            // s_waitcnt vmcnt(0) where the branch rejoins.  The observation row of a step without an update is row 0
            // (cache-resident); the inputs of step k + 1 stay in flight during this step's arithmetic.
            const bool ui_ok = ui < p.Tmax;  // an observation column past the padded batch: flagged, update skipped
            const bool upd = ui >= 0 && ui_ok;
            double zk[4];
            load_vec(p.z, (size_t)(upd ? ui : 0), B, t, zk);
            {
                const size_t o = (size_t)(k + 1 < ns ? k + 1 : k) * B + t;
                dt_n = p.dt[o];
                sr_n = p.sog_rate[o];
                cr_n = p.cog_rate[o];
                ui_n = p.upd_idx[o];
            }
            // row 0's smoother rows were taken from the prior above; every later row k is the state this predict starts from
            double* work = (kGains && !(k == 0 && initial_update)) ? p.rts_work : nullptr;
            const bool warm = (k & (kColdEvery - 1)) != 0;
            if constexpr (kPlain) {
                // The observation and the inputs of step k + 1, loaded at the top of this step, are consumed in front of the
                // step's first store (some 2 000 instructions after the loads): a wait for them further down -- the update,
                // the loop edge -- would cover the work-row and history stores issued in between (DESIGN.md section 5,
                // "Store drain").  The general loop has such a wait in the same place, where recorded noise would be added.
                auto consume_loads = [&]() {
                    STE_UNROLL
                    for (int c = 0; c < 4; ++c) zk[c] = in_vgpr(zk[c]);
                    dt_n = in_vgpr(dt_n);
                    sr_n = in_vgpr(sr_n);
                    cr_n = in_vgpr(cr_n);
                    ui_n = in_vgpr(ui_n);
                };
                st |= lane_predict<kGains, kSched, true>(p.m, x, P, V, warm, dt, sr, cr, nullptr, nullptr, (size_t)k, B, t, work, upd,
                                                         false, flagged, first_bad, tk, Qv, consume_loads);
            } else {
                st |= lane_predict<kGains, kSched>(p.m, x, P, V, warm, dt, sr, cr, p.noise_pred, p.noise_rts, (size_t)k, B, t, work,
                                                   upd || noise_mode, noise_mode, flagged, first_bad, tk, Qv);
            }
            if constexpr (kLik != kLikOff) {
                UpdLik u;
                u.nis = __builtin_nan("");
                if (upd) {
                    st |= lane_update<kFastUpd, kRobust, true, kTrackNoise>(p.m, x, P, zk, p.noise_upd, (size_t)k + 1, B, t, &u, Rt);
                    lik_sum += update_loglik(u);
                    lik_dof += u.rank;
                    lik_nupd += 1;
                }
                if (lk->nis) st_stream(&lk->nis[((size_t)k + 1) * B + t], u.nis);
            } else {
                if (upd) st |= lane_update<kFastUpd, kRobust, false, kTrackNoise>(p.m, x, P, zk, noise_ptr<kPlain>(p.noise_upd), (size_t)k + 1, B, t, nullptr, Rt);
            }
            if (!ui_ok) st |= STE_STATUS_BAD_INDEX;
            if constexpr (kPlain)
                store_hist_packed(p, (size_t)k + 1, B, t, x, P);
            else if (kLik != kLikOnly) store_hist(p, (size_t)k + 1, B, t, x, P);
        }
    }
    double chk = 0.0;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) chk += x[c] * 0.0;
    STE_UNROLL
    for (int e = 0; e < 10; ++e) chk += P[e] * 0.0;
    if (!(chk == 0.0)) st |= STE_STATUS_NAN;  // inf*0 and nan*0 are NaN
    p.status[t] = st;
    if constexpr (kLik != kLikOff) {
        lk->loglik[t] = lik_sum;
        if (lk->dof) lk->dof[t] = lik_dof;
        if (lk->nupd) lk->nupd[t] = lik_nupd;
    }
}

template <bool kGains, bool kFastUpd, bool kRobust = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ukf_forward_l1(const KParams p) {
    forward_tile_l1<kGains, kFastUpd, kRobust, false>(p, (size_t)blockIdx.x * 64 + threadIdx.x);
}

// ukf_forward_l1<true, true, false> for a plain batch (forward_tile_l1: kPlain) -- the pass the benchmark, run_fleet and the
// CLI launch.  A kernel of its own name: the general kernels keep theirs, and their code.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ukf_forward_l1_plain(const KParams p) {
    forward_tile_l1<true, true, false, false, kLikOff, false, true>(p, (size_t)blockIdx.x * 64 + threadIdx.x);
}

// ukf_forward_l1 with the innovation log-likelihood (ste_ukf_forward_loglik_f64).  KParams stays the first argument (late_k0
// reads it at its own offset); the likelihood's outputs follow it.
template <bool kGains, bool kFastUpd, bool kRobust, int kLik>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ukf_forward_lik(const KParams p, const LikParams l) {
    forward_tile_l1<kGains, kFastUpd, kRobust, false, kLik>(p, (size_t)blockIdx.x * 64 + threadIdx.x, &l);
}

// The lane-per-track forward pass with per-track noise (ste_ukf_forward_noise_f64): the bodies of ukf_forward_l1 (kLikOff;
// `l` is not read) and ukf_forward_lik with the track's own Q / R.  KParams stays the first argument (late_k0).
template <bool kGains, bool kFastUpd, bool kRobust, int kLik>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ukf_forward_tn(const KParams p, const LikParams l,
                                                                                                 const NoiseParams nz) {
    forward_tile_l1<kGains, kFastUpd, kRobust, false, kLik, true>(p, (size_t)blockIdx.x * 64 + threadIdx.x, &l, &nz);
}

// ---------------------------------------------------------------------------------------------------------------
// The forward passes of MANY windows as one launch of resident waves working through a host-made schedule
// (ste_ukf_forward_sched_f64; DESIGN.md section 5, "Scheduled forward pass").
//
// A forward wave is indivisible for a whole pass (3.6-4.5 ms at 500 steps) when every window is a launch of its own: W
// windows of T tiles on S SIMDs then cost ceil(W T / S) pass times although they hold only W T / S pass times of work --
// the driver's 20 steps (3 140 tiles on 1 024 SIMDs) pay 4 generations for 3.07, a 100 000-track fleet 2 for 1.53.  Here the
// unit of work is a (tile, time slice) ITEM -- 64 tracks x one STE_SLICE_ALIGN-aligned step range, the slices of
// ste_ukf_forward_f64, bit-identical because a slice starts from the history row the previous one left -- and the launch
// is one wave per SIMD, each walking its own column of a [rounds][waves] item table.  Slices of one tile may run on
// different waves: a finished slice publishes the tile's slice count (release, agent scope: its history rows, work rows and
// status are in memory before the count moves) and the next slice acquires it.  The table comes from the host, which checks
// that every tile's slices appear in order, at most one per round -- so a wait only ever looks at an EARLIER round, and with
// all waves resident (the launch is sized to the SIMDs its stream may use) it is satisfied without spinning in the common
// case.  Every wait is bounded (s_memrealtime): a schedule that cannot progress raises the launch's error word and every
// wave leaves, instead of hanging the device.
// A window whose tiles have all finished their last slice bumps window_done[w]; smoothers wait for that count
// (ste_stream_wait_counter: a one-wave gate kernel on the smoother's stream).
// ---------------------------------------------------------------------------------------------------------------
struct SchedItem {
    int kp;    // index into the KParams table (one entry per (window, run of slices)), < 0: nothing to do this round
    int tile;  // 64-track tile of that window | slices of the tile done once this item has run << 24
    int prog;  // index of the tile's progress counter
    int meta;  // slice | last-slice flag << 8 | window << 9 (22 bits) | hand-over flags: bit 31 = the slice before this one ran
               // on ANOTHER wave (wait for the tile's count and acquire), bit 30 = the next slice runs on another wave, or there is
               // none (release and publish).  A tile that stays on its wave -- the rule -- needs neither: a wave sees its own stores.
};
struct SchedParams {
    const KParams* kps;
    const SchedItem* items;  // [nrounds][nwaves]
    int nrounds, nwaves;
    int* progress;     // [tiles of all windows] slices finished, zeroed before the launch
    int* window_done;  // [nwindows] tiles finished, zeroed before the launch
    int* error;        // one word, zeroed before the launch: 1 = a wait timed out (the schedule could not progress)
    unsigned long long timeout_ticks;  // bound of a single wait, in s_memrealtime ticks (100 MHz)
    int* started;      // optional, zeroed before the launch: waves that have begun (== nwaves: the launch is resident)
};

template <bool kGains, bool kFastUpd, bool kRobust>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ukf_forward_sched(const SchedParams sp) {
    typedef const KParams __attribute__((address_space(4))) ConstKParams;  // the table is constant for the launch: scalar loads,
                                                                           // re-materialised where they are used like kernel arguments
    if (sp.started && threadIdx.x == 0) __hip_atomic_fetch_add(sp.started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int r = 0; r < sp.nrounds; ++r) {
        const SchedItem* ip = sp.items + ((size_t)r * sp.nwaves + blockIdx.x);
        const int kp = __builtin_amdgcn_readfirstlane(ip->kp);
        if (kp < 0) continue;
        const int tile_word = __builtin_amdgcn_readfirstlane(ip->tile), prog = __builtin_amdgcn_readfirstlane(ip->prog);
        const int tile = tile_word & 0xffffff, publish = (tile_word >> 24) & 0xff;  // publish: slices done once this item has run
        const int meta = __builtin_amdgcn_readfirstlane(ip->meta);
        const int slice = meta & 0xff;
        // (the error word is looked at only where a wave waits: a launch that cannot progress ends through its bounded waits)
        if (meta < 0 && (__hip_atomic_load(sp.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ||
                         !sched_wait(sp.progress + prog, slice, sp.timeout_ticks))) {
            if (threadIdx.x == 0) __hip_atomic_store(sp.error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const KParams& p = *(const KParams*)(ConstKParams*)(uintptr_t)(sp.kps + kp);
        if (threadIdx.x == 0) *(volatile int*)&g_sched_word[0] = p.k0;
        forward_tile_l1<kGains, kFastUpd, kRobust, true>(p, (size_t)tile * 64 + threadIdx.x);
        if (meta & 0x40000000) {
            // publish: this wave's stores have been acknowledged, then made visible at agent scope, before the count moves
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (threadIdx.x == 0) {
                __hip_atomic_store(sp.progress + prog, publish, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (meta & 0x100)
                    __hip_atomic_fetch_add(sp.window_done + ((meta >> 9) & 0x1fffff), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
// ukf_forward_sched<true, true, false> when every parameter block of the table is a plain batch's (ukf_forward_l1_plain).  The
// wave loop is ukf_forward_sched's, line for line, repeated here and not shared through a device function: the general kernels
// keep their code to the byte that way (as a function of two callers the loop compiled to other scalar registers).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void ukf_forward_sched_plain(const SchedParams sp) {
    typedef const KParams __attribute__((address_space(4))) ConstKParams;  // the table is constant for the launch: scalar loads,
                                                                           // re-materialised where they are used like kernel arguments
    if (sp.started && threadIdx.x == 0) __hip_atomic_fetch_add(sp.started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int r = 0; r < sp.nrounds; ++r) {
        const SchedItem* ip = sp.items + ((size_t)r * sp.nwaves + blockIdx.x);
        const int kp = __builtin_amdgcn_readfirstlane(ip->kp);
        if (kp < 0) continue;
        const int tile_word = __builtin_amdgcn_readfirstlane(ip->tile), prog = __builtin_amdgcn_readfirstlane(ip->prog);
        const int tile = tile_word & 0xffffff, publish = (tile_word >> 24) & 0xff;  // publish: slices done once this item has run
        const int meta = __builtin_amdgcn_readfirstlane(ip->meta);
        const int slice = meta & 0xff;
        // (the error word is looked at only where a wave waits: a launch that cannot progress ends through its bounded waits)
        if (meta < 0 && (__hip_atomic_load(sp.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ||
                         !sched_wait(sp.progress + prog, slice, sp.timeout_ticks))) {
            if (threadIdx.x == 0) __hip_atomic_store(sp.error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const KParams& p = *(const KParams*)(ConstKParams*)(uintptr_t)(sp.kps + kp);
        if (threadIdx.x == 0) *(volatile int*)&g_sched_word[0] = p.k0;
        forward_tile_l1<true, true, false, true, kLikOff, false, true>(p, (size_t)tile * 64 + threadIdx.x);
        if (meta & 0x40000000) {
            // publish: this wave's stores have been acknowledged, then made visible at agent scope, before the count moves
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (threadIdx.x == 0) {
                __hip_atomic_store(sp.progress + prog, publish, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (meta & 0x100)
                    __hip_atomic_fetch_add(sp.window_done + ((meta >> 9) & 0x1fffff), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// Table upload of a scheduled launch as a kernel on the launch's own stream: copies `ncopy` 16-byte words from page-locked host
// memory (read over the host link) into the device workspace and clears the `nzero` words behind them (the progress counters).
// Nothing but kernels of this stream between two launches: no copy-engine transfer (an engine, and a queue, shared with
// whatever else the node is doing) in front of every scheduled launch.
__global__ __launch_bounds__(256) void sched_upload(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t ncopy, size_t nzero) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncopy + nzero; i += stride)
        dst[i] = i < ncopy ? src[i] : make_uint4(0, 0, 0, 0);
}

// One wave that leaves when *counter >= need (or after the bound, raising *error): what a smoother's stream runs in front of
// the smoother of a window whose forward pass is part of a scheduled launch on another stream.
__global__ __launch_bounds__(64) void sched_gate(const int* counter, int need, int* error, unsigned long long timeout_ticks) {
    if (!sched_wait(counter, need, timeout_ticks) && threadIdx.x == 0 && error)
        __hip_atomic_store(error, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


// ---------------------------------------------------------------------------------------------------------------
// URTSS backward pass, one lane per track (unscented.py:285-351)
// ---------------------------------------------------------------------------------------------------------------
// The literal smoother: recomputes the fan, its nine great-circle steps and both pseudo-inverses per step.  Used when
// there are no work rows from the forward pass (rts_work == NULL, a history that ste_ukf_forward_f64 did not write).
// kTrackNoise: track t's own Q (ste_urtss_backward_noise_f64), nz.Q[tix(r, c) * ld + t], instead of the shared p.m.Q.  nz.Q is
// not NULL there (launch_backward takes <false> without a per-track Q), and <false> never reads nz.  The body stays in the
// kernel: moved into an inline function it is optimised before it meets the kernel's arguments and comes out differently.
template <bool kTrackNoise>
__global__ __launch_bounds__(64) void urtss_backward_l1(const KParams p, const NoiseParams nz) {
    const size_t B = (size_t)p.ld;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    auto track_Q = [&](int r, int c) -> double {  // entry (r, c) of this track's process noise, loaded where it is used
        if constexpr (kTrackNoise)
            return nz.Q[(size_t)tix(r, c) * B + t];
        else
            return p.m.Q[r * 4 + c];
    };
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
                for (int c = 0; c < 4; ++c) Pb[r][c] += track_Q(r, c);
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
}

// ---------------------------------------------------------------------------------------------------------------
// single-function kernels (fine-grained API parity: geodetic_dynamics, compute_sigma_points)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void geodetic_kernel(size_t count, const double* x, const double* dt,
                                                      const double* sr, const double* cr, double* out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double xi[4], o[4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xi[c] = x[c * count + i];
    geodetic_step(xi, dt[i], sr[i], cr[i], o);
    STE_UNROLL
    for (int c = 0; c < 4; ++c) out[c * count + i] = o[c];
}

__global__ __launch_bounds__(64) void sigma_points_kernel(size_t count, const double* x, const double* P,
                                                          double scale, double* out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double xi[4], Pi[4][4], sig[9][4];
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xi[c] = x[c * count + i];
    load_mat(P, 0, count, i, Pi);
    sigma_fan(xi, Pi, scale, sig);
    STE_UNROLL
    for (int j = 0; j < 9; ++j) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) out[((size_t)j * 4 + c) * count + i] = sig[j][c];
    }
}

// Sigma fan for a general state dimension n <= kMaxGenericN (unscented.py:76-107 accepts any n; the reference's own
// unit tests use n = 2).  Not a hot path: one lane per matrix, run-time loops, arrays in scratch.
constexpr int kMaxGenericN = 16;
__global__ __launch_bounds__(64) void sigma_points_generic_kernel(int n, size_t count, const double* x,
                                                                  const double* P, double scale, double* out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double A[kMaxGenericN][kMaxGenericN], V[kMaxGenericN][kMaxGenericN];
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            A[r][c] = scale * 0.5 * (P[((size_t)r * n + c) * count + i] + P[((size_t)c * n + r) * count + i]);
            V[r][c] = (r == c) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (!(apq * apq > kRotTol2 * fabs(app * aqq))) continue;
                rotated = true;
                const double delta = aqq - app;
                double t = 2.0 * apq / (fabs(delta) + sqrt(delta * delta + 4.0 * apq * apq));
                t = delta < 0.0 ? -t : t;
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                for (int r = 0; r < n; ++r) {  // columns p, q
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = c * arp - s * arq;
                    A[r][q] = s * arp + c * arq;
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
                for (int r = 0; r < n; ++r) {  // rows p, q
                    const double apr = A[p][r], aqr = A[q][r];
                    A[p][r] = c * apr - s * aqr;
                    A[q][r] = s * apr + c * aqr;
                }
                A[p][q] = 0.0;
                A[q][p] = 0.0;
            }
        if (!rotated) break;
    }
    const size_t m = 2 * (size_t)n + 1;
    for (int c = 0; c < n; ++c) out[((size_t)0 * n + c) * count + i] = x[(size_t)c * count + i];
    for (int col = 0; col < n; ++col)
        for (int r = 0; r < n; ++r) {
            double t = 0.0;  // T[r][col] = sum_l V[r][l] sqrt(max(w_l,0)) V[col][l]
            for (int l = 0; l < n; ++l) t += V[r][l] * sqrt(fmax(A[l][l], 0.0)) * V[col][l];
            const double xr = x[(size_t)r * count + i];
            out[((size_t)(1 + col) * n + r) * count + i] = xr + t;
            out[((size_t)(1 + n + col) * n + r) * count + i] = xr - t;
        }
    (void)m;
}

// One predict (unscented.py:144-207) / one update (:209-265) on `count` independent (x, P) pairs.
__global__ __launch_bounds__(64) void predict_kernel(size_t count, const Mats m, const double* x, const double* P,
                                                     const double* dt, const double* sr, const double* cr,
                                                     const double* noise, double* x_out, double* P_out,
                                                     int32_t* status) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double xi[4], Pi[4][4];
    load_vec(x, 0, count, i, xi);
    load_mat(P, 0, count, i, Pi);
    // the inputs too: the Jacobi sweeps skip a rotation whose pivot is NaN, so a NaN in an off-diagonal entry of P alone can
    // leave the eigenvalues, and with them every output, finite
    const bool in_ok = all_finite(xi, Pi);
    int st = ukf_predict(m, xi, Pi, dt[i], sr[i], cr[i], noise, 0, count, i);
    if (!in_ok || !all_finite(xi, Pi)) st |= STE_STATUS_NAN;
    store_vec(x_out, 0, count, i, xi);
    store_mat(P_out, 0, count, i, Pi);
    if (status) status[i] = st;
}

__global__ __launch_bounds__(64) void update_kernel(size_t count, const Mats m, const double* x, const double* P,
                                                    const double* z, const double* noise, double* x_out,
                                                    double* P_out, int32_t* status) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double xi[4], Pi[4][4], zi[4];
    load_vec(x, 0, count, i, xi);
    load_mat(P, 0, count, i, Pi);
    load_vec(z, 0, count, i, zi);
    int st = ukf_update(m, xi, Pi, zi, noise, 0, count, i);
    if (!all_finite(xi, Pi)) st |= STE_STATUS_NAN;
    store_vec(x_out, 0, count, i, xi);
    store_mat(P_out, 0, count, i, Pi);
    if (status) status[i] = st;
}

// Robustification terms for `count` independent (x, P, z) triples (criterion_index / update_lambda_factor).
__global__ __launch_bounds__(64) void robust_terms_kernel(size_t count, const Mats m, const double* x, const double* P,
                                                          const double* z, double* gamma, double* denom) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double H[4][4], R[4][4], xi[4], Pi[4][4], zi[4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            H[r][c] = m.H[r * 4 + c];
            R[r][c] = m.R[r * 4 + c];
        }
    }
    load_vec(x, 0, count, i, xi);
    load_mat(P, 0, count, i, Pi);
    load_vec(z, 0, count, i, zi);
    double g, d;
    robust_terms(H, R, xi, Pi, zi, g, d);
    gamma[i] = g;
    denom[i] = d;
}

}  // namespace ste

// ===============================================================================================================
// C ABI
// ===============================================================================================================
namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return STE_OK;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return STE_ELAUNCH;
}
}  // namespace

// ste_err.h: the same error string for the other translation units of this ABI (ste_prep.hip)
int ste::abi_fail(int code, const char* msg) { return fail(code, "%s", msg); }
int ste::abi_check_hip(hipError_t e, const char* what) { return check_hip(e, what); }

namespace {

// H selects lon / lat: H = diag(1, 1, 0, 0), what the closed-form update needs of it
static bool selects_lon_lat(const double* H) {
    bool sel = true;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) sel = sel && H[r * 4 + c] == ((r == c && r < 2) ? 1.0 : 0.0);
    return sel;
}

int make_params(const ste_ukf_batch_f64* b, bool need_sm_out, ste::KParams* kp, bool need_hist = true) {
    if (!b) return fail(STE_EINVAL, "batch pointer is NULL");
    if (b->n != 4) return fail(STE_EINVAL, "state dimension n must be 4 (heading index 3 is hard-wired, unscented.py:250)");
    if (b->B <= 0) return fail(STE_EINVAL, "B must be > 0");
    if (b->Nmax < 0) return fail(STE_EINVAL, "Nmax must be >= 0");
    if (b->Tmax < 1) return fail(STE_EINVAL, "Tmax must be >= 1");
    if (!b->H || !b->Q || !b->R) return fail(STE_EINVAL, "H, Q and R (host 4x4) are required");
    if (!b->x0 || !b->P0) return fail(STE_EINVAL, "x0 and P0 are required");
    if (b->Nmax > 0 && (!b->dt || !b->sog_rate || !b->cog_rate || !b->upd_idx))
        return fail(STE_EINVAL, "dt, sog_rate, cog_rate and upd_idx are required when Nmax > 0");
    if (!b->z) return fail(STE_EINVAL, "z is required");
    if (need_hist && (!b->fwd_mean || !b->fwd_cov)) return fail(STE_EINVAL, "fwd_mean, fwd_cov and status are required");
    if (!b->status) return fail(STE_EINVAL, "fwd_mean, fwd_cov and status are required");
    if (need_sm_out && (!b->sm_mean || !b->sm_cov)) return fail(STE_EINVAL, "sm_mean and sm_cov are required");
    kp->B = b->B;
    kp->Nmax = b->Nmax;
    kp->Tmax = b->Tmax;
    if ((b->flags & STE_FLAG_LANES_1) && (b->flags & STE_FLAG_LANES_4))
        return fail(STE_EINVAL, "STE_FLAG_LANES_1 and STE_FLAG_LANES_4 exclude each other");
    kp->flags = b->flags;
    kp->tuning = b->tuning;
    kp->m.fan_scale = b->fan_scale;
    kp->m.w0 = b->w0;
    kp->m.wi = b->wi;
    memcpy(kp->m.H, b->H, sizeof(double) * 16);
    memcpy(kp->m.Q, b->Q, sizeof(double) * 16);
    memcpy(kp->m.R, b->R, sizeof(double) * 16);
    kp->m.chi_alpha = b->chi_alpha;
    kp->m.robust_iters = (b->flags & STE_FLAG_ROBUST) ? (b->robust_max_iter > 0 ? b->robust_max_iter : 50) : 0;
    // The sigma weights sum to one for every weight0 the reference accepts (unscented.py:125-132: wi = (1 - w0) / 2n);
    // the streamed moments of the forward kernels rely on it.
    if (!(fabs(b->w0 + 8.0 * b->wi - 1.0) <= 1e-14))
        return fail(STE_EINVAL, "sigma weights must sum to one: w0 + 2 n wi = 1 (unscented.py:125-132)");
    {
        bool sel = selects_lon_lat(b->H);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c)
                if (r >= 2 || c >= 2) sel = sel && b->R[r * 4 + c] == 0.0;
        kp->fast_upd = sel && b->R[1] == b->R[4];
    }
    kp->nsteps = b->nsteps;
    kp->x0 = b->x0;
    kp->P0 = b->P0;
    kp->dt = b->dt;
    kp->sog_rate = b->sog_rate;
    kp->cog_rate = b->cog_rate;
    kp->sog_rate_rts = b->sog_rate_rts;
    kp->cog_rate_rts = b->cog_rate_rts;
    kp->upd_idx = b->upd_idx;
    kp->z = b->z;
    kp->noise_pred = b->noise_pred;
    kp->noise_upd = b->noise_upd;
    kp->noise_rts = b->noise_rts;
    kp->fwd_mean = b->fwd_mean;
    kp->fwd_cov = b->fwd_cov;
    kp->sm_mean = b->sm_mean;
    kp->sm_cov = b->sm_cov;
    kp->status = b->status;
    // the forward pass leaves the smoother's rows (see kWorkD)
    // (smoother rates of its own only move x_b and P_b by a known amount: load_recur_row)
    kp->rts_work = b->rts_work;
    if (b->track_stride != 0 && (b->track_stride < b->B || b->track_stride > 0x7fffffff))
        return fail(STE_EINVAL, "track_stride must be 0 (= B) or in [B, 2^31): a window lies inside the rows of its fleet");
    kp->ld = b->track_stride ? (int)b->track_stride : b->B;
    kp->k0 = 0;
    kp->qpw = 16;
    kp->first_bad = b->rts_work ? b->rts_work + (size_t)b->Nmax * STE_RTS_WORK_ROWS * (size_t)kp->ld : nullptr;
    kp->sm_pos = b->sm_pos;
    return STE_OK;
}

// The forward pass in time slices (ste.h: step_begin / step_end).  A slice that starts at step k0 > 0 is the same kernel
// started from history row k0: x0 / P0 point at that row, every per-step array at its row k0, the histories and work
// rows likewise, the initial update is off and Nmax is the slice's length.  Slice boundaries are multiples of
// STE_SLICE_ALIGN = kColdEvery, the steps at which the eigenvector basis of the fan's square root restarts from the
// identity in a whole pass too -- so the history row is the complete state and the slices reproduce the whole pass bit
// for bit.  (The quad mapping keeps both triangles of P in its lanes and a packed history holds one: slices of that
// combination are refused.)
static_assert(STE_SLICE_ALIGN == ste::kColdEvery, "include/ste.h: STE_SLICE_ALIGN");
int slice_params(const ste_ukf_batch_f64* b, ste::KParams* kp) {
    const int k0 = b->step_begin, k1 = b->step_end ? b->step_end : b->Nmax;
    if (k0 < 0 || k1 > b->Nmax || k0 > k1 || (k0 == k1 && b->Nmax > 0))
        return fail(STE_EINVAL, "time slice: need 0 <= step_begin < step_end <= Nmax (step_end 0 = Nmax)");
    if (k0 % STE_SLICE_ALIGN != 0 || (k1 != b->Nmax && k1 % STE_SLICE_ALIGN != 0))
        return fail(STE_EINVAL, "time slice: step_begin and step_end must be multiples of STE_SLICE_ALIGN (64) or the ends of the pass");
    if (k0 == 0 && k1 == b->Nmax) return STE_OK;
    const bool packed = (b->flags & STE_FLAG_PACKED_COV) != 0;
    if (packed && ste::choose_lanes(kp->B, kp->flags) == 4)
        return fail(STE_EINVAL, "time slices with packed covariances need the lane-per-track mapping (STE_FLAG_LANES_1)");
    const size_t ld = (size_t)kp->ld, r0 = (size_t)k0;
    kp->Nmax = k1 - k0;
    kp->k0 = k0;
    if (k0 > 0) {
        kp->flags = (kp->flags | ste::kFlagContinue | STE_FLAG_NO_INITIAL_UPDATE) & ~STE_FLAG_SHARED_P0;
        kp->x0 = b->fwd_mean + r0 * 4 * ld;
        kp->P0 = b->fwd_cov + r0 * (packed ? 10 : 16) * ld;
        kp->dt += r0 * ld;
        kp->sog_rate += r0 * ld;
        kp->cog_rate += r0 * ld;
        kp->upd_idx += r0 * ld;
        if (kp->noise_pred) kp->noise_pred += r0 * 4 * ld;
        if (kp->noise_upd) kp->noise_upd += r0 * 4 * ld;  // row k + 1 belongs to the update after step k
        if (kp->noise_rts) kp->noise_rts += r0 * 4 * ld;
        kp->fwd_mean += r0 * 4 * ld;
        kp->fwd_cov += r0 * (packed ? 10 : 16) * ld;
        if (kp->rts_work) kp->rts_work += r0 * STE_RTS_WORK_ROWS * ld;
    }
    return STE_OK;
}

// The instantiations of the lane-per-track forward kernels, in one place: kGains (the smoother's work rows) is free, and
// (kFastUpd, kRobust) is (0, 0), (1, 0) or (1, 1) -- robust rescaling without the closed-form update runs the
// <..., false, false> kernel, whose general update reads robust_iters itself.  `f` gets the three as std::bool_constants.
template <class F>
auto with_forward_variant(const ste::KParams& kp, F&& f) {
    return ste::with_bool(kp.rts_work != nullptr, [&](auto gains) {
        if (kp.fast_upd && kp.m.robust_iters > 0) return f(gains, std::true_type{}, std::true_type{});
        if (kp.fast_upd) return f(gains, std::true_type{}, std::false_type{});
        return f(gains, std::false_type{}, std::false_type{});
    });
}
// ... as a number: do two batches take the same instantiation?
int forward_variant(const ste::KParams& kp) {
    return with_forward_variant(kp, [](auto gains, auto fast, auto robust) { return gains() | fast() << 1 | robust() << 2; });
}

// Every forward launch but the scheduled one.  `lp`: with the innovation log-likelihood (lane per track, whole passes: the
// entry points check); with histories the kernel is the plain pass's, plus the likelihood, without them kLikOnly.  `np`:
// per-track noise.  Both NULL: the plain pass, quad or lane per track.  `fn`: the entry point, for the message.
int launch_forward(const char* fn, const ste::KParams& kp, const ste::LikParams* lp, const ste::NoiseParams* np, hipStream_t s) {
    if (ste::choose_lanes(kp.B, kp.flags) == 4)  // (never with lp or np: their entry points set STE_FLAG_LANES_1)
        return ste::launch_forward_q4(kp, s);
    const bool hist = kp.fwd_mean != nullptr;  // (missing only with a likelihood: make_params)
    if (!hist && kp.rts_work) return fail(STE_EINVAL, "%s: rts_work needs the histories", fn);
    const dim3 grid((unsigned)((kp.B + 63) / 64)), block(64);
    const ste::LikParams l0 = lp ? *lp : ste::LikParams{nullptr, nullptr, nullptr, nullptr};
    with_forward_variant(kp, [&](auto gains, auto fast, auto robust) {
        constexpr bool kG = decltype(gains)::value, kF = decltype(fast)::value, kR = decltype(robust)::value;
        auto launch = [&](auto lik) {
            constexpr int kLik = decltype(lik)::value;
            if (np)
                hipLaunchKernelGGL((ste::ukf_forward_tn<kG, kF, kR, kLik>), grid, block, 0, s, kp, l0, *np);
            else if constexpr (kLik != ste::kLikOff)
                hipLaunchKernelGGL((ste::ukf_forward_lik<kG, kF, kR, kLik>), grid, block, 0, s, kp, l0);
            else if (kG && kF && !kR && ste::plain_batch(kp))
                hipLaunchKernelGGL(ste::ukf_forward_l1_plain, grid, block, 0, s, kp);
            else
                hipLaunchKernelGGL((ste::ukf_forward_l1<kG, kF, kR>), grid, block, 0, s, kp);
        };
        if (!lp)
            launch(std::integral_constant<int, ste::kLikOff>{});
        else if (hist)
            launch(std::integral_constant<int, ste::kLikHist>{});
        else if constexpr (!kG)  // (no histories, no work rows: refused above)
            launch(std::integral_constant<int, ste::kLikOnly>{});
    });
    return check_hip(hipGetLastError(), np ? "ukf_forward_tn launch" : lp ? "ukf_forward_lik launch" : "ukf_forward launch");
}

// `np`: per-track noise, or NULL.  With the forward pass's work rows: the smoothers of ste_smooth.hip; without them the
// stand-alone smoother, which reads Q alone and takes the shared instantiation without a per-track Q.
int launch_backward(const ste::KParams& kp, const ste::NoiseParams* np, hipStream_t s) {
    if (kp.rts_work) return ste::launch_backward_work(kp, np, s);
    const dim3 grid((unsigned)((kp.B + 63) / 64)), block(64);
    const bool tn = np && np->Q;
    const ste::NoiseParams nz = tn ? *np : ste::NoiseParams{nullptr, nullptr};
    ste::with_bool(tn, [&](auto t) { hipLaunchKernelGGL(ste::urtss_backward_l1<decltype(t)::value>, grid, block, 0, s, kp, nz); });
    return check_hip(hipGetLastError(), "urtss_backward launch");
}

// ---- per-track noise (ste_ukf_noise_f64) -----------------------------------------------------------------------------
// The checks the three *_noise entry points share, and the route: with a per-track R the closed-form update is the caller's
// promise (STE_NOISE_R_BLOCK2) instead of a look at b->R -- the library cannot read device memory before a launch.
int noise_params(const char* fn, const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, ste::NoiseParams* np) {
    if (!b) return fail(STE_EINVAL, "batch pointer is NULL");
    if (!nz) return fail(STE_EINVAL, "%s: the per-track noise (nz) is NULL", fn);
    if (!nz->Q && !nz->R)
        return fail(STE_EINVAL, "%s: nz->Q and nz->R are both NULL: that is the plain call (without the _noise suffix)", fn);
    if (nz->flags & ~(uint32_t)STE_NOISE_R_BLOCK2) return fail(STE_EINVAL, "%s: unknown bits in nz->flags", fn);
    if (b->flags & STE_FLAG_LANES_4)
        return fail(STE_EINVAL, "%s: the quad forward kernel has no per-track noise: STE_FLAG_LANES_4 is refused", fn);
    np->Q = nz->Q;
    np->R = nz->R;
    return STE_OK;
}
void noise_route(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, ste::KParams* kp) {
    kp->flags |= STE_FLAG_LANES_1;
    if (!nz->R) return;  // shared R: make_params has looked at it
    kp->fast_upd = selects_lon_lat(b->H) && (nz->flags & STE_NOISE_R_BLOCK2) != 0;
}

// "whole passes only", for the entry point `fn`; `why`: what stands in the way of time slices, or where they go instead
int whole_passes(const char* fn, const ste_ukf_batch_f64* b, const char* why) {
    if (b->step_begin == 0 && (b->step_end == 0 || b->step_end == b->Nmax)) return STE_OK;
    snprintf(g_err, sizeof(g_err), "%s runs whole passes: %s", fn, why);
    return STE_EINVAL;
}

// What a forward pass with the innovation log-likelihood asks of its arguments, before make_params (b is not NULL).  `hist`:
// the pass writes its histories too.  The likelihood kernels are lane per track (ste_ukf_forward_noise_f64 has refused the
// quad mapping before it comes here, in words of its own).
int lik_params(const char* fn, const ste_ukf_batch_f64* b, const ste_ukf_loglik_f64* l, ste::LikParams* lp, bool* hist) {
    if (!l) return fail(STE_EINVAL, "%s: the likelihood outputs (l) are NULL", fn);
    if (!l->loglik) return fail(STE_EINVAL, "%s: l->loglik is required", fn);
    *hist = b->fwd_mean != nullptr;
    if (*hist != (b->fwd_cov != nullptr))
        return fail(STE_EINVAL, "%s: fwd_mean and fwd_cov go together: both (histories) or neither (the likelihood alone)", fn);
    if (!*hist && b->rts_work)
        return fail(STE_EINVAL, "%s: rts_work needs the histories (the smoother reads both); pass fwd_mean and fwd_cov, or no "
                                "rts_work", fn);
    if (b->flags & STE_FLAG_LANES_4)
        return fail(STE_EINVAL, "%s runs the lane-per-track mapping only: STE_FLAG_LANES_4 is refused", fn);
    *lp = {l->loglik, l->dof, l->nupd, l->nis};
    return whole_passes(fn, b, "the likelihood sums over every update, so time slices (step_begin / step_end) are refused");
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct SchedLayout {
    size_t kps, items, progress, total;  // byte offsets into the workspace (kps and items are uploaded, progress is zeroed)
};
SchedLayout sched_layout(size_t nkp, size_t nitems, size_t ntiles) {
    SchedLayout l;
    l.kps = 0;
    l.items = align16(nkp * sizeof(ste::KParams));
    l.progress = l.items + align16(nitems * sizeof(ste::SchedItem));
    l.total = l.progress + align16(ntiles * sizeof(int));
    return l;
}
// THE layout of a scheduled forward launch's workspace: the launch, ste_ukf_forward_sched_workspace and
// ste_ukf_forward_sched_progress_offset all come here, so the per-tile counters sit where a caller is told to look for them
// whatever the mix of window lengths.  The parameter-block region is sized by the bound a caller can compute without the
// windows -- max_slices (max_slices + 1) / 2 runs of consecutive slices for each of nwindows -- not by what the windows at hand
// need (the launch packs theirs at the front of it).
SchedLayout sched_layout_for(size_t nwindows, size_t max_slices, size_t ntiles, size_t nrounds, size_t nwaves) {
    return sched_layout(nwindows * (max_slices * (max_slices + 1) / 2), nrounds * nwaves, ntiles);
}

// `ncopy` bytes of a schedule's table from the caller's host workspace into the device workspace and `nzero` zero bytes behind
// them (multiples of 16).  Page-locked host memory: a kernel on `s` reads it in place (no copy engine between two launches);
// anything else: a staged copy.
int upload_table(char* dw, const char* hw, size_t ncopy, size_t nzero, hipStream_t s, const char* what) {
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    const bool locked = hipPointerGetAttributes(&attr, hw) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer &&
                        ((uintptr_t)attr.devicePointer & 15) == 0 && ((uintptr_t)dw & 15) == 0;
    if (locked) {
        const size_t nwords = (ncopy + nzero) / 16;
        const unsigned blocks = (unsigned)std::min<size_t>(256, (nwords + 255) / 256);
        hipLaunchKernelGGL(ste::sched_upload, dim3(blocks), dim3(256), 0, s, (uint4*)dw, (const uint4*)attr.devicePointer, ncopy / 16,
                           nzero / 16);
        return check_hip(hipGetLastError(), what);
    }
    (void)hipGetLastError();  // (the attribute query of pageable memory reports an error: not this call's)
    int rc = check_hip(hipMemcpyAsync(dw, hw, ncopy, hipMemcpyHostToDevice, s), what);
    if (rc || !nzero) return rc;
    return check_hip(hipMemsetAsync(dw + ncopy, 0, nzero, s), what);
}

}  // namespace

extern "C" {

int ste_version(void) { return STE_VERSION; }

#ifdef STE_DEBUG_SWEEPS
int ste_dbg_counters(unsigned long long* out, int reset) {  // developer instrumentation, not part of the ABI
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(ste::g_dbg), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[64] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(ste::g_dbg), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

const char* ste_last_error(void) { return g_err; }

int ste_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ste_stream_create_cu_range(int32_t first_cu, int32_t num_cus, void** stream) {
    if (!stream) return fail(STE_EINVAL, "stream out-pointer is NULL");
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return fail(STE_ENOGPU, "no HIP device");
    const int ncu = prop.multiProcessorCount;
    if (first_cu < 0 || num_cus < 1 || first_cu + num_cus > ncu)
        return fail(STE_EINVAL, "CU range must lie inside [0, multiProcessorCount)");
    uint32_t mask[32];
    memset(mask, 0, sizeof(mask));
    const int words = (ncu + 31) / 32;
    if (words > 32) return fail(STE_EINVAL, "device has more than 1024 CUs");
    for (int i = first_cu; i < first_cu + num_cus; ++i) mask[i / 32] |= 1u << (i % 32);
    hipStream_t s = nullptr;
    int rc = check_hip(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask), "hipExtStreamCreateWithCUMask");
    if (rc) return rc;
    *stream = (void*)s;
    return STE_OK;
}

int ste_stream_destroy(void* stream) {
    if (!stream) return STE_OK;
    return check_hip(hipStreamDestroy((hipStream_t)stream), "hipStreamDestroy");
}

int ste_ukf_forward_f64(const ste_ukf_batch_f64* b, void* stream) {
    ste::KParams kp;
    int rc = make_params(b, false, &kp);
    if (rc) return rc;
    rc = slice_params(b, &kp);
    if (rc) return rc;
    return launch_forward("ste_ukf_forward_f64", kp, nullptr, nullptr, (hipStream_t)stream);
}

int ste_ukf_forward_loglik_f64(const ste_ukf_batch_f64* b, const ste_ukf_loglik_f64* l, void* stream) {
    const char* fn = "ste_ukf_forward_loglik_f64";
    if (!b) return fail(STE_EINVAL, "batch pointer is NULL");
    ste::LikParams lp;
    bool hist;
    int rc = lik_params(fn, b, l, &lp, &hist);
    if (rc) return rc;
    ste::KParams kp;
    rc = make_params(b, false, &kp, hist);
    if (rc) return rc;
    kp.flags |= STE_FLAG_LANES_1;
    return launch_forward(fn, kp, &lp, nullptr, (hipStream_t)stream);
}

size_t ste_ukf_forward_sched_workspace(int32_t nwindows, int32_t max_slices, int64_t ntiles_total, int32_t nrounds,
                                       int32_t nwaves) {
    if (nwindows < 0 || max_slices < 0 || ntiles_total < 0 || nrounds < 0 || nwaves < 0) return 0;
    // a parameter block per (window, run of consecutive slices): max_slices (max_slices + 1) / 2 of them per window
    return sched_layout_for((size_t)nwindows, (size_t)max_slices, (size_t)ntiles_total, (size_t)nrounds, (size_t)nwaves).total;
}

int ste_ukf_forward_sched_f64(const ste_fwd_sched_f64* sc, void* stream) {
    if (!sc) return fail(STE_EINVAL, "schedule pointer is NULL");
    if (sc->nwindows < 1 || !sc->windows) return fail(STE_EINVAL, "scheduled forward pass: nwindows >= 1 and windows are required");
    if (sc->nwaves < 1 || sc->nrounds < 1 || !sc->items) return fail(STE_EINVAL, "scheduled forward pass: nwaves, nrounds >= 1 and items are required");
    if (!sc->host_ws || !sc->dev_ws || !sc->window_done || !sc->error)
        return fail(STE_EINVAL, "scheduled forward pass: host_ws, dev_ws, window_done and error are required");
    const int step = sc->slice_steps ? sc->slice_steps : STE_SLICE_ALIGN;
    if (step < STE_SLICE_ALIGN || step % STE_SLICE_ALIGN != 0)
        return fail(STE_EINVAL, "scheduled forward pass: slice_steps must be a positive multiple of STE_SLICE_ALIGN (64)");
    if (sc->nwindows >= (1 << 21)) return fail(STE_EINVAL, "scheduled forward pass: too many windows");
    // per window: slices, tiles, and where its KParams and progress counters start
    std::vector<int> nslices((size_t)sc->nwindows), kp0((size_t)sc->nwindows), tile0((size_t)sc->nwindows + 1);
    size_t nkp = 0, ntiles = 0;
    int max_slices = 0;
    for (int w = 0; w < sc->nwindows; ++w) {
        const ste_ukf_batch_f64& b = sc->windows[w];
        if (b.B <= 0 || b.Nmax < 0) return fail(STE_EINVAL, "scheduled forward pass: a window has B <= 0 or Nmax < 0");
        if (b.step_begin != 0 || b.step_end != 0) return fail(STE_EINVAL, "scheduled forward pass: windows must not carry a step range of their own");
        if (b.flags & STE_FLAG_LANES_4) return fail(STE_EINVAL, "scheduled forward pass: lane-per-track only (STE_FLAG_LANES_4 is set)");
        nslices[w] = std::max(1, (b.Nmax + step - 1) / step);
        if (nslices[w] > 255) return fail(STE_EINVAL, "scheduled forward pass: more than 255 time slices per window; raise slice_steps");
        max_slices = std::max(max_slices, nslices[w]);
        kp0[w] = (int)nkp;
        tile0[w] = (int)ntiles;
        nkp += (size_t)nslices[w] * ((size_t)nslices[w] + 1) / 2;  // one per run of slices [q0, q1], q0 <= q1
        ntiles += ((size_t)b.B + 63) / 64;
        if (ntiles > 0x7fffffff) return fail(STE_EINVAL, "scheduled forward pass: too many tiles");
    }
    tile0[sc->nwindows] = (int)ntiles;
    // the windows' blocks (nkp of them, packed by kp0) fill the front of a region sized for nwindows windows of max_slices
    // slices each: the item table and the counters behind it are where the two size functions say, for any mix of lengths
    const SchedLayout lay = sched_layout_for((size_t)sc->nwindows, (size_t)max_slices, ntiles, (size_t)sc->nrounds, (size_t)sc->nwaves);
    if (sc->ws_bytes < lay.total) return fail(STE_EINVAL, "scheduled forward pass: workspace too small (ste_ukf_forward_sched_workspace)");
    char* hw = (char*)sc->host_ws;
    ste::KParams* kps = (ste::KParams*)(hw + lay.kps);
    // parameter block of window w for the run of slices [q0, q1]: built when a (merged) item first needs it
    const ste::KParams* first = nullptr;  // the first block built: every other takes the same kernel
    bool all_plain = true;                // ... the plain one only if every block of the table is a plain batch's
    std::vector<char> have(nkp, 0);
    auto run_index = [&](int w, int q0, int q1) { return kp0[w] + q0 * nslices[w] - q0 * (q0 - 1) / 2 + (q1 - q0); };
    auto run_params = [&](int w, int q0, int q1, int* index) -> int {
        const int k = run_index(w, q0, q1);
        *index = k;
        if (have[(size_t)k]) return STE_OK;
        ste_ukf_batch_f64 b = sc->windows[w];
        b.flags |= STE_FLAG_LANES_1;
        b.step_begin = q0 * step;
        b.step_end = std::min(b.Nmax, (q1 + 1) * step);
        ste::KParams* kp = kps + k;
        int rc = make_params(&b, false, kp);
        if (rc) return rc;
        rc = slice_params(&b, kp);
        if (rc) return rc;
        if (first && forward_variant(*kp) != forward_variant(*first))
            return fail(STE_EINVAL, "scheduled forward pass: the windows must agree on H / R structure, robust flag and rts_work (one kernel runs them all)");
        if (!first) first = kp;
        all_plain = all_plain && ste::plain_batch(*kp);
        have[(size_t)k] = 1;
        return STE_OK;
    };
    // items: (window, tile) per (round, wave); the slice is the tile's number of earlier appearances.  Every tile must run
    // all its slices, in rounds that strictly increase.
    ste::SchedItem* items = (ste::SchedItem*)(hw + lay.items);
    std::vector<int> next_slice(ntiles, 0), last_round(ntiles, -1), last_wave(ntiles, -1);
    std::vector<size_t> last_item(ntiles, 0);
    for (int r = 0; r < sc->nrounds; ++r)
        for (int v = 0; v < sc->nwaves; ++v) {
            const size_t i = (size_t)r * sc->nwaves + v;
            const int w = sc->items[2 * i], tile = sc->items[2 * i + 1];
            ste::SchedItem it = {-1, 0, 0, 0};
            if (w >= 0) {
                if (w >= sc->nwindows) return fail(STE_EINVAL, "scheduled forward pass: an item names a window that does not exist");
                if (tile < 0 || tile >= tile0[w + 1] - tile0[w]) return fail(STE_EINVAL, "scheduled forward pass: an item names a tile outside its window");
                const int g = tile0[w] + tile, q = next_slice[g];
                if (q >= nslices[w]) return fail(STE_EINVAL, "scheduled forward pass: a tile is scheduled for more slices than it has");
                if (last_round[g] >= r) return fail(STE_EINVAL, "scheduled forward pass: two slices of one tile in the same round");
                it.kp = 0;  // (set below, once runs of slices are known)
                it.tile = tile;
                it.prog = g;
                it.meta = q | (q + 1 == nslices[w] ? 0x100 : 0) | (w << 9);
                if (q + 1 == nslices[w]) it.meta |= 0x40000000;  // the window's smoother reads what the last slice leaves
                if (q > 0 && last_wave[g] != v) {                 // the tile changes waves: hand over through memory
                    it.meta |= (int)0x80000000u;
                    items[last_item[g]].meta |= 0x40000000;
                }
                next_slice[g] = q + 1;
                last_round[g] = r;
                last_wave[g] = v;
                last_item[g] = i;
            }
            items[i] = it;
        }
    for (int w = 0; w < sc->nwindows; ++w)
        for (int g = tile0[w]; g < tile0[w + 1]; ++g)
            if (next_slice[g] != nslices[w]) return fail(STE_EINVAL, "scheduled forward pass: a tile is missing slices (every tile of every window must run all of them)");
    // Runs: consecutive slices of a tile that follow one another on the SAME wave, nothing in between, become one item over
    // the whole step range -- the step loop of a plain forward pass, with no state written out and read back at the slice
    // boundaries inside it (same bits: that is what a slice boundary is).  The run publishes the count of its last slice;
    // the rounds it swallows are idle entries of that wave's column.
    for (int v = 0; v < sc->nwaves; ++v)
        for (int r = 0; r < sc->nrounds;) {
            ste::SchedItem& head = items[(size_t)r * sc->nwaves + v];
            if (head.kp < 0) {
                ++r;
                continue;
            }
            const int w = (head.meta >> 9) & 0x1fffff, q0 = head.meta & 0xff;
            int q1 = q0, r2 = r + 1;
            while (r2 < sc->nrounds) {
                ste::SchedItem& nx = items[(size_t)r2 * sc->nwaves + v];
                if (nx.kp < 0 || nx.prog != head.prog || (nx.meta & 0xff) != q1 + 1 || nx.meta < 0) break;
                // the run keeps its first slice's number, window and acquire flag; last-slice and release flags are its last slice's
                head.meta = (head.meta & (int)(0xffu | (0x1fffffu << 9) | 0x80000000u)) | (nx.meta & 0x40000100);
                ++q1;
                nx.kp = -1;
                ++r2;
            }
            int k = 0;
            const int rc = run_params(w, q0, q1, &k);
            if (rc) return rc;
            head.kp = k;
            head.tile |= (q1 + 1) << 24;  // the slice count the run publishes
            r = r2;
        }
    if (ntiles >= (1u << 24)) return fail(STE_EINVAL, "scheduled forward pass: a window has too many tiles");
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return fail(STE_ENOGPU, "no HIP device");
    // every wave of the launch must be resident at once (a wait may look at any other wave's earlier rounds): one per SIMD
    if (sc->nwaves > 4 * ncu) return fail(STE_EINVAL, "scheduled forward pass: nwaves exceeds the device's SIMD count (4 per compute unit)");
    hipStream_t s = (hipStream_t)stream;
    char* dw = (char*)sc->dev_ws;
    int rc = upload_table(dw, hw, lay.progress, lay.total - lay.progress, s, "scheduled forward pass: table upload");
    if (rc) return rc;
    ste::SchedParams sp;
    sp.kps = (const ste::KParams*)(dw + lay.kps);
    sp.items = (const ste::SchedItem*)(dw + lay.items);
    sp.nrounds = sc->nrounds;
    sp.nwaves = sc->nwaves;
    sp.progress = (int*)(dw + lay.progress);
    sp.window_done = sc->window_done;
    sp.error = sc->error;
    sp.timeout_ticks = (unsigned long long)((sc->timeout_s > 0 ? sc->timeout_s : 2.0) * 1e8);
    sp.started = sc->started;
    const dim3 grid((unsigned)sc->nwaves), block(64);
    if (!first) return fail(STE_EINVAL, "scheduled forward pass: no kernel variant");
    with_forward_variant(*first, [&](auto gains, auto fast, auto robust) {
        constexpr bool kG = decltype(gains)::value, kF = decltype(fast)::value, kR = decltype(robust)::value;
        if (kG && kF && !kR && all_plain)
            hipLaunchKernelGGL(ste::ukf_forward_sched_plain, grid, block, 0, s, sp);
        else
            hipLaunchKernelGGL((ste::ukf_forward_sched<kG, kF, kR>), grid, block, 0, s, sp);
    });
    return check_hip(hipGetLastError(), "ukf_forward_sched launch");
}

int ste_stream_wait_counter(const int32_t* counter, int32_t need, int32_t* error, double timeout_s, void* stream) {
    if (!counter) return fail(STE_EINVAL, "counter is NULL");
    hipLaunchKernelGGL(ste::sched_gate, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)counter, (int)need, (int*)error,
                       (unsigned long long)((timeout_s > 0 ? timeout_s : 2.0) * 1e8));
    return check_hip(hipGetLastError(), "sched_gate launch");
}

size_t ste_ukf_forward_sched_progress_offset(int32_t nwindows, int32_t max_slices, int64_t ntiles_total, int32_t nrounds,
                                             int32_t nwaves) {
    if (nwindows < 0 || max_slices < 0 || ntiles_total < 0 || nrounds < 0 || nwaves < 0) return 0;
    return sched_layout_for((size_t)nwindows, (size_t)max_slices, (size_t)ntiles_total, (size_t)nrounds, (size_t)nwaves).progress;
}

size_t ste_urtss_backward_sched_workspace(int32_t nwindows, int64_t ntiles_total) {
    if (nwindows < 0 || ntiles_total < 0) return 0;
    return align16((size_t)nwindows * sizeof(ste::KParams)) + align16((size_t)ntiles_total * sizeof(ste::SmoothItem));
}

int ste_urtss_backward_sched_f64(const ste_bwd_sched_f64* sc, void* stream) {
    if (!sc) return fail(STE_EINVAL, "schedule pointer is NULL");
    if (sc->nwindows < 1 || !sc->windows) return fail(STE_EINVAL, "scheduled smoother: nwindows >= 1 and windows are required");
    if (sc->nitems < 1 || !sc->items) return fail(STE_EINVAL, "scheduled smoother: nitems >= 1 and items are required");
    if (!sc->host_ws || !sc->dev_ws || !sc->progress || !sc->error)
        return fail(STE_EINVAL, "scheduled smoother: host_ws, dev_ws, progress and error are required");
    const int step = sc->slice_steps ? sc->slice_steps : STE_SLICE_ALIGN;
    if (step < STE_SLICE_ALIGN || step % STE_SLICE_ALIGN != 0)
        return fail(STE_EINVAL, "scheduled smoother: slice_steps must be a positive multiple of STE_SLICE_ALIGN (64)");
    const size_t kp_bytes = align16((size_t)sc->nwindows * sizeof(ste::KParams));
    const size_t total = kp_bytes + align16((size_t)sc->nitems * sizeof(ste::SmoothItem));
    if (sc->ws_bytes < total) return fail(STE_EINVAL, "scheduled smoother: workspace too small (ste_urtss_backward_sched_workspace)");
    char* hw = (char*)sc->host_ws;
    ste::KParams* kps = (ste::KParams*)hw;
    std::vector<int> nslices((size_t)sc->nwindows), tile0((size_t)sc->nwindows + 1);
    size_t ntiles = 0;
    int shift = -1;
    bool all_plain = true;  // the plain kernel only if every window is a plain batch (ste_ukf.h: plain_batch)
    for (int w = 0; w < sc->nwindows; ++w) {
        const ste_ukf_batch_f64& b = sc->windows[w];
        if (b.B <= 0 || b.Nmax <= 0) return fail(STE_EINVAL, "scheduled smoother: a window has B <= 0 or Nmax <= 0");
        if (b.step_begin != 0 || b.step_end != 0) return fail(STE_EINVAL, "scheduled smoother: windows must not carry a step range of their own");
        int rc = make_params(&b, true, kps + w);
        if (rc) return rc;
        const ste::KParams& kp = kps[w];
        // one kernel runs every window: the one-kernel smoother from the forward pass's work rows (what launch_backward picks
        // for a batch of more than kLeanSmootherMaxTracks tracks), with or without rates of its own
        if (!kp.rts_work || ste::lean_smoother(kp))
            return fail(STE_EINVAL, "scheduled smoother: every window must take the one-kernel smoother (rts_work, more than 4096 tracks or tuning bit 10)");
        const int sh = (kp.sog_rate_rts || kp.cog_rate_rts) ? 1 : 0;
        if (shift >= 0 && sh != shift) return fail(STE_EINVAL, "scheduled smoother: the windows must agree on smoother rates (one kernel runs them all)");
        shift = sh;
        all_plain = all_plain && ste::plain_batch(kp);
        nslices[w] = std::max(1, (b.Nmax + step - 1) / step);
        tile0[w] = (int)ntiles;
        ntiles += ((size_t)b.B + 63) / 64;
        if (ntiles > 0x7fffffff) return fail(STE_EINVAL, "scheduled smoother: too many tiles");
    }
    tile0[sc->nwindows] = (int)ntiles;
    if ((size_t)sc->nitems != ntiles) return fail(STE_EINVAL, "scheduled smoother: items must name every tile of every window once");
    ste::SmoothItem* items = (ste::SmoothItem*)(hw + kp_bytes);
    std::vector<char> seen(ntiles, 0);
    for (int i = 0; i < sc->nitems; ++i) {
        const int w = sc->items[2 * i], t = sc->items[2 * i + 1];
        if (w < 0 || w >= sc->nwindows || t < 0 || t >= tile0[w + 1] - tile0[w])
            return fail(STE_EINVAL, "scheduled smoother: an item names a window or tile that does not exist");
        if (seen[(size_t)(tile0[w] + t)]) return fail(STE_EINVAL, "scheduled smoother: a tile appears twice");
        seen[(size_t)(tile0[w] + t)] = 1;
        items[i].kp = w;
        items[i].tile = t;
        items[i].prog = tile0[w] + t;
        items[i].need = nslices[w];
    }
    hipStream_t s = (hipStream_t)stream;
    char* dw = (char*)sc->dev_ws;
    int rc = upload_table(dw, hw, total, 0, s, "scheduled smoother: table upload");
    if (rc) return rc;
    ste::SmoothSchedParams sp;
    sp.kps = (const ste::KParams*)dw;
    sp.items = (const ste::SmoothItem*)(dw + kp_bytes);
    sp.progress = sc->progress;
    sp.error = sc->error;
    sp.timeout_ticks = (unsigned long long)((sc->timeout_s > 0 ? sc->timeout_s : 2.0) * 1e8);
    return ste::launch_recur_sched(shift != 0, all_plain, sc->nitems, sp, s);
}

int ste_urtss_backward_f64(const ste_ukf_batch_f64* b, void* stream) {
    ste::KParams kp;
    int rc = make_params(b, true, &kp);
    if (rc) return rc;
    return launch_backward(kp, nullptr, (hipStream_t)stream);
}

int ste_ukf_urtss_f64(const ste_ukf_batch_f64* b, void* stream) {
    const char* fn = "ste_ukf_urtss_f64";
    ste::KParams kp;
    int rc = make_params(b, true, &kp);
    if (rc) return rc;
    rc = whole_passes(fn, b, "time slices go through ste_ukf_forward_f64");
    if (rc) return rc;
    rc = launch_forward(fn, kp, nullptr, nullptr, (hipStream_t)stream);
    if (rc) return rc;
    return launch_backward(kp, nullptr, (hipStream_t)stream);
}

int ste_ukf_forward_noise_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_ukf_loglik_f64* l, void* stream) {
    const char* fn = "ste_ukf_forward_noise_f64";
    ste::NoiseParams np;
    int rc = noise_params(fn, b, nz, &np);
    if (rc) return rc;
    ste::LikParams lp;
    bool hist = true;
    if (l) {
        rc = lik_params(fn, b, l, &lp, &hist);
        if (rc) return rc;
    }
    ste::KParams kp;
    rc = make_params(b, false, &kp, hist);
    if (rc) return rc;
    noise_route(b, nz, &kp);
    if (!l) {  // (with the likelihood: whole passes, lik_params)
        rc = slice_params(b, &kp);
        if (rc) return rc;
    }
    return launch_forward(fn, kp, l ? &lp : nullptr, &np, (hipStream_t)stream);
}

int ste_urtss_backward_noise_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, void* stream) {
    ste::NoiseParams np;
    int rc = noise_params("ste_urtss_backward_noise_f64", b, nz, &np);
    if (rc) return rc;
    ste::KParams kp;
    rc = make_params(b, true, &kp);
    if (rc) return rc;
    return launch_backward(kp, &np, (hipStream_t)stream);
}

int ste_ukf_urtss_noise_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, void* stream) {
    const char* fn = "ste_ukf_urtss_noise_f64";
    ste::NoiseParams np;
    int rc = noise_params(fn, b, nz, &np);
    if (rc) return rc;
    ste::KParams kp;
    rc = make_params(b, true, &kp);
    if (rc) return rc;
    rc = whole_passes(fn, b, "time slices go through ste_ukf_forward_noise_f64");
    if (rc) return rc;
    noise_route(b, nz, &kp);
    rc = launch_forward(fn, kp, nullptr, &np, (hipStream_t)stream);
    if (rc) return rc;
    return launch_backward(kp, &np, (hipStream_t)stream);
}

// ---- posterior track sampling (ste_ukf_sample_f64) ---------------------------------------------------------------------
namespace {
int sample_params(const char* fn, const ste_ukf_batch_f64* b, const ste_ukf_sample_f64* sm, ste::KParams* kp) {
    if (!b) return fail(STE_EINVAL, "batch pointer is NULL");
    if (!sm) return fail(STE_EINVAL, "%s: the sampler arguments (sm) are NULL", fn);
    if (!sm->samples || !sm->coef) return fail(STE_EINVAL, "%s: sm->samples and sm->coef are required", fn);
    if (sm->nsamples < 1) return fail(STE_EINVAL, "%s: sm->nsamples must be >= 1", fn);
    if (sm->flags != 0) return fail(STE_EINVAL, "%s: sm->flags must be 0", fn);
    if (!b->rts_work || !b->fwd_mean || !b->fwd_cov)
        return fail(STE_EINVAL, "%s samples from a completed forward pass with rts_work: rts_work, fwd_mean and fwd_cov are "
                                "required", fn);
    int rc = whole_passes(fn, b, "the sampler walks every row of a track, so time slices (step_begin / step_end) are refused");
    if (rc) return rc;
    rc = make_params(b, true, kp);
    if (rc) return rc;
    if (sm->nsamples > 65535) return fail(STE_EINVAL, "%s: sm->nsamples is limited to 65535 per call (one grid row per sample group)", fn);
    return STE_OK;
}
}  // namespace

int ste_urtss_sample_prepare_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64* sm,
                                 void* stream) {
    ste::KParams kp;
    int rc = sample_params("ste_urtss_sample_prepare_f64", b, sm, &kp);
    if (rc) return rc;
    return ste::launch_sample_coef(kp, nz, *sm, (hipStream_t)stream);
}

int ste_urtss_sample_draw_f64(const ste_ukf_batch_f64* b, const ste_ukf_sample_f64* sm, void* stream) {
    ste::KParams kp;
    int rc = sample_params("ste_urtss_sample_draw_f64", b, sm, &kp);
    if (rc) return rc;
    return ste::launch_sample_recur(kp, *sm, (hipStream_t)stream);
}

int ste_urtss_sample_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64* sm, void* stream) {
    ste::KParams kp;
    int rc = sample_params("ste_urtss_sample_f64", b, sm, &kp);
    if (rc) return rc;
    rc = ste::launch_sample_coef(kp, nz, *sm, (hipStream_t)stream);
    if (rc) return rc;
    return ste::launch_sample_recur(kp, *sm, (hipStream_t)stream);
}

// ---- lag-one cross-covariance of the smoother (ste_lag_one_f64; the kernel is in ste_lagone.hip) ---------------------------
int ste_urtss_lag_one_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_lag_one_f64* lg, void* stream) {
    const char* fn = "ste_urtss_lag_one_f64";
    if (!b) return fail(STE_EINVAL, "batch pointer is NULL");
    if (!lg) return fail(STE_EINVAL, "%s: the lag-one arguments (lg) are NULL", fn);
    if (!lg->lag1) return fail(STE_EINVAL, "%s: lg->lag1 is required", fn);
    if (lg->flags & ~STE_LAG1_POSITION) return fail(STE_EINVAL, "%s: lg->flags has unknown bits (STE_LAG1_POSITION is the only one)", fn);
    if (lg->reserved != 0) return fail(STE_EINVAL, "%s: lg->reserved must be 0", fn);
    if (!b->rts_work || !b->fwd_mean || !b->fwd_cov)
        return fail(STE_EINVAL, "%s forms the gains from a completed forward pass with rts_work: rts_work, fwd_mean and fwd_cov "
                                "are required", fn);
    int rc = whole_passes(fn, b, "the lag-one covariance covers every row of a track, so time slices (step_begin / step_end) are refused");
    if (rc) return rc;
    ste::KParams kp;
    rc = make_params(b, true, &kp);  // sm_mean and sm_cov among it: row k + 1 of sm_cov is the second factor
    if (rc) return rc;
    return ste::launch_lag_one(kp, nz, *lg, (hipStream_t)stream);
}

int ste_geodetic_dynamics_f64(int64_t count, const double* x, const double* dt, const double* sog_rate,
                              const double* cog_rate, double* out, void* stream) {
    if (count < 0) return fail(STE_EINVAL, "count must be >= 0");
    if (count == 0) return STE_OK;
    if (!x || !dt || !sog_rate || !cog_rate || !out) return fail(STE_EINVAL, "NULL pointer argument");
    const unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL(ste::geodetic_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (size_t)count, x, dt,
                       sog_rate, cog_rate, out);
    return check_hip(hipGetLastError(), "geodetic_dynamics launch");
}

int ste_ukf_predict_f64(int64_t count, const double* x, const double* P, const double* dt, const double* sog_rate,
                        const double* cog_rate, const double* noise, const double* Q, double fan_scale, double w0,
                        double wi, double* x_out, double* P_out, int32_t* status, void* stream) {
    if (count < 0) return fail(STE_EINVAL, "count must be >= 0");
    if (count == 0) return STE_OK;
    if (!x || !P || !dt || !sog_rate || !cog_rate || !Q || !x_out || !P_out) return fail(STE_EINVAL, "NULL pointer argument");
    ste::Mats m;
    memset(&m, 0, sizeof(m));
    m.fan_scale = fan_scale;
    m.w0 = w0;
    m.wi = wi;
    memcpy(m.Q, Q, sizeof(double) * 16);
    const unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL(ste::predict_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (size_t)count, m, x, P, dt,
                       sog_rate, cog_rate, noise, x_out, P_out, status);
    return check_hip(hipGetLastError(), "ukf_predict launch");
}

int ste_ukf_update_f64(int64_t count, const double* x, const double* P, const double* z, const double* noise,
                       const double* H, const double* R, double* x_out, double* P_out, int32_t* status, void* stream) {
    if (count < 0) return fail(STE_EINVAL, "count must be >= 0");
    if (count == 0) return STE_OK;
    if (!x || !P || !z || !H || !R || !x_out || !P_out) return fail(STE_EINVAL, "NULL pointer argument");
    ste::Mats m;
    memset(&m, 0, sizeof(m));
    memcpy(m.H, H, sizeof(double) * 16);
    memcpy(m.R, R, sizeof(double) * 16);
    const unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL(ste::update_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (size_t)count, m, x, P, z,
                       noise, x_out, P_out, status);
    return check_hip(hipGetLastError(), "ukf_update launch");
}

int ste_ukf_robust_terms_f64(int64_t count, const double* x, const double* P, const double* z, const double* H,
                             const double* R, double* gamma, double* denom, void* stream) {
    if (count < 0) return fail(STE_EINVAL, "count must be >= 0");
    if (count == 0) return STE_OK;
    if (!x || !P || !z || !H || !R || !gamma || !denom) return fail(STE_EINVAL, "NULL pointer argument");
    ste::Mats m;
    memset(&m, 0, sizeof(m));
    memcpy(m.H, H, sizeof(double) * 16);
    memcpy(m.R, R, sizeof(double) * 16);
    const unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL(ste::robust_terms_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (size_t)count, m, x, P, z,
                       gamma, denom);
    return check_hip(hipGetLastError(), "robust_terms launch");
}

int ste_sigma_points_f64(int64_t count, const double* x, const double* P, double scale, double* out, void* stream) {
    if (count < 0) return fail(STE_EINVAL, "count must be >= 0");
    if (count == 0) return STE_OK;
    if (!x || !P || !out) return fail(STE_EINVAL, "NULL pointer argument");
    const unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL(ste::sigma_points_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (size_t)count, x, P,
                       scale, out);
    return check_hip(hipGetLastError(), "sigma_points launch");
}

int ste_sigma_points_generic_f64(int32_t n, int64_t count, const double* x, const double* P, double scale, double* out,
                                 void* stream) {
    if (n < 1 || n > ste::kMaxGenericN) return fail(STE_EINVAL, "n must be in 1..16");
    if (count < 0) return fail(STE_EINVAL, "count must be >= 0");
    if (count == 0) return STE_OK;
    if (!x || !P || !out) return fail(STE_EINVAL, "NULL pointer argument");
    const unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL(ste::sigma_points_generic_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, (int)n,
                       (size_t)count, x, P, scale, out);
    return check_hip(hipGetLastError(), "sigma_points_generic launch");
}

}  // extern "C"
