// ste_smooth.h — what the work-row smoothers (ste_smooth.hip), the posterior-track sampler (ste_sample.hip) and the lag-one
// covariance (ste_lagone.hip) share on the
// device: how a row that the forward pass left in rts_work is read, and the gain K = D pinv(P_b) formed from it -- one
// function for the one-kernel smoother, the gains pass of the two-kernel form and the sampler's coefficients: same code, same
// bits.  The row layout itself (kWorkD ...) is in ste_ukf.h.  Everything here is inlined into its callers.
#pragma once
#include "ste_ukf.h"

namespace ste {

// Is work row k "full" (x_b and P_b stored)?  Mirrors the forward kernels' choice: full when the step was followed by a
// measurement update (ui = upd_idx[k] names a valid observation), for row 0 of a run that starts with an update, and
// throughout a run with recorded noise.
__device__ __forceinline__ bool work_row_full(const KParams& p, int k, int ui, bool always_full) {
    return always_full || (ui >= 0 && ui < p.Tmax) || (k == 0 && !(p.flags & STE_FLAG_NO_INITIAL_UPDATE));
}

struct RecurRow {
    double D2[8], xk[4], Pk[10];  // columns 0-1 of D of step k (rows 2-3 only with recorded noise); filtered row k
    double shift[2];              // smoother rates that differ from the forward rates: what they add to x_b[2:4]
};
// Speed and heading pass through the process model as x + rate * dt (non_linear_process.py:74-75) and the position
// components do not see the rates at all, so a smoother step that uses other rates than the forward step did
// (unscented.py:287-292: the smoother indexes the repeated rate arrays by step) sees the same propagated fan moved by
// (0, 0, d_sog * dt, d_cog * dt): x_b moves by that much, the fan's spread and D not at all, and P_b -- taken about the
// filtered mean x_k (:324-325) -- becomes C + b' b'^T with the new b' = x_b' - x_k.
// kPlain: a plain batch (ste_ukf.h: plain_batch), the packed layout compiled in.
template <bool kShift, bool kPlain = false>
__device__ __forceinline__ void load_recur_row(const KParams& p, size_t k, size_t B, size_t t, bool d_rows23, RecurRow& g) {
    g.shift[0] = g.shift[1] = 0.0;
    if (kShift) {
        const double dt = p.dt[k * B + t];
        if (p.sog_rate_rts) g.shift[0] = (p.sog_rate_rts[k * B + t] - p.sog_rate[k * B + t]) * dt;
        if (p.cog_rate_rts) g.shift[1] = (p.cog_rate_rts[k * B + t] - p.cog_rate[k * B + t]) * dt;
    }
    const double* w = p.rts_work + (k * kWorkElems) * B + t;
    STE_UNROLL
    for (int e = 0; e < 4; ++e) g.D2[e] = w[(kWorkD + e) * B];
    if (d_rows23) {
        STE_UNROLL
        for (int e = 4; e < 8; ++e) g.D2[e] = w[(kWorkD + e) * B];
    }
    load_vec(p.fwd_mean, k, B, t, g.xk);
    if constexpr (kPlain)
        load_cov_p<true>(p.fwd_cov, k, B, t, g.Pk);
    else
        load_cov_p(p.fwd_cov, (p.flags & STE_FLAG_PACKED_COV) != 0, k, B, t, g.Pk);
}

// Every value load_recur_row loads, consumed (in_vgpr): in front of a step loop whose rows are loaded a step ahead, so that
// the loop is entered with nothing pending.  Without recorded noise rows 2-3 of D are neither loaded nor read.
template <bool kShift>
__device__ __forceinline__ void consume_recur_row(bool d_rows23, RecurRow& g) {
    if (kShift) {
        g.shift[0] = in_vgpr(g.shift[0]);
        g.shift[1] = in_vgpr(g.shift[1]);
    }
    STE_UNROLL
    for (int e = 0; e < 4; ++e) g.D2[e] = in_vgpr(g.D2[e]);
    if (d_rows23) {
        STE_UNROLL
        for (int e = 4; e < 8; ++e) g.D2[e] = in_vgpr(g.D2[e]);
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) g.xk[c] = in_vgpr(g.xk[c]);
    STE_UNROLL
    for (int e = 0; e < 10; ++e) g.Pk[e] = in_vgpr(g.Pk[e]);
}

// x_b, P_b as the forward pass stored them in work row k (a full row, work_row_full)
__device__ __forceinline__ void load_stored_xb_pb(const KParams& p, size_t k, size_t B, size_t t, double (&xb)[4], double (&Pb)[10]) {
    const double* w = p.rts_work + (k * kWorkElems) * B + t;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xb[c] = w[(kWorkXb + c) * B];
    STE_UNROLL
    for (int e = 0; e < 10; ++e) Pb[e] = w[(kWorkPb + e) * B];
}

// What the smoother's step k needs besides the recurrence itself: x_b, P_b (stored, or rebuilt from history rows k and
// k + 1) and the gain K = D pinv(P_b) (unscented.py:315-333).  `cur` = work-row / history data of step k, (xn, Pn) = filtered
// row k + 1, `full` = work row k holds x_b and P_b.  Shared by the one-kernel smoother (urtss_recur_l1) and the two-kernel
// form for small batches (urtss_gains_all + urtss_recur_lean): same code, same bits.
// kTrackNoise: the four entries of Q it reads come from `q4` (Q[0][2], Q[0][3], Q[1][2], Q[1][3] of this track, see
// track_q4) instead of from the kernel arguments.
// kRowAhead (the step loop of smooth_tile_l1): on a full row `xb` / `Pb` come in holding the stored x_b, P_b, loaded by the
// caller a row ahead (load_stored_xb_pb) -- in front of the previous row's stores, so that the step waits for neither the
// loads' latency nor those stores' acknowledgements ("Store drain"); on other rows they are formed here.
// kPlain: a plain batch (no recorded noise: the caller passes always_full = false, and noise_rts is not looked at).
template <bool kShift, bool kTrackNoise = false, bool kRowAhead = false, bool kPlain = false>
__device__ __forceinline__ int smoother_step_gain(const KParams& p, int k, size_t B, size_t t, const RecurRow& cur,
                                                  const double (&xn)[4], const double (&Pn)[10], bool full, bool always_full,
                                                  bool all_eig, double kappa, double first_bad, double (&xb)[4],
                                                  double (&Pb)[10], double (&K)[4][4], const double* q4 = nullptr) {
    // x_b, P_b: stored (a quarter of the steps of the bench batch), or the prediction itself -- the step was not followed by
    // an update, so row k + 1 of the filtered history is x^-, P^-, and P_b = P^- + b b^T with b = x^- - x_k
    if (!kRowAhead || !full) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) xb[c] = xn[c];
        if (kShift) {  // the smoother's own rates (load_recur_row)
            xb[2] += cur.shift[0];
            xb[3] += cur.shift[1];
        }
        double bv[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) bv[c] = xb[c] - cur.xk[c];
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = r; c < 4; ++c) Pb[tix(r, c)] = fma(bv[r], bv[c], Pn[tix(r, c)]);
        }
    }
    if (full) {
        if (!kRowAhead) load_stored_xb_pb(p, (size_t)k, B, t, xb, Pb);
        if (kShift) {
            // stored with the forward rates: P_b = C + b b^T with b = (weighted mean of the fan) - x_k, i.e. x_b - x_k
            // less the recorded noise that was added to x_b (unscented.py:319-325); now b' = b + s, s = (0, 0, shift):
            // P_b' = P_b + b s^T + s b^T + s s^T
            double bv[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) bv[c] = xb[c] - cur.xk[c];
            if constexpr (!kPlain) {
                if (p.noise_rts) {
                    STE_UNROLL
                    for (int c = 0; c < 4; ++c) bv[c] -= p.noise_rts[((size_t)k * 4 + c) * B + t];
                }
            }
            const double s2 = cur.shift[0], s3 = cur.shift[1];
            Pb[tix(0, 2)] = fma(bv[0], s2, Pb[tix(0, 2)]);
            Pb[tix(1, 2)] = fma(bv[1], s2, Pb[tix(1, 2)]);
            Pb[tix(0, 3)] = fma(bv[0], s3, Pb[tix(0, 3)]);
            Pb[tix(1, 3)] = fma(bv[1], s3, Pb[tix(1, 3)]);
            Pb[tix(2, 2)] = fma(bv[2] + bv[2] + s2, s2, Pb[tix(2, 2)]);
            Pb[tix(3, 3)] = fma(bv[3] + bv[3] + s3, s3, Pb[tix(3, 3)]);
            Pb[tix(2, 3)] = fma(bv[2], s3, fma(s2, bv[3] + s3, Pb[tix(2, 3)]));
            xb[2] += s2;
            xb[3] += s3;
        }
    }
    // the gain K = D pinv(P_b) (unscented.py:333)
    double D[4][4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        D[r][0] = cur.D2[r * 2 + 0];
        D[r][1] = cur.D2[r * 2 + 1];
        D[r][2] = kappa * cur.Pk[tix(r, 2)];
        D[r][3] = kappa * cur.Pk[tix(r, 3)];
    }
    if (!always_full) {
        // rows 2-3 of D's first two columns are the cross moments of (speed, heading) with (lon, lat) about the
        // predicted mean, i.e. the corresponding entries of P^- before Q was added.  Where the step was not followed
        // by an update P^- is row k + 1 of the filtered history itself; on a full row (x_b, P_b stored) it is
        // P_b - b b^T with b = x_b - x_k (no recorded noise here): D[2:4, 0:2] = (P^- - Q)[0:2, 2:4]^T.  (Forming
        // P_b = P^- + b b^T first and subtracting b b^T again on every row cost ~eps |b_c b_r| on small cross moments.)
        double bv[4];
        STE_UNROLL
        for (int c = 0; c < 4; ++c) bv[c] = xb[c] - cur.xk[c];
        STE_UNROLL
        for (int r = 2; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 2; ++c) {
                const double pm = full ? fma(-bv[c], bv[r], Pb[tix(c, r)]) : Pn[tix(c, r)];
                if constexpr (kTrackNoise)
                    D[r][c] = pm - q4[c * 2 + (r - 2)];
                else
                    D[r][c] = pm - p.m.Q[c * 4 + r];
            }
        }
    }
    if (__builtin_expect(__any((double)k >= first_bad), 0)) {
        if ((double)k >= first_bad) {
            const double* w = p.rts_work + ((size_t)k * kWorkElems) * B + t;
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                D[r][2] = w[(kWorkD23 + r * 2 + 0) * B];
                D[r][3] = w[(kWorkD23 + r * 2 + 1) * B];
            }
            // In the step loop, waited for in this cold branch: pending where it rejoins, these loads make every step wait
            // for all the wave has in flight, the previous row's stores included, at the head of the solve.
            if (kRowAhead) {
                STE_UNROLL
                for (int r = 0; r < 4; ++r) {
                    D[r][2] = in_vgpr(D[r][2]);
                    D[r][3] = in_vgpr(D[r][3]);
                }
            }
        }
    }
    return smoother_gain(Pb, D, all_eig, K);

}

// Per-track noise: the entries (0,2) (0,3) (1,2) (1,3) of track t's Q, once per track (or per lane of urtss_gains_all)
__device__ __forceinline__ void track_q4(const KParams& p, const NoiseParams& nz, size_t B, size_t t, double (&q4)[4]) {
    STE_UNROLL
    for (int c = 0; c < 2; ++c) {
        STE_UNROLL
        for (int r = 2; r < 4; ++r) q4[c * 2 + (r - 2)] = nz.Q ? nz.Q[(size_t)tix(c, r) * B + t] : p.m.Q[c * 4 + r];
    }
}

// The two-kernel smoother (ste_smooth.hip: urtss_gains_all + urtss_recur_lean) leaves the gains in the work rows:
constexpr int kLeanK01 = kWorkD, kLeanK23 = kWorkD23;  // K[r][0:2] at kLeanK01 + 2 r, K[r][2:4] at kLeanK23 + 2 r

struct LeanRow {
    double K[4][4], xb[4], Pb[10], xk[4], Pk[10];
};
__device__ __forceinline__ void load_lean_row(const KParams& p, size_t k, size_t B, size_t t, bool packed, LeanRow& g) {
    const double* w = p.rts_work + (k * kWorkElems) * B + t;
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        g.K[r][0] = w[(kLeanK01 + 2 * r + 0) * B];
        g.K[r][1] = w[(kLeanK01 + 2 * r + 1) * B];
        g.K[r][2] = w[(kLeanK23 + 2 * r + 0) * B];
        g.K[r][3] = w[(kLeanK23 + 2 * r + 1) * B];
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) g.xb[c] = w[(kWorkXb + c) * B];
    STE_UNROLL
    for (int e = 0; e < 10; ++e) g.Pb[e] = w[(kWorkPb + e) * B];
    load_vec(p.fwd_mean, k, B, t, g.xk);
    load_cov_p(p.fwd_cov, packed, k, B, t, g.Pk);
}

}  // namespace ste
