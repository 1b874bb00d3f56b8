// ste_lagone.hip — the lag-one cross-covariance of the unscented smoother and the exact covariance of a position at a query
// time, for gfx950 (MI355X).  fp64 throughout; no MFMA (4x4 contractions); no LDS.  include/ste.h carries the definitions
// (ste_urtss_lag_one_f64, ste_track_position_cov_f64) and tests/lag_one_cases.py restates them in NumPy.
//
// Kernels ("Lag-one covariance"):
//   urtss_lag_one<shift, track noise>   a lane per (row, track), launched like urtss_sample_coef / urtss_gains_all:
//                                       L_k = Cov(x_k, x_{k+1} | all data) = K_k P^s_{k+1}, with K_k the smoother's own gain
//                                       (smoother_step_gain on work rows in D form, load_lean_row on rows the two-kernel
//                                       smoother rewrote: ste_smooth.h, shared with ste_smooth.hip and ste_sample.hip) and
//                                       P^s_{k+1} row k + 1 of sm_cov.  No square root: what the sampler's coefficient
//                                       kernel spends on sym_sqrt_p is not spent here.  Reads the batch, writes none of it.
//   position_cov<full>                  a lane per query: the locate step of position_query (ste_position.hip), then
//                                       P(u) = (1-u)^2 P^s_k + u^2 P^s_{k+1} + (1-u) u (L_k + L_k^T) from 10 gathers (the
//                                       lon / lat block) or 36 (the whole 4 x 4).  Reads no states.  Every output word has
//                                       one writer: plain loads and stores, no atomics.
//
// The entry point of the first kernel and its argument checks are in ste_kernels.hip with the rest of the smoother's ABI; the
// second is self-contained, like ste_track_positions_f64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_ukf.h"
#include "ste_smooth.h"
#include "ste_geodesy.h"  // clamp01, is_finite; last: it switches contraction off for the rest of the file (the gain code above keeps its own)

namespace ste {

// ---------------------------------------------------------------------------------------------------------------
// L_k = K_k P^s_{k+1}
// ---------------------------------------------------------------------------------------------------------------
struct LagParams {
    double* lag1;     // [Nmax][16 or 4][ld]
    int32_t* status;  // [B] or nullptr
    int position;     // 1: the four entries of the lon / lat block
};

// acc = K[r][0] * P[0][c]; acc = fma(K[r][i], P[i][c], acc) for i = 1, 2, 3: the order of the header, as sample_cond_cov
__device__ __forceinline__ double lag_entry(const double (&K)[4][4], const double (&Ps)[10], int r, int c) {
#pragma clang fp contract(off)  // explicit fma() only: the same bits in either output form
    double acc = K[r][0] * Ps[tix(0, c)];
    STE_UNROLL
    for (int i = 1; i < 4; ++i) acc = fma(K[r][i], Ps[tix(i, c)], acc);
    return acc;
}

template <bool kShift, bool kTrackNoise>
__global__ __launch_bounds__(64) void urtss_lag_one(const KParams p, const NoiseParams nz, const LagParams lp) {
    const size_t B = (size_t)p.ld;
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= (size_t)p.B * (size_t)p.Nmax) return;
    const size_t t = g % (size_t)p.B;
    const int k = (int)(g / (size_t)p.B);
    const int ns = track_steps(p, t);
    if (k >= ns) return;  // rows past the track's last step are left as they were
    const bool packed = (p.flags & STE_FLAG_PACKED_COV) != 0;
    double K[4][4];
    int st = 0;
    const double fb_raw = p.first_bad[t];
    if (fb_raw >= 0.0) {  // the work rows hold D: the gain as urtss_gains_all forms it
        const bool always_full = p.noise_pred || p.noise_upd || p.noise_rts;
        const bool all_eig = (p.tuning & STE_TUNING_EIG_GAINS) != 0;
        const double kappa = (p.m.wi + p.m.wi) * p.m.fan_scale;
        RecurRow cur;
        load_recur_row<kShift>(p, (size_t)k, B, t, always_full, cur);
        double xn[4], Pn[10], xb[4], Pb[10], q4[4] = {0.0, 0.0, 0.0, 0.0};
        load_vec(p.fwd_mean, (size_t)k + 1, B, t, xn);
        load_cov_p(p.fwd_cov, packed, (size_t)k + 1, B, t, Pn);
        const bool full = work_row_full(p, k, p.upd_idx[(size_t)k * B + t], always_full);
        if constexpr (kTrackNoise) track_q4(p, nz, B, t, q4);
        st |= smoother_step_gain<kShift, kTrackNoise>(p, k, B, t, cur, xn, Pn, full, always_full, all_eig, kappa, fb_raw, xb, Pb, K, q4);
    } else {  // the two-kernel smoother has been here: the rows hold K (of the row, only the gain is used)
        LeanRow lr;
        load_lean_row(p, (size_t)k, B, t, packed, lr);
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) K[r][c] = lr.K[r][c];
        }
    }
    double Ps[10];
    load_cov_p(p.sm_cov, packed, (size_t)k + 1, B, t, Ps);
    double chk = 0.0;
    if (lp.position) {
        double* out = lp.lag1 + ((size_t)k * 4) * B + t;
        STE_UNROLL
        for (int r = 0; r < 2; ++r) {
            STE_UNROLL
            for (int c = 0; c < 2; ++c) {
                const double v = lag_entry(K, Ps, r, c);
                st_stream(&out[(size_t)(2 * r + c) * B], v);
                chk += v * 0.0;
            }
        }
    } else {
        double* out = lp.lag1 + ((size_t)k * 16) * B + t;
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) {
                const double v = lag_entry(K, Ps, r, c);
                st_stream(&out[(size_t)(4 * r + c) * B], v);
                chk += v * 0.0;
            }
        }
    }
    if (!(chk == 0.0)) st |= STE_STATUS_NAN;
    if (st && lp.status) atomicOr(&lp.status[t], st);
}

int launch_lag_one(const KParams& kp, const ste_ukf_noise_f64* nz, const ste_lag_one_f64& lg, hipStream_t s) {
    const LagParams lp = {lg.lag1, lg.status, (lg.flags & STE_LAG1_POSITION) ? 1 : 0};
    if (lp.status) {
        int rc = abi_check_hip(hipMemsetAsync(lp.status, 0, sizeof(int32_t) * (size_t)kp.B, s), "urtss_lag_one status reset");
        if (rc) return rc;
    }
    if (kp.Nmax == 0) return STE_OK;
    const bool shift = kp.sog_rate_rts || kp.cog_rate_rts, tn = nz && nz->Q;
    const NoiseParams np = tn ? NoiseParams{nz->Q, nz->R} : NoiseParams{nullptr, nullptr};
    const dim3 grid((unsigned)(((size_t)kp.B * (size_t)kp.Nmax + 63) / 64)), block(64);
    with_bool(shift, [&](auto sh) {
        with_bool(tn, [&](auto t) {
            hipLaunchKernelGGL((urtss_lag_one<decltype(sh)::value, decltype(t)::value>), grid, block, 0, s, kp, np, lp);
        });
    });
    return abi_check_hip(hipGetLastError(), "urtss_lag_one launch");
}

// ---------------------------------------------------------------------------------------------------------------
// P(u) at query times
// ---------------------------------------------------------------------------------------------------------------
namespace {

struct PCovParams {
    int B, Nmax;
    int packed;    // cov holds upper triangles [row][10] (STE_FLAG_PACKED_COV of the batch), else [row][16]
    int lag_rows;  // 16, or 4 (STE_PCOV_LAG1_POSITION)
    size_t ld;     // tracks per row (track_stride, or B)
    size_t nq;
    const int32_t* nsteps;  // [B] or nullptr
    const int32_t* qtrack;  // [Q]
    const double* qtime;    // [Q]
    const double* t0;       // [ld] or nullptr
    const double* knots;    // [Nmax+1][ld], read only
    const double* cov;      // [Nmax+1][10 or 16][ld]
    const double* lag1;     // [Nmax][lag_rows][ld]
    double* pcov;           // [3 or 10][Q], or nullptr
    int32_t* step;          // [Q] each, or nullptr
    double* frac;
    int32_t* status;
};

// P_rc = ((w0 w0) A_rc + (w1 w1) B_rc) + (w0 w1) (L_rc + L_cr), evaluated as written
__device__ __forceinline__ double blend(double w00, double w11, double w01, double a, double b, double lrc, double lcr) {
#pragma clang fp contract(off)
    return (w00 * a + w11 * b) + w01 * (lrc + lcr);
}

template <bool kFull>
__global__ __launch_bounds__(64) void position_cov(const PCovParams p) {
#pragma clang fp contract(off)
    const size_t q = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= p.nq) return;
    const size_t ld = p.ld, nq = p.nq;
    const double nan = __builtin_nan("");

    // locate: position_query's (ste_position.hip), statement for statement
    int status = 0, row = -1;
    double u = nan;
    bool interior = false;
    const int t = p.qtrack[q];
    if (t < 0 || t >= p.B) {
        status = STE_POS_BAD_INDEX;  // nothing of the query's track is read
    } else {
        const double t0 = p.t0 ? p.t0[t] : 0.0;
        const double* kn = p.knots + (size_t)t;  // T_k: kn[k * ld]
        const double T0 = kn[0];
        const double tq = p.qtime[q];
        if (!(is_finite(t0) && T0 == T0 && is_finite(tq))) {
            status = STE_POS_BAD_TIME;
        } else {
            const int ns = track_steps(p, t);
            const double tau0 = t0 + T0;
            if (tq == tau0) {
                row = 0;
                u = 0.0;
            } else if (ns == 0 || !(tq >= tau0) || !(tq <= t0 + kn[(size_t)ns * ld])) {
                status = STE_POS_OUTSIDE;  // never extrapolated
            } else {
                int lo = 1, hi = ns;  // the smallest j in [1, ns] with tq <= tau_j; tau_ns qualifies
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (tq <= t0 + kn[(size_t)mid * ld]) hi = mid;
                    else lo = mid + 1;
                }
                const double T1 = kn[(size_t)lo * ld];
                if (tq == t0 + T1) {
                    row = lo;
                    u = 0.0;
                } else {
                    const double Tk = kn[(size_t)(lo - 1) * ld];
                    row = lo - 1;
                    u = clamp01((tq - (t0 + Tk)) / (T1 - Tk));
                    interior = true;
                }
            }
        }
    }
    if (p.step) p.step[q] = row;
    if (p.frac) p.frac[q] = u;
    if (p.status) p.status[q] = status;
    if (!p.pcov) return;
    constexpr int kOut = kFull ? 10 : 3, kDim = kFull ? 4 : 2;
    if (row < 0) {
        STE_UNROLL
        for (int e = 0; e < kOut; ++e) p.pcov[(size_t)e * nq + q] = nan;
        return;
    }
    const bool packed = p.packed != 0;
    const double* ca = p.cov + (size_t)t;  // entry e of row j: ca[(cov_at(packed, j, r, c)) * ld]
    if (!interior) {  // a knot hit copies row `row`: the neighbouring row and the lag-one block are not read
        int e = 0;
        STE_UNROLL
        for (int r = 0; r < kDim; ++r) {
            STE_UNROLL
            for (int c = r; c < kDim; ++c) p.pcov[(size_t)(e++) * nq + q] = ca[cov_at(packed, (size_t)row, r, c) * ld];
        }
        return;
    }
    const double w1 = u, w0 = 1.0 - u;
    const double w00 = w0 * w0, w11 = w1 * w1, w01 = w0 * w1;
    const double* la = p.lag1 + ((size_t)row * (size_t)p.lag_rows) * ld + (size_t)t;
    const int ls = p.lag_rows == 16 ? 4 : 2;  // L[r][c] is entry ls * r + c of a lag1 row (kFull: always the 16-entry form)
    double A[kOut], Bn[kOut], L[kDim][kDim];
    {
        int e = 0;
        STE_UNROLL
        for (int r = 0; r < kDim; ++r) {
            STE_UNROLL
            for (int c = r; c < kDim; ++c) {
                A[e] = ca[cov_at(packed, (size_t)row, r, c) * ld];
                Bn[e] = ca[cov_at(packed, (size_t)row + 1, r, c) * ld];
                ++e;
            }
        }
        STE_UNROLL
        for (int r = 0; r < kDim; ++r) {
            STE_UNROLL
            for (int c = 0; c < kDim; ++c) L[r][c] = la[(size_t)(ls * r + c) * ld];
        }
    }
    int e = 0;
    STE_UNROLL
    for (int r = 0; r < kDim; ++r) {
        STE_UNROLL
        for (int c = r; c < kDim; ++c) {
            p.pcov[(size_t)e * nq + q] = blend(w00, w11, w01, A[e], Bn[e], L[r][c], L[c][r]);
            ++e;
        }
    }
}

}  // namespace
}  // namespace ste

extern "C" int ste_track_position_cov_f64(const ste_ukf_batch_f64* b, const ste_position_cov_f64* pc, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_track_position_cov_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!pc) return refuse("the covariance arguments (pc) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!pc->qtrack) return refuse("pc->qtrack is required");
    if (!pc->qtime) return refuse("pc->qtime is required");
    if (!pc->knots)
        return refuse("pc->knots is required (what ste_track_positions_f64 left in its workspace, [Nmax+1][track_stride])");
    if (pc->nqueries < 1 || pc->nqueries > STE_POSITIONS_MAX_QUERIES)
        return refuse("pc->nqueries must be between 1 and STE_POSITIONS_MAX_QUERIES (2^26)");
    if (pc->flags & ~(STE_PCOV_FULL | STE_PCOV_LAG1_POSITION))
        return refuse("pc->flags has unknown bits (STE_PCOV_FULL and STE_PCOV_LAG1_POSITION are the two)");
    if (pc->reserved != 0) return refuse("pc->reserved must be 0");
    const bool full = (pc->flags & STE_PCOV_FULL) != 0, lag_pos = (pc->flags & STE_PCOV_LAG1_POSITION) != 0;
    if (full && lag_pos) return refuse("STE_PCOV_FULL needs the 16-entry lag1, not the position form (STE_PCOV_LAG1_POSITION)");
    if (!pc->pcov && !pc->step && !pc->frac && !pc->status)
        return refuse("no output asked for (pcov, step, frac and status are all NULL)");
    if (pc->pcov && !pc->cov) return refuse("pc->cov is required with pcov");
    if (pc->pcov && !pc->lag1 && b->Nmax > 0)
        return refuse("pc->lag1 is required with pcov when Nmax > 0 (ste_urtss_lag_one_f64 writes it)");
    PCovParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.packed = (b->flags & STE_FLAG_PACKED_COV) ? 1 : 0;
    p.lag_rows = lag_pos ? 4 : 16;
    p.ld = track_ld(b);
    p.nq = (size_t)pc->nqueries;
    p.nsteps = b->nsteps;
    p.qtrack = pc->qtrack;
    p.qtime = pc->qtime;
    p.t0 = pc->t0;
    p.knots = pc->knots;
    p.cov = pc->cov;
    p.lag1 = pc->lag1;
    p.pcov = pc->pcov;
    p.step = pc->step;
    p.frac = pc->frac;
    p.status = pc->status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((p.nq + 63) / 64)), block(64);
    with_bool(full, [&](auto f) { hipLaunchKernelGGL((position_cov<decltype(f)::value>), grid, block, 0, s, p); });
    return abi_check_hip(hipGetLastError(), "position_cov launch");
}
