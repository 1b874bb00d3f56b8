// ste_sample.hip — posterior ship tracks drawn from the unscented smoother by backward simulation, for gfx950 (MI355X), and
// their launches.  fp64 throughout; no MFMA (4x4 contractions); no LDS.  The gain of a row is the smoother's own
// (smoother_step_gain, or the gains the two-kernel smoother left in the work rows): ste_smooth.h, shared with ste_smooth.hip.
// The entry points (ste_urtss_sample_*_f64) and their argument checks are in ste_kernels.hip with the rest of the ABI.
//
// Kernels:
//   urtss_sample_coef + urtss_sample_recur   posterior tracks by backward simulation from the smoother's own gains: the
//                                        coefficients of every (row, track) at once, then a lane per track and up to 4 samples per lane
//
// Reference semantics (paths relative to the reference's src/track_estimators/kalman_filters/):
//   backward : unscented.py:285-351 (rts_step)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_ukf.h"
#include "ste_smooth.h"

namespace ste {

// ---------------------------------------------------------------------------------------------------------------
// Posterior TRACKS from the smoother (ste_urtss_sample_f64): backward simulation with the smoother's own per-step
// quantities.  The smoother gives marginals (sm_mean, sm_cov per row); a track drawn from the joint posterior ties
// neighbouring rows together through the gains:
//     row ns:  x_ns = m_ns + T_ns xi_ns,                         T_ns = symsqrt(P_ns)
//     row k :  y = x_{k+1} - x_b,k (heading wrapped),  x_k = (m_k + K_k y) + T_k xi_k,   T_k = symsqrt(P_k - K_k P_b,k K_k^T)
// with m, P the filtered rows, x_b, P_b, K = D pinv(P_b) exactly what smoother_step_gain forms (P_b about the filtered mean,
// as the reference has it) and xi standard normal draws.  With xi = 0 this IS the smoother's mean recursion (same operation
// order: same bits), and Cov(x_k) = C_k + K Cov(x_{k+1}) K^T is the smoother's covariance recursion, so the ensemble covariance
// of the samples is sm_cov.  The root is the symmetric one of the sigma fan (sym_sqrt_p, cold start, negative eigenvalues
// clamped), not a Cholesky factor: C_k is only semi-definite where Q has zero directions.
//   urtss_sample_coef    a lane per (row, track), like urtss_gains_all: K (16) | x_b (4) | T packed (10) of every row into a
//                        coefficient buffer of the caller's; reads the work rows in either form (D: smoother_step_gain; gains:
//                        as load_lean_row) and writes none of the batch's arrays
//   urtss_sample_recur   a lane per track and 1, 2 or 4 samples per lane (blockIdx.y walks the sample groups): the
//                        recurrence, coefficient row and draws one row ahead in flight, draws consumed and samples written in
//                        the same buffer
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCoefK = 0, kCoefXb = 16, kCoefT = 20, kCoefElems = 30;  // include/ste.h: ste_ukf_sample_f64.coef
constexpr int kMaxSamplesPerLane = 4;

struct SampleParams {
    double* samples;  // [S][Nmax+1][4][ld]
    double* coef;     // [Nmax+1][kCoefElems][ld]
    int32_t* status;  // [B] or nullptr
    int nsamples;
};

// C = P_k - K P_b K^T, packed
__device__ __forceinline__ void sample_cond_cov(const double (&Pk)[10], const double (&K)[4][4], const double (&Pb)[10],
                                                double (&Cc)[10]) {
#pragma clang fp contract(off)  // explicit fma() only: the same bits whichever form the work rows were in
    double KPb[4][4];
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            double acc = K[r][0] * Pb[tix(0, c)];
            STE_UNROLL
            for (int i = 1; i < 4; ++i) acc = fma(K[r][i], Pb[tix(i, c)], acc);
            KPb[r][c] = acc;
        }
    }
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) {
            double acc = KPb[r][0] * K[c][0];
            STE_UNROLL
            for (int i = 1; i < 4; ++i) acc = fma(KPb[r][i], K[c][i], acc);
            Cc[tix(r, c)] = Pk[tix(r, c)] - acc;
        }
    }
}

template <bool kShift, bool kTrackNoise>
__global__ __launch_bounds__(64) void urtss_sample_coef(const KParams p, const NoiseParams nz, const SampleParams sp) {
    const size_t B = (size_t)p.ld;
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= (size_t)p.B * ((size_t)p.Nmax + 1)) return;
    const size_t t = g % (size_t)p.B;
    const int k = (int)(g / (size_t)p.B);
    const int ns = track_steps(p, t);
    if (k > ns) return;
    const bool packed = (p.flags & STE_FLAG_PACKED_COV) != 0;
    double* cw = sp.coef + ((size_t)k * kCoefElems) * B + t;
    double Cc[10];
    double chk = 0.0;
    int st = 0;
    if (k == ns) {
        load_cov_p(p.fwd_cov, packed, (size_t)k, B, t, Cc);  // the last row is drawn from the filtered distribution itself
    } else {
        double K[4][4], xb[4], Pb[10], Pk[10];
        const double fb_raw = p.first_bad[t];
        if (fb_raw >= 0.0) {  // the work rows hold D: the gain as urtss_gains_all forms it
            const bool always_full = p.noise_pred || p.noise_upd || p.noise_rts;
            const bool all_eig = (p.tuning & STE_TUNING_EIG_GAINS) != 0;
            const double kappa = (p.m.wi + p.m.wi) * p.m.fan_scale;
            RecurRow cur;
            load_recur_row<kShift>(p, (size_t)k, B, t, always_full, cur);
            double xn[4], Pn[10], q4[4] = {0.0, 0.0, 0.0, 0.0};
            load_vec(p.fwd_mean, (size_t)k + 1, B, t, xn);
            load_cov_p(p.fwd_cov, packed, (size_t)k + 1, B, t, Pn);
            const bool full = work_row_full(p, k, p.upd_idx[(size_t)k * B + t], always_full);
            if constexpr (kTrackNoise) track_q4(p, nz, B, t, q4);
            st |= smoother_step_gain<kShift, kTrackNoise>(p, k, B, t, cur, xn, Pn, full, always_full, all_eig, kappa, fb_raw, xb, Pb, K, q4);
            STE_UNROLL
            for (int e = 0; e < 10; ++e) Pk[e] = cur.Pk[e];
        } else {  // the two-kernel smoother has been here: the rows hold K, x_b and P_b
            LeanRow lr;
            load_lean_row(p, (size_t)k, B, t, packed, lr);
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                xb[r] = lr.xb[r];
                STE_UNROLL
                for (int c = 0; c < 4; ++c) K[r][c] = lr.K[r][c];
            }
            STE_UNROLL
            for (int e = 0; e < 10; ++e) {
                Pb[e] = lr.Pb[e];
                Pk[e] = lr.Pk[e];
            }
        }
        sample_cond_cov(Pk, K, Pb, Cc);
        STE_UNROLL
        for (int r = 0; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < 4; ++c) {
                cw[(kCoefK + r * 4 + c) * B] = K[r][c];
                chk += K[r][c] * 0.0;
            }
            cw[(kCoefXb + r) * B] = xb[r];
            chk += xb[r] * 0.0;
        }
    }
    double T[10], V[4][4];
    st |= sym_sqrt_p(Cc, 1.0, T, V, false);
    STE_UNROLL
    for (int e = 0; e < 10; ++e) {
        cw[(kCoefT + e) * B] = T[e];
        chk += T[e] * 0.0;
    }
    if (!(chk == 0.0)) st |= STE_STATUS_NAN;
    if (st && sp.status) atomicOr(&sp.status[t], st);
}

template <int kSpl>
struct SampleRow {
    double c[kCoefElems], m[4], xi[kSpl][4];
};
template <int kSpl>
__device__ __forceinline__ void load_sample_row(const KParams& p, const SampleParams& sp, size_t k, size_t B, size_t t,
                                                size_t s0, int nloc, SampleRow<kSpl>& g) {
    const double* cw = sp.coef + (k * kCoefElems) * B + t;
    STE_UNROLL
    for (int e = 0; e < kCoefElems; ++e) g.c[e] = cw[(size_t)e * B];
    load_vec(p.fwd_mean, k, B, t, g.m);
    const size_t rows = (size_t)p.Nmax + 1;
    STE_UNROLL
    for (int j = 0; j < kSpl; ++j) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) g.xi[j][c] = j < nloc ? sp.samples[(((s0 + j) * rows + k) * 4 + c) * B + t] : 0.0;
    }
}

// The recurrence.  A lane carries kSpl samples against ONE load of the row's 30 coefficients and its filtered mean: like
// urtss_recur_lean the loop is bound by load and address issue, not by fp64 (per sample and row: 4 loads, 4 stores, ~45 fp64
// operations), so the 34 shared loads are what sharing saves.  The operation order of m_k + K y is the smoother's (accumulator
// starts at m_k, fma over the columns); T xi is formed on its own and added afterwards, so that zero draws give the smoother's
// bits.  Rows past a track's last are neither read nor written.
template <int kSpl>
__global__ __launch_bounds__(64) void urtss_sample_recur(const KParams p, const SampleParams sp) {
#pragma clang fp contract(off)  // explicit fma() only: a sample's bits do not depend on its slot in the lane
    const size_t B = (size_t)p.ld;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const int ns = track_steps(p, t);
    const size_t s0 = (size_t)blockIdx.y * kSpl;
    const int nloc = min(kSpl, sp.nsamples - (int)s0);
    const size_t rows = (size_t)p.Nmax + 1;
    double xs[kSpl][4];
    STE_UNROLL
    for (int j = 0; j < kSpl; ++j) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) xs[j][c] = 0.0;
    }
    SampleRow<kSpl> nxt;
    load_sample_row<kSpl>(p, sp, (size_t)ns, B, t, s0, nloc, nxt);
    for (int k = p.Nmax; k >= 0; --k) {
        if (!__any(k <= ns)) continue;  // ragged batch: nobody in this wave has reached its last row yet
        if (k <= ns) {
            const SampleRow<kSpl> cur = nxt;
            // the next row (its draws included, read before anything of this lane's is written): in flight during the arithmetic
            load_sample_row<kSpl>(p, sp, (size_t)max(k - 1, 0), B, t, s0, nloc, nxt);
            STE_UNROLL
            for (int j = 0; j < kSpl; ++j) {
                if (j < nloc) {
                    double x[4];
                    if (k < ns) {
                        double y[4];
                        STE_UNROLL
                        for (int c = 0; c < 4; ++c) y[c] = xs[j][c] - cur.c[kCoefXb + c];
                        y[3] = wrap180(y[3]);
                        STE_UNROLL
                        for (int r = 0; r < 4; ++r) {
                            double acc = cur.m[r];
                            STE_UNROLL
                            for (int c = 0; c < 4; ++c) acc = fma(cur.c[kCoefK + r * 4 + c], y[c], acc);
                            x[r] = acc;
                        }
                    } else {
                        STE_UNROLL
                        for (int r = 0; r < 4; ++r) x[r] = cur.m[r];
                    }
                    STE_UNROLL
                    for (int r = 0; r < 4; ++r) {
                        double e = cur.c[kCoefT + tix(r, 0)] * cur.xi[j][0];
                        STE_UNROLL
                        for (int c = 1; c < 4; ++c) e = fma(cur.c[kCoefT + tix(r, c)], cur.xi[j][c], e);
                        x[r] += e;
                    }
                    x[3] = floored_mod(x[3], 360.0);
                    STE_UNROLL
                    for (int c = 0; c < 4; ++c) {
                        st_stream(&sp.samples[(((s0 + j) * rows + (size_t)k) * 4 + c) * B + t], x[c]);
                        xs[j][c] = x[c];
                    }
                }
            }
        }
    }
}

// ===============================================================================================================
// launches (declared in ste_err.h; the entry points are in ste_kernels.hip)
// ===============================================================================================================
namespace {
// Samples per lane of urtss_sample_recur.  Measured at 10 000 tracks x 500 steps ("Posterior tracks"; ms for 1 / 2 / 4
// per lane): 16 samples 4.13 / 2.23 / 1.60 -- the 34 shared loads of a row are what a lane saves --, 8 samples 1.85 / 1.17 / 1.26,
// 4 samples 0.98 / 0.88 / 1.17: sharing pays only while the launch still has the waves to hide its latency, and a lane that
// carries more samples (248 registers at 4, 200 at 2) needs more of them: 628 waves are enough for 4 per lane, 314 are not but
// are for 2.  So: 4 per lane from 512 waves on, else 2 from 256 on, else 1.  Same bits whichever is taken
// (tests/test_track_sampling.py).  ste_dbg_sample_lanes forces one for a measurement (0 = this rule).
constexpr size_t kSampleWavesPerSample = 128;
int g_samples_per_lane = 0;
int pick_samples_per_lane(int B, int nsamples) {
    if (g_samples_per_lane) return g_samples_per_lane;
    const size_t tiles = ((size_t)B + 63) / 64;
    for (int spl = kMaxSamplesPerLane; spl > 1; spl /= 2)
        if (tiles * (((size_t)nsamples + spl - 1) / spl) >= kSampleWavesPerSample * spl) return spl;
    return 1;
}
}  // namespace

int launch_sample_coef(const KParams& kp, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64& sm, hipStream_t s) {
    const SampleParams sp = {sm.samples, sm.coef, sm.status, sm.nsamples};
    if (sp.status) {
        int rc = abi_check_hip(hipMemsetAsync(sp.status, 0, sizeof(int32_t) * (size_t)kp.B, s), "urtss_sample_coef status reset");
        if (rc) return rc;
    }
    const bool shift = kp.sog_rate_rts || kp.cog_rate_rts, tn = nz && nz->Q;
    const NoiseParams np = tn ? NoiseParams{nz->Q, nz->R} : NoiseParams{nullptr, nullptr};
    const dim3 grid((unsigned)(((size_t)kp.B * ((size_t)kp.Nmax + 1) + 63) / 64)), block(64);
    with_bool(shift, [&](auto sh) {
        with_bool(tn, [&](auto t) {
            hipLaunchKernelGGL((urtss_sample_coef<decltype(sh)::value, decltype(t)::value>), grid, block, 0, s, kp, np, sp);
        });
    });
    return abi_check_hip(hipGetLastError(), "urtss_sample_coef launch");
}

int launch_sample_recur(const KParams& kp, const ste_ukf_sample_f64& sm, hipStream_t s) {
    const SampleParams sp = {sm.samples, sm.coef, sm.status, sm.nsamples};
    const int spl = pick_samples_per_lane(kp.B, sp.nsamples);
    const dim3 grid((unsigned)((kp.B + 63) / 64), (unsigned)((sp.nsamples + spl - 1) / spl)), block(64);
    switch (spl) {
        case 1: hipLaunchKernelGGL(urtss_sample_recur<1>, grid, block, 0, s, kp, sp); break;
        case 2: hipLaunchKernelGGL(urtss_sample_recur<2>, grid, block, 0, s, kp, sp); break;
        default: hipLaunchKernelGGL(urtss_sample_recur<4>, grid, block, 0, s, kp, sp); break;
    }
    return abi_check_hip(hipGetLastError(), "urtss_sample_recur launch");
}

}  // namespace ste

extern "C" {
int ste_dbg_sample_lanes(int samples_per_lane) {  // developer instrumentation, not part of the ABI: 1, 2, 4 or 0 (by launch size); returns the old value
    const int old = ste::g_samples_per_lane;
    if (samples_per_lane == 0 || samples_per_lane == 1 || samples_per_lane == 2 || samples_per_lane == 4)
        ste::g_samples_per_lane = samples_per_lane;
    return old;
}
}  // extern "C"
