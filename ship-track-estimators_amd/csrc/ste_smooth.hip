// ste_smooth.hip — the unscented RTS smoothers that start from the rows the forward pass left in rts_work, for gfx950
// (MI355X), and their launches.  fp64 throughout; no MFMA (4x4 contractions); the whole per-track state lives in VGPRs.  No
// kernel of this file declares LDS or synchronises through it.  The stand-alone smoother (urtss_backward_l1, rts_work ==
// NULL) stays in ste_kernels.hip with the forward pass whose device functions it shares; what this file shares with the
// sampler (ste_sample.hip) is in ste_smooth.h, the kernel arguments and the history loads and stores in ste_ukf.h.
//
// Kernels:
//   urtss_recur_l1                       smoother from those rows, one lane per track: gain K = D pinv(P_b), recurrence
//                                        (batches that fill the chip)
//   urtss_recur_l1_plain / _sched_plain  urtss_recur_l1 / urtss_recur_sched for plain batches (ste_ukf.h: plain_batch): packed
//                                        layout, no recorded noise and no position copy compiled in
//   urtss_recur_tn                       the same with per-track Q (ste_ukf_noise_f64), loaded from NoiseParams
//   urtss_recur_sched                    the same body for every window of a scheduled forward launch as one launch: a wave
//                                        per tile, waiting for its own tile's forward pass
//   urtss_gains_all + urtss_recur_lean   the same smoother in two kernels for batches of <= 4 096 tracks: every gain of
//     / urtss_recur_lean_q4              every (step, track) at once, written back into the work rows, then the bare
//                                        recurrence, one lane or one DPP quad per track -- bit-identical to urtss_recur_l1
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
#include "ste_quad.h"

namespace ste {

// ---------------------------------------------------------------------------------------------------------------
// URTSS backward pass from the rows the forward pass left in rts_work: per step the gain K = D pinv(P_b)
// (unscented.py:333) and the recurrence of :337-349,
//     y = x^s_{k+1} - x_b (heading wrapped),  x^s_k = x_k + K y,  P^s_k = P_k + K (P^s_{k+1} - P_b) K^T,
// one lane per track.  Columns 0-1 of D come from the work row, columns 2-3 from the filtered covariance of row k (or the
// work row, at and after the track's first bad square root); x_b and P_b from the work row where they were stored (see
// kWorkD) and otherwise from the filtered rows k and k + 1 the recurrence reads anyway.  Per track-step it reads 8 + 14
// doubles (D; mean and upper triangle of the filtered covariance), plus 14 on the steps that were followed by an
// update, and writes the 20 of the smoothed row.  No LDS, no barriers: the kernel is a chain of ~300 fp64 instructions
// per step whose loads are one row ahead; it is meant to run beside the forward passes of the next batches, whose waves
// take the issue slots it leaves (batch.SmootherPipeline).  Only reads the work rows: repeatable.
// ---------------------------------------------------------------------------------------------------------------
// kShift: the smoother has rates of its own (sog_rate_rts / cog_rate_rts); compiled out for batches that share them.
// kPlain: a plain batch (ste_ukf.h: plain_batch) -- always_full is false, the covariance rows are loaded and stored with the
// packed layout compiled in, and there is no position copy: nothing that is fixed for the launch is tested or kept live
// in the step loop.  Same arithmetic, same bits.
template <bool kShift, bool kTrackNoise = false, bool kPlain = false>
__device__ __forceinline__ void smooth_tile_l1(const KParams& p, const size_t t, const NoiseParams* nz = nullptr) {
    const size_t B = (size_t)p.ld;
    if (t >= (size_t)p.B) return;
    double q4[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (kTrackNoise) track_q4(p, *nz, B, t, q4);
    const int ns = p.nsteps ? p.nsteps[t] : p.Nmax;
    static_assert(!kPlain || !kTrackNoise, "plain batches: the shared-noise entry points only");
    const bool always_full = kPlain ? false : (p.noise_pred || p.noise_upd || p.noise_rts);
    const bool all_eig = (p.tuning & STE_TUNING_EIG_GAINS) != 0;
    const double kappa = (p.m.wi + p.m.wi) * p.m.fan_scale;  // D[:, 2:4] = kappa P_k[:, 2:4] for an exact square root
    // first step at and after which this track's columns 2-3 of D are stored (kNeverBad: never)
    const double first_bad = p.first_bad[t];
    const int last_row = p.Nmax > 0 ? p.Nmax - 1 : 0;
    auto clampk = [&](int k) -> int { return min(max(k, 0), last_row); };

    // row ns: smoothed = filtered; it is also "filtered row k + 1" of the first step
    double xs[4], Ps[10], xn[4], Pn[10];
    const bool packed = kPlain ? true : (p.flags & STE_FLAG_PACKED_COV) != 0;
    load_vec(p.fwd_mean, (size_t)ns, B, t, xs);
    if constexpr (kPlain)
        load_cov_p<true>(p.fwd_cov, (size_t)ns, B, t, Ps);
    else
        load_cov_p(p.fwd_cov, packed, (size_t)ns, B, t, Ps);
    store_vec(p.sm_mean, (size_t)ns, B, t, xs);
    if constexpr (kPlain) {
        store_cov_p<true>(p.sm_cov, (size_t)ns, B, t, Ps);
    } else {
        store_cov_p(p.sm_cov, packed, (size_t)ns, B, t, Ps);
        store_pos(p, (size_t)ns, B, t, xs);
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xn[c] = xs[c];
    STE_UNROLL
    for (int e = 0; e < 10; ++e) Pn[e] = Ps[e];

    // The row of the first step this lane processes and, where that row is full, its stored x_b, P_b: a full row's 14 words
    // are loaded a row ahead too, into the registers x_b and P_b of the current step leave free -- so the update index that
    // says whether a row is full is loaded two rows ahead.
    RecurRow nxt;
    int ui_n = -1, ui_nn = -1;
    double xb[4] = {0.0, 0.0, 0.0, 0.0}, Pb[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ns > 0) {
        load_recur_row<kShift, kPlain>(p, (size_t)(ns - 1), B, t, always_full, nxt);
        ui_n = p.upd_idx[(size_t)(ns - 1) * B + t];
        ui_nn = p.upd_idx[(size_t)clampk(ns - 2) * B + t];
        if (work_row_full(p, ns - 1, ui_n, always_full)) load_stored_xb_pb(p, (size_t)(ns - 1), B, t, xb, Pb);
    }
    // Consumed here, once: nothing pending from the prologue reaches the loop header, so the waits of a step (whose loads are
    // older than the stores of the row before) do not cover those stores (in_vgpr, ste_math.h).
    consume_recur_row<kShift>(always_full, nxt);
    ui_n = in_vgpr(ui_n);
    ui_nn = in_vgpr(ui_nn);
    STE_UNROLL
    for (int c = 0; c < 4; ++c) xb[c] = in_vgpr(xb[c]);
    STE_UNROLL
    for (int e = 0; e < 10; ++e) Pb[e] = in_vgpr(Pb[e]);
    int st = 0;
    for (int k = p.Nmax - 1; k >= 0; --k) {
        if (!__any(k < ns)) continue;  // ragged batch: nobody in this wave has reached its last step yet
        if (k < ns) {
            const RecurRow cur = nxt;
            const bool full = work_row_full(p, k, ui_n, always_full);
            double K[4][4];
            st |= smoother_step_gain<kShift, kTrackNoise, true, kPlain>(p, k, B, t, cur, xn, Pn, full, always_full, all_eig, kappa, first_bad, xb, Pb, K, q4);
            // y = x^s_{k+1} - x_b and dP = P^s_{k+1} - P_b first: x_b, P_b of this step are done with, and their registers take
            // the stored ones of the next step
            double y[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) y[c] = xs[c] - xb[c];
            y[3] = wrap180(y[3]);
            double dP[10];
            STE_UNROLL
            for (int e = 0; e < 10; ++e) dP[e] = Ps[e] - Pb[e];
            // the row of the next step, and its stored x_b, P_b if it is full: in front of this row's stores, in flight during
            // the recurrence arithmetic below and across the loop edge (row 0 again on the last step: in bounds, not used)
            const int kn = clampk(k - 1);
            load_recur_row<kShift, kPlain>(p, (size_t)kn, B, t, always_full, nxt);
            ui_n = ui_nn;
            if (work_row_full(p, kn, ui_n, always_full)) load_stored_xb_pb(p, (size_t)kn, B, t, xb, Pb);
            ui_nn = p.upd_idx[(size_t)clampk(k - 2) * B + t];
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                double acc = cur.xk[r];
                STE_UNROLL
                for (int c = 0; c < 4; ++c) acc = fma(K[r][c], y[c], acc);
                xs[r] = acc;
            }
            xs[3] = floored_mod(xs[3], 360.0);
            // P^s_k = P_k + K (P^s_{k+1} - P_b) K^T, symmetric operands packed
            double KdP[4][4];
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) {
                    double acc = K[r][0] * dP[tix(0, c)];
                    STE_UNROLL
                    for (int i = 1; i < 4; ++i) acc = fma(K[r][i], dP[tix(i, c)], acc);
                    KdP[r][c] = acc;
                }
            }
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = r; c < 4; ++c) {
                    double acc = KdP[r][0] * K[c][0];
                    STE_UNROLL
                    for (int i = 1; i < 4; ++i) acc = fma(KdP[r][i], K[c][i], acc);
                    Ps[tix(r, c)] = cur.Pk[tix(r, c)] + acc;
                }
            }
            store_vec(p.sm_mean, (size_t)k, B, t, xs);
            if constexpr (kPlain) {
                store_cov_p<true>(p.sm_cov, (size_t)k, B, t, Ps);
            } else {
                store_cov_p(p.sm_cov, packed, (size_t)k, B, t, Ps);
                store_pos(p, (size_t)k, B, t, xs);
            }
            // row k becomes "row k + 1" of the next step
            STE_UNROLL
            for (int c = 0; c < 4; ++c) xn[c] = cur.xk[c];
            STE_UNROLL
            for (int e = 0; e < 10; ++e) Pn[e] = cur.Pk[e];
        }
    }
    double chk = 0.0;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) chk += xs[c] * 0.0;
    STE_UNROLL
    for (int e = 0; e < 10; ++e) chk += Ps[e] * 0.0;
    if (!(chk == 0.0)) st |= STE_STATUS_NAN;
    if (st) atomicOr(&p.status[t], st);
}

template <bool kShift>
__global__ __launch_bounds__(64) void urtss_recur_l1(const KParams p) {
    smooth_tile_l1<kShift>(p, (size_t)blockIdx.x * 64 + threadIdx.x);
}
// urtss_recur_l1 for a plain batch (smooth_tile_l1: kPlain).  A kernel of its own name: the general kernels keep theirs.
template <bool kShift>
__global__ __launch_bounds__(64) void urtss_recur_l1_plain(const KParams p) {
    smooth_tile_l1<kShift, false, true>(p, (size_t)blockIdx.x * 64 + threadIdx.x);
}
template <bool kShift>
__global__ __launch_bounds__(64) void urtss_recur_tn(const KParams p, const NoiseParams nz) {
    smooth_tile_l1<kShift, true>(p, (size_t)blockIdx.x * 64 + threadIdx.x, &nz);
}

// The smoothers of every window of a scheduled forward launch as ONE launch (ste_urtss_backward_sched_f64): a wave per
// (window, 64-track tile), in the order the schedule finishes the tiles, each waiting (bounded) for ITS tile's last slice
// -- a tile is smoothed as soon as it has been filtered, not when the last tile of its window has.  The body is
// urtss_recur_l1's.  Waves that wait hold a wave slot each: the launch goes behind a gate on the forward launch's started-wave
// count, so that every forward wave has its SIMD before a waiting smoother wave could be in its way (include/ste.h).
template <bool kShift>
__global__ __launch_bounds__(64) void urtss_recur_sched(const SmoothSchedParams sp) {
    typedef const KParams __attribute__((address_space(4))) ConstKParams;
    const SmoothItem* ip = sp.items + blockIdx.x;
    const int kp = __builtin_amdgcn_readfirstlane(ip->kp), tile = __builtin_amdgcn_readfirstlane(ip->tile);
    const int prog = __builtin_amdgcn_readfirstlane(ip->prog), need = __builtin_amdgcn_readfirstlane(ip->need);
    if (__hip_atomic_load(sp.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ||
        !sched_wait(sp.progress + prog, need, sp.timeout_ticks)) {
        if (threadIdx.x == 0) __hip_atomic_store(sp.error, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const KParams& p = *(const KParams*)(ConstKParams*)(uintptr_t)(sp.kps + kp);
    smooth_tile_l1<kShift>(p, (size_t)tile * 64 + threadIdx.x);
}
// urtss_recur_sched when every window of the table is a plain batch (urtss_recur_l1_plain).  The same lines again, not a
// shared device function: the general kernels keep their code to the byte that way.
template <bool kShift>
__global__ __launch_bounds__(64) void urtss_recur_sched_plain(const SmoothSchedParams sp) {
    typedef const KParams __attribute__((address_space(4))) ConstKParams;
    const SmoothItem* ip = sp.items + blockIdx.x;
    const int kp = __builtin_amdgcn_readfirstlane(ip->kp), tile = __builtin_amdgcn_readfirstlane(ip->tile);
    const int prog = __builtin_amdgcn_readfirstlane(ip->prog), need = __builtin_amdgcn_readfirstlane(ip->need);
    if (__hip_atomic_load(sp.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ||
        !sched_wait(sp.progress + prog, need, sp.timeout_ticks)) {
        if (threadIdx.x == 0) __hip_atomic_store(sp.error, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const KParams& p = *(const KParams*)(ConstKParams*)(uintptr_t)(sp.kps + kp);
    smooth_tile_l1<kShift, false, true>(p, (size_t)tile * 64 + threadIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------
// The same smoother in two kernels, for SMALL batches (a few waves: the real-data runs -- BASELINE configs[0] and [3], the
// reference's 116-ship file).  There a wave of urtss_recur_l1 has a SIMD, indeed most of the chip, to itself, and its step
// is a chain: the loads of x_b / P_b on full rows issued where they are needed, the gain solve (with the eigenvalue route out
// of line for lanes whose P_b is close to singular), then the recurrence -- 4.7 us per step on configs[3].  But only the
// recurrence  x^s_k = x_k + K_k (x^s_{k+1} - x_b),  P^s_k = P_k + K_k (P^s_{k+1} - P_b) K_k^T  is sequential; x_b, P_b and the
// gain K_k = D_k pinv(P_b) depend on the forward pass alone (unscented.py:297-333).  So:
//   urtss_gains_all   one lane per (step, track): x_b, P_b, K for every step of every track at once, written back into the
//                     work row of that step (K over the D columns it was formed from, x_b and P_b into their slots on every row);
//   urtss_recur_lean  one lane per track: loads K, x_b, P_b and the filtered row a step ahead, runs the recurrence.
// Same device functions, same arithmetic, same bits as urtss_recur_l1.  The work rows hold K afterwards: the word that keeps
// a track's first bad square root is stored negated (-(v) - 1) by the second kernel to say so, and a repeated
// ste_urtss_backward_f64 on the same forward result skips the first kernel (the call stays repeatable).  Not for large
// batches: 440 B more traffic per track-step, which a batch that fills the chip cannot afford (launch_backward).
// ---------------------------------------------------------------------------------------------------------------
// kTrackNoise: this lane's track's four entries of Q (track_q4) go to smoother_step_gain; the shared instantiations never read nz.
template <bool kShift, bool kTrackNoise>
__global__ __launch_bounds__(64) void urtss_gains_all(const KParams p, const NoiseParams nz) {
    const size_t B = (size_t)p.ld;
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= (size_t)p.B * (size_t)p.Nmax) return;
    const size_t t = g % (size_t)p.B;
    const int k = (int)(g / (size_t)p.B);
    const int ns = p.nsteps ? p.nsteps[t] : p.Nmax;
    if (k >= ns) return;
    const double fb_raw = p.first_bad[t];
    if (fb_raw < 0.0) return;  // the rows of this track already hold gains (a repeated backward call)
    const bool always_full = p.noise_pred || p.noise_upd || p.noise_rts;
    const bool all_eig = (p.tuning & STE_TUNING_EIG_GAINS) != 0;
    const double kappa = (p.m.wi + p.m.wi) * p.m.fan_scale;
    const bool packed = (p.flags & STE_FLAG_PACKED_COV) != 0;
    RecurRow cur;
    load_recur_row<kShift>(p, (size_t)k, B, t, always_full, cur);
    double xn[4], Pn[10];
    load_vec(p.fwd_mean, (size_t)k + 1, B, t, xn);
    load_cov_p(p.fwd_cov, packed, (size_t)k + 1, B, t, Pn);
    const bool full = work_row_full(p, k, p.upd_idx[(size_t)k * B + t], always_full);
    double xb[4], Pb[10], K[4][4], q4[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (kTrackNoise) track_q4(p, nz, B, t, q4);
    const int st = smoother_step_gain<kShift, kTrackNoise>(p, k, B, t, cur, xn, Pn, full, always_full, all_eig, kappa, fb_raw, xb, Pb, K, q4);
    double* w = p.rts_work + ((size_t)k * kWorkElems) * B + t;
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        w[(kLeanK01 + 2 * r + 0) * B] = K[r][0];
        w[(kLeanK01 + 2 * r + 1) * B] = K[r][1];
        w[(kLeanK23 + 2 * r + 0) * B] = K[r][2];
        w[(kLeanK23 + 2 * r + 1) * B] = K[r][3];
    }
    STE_UNROLL
    for (int c = 0; c < 4; ++c) w[(kWorkXb + c) * B] = xb[c];
    STE_UNROLL
    for (int e = 0; e < 10; ++e) w[(kWorkPb + e) * B] = Pb[e];
    if (st) atomicOr(&p.status[t], st);
}

__global__ __launch_bounds__(64) void urtss_recur_lean(const KParams p) {
    const size_t B = (size_t)p.ld;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const int ns = p.nsteps ? p.nsteps[t] : p.Nmax;
    const bool packed = (p.flags & STE_FLAG_PACKED_COV) != 0;
    const int last_row = p.Nmax > 0 ? p.Nmax - 1 : 0;
    {
        const double fb = p.first_bad[t];
        if (fb >= 0.0) p.first_bad[t] = -fb - 1.0;  // the work rows of this track hold gains from here on (see above)
    }
    double xs[4], Ps[10];
    load_vec(p.fwd_mean, (size_t)ns, B, t, xs);
    load_cov_p(p.fwd_cov, packed, (size_t)ns, B, t, Ps);
    store_vec(p.sm_mean, (size_t)ns, B, t, xs);
    store_cov_p(p.sm_cov, packed, (size_t)ns, B, t, Ps);
    store_pos(p, (size_t)ns, B, t, xs);
    LeanRow nxt;
    if (ns > 0) load_lean_row(p, (size_t)(ns - 1), B, t, packed, nxt);
    for (int k = p.Nmax - 1; k >= 0; --k) {
        if (!__any(k < ns)) continue;
        if (k < ns) {
            const LeanRow cur = nxt;
            load_lean_row(p, (size_t)min(max(k - 1, 0), last_row), B, t, packed, nxt);  // in flight during this step's arithmetic
            double y[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) y[c] = xs[c] - cur.xb[c];
            y[3] = wrap180(y[3]);
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                double acc = cur.xk[r];
                STE_UNROLL
                for (int c = 0; c < 4; ++c) acc = fma(cur.K[r][c], y[c], acc);
                xs[r] = acc;
            }
            xs[3] = floored_mod(xs[3], 360.0);
            double dP[10];
            STE_UNROLL
            for (int e = 0; e < 10; ++e) dP[e] = Ps[e] - cur.Pb[e];
            double KdP[4][4];
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = 0; c < 4; ++c) {
                    double acc = cur.K[r][0] * dP[tix(0, c)];
                    STE_UNROLL
                    for (int i = 1; i < 4; ++i) acc = fma(cur.K[r][i], dP[tix(i, c)], acc);
                    KdP[r][c] = acc;
                }
            }
            STE_UNROLL
            for (int r = 0; r < 4; ++r) {
                STE_UNROLL
                for (int c = r; c < 4; ++c) {
                    double acc = KdP[r][0] * cur.K[c][0];
                    STE_UNROLL
                    for (int i = 1; i < 4; ++i) acc = fma(KdP[r][i], cur.K[c][i], acc);
                    Ps[tix(r, c)] = cur.Pk[tix(r, c)] + acc;
                }
            }
            store_vec(p.sm_mean, (size_t)k, B, t, xs);
            store_cov_p(p.sm_cov, packed, (size_t)k, B, t, Ps);
            store_pos(p, (size_t)k, B, t, xs);
        }
    }
    double chk = 0.0;
    STE_UNROLL
    for (int c = 0; c < 4; ++c) chk += xs[c] * 0.0;
    STE_UNROLL
    for (int e = 0; e < 10; ++e) chk += Ps[e] * 0.0;
    if (!(chk == 0.0)) atomicOr(&p.status[t], STE_STATUS_NAN);
}

// The lean recurrence with ONE DPP QUAD PER TRACK.  A block of a few tracks runs urtss_recur_lean at the pace at which one
// wave issues its ~450 instructions per step (44 loads and 16-22 stores with their 64-bit address arithmetic, ~180 fp64
// operations): 1.3 us per step on configs[3], and neither deeper prefetch nor a run-ahead wave warming L2 nor plain instead
// of nontemporal stores moved it -- it is issue, not latency.  Here lane q of a quad owns row q: K[q][:], x[q], and the part
// (q, c >= q) of the packed covariances; y and dP are broadcast through the quad, the K rows of the lanes to the right come
// by quad rotation: ~60 fp64 operations, 52 DPP moves, 14 loads and <= 9 stores per lane and step.  Every element is
// computed by exactly one lane with urtss_recur_lean's sequence of operations: same bits (tests/test_fleet.py).
struct LeanRowQ {
    double K[4], xb, xk, Pb[4], Pk[4];  // row q of K; element q of x_b and x_k; slot j = element (q, q + j) of P_b and P_k
};
__device__ __forceinline__ int pidx(int r, int c) { return r * 4 - (r * (r - 1)) / 2 + (c - r); }  // tix for r <= c at run time
__device__ __forceinline__ void load_lean_row_q(const KParams& p, size_t k, size_t B, size_t t, int q, bool packed, LeanRowQ& g) {
    const double* w = p.rts_work + (k * kWorkElems) * B + t;
    g.K[0] = w[(size_t)(kLeanK01 + 2 * q + 0) * B];
    g.K[1] = w[(size_t)(kLeanK01 + 2 * q + 1) * B];
    g.K[2] = w[(size_t)(kLeanK23 + 2 * q + 0) * B];
    g.K[3] = w[(size_t)(kLeanK23 + 2 * q + 1) * B];
    g.xb = w[(size_t)(kWorkXb + q) * B];
    g.xk = p.fwd_mean[(k * 4 + (size_t)q) * B + t];
    STE_UNROLL
    for (int j = 0; j < 4; ++j) {
        const int c = min(q + j, 3);  // slots past the row's end repeat its last element and are never used
        g.Pb[j] = w[(size_t)(kWorkPb + pidx(q, c)) * B];
        g.Pk[j] = p.fwd_cov[(packed ? k * 10 + (size_t)pidx(q, c) : k * 16 + (size_t)(q * 4 + c)) * B + t];
    }
}
// x[q], P(q, q + j) -> history row `row` (both triangles of the full layout: the lane that computed (r, c) also stores (c, r))
__device__ __forceinline__ void store_lean_row_q(const KParams& p, size_t row, size_t B, size_t t, int q, bool packed, double x,
                                                 const double (&P)[4]) {
    st_stream(&p.sm_mean[(row * 4 + (size_t)q) * B + t], x);
    if (p.sm_pos && q < 2) st_stream(&p.sm_pos[(row * 2 + (size_t)q) * B + t], x);
    STE_UNROLL
    for (int j = 0; j < 4; ++j) {
        const int c = q + j;
        if (c < 4) {
            if (packed) {
                st_stream(&p.sm_cov[(row * 10 + (size_t)pidx(q, c)) * B + t], P[j]);
            } else {
                st_stream(&p.sm_cov[(row * 16 + (size_t)(q * 4 + c)) * B + t], P[j]);
                if (j) st_stream(&p.sm_cov[(row * 16 + (size_t)(c * 4 + q)) * B + t], P[j]);
            }
        }
    }
}
// value held by lane (q + J) mod 4 of the quad
template <int J>
__device__ __forceinline__ double quad_rot(double v) {
    static_assert(J >= 1 && J <= 3, "quad rotation");
    return dpp_move<(J == 1) ? 0x39 : (J == 2) ? 0x4E : 0x93>(v);  // quad_perm [1,2,3,0] / [2,3,0,1] / [3,0,1,2]
}

__global__ __launch_bounds__(64) void urtss_recur_lean_q4(const KParams p) {
    const size_t B = (size_t)p.ld;
    const int q = threadIdx.x & 3;
    const size_t t = (size_t)blockIdx.x * 16 + (threadIdx.x >> 2);
    if (t >= (size_t)p.B) return;  // whole quads leave
    const int ns = p.nsteps ? p.nsteps[t] : p.Nmax;
    const bool packed = (p.flags & STE_FLAG_PACKED_COV) != 0;
    const int last_row = p.Nmax > 0 ? p.Nmax - 1 : 0;
    if (q == 0) {
        const double fb = p.first_bad[t];
        if (fb >= 0.0) p.first_bad[t] = -fb - 1.0;  // the work rows of this track hold gains from here on (urtss_recur_lean)
    }
    double xs, Ps[4];  // x^s[q]; slot j = P^s(q, q + j)
    xs = p.fwd_mean[((size_t)ns * 4 + (size_t)q) * B + t];
    STE_UNROLL
    for (int j = 0; j < 4; ++j) {
        const int c = min(q + j, 3);
        Ps[j] = p.fwd_cov[(packed ? (size_t)ns * 10 + (size_t)pidx(q, c) : (size_t)ns * 16 + (size_t)(q * 4 + c)) * B + t];
    }
    store_lean_row_q(p, (size_t)ns, B, t, q, packed, xs, Ps);
    LeanRowQ nxt;
    if (ns > 0) load_lean_row_q(p, (size_t)(ns - 1), B, t, q, packed, nxt);
    for (int k = p.Nmax - 1; k >= 0; --k) {
        if (!__any(k < ns)) continue;
        if (k < ns) {
            const LeanRowQ cur = nxt;
            load_lean_row_q(p, (size_t)min(max(k - 1, 0), last_row), B, t, q, packed, nxt);  // in flight during this step
            // y = x^s_{k+1} - x_b, the course difference wrapped (lane 3's element)
            double yq = xs - cur.xb;
            {
                const double yw = wrap180(yq);
                yq = (q == 3) ? yw : yq;
            }
            const double y0 = bcast<0>(yq), y1 = bcast<1>(yq), y2 = bcast<2>(yq), y3 = bcast<3>(yq);
            double acc = cur.xk;
            acc = fma(cur.K[0], y0, acc);
            acc = fma(cur.K[1], y1, acc);
            acc = fma(cur.K[2], y2, acc);
            acc = fma(cur.K[3], y3, acc);
            {
                const double am = floored_mod(acc, 360.0);
                xs = (q == 3) ? am : acc;
            }
            // dP = P^s_{k+1} - P_b on the owner of each element, then the whole symmetric matrix to every lane of the quad
            double d[4];
            STE_UNROLL
            for (int j = 0; j < 4; ++j) d[j] = Ps[j] - cur.Pb[j];
            double dP[10];
            dP[tix(0, 0)] = bcast<0>(d[0]);
            dP[tix(0, 1)] = bcast<0>(d[1]);
            dP[tix(0, 2)] = bcast<0>(d[2]);
            dP[tix(0, 3)] = bcast<0>(d[3]);
            dP[tix(1, 1)] = bcast<1>(d[0]);
            dP[tix(1, 2)] = bcast<1>(d[1]);
            dP[tix(1, 3)] = bcast<1>(d[2]);
            dP[tix(2, 2)] = bcast<2>(d[0]);
            dP[tix(2, 3)] = bcast<2>(d[1]);
            dP[tix(3, 3)] = bcast<3>(d[0]);
            // row q of K dP
            double KdP[4];
            STE_UNROLL
            for (int c = 0; c < 4; ++c) {
                double a2 = cur.K[0] * dP[tix(0, c)];
                STE_UNROLL
                for (int i = 1; i < 4; ++i) a2 = fma(cur.K[i], dP[tix(i, c)], a2);
                KdP[c] = a2;
            }
            // P^s(q, q + j) = P_k(q, q + j) + sum_i KdP[q][i] K[q + j][i]: the K row of the lane j places to the right
            {
                double a2 = KdP[0] * cur.K[0];
                STE_UNROLL
                for (int i = 1; i < 4; ++i) a2 = fma(KdP[i], cur.K[i], a2);
                Ps[0] = cur.Pk[0] + a2;
            }
            {
                const double k0 = quad_rot<1>(cur.K[0]), k1 = quad_rot<1>(cur.K[1]), k2 = quad_rot<1>(cur.K[2]), k3 = quad_rot<1>(cur.K[3]);
                double a2 = KdP[0] * k0;
                a2 = fma(KdP[1], k1, a2);
                a2 = fma(KdP[2], k2, a2);
                a2 = fma(KdP[3], k3, a2);
                Ps[1] = cur.Pk[1] + a2;
            }
            {
                const double k0 = quad_rot<2>(cur.K[0]), k1 = quad_rot<2>(cur.K[1]), k2 = quad_rot<2>(cur.K[2]), k3 = quad_rot<2>(cur.K[3]);
                double a2 = KdP[0] * k0;
                a2 = fma(KdP[1], k1, a2);
                a2 = fma(KdP[2], k2, a2);
                a2 = fma(KdP[3], k3, a2);
                Ps[2] = cur.Pk[2] + a2;
            }
            {
                const double k0 = quad_rot<3>(cur.K[0]), k1 = quad_rot<3>(cur.K[1]), k2 = quad_rot<3>(cur.K[2]), k3 = quad_rot<3>(cur.K[3]);
                double a2 = KdP[0] * k0;
                a2 = fma(KdP[1], k1, a2);
                a2 = fma(KdP[2], k2, a2);
                a2 = fma(KdP[3], k3, a2);
                Ps[3] = cur.Pk[3] + a2;
            }
            store_lean_row_q(p, (size_t)k, B, t, q, packed, xs, Ps);
        }
    }
    double chk = xs * 0.0;
    STE_UNROLL
    for (int j = 0; j < 4; ++j)
        if (q + j < 4) chk += Ps[j] * 0.0;
    if (!(chk == 0.0)) atomicOr(&p.status[t], STE_STATUS_NAN);
}

// ===============================================================================================================
// launches (declared in ste_err.h; launch_backward and the entry points are in ste_kernels.hip)
// ===============================================================================================================
// Batches of at most this many tracks smooth with the two-kernel form (urtss_gains_all + urtss_recur_lean): up to there the
// one-kernel smoother is a few waves running a latency chain of ~1.5-4.7 us per step, and the extra 440 B per track-step of
// the gains pass cost less than the chain they remove; a batch that fills the chip is bound by bytes and issue instead.
// STE_TUNING_TWO_KERNEL_SMOOTHER forces the two-kernel form, STE_TUNING_ONE_KERNEL_SMOOTHER the one-kernel form (tests,
// measurements); the choice must not change between the backward calls made on one forward result (the first two-kernel call
// turns the work rows into gains).
constexpr int kLeanSmootherMaxTracks = 4096;
bool lean_smoother(const KParams& kp) {
    return kp.rts_work && kp.Nmax > 0 && ((kp.tuning & STE_TUNING_TWO_KERNEL_SMOOTHER) || (!(kp.tuning & STE_TUNING_ONE_KERNEL_SMOOTHER) && kp.B <= kLeanSmootherMaxTracks));
}

// The smoothers that read the work rows (kp.rts_work is set).  `np`: per-track noise, or NULL.  The smoother reads Q alone:
// without a per-track Q it takes the shared instantiations, and the lean recurrences read no Q at all.
int launch_backward_work(const KParams& kp, const NoiseParams* np, hipStream_t s) {
    const dim3 grid((unsigned)((kp.B + 63) / 64)), block(64);
    const bool shift = kp.sog_rate_rts || kp.cog_rate_rts, tn = np && np->Q;
    const NoiseParams nz = tn ? *np : NoiseParams{nullptr, nullptr};
    auto with_shift_tn = [&](auto&& f) { with_bool(shift, [&](auto sh) { with_bool(tn, [&](auto t) { f(sh, t); }); }); };
    if (lean_smoother(kp)) {
        const dim3 ggrid((unsigned)(((size_t)kp.B * (size_t)kp.Nmax + 63) / 64));
        with_shift_tn([&](auto sh, auto t) {
            hipLaunchKernelGGL((urtss_gains_all<decltype(sh)::value, decltype(t)::value>), ggrid, block, 0, s, kp, nz);
        });
        int rc = abi_check_hip(hipGetLastError(), "urtss_gains_all launch");
        if (rc) return rc;
        // the recurrence: a quad per track (16 tracks per wave); STE_TUNING_LANE_RECURRENCE keeps the lane-per-track form
        if (kp.tuning & STE_TUNING_LANE_RECURRENCE)
            hipLaunchKernelGGL(urtss_recur_lean, grid, block, 0, s, kp);
        else
            hipLaunchKernelGGL(urtss_recur_lean_q4, dim3((unsigned)((kp.B + 15) / 16)), block, 0, s, kp);
        return abi_check_hip(hipGetLastError(), "urtss_recur_lean launch");
    }
    with_shift_tn([&](auto sh, auto t) {
        if constexpr (decltype(t)::value)
            hipLaunchKernelGGL(urtss_recur_tn<decltype(sh)::value>, grid, block, 0, s, kp, nz);
        else if (!np && plain_batch(kp))
            hipLaunchKernelGGL(urtss_recur_l1_plain<decltype(sh)::value>, grid, block, 0, s, kp);
        else
            hipLaunchKernelGGL(urtss_recur_l1<decltype(sh)::value>, grid, block, 0, s, kp);
    });
    return abi_check_hip(hipGetLastError(), "urtss_recur launch");
}

// The launch of ste_urtss_backward_sched_f64: a wave per item of the table that entry point has built and uploaded.
// `plain`: every window of the table is a plain batch (ste_ukf.h: plain_batch).
int launch_recur_sched(bool shift, bool plain, int nitems, const SmoothSchedParams& sp, hipStream_t s) {
    with_bool(shift, [&](auto sh) {
        if (plain)
            hipLaunchKernelGGL(urtss_recur_sched_plain<decltype(sh)::value>, dim3((unsigned)nitems), dim3(64), 0, s, sp);
        else
            hipLaunchKernelGGL(urtss_recur_sched<decltype(sh)::value>, dim3((unsigned)nitems), dim3(64), 0, s, sp);
    });
    return abi_check_hip(hipGetLastError(), "urtss_recur_sched launch");
}

}  // namespace ste
