// ste_ukf.h — what the translation units of the UKF / URTSS kernels (ste_kernels.hip, ste_forward_quad.hip, ste_smooth.hip,
// ste_sample.hip) share: the kernel arguments, the work-row layout, the bounded wait of the scheduled launches, and the loads
// and stores of the SoA histories (track index fastest, so a wave's accesses are contiguous runs).  Everything here is
// inlined into its callers: the library is built without relocatable device code, each .hip is a code object of its own,
// and a kernel is instantiated in the one file that launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_math.h"
#include "ste_lane.h"

namespace ste {

struct KParams {
    int B, Nmax, Tmax;
    unsigned flags;
    int tuning;
    int fast_upd;  // H = diag(1, 1, 0, 0), R confined to the same block: closed-form update (and closed-form robust rescaling)
    Mats m;
    const int32_t* nsteps;
    const double* x0;
    const double* P0;
    const double* dt;
    const double* sog_rate;
    const double* cog_rate;
    const double* sog_rate_rts;
    const double* cog_rate_rts;
    const int32_t* upd_idx;
    const double* z;
    const double* noise_pred;
    const double* noise_upd;
    const double* noise_rts;
    double* fwd_mean;
    double* fwd_cov;
    double* sm_mean;
    double* sm_cov;
    int32_t* status;
    double* rts_work;  // [Nmax][kWorkElems][ld] smoother gains produced by the forward pass, or nullptr
    int ld;            // tracks per row of every per-track array (ste.h: track_stride; = B for a batch of its own)
    int k0;            // forward pass, time slices: absolute index of this launch's step 0 (0 for a whole pass); every
                       // per-step pointer above already names row k0, Nmax is the slice's length (see slice_params)
    int qpw;           // quad forward kernel: quads (tracks) per wave, 1 .. 16 (launch_forward: fewer when waves are scarce)
    double* first_bad; // [ld] the last row of rts_work (first bad square root per track), or nullptr
    double* sm_pos;    // [Nmax+1][2][ld] smoothed lon / lat beside sm_mean, or nullptr
};

// kTrackNoise: per-track Q and R (ste_ukf_noise_f64), a further kernel argument of the *_tn entry kernels: upper triangles
// [10][ld] in the order of STE_FLAG_PACKED_COV, track index fastest; nullptr = the shared matrix of KParams.  Q goes into
// the ten Qv registers once per track (forward) or is read once per track before the backward loop (smoothers); R is
// read at each update (lane_update / ukf_update).
struct NoiseParams {
    const double* Q;
    const double* R;
};

// The scheduled smoother (ste_urtss_backward_sched_f64 builds the table in ste_kernels.hip, urtss_recur_sched of ste_smooth.hip
// reads it): one item per (window, 64-track tile), and the kernel's arguments.
struct SmoothItem {
    int kp;    // index of the window's parameter block
    int tile;  // 64-track tile of that window
    int prog;  // index of the tile's progress counter (the forward launch's)
    int need;  // slices of a forward pass of that window: the count the tile's counter reaches
};
struct SmoothSchedParams {
    const KParams* kps;
    const SmoothItem* items;
    const int* progress;
    int* error;  // 2 = a smoother wave waited longer than its bound
    unsigned long long timeout_ticks;
};

// ste.h flags are 8 bits wide; this one is set by slice_params only: the launch continues a forward pass at step k0 > 0
constexpr unsigned kFlagContinue = 0x10000u;

// A kernel argument fetched where it is used (volatile: neither merged with an earlier load of the same word nor hoisted).
// The forward kernels sit at the edge of both register files; an argument kept live across the step loop for one rare use
// costs spills inside the loop (with the slice offset held in a scalar register: 62 instead of 12 lane reads per step).
__device__ __forceinline__ int late_k0() {
    typedef const char __attribute__((address_space(4))) * kptr;
    kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    return *(const volatile int __attribute__((address_space(4)))*)(ka + offsetof(KParams, k0));
}

// wave-uniform: spin (sleeping) until *flag >= need or the bound is reached
__device__ __forceinline__ bool sched_wait(const int* flag, int need, unsigned long long timeout_ticks) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > timeout_ticks) return false;
            __builtin_amdgcn_s_sleep(64);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}

constexpr int kColdEvery = 64;  // power of two

// rts_work row layout (round 3): columns 0-1 of D, row-major 4 x 2 (8) | x_b (4) | P_b upper triangle, row-major (10) |
// columns 2-3 of D, row-major 4 x 2 (8).
// The smoother's step k (unscented.py:297-333) starts from the same filtered state as the forward predict of step k, with
// the same dt and rates, so its fan, its back-prediction x_b, its P_b and its cross-covariance D are values the predict
// already holds: the forward kernels leave them here and the backward pass is the gain solve K = D pinv(P_b) (:333) plus
// the recurrence (:337-349).  What is written is only what cannot be had cheaper:
//   * x_b and P_b only for the steps where they do not follow from the filtered history -- steps followed by a
//     measurement update, row 0 when the run starts with an update, every step of a run with recorded noise; elsewhere
//     x_b = fwd_mean[k + 1] and P_b = fwd_cov[k + 1] + b b^T with b = fwd_mean[k + 1] - fwd_mean[k];
//   * columns 2-3 of D only at and after a track's first clamped / unconverged square root: speed and heading pass
//     through the process model with unit slope (non_linear_process.py:74-75), so D[:, 2:4] = 2 wi (T T)[:, 2:4], which for
//     an exact T = sqrtm(scale P_k) is (2 wi scale) P_k[:, 2:4] -- the filtered covariance the smoother reads anyway.
//     The step index of that first bad square root is kept, as a double, in the B words that follow the Nmax rows
//     (kNeverBad when there is none): the smoother never looks at status[], one kernel smooths every track.
constexpr int kWorkD = 0, kWorkXb = 8, kWorkPb = 12, kWorkD23 = 22, kWorkElems = STE_RTS_WORK_ROWS;
static_assert(kWorkElems == 30, "include/ste.h: STE_RTS_WORK_ROWS");
constexpr double kNeverBad = 1e300;

__device__ __forceinline__ void load_mat(const double* base, size_t row, size_t B, size_t t, double (&M)[4][4]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) M[r][c] = base[(row * 16 + r * 4 + c) * B + t];
    }
}
// Histories and work rows are written once and read by another kernel milliseconds later: nontemporal stores (no change at
// round 2's 1.01 ms per step; +1.2 % now that the pipeline moves 3.7 TB/s: 7.48 -> 7.57e9 track-steps/s, same box, twice;
// nontemporal loads on the smoother's side: nothing).
__device__ __forceinline__ void st_stream(double* p, double v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_mat(double* base, size_t row, size_t B, size_t t, const double (&M)[4][4]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) st_stream(&base[(row * 16 + r * 4 + c) * B + t], M[r][c]);
    }
}
__device__ __forceinline__ void load_vec(const double* base, size_t row, size_t B, size_t t, double (&v)[4]) {
    STE_UNROLL
    for (int c = 0; c < 4; ++c) v[c] = base[(row * 4 + c) * B + t];
}
__device__ __forceinline__ void store_vec(double* base, size_t row, size_t B, size_t t, const double (&v)[4]) {
    STE_UNROLL
    for (int c = 0; c < 4; ++c) st_stream(&base[(row * 4 + c) * B + t], v[c]);
}

__device__ __forceinline__ void store_pos(const KParams& p, size_t row, size_t B, size_t t, const double (&xs)[4]) {
    if (p.sm_pos) {  // the tensor configs[2] exchanges between GPUs: smoothed lon / lat on their own (ste.h: sm_pos)
        st_stream(&p.sm_pos[(row * 2 + 0) * B + t], xs[0]);
        st_stream(&p.sm_pos[(row * 2 + 1) * B + t], xs[1]);
    }
}

// A "plain batch": packed covariances, no recorded noise, no position copy -- DeviceBatch's default, and what the benchmark,
// run_fleet and the CLI launch.  All three are facts of the launch that the general step loops test at every step (and keep
// a pointer live for); the host picks kernels with them compiled in (kPlain of forward_tile_l1 / smooth_tile_l1).
inline bool plain_batch(const KParams& kp) {
    return (kp.flags & STE_FLAG_PACKED_COV) && !kp.noise_pred && !kp.noise_upd && !kp.noise_rts && !kp.sm_pos;
}

// Covariance histories (fwd_cov, sm_cov) come in two layouts: [row][16][B] full 4 x 4 matrices, the reference's return
// shape, or -- STE_FLAG_PACKED_COV -- [row][10][B] upper triangles (row-major: 00 01 02 03 11 12 13 22 23 33).  The
// matrices are symmetric by construction, so the packed form loses nothing; it takes 48 of 128 bytes off every history
// row written and lets the host expand on its way out (DeviceBatch.download).
__device__ __forceinline__ size_t cov_at(bool packed, size_t row, int r, int c) {  // r <= c
    return packed ? row * 10 + (size_t)(r * 4 - (r * (r - 1)) / 2 + (c - r)) : row * 16 + (size_t)(r * 4 + c);
}
// packed symmetric -> history row
__device__ __forceinline__ void store_cov_p(double* base, bool packed, size_t row, size_t B, size_t t, const double (&P)[10]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) st_stream(&base[cov_at(packed, row, r, c) * B + t], P[tix(r, c)]);
    }
    if (!packed) {
        STE_UNROLL
        for (int r = 1; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < r; ++c) st_stream(&base[(row * 16 + r * 4 + c) * B + t], P[tix(r, c)]);
        }
    }
}
__device__ __forceinline__ void load_cov_p(const double* base, bool packed, size_t row, size_t B, size_t t, double (&P)[10]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) P[tix(r, c)] = base[cov_at(packed, row, r, c) * B + t];
    }
}
// The same three with the layout as a template argument, for the "plain batch" step loops (plain_batch below).  With a
// run-time `packed` the six entries whose packed and full indices differ cost a 64-bit (row_sel + const) * B each, per row;
// with the layout compiled in every entry is the one before it plus B.
template <bool kPacked>
__device__ __forceinline__ size_t cov_at(size_t row, int r, int c) {  // r <= c
    return kPacked ? row * 10 + (size_t)(r * 4 - (r * (r - 1)) / 2 + (c - r)) : row * 16 + (size_t)(r * 4 + c);
}
template <bool kPacked>
__device__ __forceinline__ void store_cov_p(double* base, size_t row, size_t B, size_t t, const double (&P)[10]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) st_stream(&base[cov_at<kPacked>(row, r, c) * B + t], P[tix(r, c)]);
    }
    if (!kPacked) {
        STE_UNROLL
        for (int r = 1; r < 4; ++r) {
            STE_UNROLL
            for (int c = 0; c < r; ++c) st_stream(&base[(row * 16 + r * 4 + c) * B + t], P[tix(r, c)]);
        }
    }
}
template <bool kPacked>
__device__ __forceinline__ void load_cov_p(const double* base, size_t row, size_t B, size_t t, double (&P)[10]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = r; c < 4; ++c) P[tix(r, c)] = base[cov_at<kPacked>(row, r, c) * B + t];
    }
}
// full 4 x 4 <-> history row (the literal kernels); the packed layout keeps the upper triangle
__device__ __forceinline__ void store_cov_m(double* base, bool packed, size_t row, size_t B, size_t t, const double (&M)[4][4]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            if (c >= r)
                st_stream(&base[cov_at(packed, row, r, c) * B + t], M[r][c]);
            else if (!packed)
                st_stream(&base[(row * 16 + r * 4 + c) * B + t], M[r][c]);
        }
    }
}
__device__ __forceinline__ void load_cov_m(const double* base, bool packed, size_t row, size_t B, size_t t, double (&M)[4][4]) {
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) {
            if (packed)
                M[r][c] = base[cov_at(true, row, r < c ? r : c, r < c ? c : r) * B + t];
            else
                M[r][c] = base[(row * 16 + r * 4 + c) * B + t];
        }
    }
}

__device__ __forceinline__ bool all_finite(const double (&x)[4], const double (&P)[4][4]) {
    double acc = 0.0;
    STE_UNROLL
    for (int r = 0; r < 4; ++r) {
        acc += x[r] * 0.0;
        STE_UNROLL
        for (int c = 0; c < 4; ++c) acc += P[r][c] * 0.0;
    }
    return acc == 0.0;  // inf*0 and nan*0 are NaN
}

}  // namespace ste
