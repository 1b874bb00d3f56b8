// ste_noisefit.hip — the M-step of an EM fit of the measurement noise R (include/ste.h: ste_ukf_noise_moments_f64,
// ste_ukf_noise_mstep_f64).  The E-step is the forward pass and the smoother the library already has; what the M-step needs
// of them, the smoothed marginals, is on the device when the smoother ends.  The header carries the definitions and
// tests/noise_fit_cases.py restates both kernels in NumPy, bit for bit.
//
//   noise_moments<packed>   a lane per track, one sequential pass over the track's steps: for every update the residual of
//                           its observation against the smoothed row the update produced, and H P^s H^T, summed in step
//                           order.  Nothing is contracted, so NumPy reproduces the bits.  A wave of a 10 000-track batch is
//                           one of 157 on 1 024 SIMDs, alone on its SIMD and bound by the latency of its loads: upd_idx is
//                           read kAhead steps at a time, the next group of them in flight during the arithmetic of the
//                           current one, and the 18 loads of an update's rows (mean 4, observation 4, upper triangle 10) are issued together.
//   noise_mstep_groups      a wave per group: strided partial sums per lane, a fixed shuffle tree, the projection in lane 0,
//                           the group's triangle stored to every member.  The order of the additions is fixed, so R -- and
//                           every history computed with it -- has the same bits in every run.
//   noise_mstep_tracks      every track a group of its own: a lane per track.
// Every output has one writer: plain vector stores.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_math.h"

#pragma clang fp contract(off)  // every expression as written: the restatement in NumPy has no fma

namespace ste {
namespace {

constexpr int kAhead = 8;  // steps whose upd_idx is loaded at once

struct MomentParams {
    int B, Nmax, Tmax;
    size_t ld;              // tracks per row (track_stride, or B)
    double H[16];           // kernel arguments: scalar registers
    const int32_t* nsteps;  // [B] or nullptr
    const int32_t* upd_idx; // [Nmax][ld]
    const int32_t* status;  // [B] or nullptr
    const double* z;        // [Tmax][4][ld]
    const double* sm_mean;  // [Nmax+1][4][ld]
    const double* sm_cov;   // [Nmax+1][10 or 16][ld]
    double* moments;        // [10][ld]
    int32_t* count;         // [ld]
    double* vsum;           // [4][ld] or nullptr
    int32_t* track_status;  // [B] or nullptr
};

// index of (r, c), r <= c, in a packed symmetric 4x4: 00 01 02 03 11 12 13 22 23 33
__host__ __device__ constexpr int tri(int r, int c) { return r * 4 - (r * (r - 1)) / 2 + (c - r); }

template <bool kPacked>
__global__ __launch_bounds__(64) void noise_moments(const MomentParams p) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const size_t ld = p.ld;
    int tst = 0;
    if (p.status && (p.status[t] & STE_STATUS_NAN)) tst = STE_NOISE_TRACK_NAN;
    const int ns = tst ? 0 : track_steps(p, t);
    constexpr int kCovRows = kPacked ? 10 : 16;

    double S[10], vs[4] = {0.0, 0.0, 0.0, 0.0};
    STE_UNROLL
    for (int e = 0; e < 10; ++e) S[e] = 0.0;
    int n = 0;
    bool finite = true;

    // upd_idx of steps [k0, k0 + kAhead): rows past Nmax do not exist, steps past ns are no updates
    auto load_idx = [&](int k0, int (&ui)[kAhead]) {
        STE_UNROLL
        for (int j = 0; j < kAhead; ++j) {
            const int k = k0 + j;
            ui[j] = k < ns ? p.upd_idx[(size_t)k * ld + t] : -1;  // ns <= Nmax
        }
    };
    int nxt[kAhead];
    load_idx(0, nxt);
    for (int k0 = 0; __any(k0 < ns); k0 += kAhead) {
        int cur[kAhead];
        STE_UNROLL
        for (int j = 0; j < kAhead; ++j) cur[j] = nxt[j];
        load_idx(k0 + kAhead, nxt);  // in flight during this group's arithmetic
        // one copy of the body: the wave waits for loads, it does not issue, and kAhead copies would only be more code
#pragma unroll 1
        for (int j = 0; j < kAhead; ++j) {
            int ui = cur[0];  // cur[j] by selects: j is the wave's, and the array stays in registers
            STE_UNROLL
            for (int i = 1; i < kAhead; ++i) ui = j == i ? cur[i] : ui;
            const bool upd = ui >= 0 && ui < p.Tmax;  // cur[j] is -1 for k >= ns
            if (!__any(upd)) continue;
            if (upd) {
                const size_t row = (size_t)(k0 + j) + 1;  // <= ns <= Nmax
                const double* mp = p.sm_mean + (row * 4) * ld + t;
                const double* cp = p.sm_cov + (row * kCovRows) * ld + t;
                const double* zp = p.z + ((size_t)ui * 4) * ld + t;
                double m[4], z[4], P[10];
                STE_UNROLL
                for (int c = 0; c < 4; ++c) {
                    m[c] = mp[(size_t)c * ld];
                    z[c] = zp[(size_t)c * ld];
                }
                STE_UNROLL
                for (int r = 0; r < 4; ++r) {
                    STE_UNROLL
                    for (int c = r; c < 4; ++c) P[tri(r, c)] = cp[(size_t)(kPacked ? tri(r, c) : r * 4 + c) * ld];
                }
                double v[4];
                STE_UNROLL
                for (int r = 0; r < 4; ++r) {
                    const double hm = ((p.H[r * 4 + 0] * m[0] + p.H[r * 4 + 1] * m[1]) + p.H[r * 4 + 2] * m[2]) + p.H[r * 4 + 3] * m[3];
                    v[r] = z[r] - hm;
                }
                v[3] = wrap180(v[3]);
                STE_UNROLL
                for (int r = 0; r < 4; ++r) {
                    double G[4];  // row r of H P
                    STE_UNROLL
                    for (int c = 0; c < 4; ++c) {
                        auto Pe = [&](int i) { return P[i <= c ? tri(i, c) : tri(c, i)]; };
                        G[c] = ((p.H[r * 4 + 0] * Pe(0) + p.H[r * 4 + 1] * Pe(1)) + p.H[r * 4 + 2] * Pe(2)) + p.H[r * 4 + 3] * Pe(3);
                    }
                    STE_UNROLL
                    for (int c = r; c < 4; ++c) {
                        const double gh = ((G[0] * p.H[c * 4 + 0] + G[1] * p.H[c * 4 + 1]) + G[2] * p.H[c * 4 + 2]) + G[3] * p.H[c * 4 + 3];
                        const double term = v[r] * v[c] + gh;
                        finite = finite && (term * 0.0 == 0.0);
                        S[tri(r, c)] = S[tri(r, c)] + term;
                    }
                }
                STE_UNROLL
                for (int c = 0; c < 4; ++c) vs[c] = vs[c] + v[c];
                ++n;
            }
        }
    }
    if (!finite) tst |= STE_NOISE_TRACK_NOT_FINITE;
    const bool usable = tst == 0;
    STE_UNROLL
    for (int e = 0; e < 10; ++e) p.moments[(size_t)e * ld + t] = usable ? S[e] : 0.0;
    p.count[t] = usable ? n : 0;
    if (p.vsum) {
        STE_UNROLL
        for (int c = 0; c < 4; ++c) p.vsum[(size_t)c * ld + t] = usable ? vs[c] : 0.0;
    }
    if (p.track_status) p.track_status[t] = tst;
}

struct MstepParams {
    int ntracks, ngroups, nmembers, structure;
    size_t ld;
    const double* moments;         // [10][ld]
    const int32_t* count;          // [ld]
    const int32_t* group_offsets;  // [G + 1] or nullptr
    const int32_t* group_members;  // [nmembers] or nullptr
    double* R_group;               // [10][G]
    int32_t* n_group;              // [G]
    int32_t* group_status;         // [G]
    double* R_tracks;              // [10][ld]
};

// The projection of the sums (entries 00, 01, 11) over n onto `structure`: the triangle's three entries that can be non-zero,
// and the status of the group.
__device__ __forceinline__ int project(int structure, double s00, double s01, double s11, int n, double& r00, double& r01,
                                       double& r11) {
    const double dn = (double)n;
    const double m00 = s00 / dn, m01 = s01 / dn, m11 = s11 / dn;
    if (structure == STE_NOISE_FIT_SCALAR) {
        r00 = r11 = (m00 + m11) / 2.0;
        r01 = 0.0;
    } else if (structure == STE_NOISE_FIT_DIAG2) {
        r00 = m00;
        r11 = m11;
        r01 = 0.0;
    } else {
        r00 = m00;
        r01 = m01;
        r11 = m11;
    }
    int st = n == 0 ? STE_NOISE_GROUP_EMPTY : 0;
    if (!(r00 > 0.0 && r00 * 0.0 == 0.0 && r11 > 0.0 && r11 * 0.0 == 0.0 && r01 * 0.0 == 0.0)) st |= STE_NOISE_GROUP_BAD_VARIANCE;
    return st;
}

// entry e of the triangle (r00, r01, 0, 0, r11, 0, 0, 0, 0, 0)
__device__ __forceinline__ double tri_entry(int e, double r00, double r01, double r11) {
    return e == 0 ? r00 : (e == 1 ? r01 : (e == 4 ? r11 : 0.0));
}

__global__ __launch_bounds__(64) void noise_mstep_groups(const MstepParams p) {
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (g >= p.ngroups) return;
    const int lo = min(max(p.group_offsets[g], 0), p.nmembers);
    const int hi = min(max(p.group_offsets[g + 1], lo), p.nmembers);
    double s00 = 0.0, s01 = 0.0, s11 = 0.0;
    int n = 0, bad = 0;
    for (int i = lo + lane; i < hi; i += 64) {
        const int t = p.group_members[i];
        if (t < 0 || t >= p.ntracks) {
            bad = 1;
            continue;
        }
        s00 = s00 + p.moments[(size_t)tri(0, 0) * p.ld + t];
        s01 = s01 + p.moments[(size_t)tri(0, 1) * p.ld + t];
        s11 = s11 + p.moments[(size_t)tri(1, 1) * p.ld + t];
        n = n + p.count[t];
    }
    STE_UNROLL
    for (int off = 32; off >= 1; off >>= 1) {  // lane l < off: its own value + lane l + off's
        s00 = s00 + __shfl_down(s00, off, 64);
        s01 = s01 + __shfl_down(s01, off, 64);
        s11 = s11 + __shfl_down(s11, off, 64);
        n = n + __shfl_down(n, off, 64);
    }
    double r00, r01, r11;
    int st = project(p.structure, s00, s01, s11, n, r00, r01, r11);  // lane 0's is the group's
    r00 = __shfl(r00, 0, 64);
    r01 = __shfl(r01, 0, 64);
    r11 = __shfl(r11, 0, 64);
    st = __shfl(st, 0, 64) | (__any(bad) ? STE_NOISE_GROUP_BAD_MEMBER : 0);
    n = __shfl(n, 0, 64);
    if (lane < 10) p.R_group[(size_t)lane * p.ngroups + g] = tri_entry(lane, r00, r01, r11);
    if (lane == 0) {
        p.n_group[g] = n;
        p.group_status[g] = st;
    }
    if (st & (STE_NOISE_GROUP_EMPTY | STE_NOISE_GROUP_BAD_VARIANCE)) return;
    for (int i = lo + lane; i < hi; i += 64) {
        const int t = p.group_members[i];
        if (t < 0 || t >= p.ntracks) continue;
        STE_UNROLL
        for (int e = 0; e < 10; ++e) p.R_tracks[(size_t)e * p.ld + t] = tri_entry(e, r00, r01, r11);
    }
}

__global__ __launch_bounds__(64) void noise_mstep_tracks(const MstepParams p) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.ntracks) return;
    const double s00 = 0.0 + p.moments[(size_t)tri(0, 0) * p.ld + t];
    const double s01 = 0.0 + p.moments[(size_t)tri(0, 1) * p.ld + t];
    const double s11 = 0.0 + p.moments[(size_t)tri(1, 1) * p.ld + t];
    const int n = p.count[t];
    double r00, r01, r11;
    const int st = project(p.structure, s00, s01, s11, n, r00, r01, r11);
    STE_UNROLL
    for (int e = 0; e < 10; ++e) p.R_group[(size_t)e * p.ngroups + t] = tri_entry(e, r00, r01, r11);
    p.n_group[t] = n;
    p.group_status[t] = st;
    if (st) return;
    STE_UNROLL
    for (int e = 0; e < 10; ++e) p.R_tracks[(size_t)e * p.ld + t] = tri_entry(e, r00, r01, r11);
}

}  // namespace
}  // namespace ste

extern "C" int ste_ukf_noise_moments_f64(const ste_ukf_batch_f64* b, const ste_noise_moments_f64* nm, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_ukf_noise_moments_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!nm) return refuse("the moment arguments (nm) are NULL");
    if (b->B <= 0 || b->Nmax < 0 || b->Tmax < 1) return refuse("B must be > 0, Nmax >= 0 and Tmax >= 1");
    if (int rc = refuse.stride(b)) return rc;
    if (!nm->moments || !nm->count) return refuse("nm->moments and nm->count are required");
    if (nm->flags != 0 || nm->reserved != 0) return refuse("nm->flags and nm->reserved must be 0");
    if (!b->H) return refuse("the batch's H is required");
    if (!b->sm_mean || !b->sm_cov)
        return refuse("sm_mean and sm_cov are required (the moments are taken about the smoothed track)");
    if (!b->z || !b->upd_idx) return refuse("z and upd_idx are required");
    if (b->flags & STE_FLAG_ROBUST)
        return refuse("STE_FLAG_ROBUST is refused (the filter rescales R per update; the M-step is not defined for it)");
    if (b->noise_upd)
        return refuse("recorded noise is refused (noise_upd: the update saw z + noise, the residual is taken from z)");
    if (b->step_begin != 0 || (b->step_end != 0 && b->step_end != b->Nmax))
        return refuse("time slices are refused (step_begin / step_end): the moments are those of whole passes");
    MomentParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.Tmax = b->Tmax;
    p.ld = track_ld(b);
    for (int i = 0; i < 16; ++i) p.H[i] = b->H[i];
    p.nsteps = b->nsteps;
    p.upd_idx = b->upd_idx;
    p.status = b->status;
    p.z = b->z;
    p.sm_mean = b->sm_mean;
    p.sm_cov = b->sm_cov;
    p.moments = nm->moments;
    p.count = nm->count;
    p.vsum = nm->vsum;
    p.track_status = nm->track_status;
    const dim3 grid((unsigned)((p.B + 63) / 64)), block(64);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (b->flags & STE_FLAG_PACKED_COV) hipLaunchKernelGGL(noise_moments<true>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(noise_moments<false>, grid, block, 0, s, p);
    return abi_check_hip(hipGetLastError(), "noise_moments launch");
}

extern "C" int ste_ukf_noise_mstep_f64(const ste_noise_mstep_f64* ms, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_ukf_noise_mstep_f64"};
    if (!ms) return refuse("the M-step arguments (ms) are NULL");
    if (ms->ntracks <= 0 || ms->ngroups <= 0 || ms->nmembers < 0)
        return refuse("ntracks and ngroups must be > 0 and nmembers >= 0");
    if (ms->ld != 0 && ms->ld < ms->ntracks) return refuse("ld must be 0 or >= ntracks");
    if (!ms->moments || !ms->count) return refuse("ms->moments and ms->count are required");
    if (!ms->R_group || !ms->n_group || !ms->group_status || !ms->R_tracks)
        return refuse("ms->R_group, ms->n_group, ms->group_status and ms->R_tracks are required");
    if (!ms->group_offsets != !ms->group_members)
        return refuse("group_offsets and group_members come together (both NULL: every track a group of its own)");
    if (!ms->group_offsets && ms->ngroups != ms->ntracks)
        return refuse("without groups every track is a group: ngroups must equal ntracks");
    if (ms->structure != STE_NOISE_FIT_SCALAR && ms->structure != STE_NOISE_FIT_DIAG2 && ms->structure != STE_NOISE_FIT_BLOCK2)
        return refuse("ms->structure must be STE_NOISE_FIT_SCALAR, _DIAG2 or _BLOCK2");
    if (ms->reserved != 0) return refuse("ms->reserved must be 0");
    MstepParams p;
    p.ntracks = ms->ntracks;
    p.ngroups = ms->ngroups;
    p.nmembers = ms->nmembers;
    p.structure = ms->structure;
    p.ld = (size_t)(ms->ld ? ms->ld : ms->ntracks);
    p.moments = ms->moments;
    p.count = ms->count;
    p.group_offsets = ms->group_offsets;
    p.group_members = ms->group_members;
    p.R_group = ms->R_group;
    p.n_group = ms->n_group;
    p.group_status = ms->group_status;
    p.R_tracks = ms->R_tracks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ms->group_offsets) hipLaunchKernelGGL(noise_mstep_groups, dim3((unsigned)p.ngroups), dim3(64), 0, s, p);
    else hipLaunchKernelGGL(noise_mstep_tracks, dim3((unsigned)((p.ntracks + 63) / 64)), dim3(64), 0, s, p);
    return abi_check_hip(hipGetLastError(), "noise_mstep launch");
}
