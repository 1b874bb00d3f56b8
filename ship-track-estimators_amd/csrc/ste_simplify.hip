// ste_simplify.hip — tracks that stay on the device made smaller within a tolerance (include/ste.h: ste_track_simplify_f64): the
// time-aware Douglas-Peucker rule (the deviation of a row from the chord between its surviving neighbours, taken at the row's own
// time) and, with STE_SIMPLIFY_SHAPE, the classic perpendicular one; keep flags, counts and the kept rows compacted into a fleet
// of their own, for S tracks per ship (the sampler's output, or sm_mean / fwd_mean as S = 1).  The header carries the definition
// and tests/simplify_cases.py restates it in NumPy, bit for bit.
//
//   track_simplify<shape, work>   a WAVE per (sample, track) item, a block is one wave (the mapping of route_metrics): the
//                                 recursion of one track splits where its own rows say, so a lane per track would diverge on
//                                 every range, while the rows of one range are independent and go one per lane.
//
// Staging.  The wave reads its track's rows 64 at a time (the next strip's loads are issued before the current strip's
// arithmetic) and forms the unwrapped longitude X and the clock T, both sums "in order": the 64 terms of a strip are added one
// after the other by every lane alike, term l read from lane l, and lane l keeps the sum after its own term.  The chain is 64
// dependent additions per strip with no memory access in it.  X, Y, T and one keep flag per row live in LDS (dynamic, sized by the
// launch to min(Nmax + 1, kLdsRows) rows, so that short fleets keep their occupancy); a track with more rows keeps them in the
// wave's slice of `work`, through the same code.
//
// Ranges.  (i, j) is uniform over the wave.  Lanes take rows i + 1 + lane, + 64, ... and hold a running (d2, row) maximum under
// the rule's order (strict >, rows ascending); one butterfly over the 64 lanes on "larger d2, then smaller row" gives every lane
// the winner.  Pending ranges lie on an LDS stack: the wave goes on with the shorter part and pushes the longer one, so the
// stack holds at most log2(rows) entries whatever the track (32 for rows counted in int32).
//
// Compaction.  A ballot and a popcount prefix over the flags in strips of 64 give a kept row its place m; the lane that holds
// it copies the row and sums its own dt segment up to the next flag.  Every output has one writer, there are no atomics and
// nothing waits on another wave.  Blocks are dealt to the XCDs in turn, so the items are permuted in groups of 64: the 8
// neighbouring tracks that share a 64-byte segment of a row of `states` go to one XCD and meet in its L2.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

#ifndef STE_SIMPLIFY_LDS_ROWS
#define STE_SIMPLIFY_LDS_ROWS 2048  // rows of a track kept in LDS ("Simplification")
#endif

namespace ste {
namespace {

constexpr int kLdsRows = STE_SIMPLIFY_LDS_ROWS;
constexpr int kStack = 32;               // pending ranges: the shorter part is taken first, so log2(2^31 rows) bounds them
constexpr int kWorkWaves = 1024;         // blocks of a launch that needs `work`: one slice each
constexpr int kWorkBytesPerRow = 32;     // X 8, Y 8, T 8, flag 1, and 7 unused
constexpr int kBytesPerLdsRow = 25;      // X 8, Y 8, T 8, flag 1
constexpr int kMaxNmax = 0x7fffffff - 256;  // rows are counted in int32
static_assert(kLdsRows >= 64 && kLdsRows % 8 == 0 && kLdsRows * kBytesPerLdsRow + kStack * 8 <= 65536,
              "LDS of a block stays at or below 64 KiB");
static_assert(kWorkWaves % 64 == 0, "items are permuted in groups of 64 blocks");

struct SimplifyParams {
    int B, Nmax, nstates, cap, lds_rows;
    size_t ld;               // tracks per row (track_stride, or B)
    const int32_t* nsteps;   // [B] or nullptr
    const double* dt;        // [Nmax][ld] or nullptr (shape without out_dt)
    const double* states;    // [S][Nmax+1][4][ld]
    const double* tol;       // [ld] or nullptr
    const double* scale;     // [ld] or nullptr
    double tol_all, scale_all;
    char* work;              // gridDim.x slices of (Nmax + 1) * kWorkBytesPerRow bytes, or nullptr
    uint8_t* keep;           // [S][Nmax+1][ld] or nullptr
    int32_t* nkeep;          // [S][ld] or nullptr
    double* worst_sq;        // [S][ld] or nullptr
    int32_t* status;         // [S][ld] or nullptr
    int32_t* rows;           // [S][cap][ld] or nullptr
    double* out_states;      // [S][cap][4][ld] or nullptr
    double* out_dt;          // [S][cap-1][ld] or nullptr
};

// One (sample, track) item with ns + 1 rows.  X, Y, T and K hold ns + 1 entries each, in LDS or in the wave's slice of `work`.
template <bool kShape>
__device__ __forceinline__ void simplify_item(const SimplifyParams& p, size_t s, size_t t, int ns, double* X, double* Y, double* T,
                                              uint8_t* K, int2* stack, int lane) {
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1;
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    const double* dt = p.dt ? p.dt + t : nullptr;           // step k: dt[k * ld]
    const double nan = __builtin_nan("");
    const double c = p.scale ? p.scale[t] : p.scale_all, tol = p.tol ? p.tol[t] : p.tol_all;
    const double tol2 = tol * tol;
    int status = 0;
    if (!(is_finite(c) && c >= 0.0 && is_finite(tol) && tol >= 0.0)) status |= STE_SIMPLIFY_BAD_LIMIT;

    // ---- staging: X, Y and (with the clock) T of rows 0 .. ns -------------------------------------------------------------
    const double lon0 = st[0], lat0 = st[ld];
    bool broken = !is_finite(lat0), badt = false;
    if (lane == 0) {
        X[0] = lon0, Y[0] = lat0;
        if constexpr (!kShape) T[0] = 0.0;
    }
    double accX = lon0, accT = 0.0, carry = lon0;  // the sums after row `base`, and that row's longitude
    double nlon = 0.0, nlat = 0.0, ndt = 0.0;
    if (lane < ns) {  // row lane + 1 and step lane
        nlon = st[((size_t)lane * 4 + 4) * ld];
        nlat = st[((size_t)lane * 4 + 5) * ld];
        if constexpr (!kShape) ndt = dt[(size_t)lane * ld];
    }
    for (int base = 0; base < ns; base += 64) {
        const int k = base + lane;  // this lane's step, from row k to row k + 1
        const bool live = k < ns;
        const double lon = nlon, lat = nlat;
        double d = ndt;
        if (ns - 64 > k) {  // the next strip's loads, in flight during this strip's sums (k + 64 < ns without overflow)
            const size_t r = (size_t)k + 65;
            nlon = st[(r * 4) * ld];
            nlat = st[(r * 4 + 1) * ld];
            if constexpr (!kShape) ndt = dt[((size_t)k + 64) * ld];
        }
        double plon = __shfl_up(lon, 1, 64);
        if (lane == 0) plon = carry;
        carry = lane_value(lon, 63);
        double delta = 0.0;
        if (live) {
            delta = wrap180(lon - plon);
            if (!(fabs(delta) < 90.0) || !is_finite(lat)) broken = true;
            if constexpr (!kShape) {
                if (!(d >= 0.0 && is_finite(d))) badt = true;
            }
        } else {
            d = 0.0;
        }
        double myX = 0.0, myT = 0.0;
        const int nlive = ns - base;  // steps of this strip, 64 or more for a full one; the lanes past them hold zeros
#pragma unroll 1
        for (int l0 = 0; l0 < 64 && l0 < nlive; l0 += 8) {  // eight terms at a time: their lane reads fit the scalar registers
#pragma unroll
            for (int q = 0; q < 8; ++q) {  // in order: term l joins the sum of terms 0 .. l - 1
                const int l = l0 + q;
                accX = accX + lane_value(delta, l);
                if constexpr (!kShape) accT = accT + lane_value(d, l);
                if (lane == l) {
                    myX = accX;
                    if constexpr (!kShape) myT = accT;
                }
            }
        }
        if (live) {
            X[k + 1] = myX, Y[k + 1] = lat;
            if constexpr (!kShape) T[k + 1] = myT;
        }
    }
    if (__ballot(broken) != 0ull) status |= STE_SIMPLIFY_BROKEN;
    if (__ballot(badt) != 0ull) status |= STE_SIMPLIFY_BAD_TIME;
    status = first_lane(status);

    // ---- the flags -------------------------------------------------------------------------------------------------------
    const bool identity = status != 0;
    for (int k = lane; k <= ns; k += 64) K[k] = (identity || k == 0 || k == ns) ? 1 : 0;
    __syncthreads();  // X, Y, T and the flags are whole before any lane reads another lane's rows

    int nkeep = identity ? ns + 1 : (ns >= 1 ? 2 : 1);
    double worst = identity ? nan : 0.0;
    if (!identity && ns > 1) {
        int i = 0, j = ns, sp = 0;
        for (;;) {  // a range (i, j) with j > i + 1, uniform over the wave
            const double Xi = X[i], Yi = Y[i];
            const double xj = (X[j] - Xi) * c, yj = Y[j] - Yi;
            double Ti = 0.0, den;
            if constexpr (kShape) {
                den = xj * xj + yj * yj;
            } else {
                Ti = T[i];
                den = T[j] - Ti;
            }
            double best = -1.0;
            int bk = 0x7fffffff;
            for (int k = i + 1 + lane; k < j; k += 64) {
                const double xk = (X[k] - Xi) * c, yk = Y[k] - Yi;
                double u = 0.0;
                if constexpr (kShape) {
                    if (den > 0.0) u = clamp01((xk * xj + yk * yj) / den);
                } else {
                    if (den > 0.0) u = (T[k] - Ti) / den;
                }
                const double ex = xk - u * xj, ey = yk - u * yj;
                const double d2 = ex * ex + ey * ey;
                if (d2 > best) best = d2, bk = k;
            }
            // The largest d2, and among equal ones the smallest row.  A range of n < 64 rows lives in lanes 0 .. n - 1: the steps
            // with off >= n would only bring in (-1, none), and the steps below them leave lane 0 with the whole range's winner.
            const int n = j - i - 1;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                if (n > off) {  // uniform
                    const double ob = __shfl_xor(best, off, 64);
                    const int ok = __shfl_xor(bk, off, 64);
                    if (ob > best || (ob == best && ok < bk)) best = ob, bk = ok;
                }
            }
            best = first_lane(best);
            bk = first_lane(bk);
            bool pop = true;
            if (best > tol2) {  // then bk is a row of the range
                if (lane == 0) K[bk] = 1;
                ++nkeep;
                const bool left = bk > i + 1, right = j > bk + 1;
                if (left && right) {  // go on with the shorter part: what is pushed is at least as long as what follows it
                    const bool left_short = bk - i <= j - bk;
                    if (sp < kStack) stack[sp] = left_short ? make_int2(bk, j) : make_int2(i, bk);
                    ++sp;
                    if (left_short) j = bk;
                    else i = bk;
                    pop = false;
                } else if (left) {
                    j = bk, pop = false;
                } else if (right) {
                    i = bk, pop = false;
                }
            } else if (best > worst) {
                worst = best;
            }
            if (pop) {
                if (sp == 0) break;
                --sp;
                const int2 e = stack[sp < kStack ? sp : kStack - 1];
                i = first_lane(e.x), j = first_lane(e.y);
            }
        }
        __syncthreads();  // lane 0's flags are whole before the other lanes read them
    }

    // ---- outputs: one writer each --------------------------------------------------------------------------------------------
    const bool compact = p.rows || p.out_states || p.out_dt;
    if (compact && nkeep > p.cap) status |= STE_SIMPLIFY_TRUNCATED;
    if (lane == 0) {
        const size_t o = s * ld + t;
        if (p.nkeep) p.nkeep[o] = nkeep;
        if (p.worst_sq) p.worst_sq[o] = worst;
        if (p.status) p.status[o] = status;
    }
    if (p.keep) {
        uint8_t* kp = p.keep + (s * rows) * ld + t;
        for (int k = lane; k <= ns; k += 64) kp[(size_t)k * ld] = K[k];
    }
    if (compact) {
        const size_t cap = (size_t)p.cap;
        int before = 0;  // kept rows below this strip
        for (int k0 = 0; k0 <= ns && before < p.cap; k0 += 64) {
            const int k = k0 + lane;
            const bool kept = k <= ns && K[k] != 0;
            const unsigned long long mask = __ballot(kept);
            const int m = before + __popcll(mask & ((1ull << lane) - 1ull));
            if (kept && m < p.cap) {
                if (p.rows) p.rows[(s * cap + (size_t)m) * ld + t] = k;
                if (p.out_states) {
                    double* os = p.out_states + ((s * cap + (size_t)m) * 4) * ld + t;
#pragma unroll
                    for (int q = 0; q < 4; ++q) os[(size_t)q * ld] = st[((size_t)k * 4 + q) * ld];
                }
                if (p.out_dt && k < ns && m < p.cap - 1) {  // row ns is kept, so the segment ends at or before it
                    double acc = dt[(size_t)k * ld];
                    for (int q = k + 1; K[q] == 0; ++q) acc = acc + dt[(size_t)q * ld];
                    p.out_dt[(s * (cap - 1) + (size_t)m) * ld + t] = acc;
                }
            }
            before += __popcll(mask);
        }
    }
    __syncthreads();  // the next item writes X, Y, T and the flags again
}

template <bool kShape, bool kWork>
__global__ __launch_bounds__(64) void track_simplify(const SimplifyParams p) {
    extern __shared__ double lds[];
    const int lane = (int)threadIdx.x;
    const int R = p.lds_rows;  // a multiple of 8
    double* const sX = lds;
    double* const sY = lds + R;
    double* const sT = lds + 2 * (size_t)R;
    uint8_t* const sK = reinterpret_cast<uint8_t*>(lds + 3 * (size_t)R);
    int2* const stack = reinterpret_cast<int2*>(sK + R);
    const size_t B = (size_t)p.B, nitems = (size_t)p.nstates * B;

    // Blocks b, b + 8, b + 16, ... share an XCD: within a group of 64 blocks, block 8 * q + x takes item 8 * x + q, so that the
    // 8 blocks of the group on one XCD hold 8 neighbouring tracks.  gridDim.x is a multiple of 64.
#ifdef STE_SIMPLIFY_PLAIN_ITEMS  // block b takes item b, for timing ("Simplification")
    const size_t first = blockIdx.x;
#else
    const size_t r = blockIdx.x & 63u;
    const size_t first = ((size_t)blockIdx.x - r) + (r & 7u) * 8 + (r >> 3);
#endif
    for (size_t item = first; item < nitems; item += gridDim.x) {
        const size_t s = item / B, t = item - s * B;
        const int ns = track_steps(p, t);
        if constexpr (kWork) {
            if (ns + 1 > R) {  // uniform over the wave
                const size_t rows = (size_t)p.Nmax + 1;
                char* const slice = p.work + (size_t)blockIdx.x * rows * kWorkBytesPerRow;
                simplify_item<kShape>(p, s, t, ns, reinterpret_cast<double*>(slice), reinterpret_cast<double*>(slice + rows * 8),
                                      reinterpret_cast<double*>(slice + rows * 16), reinterpret_cast<uint8_t*>(slice + rows * 24),
                                      stack, lane);
                continue;
            }
        }
        simplify_item<kShape>(p, s, t, ns, sX, sY, sT, sK, stack, lane);
    }
}

unsigned simplify_blocks(uint64_t items, bool work) {
    const uint64_t cap = work ? (uint64_t)kWorkWaves : 0x7fffffc0ull;
    const uint64_t n = items < cap ? items : cap;
    return (unsigned)((n + 63) / 64 * 64);
}

}  // namespace
}  // namespace ste

extern "C" int ste_track_simplify_lds_rows(void) { return ste::kLdsRows; }

extern "C" size_t ste_track_simplify_workspace(int32_t Nmax, int32_t nstates, int32_t B) {
    using namespace ste;
    if (Nmax < kLdsRows || nstates < 1 || B < 1) return 0;  // Nmax + 1 rows fit the LDS
    const uint64_t items = (uint64_t)nstates * (uint64_t)B;
    return (size_t)((uint64_t)simplify_blocks(items, true) * ((uint64_t)Nmax + 1) * kWorkBytesPerRow);
}

extern "C" int ste_track_simplify_f64(const ste_ukf_batch_f64* b, const ste_simplify_f64* sf, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_track_simplify_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!sf) return refuse("the simplification arguments (sf) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (b->Nmax > kMaxNmax) return refuse("Nmax is limited to 2^31 - 257 (rows are counted in int32)");
    if (int rc = refuse.stride(b)) return rc;
    if (!sf->states) return refuse("sf->states is required");
    if (int rc = refuse.nstates("sf->nstates", sf->nstates)) return rc;
    if ((sf->flags & ~STE_SIMPLIFY_SHAPE) != 0) return refuse("sf->flags must be 0 or STE_SIMPLIFY_SHAPE");
    if (sf->reserved != 0) return refuse("sf->reserved must be 0");
    if (!sf->tolerance && !(sf->tolerance_all >= 0.0 && sf->tolerance_all * 0.0 == 0.0))
        return refuse("sf->tolerance_all must be finite and >= 0 when sf->tolerance is NULL");
    if (!sf->lon_scale && !(sf->lon_scale_all >= 0.0 && sf->lon_scale_all * 0.0 == 0.0))
        return refuse("sf->lon_scale_all must be finite and >= 0 when sf->lon_scale is NULL");
    const bool compact = sf->rows || sf->out_states || sf->out_dt;
    if (compact && sf->cap == 0) return refuse("rows, out_states and out_dt need sf->cap, the rows they hold");
    if (compact && (sf->cap < 1 || (int64_t)sf->cap > (int64_t)b->Nmax + 1))
        return refuse("sf->cap must be between 1 and Nmax + 1");
    const bool shape = (sf->flags & STE_SIMPLIFY_SHAPE) != 0;
    if (!b->dt && (!shape || sf->out_dt))
        return refuse("the batch's dt is required (the clock of the rule, and the terms of out_dt)");
    if (!sf->keep && !sf->nkeep && !sf->worst_sq && !sf->status && !compact)
        return refuse("no output asked for (keep, nkeep, worst_sq, status, rows, out_states and out_dt are all NULL)");
    const size_t need = ste_track_simplify_workspace(b->Nmax, sf->nstates, b->B);
    if (need > 0 && (!sf->work || sf->work_bytes < 0 || (uint64_t)sf->work_bytes < (uint64_t)need))
        return refuse("sf->work is required with work_bytes >= ste_track_simplify_workspace(Nmax, nstates, B) when Nmax + 1 exceeds ste_track_simplify_lds_rows()");
    SimplifyParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = sf->nstates;
    p.cap = compact ? sf->cap : 0;
    const int64_t nrows = (int64_t)b->Nmax + 1;
    p.lds_rows = (int)((nrows < kLdsRows ? nrows : (int64_t)kLdsRows) + 7) / 8 * 8;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = (!shape || sf->out_dt) ? b->dt : nullptr;
    p.states = sf->states;
    p.tol = sf->tolerance;
    p.scale = sf->lon_scale;
    p.tol_all = sf->tolerance_all;
    p.scale_all = sf->lon_scale_all;
    p.work = need > 0 ? reinterpret_cast<char*>(sf->work) : nullptr;
    p.keep = sf->keep;
    p.nkeep = sf->nkeep;
    p.worst_sq = sf->worst_sq;
    p.status = sf->status;
    p.rows = sf->rows;
    p.out_states = sf->out_states;
    p.out_dt = sf->out_dt;
    // a block per item while the rows fit the LDS: the hardware hands out the items; with `work`, one block per slice
    const unsigned nblocks = simplify_blocks((uint64_t)sf->nstates * (uint64_t)b->B, need > 0);
    const size_t lds_bytes = (size_t)p.lds_rows * kBytesPerLdsRow + kStack * sizeof(int2);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_bool(shape, [&](auto sh) {
        with_bool(need > 0, [&](auto wk) {
            hipLaunchKernelGGL((track_simplify<decltype(sh)::value, decltype(wk)::value>), dim3(nblocks), dim3(64), lds_bytes, s, p);
        });
    });
    return abi_check_hip(hipGetLastError(), "track_simplify launch");
}
