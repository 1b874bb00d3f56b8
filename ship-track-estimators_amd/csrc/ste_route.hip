// ste_route.hip — pairs of tracks that stay on the device as CURVES, without a clock (include/ste.h: ste_route_metrics_f64): the
// discrete Frechet distance of two routes with the cell that attains it, and the dynamic-time-warping cost with the length of
// its path, for S tracks per ship (the sampler's output, or sm_mean / fwd_mean as S = 1).  Both are an (ns_i + 1) x (ns_j + 1)
// dynamic programme per (sample, pair).  The header carries the definitions and tests/route_cases.py restates them in NumPy.
//
//   route_metrics<model, dtw>   a WAVE per (sample, pair) item, a block is one wave.  The rows of track i are taken in strips of
//                               64: lane l owns row a0 + l and holds its unit vector in registers.  The columns of track j are
//                               swept skewed: at tick t lane l does column cs + t - l, so the cells of one tick lie on an
//                               anti-diagonal and depend on nothing of the same tick.  A lane needs from lane l - 1 that lane's
//                               result of the last tick (the cell above) and of the tick before (the diagonal one): one cross-lane
//                               move per carried word per tick, the diagonal being the move of the tick before kept in a
//                               register.  From itself it needs the last tick (the cell to the left).
//
// Track j's unit vectors are computed 64 columns at a time, one column per lane, and staged in an LDS ring of 128 columns: the
// lanes of a tick read 64 consecutive columns, which always lie in the chunk being swept and the one before it.  A row of the
// strided `states` layout is read once per strip, not once per cell; the next chunk's rows are requested before the ticks of
// the current one.  The strip's last lane writes its row of the tables (the BOUNDARY ROW) for lane 0 of the next strip: to LDS
// while ns_j + 1 <= kLdsCols, to the wave's slice of `work` beyond that.  Lane 63 writes column c 63 ticks after lane 0 has
// read it, so the row is updated in place.  With a band a strip sweeps only columns a0 - band .. a0 + 63 + band.
//
// A cell that does not exist or is not admissible holds +inf in both tables: it then never replaces a predecessor (strict <) and
// is never chosen before an admissible one whose value is finite.  A cell whose F is +inf has lost its `at`, but such a pair
// ends with F = +inf and STE_ROUTE_NOT_FINITE; D is finite in every admissible cell.  Nothing waits on another block, there
// are no atomics and every output has one writer.  The leg function runs once per (sample, pair), on the lane that holds the
// last cell.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

#ifndef STE_ROUTE_LDS_COLS
#define STE_ROUTE_LDS_COLS 512  // columns of the boundary row kept in LDS ("Routes")
#endif

namespace ste {
namespace {

constexpr int kLdsCols = STE_ROUTE_LDS_COLS;
constexpr int kRing = 128;               // columns of track j staged at a time: the chunk being swept and the one before it
constexpr int kWorkWaves = 2048;         // blocks of a launch that needs `work`: one slice each
constexpr int kWorkBytesPerCol = 32;     // F 8, at 8, D 8, L 4, and 4 unused
constexpr int kMaxNmax = 0x7fffffff - 256;  // ticks and columns are counted in int32
constexpr double kTwoR = 2.0 * kEarthKm;
static_assert(kLdsCols >= 64 && kLdsCols * 28 + kRing * 24 <= 65536, "static LDS of a block stays at or below 64 KiB");

struct RouteParams {
    int B, Nmax, nstates, band;
    bool reverse;
    size_t ld;              // tracks per row (track_stride, or B)
    size_t npairs;
    const int32_t* nsteps;  // [B] or nullptr
    const double* states;   // [S][Nmax+1][4][ld]
    const int32_t* pairs;   // [P][2]
    char* work;             // gridDim.x slices of (Nmax + 1) * kWorkBytesPerCol bytes, or nullptr
    double* frechet;        // [S][P] or nullptr
    int32_t* frechet_at;    // [S][P][2] or nullptr
    double* dtw;            // [S][P] or nullptr
    int32_t* dtw_len;       // [S][P] or nullptr
    int32_t* status;        // [S][P] or nullptr
};

template <int kModel, bool kDtw>
__global__ __launch_bounds__(64) void route_metrics(const RouteParams p) {
    __shared__ double rx[kRing], ry[kRing], rz[kRing];
    __shared__ double sF[kLdsCols];
    __shared__ int32_t sA[kLdsCols], sB[kLdsCols];
    __shared__ double sD[kDtw ? kLdsCols : 1];
    __shared__ int32_t sL[kDtw ? kLdsCols : 1];
    const int lane = (int)threadIdx.x;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, P = p.npairs;
    const size_t nitems = (size_t)p.nstates * P;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const int band = p.band;

    // the wave's slice of `work`: the boundary row of a pair with more than kLdsCols columns
    char* const slice = p.work ? p.work + (size_t)blockIdx.x * rows * kWorkBytesPerCol : nullptr;
    double* const gF = reinterpret_cast<double*>(slice);
    int32_t* const gA = reinterpret_cast<int32_t*>(slice + rows * 8);
    int32_t* const gB = reinterpret_cast<int32_t*>(slice + rows * 12);
    double* const gD = reinterpret_cast<double*>(slice + rows * 16);
    int32_t* const gL = reinterpret_cast<int32_t*>(slice + rows * 24);

    for (size_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const size_t s = item / P, pr = item - s * P;
        const int i = p.pairs[2 * pr], j = p.pairs[2 * pr + 1];
        int status = 0, nsi = 0, nsj = 0;
        if (i < 0 || i >= p.B || j < 0 || j >= p.B) {
            status = STE_ROUTE_BAD_INDEX;  // nothing of the pair is read
        } else {
            nsi = track_steps(p, i);
            nsj = track_steps(p, j);
            if (band > 0 && (nsi > nsj ? nsi - nsj : nsj - nsi) > band) status = STE_ROUTE_NO_PATH;
        }
        const double* sti = p.states + (s * rows * 4) * ld + (size_t)(status ? 0 : i);  // row k, component c: sti[(k * 4 + c) * ld]
        const double* stj = p.states + (s * rows * 4) * ld + (size_t)(status ? 0 : j);

        // the tables at (ns_i, ns_j), on the lane that owns row ns_i
        double oF = inf, oD = 0.0;
        int oa = -1, ob = -1, oL = 0;

        if (status == 0) {  // uniform over the wave
            const int m = nsj + 1;
            const bool lds = m <= kLdsCols;
            int pcs = 0, pce = -1;  // the columns the strip before this one has written to the boundary row
            for (int a0 = 0;; a0 += 64) {
                const int nl = nsi - a0 >= 63 ? 64 : nsi - a0 + 1;  // rows of this strip
                const bool more = nsi - a0 >= 64;                   // a strip follows: the last lane writes the boundary row
                const int a = a0 + lane;
                const bool rowok = lane < nl;
                double ux = 0.0, uy = 0.0, uz = 0.0;
                if (rowok) unit_vector(sti[((size_t)a * 4) * ld], sti[((size_t)a * 4 + 1) * ld], ux, uy, uz);
                const int cs = band > 0 && a0 > band ? a0 - band : 0;
                const int ce = band > 0 && (long long)a0 + 63 + band < (long long)nsj ? a0 + 63 + band : nsj;
                const int ncols = ce - cs + 1, T = ncols + nl - 1;

                // this lane's cell of the last tick (left), and lane l - 1's of the last tick (up) and of the one before (diag)
                double lF = inf, dF = inf, lD = inf, dD = inf;
                int lA = -1, lB = -1, dA = -1, dB = -1, lL = 0, dL = 0;
                if (lane == 0 && a0 > 0 && cs - 1 >= pcs && cs - 1 <= pce) {  // cell (a0 - 1, cs - 1) of the boundary row
                    const int c = cs - 1;
                    if (lds) {
                        dF = sF[c], dA = sA[c], dB = sB[c];
                        if constexpr (kDtw) dD = sD[c], dL = sL[c];
                    } else {
                        dF = gF[c], dA = gA[c], dB = gB[c];
                        if constexpr (kDtw) dD = gD[c], dL = gL[c];
                    }
                }

                // rows of track j for the first chunk of columns
                double nlon = 0.0, nlat = 0.0;
                if (lane < ncols) {
                    const size_t r = (size_t)(p.reverse ? nsj - (cs + lane) : cs + lane);
                    nlon = stj[(r * 4) * ld];
                    nlat = stj[(r * 4 + 1) * ld];
                }
                for (int t0 = 0; t0 < T; t0 += 64) {
                    {  // columns cs + t0 .. cs + t0 + 63 into the ring; the slots are those of the chunk before the last one
                        double x, y, z;
                        unit_vector(nlon, nlat, x, y, z);
                        const int slot = (t0 + lane) & (kRing - 1);
                        rx[slot] = x, ry[slot] = y, rz[slot] = z;
                    }
                    __syncthreads();
                    if (t0 + 64 + lane < ncols) {  // the next chunk's rows, in flight during this chunk's ticks
                        const int c = cs + t0 + 64 + lane;
                        const size_t r = (size_t)(p.reverse ? nsj - c : c);
                        nlon = stj[(r * 4) * ld];
                        nlat = stj[(r * 4 + 1) * ld];
                    }
                    const int tn = T - t0 < 64 ? T - t0 : 64;
                    for (int tt = 0; tt < tn; ++tt) {
                        const int t = t0 + tt, rel = t - lane, b = cs + rel;
                        const bool inrange = rel >= 0 && b <= ce;
                        const bool valid = rowok && inrange && (band == 0 || (a > b ? a - b : b - a) <= band);
                        // the cell above: lane l - 1's last tick, or the boundary row
                        double uF = lane_up(lF), uD = inf;
                        int uA = lane_up(lA), uB = lane_up(lB), uL = 0;
                        if constexpr (kDtw) uD = lane_up(lD), uL = lane_up(lL);
                        if (lane == 0) {
                            uF = inf, uA = -1, uB = -1, uD = inf, uL = 0;
                            if (a0 > 0 && inrange && b >= pcs && b <= pce) {
                                if (lds) {
                                    uF = sF[b], uA = sA[b], uB = sB[b];
                                    if constexpr (kDtw) uD = sD[b], uL = sL[b];
                                } else {
                                    uF = gF[b], uA = gA[b], uB = gB[b];
                                    if constexpr (kDtw) uD = gD[b], uL = gL[b];
                                }
                            }
                        }
                        const int slot = rel & (kRing - 1);
                        const double ex = ux - rx[slot], ey = uy - ry[slot], ez = uz - rz[slot];
                        double q = (ex * ex + ey * ey) + ez * ez;
                        q = q * 0.0 == 0.0 ? q : inf;
                        const bool origin = a == 0 && b == 0;
                        // Frechet: the predecessor in the order diag, up, left; a later one only when strictly smaller
                        double mF = dF;
                        int mA = dA, mB = dB;
                        if (uF < mF) mF = uF, mA = uA, mB = uB;
                        if (lF < mF) mF = lF, mA = lA, mB = lB;
                        const bool here = origin || q >= mF;
                        const double cF = valid ? (here ? q : mF) : inf;
                        const int cA = here ? a : mA, cB = here ? b : mB;
                        double cD = inf;
                        int cL = 0;
                        if constexpr (kDtw) {
                            double h = 0.5 * sqrt(q);
                            h = h > 1.0 ? 1.0 : h;
                            const double cost = kTwoR * asin(h);
                            double mD = dD;
                            int mL = dL;
                            if (uD < mD) mD = uD, mL = uL;
                            if (lD < mD) mD = lD, mL = lL;
                            cD = valid ? (origin ? cost : cost + mD) : inf;
                            cL = origin ? 1 : 1 + mL;
                        }
                        if (valid && a == nsi && b == nsj) oF = cF, oa = cA, ob = cB, oD = cD, oL = cL;
                        if (more && lane == 63 && inrange) {
                            if (lds) {
                                sF[b] = cF, sA[b] = cA, sB[b] = cB;
                                if constexpr (kDtw) sD[b] = cD, sL[b] = cL;
                            } else {
                                gF[b] = cF, gA[b] = cA, gB[b] = cB;
                                if constexpr (kDtw) gD[b] = cD, gL[b] = cL;
                            }
                        }
                        dF = uF, dA = uA, dB = uB;
                        lF = cF, lA = cA, lB = cB;
                        if constexpr (kDtw) dD = uD, dL = uL, lD = cD, lL = cL;
                    }
                }
                __syncthreads();  // the boundary row is whole, in LDS or in `work`, before lane 0 of the next strip reads it
                pcs = cs, pce = ce;
                if (!more) break;
            }
        }

        // one writer per (sample, pair): the lane that owns row ns_i, or lane 0 of a pair that was not walked
        if (lane == (status ? 0 : (nsi & 63))) {
            if (status == 0 && !(oF < inf)) status = STE_ROUTE_NOT_FINITE;
            const bool bad = status != 0;
            const int rj = bad ? -1 : (p.reverse ? nsj - ob : ob);
            const size_t o = s * P + pr;
            if (p.status) p.status[o] = status;
            if (p.frechet_at) p.frechet_at[2 * o] = bad ? -1 : oa, p.frechet_at[2 * o + 1] = rj;
            if constexpr (kDtw) {
                if (p.dtw) p.dtw[o] = bad ? nan : oD;
                if (p.dtw_len) p.dtw_len[o] = bad ? 0 : oL;
            }
            if constexpr (kModel != kNoLeg) {
                double d = nan;
                if (!bad) {  // oa <= ns_i and rj <= ns_j: rows that the sweep has read
                    d = leg_km_deg<kModel>(sti[((size_t)oa * 4) * ld], sti[((size_t)oa * 4 + 1) * ld],
                                             stj[((size_t)rj * 4) * ld], stj[((size_t)rj * 4 + 1) * ld]);
                }
                p.frechet[o] = d;
            }
        }
        __syncthreads();  // the next item's strips write the ring and the boundary row again
    }
}

template <int kModel, bool kDtw>
void launch_route(const RouteParams& p, unsigned nblocks, hipStream_t s) {
    hipLaunchKernelGGL((route_metrics<kModel, kDtw>), dim3(nblocks), dim3(64), 0, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_route_lds_cols(void) { return ste::kLdsCols; }

extern "C" size_t ste_route_workspace(int32_t Nmax, int32_t nstates, int64_t npairs) {
    using namespace ste;
    if (Nmax < kLdsCols || nstates < 1 || npairs < 1) return 0;  // Nmax + 1 columns fit the LDS
    const uint64_t items = (uint64_t)nstates * (uint64_t)npairs;
    const uint64_t waves = items < (uint64_t)kWorkWaves ? items : (uint64_t)kWorkWaves;
    return (size_t)(waves * ((uint64_t)Nmax + 1) * kWorkBytesPerCol);
}

extern "C" int ste_route_metrics_f64(const ste_ukf_batch_f64* b, const ste_route_f64* ro, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_route_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!ro) return refuse("the route arguments (ro) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (b->Nmax > kMaxNmax) return refuse("Nmax is limited to 2^31 - 257 (columns and ticks are counted in int32)");
    if (int rc = refuse.stride(b)) return rc;
    if (!ro->states) return refuse("ro->states is required");
    if (!ro->pairs) return refuse("ro->pairs is required");
    if (int rc = refuse.nstates("ro->nstates", ro->nstates)) return rc;
    if (ro->npairs < 1 || ro->npairs > STE_ROUTE_MAX_PAIRS)
        return refuse("ro->npairs must be between 1 and STE_ROUTE_MAX_PAIRS (2^26)");
    if (ro->frechet && refuse.model("ro->model", ro->model, " when frechet is asked for")) return STE_EINVAL;
    if (ro->band < 0) return refuse("ro->band must be >= 0 (0 = no band)");
    if ((ro->flags & ~STE_ROUTE_REVERSE_J) != 0) return refuse("ro->flags must be 0 or STE_ROUTE_REVERSE_J");
    if (!ro->frechet && !ro->frechet_at && !ro->dtw && !ro->dtw_len && !ro->status)
        return refuse("no output asked for (frechet, frechet_at, dtw, dtw_len and status are all NULL)");
    const size_t need = ste_route_workspace(b->Nmax, ro->nstates, ro->npairs);
    if (need > 0 && (!ro->work || ro->work_bytes < 0 || (uint64_t)ro->work_bytes < (uint64_t)need))
        return refuse("ro->work is required with work_bytes >= ste_route_workspace(Nmax, nstates, npairs) when Nmax + 1 exceeds ste_route_lds_cols()");
    RouteParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = ro->nstates;
    p.band = ro->band > b->Nmax ? 0 : ro->band;  // a band that wide admits every cell
    p.reverse = (ro->flags & STE_ROUTE_REVERSE_J) != 0;
    p.ld = track_ld(b);
    p.npairs = (size_t)ro->npairs;
    p.nsteps = b->nsteps;
    p.states = ro->states;
    p.pairs = ro->pairs;
    p.work = need > 0 ? reinterpret_cast<char*>(ro->work) : nullptr;
    p.frechet = ro->frechet;
    p.frechet_at = ro->frechet_at;
    p.dtw = ro->dtw;
    p.dtw_len = ro->dtw_len;
    p.status = ro->status;
    // a block per item while the boundary row fits the LDS: the hardware hands out the items; with `work`, one block per slice
    const uint64_t items = (uint64_t)ro->nstates * (uint64_t)ro->npairs;
    const uint64_t cap = need > 0 ? (uint64_t)kWorkWaves : 0x7fffffffull;
    const unsigned nblocks = (unsigned)(items < cap ? items : cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool dtw = ro->dtw || ro->dtw_len;
    const int model = ro->frechet ? ro->model : kNoLeg;
    with_bool(dtw, [&](auto w) {
        constexpr bool kD = decltype(w)::value;
        if (model == STE_PREP_SPHERE) launch_route<STE_PREP_SPHERE, kD>(p, nblocks, s);
        else if (model == STE_PREP_WGS84) launch_route<STE_PREP_WGS84, kD>(p, nblocks, s);
        else launch_route<kNoLeg, kD>(p, nblocks, s);
    });
    return abi_check_hip(hipGetLastError(), "route_metrics launch");
}
