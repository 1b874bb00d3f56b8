// ste_line.hip — tracks that stay on the device against FIXED POLYLINES (include/ste.h: ste_line_metrics_f64): how close every
// ship came to every one of M lines (coasts, cables, routes, gates), when, on which segment and where along it, and how often,
// in which direction and when it crossed the line, for S tracks per ship (the sampler's output, or sm_mean / fwd_mean as
// S = 1).  The header carries the definitions (the sites' clock and metric, the regions' frame and crossing rule) and
// tests/line_cases.py restates them in NumPy.
//
//   line_metrics<model, cross>   a lane per track, so the rows of [4][track_stride] are read coalesced; a block is one wave:
//                                64 ships against ONE line, for one sample.  The step loop is outermost: a step is loaded
//                                once, its delta, soundness and length are worked out once, and then the line's segments are
//                                walked in index order.  A (step, segment) pair costs one cos and six divisions: two for the
//                                crossing, four for the point-against-segment candidates.  The line is the fastest grid
//                                dimension: the waves that are resident together read the same rows.
//
// The vertices are the same for every lane.  They are staged in LDS kLineChunk segments (kLineChunk + 1 vertices) at a time and
// read back at one address for the whole wave, a broadcast; a segment's second vertex is the next one's first, so one vertex
// is read per pair.  A line of at most kLineChunk segments is staged once, before the step loop; a longer one is staged again
// chunk by chunk in every step that has a sound lane, which costs two coalesced loads per 64 pairs of arithmetic.  The step
// loop runs to the largest nsteps of the wave so that every lane takes part in the staging; a lane past its own nsteps
// computes nothing.  The running state of the line (best q, time, position, segment, fraction, four crossing quantities) lives
// in registers.  The leg function (haversine or the WGS84 inverse) runs once per (sample, line, track) after the loop.  Every
// output has one writer: plain vector loads and stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

#ifndef STE_LINE_CHUNK
#define STE_LINE_CHUNK 64  // segments staged at a time: one vertex per lane and one more ("Lines")
#endif
#ifdef STE_LINE_WAVES  // waves per SIMD, for timing other forms; unset, the compiler's own choice stands ("Lines")
#define STE_LINE_OCCUPANCY __attribute__((amdgpu_waves_per_eu(STE_LINE_WAVES, STE_LINE_WAVES)))
#else
#define STE_LINE_OCCUPANCY
#endif

namespace ste {
namespace {

constexpr int kLineChunk = STE_LINE_CHUNK;
static_assert(kLineChunk >= 1 && kLineChunk <= 64, "a chunk is staged by one pass of the wave plus one vertex");
constexpr double kKd = kEarthKm * kDeg2Rad;  // km per degree of a great circle, one double

struct LineParams {
    int B, Nmax, nstates, nlines, nvert;
    size_t ld;               // tracks per row (track_stride, or B)
    const int32_t* nsteps;   // [B] or nullptr
    const double* dt;        // [Nmax][ld]
    const double* states;    // [S][Nmax+1][4][ld]
    const double* vert;      // [2][V]
    const int32_t* first;    // [M+1]
    const double* lon_ref;   // [M]
    const double* t0;        // [ld] or nullptr
    double* min_dist;        // [S][M][ld] each, or nullptr
    double* min_time;
    int32_t* min_seg;
    double* min_frac;
    int32_t* ncross;
    int32_t* net_cross;
    double* first_cross;
    double* last_cross;
    double* sound_time;      // [S][ld] or nullptr
    int32_t* nbroken;
    int32_t* track_status;   // [ld] or nullptr
    int32_t* line_status;    // [M] or nullptr
};


template <int kModel, bool kCross>
__global__ __launch_bounds__(64) STE_LINE_OCCUPANCY void line_metrics(const LineParams p) {
    __shared__ double svx[kLineChunk + 1], svy[kLineChunk + 1];
    const int M = p.nlines, V = p.nvert;
    const int m = (int)(blockIdx.x % (unsigned)M);
    const unsigned ttile = blockIdx.x / (unsigned)M;
    const int lane = (int)threadIdx.x;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = blockIdx.y;
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    // the line: uniform over the wave.  With a bad range nothing of it is read.
    const int f0 = p.first[m], f1 = p.first[m + 1];
    const double ref = p.lon_ref[m];
    const bool range_ok = f0 >= 0 && f1 <= V && f1 >= f0 + 2;  // f0 <= f1 <= V <= 2^20 where the last comparison is reached
    const int nseg = range_ok ? f1 - f0 - 1 : 0;
    const double* vx = p.vert + (range_ok ? f0 : 0);
    const double* vy = vx + V;
    bool lbad = !range_ok || !is_finite(ref);
    if (range_ok) {
        bool mine = false;
        for (int i = lane; i <= nseg; i += 64) {
            const double x = vx[i], y = vy[i];
            if (!(is_finite(x) && is_finite(y) && fabs(x - ref) <= 90.0)) mine = true;
        }
        lbad = lbad || __ballot(mine) != 0;
    }
    if (p.line_status && ttile == 0 && s == 0 && lane == 0) p.line_status[m] = lbad ? STE_LINE_BAD_LINE : 0;
    const int L = lbad ? 0 : nseg;  // segments to walk
    const bool single = L <= kLineChunk;
    if (single && L > 0) {  // the whole line, once
        if (lane <= L) {
            svx[lane] = vx[lane];
            svy[lane] = vy[lane];
        }
        if (lane == 0 && L == 64) {
            svx[64] = vx[64];
            svy[64] = vy[64];
        }
        __syncthreads();
    }

    const size_t t = (size_t)ttile * 64 + lane;
    const bool live = t < (size_t)p.B;
    const double t0 = live && p.t0 ? p.t0[t] : 0.0;
    bool tbad = !is_finite(t0);
    // a bad line is walked by the block of line 0 alone, for the track's own outputs
    const bool walk = live && !tbad && (!lbad || m == 0);
    const int ns = walk ? track_steps(p, t) : 0;
    int nsmax = ns;  // the wave's largest: every lane takes part in the staging of every step
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nsmax = max(nsmax, __shfl_xor(nsmax, off, 64));

    double best_q = inf, mt = nan, posx = nan, posy = nan, frac = nan;
    int seg = -1;
    int ncross = 0, net = 0;
    double first = nan, last = nan;
    double sound_time = 0.0;
    int nbroken = 0;

    const double* st = p.states + (s * rows * 4) * ld + (live ? t : 0);  // row k, component c: st[(k * 4 + c) * ld]
    const double* dtp = p.dt + (live ? t : 0);
    double lon = 0.0, lat = 0.0, lon1 = 0.0, lat1 = 0.0, dtk = 0.0, T = 0.0;
    if (ns > 0) {  // rows past nsteps are never read
        dtk = dtp[0];
        lon = st[0];
        lat = st[ld];
        lon1 = st[4 * ld];
        lat1 = st[5 * ld];
    }
    for (int k = 0; k < nsmax; ++k) {
        const bool active = k < ns;
        // what the next step needs, in flight during this step's arithmetic
        double ndt = 0.0, plon = 0.0, plat = 0.0;
        if (k + 1 < ns) {
            const size_t r = (size_t)k + 2;
            ndt = dtp[(r - 1) * ld];
            plon = st[(r * 4) * ld];
            plat = st[(r * 4 + 1) * ld];
        }
        if (active && !(dtk >= 0.0 && is_finite(dtk))) tbad = true;
        const double lo = t0 + T, T1 = T + dtk, hi = t0 + T1;
        const double len = hi - lo;
        const double delta = wrap180(lon1 - lon);
        const bool examined = active && hi > lo;
        const bool sound = examined && fabs(delta) < 90.0 && is_finite(lat) && is_finite(lat1);
        if (examined && !sound) ++nbroken;
        if (sound) sound_time = sound_time + len;
        if (L > 0 && __ballot(sound) != 0) {  // uniform
            const double x0 = ref + wrap180(lon - ref), y0 = lat, x1 = x0 + delta, y1 = lat1;
            const double dx = x1 - x0, dy = y1 - y0, ysum = y0 + y1;
            double umin = inf, umax = -inf;
            for (int c0 = 0; c0 < L; c0 += kLineChunk) {
                const int nc = min(kLineChunk, L - c0);
                if (!single) {  // vertices c0 .. c0 + nc of the line
                    __syncthreads();
                    if (lane <= nc) {
                        svx[lane] = vx[c0 + lane];
                        svy[lane] = vy[c0 + lane];
                    }
                    if (lane == 0 && nc == 64) {
                        svx[64] = vx[c0 + 64];
                        svy[64] = vy[c0 + 64];
                    }
                    __syncthreads();
                }
                double px = svx[0], py = svy[0];
                for (int j = 0; j < nc; ++j) {
                    const double qx = svx[j + 1], qy = svy[j + 1];
                    if (sound) {
                        const double ex = qx - px, ey = qy - py;
                        const double wx = px - x0, wy = py - y0;
                        const double den = dx * ey - dy * ex;
                        const double u = (wx * ey - wy * ex) / den, v = (wx * dy - wy * dx) / den;
                        const bool cr = den != 0.0 && u >= 0.0 && u < 1.0 && v >= 0.0 && v < 1.0;
                        if constexpr (kCross) {
                            if (cr) {
                                ++ncross;
                                net += den < 0.0 ? 1 : -1;
                                umin = u < umin ? u : umin;
                                umax = u > umax ? u : umax;
                            }
                        }
                        const double kc = kKd * cos(0.25 * (ysum + (py + qy)) * kDeg2Rad);
                        const double a0x = kc * wx, a0y = kKd * wy;
                        const double a1x = kc * (qx - x0), a1y = kKd * (qy - y0);
                        const double dkx = kc * dx, dky = kKd * dy;
                        const double ekx = a1x - a0x, eky = a1y - a0y;
                        const double dd = dkx * dkx + dky * dky, ee = ekx * ekx + eky * eky;
                        const double b0x = a0x - dkx, b0y = a0y - dky;
                        // the candidates in the header's order; a later one replaces an earlier one only when it is closer
                        double cq = cr ? 0.0 : inf, cu = cr ? u : 0.0, cv = cr ? v : 0.0;
                        {
                            const double u2 = dd > 0.0 ? clamp01((a0x * dkx + a0y * dky) / dd) : 0.0;
                            const double gx = a0x - u2 * dkx, gy = a0y - u2 * dky;
                            const double q = gx * gx + gy * gy;
                            if (q < cq) cq = q, cu = u2, cv = 0.0;
                        }
                        {
                            const double u3 = dd > 0.0 ? clamp01((a1x * dkx + a1y * dky) / dd) : 0.0;
                            const double gx = a1x - u3 * dkx, gy = a1y - u3 * dky;
                            const double q = gx * gx + gy * gy;
                            if (q < cq) cq = q, cu = u3, cv = 1.0;
                        }
                        {
                            const double v4 = ee > 0.0 ? clamp01(-(a0x * ekx + a0y * eky) / ee) : 0.0;
                            const double gx = a0x + v4 * ekx, gy = a0y + v4 * eky;
                            const double q = gx * gx + gy * gy;
                            if (q < cq) cq = q, cu = 0.0, cv = v4;
                        }
                        {
                            const double v5 = ee > 0.0 ? clamp01(-(b0x * ekx + b0y * eky) / ee) : 0.0;
                            const double gx = b0x + v5 * ekx, gy = b0y + v5 * eky;
                            const double q = gx * gx + gy * gy;
                            if (q < cq) cq = q, cu = 1.0, cv = v5;
                        }
                        if (cq < best_q) {
                            best_q = cq;
                            mt = lo + cu * len;
                            posx = x0 + cu * dx;
                            posy = y0 + cu * dy;
                            seg = c0 + j;
                            frac = cv;
                        }
                    }
                    px = qx;
                    py = qy;
                }
            }
            if constexpr (kCross) {
                if (sound && umax >= 0.0) {  // this step has a crossing
                    if (!(first == first)) first = lo + umin * len;
                    last = lo + umax * len;
                }
            }
        }
        T = T1;
        dtk = ndt;
        lon = lon1;
        lat = lat1;
        lon1 = plon;
        lat1 = plat;
    }
    if (!live) return;

    if (m == 0) {
        if (p.track_status && s == 0) p.track_status[t] = tbad ? STE_LINE_BAD_TIME : 0;
        if (p.sound_time) p.sound_time[s * ld + t] = tbad ? 0.0 : sound_time;
        if (p.nbroken) p.nbroken[s * ld + t] = tbad ? 0 : nbroken;
    }
    const size_t o = (s * (size_t)M + (size_t)m) * ld + t;
    const bool bad = tbad || lbad;
    const bool found = !bad && best_q < inf;
    if (p.min_time) p.min_time[o] = found ? mt : nan;
    if (p.min_seg) p.min_seg[o] = found ? seg : -1;
    if (p.min_frac) p.min_frac[o] = found ? frac : nan;
    if constexpr (kCross) {
        if (p.ncross) p.ncross[o] = bad ? 0 : ncross;
        if (p.net_cross) p.net_cross[o] = bad ? 0 : net;
        if (p.first_cross) p.first_cross[o] = bad ? nan : first;
        if (p.last_cross) p.last_cross[o] = bad ? nan : last;
    }
    if constexpr (kModel != kNoLeg) {
        double d = nan;
        if (found) {  // seg < nseg: both vertices lie inside the line's range
            const double ax = vx[seg], ay = vy[seg], bx = vx[seg + 1], by = vy[seg + 1];
            d = leg_km_deg<kModel>(posx, posy, ax + frac * (bx - ax), ay + frac * (by - ay));
        }
        p.min_dist[o] = d;
    }
}

template <int kModel, bool kCross>
void launch_line(const LineParams& p, unsigned nblocks, hipStream_t s) {
    const dim3 grid(nblocks, (unsigned)p.nstates), block(64);
    hipLaunchKernelGGL((line_metrics<kModel, kCross>), grid, block, 0, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_line_chunk(void) { return ste::kLineChunk; }

extern "C" int ste_line_metrics_f64(const ste_ukf_batch_f64* b, const ste_line_f64* li, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_line_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!li) return refuse("the line arguments (li) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!li->states) return refuse("li->states is required");
    if (!li->vert) return refuse("li->vert is required");
    if (!li->first) return refuse("li->first is required (nlines + 1 vertex offsets)");
    if (!li->lon_ref) return refuse("li->lon_ref is required (one meridian per line)");
    if (int rc = refuse.nstates("li->nstates", li->nstates, " (one grid row per track of a ship)")) return rc;
    if (li->nlines < 1 || li->nlines > STE_LINES_MAX) return refuse("li->nlines must be between 1 and STE_LINES_MAX (4096)");
    if (li->nvert < 2 || li->nvert > STE_LINE_MAX_VERT_TOTAL)
        return refuse("li->nvert must be between 2 and STE_LINE_MAX_VERT_TOTAL (1048576)");
    if (li->min_dist && refuse.model("li->model", li->model, " when min_dist is asked for")) return STE_EINVAL;
    if (li->flags != 0) return refuse("li->flags must be 0");
    if (li->reserved != 0) return refuse("li->reserved must be 0");
    if (!b->dt) return refuse("the batch's dt is required (the clock is made of its sums)");
    if (!li->min_dist && !li->min_time && !li->min_seg && !li->min_frac && !li->ncross && !li->net_cross && !li->first_cross &&
        !li->last_cross && !li->sound_time && !li->nbroken && !li->track_status && !li->line_status)
        return refuse("no output asked for (min_dist, min_time, min_seg, min_frac, ncross, net_cross, first_cross, last_cross, sound_time, nbroken, track_status and line_status are all NULL)");
    LineParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = li->nstates;
    p.nlines = li->nlines;
    p.nvert = li->nvert;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = li->states;
    p.vert = li->vert;
    p.first = li->first;
    p.lon_ref = li->lon_ref;
    p.t0 = li->t0;
    p.min_dist = li->min_dist;
    p.min_time = li->min_time;
    p.min_seg = li->min_seg;
    p.min_frac = li->min_frac;
    p.ncross = li->ncross;
    p.net_cross = li->net_cross;
    p.first_cross = li->first_cross;
    p.last_cross = li->last_cross;
    p.sound_time = li->sound_time;
    p.nbroken = li->nbroken;
    p.track_status = li->track_status;
    p.line_status = li->line_status;
    const uint64_t nblocks = (uint64_t)li->nlines * (uint64_t)(((int64_t)b->B + 63) / 64);
    if (nblocks > 0x7fffffffull)
        return refuse("ceil(B / 64) * nlines exceeds 2^31 - 1 blocks: split the lines or the tracks over calls");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool cross = li->ncross || li->net_cross || li->first_cross || li->last_cross;
    const int model = li->min_dist ? li->model : kNoLeg;
    with_bool(cross, [&](auto c) {
        constexpr bool kC = decltype(c)::value;
        if (model == STE_PREP_SPHERE) launch_line<STE_PREP_SPHERE, kC>(p, (unsigned)nblocks, s);
        else if (model == STE_PREP_WGS84) launch_line<STE_PREP_WGS84, kC>(p, (unsigned)nblocks, s);
        else launch_line<kNoLeg, kC>(p, (unsigned)nblocks, s);
    });
    return abi_check_hip(hipGetLastError(), "line_metrics launch");
}
