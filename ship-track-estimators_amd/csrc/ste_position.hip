// ste_position.hip — where tracks that stay on the device were at given clock times (include/ste.h: ste_track_positions_f64):
// position, speed and heading of S tracks per ship (the sampler's output, or sm_mean / fwd_mean as S = 1) at a list of (track,
// time) queries, and the moments of the positions OVER THE SAMPLES about an anchor, continued from call to call.  The header
// carries the definitions and tests/position_cases.py restates them in NumPy.
//
//   position_knots              a lane per track: the in-order sums T_k of dt, written to the caller's workspace (rows of
//                               track_stride, like dt: both coalesced).  Row 0 holds 0, or NaN when a dt is not finite and >= 0.
//   position_query<vel, mom>    a lane per query.  The time-to-(step, fraction) search is a bisection of the track's column of
//                               knots -- ceil(log2(Nmax + 1)) dependent loads; lanes of a list sorted by (track, time) share
//                               lines -- and does not depend on the sample.  The lane then loops over the samples: always with
//                               moments, because the order of the additions is part of the definition, and without them from
//                               kLaneLoopQueries queries on, where the list alone fills the device.  Shorter lists put the
//                               samples along blockIdx.y (the mapping of encounter_metrics), every row of the grid repeating
//                               the search: at S = 16 that is 3 times as fast on 1 000 queries, the same on 10 000, and 2.8 ms
//                               against 2.0 on a million ("Positions").
//                               The bits are the same either way.
//
// The rows of the next sample are requested before the arithmetic of the current one.  The reads are gathers: 8 B per (sample,
// row, component) at addresses the query list decides.  No transcendental anywhere; every output word has one writer: plain
// loads and stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

namespace ste {
namespace {

struct PosParams {
    int B, Nmax, nstates;
    int per_lane;           // samples a lane of position_query walks: nstates, or 1 with the samples along blockIdx.y
    size_t ld;              // tracks per row (track_stride, or B)
    size_t nq;
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld]; read by position_knots alone
    const double* states;   // [S][Nmax+1][4][ld]
    const int32_t* qtrack;  // [Q]
    const double* qtime;    // [Q]
    const double* t0;       // [ld] or nullptr
    double* knots;          // [Nmax+1][ld]
    const double* anchor;   // [2][Q]
    double* lon;            // [S][Q] each, or nullptr
    double* lat;
    double* speed;
    double* heading;
    int32_t* step;          // [Q] each, or nullptr
    double* frac;
    int32_t* status;
    int32_t* count;         // [Q] and [5][Q], accumulated, or nullptr
    double* moments;
};

constexpr size_t kLaneLoopQueries = (size_t)1 << 14;  // 256 waves, one for every CU: the two mappings tie at 10 000 queries


__global__ __launch_bounds__(64) void position_knots(const PosParams p) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const int ns = track_steps(p, t);
    double T = 0.0;
    bool bad = false;
    for (int k = 0; k < ns; ++k) {
        const double d = p.dt[(size_t)k * p.ld + t];
        bad = bad || !(d >= 0.0 && is_finite(d));
        T = T + d;
        p.knots[((size_t)k + 1) * p.ld + t] = T;
    }
    p.knots[t] = bad ? __builtin_nan("") : 0.0;
}

// the rows one (sample, query) reads: row a, and row a + 1 of an interior query
struct PosRows {
    double lon0, lat0, s0, h0;
    double lon1, lat1, s1, h1;
};

template <bool kVel>
__device__ __forceinline__ void load_rows(PosRows& r, const double* st, size_t ld, bool interior) {
    r.lon0 = st[0];
    r.lat0 = st[ld];
    if constexpr (kVel) {
        r.s0 = st[2 * ld];
        r.h0 = st[3 * ld];
    }
    if (interior) {  // on a knot hit the neighbouring row is not read
        r.lon1 = st[4 * ld];
        r.lat1 = st[5 * ld];
        if constexpr (kVel) {
            r.s1 = st[6 * ld];
            r.h1 = st[7 * ld];
        }
    }
}

template <bool kVel, bool kMom>
__global__ __launch_bounds__(64) void position_query(const PosParams p) {
    const size_t q = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= p.nq) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, nq = p.nq;
    const double nan = __builtin_nan("");

    // locate: the same for every sample
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
    if (blockIdx.y == 0) {
        if (p.step) p.step[q] = row;
        if (p.frac) p.frac[q] = u;
        if (p.status) p.status[q] = status;
    }

    // the samples of this lane: all of them (per_lane = S; always so with moments, whose order is part of the definition), or
    // this grid row's one (per_lane = 1)
    const size_t s_begin = (size_t)blockIdx.y * (size_t)p.per_lane;
    const size_t s_end = s_begin + (size_t)p.per_lane;  // per_lane divides nstates
    const bool located = row >= 0;
    if (!located) {
        for (size_t s = s_begin; s < s_end; ++s) {
            const size_t o = s * nq + q;
            if (p.lon) p.lon[o] = nan;
            if (p.lat) p.lat[o] = nan;
            if constexpr (kVel) {
                if (p.speed) p.speed[o] = nan;
                if (p.heading) p.heading[o] = nan;
            }
        }
        return;  // nothing is added to count or moments
    }
    int cnt = 0;
    double ax = 0.0, ay = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
    if constexpr (kMom) {
        ax = p.anchor[q];
        ay = p.anchor[nq + q];
        cnt = p.count[q];
        m0 = p.moments[q];
        m1 = p.moments[nq + q];
        m2 = p.moments[2 * nq + q];
        m3 = p.moments[3 * nq + q];
        m4 = p.moments[4 * nq + q];
    }
    const double* st = p.states + ((size_t)row * 4) * ld + (size_t)t;  // sample s: + s * rows * 4 * ld
    const size_t sample = rows * 4 * ld;
    PosRows cur{}, nxt{};
    load_rows<kVel>(cur, st + s_begin * sample, ld, interior);
    for (size_t s = s_begin; s < s_end; ++s) {
        if (s + 1 < s_end) load_rows<kVel>(nxt, st + (s + 1) * sample, ld, interior);  // in flight during this sample's arithmetic
        double lon, lat, speed = nan, heading = nan;
        if (!interior) {
            lon = wrap180(cur.lon0);
            lat = cur.lat0;
            if constexpr (kVel) {
                speed = cur.s0;
                heading = floored_mod360(cur.h0);
            }
        } else {
            const double delta = wrap180(cur.lon1 - cur.lon0);
            if (fabs(delta) < 90.0 && is_finite(cur.lat0) && is_finite(cur.lat1)) {
                lon = wrap180(cur.lon0 + u * delta);
                lat = cur.lat0 + u * (cur.lat1 - cur.lat0);
                if constexpr (kVel) {
                    speed = cur.s0 + u * (cur.s1 - cur.s0);
                    heading = floored_mod360(cur.h0 + u * wrap180(cur.h1 - cur.h0));
                }
            } else {
                lon = lat = nan;  // a broken step
            }
        }
        const size_t o = s * nq + q;
        if (p.lon) p.lon[o] = lon;
        if (p.lat) p.lat[o] = lat;
        if constexpr (kVel) {
            if (p.speed) p.speed[o] = speed;
            if (p.heading) p.heading[o] = heading;
        }
        if constexpr (kMom) {
            const double dx = wrap180(lon - ax), dy = lat - ay;
            if (is_finite(dx) && is_finite(dy)) {
                ++cnt;
                m0 = m0 + dx;
                m1 = m1 + dy;
                m2 = m2 + dx * dx;
                m3 = m3 + dx * dy;
                m4 = m4 + dy * dy;
            }
        }
        cur = nxt;
    }
    if constexpr (kMom) {
        p.count[q] = cnt;
        p.moments[q] = m0;
        p.moments[nq + q] = m1;
        p.moments[2 * nq + q] = m2;
        p.moments[3 * nq + q] = m3;
        p.moments[4 * nq + q] = m4;
    }
}

}  // namespace
}  // namespace ste

extern "C" int ste_track_positions_f64(const ste_ukf_batch_f64* b, const ste_positions_f64* po, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_track_positions_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!po) return refuse("the position arguments (po) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!po->states) return refuse("po->states is required");
    if (!po->qtrack) return refuse("po->qtrack is required");
    if (!po->qtime) return refuse("po->qtime is required");
    if (!po->knots) return refuse("po->knots is required (the workspace of the knot times, [Nmax+1][track_stride])");
    if (int rc = refuse.nstates("po->nstates", po->nstates, " (one grid row per sample)")) return rc;
    if (po->nqueries < 1 || po->nqueries > STE_POSITIONS_MAX_QUERIES)
        return refuse("po->nqueries must be between 1 and STE_POSITIONS_MAX_QUERIES (2^26)");
    if (po->flags & ~STE_POS_REUSE_KNOTS) return refuse("po->flags has unknown bits (STE_POS_REUSE_KNOTS is the only one)");
    const bool reuse = (po->flags & STE_POS_REUSE_KNOTS) != 0;
    if (!reuse && !b->dt) return refuse("the batch's dt is required without STE_POS_REUSE_KNOTS (the knots are its sums)");
    if ((po->count != nullptr) != (po->moments != nullptr))
        return refuse("po->count and po->moments go together (both or neither)");
    if (po->count && !po->anchor) return refuse("po->anchor is required when count and moments are asked for");
    if (!po->lon && !po->lat && !po->speed && !po->heading && !po->step && !po->frac && !po->status && !po->count)
        return refuse("no output asked for (lon, lat, speed, heading, step, frac, status, count and moments are all NULL)");
    PosParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = po->nstates;
    p.ld = track_ld(b);
    p.nq = (size_t)po->nqueries;
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = po->states;
    p.qtrack = po->qtrack;
    p.qtime = po->qtime;
    p.t0 = po->t0;
    p.knots = po->knots;
    p.anchor = po->anchor;
    p.lon = po->lon;
    p.lat = po->lat;
    p.speed = po->speed;
    p.heading = po->heading;
    p.step = po->step;
    p.frac = po->frac;
    p.status = po->status;
    p.count = po->count;
    p.moments = po->moments;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!reuse) {
        hipLaunchKernelGGL(position_knots, dim3((unsigned)((p.B + 63) / 64)), dim3(64), 0, s, p);
        const int rc = abi_check_hip(hipGetLastError(), "position_knots launch");
        if (rc != STE_OK) return rc;
    }
    const bool vel = po->speed || po->heading, mom = po->count != nullptr;
    p.per_lane = mom || p.nq >= kLaneLoopQueries ? p.nstates : 1;
    const dim3 grid((unsigned)((p.nq + 63) / 64), p.per_lane == 1 ? (unsigned)p.nstates : 1u), block(64);
    with_bool(vel, [&](auto v) {
        with_bool(mom, [&](auto m) {
            hipLaunchKernelGGL((position_query<decltype(v)::value, decltype(m)::value>), grid, block, 0, s, p);
        });
    });
    return abi_check_hip(hipGetLastError(), "position_query launch");
}
