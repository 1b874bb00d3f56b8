// ste_field.hip — the values of a space-time gridded field where tracks that stay on the device were at given clock times
// (include/ste.h: ste_field_values_f64): per (sample, query) the position of ste_track_positions_f64 is formed and the field
// [nt][ny][nx] is read there, trilinear with no-data handling or at the nearest node, and the count, the moments and the
// extremes of the value OVER THE SAMPLES about an anchor are continued from call to call.  The header carries the definitions
// and tests/field_cases.py restates them in NumPy.  The locate and the interpolation along the step are those of
// ste_position.hip, restated here (tests/test_field_values.py holds the two copies to each other).
//
//   field_query<T, nearest, acc>   a lane per query.  The bisection of the track's column of knots and the time axis of the
//                                  field do not depend on the sample and are done once per lane.  The lane then loops over the
//                                  samples: always with accumulators, because the order of the additions is part of the
//                                  definition, and without them from kLaneLoopQueries queries on; shorter lists put the samples
//                                  along blockIdx.y (the mapping and the threshold of position_query).  T is the field's type,
//                                  double or float: a float field halves the bytes of the eight corner reads.
//
// The rows of the next sample are requested before the arithmetic of the current one, and the (up to) eight corner loads of a
// sample are issued together, before any of them is looked at: every corner's address is valid (clamped or wrapped), so a corner
// of weight zero is read and then left out.  The reads are gathers at addresses the query list decides; lanes of a list sorted by
// (track, time) share a track's lines and its cells.  No transcendental anywhere; every output word has one writer: plain loads
// and stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

namespace ste {
namespace {

struct FieldParams {
    int B, Nmax, nstates;
    int per_lane;           // samples a lane walks: nstates, or 1 with the samples along blockIdx.y
    size_t ld;              // tracks per row (track_stride, or B)
    size_t nq;
    const int32_t* nsteps;  // [B] or nullptr
    const double* states;   // [S][Nmax+1][4][ld]
    const int32_t* qtrack;  // [Q]
    const double* qtime;    // [Q]
    const double* t0;       // [ld] or nullptr
    const double* knots;    // [Nmax+1][ld], read only
    int nx, ny, nt;
    bool periodic;
    double lon0, lat0, dlon, dlat, lon_ref, time0, dtime, min_cover;
    const void* values;     // [nt][ny][nx] of T
    const double* vanchor;  // [Q]
    double* value;          // [S][Q] each, or nullptr
    double* cover;
    int32_t* status;        // [Q] or nullptr
    int32_t* count;         // [3][Q], [2][Q], [Q], [Q]: accumulated, each or nullptr
    double* moments;
    double* vmin;
    double* vmax;
};

constexpr size_t kLaneLoopQueries = (size_t)1 << 14;  // the threshold of position_query: 256 waves, one for every CU

// the rows one (sample, query) reads: lon and lat of row a, and of row a + 1 of an interior query
struct FieldRows {
    double lon0, lat0, lon1, lat1;
};

__device__ __forceinline__ void load_rows(FieldRows& r, const double* st, size_t ld, bool interior) {
    r.lon0 = st[0];
    r.lat0 = st[ld];
    if (interior) {  // on a knot hit the neighbouring row is not read
        r.lon1 = st[4 * ld];
        r.lat1 = st[5 * ld];
    }
}

// the two nodes and the fraction along an axis of n nodes at h = g - 0.5, by the non-periodic rule: the outer half cells are
// a constant continuation
__device__ __forceinline__ void axis_clamped(double h, int n, int& i0, int& i1, double& f) {
    const double fl = floor(h);
    if (fl < 0.0) {
        i0 = i1 = 0;
        f = 0.0;
    } else if (fl >= (double)(n - 1)) {
        i0 = i1 = n - 1;
        f = 0.0;
    } else {
        i0 = (int)fl;
        i1 = i0 + 1;
        f = h - fl;
    }
}

__device__ __forceinline__ int floored_mod_int(int i, int n) {
    i %= n;
    return i < 0 ? i + n : i;
}

enum : int { kNowhere = 0, kOnGrid = 1, kOffGrid = 2 };

// One sample at (lon, lat), slabs it0 / it1 with the fraction ft (nearest: slab it0).  -> value, cover and where it counts.
template <typename T, bool kNearest>
__device__ __forceinline__ int field_sample(const FieldParams& p, const T* __restrict__ vals, double lon, double lat, int it0,
                                            int it1, double ft, double& value, double& cover) {
    const double nan = __builtin_nan("");
    value = nan;
    cover = nan;
    if (!(is_finite(lon) && is_finite(lat))) return kNowhere;
    const double x = p.lon_ref + wrap180(lon - p.lon_ref);
    const double gx = (x - p.lon0) / p.dlon, gy = (lat - p.lat0) / p.dlat;
    const bool onx = p.periodic ? true : (gx >= 0.0 && gx < (double)p.nx);
    if (!(onx && gy >= 0.0 && gy < (double)p.ny)) {
        cover = 0.0;
        return kOffGrid;
    }
    const size_t nx = (size_t)p.nx, slab = (size_t)p.ny * nx;
    if constexpr (kNearest) {
        int ix = (int)floor(gx);
        if (p.periodic) ix = floored_mod_int(ix, p.nx);
        const int iy = (int)floor(gy);
        const double v = (double)vals[(size_t)it0 * slab + (size_t)iy * nx + (size_t)ix];
        value = v;
        cover = v == v ? 1.0 : 0.0;
        return kOnGrid;
    } else {
        int ix0, ix1, iy0, iy1;
        double fx, fy;
        const double hx = gx - 0.5;
        if (p.periodic) {
            const double fl = floor(hx);
            fx = hx - fl;
            ix0 = floored_mod_int((int)fl, p.nx);
            ix1 = ix0 + 1 == p.nx ? 0 : ix0 + 1;
        } else {
            axis_clamped(hx, p.nx, ix0, ix1, fx);
        }
        axis_clamped(gy - 0.5, p.ny, iy0, iy1, fy);
        const size_t t0 = (size_t)it0 * slab, t1 = (size_t)it1 * slab;
        const size_t r0 = (size_t)iy0 * nx, r1 = (size_t)iy1 * nx;
        // the eight corners, c = 4 e + 2 b + a, asked for together
        T raw[8];
        raw[0] = vals[t0 + r0 + (size_t)ix0];
        raw[1] = vals[t0 + r0 + (size_t)ix1];
        raw[2] = vals[t0 + r1 + (size_t)ix0];
        raw[3] = vals[t0 + r1 + (size_t)ix1];
        raw[4] = vals[t1 + r0 + (size_t)ix0];
        raw[5] = vals[t1 + r0 + (size_t)ix1];
        raw[6] = vals[t1 + r1 + (size_t)ix0];
        raw[7] = vals[t1 + r1 + (size_t)ix1];
        const double wx[2] = {1.0 - fx, fx}, wy[2] = {1.0 - fy, fy}, wt[2] = {1.0 - ft, ft};
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double w = (wt[c >> 2] * wy[(c >> 1) & 1]) * wx[c & 1];
            const double v = (double)raw[c];
            if (w != 0.0 && v == v) {
                num = num + w * v;
                den = den + w;
            }
        }
        cover = den;
        value = (den > 0.0 && den >= p.min_cover) ? num / den : nan;
        return kOnGrid;
    }
}

template <typename T, bool kNearest, bool kAcc>
__global__ __launch_bounds__(64) void field_query(const FieldParams p) {
    const size_t q = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= p.nq) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, nq = p.nq;
    const double nan = __builtin_nan("");

    // locate (ste_position.hip: position_query), then the time axis of the field: the same for every sample
    int status = 0, row = -1;
    double u = nan;
    bool interior = false;
    int it0 = 0, it1 = 0;
    double ft = 0.0;
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
            if (row >= 0 && p.nt > 1) {
                const double last = (double)(p.nt - 1);
                const double gt = (tq - p.time0) / p.dtime;
                if (!(gt >= 0.0 && gt <= last)) {
                    status = STE_FLD_TIME_OUTSIDE;  // no extrapolation in time
                    row = -1;
                } else if constexpr (kNearest) {
                    it0 = it1 = (int)fmin(floor(gt + 0.5), last);
                } else {
                    const double fl = floor(gt);
                    if (fl >= last) {
                        it0 = it1 = p.nt - 1;
                    } else {
                        it0 = (int)fl;
                        it1 = it0 + 1;
                        ft = gt - fl;
                    }
                }
            }
        }
    }
    if (blockIdx.y == 0 && p.status) p.status[q] = status;

    // the samples of this lane: all of them (per_lane = S; always so with accumulators), or this grid row's one (per_lane = 1)
    const size_t s_begin = (size_t)blockIdx.y * (size_t)p.per_lane;
    const size_t s_end = s_begin + (size_t)p.per_lane;  // per_lane divides nstates
    if (row < 0) {
        for (size_t s = s_begin; s < s_end; ++s) {
            const size_t o = s * nq + q;
            if (p.value) p.value[o] = nan;
            if (p.cover) p.cover[o] = nan;
        }
        return;  // nothing is added to any accumulator
    }
    int c0 = 0, c1 = 0, c2 = 0;
    double va = 0.0, m0 = 0.0, m1 = 0.0, lo_v = nan, hi_v = nan;
    if constexpr (kAcc) {
        va = p.vanchor[q];
        if (p.count) {
            c0 = p.count[q];
            c1 = p.count[nq + q];
            c2 = p.count[2 * nq + q];
        }
        if (p.moments) {
            m0 = p.moments[q];
            m1 = p.moments[nq + q];
        }
        if (p.vmin) lo_v = p.vmin[q];
        if (p.vmax) hi_v = p.vmax[q];
    }
    const T* __restrict__ vals = static_cast<const T*>(p.values);
    const double* st = p.states + ((size_t)row * 4) * ld + (size_t)t;  // sample s: + s * rows * 4 * ld
    const size_t sample = rows * 4 * ld;
    FieldRows cur{}, nxt{};
    load_rows(cur, st + s_begin * sample, ld, interior);
    for (size_t s = s_begin; s < s_end; ++s) {
        if (s + 1 < s_end) load_rows(nxt, st + (s + 1) * sample, ld, interior);  // in flight during this sample's arithmetic
        double lon, lat;
        if (!interior) {
            lon = wrap180(cur.lon0);
            lat = cur.lat0;
        } else {
            const double delta = wrap180(cur.lon1 - cur.lon0);
            if (fabs(delta) < 90.0 && is_finite(cur.lat0) && is_finite(cur.lat1)) {
                lon = wrap180(cur.lon0 + u * delta);
                lat = cur.lat0 + u * (cur.lat1 - cur.lat0);
            } else {
                lon = lat = nan;  // a broken step
            }
        }
        double value, cover;
        const int where = field_sample<T, kNearest>(p, vals, lon, lat, it0, it1, ft, value, cover);
        const size_t o = s * nq + q;
        if (p.value) p.value[o] = value;
        if (p.cover) p.cover[o] = cover;
        if constexpr (kAcc) {
            if (where == kOffGrid) ++c2;
            if (where == kOnGrid && value != value) ++c1;
            const double d = value - va;
            if (is_finite(value) && is_finite(d)) {
                ++c0;
                m0 = m0 + d;
                m1 = m1 + d * d;
                if (!(lo_v <= value)) lo_v = value;
                if (!(hi_v >= value)) hi_v = value;
            }
        }
        cur = nxt;
    }
    if constexpr (kAcc) {
        if (p.count) {
            p.count[q] = c0;
            p.count[nq + q] = c1;
            p.count[2 * nq + q] = c2;
        }
        if (p.moments) {
            p.moments[q] = m0;
            p.moments[nq + q] = m1;
        }
        if (p.vmin) p.vmin[q] = lo_v;
        if (p.vmax) p.vmax[q] = hi_v;
    }
}

}  // namespace
}  // namespace ste

extern "C" int ste_field_values_f64(const ste_ukf_batch_f64* b, const ste_field_f64* f, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_field_values_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!f) return refuse("the field arguments (f) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!f->states) return refuse("f->states is required");
    if (!f->qtrack) return refuse("f->qtrack is required");
    if (!f->qtime) return refuse("f->qtime is required");
    if (!f->knots)
        return refuse("f->knots is required (the knot times a previous ste_track_positions_f64 "
                      "on this batch left, [Nmax+1][track_stride])");
    if (!f->values) return refuse("f->values is required");
    if (int rc = refuse.nstates("f->nstates", f->nstates, " (one grid row per sample)")) return rc;
    if (f->nqueries < 1 || f->nqueries > STE_POSITIONS_MAX_QUERIES)
        return refuse("f->nqueries must be between 1 and STE_POSITIONS_MAX_QUERIES (2^26)");
    if (f->flags & ~(STE_GRID_PERIODIC_LON | STE_FLD_NEAREST | STE_FLD_VALUES_F32)) return refuse("f->flags has unknown bits");
    if (f->reserved != 0) return refuse("f->reserved must be 0");
    if (f->nx < 1 || f->ny < 1 || (int64_t)f->nx * (int64_t)f->ny > (int64_t)STE_GRID_MAX_CELLS)
        return refuse("f->nx and f->ny must be >= 1 and nx * ny <= STE_GRID_MAX_CELLS (2^26)");
    if (f->nt < 1 || f->nt > STE_FIELD_MAX_SLABS) return refuse("f->nt must be between 1 and STE_FIELD_MAX_SLABS (65536)");
    if (!std::isfinite(f->lon0) || !std::isfinite(f->lat0) || !std::isfinite(f->lon_ref))
        return refuse("f->lon0, f->lat0 and f->lon_ref must be finite");
    if (!std::isfinite(f->dlon) || !std::isfinite(f->dlat) || !(f->dlon >= 1e-6) || !(f->dlat >= 1e-6))
        return refuse("f->dlon and f->dlat must be finite and >= 1e-6 degrees");
    const bool periodic = (f->flags & STE_GRID_PERIODIC_LON) != 0;
    const double width = (double)f->nx * f->dlon;
    if (periodic) {
        if (width != 360.0) return refuse("STE_GRID_PERIODIC_LON needs nx * dlon == 360 exactly");
        if (!(fabs(f->lon0 - f->lon_ref) <= 360.0)) return refuse("a periodic grid's lon0 must lie within lon_ref +- 360");
    } else if (!(f->lon0 - f->lon_ref >= -90.0 && (f->lon0 + width) - f->lon_ref <= 90.0)) {
        return refuse("a grid without STE_GRID_PERIODIC_LON must lie within lon_ref +- 90 "
                      "(at most 180 degrees wide)");
    }
    if (!std::isfinite(f->time0)) return refuse("f->time0 must be finite");
    if (f->nt > 1 && !(std::isfinite(f->dtime) && f->dtime > 0.0)) return refuse("f->dtime must be finite and > 0 when nt > 1");
    if (!(f->min_cover >= 0.0 && f->min_cover <= 1.0)) return refuse("f->min_cover must lie in [0, 1]");
    const bool acc = f->count || f->moments || f->vmin || f->vmax;
    if (acc && !f->vanchor) return refuse("f->vanchor is required when count, moments, vmin or vmax is asked for");
    if (!f->value && !f->cover && !f->status && !acc)
        return refuse("no output asked for (value, cover, status, count, moments, vmin and vmax are all NULL)");
    FieldParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = f->nstates;
    p.ld = track_ld(b);
    p.nq = (size_t)f->nqueries;
    p.nsteps = b->nsteps;
    p.states = f->states;
    p.qtrack = f->qtrack;
    p.qtime = f->qtime;
    p.t0 = f->t0;
    p.knots = f->knots;
    p.nx = f->nx;
    p.ny = f->ny;
    p.nt = f->nt;
    p.periodic = periodic;
    p.lon0 = f->lon0;
    p.lat0 = f->lat0;
    p.dlon = f->dlon;
    p.dlat = f->dlat;
    p.lon_ref = f->lon_ref;
    p.time0 = f->time0;
    p.dtime = f->dtime;
    p.min_cover = f->min_cover;
    p.values = f->values;
    p.vanchor = f->vanchor;
    p.value = f->value;
    p.cover = f->cover;
    p.status = f->status;
    p.count = f->count;
    p.moments = f->moments;
    p.vmin = f->vmin;
    p.vmax = f->vmax;
    p.per_lane = acc || p.nq >= kLaneLoopQueries ? p.nstates : 1;
    const dim3 grid((unsigned)((p.nq + 63) / 64), p.per_lane == 1 ? (unsigned)p.nstates : 1u), block(64);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool f32 = (f->flags & STE_FLD_VALUES_F32) != 0, nearest = (f->flags & STE_FLD_NEAREST) != 0;
    with_bool(f32, [&](auto single) {
        using T = std::conditional_t<decltype(single)::value, float, double>;
        with_bool(nearest, [&](auto nr) {
            with_bool(acc, [&](auto ac) {
                hipLaunchKernelGGL((field_query<T, decltype(nr)::value, decltype(ac)::value>), grid, block, 0, s, p);
            });
        });
    });
    return abi_check_hip(hipGetLastError(), "field_query launch");
}
