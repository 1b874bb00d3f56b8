// ste_path.hip — path quantities of tracks that stay on the device (include/ste.h: ste_path_metrics_f64): distance sailed
// and the time of the first crossing of a meridian or a parallel, for S tracks per ship (the sampler's output, or sm_mean /
// fwd_mean as S = 1).
//
// What the reference offers for this is a per-ship Python loop over utils.haversine_formula / geographiclib_distance
// (utils.py:9-113) on a downloaded history; for posterior samples that download is S x [Nmax+1][4][B] doubles, while the values
// wanted are one or two doubles per (sample, ship).
//
//   path_metrics<model, line>   a lane per track, samples along blockIdx.y (the mapping of urtss_sample_recur), one sequential
//                               pass over the track's rows.  The sum is sequential on purpose: leg k is added to the sum of
//                               legs 0 .. k-1, so dist IS cumdist row nsteps, and a value's bits depend on that track's rows
//                               alone -- not on S, the window, or which outputs were asked for.
//
// The loop reads 16 B per (sample, track, row) and spends a haversine (sphere: ~6 transcendentals, since radians and cos(lat)
// of row k+1 are carried into leg k+1) or an inverse geodesic (WGS84: wgs84_leg works on degrees and reduces its arguments
// itself, so nothing carries over) on them: it is bound by fp64 arithmetic and, for few waves, by the latency of the row
// loads, which is why the next row's two loads are issued before the arithmetic of the current leg.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

namespace ste {
namespace {

struct PathParams {
    int B, Nmax, nstates, axis;  // axis: 0 = meridian, 1 = parallel (read by the line kernels only)
    size_t ld;                   // tracks per row (track_stride, or B)
    const int32_t* nsteps;       // [B] or nullptr
    const double* dt;            // [Nmax][ld] (line kernels only)
    const double* states;        // [S][Nmax+1][4][ld]
    const double* line_value;    // [ld]
    double* dist;                // [S][ld] or nullptr
    double* cumdist;             // [S][Nmax+1][ld] or nullptr
    double* cross_time;          // [S][ld] or nullptr
    int32_t* ncross;             // [S][ld] or nullptr
};

// signed offset of a row from the line, degrees: lat - v for a parallel, wrap180(lon - v) for a meridian
__device__ __forceinline__ double line_offset(int axis, double lon_deg, double lat_deg, double v) {
    return axis == 1 ? lat_deg - v : wrap180(lon_deg - v);
}

template <int kModel, bool kLine>
__global__ __launch_bounds__(64) void path_metrics(const PathParams p) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = blockIdx.y;
    const int ns = track_steps(p, t);
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    double* cum = p.cumdist ? p.cumdist + (s * rows) * ld + t : nullptr;

    double lon = st[0], lat = st[ld];
    TrackPoint<kModel> cur = track_point<kModel>(lon, lat);
    double dist = 0.0;
    if (cum) cum[0] = 0.0;

    // crossing state: held by the line kernels only
    double v = 0.0, a0 = 0.0, T = 0.0, dtk = 0.0, first = __builtin_nan("");
    int nc = 0;
    if constexpr (kLine) {
        v = p.line_value[t];
        a0 = line_offset(p.axis, lon, lat, v);
    }
    // row 1 (and dt of step 0) on their way; rows past ns are never read
    double nlon = 0.0, nlat = 0.0, ndt = 0.0;
    if (ns > 0) {
        nlon = st[4 * ld];
        nlat = st[5 * ld];
        if constexpr (kLine) ndt = p.dt[t];
    }
    for (int k = 0; k < ns; ++k) {
        lon = nlon;
        lat = nlat;
        if constexpr (kLine) dtk = ndt;
        if (k + 1 < ns) {  // the next row's two loads, in flight during this leg's arithmetic
            const size_t r = (size_t)k + 2;
            nlon = st[(r * 4) * ld];
            nlat = st[(r * 4 + 1) * ld];
            if constexpr (kLine) ndt = p.dt[((size_t)k + 1) * ld + t];
        }
        const TrackPoint<kModel> nxt = track_point<kModel>(lon, lat);
        dist += track_leg_km<kModel>(cur, nxt);
        if (cum) cum[((size_t)k + 1) * ld] = dist;
        cur = nxt;
        if constexpr (kLine) {
            const double a1 = line_offset(p.axis, lon, lat, v);
            const double d = a0 - a1;
            // d finite: both offsets are; |d| < 180 always holds for a parallel between finite latitudes
            bool cross = ((a0 < 0.0) != (a1 < 0.0)) && (d * 0.0 == 0.0);
            if (p.axis == 0) cross = cross && fabs(a1 - a0) < 180.0;
            if (cross) {
                if (nc == 0) first = T + dtk * a0 / d;
                ++nc;
            }
            T += dtk;
            a0 = a1;
        }
    }
    if (p.dist) p.dist[s * ld + t] = dist;
    if constexpr (kLine) {
        if (p.cross_time) p.cross_time[s * ld + t] = first;
        if (p.ncross) p.ncross[s * ld + t] = nc;
    }
}

template <int kModel, bool kLine>
void launch_path(const PathParams& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.B + 63) / 64), (unsigned)p.nstates), block(64);
    hipLaunchKernelGGL((path_metrics<kModel, kLine>), grid, block, 0, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_path_metrics_f64(const ste_ukf_batch_f64* b, const ste_path_f64* pm, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_path_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!pm) return refuse("the path arguments (pm) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!pm->states) return refuse("pm->states is required");
    if (int rc = refuse.nstates("pm->nstates", pm->nstates, " (one grid row per track of a ship)")) return rc;
    if (int rc = refuse.model("pm->model", pm->model)) return rc;
    if (pm->line_axis < -1 || pm->line_axis > 1)
        return refuse("pm->line_axis must be -1 (no line), 0 (meridian) or 1 (parallel)");
    if (pm->reserved != 0) return refuse("pm->reserved must be 0");
    const bool line = pm->line_axis >= 0;
    if (line && !pm->line_value) return refuse("a line needs pm->line_value");
    if (line && !b->dt) return refuse("a line needs the batch's dt (crossing times are sums of it)");
    if (!line && (pm->cross_time || pm->ncross)) return refuse("pm->cross_time and pm->ncross need a line (line_axis 0 or 1)");
    if (!pm->dist && !pm->cumdist && !pm->cross_time && !pm->ncross)
        return refuse("no output asked for (dist, cumdist, cross_time and ncross are all NULL)");
    PathParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = pm->nstates;
    p.axis = pm->line_axis;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = pm->states;
    p.line_value = pm->line_value;
    p.dist = pm->dist;
    p.cumdist = pm->cumdist;
    p.cross_time = pm->cross_time;
    p.ncross = pm->ncross;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool sphere = pm->model == STE_PREP_SPHERE;
    if (sphere && line) launch_path<STE_PREP_SPHERE, true>(p, s);
    else if (sphere) launch_path<STE_PREP_SPHERE, false>(p, s);
    else if (line) launch_path<STE_PREP_WGS84, true>(p, s);
    else launch_path<STE_PREP_WGS84, false>(p, s);
    return abi_check_hip(hipGetLastError(), "path_metrics launch");
}
