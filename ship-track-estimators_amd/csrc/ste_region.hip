// ste_region.hip — tracks that stay on the device against a polygon (include/ste.h: ste_region_metrics_f64): time spent inside,
// the time of the first entry, the number of entries, distance sailed inside and the inside flag of every row, for S tracks per
// ship (the sampler's output, or sm_mean / fwd_mean as S = 1).  The geometry is planar in (lon, lat), which is what a GeoJSON or
// shapefile polygon means; the header carries the definitions and tests/region_metrics_cases.py restates them in NumPy.
//
//   region_metrics<model, dist>   a lane per track, samples along blockIdx.y, one in-order pass over the track's rows (the
//                                 mapping of path_metrics).  The polygon is the same for every lane: each block (one wave) stages
//                                 it in LDS once, 16 B per vertex, and every edge is then two broadcast reads.  The bounding box
//                                 of the polygon is reduced from the staged vertices (min / max are exact in any order).
//                                 (Uniform const __restrict__ loads instead of LDS were 4 - 14 % slower: DESIGN.md, "Regions".)
//
// Per step the work is one loop over the V edges that serves two tests at once: the even-odd ray test of row k + 1 (whose
// flag is carried into step k + 1) and the segment-against-edge intersections of step k.  A lane enters the loop only when row
// k + 1 lies in the polygon's bounding box or the step's bounding box meets it; when no lane of the wave does, the wave branches
// over the loop (__any), which is the common case for a fleet of which few ships are near the region.  The fraction of a step
// inside is i0 + sum over crossings of sigma (1 - u) in edge order, clamped to [0, 1]: no crossing is stored or sorted.  A
// value's bits depend on that track's rows and the polygon alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

namespace ste {
namespace {

struct RegionParams {
    int B, Nmax, nstates, nvert;
    size_t ld;              // tracks per row (track_stride, or B)
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld] or nullptr (then no time is computed)
    const double* states;   // [S][Nmax+1][4][ld]
    const double* vert;     // [2][V]
    double lon_ref;
    double* time_inside;   // [S][ld] or nullptr
    double* first_entry;   // [S][ld] or nullptr
    int32_t* nenter;       // [S][ld] or nullptr
    int32_t* nbroken;      // [S][ld] or nullptr
    double* dist_inside;   // [S][ld] or nullptr
    uint8_t* inside;       // [S][Nmax+1][ld] or nullptr
};

struct Box {
    double xmin, xmax, ymin, ymax;
};

// closed comparisons, so a NaN coordinate is outside
__device__ __forceinline__ bool in_box(const Box& b, double x, double y) {
    return x >= b.xmin && x <= b.xmax && y >= b.ymin && y <= b.ymax;
}

// does edge P -> Q toggle the even-odd count of the ray from (x, y) towards +x?
__device__ __forceinline__ bool ray_toggles(double px, double py, double qx, double qy, double x, double y) {
    if ((py > y) == (qy > y)) return false;
    return x < px + (y - py) * (qx - px) / (qy - py);
}

// Can RN(num / den) lie in [0, 1)?  False only when it certainly does not, so that the two divisions of an edge are spent on
// the few edges a step may cross; the decision itself is always taken on the quotients, as the header defines it.  den != 0.
//   |num| >= |den|                          the quotient is >= 1 or <= -1 (rounding is monotone and den / den = 1)
//   signs differ, num normal, |den| <= 2^52  the quotient is negative and at least 2^-1074 in size, so not even -0
// NaN fails both comparisons and goes on to the division.
__device__ __forceinline__ bool may_be_unit(double num, double den) {
    if (fabs(num) >= fabs(den)) return false;
    if ((num < 0.0) != (den < 0.0) && fabs(num) >= 2.2250738585072014e-308 && fabs(den) <= 4503599627370496.0) return false;
    return true;
}

__device__ bool row_inside(const double* __restrict__ vx, const double* __restrict__ vy, int V, const Box& box, double x,
                           double y) {
    bool c = false;
    if (in_box(box, x, y)) {
        double px = vx[0], py = vy[0];
        for (int i = 0; i < V; ++i) {
            const int j = i + 1 == V ? 0 : i + 1;
            const double qx = vx[j], qy = vy[j];
            if (ray_toggles(px, py, qx, qy, x, y)) c = !c;
            px = qx;
            py = qy;
        }
    }
    return c;
}

// the leg of path_metrics between two rows given in degrees: leg_km_deg (ste_geodesy.h) without its poison term, on purpose
template <int kModel>
__device__ __forceinline__ double region_leg_km(double lon1, double lat1, double lon2, double lat2) {
    if constexpr (kModel == STE_PREP_SPHERE) {
        const double a1 = lat1 * kDeg2Rad, a2 = lat2 * kDeg2Rad;
        return sphere_dist_km(lon1 * kDeg2Rad, a1, cos(a1), lon2 * kDeg2Rad, a2, cos(a2));
    } else {
        return wgs84_leg(lon1, lat1, lon2, lat2).dist_km;
    }
}

template <int kModel, bool kDist>
__global__ __launch_bounds__(64) void region_metrics(const RegionParams p) {
    const int V = p.nvert;
    Box box;
    extern __shared__ double poly[];  // px[0 .. V), py[0 .. V)
    double* vx = poly;
    double* vy = poly + V;
    box.xmin = box.ymin = __builtin_inf();
    box.xmax = box.ymax = -__builtin_inf();
    for (int i = threadIdx.x; i < V; i += 64) {
        const double x = p.vert[i], y = p.vert[V + i];
        vx[i] = x;
        vy[i] = y;
        box.xmin = fmin(box.xmin, x);
        box.xmax = fmax(box.xmax, x);
        box.ymin = fmin(box.ymin, y);
        box.ymax = fmax(box.ymax, y);
    }
    for (int o = 32; o > 0; o >>= 1) {
        box.xmin = fmin(box.xmin, __shfl_xor(box.xmin, o));
        box.xmax = fmax(box.xmax, __shfl_xor(box.xmax, o));
        box.ymin = fmin(box.ymin, __shfl_xor(box.ymin, o));
        box.ymax = fmax(box.ymax, __shfl_xor(box.ymax, o));
    }
    __syncthreads();
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = blockIdx.y;
    const int ns = track_steps(p, t);
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    uint8_t* mask = p.inside ? p.inside + (s * rows) * ld + t : nullptr;
    const bool timed = p.dt != nullptr;
    const double ref = p.lon_ref;

    double lon = st[0], lat = st[ld];
    double ax = ref + wrap180(lon - ref);
    bool i0 = row_inside(vx, vy, V, box, ax, lat);
    if (mask) mask[0] = i0 ? 1 : 0;
    double T = 0.0, tin = 0.0, din = 0.0, first = i0 ? 0.0 : __builtin_nan("");
    int nent = i0 ? 1 : 0, nbrk = 0;

    // row 1 (and dt of step 0) on their way; rows past ns are never read
    double nlon = 0.0, nlat = 0.0, ndt = 0.0;
    if (ns > 0) {
        nlon = st[4 * ld];
        nlat = st[5 * ld];
        if (timed) ndt = p.dt[t];
    }
    for (int k = 0; k < ns; ++k) {
        const double lon1 = nlon, lat1 = nlat, dtk = ndt;
        if (k + 1 < ns) {  // the next row's two loads, in flight during this step's arithmetic
            const size_t r = (size_t)k + 2;
            nlon = st[(r * 4) * ld];
            nlat = st[(r * 4 + 1) * ld];
            if (timed) ndt = p.dt[((size_t)k + 1) * ld + t];
        }
        const double x1 = ref + wrap180(lon1 - ref);  // row k + 1 as a row
        const double delta = wrap180(lon1 - lon);
        const double bx = ax + delta;                 // row k + 1 as the end of step k
        const double dx = bx - ax, dy = lat1 - lat;
        const bool sound = fabs(delta) < 90.0 && lat * 0.0 == 0.0 && lat1 * 0.0 == 0.0;
        const bool need_row = in_box(box, x1, lat1);
        // the step's bounding box against the polygon's, strict comparisons: touching boxes go through the loop
        const bool need_seg = sound && !((ax > bx ? ax : bx) < box.xmin || (ax < bx ? ax : bx) > box.xmax ||
                                         (lat > lat1 ? lat : lat1) < box.ymin || (lat < lat1 ? lat : lat1) > box.ymax);
        bool i1 = false;
        double acc = i0 ? 1.0 : 0.0, umin = 2.0;
        int ent = 0;
        if (__any(need_row || need_seg)) {
            if (need_row || need_seg) {
                // edge i is P -> Q; the vertex after Q is on its way while the edge is worked on
                double px = vx[0], py = vy[0], qx = vx[1], qy = vy[1];
                for (int i = 0; i < V; ++i) {
                    int j = i + 2;
                    j = j >= V ? j - V : j;
                    const double rx = vx[j], ry = vy[j];
                    if (need_row && ray_toggles(px, py, qx, qy, x1, lat1)) i1 = !i1;
                    if (need_seg) {
                        const double ex = qx - px, ey = qy - py, wx = px - ax, wy = py - lat;
                        const double den = dx * ey - dy * ex;
                        const double nu = wx * ey - wy * ex, nv = wx * dy - wy * dx;
                        if (den != 0.0 && may_be_unit(nu, den) && may_be_unit(nv, den)) {
                            const double u = nu / den, v = nv / den;
                            if (u >= 0.0 && u < 1.0 && v >= 0.0 && v < 1.0) {
                                if (den < 0.0) {  // entering: the polygon is counter-clockwise
                                    acc = acc + (1.0 - u);
                                    ++ent;
                                    umin = u < umin ? u : umin;
                                } else {
                                    acc = acc - (1.0 - u);
                                }
                            }
                        }
                    }
                    px = qx;
                    py = qy;
                    qx = rx;
                    qy = ry;
                }
            }
        }
        if (mask) mask[((size_t)k + 1) * ld] = i1 ? 1 : 0;
        if (sound) {
            const double f = acc < 0.0 ? 0.0 : (acc > 1.0 ? 1.0 : acc);
            if (ent > 0 && nent == 0) first = T + dtk * umin;
            nent += ent;
            tin = tin + dtk * f;
            if constexpr (kDist) {
                if (f > 0.0) din = din + region_leg_km<kModel>(lon, lat, lon1, lat1) * f;
            }
        } else {
            ++nbrk;
            if (i1 && !i0) {
                if (nent == 0) first = T + dtk;
                ++nent;
            }
        }
        T = T + dtk;
        lon = lon1;
        lat = lat1;
        ax = x1;
        i0 = i1;
    }
    const size_t o = s * ld + t;
    if (p.time_inside) p.time_inside[o] = tin;
    if (p.first_entry) p.first_entry[o] = first;
    if (p.nenter) p.nenter[o] = nent;
    if (p.nbroken) p.nbroken[o] = nbrk;
    if constexpr (kDist) p.dist_inside[o] = din;
}

template <int kModel, bool kDist>
void launch_region(const RegionParams& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.B + 63) / 64), (unsigned)p.nstates), block(64);
    const size_t lds = (size_t)p.nvert * 2 * sizeof(double);
    hipLaunchKernelGGL((region_metrics<kModel, kDist>), grid, block, lds, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_region_metrics_f64(const ste_ukf_batch_f64* b, const ste_region_f64* rg, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_region_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!rg) return refuse("the region arguments (rg) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!rg->states) return refuse("rg->states is required");
    if (!rg->vert) return refuse("rg->vert is required");
    if (int rc = refuse.nstates("rg->nstates", rg->nstates, " (one grid row per track of a ship)")) return rc;
    if (rg->nvert < 3 || rg->nvert > STE_REGION_MAX_VERT)
        return refuse("rg->nvert must be between 3 and STE_REGION_MAX_VERT (1024)");
    if (rg->reserved != 0) return refuse("rg->reserved must be 0");
    if (!std::isfinite(rg->lon_ref)) return refuse("rg->lon_ref must be finite");
    if (rg->dist_inside && refuse.model("rg->model", rg->model, " when dist_inside is asked for")) return STE_EINVAL;
    if (!b->dt && (rg->time_inside || rg->first_entry))
        return refuse("time_inside and first_entry need the batch's dt (they are sums of it)");
    if (!rg->time_inside && !rg->first_entry && !rg->nenter && !rg->nbroken && !rg->dist_inside && !rg->inside)
        return refuse("no output asked for (time_inside, first_entry, nenter, nbroken, dist_inside and inside are all NULL)");
    RegionParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = rg->nstates;
    p.nvert = rg->nvert;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = rg->states;
    p.vert = rg->vert;
    p.lon_ref = rg->lon_ref;
    p.time_inside = rg->time_inside;
    p.first_entry = rg->first_entry;
    p.nenter = rg->nenter;
    p.nbroken = rg->nbroken;
    p.dist_inside = rg->dist_inside;
    p.inside = rg->inside;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!rg->dist_inside) launch_region<STE_PREP_SPHERE, false>(p, s);
    else if (rg->model == STE_PREP_SPHERE) launch_region<STE_PREP_SPHERE, true>(p, s);
    else launch_region<STE_PREP_WGS84, true>(p, s);
    return abi_check_hip(hipGetLastError(), "region_metrics launch");
}
