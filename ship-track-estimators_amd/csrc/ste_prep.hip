// ste_prep.hip — observation preparation for a batch of tracks: speed / course over ground and their rates.
//
// Device counterpart of ShipTrack.calculate_sog / calculate_cog / calculate_sog_rate / calculate_cog_rate /
// get_measurements (reference src/track_estimators/ship_track.py:197-338) for many tracks at once: one thread per
// (observation, track), track index fastest, every read and write coalesced.  The kernel is pure streaming work
// (24 B in, 64 B out per observation) with ~10 transcendentals per observation on the sphere and a short fixed-point
// Newton iteration on the ellipsoid, so it is HBM/latency trivial next to the filter; it exists so that raw lon/lat/time can
// go to smoothed tracks without a per-ship Python loop.
//
//   model 0  sphere of radius 6378.137 km: haversine_formula + heading        (reference utils.py:75-147)
//   model 1  WGS84 inverse geodesic: geographiclib_distance + _heading         (reference utils.py:9-72)
//            geographiclib itself is a third-party dependency that is not part of the reference tree; the inverse
//            problem is solved by its published algorithm (Karney 2013), exactly as track_estimators/geodesic.py does on
//            the host (it reproduces the reference's CLI fixture to the last bit, tests/test_geodesic_karney.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_math.h"
#include "ste_geodesy.h"  // last: it switches contraction off for the rest of the file

// The leg functions (Leg, sphere_leg, wgs84_leg) live in ste_geodesy.h; like them, the rates below must keep exact zeros
// (0 / 0 = NaN on a duplicate timestamp), so this file is compiled without contraction.
#pragma clang fp contract(off)

namespace ste {
namespace {

struct PrepParams {
    int B, T, model;
    const int32_t* nobs;
    const double *lon, *lat, *gap;
    double *sog, *cog, *sog_rate, *cog_rate, *z;
    int32_t* status;
};

template <int kModel>
__device__ __forceinline__ Leg leg_of(const PrepParams& p, int j, int t) {
    const size_t a = (size_t)j * p.B + t, b = a + p.B;
    const double lon1 = p.lon[a], lat1 = p.lat[a], lon2 = p.lon[b], lat2 = p.lat[b];
    return kModel == 0 ? sphere_leg(lon1, lat1, lon2, lat2) : wgs84_leg(lon1, lat1, lon2, lat2);
}

// Observation i of a track with n observations uses leg j = min(i, n-2) (the last value is repeated,
// ship_track.py:220, :275); its rate is the backward difference against observation i-1 over gap[i-1], 0 for i = 0
// (ship_track.py:242-246, :296-300).  The previous observation's leg is recomputed here rather than read back, so the
// kernel is one pass with no ordering between threads; both evaluations run the same code and agree bit for bit.
template <int kModel>
__global__ void __launch_bounds__(256) track_prep(PrepParams p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.T * p.B) return;
    const int t = (int)(idx % p.B), i = (int)(idx / p.B);
    const int n = p.nobs ? min(p.nobs[t], p.T) : p.T;
    double sog = 0.0, cog = 0.0, sr = 0.0, cr = 0.0;
    if (i < n && n >= 2) {
        const int j = min(i, n - 2);
        const Leg cur = leg_of<kModel>(p, j, t);
        if (kModel == 1 && !cur.converged && p.status) atomicOr(&p.status[t], STE_PREP_STATUS_NOCONV);
        sog = cur.dist_km / p.gap[(size_t)j * p.B + t];
        cog = cur.head_deg;
        if (i >= 1) {
            const int jp = min(i - 1, n - 2);
            double sog_p = sog, cog_p = cog;
            if (jp != j) {
                const Leg prev = leg_of<kModel>(p, jp, t);
                sog_p = prev.dist_km / p.gap[(size_t)jp * p.B + t];
                cog_p = prev.head_deg;
            }
            const double g = p.gap[(size_t)(i - 1) * p.B + t];
            sr = (sog - sog_p) / g;
            cr = (cog - cog_p) / g;
        }
    }
    p.sog[idx] = sog;
    p.cog[idx] = cog;
    p.sog_rate[idx] = sr;
    p.cog_rate[idx] = cr;
    if (p.z) {
        const size_t zb = ((size_t)i * 4) * p.B + t;
        const bool live = i < n;
        p.z[zb] = live ? p.lon[idx] : 0.0;
        p.z[zb + p.B] = live ? p.lat[idx] : 0.0;
        p.z[zb + 2 * (size_t)p.B] = sog;
        p.z[zb + 3 * (size_t)p.B] = cog;
    }
}

}  // namespace
}  // namespace ste

extern "C" int ste_track_prep_f64(const ste_prep_batch_f64* b, void* stream) {
    using namespace ste;
    if (!b) return abi_fail(STE_EINVAL, "prep batch pointer is NULL");
    if (b->B <= 0 || b->Tmax < 1) return abi_fail(STE_EINVAL, "B must be > 0 and Tmax >= 1");
    if (b->model != STE_PREP_SPHERE && b->model != STE_PREP_WGS84)
        return abi_fail(STE_EINVAL, "model must be STE_PREP_SPHERE or STE_PREP_WGS84");
    if (!b->lon || !b->lat || !b->sog || !b->cog || !b->sog_rate || !b->cog_rate)
        return abi_fail(STE_EINVAL, "lon, lat, sog, cog, sog_rate and cog_rate are required");
    if (b->Tmax > 1 && !b->gap) return abi_fail(STE_EINVAL, "gap is required when Tmax > 1");
    PrepParams p{b->B, b->Tmax, b->model, b->nobs, b->lon, b->lat, b->gap, b->sog, b->cog, b->sog_rate, b->cog_rate, b->z,
                 b->status};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (b->status) {
        int rc = abi_check_hip(hipMemsetAsync(b->status, 0, sizeof(int32_t) * (size_t)b->B, s), "track_prep status reset");
        if (rc) return rc;
    }
    const size_t total = (size_t)b->B * b->Tmax;
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (b->model == STE_PREP_SPHERE)
        hipLaunchKernelGGL(track_prep<0>, dim3(grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(track_prep<1>, dim3(grid), dim3(256), 0, s, p);
    return abi_check_hip(hipGetLastError(), "track_prep launch");
}
