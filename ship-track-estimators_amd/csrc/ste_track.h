// ste_track.h — what the track-metric kernels (paths, speeds, errors, regions, grids, rasters, sites, lines, routes,
// encounters and their candidates, positions, fields, simplification) share on the device: a row as the leg functions want
// it and the leg between two such rows, the unit vector of a row, and the wave helpers.  The clamped step count, track_steps,
// is in ste_math.h (the sampler needs it too and cannot include this header).  Every expression is evaluated as written: this
// header includes ste_geodesy.h, which switches contraction off for the rest of the including file, so include it last (but
// for ste_gridwalk.h).  The host side of what the calls share is in ste_err.h.  A kernel takes a helper from here only where
// it compiles to the code it had with the helper written out (tools/kernel_code_diff.py); DESIGN.md, "What the metric
// kernels share", lists the private copies that stayed for that reason.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ste.h"
#include "ste_math.h"
#include "ste_geodesy.h"

namespace ste {
namespace {

// A row as its leg function wants it.  Sphere: radians and cos(lat), converted once per row, so that the radians and the
// cosine of row k+1 are carried from leg k into leg k+1.  WGS84: degrees.
template <int kModel>
struct TrackPoint {
    double lon, lat, c;
};
template <int kModel>
__device__ __forceinline__ TrackPoint<kModel> track_point(double lon_deg, double lat_deg) {
    if constexpr (kModel == STE_PREP_SPHERE) {
        const double lat = lat_deg * kDeg2Rad;
        return {lon_deg * kDeg2Rad, lat, cos(lat)};
    } else {
        return {lon_deg, lat_deg, 0.0};
    }
}
// the operations of leg_km_deg (ste_geodesy.h) on two such rows
template <int kModel>
__device__ __forceinline__ double track_leg_km(const TrackPoint<kModel>& a, const TrackPoint<kModel>& b) {
    if constexpr (kModel == STE_PREP_SPHERE) {
        return sphere_dist_km(a.lon, a.lat, a.c, b.lon, b.lat, b.c);
    } else {
        // a non-finite coordinate must come out as NaN whichever branch of the solver it reaches (x * 0 is 0 for finite x)
        const double poison = (a.lon + a.lat + b.lon + b.lat) * 0.0;
        return wgs84_leg(a.lon, a.lat, b.lon, b.lat).dist_km + poison;
    }
}

// the unit vector of a row given in degrees
__device__ __forceinline__ void unit_vector(double lon, double lat, double& x, double& y, double& z) {
    const double lam = lon * kDeg2Rad, phi = lat * kDeg2Rad;
    const double c = cos(phi);
    x = c * cos(lam);
    y = c * sin(lam);
    z = sin(phi);
}

// ---- wave helpers ---------------------------------------------------------------------------------------------------
// the smallest / largest v of the wave's 64 lanes, uniform
__device__ __forceinline__ int wave_min(int v) {
    for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m));
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max(int v) {
    for (int m = 32; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m));
    return __builtin_amdgcn_readfirstlane(v);
}

// x of the first active lane, in every lane
__device__ __forceinline__ int first_lane(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double first_lane(double x) {
    return __hiloint2double(first_lane(__double2hiint(x)), first_lane(__double2loint(x)));
}
// x of lane l (uniform), in every lane
__device__ __forceinline__ double lane_value(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// the value of lane l - 1; lane 0 gets something its caller replaces
__device__ __forceinline__ int lane_up(int x) {
#ifdef STE_ROUTE_DPP  // a DPP wave shift instead of ds_bpermute, for timing ("Routes")
    return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false);
#else
    return __shfl_up(x, 1, 64);
#endif
}
__device__ __forceinline__ double lane_up(double x) {
    return __hiloint2double(lane_up(__double2hiint(x)), lane_up(__double2loint(x)));
}

}  // namespace
}  // namespace ste
