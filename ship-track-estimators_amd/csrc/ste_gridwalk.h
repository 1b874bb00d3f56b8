// ste_gridwalk.h — the walk of a track's sound step through the cells of a regular lon / lat grid (include/ste.h, GRIDS:
// Pieces.), for the kernels that lay tracks on such a grid: the grid lines a step crosses, the cell it starts in, the soundness
// test of a step, and the walk itself, which hands every piece (column, row, ticks) to a sink.  ste_raster.hip is built on all
// of it; ste_grid.hip takes the leaves (Lines, grid_lines, grid_start, unit_clamp, step_ticks) and keeps its own walk, with two
// call sites of its adder, and the soundness test written out ("What the metric kernels share" and §9);
// tests/test_raster_metrics.py holds the two walks to each other.  Every expression is evaluated as written: include this
// header after ste_track.h or ste_geodesy.h, which switch contraction off for the rest of the including file.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ste.h"

namespace ste {
namespace gridwalk {

constexpr double kTicksPerHour = (double)STE_GRID_TICKS_PER_HOUR;

// what of a grid the walk needs
struct Geom {
    int nx, ny;
    bool periodic;
};

// the grid lines strictly between gA and gB, in the order met: first, last, direction (none: first past last)
struct Lines {
    int i, iend, s;
};

__device__ __forceinline__ Lines grid_lines(double gA, double gB, int n, bool periodic) {
    if (gB > gA) {
        double lo = floor(gA) + 1.0, hi = ceil(gB) - 1.0;
        if (!periodic) {
            lo = 0.0 > lo ? 0.0 : lo;
            hi = (double)n < hi ? (double)n : hi;
        }
        if (lo <= hi) return {(int)lo, (int)hi, 1};
        return {0, -1, 1};
    }
    if (gB < gA) {
        double hi = ceil(gA) - 1.0, lo = floor(gB) + 1.0;
        if (!periodic) {
            lo = 0.0 > lo ? 0.0 : lo;
            hi = (double)n < hi ? (double)n : hi;
        }
        if (lo <= hi) return {(int)hi, (int)lo, -1};
        return {0, 1, -1};
    }
    return {0, -1, 1};
}

// the index of the cell (or of the outside: -1 and n) that floor f of a grid coordinate lies in
__device__ __forceinline__ int grid_start(double f, int n, bool periodic) {
    if (periodic) return (int)f;
    f = -1.0 > f ? -1.0 : f;
    f = (double)n < f ? (double)n : f;
    return (int)f;
}

__device__ __forceinline__ double unit_clamp(double u) {
    u = 0.0 > u ? 0.0 : u;
    return 1.0 < u ? 1.0 : u;
}

// is the step from (lon, lat) over delta = wrap180(lon1 - lon) degrees of longitude to lat1 in d hours SOUND?
__device__ __forceinline__ bool step_sound(double delta, double lat, double lat1, double d) {
    return fabs(delta) < 90.0 && lat * 0.0 == 0.0 && lat1 * 0.0 == 0.0 && d >= 0.0 && d * kTicksPerHour < 4503599627370496.0;
}

// the ticks of a sound step of d hours
__device__ __forceinline__ int64_t step_ticks(double d) { return (int64_t)llrint(d * kTicksPerHour); }

// A sound step, from grid coordinates (gxA, gyA) to (gxB, gyB), (fxA, fyA) the floors of the first: its dtq ticks split at the
// grid lines it crosses (none: one piece), x-lines and y-lines merged by u, ties to x.  sink(ix, iy, q) gets every piece in the
// order sailed, the empty ones too (q == 0), with the indices before wrapping; the pieces sum to dtq.
template <class Sink>
__device__ __forceinline__ void walk(const Geom& g, Sink&& sink, double gxA, double gyA, double gxB, double gyB, double fxA,
                                     double fyA, int64_t dtq) {
    const double dgx = gxB - gxA, dgy = gyB - gyA, dtd = (double)dtq;
    Lines lx = grid_lines(gxA, gxB, g.nx, g.periodic), ly = grid_lines(gyA, gyB, g.ny, false);
    int ix = grid_start(fxA, g.nx, g.periodic), iy = grid_start(fyA, g.ny, false);
    int64_t tprev = 0;
    bool morex = (lx.i - lx.iend) * lx.s <= 0, morey = (ly.i - ly.iend) * ly.s <= 0;
    double ux = morex ? unit_clamp(((double)lx.i - gxA) / dgx) : 2.0;
    double uy = morey ? unit_clamp(((double)ly.i - gyA) / dgy) : 2.0;
    for (;;) {  // a piece per turn, the step's last piece in the last one: the sink is called from one place
        const bool more = morex || morey, takex = ux <= uy;
        int64_t tq = dtq;
        if (more) {
            tq = (int64_t)llrint((takex ? ux : uy) * dtd);
            tq = tq > tprev ? tq : tprev;
        }
        sink(ix, iy, tq - tprev);
        if (!more) break;
        tprev = tq;
        if (takex) {
            ix = lx.s > 0 ? lx.i : lx.i - 1;
            lx.i += lx.s;
            morex = (lx.i - lx.iend) * lx.s <= 0;
            ux = morex ? unit_clamp(((double)lx.i - gxA) / dgx) : 2.0;
        } else {
            iy = ly.s > 0 ? ly.i : ly.i - 1;
            ly.i += ly.s;
            morey = (ly.i - ly.iend) * ly.s <= 0;
            uy = morey ? unit_clamp(((double)ly.i - gyA) / dgy) : 2.0;
        }
    }
}

}  // namespace gridwalk
}  // namespace ste
