// ste_grid.hip — tracks that stay on the device on a regular lon / lat grid (include/ste.h: ste_grid_metrics_f64): the time every
// cell of the grid is occupied, summed over the tracks of the call, and how often a cell is entered.  Time is counted in integer
// ticks of 2^-20 h, so the sums are exact and do not depend on the order of the additions: windows, sample chunks and launch
// order cannot move a bit of the grid.  The header carries the definitions; tests/grid_metrics_cases.py restates them in Python.
//
//   grid_metrics   a lane per track, samples along blockIdx.y, one in-order pass over the track's rows (the mapping of
//                  path_metrics and region_metrics); the next row's two loads and the next dt are issued before the current
//                  step's arithmetic.  A lane keeps its current run -- (cell, ticks) -- in registers and issues one no-return
//                  64-bit integer atomic add to `ticks` (and one to `entries`) when the cell changes and at the end of the track.
//                  For a grid of at most 256 cells (kLds) the adds go to a copy of the grid in LDS, which the block adds to
//                  the grid cell by cell at its end: on so small a grid many lanes flush to one address, and that is 4 times
//                  slower in global memory.  Larger copies cost more in occupancy than they save ("Grids").
//
// A step whose two ends have the same floor on both axes crosses no grid line: its ticks go to the run with no further
// division.  Every other step goes to the walker, which merges the x-lines and the y-lines the step crosses by their parameter
// u; it sits behind __any, so a wave none of whose ships changes its cell in a step never enters it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last but the walk: it switches contraction off for the rest of the file
#include "ste_gridwalk.h"

namespace ste {
namespace {

using namespace gridwalk;  // kTicksPerHour, Lines, grid_lines, grid_start, unit_clamp, step_ticks

struct GridParams {
    int B, Nmax, nstates, nx, ny;
    bool periodic;
    size_t ld;              // tracks per row (track_stride, or B)
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld]
    const double* states;   // [S][Nmax+1][4][ld]
    double lon0, lat0, dlon, dlat, lon_ref;
    int64_t* ticks;    // [ny][nx] or nullptr
    int64_t* entries;  // [ny][nx] or nullptr
    int64_t* outside;  // [S][ld] or nullptr
    int64_t* total;    // [S][ld] or nullptr
    int32_t* nbroken;  // [S][ld] or nullptr
};

constexpr int kRunNone = -2;     // no piece yet
constexpr int kRunOutside = -1;  // off the grid

constexpr int kLdsCells = 256;  // grids of up to this many cells are summed in a copy per block ("Grids")

// relaxed, no return value: nothing in the kernel reads the grid
__device__ __forceinline__ void grid_add(int64_t* base, int cell, int64_t v) {
    __hip_atomic_fetch_add(base + cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lds_add(int64_t* base, int cell, int64_t v) {
    __hip_atomic_fetch_add(base + cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The run of a track: a maximal stretch of consecutive non-empty pieces in one cell.  (ix, iy) are the indices the last piece
// was filed under, before wrapping: a piece with the same pair is in the same cell, and needs no index arithmetic.
struct Run {
    int cell, ix, iy;
    int64_t acc, outside;
    int64_t *tk, *en;  // where the run's ticks and entries go: the grid, or the block's copy of it
};

template <bool kLds>
__device__ __forceinline__ void run_flush(const GridParams& p, Run& r) {
    if (r.cell == kRunOutside) r.outside += r.acc;
    else if (r.cell >= 0 && r.tk) {
        if constexpr (kLds) lds_add(r.tk, r.cell, r.acc);
        else grid_add(r.tk, r.cell, r.acc);
    }
}

template <bool kLds>
__device__ __forceinline__ void run_add(const GridParams& p, Run& r, int ix, int iy, int64_t q) {
    if (q == 0) return;  // a piece of no ticks adds nothing and is no entry
    if (r.cell != kRunNone && ix == r.ix && iy == r.iy) {
        r.acc += q;
        return;
    }
    r.ix = ix;
    r.iy = iy;
    if (p.periodic) {
        ix %= p.nx;
        ix = ix < 0 ? ix + p.nx : ix;
    }
    const int c = (ix >= 0 && ix < p.nx && iy >= 0 && iy < p.ny) ? iy * p.nx + ix : kRunOutside;
    if (c != r.cell) {
        run_flush<kLds>(p, r);
        r.cell = c;
        r.acc = 0;
        if (c >= 0 && r.en) {
            if constexpr (kLds) lds_add(r.en, c, 1);
            else grid_add(r.en, c, 1);
        }
    }
    r.acc += q;
}

// A sound step that crosses grid lines: its dtq ticks split at the lines, x-lines and y-lines merged by u, ties to x.  The
// pieces of gridwalk::walk, from the same leaves, but with two call sites of the adder.
template <bool kLds>
__device__ void grid_walk(const GridParams& p, Run& r, double gxA, double gyA, double gxB, double gyB, double fxA, double fyA,
                          int64_t dtq) {
    const double dgx = gxB - gxA, dgy = gyB - gyA, dtd = (double)dtq;
    Lines lx = grid_lines(gxA, gxB, p.nx, p.periodic), ly = grid_lines(gyA, gyB, p.ny, false);
    int ix = grid_start(fxA, p.nx, p.periodic), iy = grid_start(fyA, p.ny, false);
    int64_t tprev = 0;
    bool morex = (lx.i - lx.iend) * lx.s <= 0, morey = (ly.i - ly.iend) * ly.s <= 0;
    double ux = morex ? unit_clamp(((double)lx.i - gxA) / dgx) : 2.0;
    double uy = morey ? unit_clamp(((double)ly.i - gyA) / dgy) : 2.0;
    while (morex || morey) {
        const bool takex = ux <= uy;
        int64_t tq = (int64_t)llrint((takex ? ux : uy) * dtd);
        tq = tq > tprev ? tq : tprev;
        run_add<kLds>(p, r, ix, iy, tq - tprev);
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
    run_add<kLds>(p, r, ix, iy, dtq - tprev);
}

// one track: tk and en are where its runs' ticks and entries go (the grid, or the block's copy of it), or nullptr
template <bool kLds>
__device__ __forceinline__ void grid_track(const GridParams& p, size_t t, size_t sample, int64_t* tk, int64_t* en) {
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = sample;
    const int ns = track_steps(p, t);
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    const double ref = p.lon_ref;
    Run r{kRunNone, 0, 0, 0, 0, tk, en};
    int64_t total = 0;
    int nbrk = 0;
    if (ns > 0) {
        double lon = st[0], lat = st[ld];
        double ax = ref + wrap180(lon - ref);
        double gyA = (lat - p.lat0) / p.dlat;
        // row 1 and dt of step 0 on their way; rows past ns are never read
        double nlon = st[4 * ld], nlat = st[5 * ld], ndt = p.dt[t];
        for (int k = 0; k < ns; ++k) {
            const double lon1 = nlon, lat1 = nlat, d = ndt;
            if (k + 1 < ns) {  // the next row's two loads and the next dt, in flight during this step's arithmetic
                const size_t rw = (size_t)k + 2;
                nlon = st[(rw * 4) * ld];
                nlat = st[(rw * 4 + 1) * ld];
                ndt = p.dt[((size_t)k + 1) * ld + t];
            }
            const double x1 = ref + wrap180(lon1 - ref);
            const double delta = wrap180(lon1 - lon);
            const double gyB = (lat1 - p.lat0) / p.dlat;  // gyA of the next step: the same expression
            // step_sound(delta, lat, lat1, d), written out: through the function the comparisons come out in another order
            const bool sound = fabs(delta) < 90.0 && lat * 0.0 == 0.0 && lat1 * 0.0 == 0.0 && d >= 0.0 &&
                               d * kTicksPerHour < 4503599627370496.0;
            int64_t dtq = 0;
            double gxA = 0.0, gxB = 0.0, fxA = 0.0, fyA = 0.0;
            bool walk = false;
            if (sound) {
                dtq = step_ticks(d);
                total += dtq;
                gxA = (ax - p.lon0) / p.dlon;
                gxB = ((ax + delta) - p.lon0) / p.dlon;
                fxA = floor(gxA);
                fyA = floor(gyA);
                walk = !(fxA == floor(gxB) && fyA == floor(gyB));
            } else {
                ++nbrk;
            }
            if (__any(walk)) {
                if (walk) grid_walk<kLds>(p, r, gxA, gyA, gxB, gyB, fxA, fyA, dtq);
            }
            if (sound && !walk) run_add<kLds>(p, r, grid_start(fxA, p.nx, p.periodic), grid_start(fyA, p.ny, false), dtq);
            lon = lon1;
            lat = lat1;
            ax = x1;
            gyA = gyB;
        }
        run_flush<kLds>(p, r);
    }
    const size_t o = s * ld + t;
    if (p.outside) p.outside[o] = r.outside;
    if (p.total) p.total[o] = total;
    if (p.nbroken) p.nbroken[o] = nbrk;
}

template <bool kLds>
__global__ __launch_bounds__(64) void grid_metrics(const GridParams p) {
    extern __shared__ int64_t copy[];  // kLds: ticks[nx * ny] if asked for, then entries[nx * ny] if asked for
    const int ncell = p.nx * p.ny;
    int64_t *tk = p.ticks, *en = p.entries;
    if constexpr (kLds) {
        tk = p.ticks ? copy : nullptr;
        en = p.entries ? copy + (p.ticks ? ncell : 0) : nullptr;
        const int n = ncell * ((p.ticks ? 1 : 0) + (p.entries ? 1 : 0));
        for (int c = threadIdx.x; c < n; c += 64) copy[c] = 0;
        __syncthreads();
    }
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t < (size_t)p.B) grid_track<kLds>(p, t, blockIdx.y, tk, en);
    if constexpr (kLds) {  // the block's sums into the grid, a cell per lane
        __syncthreads();
        for (int c = threadIdx.x; c < ncell; c += 64) {
            if (tk && tk[c]) grid_add(p.ticks, c, tk[c]);
            if (en && en[c]) grid_add(p.entries, c, en[c]);
        }
    }
}

}  // namespace
}  // namespace ste

extern "C" int ste_grid_metrics_f64(const ste_ukf_batch_f64* b, const ste_grid_f64* g, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_grid_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!g) return refuse("the grid arguments (g) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!g->states) return refuse("g->states is required");
    if (int rc = refuse.nstates("g->nstates", g->nstates, " (one grid row per track of a ship)")) return rc;
    if (g->flags & ~STE_GRID_PERIODIC_LON) return refuse("g->flags has unknown bits");
    if (g->nx < 1 || g->ny < 1 || (int64_t)g->nx * (int64_t)g->ny > (int64_t)STE_GRID_MAX_CELLS)
        return refuse("g->nx and g->ny must be >= 1 and nx * ny <= STE_GRID_MAX_CELLS (2^26)");
    if (!std::isfinite(g->lon0) || !std::isfinite(g->lat0) || !std::isfinite(g->lon_ref))
        return refuse("g->lon0, g->lat0 and g->lon_ref must be finite");
    if (!std::isfinite(g->dlon) || !std::isfinite(g->dlat) || !(g->dlon >= 1e-6) || !(g->dlat >= 1e-6))
        return refuse("g->dlon and g->dlat must be finite and >= 1e-6 degrees");
    const bool periodic = (g->flags & STE_GRID_PERIODIC_LON) != 0;
    const double width = (double)g->nx * g->dlon;
    if (periodic) {
        if (width != 360.0) return refuse("STE_GRID_PERIODIC_LON needs nx * dlon == 360 exactly");
        if (!(fabs(g->lon0 - g->lon_ref) <= 360.0)) return refuse("a periodic grid's lon0 must lie within lon_ref +- 360");
    } else if (!(g->lon0 - g->lon_ref >= -90.0 && (g->lon0 + width) - g->lon_ref <= 90.0)) {
        return refuse("a grid without STE_GRID_PERIODIC_LON must lie within lon_ref +- 90 "
                      "(at most 180 degrees wide)");
    }
    if (!b->dt) return refuse("the batch's dt is required (every output is a sum of it)");
    if (!g->ticks && !g->entries && !g->outside && !g->total && !g->nbroken)
        return refuse("no output asked for (ticks, entries, outside, total and nbroken are all NULL)");
    GridParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = g->nstates;
    p.nx = g->nx;
    p.ny = g->ny;
    p.periodic = periodic;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = g->states;
    p.lon0 = g->lon0;
    p.lat0 = g->lat0;
    p.dlon = g->dlon;
    p.dlat = g->dlat;
    p.lon_ref = g->lon_ref;
    p.ticks = g->ticks;
    p.entries = g->entries;
    p.outside = g->outside;
    p.total = g->total;
    p.nbroken = g->nbroken;
    const dim3 grid((unsigned)((p.B + 63) / 64), (unsigned)p.nstates), block(64);
    if (p.nx * p.ny <= kLdsCells) {
        const size_t lds = (size_t)p.nx * p.ny * 8 * ((p.ticks ? 1 : 0) + (p.entries ? 1 : 0));
        hipLaunchKernelGGL(grid_metrics<true>, grid, block, lds, static_cast<hipStream_t>(stream), p);
        return abi_check_hip(hipGetLastError(), "grid_metrics launch");
    }
    hipLaunchKernelGGL(grid_metrics<false>, grid, block, 0, static_cast<hipStream_t>(stream), p);
    return abi_check_hip(hipGetLastError(), "grid_metrics launch");
}
