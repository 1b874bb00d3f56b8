// ste_raster.hip — tracks that stay on the device against a gridded field (include/ste.h: ste_raster_metrics_f64): a land mask,
// a depth, a density.  The gather half of ste_grid.hip: a lane walks its track's pieces through the cells of the grid and READS
// the value of every cell it comes to, where the grid kernel adds ticks to it.  Time is counted in integer ticks of 2^-20 h and
// every floating-point sum takes its terms in track order, so windows, sample slices and the outputs asked for cannot move a
// bit.  The header carries the definitions; tests/raster_cases.py restates them in Python.
//
//   raster_metrics   a lane per track, samples along blockIdx.y, one in-order pass over the track's rows (the mapping of
//                    grid_metrics); the next row's two loads and the next dt are issued before the current step's arithmetic.
//                    A lane keeps its current run -- (cell, ticks, start, value) -- in registers.  The run's value is asked
//                    for when the run begins (one scattered 8-byte load, a lane per address) and looked at when the run ends:
//                    the weighted sum, the extremes, the hit test and the excursions all happen at the flush, so the load has
//                    the whole run to come back.  Instantiated on what changes the loop: the threshold outputs, row_value,
//                    and a copy of the raster in LDS ("Rasters", has the forms measured).
//
// A step that crosses no grid line and stays in the cell of the lane's run adds its ticks to the run with no further division.
// Every other step goes to the walker of ste_gridwalk.h behind __any, as in grid_metrics; a step that crosses no line but
// begins a run (the track's first, the first after a broken step that moved the ship) is one piece of the walker, so the
// code of a cell change exists once in the loop.
//
// Two forms that DESIGN.md measures against the one above are kept as build options of this file, bit for bit the same:
//   -DSTE_RASTER_EAGER=1        the value is looked at where it is asked for: NaN test, extremes and hit test at the cell change
//   -DSTE_RASTER_LDS_CELLS=n    rasters of at most n cells are staged in LDS by the block and read from there
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last but the walk: it switches contraction off for the rest of the file
#include "ste_gridwalk.h"

#ifndef STE_RASTER_EAGER
#define STE_RASTER_EAGER 0
#endif
#ifndef STE_RASTER_LDS_CELLS
#define STE_RASTER_LDS_CELLS 0  // no copy in LDS: DESIGN.md, "Rasters"
#endif

namespace ste {
namespace {

struct RasterParams {
    int B, Nmax, nstates;
    gridwalk::Geom g;
    bool below;
    size_t ld;              // tracks per row (track_stride, or B)
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld]
    const double* states;   // [S][Nmax+1][4][ld]
    const double* values;   // [ny][nx]
    double lon0, lat0, dlon, dlat, lon_ref, threshold;
    int64_t min_ticks;
    double* row_value;  // [S][Nmax+1][ld] or nullptr
};

// The per-track outputs, [S][ld] or nullptr each: the kernel's second argument.  They are wanted once, after the loop.  Read as
// arguments in the ordinary way they are loaded at the kernel's start and hold 30 scalar registers through the loop, which
// then runs out of them (up to 29 spilled to lanes); `late_outputs` reads them from the argument block where they are used.
struct RasterOut {
    int64_t *total, *outside, *valid, *nodata, *tmin, *tmax, *hit_ticks, *hit_first, *hit_longest;
    int32_t *nbroken, *nhit, *nhit_long;
    double *wsum, *vmin, *vmax;
};
constexpr size_t kOutOffset = (sizeof(RasterParams) + alignof(RasterOut) - 1) / alignof(RasterOut) * alignof(RasterOut);

__device__ __forceinline__ const RasterOut& late_outputs() {
    const char* args = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    return *(const RasterOut*)(args + kOutOffset);
}

constexpr bool kEager = STE_RASTER_EAGER != 0;
constexpr int kLdsCells = STE_RASTER_LDS_CELLS;
constexpr int kRunNone = -2;     // no piece yet
constexpr int kRunOutside = -1;  // off the grid

// The run of a track and what the track has gathered so far.  (ix, iy) are the indices the last piece was filed under, before
// wrapping: a piece with the same pair is in the same cell, and needs no index arithmetic.
struct Run {
    int cell = kRunNone, ix = 0, iy = 0;
    int64_t acc = 0, start = 0, clock = 0;  // the run's ticks and start; the ticks of all pieces so far
    double v = 0.0;                         // the run's value, asked for when it began
    bool nan = false, hit = false;          // what `classify` made of v
    int64_t outside = 0, valid = 0, nodata = 0;
    double wsum = 0.0, vmin = NAN, vmax = NAN;
    int64_t tmin = -1, tmax = -1;
    // the threshold outputs; exc: the ticks of the excursion that is open, -1 = none
    int64_t hit_ticks = 0, hit_first = -1, hit_longest = 0, exc = -1;
    int nhit = 0, nhit_long = 0;
};

__device__ __forceinline__ void excursion_end(const RasterParams& p, Run& r) {
    if (r.exc >= 0) {
        if (r.exc >= p.min_ticks) ++r.nhit_long;
        r.hit_longest = r.exc > r.hit_longest ? r.exc : r.hit_longest;
        r.exc = -1;
    }
}

// what a run on the grid is, from its value alone: no data, the extremes, a hit
template <bool kThr>
__device__ __forceinline__ void classify(const RasterParams& p, Run& r) {
    const double v = r.v;
    r.nan = v != v;
    if (r.nan) return;
    if (!(r.vmin <= v)) {
        r.vmin = v;
        r.tmin = r.start;
    }
    if (!(r.vmax >= v)) {
        r.vmax = v;
        r.tmax = r.start;
    }
    if constexpr (kThr) r.hit = p.below ? v <= p.threshold : v >= p.threshold;
}

template <bool kThr>
__device__ __forceinline__ void run_flush(const RasterParams& p, Run& r) {
    if (r.cell == kRunNone) return;
    const bool on = r.cell >= 0;
    if constexpr (!kEager) {
        if (on) classify<kThr>(p, r);
    }
    // selects, not branches: three sums behind one branch each become one store through a chosen address, and the run
    // would live in scratch
    const bool ok = on && !r.nan;
    const int64_t a = r.acc;
    r.outside += on ? 0 : a;
    r.nodata += on && r.nan ? a : 0;
    r.valid += ok ? a : 0;
    if (ok) r.wsum = r.wsum + (double)a * r.v;
    const bool hit = kThr && ok && r.hit;
    if constexpr (kThr) {
        if (hit) {
            r.hit_ticks += r.acc;
            r.hit_first = r.hit_first < 0 ? r.start : r.hit_first;
            if (r.exc < 0) {
                r.exc = 0;
                ++r.nhit;
            }
            r.exc += r.acc;
        } else {
            excursion_end(p, r);
        }
    }
}

template <bool kThr>
__device__ __forceinline__ void run_add(const RasterParams& p, const double* vals, Run& r, int ix, int iy, int64_t q) {
    if (q == 0) return;  // a piece of no ticks is no piece
    if (r.cell != kRunNone && ix == r.ix && iy == r.iy) {
        r.acc += q;
        r.clock += q;
        return;
    }
    r.ix = ix;
    r.iy = iy;
    if (p.g.periodic) {
        ix %= p.g.nx;
        ix = ix < 0 ? ix + p.g.nx : ix;
    }
    const int c = (ix >= 0 && ix < p.g.nx && iy >= 0 && iy < p.g.ny) ? iy * p.g.nx + ix : kRunOutside;
    if (c != r.cell) {
        double v = 0.0;
        if (c >= 0) v = vals[c];  // asked for here, looked at when this run ends (kEager: below)
        run_flush<kThr>(p, r);
        r.cell = c;
        r.acc = 0;
        r.start = r.clock;
        r.v = v;
        if constexpr (kEager) {
            if (c >= 0) classify<kThr>(p, r);
        }
    }
    r.acc += q;
    r.clock += q;
}

// row_value of row k at (x, gy = (lat - lat0) / dlat): the value of the cell the row lies in, NaN off the grid
__device__ __forceinline__ double row_cell_value(const RasterParams& p, const double* vals, double x, double gy) {
    const double fx = floor((x - p.lon0) / p.dlon), fy = floor(gy);
    const bool onx = p.g.periodic ? fx * 0.0 == 0.0 : (fx >= 0.0 && fx < (double)p.g.nx);
    if (!(onx && fy >= 0.0 && fy < (double)p.g.ny)) return NAN;
    int ix = (int)fx;
    if (p.g.periodic) {
        ix %= p.g.nx;
        ix = ix < 0 ? ix + p.g.nx : ix;
    }
    return vals[(int)fy * p.g.nx + ix];
}

// one track: vals is where the raster is read from (global memory, or the block's copy of it)
template <bool kThr, bool kRows>
__device__ __forceinline__ void raster_track(const RasterParams& p, size_t t, size_t sample, const double* vals) {
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = sample;
    const int ns = track_steps(p, t);
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    double* rv = kRows ? p.row_value + (s * rows) * ld + t : nullptr;  // row k: rv[k * ld]
    const double ref = p.lon_ref;
    Run r;
    int nbrk = 0;
    auto sink = [&](int ix, int iy, int64_t q) { run_add<kThr>(p, vals, r, ix, iy, q); };
    if (ns > 0 || kRows) {
        double lon = st[0], lat = st[ld];
        double ax = ref + wrap180(lon - ref);
        double gyA = (lat - p.lat0) / p.dlat;
        // row 1 and dt of step 0 on their way; rows past ns are never read
        double nlon = 0.0, nlat = 0.0, ndt = 0.0;
        if (ns > 0) {
            nlon = st[4 * ld];
            nlat = st[5 * ld];
            ndt = p.dt[t];
        }
        if constexpr (kRows) rv[0] = row_cell_value(p, vals, ax, gyA);
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
            if constexpr (kRows) rv[((size_t)k + 1) * ld] = row_cell_value(p, vals, x1, gyB);
            const bool sound = gridwalk::step_sound(delta, lat, lat1, d);
            int64_t dtq = 0;
            double gxA = 0.0, gxB = 0.0, fxA = 0.0, fyA = 0.0;
            bool walk = false;
            if (sound) {
                dtq = gridwalk::step_ticks(d);
                gxA = (ax - p.lon0) / p.dlon;
                gxB = ((ax + delta) - p.lon0) / p.dlon;
                fxA = floor(gxA);
                fyA = floor(gyA);
                // the fast path: no grid line crossed, and the cell is the run's own, by its indices before wrapping
                const bool stays = fxA == floor(gxB) && fyA == floor(gyB) && r.cell != kRunNone &&
                                   gridwalk::grid_start(fxA, p.g.nx, p.g.periodic) == r.ix &&
                                   gridwalk::grid_start(fyA, p.g.ny, false) == r.iy;
                if (stays) {
                    r.acc += dtq;
                    r.clock += dtq;
                }
                walk = !stays;  // a step that crosses no line but begins a run is walked too: one piece
            } else {
                ++nbrk;
            }
            if (__any(walk)) {
                if (walk) gridwalk::walk(p.g, sink, gxA, gyA, gxB, gyB, fxA, fyA, dtq);
            }
            lon = lon1;
            lat = lat1;
            ax = x1;
            gyA = gyB;
        }
        run_flush<kThr>(p, r);
        if constexpr (kThr) excursion_end(p, r);
    }
    const RasterOut& out = late_outputs();
    const size_t o = s * ld + t;
    if (out.total) out.total[o] = r.clock;  // every piece went through the sink, and a step's pieces sum to its dtq
    if (out.outside) out.outside[o] = r.outside;
    if (out.nbroken) out.nbroken[o] = nbrk;
    if (out.valid) out.valid[o] = r.valid;
    if (out.nodata) out.nodata[o] = r.nodata;
    if (out.wsum) out.wsum[o] = r.wsum;
    if (out.vmin) out.vmin[o] = r.vmin;
    if (out.vmax) out.vmax[o] = r.vmax;
    if (out.tmin) out.tmin[o] = r.tmin;
    if (out.tmax) out.tmax[o] = r.tmax;
    if constexpr (kThr) {
        if (out.hit_ticks) out.hit_ticks[o] = r.hit_ticks;
        if (out.hit_first) out.hit_first[o] = r.hit_first;
        if (out.nhit) out.nhit[o] = r.nhit;
        if (out.nhit_long) out.nhit_long[o] = r.nhit_long;
        if (out.hit_longest) out.hit_longest[o] = r.hit_longest;
    }
}

template <bool kThr, bool kRows, bool kLds>
__global__ __launch_bounds__(64) void raster_metrics(const RasterParams p, const RasterOut) {  // RasterOut: late_outputs()
    extern __shared__ double copy[];  // kLds: values[nx * ny]
    const double* vals = p.values;
    if constexpr (kLds) {
        const int ncell = p.g.nx * p.g.ny;
        for (int c = threadIdx.x; c < ncell; c += 64) copy[c] = p.values[c];
        __syncthreads();
        vals = copy;
    }
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t < (size_t)p.B) raster_track<kThr, kRows>(p, t, blockIdx.y, vals);
}

template <bool kThr, bool kRows>
int launch_raster(const RasterParams& p, const RasterOut& out, hipStream_t stream) {
    const dim3 grid((unsigned)((p.B + 63) / 64), (unsigned)p.nstates), block(64);
    if constexpr (kLdsCells > 0) {
        if (p.g.nx * p.g.ny <= kLdsCells) {
            hipLaunchKernelGGL((raster_metrics<kThr, kRows, true>), grid, block, (size_t)p.g.nx * p.g.ny * 8, stream, p, out);
            return abi_check_hip(hipGetLastError(), "raster_metrics launch");
        }
    }
    hipLaunchKernelGGL((raster_metrics<kThr, kRows, false>), grid, block, 0, stream, p, out);
    return abi_check_hip(hipGetLastError(), "raster_metrics launch");
}

}  // namespace
}  // namespace ste

extern "C" int ste_raster_metrics_f64(const ste_ukf_batch_f64* b, const ste_raster_f64* r, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_raster_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!r) return refuse("the raster arguments (r) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!r->states) return refuse("r->states is required");
    if (int rc = refuse.nstates("r->nstates", r->nstates, " (one grid row per track of a ship)")) return rc;
    if (r->flags & ~(STE_GRID_PERIODIC_LON | STE_RASTER_BELOW | STE_RASTER_NO_THRESHOLD))
        return refuse("r->flags has unknown bits");
    if (r->nx < 1 || r->ny < 1 || (int64_t)r->nx * (int64_t)r->ny > (int64_t)STE_GRID_MAX_CELLS)
        return refuse("r->nx and r->ny must be >= 1 and nx * ny <= STE_GRID_MAX_CELLS (2^26)");
    if (!std::isfinite(r->lon0) || !std::isfinite(r->lat0) || !std::isfinite(r->lon_ref))
        return refuse("r->lon0, r->lat0 and r->lon_ref must be finite");
    if (!std::isfinite(r->dlon) || !std::isfinite(r->dlat) || !(r->dlon >= 1e-6) || !(r->dlat >= 1e-6))
        return refuse("r->dlon and r->dlat must be finite and >= 1e-6 degrees");
    const bool periodic = (r->flags & STE_GRID_PERIODIC_LON) != 0;
    const double width = (double)r->nx * r->dlon;
    if (periodic) {
        if (width != 360.0) return refuse("STE_GRID_PERIODIC_LON needs nx * dlon == 360 exactly");
        if (!(fabs(r->lon0 - r->lon_ref) <= 360.0)) return refuse("a periodic grid's lon0 must lie within lon_ref +- 360");
    } else if (!(r->lon0 - r->lon_ref >= -90.0 && (r->lon0 + width) - r->lon_ref <= 90.0)) {
        return refuse("a grid without STE_GRID_PERIODIC_LON must lie within lon_ref +- 90 "
                      "(at most 180 degrees wide)");
    }
    if (!b->dt) return refuse("the batch's dt is required (every output is a sum of it)");
    if (!r->values) return refuse("r->values is required");
    const bool thr = (r->flags & STE_RASTER_NO_THRESHOLD) == 0;
    const bool hits = r->hit_ticks || r->hit_first || r->nhit || r->nhit_long || r->hit_longest;
    if (thr) {
        if (r->threshold != r->threshold) return refuse("r->threshold is NaN (STE_RASTER_NO_THRESHOLD says there is none)");
        if (r->min_ticks < 0) return refuse("r->min_ticks must be >= 0");
    } else if (hits) {
        return refuse("with STE_RASTER_NO_THRESHOLD the hit outputs (hit_ticks, hit_first, "
                      "nhit, nhit_long, hit_longest) must be NULL");
    }
    if (!r->total && !r->outside && !r->nbroken && !r->valid && !r->nodata && !r->wsum && !r->vmin && !r->vmax && !r->tmin &&
        !r->tmax && !hits && !r->row_value)
        return refuse("no output asked for (every output pointer is NULL)");
    RasterParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = r->nstates;
    p.g = {r->nx, r->ny, periodic};
    p.below = (r->flags & STE_RASTER_BELOW) != 0;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = r->states;
    p.values = r->values;
    p.lon0 = r->lon0;
    p.lat0 = r->lat0;
    p.dlon = r->dlon;
    p.dlat = r->dlat;
    p.lon_ref = r->lon_ref;
    p.threshold = thr ? r->threshold : 0.0;
    p.min_ticks = thr ? r->min_ticks : 0;
    p.row_value = r->row_value;
    const RasterOut out{r->total, r->outside,   r->valid,     r->nodata,      r->tmin,    r->tmax, r->hit_ticks, r->hit_first,
                        r->hit_longest, r->nbroken, r->nhit,   r->nhit_long, r->wsum,        r->vmin,    r->vmax};
    hipStream_t hs = static_cast<hipStream_t>(stream);
    // the threshold bookkeeping runs only when a hit output is asked for; row_value only when it is
    return with_bool(thr && hits, [&](auto th) {
        return with_bool(r->row_value != nullptr, [&](auto rw) {
            constexpr bool kT = decltype(th)::value, kR = decltype(rw)::value;
            return launch_raster<kT, kR>(p, out, hs);
        });
    });
}
