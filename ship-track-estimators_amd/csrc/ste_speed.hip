// ste_speed.hip — how fast tracks that stay on the device went (include/ste.h: ste_speed_metrics_f64): the speed made good of
// every step (the leg of path_metrics over the step's dt), its maximum and when, the hours per speed band, and the runs of steps
// at or below (or at or above) a speed threshold -- stops and sustained speed -- for S tracks per ship (the sampler's output,
// or sm_mean / fwd_mean as S = 1).  The header carries the definitions and tests/speed_cases.py restates them in NumPy.
//
// What the reference offers for this is a per-ship Python loop over utils.haversine_formula / geographiclib_distance
// (utils.py:9-113) on a downloaded history, S x [Nmax+1][4][B] doubles for posterior samples.
//
//   speed_metrics<model, bands, runs>   a lane per track, samples along blockIdx.y, one sequential pass over the track's rows:
//                               the mapping of path_metrics, and its leg, so dist has its bits.  The template arguments say
//                               which groups of outputs exist: a call for vmax alone carries no band and no run state.
//
// The band edges travel in the kernel arguments into a table of 64 doubles in LDS, padded with +inf, and every lane finds its
// band by a search with halving strides: log2 compares, each one LDS read at the lane's own index.  (Counting the edges one by
// one against scalar operands costs a compare, an add with carry and a share of a branch per edge and step whichever way the
// edge arrives -- timed at 32 bands: 2.6 times path_metrics from the kernel arguments, 2.1 with eight edges to a scalar load,
// 2.7 from the lanes of a register by v_readlane.)  The band sums are lane-private columns of LDS ([nbands][64] doubles behind
// the table, sized by the launch: no atomics, no cross-lane traffic, and every lane's column sits on its own pair of banks
// whatever its band).  The next row's two loads and the next dt are issued before the current leg's arithmetic.  Every output
// has one writer: plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

namespace ste {
namespace {

struct SpeedParams {
    int B, Nmax, nstates, nbands;
    unsigned flags;
    size_t ld;                // tracks per row (track_stride, or B)
    const int32_t* nsteps;    // [B] or nullptr
    const double* dt;         // [Nmax][ld]
    const double* states;     // [S][Nmax+1][4][ld]
    const double* threshold;  // [ld] or nullptr
    double threshold_all, min_run;
    double* speed;            // [S][Nmax][ld] or nullptr
    double* dist;             // [S][ld] each, or nullptr
    double* sound_time;
    double* vmax;
    double* vmax_time;
    double* band_time;        // [S][nbands][ld] or nullptr
    double* cond_time;
    double* run_time;
    double* first_run;
    double* longest;
    double* longest_start;
    int32_t* nruns;
    int32_t* nbroken;
    int32_t* track_status;    // [ld] or nullptr
    double edges[STE_SPEED_MAX_BANDS + 1];
};

template <int kModel, bool kBands, bool kRuns>
__global__ __launch_bounds__(64) void speed_metrics(const SpeedParams p) {
    extern __shared__ double edge[];  // kBands: [64] edges, then [nbands][64] band sums, a column per lane
    double* const band = edge + 64;
    const int lane = (int)threadIdx.x;
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    // the wave's table of edges: lane i writes edges[i], +inf past the last one, before any lane leaves
    int top = 1;  // the first stride of the search: the largest count it can return, 2 * top - 1, covers nbands + 1
    if constexpr (kBands) {
        edge[lane] = lane <= p.nbands ? p.edges[min(lane, STE_SPEED_MAX_BANDS)] : __builtin_inf();
        __syncthreads();
        while (2 * top - 1 < p.nbands + 1) top *= 2;
    }
    if (t >= (size_t)p.B) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = blockIdx.y;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const int nb = p.nbands;
    const int ns = track_steps(p, t);
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    const double* dtp = p.dt + t;
    double* sp = p.speed ? p.speed + (s * (size_t)p.Nmax) * ld + t : nullptr;

    if constexpr (kBands) {
        for (int j = 0; j < nb; ++j) band[j * 64 + lane] = 0.0;
    }
    bool tbad = false, lbad = false;  // a bad clock, a bad limit
    double thr = 0.0;
    if constexpr (kRuns) {
        thr = p.threshold ? p.threshold[t] : p.threshold_all;
        lbad = !(thr >= 0.0 && is_finite(thr));
    }
    const bool above = (p.flags & STE_SPEED_ABOVE) != 0;

    double dist = 0.0, sound_time = 0.0, vmax = -inf, vmax_time = nan, T = 0.0;
    int nbroken = 0;
    // run state: held by the run kernels only
    double cond = 0.0, run_time = 0.0, first = nan, longest = 0.0, lstart = nan, run = 0.0, start = 0.0;
    int nruns = 0;
    bool open = false;
    auto close_run = [&]() {
        if (run >= p.min_run) {
            if (nruns == 0) first = start;
            ++nruns;
            run_time = run_time + run;
        }
        if (run > longest) {
            longest = run;
            lstart = start;
        }
        open = false;
    };

    // row 0 here, row 1 and the dt of step 0 on their way; rows past ns are never read
    TrackPoint<kModel> cur = {0.0, 0.0, 0.0};
    double nlon = 0.0, nlat = 0.0, ndt = 0.0;
    if (ns > 0) {
        cur = track_point<kModel>(st[0], st[ld]);
        nlon = st[4 * ld];
        nlat = st[5 * ld];
        ndt = dtp[0];
    }
    for (int k = 0; k < ns; ++k) {
        const double lon = nlon, lat = nlat, dtk = ndt;
        if (k + 1 < ns) {  // what the next step needs, in flight during this leg's arithmetic
            const size_t r = (size_t)k + 2;
            nlon = st[(r * 4) * ld];
            nlat = st[(r * 4 + 1) * ld];
            ndt = dtp[(r - 1) * ld];
        }
        if (!(dtk >= 0.0 && is_finite(dtk))) tbad = true;
        const TrackPoint<kModel> nxt = track_point<kModel>(lon, lat);
        // the leg of every step, skipped ones included: they are rare, and the wave stays together
        const double L = track_leg_km<kModel>(cur, nxt);
        const bool examined = dtk > 0.0;
        const double q = L / dtk;
        const bool sound = examined && is_finite(q);
        const double v = sound ? q : nan;
        if (examined && !sound) ++nbroken;
        if (sound) {
            dist = dist + L;
            sound_time = sound_time + dtk;
            if (v > vmax) {
                vmax = v;
                vmax_time = T;
            }
            if constexpr (kBands) {
                int c = 0;  // the number of edges <= v: they ascend, so a search by halving strides counts them
                for (int step = top; step > 0; step >>= 1) c += edge[c + step - 1] <= v ? step : 0;
                const int j = c - 1;
                if (j >= 0 && j < nb) band[j * 64 + lane] = band[j * 64 + lane] + dtk;
            }
        }
        if (sp) sp[(size_t)k * ld] = v;
        if constexpr (kRuns) {
            const bool qual = sound && (above ? v >= thr : v <= thr);
            if (qual) {
                cond = cond + dtk;
                if (open) {
                    run = run + dtk;
                } else {
                    open = true;
                    run = dtk;
                    start = T;
                }
            } else if (open) {
                close_run();
            }
        }
        T = T + dtk;
        cur = nxt;
    }
    if constexpr (kRuns) {
        if (open) close_run();
    }

    const size_t o = s * ld + t;
    const bool bad = tbad || lbad;
    if (p.track_status && s == 0) p.track_status[t] = (tbad ? STE_SPEED_BAD_TIME : 0) | (lbad ? STE_SPEED_BAD_LIMIT : 0);
    if (bad && sp) {
        for (int k = 0; k < ns; ++k) sp[(size_t)k * ld] = nan;
    }
    if (p.dist) p.dist[o] = bad ? 0.0 : dist;
    if (p.sound_time) p.sound_time[o] = bad ? 0.0 : sound_time;
    if (p.vmax) p.vmax[o] = bad || vmax < 0.0 ? nan : vmax;
    if (p.vmax_time) p.vmax_time[o] = bad ? nan : vmax_time;
    if (p.nbroken) p.nbroken[o] = bad ? 0 : nbroken;
    if constexpr (kBands) {
        if (p.band_time) {
            for (int j = 0; j < nb; ++j) p.band_time[(s * (size_t)nb + (size_t)j) * ld + t] = bad ? 0.0 : band[j * 64 + lane];
        }
    }
    if constexpr (kRuns) {
        if (p.cond_time) p.cond_time[o] = bad ? 0.0 : cond;
        if (p.run_time) p.run_time[o] = bad ? 0.0 : run_time;
        if (p.first_run) p.first_run[o] = bad ? nan : first;
        if (p.longest) p.longest[o] = bad ? 0.0 : longest;
        if (p.longest_start) p.longest_start[o] = bad ? nan : lstart;
        if (p.nruns) p.nruns[o] = bad ? 0 : nruns;
    }
}

template <int kModel, bool kBands, bool kRuns>
void launch_speed(const SpeedParams& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.B + 63) / 64), (unsigned)p.nstates), block(64);
    const size_t lds = kBands ? ((size_t)p.nbands + 1) * 64 * sizeof(double) : 0;
    hipLaunchKernelGGL((speed_metrics<kModel, kBands, kRuns>), grid, block, lds, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_speed_metrics_f64(const ste_ukf_batch_f64* b, const ste_speed_f64* sp, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_speed_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!sp) return refuse("the speed arguments (sp) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!sp->states) return refuse("sp->states is required");
    if (int rc = refuse.nstates("sp->nstates", sp->nstates, " (one grid row per track of a ship)")) return rc;
    if (int rc = refuse.model("sp->model", sp->model)) return rc;
    if (sp->flags & ~STE_SPEED_ABOVE) return refuse("sp->flags must be 0 or STE_SPEED_ABOVE");
    if (sp->nbands < 0 || sp->nbands > STE_SPEED_MAX_BANDS)
        return refuse("sp->nbands must be between 0 and STE_SPEED_MAX_BANDS (32)");
    if (sp->nbands > 0 && !sp->band_edges)
        return refuse("sp->band_edges is required with nbands > 0 (nbands + 1 edges on the host)");
    if (sp->nbands == 0 && sp->band_edges) return refuse("sp->band_edges must be NULL with nbands == 0");
    if (sp->nbands == 0 && sp->band_time) return refuse("sp->band_time needs bands (nbands > 0)");
    for (int i = 0; i <= sp->nbands && sp->nbands > 0; ++i) {
        const double e = sp->band_edges[i];
        if (!(std::isfinite(e) && e >= 0.0 && (i == 0 || e > sp->band_edges[i - 1])))
            return refuse("sp->band_edges must be finite, >= 0 and strictly ascending");
    }
    if (!(std::isfinite(sp->min_run_h) && sp->min_run_h >= 0.0)) return refuse("sp->min_run_h must be finite and >= 0");
    const bool runs = sp->cond_time || sp->run_time || sp->first_run || sp->longest || sp->longest_start || sp->nruns;
    if (runs && !sp->threshold && !(std::isfinite(sp->threshold_all) && sp->threshold_all >= 0.0))
        return refuse("a run output (cond_time, run_time, first_run, longest, longest_start, nruns) needs sp->threshold, or a threshold_all that is finite and >= 0");
    if (!b->dt) return refuse("the batch's dt is required (a speed is a leg over its dt)");
    if (!runs && !sp->speed && !sp->dist && !sp->sound_time && !sp->vmax && !sp->vmax_time && !sp->band_time && !sp->nbroken &&
        !sp->track_status)
        return refuse("no output asked for (speed, dist, sound_time, vmax, vmax_time, band_time, cond_time, run_time, first_run, longest, longest_start, nruns, nbroken and track_status are all NULL)");
    SpeedParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = sp->nstates;
    p.nbands = sp->nbands;
    p.flags = sp->flags;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = sp->states;
    p.threshold = sp->threshold;
    p.threshold_all = sp->threshold_all;
    p.min_run = sp->min_run_h;
    p.speed = sp->speed;
    p.dist = sp->dist;
    p.sound_time = sp->sound_time;
    p.vmax = sp->vmax;
    p.vmax_time = sp->vmax_time;
    p.band_time = sp->band_time;
    p.cond_time = sp->cond_time;
    p.run_time = sp->run_time;
    p.first_run = sp->first_run;
    p.longest = sp->longest;
    p.longest_start = sp->longest_start;
    p.nruns = sp->nruns;
    p.nbroken = sp->nbroken;
    p.track_status = sp->track_status;
    for (int i = 0; i <= STE_SPEED_MAX_BANDS; ++i) p.edges[i] = sp->nbands > 0 && i <= sp->nbands ? sp->band_edges[i] : 0.0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool sphere = sp->model == STE_PREP_SPHERE;
    with_bool(sp->band_time != nullptr, [&](auto bd) {
        with_bool(runs, [&](auto rn) {
            constexpr bool kB = decltype(bd)::value, kR = decltype(rn)::value;
            if (sphere) launch_speed<STE_PREP_SPHERE, kB, kR>(p, s);
            else launch_speed<STE_PREP_WGS84, kB, kR>(p, s);
        });
    });
    return abi_check_hip(hipGetLastError(), "speed_metrics launch");
}
