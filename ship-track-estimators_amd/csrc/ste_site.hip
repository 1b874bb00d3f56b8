// ste_site.hip — tracks that stay on the device against FIXED SITES (include/ste.h: ste_site_metrics_f64): how close every ship
// came to every one of M points (ports, anchorages, buoys), when, how long it stayed within the site's radius, from when, how
// often and for how long at a stretch, for S tracks per ship (the sampler's output, or sm_mean / fwd_mean as S = 1).  A site is
// a ship that does not move and has no clock, so a ship's own steps are the pieces and nothing is merged: the header carries
// the definitions (the encounters' rules specialised) and tests/site_cases.py restates them in NumPy.
//
//   site_metrics<model, within>   a lane per track, so the rows of [4][track_stride] are read coalesced; a wave holds its 64
//                               ships against a TILE of kSiteTile sites whose running state lives in registers.  A step is
//                               loaded once, its delta, soundness and length are worked out once, and then it costs one
//                               quadratic (one cos, one sqrt, three divisions) per site of the tile.  The site tile is the
//                               fastest grid dimension: the waves that are resident together read the same rows.
//
// The sites' X, Y and R * R are the same for every lane: they are read once, before the step loop and before any store, by
// loads whose address is uniform over the wave, and stay in scalar registers.  The rows and the dt of the next step are
// requested before the current step's arithmetic.  The leg function (haversine or the WGS84 inverse) runs once per (sample,
// site, track) after the loop, in a rolled loop over the tile fed from LDS, so its code is there once.  Every output has one
// writer: plain vector loads and stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

#ifndef STE_SITE_TILE
#define STE_SITE_TILE 4  // sites per wave: 4, 6 and 8 were timed ("Sites")
#endif
#ifndef STE_SITE_WAVES
#define STE_SITE_WAVES 2  // waves per SIMD: 2 and 3 were timed
#endif

namespace ste {
namespace {

constexpr int kSiteTile = STE_SITE_TILE;
constexpr double kKd = kEarthKm * kDeg2Rad;   // km per degree of a great circle, one double

struct SiteParams {
    int B, Nmax, nstates, nsites;
    unsigned ntiles;        // site tiles: ceil(M / kSiteTile)
    size_t ld;              // tracks per row (track_stride, or B)
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld]
    const double* states;   // [S][Nmax+1][4][ld]
    const double* sites;    // [2][M]
    const double* radius;   // [M]
    const double* t0;       // [ld] or nullptr
    double* min_dist;       // [S][M][ld] each, or nullptr
    double* min_time;
    double* time_within;
    double* first_within;
    double* longest;
    int32_t* nwithin;
    double* sound_time;     // [S][ld] or nullptr
    int32_t* nbroken;
    int32_t* track_status;  // [ld] or nullptr
    int32_t* site_status;   // [M] or nullptr
};

__device__ __forceinline__ bool site_is_bad(double X, double Y, double R) {
    return !(is_finite(X) && is_finite(Y) && R >= 0.0 && R <= STE_ENCOUNTER_MAX_RADIUS_KM);
}

template <int kModel, bool kWithin>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(STE_SITE_WAVES, STE_SITE_WAVES))) void site_metrics(const SiteParams p) {
    __shared__ double spx[kModel != kNoLeg ? kSiteTile : 1][64], spy[kModel != kNoLeg ? kSiteTile : 1][64];
    const unsigned stile = blockIdx.x % p.ntiles, ttile = blockIdx.x / p.ntiles;
    const int lane = (int)threadIdx.x;
    const int M = p.nsites, m0 = (int)stile * kSiteTile;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = blockIdx.y;
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    // the tile's sites: uniform over the wave.  A tile that reaches past M repeats the last site and stores nothing for it.
    double X[kSiteTile], Y[kSiteTile], YY[kSiteTile], R2[kSiteTile];
    bool sbad[kSiteTile];
#pragma unroll
    for (int j = 0; j < kSiteTile; ++j) {
        const int m = min(m0 + j, M - 1);
        const double R = p.radius[m];
        X[j] = p.sites[m];
        Y[j] = p.sites[(size_t)M + m];
        YY[j] = Y[j] + Y[j];
        R2[j] = R * R;
        sbad[j] = site_is_bad(X[j], Y[j], R);
    }
    if (p.site_status && ttile == 0 && s == 0 && lane < kSiteTile && m0 + lane < M) {
        const int m = m0 + lane;
        p.site_status[m] = site_is_bad(p.sites[m], p.sites[(size_t)M + m], p.radius[m]) ? STE_SITE_BAD_SITE : 0;
    }
    const size_t t = (size_t)ttile * 64 + lane;
    if (t >= (size_t)p.B) return;

    double best_q[kSiteTile], mt[kSiteTile], px[kSiteTile], py[kSiteTile];
    double within[kSiteTile], first[kSiteTile], run[kSiteTile], longest[kSiteTile];
    int nwithin[kSiteTile];
    bool open[kSiteTile];
#pragma unroll
    for (int j = 0; j < kSiteTile; ++j) {
        best_q[j] = inf;
        mt[j] = px[j] = py[j] = first[j] = nan;
        within[j] = run[j] = longest[j] = 0.0;
        nwithin[j] = 0;
        open[j] = false;
    }
    double sound_time = 0.0;
    int nbroken = 0;

    const double t0 = p.t0 ? p.t0[t] : 0.0;
    bool tbad = !is_finite(t0);
    // track_steps(p, t), written out: through the function the kernel's address arithmetic comes out in another order
    const int ns = tbad ? 0 : min(max(p.nsteps ? p.nsteps[t] : p.Nmax, 0), p.Nmax);
    const double* st = p.states + (s * rows * 4) * ld + t;  // row k, component c: st[(k * 4 + c) * ld]
    const double* dtp = p.dt + t;
    double lon = 0.0, lat = 0.0, lon1 = 0.0, lat1 = 0.0, dtk = 0.0, T = 0.0;
    if (ns > 0) {  // rows past nsteps are never read
        dtk = dtp[0];
        lon = st[0];
        lat = st[ld];
        lon1 = st[4 * ld];
        lat1 = st[5 * ld];
    }
    for (int k = 0; k < ns; ++k) {
        // what the next step needs, in flight during this step's arithmetic
        double ndt = 0.0, plon = 0.0, plat = 0.0;
        if (k + 1 < ns) {
            const size_t r = (size_t)k + 2;
            ndt = dtp[(r - 1) * ld];
            plon = st[(r * 4) * ld];
            plat = st[(r * 4 + 1) * ld];
        }
        if (!(dtk >= 0.0 && is_finite(dtk))) tbad = true;
        const double lo = t0 + T, T1 = T + dtk, hi = t0 + T1;
        const double len = hi - lo;
        const double delta = wrap180(lon1 - lon);
        const bool examined = hi > lo;
        const bool sound = examined && fabs(delta) < 90.0 && is_finite(lat) && is_finite(lat1);
        if (examined && !sound) ++nbroken;
        if (sound) {
            sound_time = sound_time + len;
            const double x0 = lon, y0 = lat, x1 = x0 + delta, y1 = lat1;
            const double sx = x1 - x0, sy = y1 - y0, ysum = y0 + y1;
#pragma unroll
            for (int j = 0; j < kSiteTile; ++j) {
                const double gx0 = wrap180(X[j] - x0), gy0 = Y[j] - y0;
                const double gx1 = gx0 - sx, gy1 = Y[j] - y1;
                const double kc = kKd * cos(0.25 * (ysum + YY[j]) * kDeg2Rad);
                const double r0x = kc * gx0, r0y = kKd * gy0, r1x = kc * gx1, r1y = kKd * gy1;
                const double dx = r1x - r0x, dy = r1y - r0y;
                const double dd = dx * dx + dy * dy, bq = r0x * dx + r0y * dy, r00 = r0x * r0x + r0y * r0y;
                const double us = dd > 0.0 ? clamp01(-bq / dd) : 0.0;
                const double mx = r0x + us * dx, my = r0y + us * dy;
                const double q = mx * mx + my * my;
                if (q < best_q[j]) {
                    best_q[j] = q;
                    mt[j] = lo + us * len;
                    px[j] = x0 + us * sx;
                    py[j] = y0 + us * sy;
                }
                if constexpr (kWithin) {
                    double ua = 0.0, ub = 0.0;  // no interval
                    if (dd > 0.0) {
                        const double disc = bq * bq - dd * (r00 - R2[j]);
                        if (disc >= 0.0) {
                            const double sq = sqrt(disc);
                            const double va = (-bq - sq) / dd, vb = (-bq + sq) / dd;
                            ua = va > 0.0 ? va : 0.0;
                            ub = vb < 1.0 ? vb : 1.0;
                        }
                    } else if (dd == 0.0 && r00 <= R2[j]) {
                        ub = 1.0;
                    }
                    if (ub > ua) {
                        const double w = (ub - ua) * len;
                        within[j] = within[j] + w;
                        if (!(open[j] && ua == 0.0)) {
                            if (nwithin[j] == 0) first[j] = lo + ua * len;
                            ++nwithin[j];
                            run[j] = w;
                        } else {
                            run[j] = run[j] + w;
                        }
                        // a run only grows, so the largest value it has had is its length when it closes
                        longest[j] = run[j] > longest[j] ? run[j] : longest[j];
                        open[j] = ub == 1.0;
                    } else {
                        open[j] = false;
                    }
                }
            }
        } else if constexpr (kWithin) {  // broken, or of zero length: every run is closed
#pragma unroll
            for (int j = 0; j < kSiteTile; ++j) open[j] = false;
        }
        T = T1;
        dtk = ndt;
        lon = lon1;
        lat = lat1;
        lon1 = plon;
        lat1 = plat;
    }

    if (stile == 0) {
        if (p.track_status && s == 0) p.track_status[t] = tbad ? STE_SITE_BAD_TIME : 0;
        if (p.sound_time) p.sound_time[s * ld + t] = tbad ? 0.0 : sound_time;
        if (p.nbroken) p.nbroken[s * ld + t] = tbad ? 0 : nbroken;
    }
#pragma unroll
    for (int j = 0; j < kSiteTile; ++j) {
        if (m0 + j < M) {  // uniform
            const size_t o = (s * (size_t)M + (size_t)(m0 + j)) * ld + t;
            const bool bad = tbad || sbad[j];
            const bool found = !bad && best_q[j] < inf;
            if constexpr (kModel != kNoLeg) {
                spx[j][lane] = found ? px[j] : nan;
                spy[j][lane] = py[j];
            }
            if (p.min_time) p.min_time[o] = found ? mt[j] : nan;
            if constexpr (kWithin) {
                if (p.time_within) p.time_within[o] = bad ? 0.0 : within[j];
                if (p.first_within) p.first_within[o] = bad ? nan : first[j];
                if (p.longest) p.longest[o] = bad ? 0.0 : longest[j];
                if (p.nwithin) p.nwithin[o] = bad ? 0 : nwithin[j];
            }
        }
    }
    if constexpr (kModel != kNoLeg) {
        // every lane reads back what it wrote itself: no barrier.  One copy of the leg function for the whole tile.
#pragma unroll 1
        for (int j = 0; j < kSiteTile && m0 + j < M; ++j) {
            const int m = m0 + j;
            const double x = spx[j][lane], y = spy[j][lane];
            double d = nan;
            if (x == x) d = leg_km_deg<kModel>(x, y, p.sites[m], p.sites[(size_t)M + m]);
            p.min_dist[(s * (size_t)M + (size_t)m) * ld + t] = d;
        }
    }
}

template <int kModel, bool kWithin>
void launch_site(const SiteParams& p, unsigned nblocks, hipStream_t s) {
    const dim3 grid(nblocks, (unsigned)p.nstates), block(64);
    hipLaunchKernelGGL((site_metrics<kModel, kWithin>), grid, block, 0, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_site_tile(void) { return ste::kSiteTile; }

extern "C" int ste_site_metrics_f64(const ste_ukf_batch_f64* b, const ste_site_f64* si, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_site_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!si) return refuse("the site arguments (si) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!si->states) return refuse("si->states is required");
    if (!si->sites) return refuse("si->sites is required");
    if (!si->radius_km) return refuse("si->radius_km is required (one radius per site)");
    if (int rc = refuse.nstates("si->nstates", si->nstates, " (one grid row per track of a ship)")) return rc;
    if (si->nsites < 1 || si->nsites > STE_SITES_MAX) return refuse("si->nsites must be between 1 and STE_SITES_MAX (65536)");
    if (si->min_dist && refuse.model("si->model", si->model, " when min_dist is asked for")) return STE_EINVAL;
    if (si->flags != 0) return refuse("si->flags must be 0");
    if (si->reserved != 0) return refuse("si->reserved must be 0");
    if (!b->dt) return refuse("the batch's dt is required (the clock is made of its sums)");
    if (!si->min_dist && !si->min_time && !si->time_within && !si->first_within && !si->longest && !si->nwithin &&
        !si->sound_time && !si->nbroken && !si->track_status && !si->site_status)
        return refuse("no output asked for (min_dist, min_time, time_within, first_within, longest, nwithin, sound_time, nbroken, track_status and site_status are all NULL)");
    SiteParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = si->nstates;
    p.nsites = si->nsites;
    p.ntiles = (unsigned)((si->nsites + kSiteTile - 1) / kSiteTile);
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = si->states;
    p.sites = si->sites;
    p.radius = si->radius_km;
    p.t0 = si->t0;
    p.min_dist = si->min_dist;
    p.min_time = si->min_time;
    p.time_within = si->time_within;
    p.first_within = si->first_within;
    p.longest = si->longest;
    p.nwithin = si->nwithin;
    p.sound_time = si->sound_time;
    p.nbroken = si->nbroken;
    p.track_status = si->track_status;
    p.site_status = si->site_status;
    const uint64_t nblocks = (uint64_t)p.ntiles * (uint64_t)(((int64_t)b->B + 63) / 64);
    if (nblocks > 0x7fffffffull)
        return refuse("ceil(B / 64) * ceil(nsites / tile) exceeds 2^31 - 1 blocks: split the sites or the tracks over calls");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool within = si->time_within || si->first_within || si->longest || si->nwithin;
    const int model = si->min_dist ? si->model : kNoLeg;
    with_bool(within, [&](auto w) {
        constexpr bool kW = decltype(w)::value;
        if (model == STE_PREP_SPHERE) launch_site<STE_PREP_SPHERE, kW>(p, (unsigned)nblocks, s);
        else if (model == STE_PREP_WGS84) launch_site<STE_PREP_WGS84, kW>(p, (unsigned)nblocks, s);
        else launch_site<kNoLeg, kW>(p, (unsigned)nblocks, s);
    });
    return abi_check_hip(hipGetLastError(), "site_metrics launch");
}
