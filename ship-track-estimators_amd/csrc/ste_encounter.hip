// ste_encounter.hip — pairs of tracks that stay on the device against each other (include/ste.h: ste_encounter_metrics_f64):
// the closest approach of two ships and its time, the time they spend within R km of each other, when that first happens and
// how often, for S tracks per ship (the sampler's output, or sm_mean / fwd_mean as S = 1).  Every ship has its own dt, so a
// pair is walked on a common clock: the two time bases are merged into PIECES on which both positions are linear in time, and
// a piece costs a quadratic in planar (lon, lat).  The header carries the definitions and tests/encounter_cases.py restates
// them in NumPy.
//
//   encounter_metrics<model, within>   a lane per pair, samples along blockIdx.y (the mapping of path_metrics), one in-order walk
//                               over the pieces of the pair.  The walk itself (the merge and the four divisions that place a
//                               piece in the two steps) does not depend on the sample; a lane that walks once for a tile of 2
//                               or 4 samples was built and timed, and was slower for its registers ("Encounters").
//
// The reads are gathers: 16 B per (sample, ship, row) at addresses that the pair list decides, so lanes of a wave touch rows of
// unrelated tracks.  A piece's loop holds one cos and one sqrt and no other transcendental; the leg function (haversine or the
// WGS84 inverse) runs once per (sample, pair) after the walk.  The rows and the dt that the next piece needs are requested before
// the current piece's arithmetic.  Every output has one writer: plain loads and stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

namespace ste {
namespace {

constexpr double kKd = kEarthKm * kDeg2Rad;   // km per degree of a great circle, one double

struct EncParams {
    int B, Nmax, nstates;
    size_t ld;              // tracks per row (track_stride, or B)
    size_t npairs;
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld]
    const double* states;   // [S][Nmax+1][4][ld]
    const int32_t* pairs;   // [P][2]
    const double* t0;       // [ld] or nullptr
    double R2;              // radius_km * radius_km
    double* min_dist;       // [S][P] each, or nullptr
    double* min_time;
    double* time_within;
    double* first_within;
    int32_t* nwithin;
    double* overlap;
    int32_t* nbroken;
    int32_t* status;        // [P] or nullptr
};


// one ship's current step in one sample: rows k and k + 1, and row k + 2 on its way
struct EncStep {
    double lon, lat;      // row k
    double lon1, lat1;    // row k + 1
    double delta, dlat;   // wrap180(lon1 - lon), lat1 - lat
    double plon, plat;    // row k + 2, loaded while the piece before it is worked on
    bool sound;
};

__device__ __forceinline__ void step_set(EncStep& s) {
    s.delta = wrap180(s.lon1 - s.lon);
    s.dlat = s.lat1 - s.lat;
    s.sound = fabs(s.delta) < 90.0 && s.lat * 0.0 == 0.0 && s.lat1 * 0.0 == 0.0;
}

__device__ __forceinline__ void step_advance(EncStep& s) {
    s.lon = s.lon1;
    s.lat = s.lat1;
    s.lon1 = s.plon;
    s.lat1 = s.plat;
    step_set(s);
}

// what one (sample, pair) accumulates over its pieces
struct EncAcc {
    double best_q, min_time, xi, yi, xj, yj;
    double within, first, overlap;
    int nwithin, nbroken;
    bool open;
};

template <bool kWithin>
__device__ __forceinline__ void piece(const EncStep& A, const EncStep& Bs, EncAcc& c, double lo, double hi, double u0a,
                                      double u1a, double u0b, double u1b, double R2) {
    if (!(A.sound && Bs.sound)) {
        ++c.nbroken;
        c.open = false;
        return;
    }
    const double len = hi - lo;
    c.overlap = c.overlap + len;
    const double xi0 = A.lon + u0a * A.delta, xi1 = A.lon + u1a * A.delta;
    const double yi0 = A.lat + u0a * A.dlat, yi1 = A.lat + u1a * A.dlat;
    const double xj0 = Bs.lon + u0b * Bs.delta, xj1 = Bs.lon + u1b * Bs.delta;
    const double yj0 = Bs.lat + u0b * Bs.dlat, yj1 = Bs.lat + u1b * Bs.dlat;
    const double gx0 = wrap180(xj0 - xi0), gy0 = yj0 - yi0;
    const double gx1 = gx0 + ((xj1 - xj0) - (xi1 - xi0)), gy1 = yj1 - yi1;
    const double kc = kKd * cos(0.25 * ((yi0 + yi1) + (yj0 + yj1)) * kDeg2Rad);
    const double r0x = kc * gx0, r0y = kKd * gy0, r1x = kc * gx1, r1y = kKd * gy1;
    const double dx = r1x - r0x, dy = r1y - r0y;
    const double dd = dx * dx + dy * dy, bq = r0x * dx + r0y * dy, r00 = r0x * r0x + r0y * r0y;
    const double us = dd > 0.0 ? clamp01(-bq / dd) : 0.0;
    const double mx = r0x + us * dx, my = r0y + us * dy;
    const double q = mx * mx + my * my;
    if (q < c.best_q) {
        c.best_q = q;
        c.min_time = lo + us * len;
        c.xi = xi0 + us * (xi1 - xi0);
        c.yi = yi0 + us * (yi1 - yi0);
        c.xj = xj0 + us * (xj1 - xj0);
        c.yj = yj0 + us * (yj1 - yj0);
    }
    if constexpr (kWithin) {
        double ua = 0.0, ub = 0.0;  // no interval
        if (dd > 0.0) {
            const double disc = bq * bq - dd * (r00 - R2);
            if (disc >= 0.0) {
                const double sq = sqrt(disc);
                const double va = (-bq - sq) / dd, vb = (-bq + sq) / dd;
                ua = va > 0.0 ? va : 0.0;
                ub = vb < 1.0 ? vb : 1.0;
            }
        } else if (dd == 0.0 && r00 <= R2) {
            ub = 1.0;
        }
        if (ub > ua) {
            c.within = c.within + (ub - ua) * len;
            if (!(c.open && ua == 0.0)) {
                if (c.nwithin == 0) c.first = lo + ua * len;
                ++c.nwithin;
            }
            c.open = ub == 1.0;
        } else {
            c.open = false;
        }
    }
}

// Two waves per SIMD, not the three the registers would allow: with three, the walk of 16 samples (states beyond the Infinity
// Cache) took 107 - 110 ms against 84 on the timing fleet and a shuffled list 257 against 241, for 6.4 against 6.6 ms at S = 1
// ("Encounters"): the gathers of a third wave evict lines the other two come back for.
template <int kModel, bool kWithin>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void encounter_metrics(const EncParams p) {
    const size_t pr = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (pr >= p.npairs) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1, s = blockIdx.y;
    const int i = p.pairs[2 * pr], j = p.pairs[2 * pr + 1];
    const double nan = __builtin_nan("");

    EncAcc c;
    c.best_q = __builtin_inf();
    c.min_time = nan;
    c.xi = c.yi = c.xj = c.yj = nan;
    c.within = c.overlap = 0.0;
    c.first = nan;
    c.nwithin = c.nbroken = 0;
    c.open = false;

    int status = 0;
    double t0i = 0.0, t0j = 0.0;
    if (i < 0 || i >= p.B || j < 0 || j >= p.B) {
        status = STE_ENC_BAD_INDEX;  // nothing of the pair is read
    } else if (p.t0) {
        t0i = p.t0[i];
        t0j = p.t0[j];
        if (!(t0i * 0.0 == 0.0 && t0j * 0.0 == 0.0)) status = STE_ENC_BAD_TIME;
    }
    if (status == 0) {
        // track_steps(p, i), written out: through the function the kernel's address arithmetic comes out in another order
        const int nsi = min(max(p.nsteps ? p.nsteps[i] : p.Nmax, 0), p.Nmax);
        const int nsj = min(max(p.nsteps ? p.nsteps[j] : p.Nmax, 0), p.Nmax);
        const double* sti = p.states + (s * rows * 4) * ld + (size_t)i;  // row k, component c: sti[(k * 4 + c) * ld]
        const double* stj = p.states + (s * rows * 4) * ld + (size_t)j;
        const double* dti = p.dt + (size_t)i;
        const double* dtj = p.dt + (size_t)j;
        EncStep A, Bs;
        int a = 0, b = 0;
        double Ta = 0.0, Tb = 0.0, dta = 0.0, dtb = 0.0;
        if (nsi > 0 && nsj > 0) {  // rows past nsteps are never read: the walk of an empty track reads nothing
            dta = dti[0];
            dtb = dtj[0];
            A.lon = sti[0];
            A.lat = sti[ld];
            A.lon1 = sti[4 * ld];
            A.lat1 = sti[5 * ld];
            Bs.lon = stj[0];
            Bs.lat = stj[ld];
            Bs.lon1 = stj[4 * ld];
            Bs.lat1 = stj[5 * ld];
            A.plon = A.plat = Bs.plon = Bs.plat = 0.0;
            step_set(A);
            step_set(Bs);
        }
        while (a < nsi && b < nsj) {
            if (!(dta >= 0.0 && dta * 0.0 == 0.0 && dtb >= 0.0 && dtb * 0.0 == 0.0)) {
                status = STE_ENC_BAD_TIME;
                break;
            }
            const double ta = t0i + Ta, Ta1 = Ta + dta, ea = t0i + Ta1;
            const double tb = t0j + Tb, Tb1 = Tb + dtb, eb = t0j + Tb1;
            const double lo = ta > tb ? ta : tb, hi = ea < eb ? ea : eb;
            const bool adva = ea <= eb, advb = eb <= ea;
            // what the next piece needs, in flight during this piece's arithmetic
            const bool la = adva && a + 1 < nsi, lb = advb && b + 1 < nsj;
            double ndta = 0.0, ndtb = 0.0;
            if (la) {
                const size_t k = (size_t)a + 2;
                ndta = dti[(k - 1) * ld];
                A.plon = sti[(k * 4) * ld];
                A.plat = sti[(k * 4 + 1) * ld];
            }
            if (lb) {
                const size_t k = (size_t)b + 2;
                ndtb = dtj[(k - 1) * ld];
                Bs.plon = stj[(k * 4) * ld];
                Bs.plat = stj[(k * 4 + 1) * ld];
            }
            if (hi > lo) {
                const double u0a = clamp01((lo - ta) / dta), u1a = clamp01((hi - ta) / dta);
                const double u0b = clamp01((lo - tb) / dtb), u1b = clamp01((hi - tb) / dtb);
                piece<kWithin>(A, Bs, c, lo, hi, u0a, u1a, u0b, u1b, p.R2);
            }
            if (adva) {
                ++a;
                Ta = Ta1;
                dta = ndta;
                if (la) step_advance(A);
            }
            if (advb) {
                ++b;
                Tb = Tb1;
                dtb = ndtb;
                if (lb) step_advance(Bs);
            }
        }
    }
    if (p.status && s == 0) p.status[pr] = status;
    const size_t o = s * p.npairs + pr;
    const bool bad = status != 0;
    const bool found = !bad && c.best_q < __builtin_inf();
    if constexpr (kModel != kNoLeg) {
        p.min_dist[o] = found ? leg_km_deg<kModel>(c.xi, c.yi, c.xj, c.yj) : nan;
    }
    if (p.min_time) p.min_time[o] = found ? c.min_time : nan;
    if constexpr (kWithin) {
        if (p.time_within) p.time_within[o] = bad ? 0.0 : c.within;
        if (p.first_within) p.first_within[o] = bad ? nan : c.first;
        if (p.nwithin) p.nwithin[o] = bad ? 0 : c.nwithin;
    }
    if (p.overlap) p.overlap[o] = bad ? 0.0 : c.overlap;
    if (p.nbroken) p.nbroken[o] = bad ? 0 : c.nbroken;
}

template <int kModel, bool kWithin>
void launch_encounter(const EncParams& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.npairs + 63) / 64), (unsigned)p.nstates), block(64);
    hipLaunchKernelGGL((encounter_metrics<kModel, kWithin>), grid, block, 0, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_encounter_metrics_f64(const ste_ukf_batch_f64* b, const ste_encounter_f64* en, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_encounter_metrics_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!en) return refuse("the encounter arguments (en) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!en->states) return refuse("en->states is required");
    if (!en->pairs) return refuse("en->pairs is required");
    if (int rc = refuse.nstates("en->nstates", en->nstates, " (one grid row per track of a ship)")) return rc;
    if (en->npairs < 1 || en->npairs > STE_ENCOUNTER_MAX_PAIRS)
        return refuse("en->npairs must be between 1 and STE_ENCOUNTER_MAX_PAIRS (2^26)");
    if (en->min_dist && refuse.model("en->model", en->model, " when min_dist is asked for")) return STE_EINVAL;
    if (!(std::isfinite(en->radius_km) && en->radius_km >= 0.0 && en->radius_km <= STE_ENCOUNTER_MAX_RADIUS_KM))
        return refuse("en->radius_km must be finite and between 0 and STE_ENCOUNTER_MAX_RADIUS_KM (1000)");
    if (en->flags != 0) return refuse("en->flags must be 0");
    if (en->reserved != 0) return refuse("en->reserved must be 0");
    if (!b->dt) return refuse("the batch's dt is required (the common clock is made of its sums)");
    if (!en->min_dist && !en->min_time && !en->time_within && !en->first_within && !en->nwithin && !en->overlap &&
        !en->nbroken && !en->status)
        return refuse("no output asked for (min_dist, min_time, time_within, first_within, nwithin, overlap, nbroken and status are all NULL)");
    EncParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = en->nstates;
    p.ld = track_ld(b);
    p.npairs = (size_t)en->npairs;
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = en->states;
    p.pairs = en->pairs;
    p.t0 = en->t0;
    p.R2 = en->radius_km * en->radius_km;
    p.min_dist = en->min_dist;
    p.min_time = en->min_time;
    p.time_within = en->time_within;
    p.first_within = en->first_within;
    p.nwithin = en->nwithin;
    p.overlap = en->overlap;
    p.nbroken = en->nbroken;
    p.status = en->status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool within = en->time_within || en->first_within || en->nwithin;
    const int model = en->min_dist ? en->model : kNoLeg;
    with_bool(within, [&](auto w) {
        constexpr bool kW = decltype(w)::value;
        if (model == STE_PREP_SPHERE) launch_encounter<STE_PREP_SPHERE, kW>(p, s);
        else if (model == STE_PREP_WGS84) launch_encounter<STE_PREP_WGS84, kW>(p, s);
        else launch_encounter<kNoLeg, kW>(p, s);
    });
    return abi_check_hip(hipGetLastError(), "encounter_metrics launch");
}
