// ste_error.hip — how far tracks that stay on the device are from where the ship really was (include/ste.h:
// ste_track_errors_f64): the distance of every row from a truth position of that row, its sums (cum_abs_diff and rmse of the
// reference's performance_metrics.py, in km instead of degrees), its split along and across the true course, and its score
// against the track's own covariance (NEES and coverage), for S tracks per ship (the sampler's output, or sm_mean / fwd_mean as
// S = 1).  The header carries the definitions and tests/error_cases.py restates them in NumPy.
//
// What the reference offers for this is performance_metrics.py on downloaded arrays, one ship at a time; for posterior samples
// that download is S x [Nmax+1][4][B] doubles, while the values wanted are a handful of numbers per (sample, ship).
//
//   track_errors<model, head, cov, tile>   a lane per track, samples along blockIdx.y (`tile` of them per lane, see below), one
//                               sequential pass over the track's rows: the mapping of path_metrics.  The template arguments say
//                               which groups of outputs exist: a call for distances only carries no heading arithmetic and no
//                               covariance loads.  The sums are sequential, so a value's bits depend on that track's rows alone.
//
// A row costs two state loads per sample, two truth loads (one more for the course, three more for the covariance) and one leg
// from the truth to the state.  The next row's loads are issued before the current row's arithmetic.  A wave skips the leg of a
// row in which none of its lanes has truth: truth is sparse where it is made of withheld reports.
// STE_ERROR_TILE samples share one lane: the truth row is read and converted (sphere: radians and cos(lat)) once for them, and
// their accumulators sit in registers; 1 is the plain mapping.  Every output has one writer: plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // last: it switches contraction off for the rest of the file

#ifndef STE_ERROR_TILE
#define STE_ERROR_TILE 1  // samples per lane; DESIGN.md, "Errors", has the timing of 1 against 4
#endif

namespace ste {
namespace {

struct ErrorParams {
    int B, Nmax, nstates, cov_rows;
    size_t ld;               // tracks per row (track_stride, or B)
    const int32_t* nsteps;   // [B] or nullptr
    const double* states;    // [S][Nmax+1][4][ld]
    const double* truth;     // [Nmax+1][2][ld]
    const double* course;    // [Nmax+1][ld] or nullptr
    const double* cov;       // [Nmax+1][cov_rows][ld] or nullptr
    // the order below is deliberate: with the per-row pointers behind the per-track ones, or nees_limit before them, the
    // covariance-only instantiations reserve a 36-byte stack frame for a group of scalar registers ("Errors")
    double *err, *cumerr, *along, *cross, *nees;                                                        // [S][Nmax+1][ld] or nullptr
    double *sum_err, *sum_sq, *max_err, *sum_along, *sum_along_sq, *sum_cross, *sum_cross_sq, *sum_nees;  // [S][ld] or nullptr
    int32_t *n, *max_row, *nbroken, *ncoursed, *nscored, *ninside;                                      // [S][ld] or nullptr
    double nees_limit;
};

// The leg from a (the truth) to b (the state): distance and, with kHead, initial heading.  Sphere: sphere_dist_km, and
// operation for operation the head_deg of sphere_leg on the radians and cosines at hand.  WGS84: wgs84_leg, whose heading
// arithmetic the compiler drops where the heading is not used.
template <int kModel, bool kHead>
__device__ __forceinline__ double error_leg(const TrackPoint<kModel>& a, const TrackPoint<kModel>& b, double& head_deg) {
    if constexpr (kModel == STE_PREP_SPHERE) {
        if constexpr (kHead) {
            const double dlon = b.lon - a.lon;
            const double east = sin(dlon) * b.c;
            const double north = a.c * sin(b.lat) - sin(a.lat) * b.c * cos(dlon);
            head_deg = floored_mod360(atan2(east, north) * kRad2Deg + 360.0);
        }
        return sphere_dist_km(a.lon, a.lat, a.c, b.lon, b.lat, b.c);
    } else {
        Leg leg;  // inlined here like in the other metric kernels: a call would take a stack frame for the callee's saved registers
        [[clang::always_inline]] leg = wgs84_leg(a.lon, a.lat, b.lon, b.lat);
        if constexpr (kHead) head_deg = leg.head_deg;
        return leg.dist_km;
    }
}

template <int kModel, bool kHead, bool kCov, int kTile>
__global__ __launch_bounds__(64) void track_errors(const ErrorParams p) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (size_t)p.B) return;
    const size_t ld = p.ld, rows = (size_t)p.Nmax + 1;
    const double nan = __builtin_nan("");
    // track_steps(p, t), written out: through the function the kernel's address arithmetic comes out in another order
    const int ns = min(max(p.nsteps ? p.nsteps[t] : p.Nmax, 0), p.Nmax);
    const int s0 = (int)blockIdx.y * kTile;
    // sample j of the tile; the last tile of a call repeats its last sample in the lanes' spare slots and stores it once
    const double* st[kTile];  // walks the rows: component c of the row at hand is st[j][c * ld]
    size_t srow[kTile];       // row k of a row output: [srow[j] + k * ld]
    bool live[kTile];
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
        live[j] = s0 + j < p.nstates;
        const size_t s = (size_t)min(s0 + j, p.nstates - 1);
        st[j] = p.states + (s * rows * 4) * ld + t;
        srow[j] = (s * rows) * ld + t;
    }
    const double* tr = p.truth + t;                     // walks the rows: component c of the row at hand is tr[c * ld]
    const double* co = kHead ? p.course + t : nullptr;  // walks the rows
    const double* cv = kCov ? p.cov + t : nullptr;      // walks the rows: entry r of the row at hand is cv[r * ld]
    const size_t cstep = kCov ? (size_t)p.cov_rows * ld : 0, c11 = (p.cov_rows == STE_ERRORS_COV_PACKED ? 4 : 5) * ld;

    double sum_err[kTile], sum_sq[kTile], max_err[kTile];
    double sum_al[kTile], sum_al2[kTile], sum_cr[kTile], sum_cr2[kTile], sum_q[kTile];
    int n[kTile], max_row[kTile], nbroken[kTile], ncoursed[kTile], nscored[kTile], ninside[kTile];
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
        sum_err[j] = sum_sq[j] = sum_al[j] = sum_al2[j] = sum_cr[j] = sum_cr2[j] = sum_q[j] = 0.0;
        max_err[j] = -__builtin_inf();
        n[j] = nbroken[j] = ncoursed[j] = nscored[j] = ninside[j] = 0;
        max_row[j] = -1;
    }

    // row 0 on its way; rows past ns are never read
    double nlon[kTile], nlat[kTile], ntlon, ntlat, ncourse = 0.0, na = 0.0, nb = 0.0, nc = 0.0;
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
        nlon[j] = st[j][0];
        nlat[j] = st[j][ld];
    }
    ntlon = tr[0];
    ntlat = tr[ld];
    if constexpr (kHead) ncourse = co[0];
    if constexpr (kCov) {
        na = cv[0];
        nb = cv[ld];
        nc = cv[c11];
    }
    for (int k = 0; k <= ns; ++k) {
        double lon[kTile], lat[kTile];
#pragma unroll
        for (int j = 0; j < kTile; ++j) {
            lon[j] = nlon[j];
            lat[j] = nlat[j];
        }
        const double tlon = ntlon, tlat = ntlat, course = ncourse, ca = na, cb = nb, cc = nc;
        if (k < ns) {  // the next row's loads, in flight during this row's arithmetic
#pragma unroll
            for (int j = 0; j < kTile; ++j) {
                st[j] += 4 * ld;
                nlon[j] = st[j][0];
                nlat[j] = st[j][ld];
            }
            tr += 2 * ld;
            ntlon = tr[0];
            ntlat = tr[ld];
            if constexpr (kHead) {
                co += ld;
                ncourse = co[0];
            }
            if constexpr (kCov) {
                cv += cstep;
                na = cv[0];
                nb = cv[ld];
                nc = cv[c11];
            }
        }
        // The leg is computed without a branch of the lane's own around it (a lane that has no truth or no state in this row
        // feeds it zeros and drops the result), so the loop body stays the one block of path_metrics; the one branch is the
        // wave's: no lane with truth in this row, no leg.
        const bool truthed = is_finite(tlon) && is_finite(tlat);
        const bool any = __ballot(truthed) != 0;
        TrackPoint<kModel> tp = {0.0, 0.0, 0.0};
        if (any) tp = track_point<kModel>(truthed ? tlon : 0.0, truthed ? tlat : 0.0);
#pragma unroll
        for (int j = 0; j < kTile; ++j) {
            double e = nan, al = nan, cr = nan, q = nan;
            if (any) {
                const bool ok = truthed && is_finite(lon[j]) && is_finite(lat[j]);
                double head = 0.0;
                const double d = error_leg<kModel, kHead>(tp, track_point<kModel>(ok ? lon[j] : 0.0, ok ? lat[j] : 0.0), head);
                const bool sound = ok && is_finite(d);
                if (truthed && !sound) ++nbroken[j];
                if (sound) {
                    e = d;
                    ++n[j];
                    sum_err[j] = sum_err[j] + e;
                    sum_sq[j] = sum_sq[j] + e * e;
                    if (e > max_err[j]) {
                        max_err[j] = e;
                        max_row[j] = k;
                    }
                    if constexpr (kHead) {
                        if (is_finite(course)) {
                            const double theta = (head - course) * kDeg2Rad;
                            al = e * cos(theta);
                            cr = e * sin(theta);
                            ++ncoursed[j];
                            sum_al[j] = sum_al[j] + al;
                            sum_al2[j] = sum_al2[j] + al * al;
                            sum_cr[j] = sum_cr[j] + cr;
                            sum_cr2[j] = sum_cr2[j] + cr * cr;
                        }
                    }
                    if constexpr (kCov) {
                        const double dx = wrap180(lon[j] - tlon), dy = lat[j] - tlat;
                        const double det = ca * cc - cb * cb;
                        const double qk = (cc * dx * dx - 2.0 * cb * dx * dy + ca * dy * dy) / det;
                        if (is_finite(ca) && is_finite(cb) && is_finite(cc) && is_finite(qk) && ca > 0.0 && det > 0.0) {
                            q = qk;
                            ++nscored[j];
                            sum_q[j] = sum_q[j] + qk;
                            if (qk <= p.nees_limit) ++ninside[j];
                        }
                    }
                }
            }
            if (live[j]) {
                const size_t o = srow[j] + (size_t)k * ld;
                if (p.err) p.err[o] = e;
                if (p.cumerr) p.cumerr[o] = sum_err[j];
                if constexpr (kHead) {
                    if (p.along) p.along[o] = al;
                    if (p.cross) p.cross[o] = cr;
                }
                if constexpr (kCov) {
                    if (p.nees) p.nees[o] = q;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kTile; ++j) {
        if (!live[j]) continue;
        const size_t o = (size_t)(s0 + j) * ld + t;
        if (p.sum_err) p.sum_err[o] = sum_err[j];
        if (p.sum_sq) p.sum_sq[o] = sum_sq[j];
        if (p.max_err) p.max_err[o] = n[j] > 0 ? max_err[j] : nan;
        if (p.n) p.n[o] = n[j];
        if (p.max_row) p.max_row[o] = max_row[j];
        if (p.nbroken) p.nbroken[o] = nbroken[j];
        if constexpr (kHead) {
            if (p.sum_along) p.sum_along[o] = sum_al[j];
            if (p.sum_along_sq) p.sum_along_sq[o] = sum_al2[j];
            if (p.sum_cross) p.sum_cross[o] = sum_cr[j];
            if (p.sum_cross_sq) p.sum_cross_sq[o] = sum_cr2[j];
            if (p.ncoursed) p.ncoursed[o] = ncoursed[j];
        }
        if constexpr (kCov) {
            if (p.sum_nees) p.sum_nees[o] = sum_q[j];
            if (p.nscored) p.nscored[o] = nscored[j];
            if (p.ninside) p.ninside[o] = ninside[j];
        }
    }
}

template <int kModel, bool kHead, bool kCov>
void launch_errors(const ErrorParams& p, hipStream_t s) {
    // a covariance comes with one sample (the call refuses more), so its kernels need no tile
    constexpr int kTile = kCov ? 1 : STE_ERROR_TILE;
    const dim3 grid((unsigned)((p.B + 63) / 64), (unsigned)((p.nstates + kTile - 1) / kTile)), block(64);
    hipLaunchKernelGGL((track_errors<kModel, kHead, kCov, kTile>), grid, block, 0, s, p);
}

}  // namespace
}  // namespace ste

extern "C" int ste_track_errors_f64(const ste_ukf_batch_f64* b, const ste_errors_f64* er, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_track_errors_f64"};
    if (!b) return refuse("batch pointer is NULL");
    if (!er) return refuse("the error arguments (er) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (int rc = refuse.stride(b)) return rc;
    if (!er->states) return refuse("er->states is required");
    if (!er->truth) return refuse("er->truth is required");
    if (int rc = refuse.nstates("er->nstates", er->nstates, " (one grid row per track of a ship)")) return rc;
    if (int rc = refuse.model("er->model", er->model)) return rc;
    if (er->reserved != 0) return refuse("er->reserved must be 0");
    if (er->cov && er->cov_rows != STE_ERRORS_COV_FULL && er->cov_rows != STE_ERRORS_COV_PACKED)
        return refuse("er->cov_rows must be 16 (full matrices) or 10 (upper triangles) with er->cov");
    if (er->cov && er->nstates > 1)
        return refuse("er->cov needs nstates == 1 (a covariance belongs to one track, not to its samples)");
    if (er->cov && !(std::isfinite(er->nees_limit) && er->nees_limit > 0.0))
        return refuse("er->nees_limit must be finite and > 0 with er->cov");
    const bool head = er->sum_along || er->sum_along_sq || er->sum_cross || er->sum_cross_sq || er->ncoursed || er->along || er->cross;
    const bool nees = er->sum_nees || er->nscored || er->ninside || er->nees;
    if (head && !er->course)
        return refuse("an along / cross output (sum_along, sum_along_sq, sum_cross, sum_cross_sq, ncoursed, along, cross) needs er->course");
    if (nees && !er->cov) return refuse("a NEES output (sum_nees, nscored, ninside, nees) needs er->cov");
    if (!head && !nees && !er->sum_err && !er->sum_sq && !er->max_err && !er->n && !er->max_row && !er->nbroken && !er->err && !er->cumerr)
        return refuse("no output asked for (every output pointer is NULL)");
    ErrorParams p;
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.nstates = er->nstates;
    p.cov_rows = er->cov ? er->cov_rows : 0;
    p.ld = track_ld(b);
    p.nsteps = b->nsteps;
    p.states = er->states;
    p.truth = er->truth;
    p.course = er->course;
    p.cov = er->cov;
    p.nees_limit = er->nees_limit;
    p.sum_err = er->sum_err;
    p.sum_sq = er->sum_sq;
    p.max_err = er->max_err;
    p.sum_along = er->sum_along;
    p.sum_along_sq = er->sum_along_sq;
    p.sum_cross = er->sum_cross;
    p.sum_cross_sq = er->sum_cross_sq;
    p.sum_nees = er->sum_nees;
    p.n = er->n;
    p.max_row = er->max_row;
    p.nbroken = er->nbroken;
    p.ncoursed = er->ncoursed;
    p.nscored = er->nscored;
    p.ninside = er->ninside;
    p.err = er->err;
    p.cumerr = er->cumerr;
    p.along = er->along;
    p.cross = er->cross;
    p.nees = er->nees;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool sphere = er->model == STE_PREP_SPHERE;
    with_bool(head, [&](auto hd) {
        with_bool(nees, [&](auto cv) {
            constexpr bool kH = decltype(hd)::value, kC = decltype(cv)::value;
            if (sphere) launch_errors<STE_PREP_SPHERE, kH, kC>(p, s);
            else launch_errors<STE_PREP_WGS84, kH, kC>(p, s);
        });
    });
    return abi_check_hip(hipGetLastError(), "track_errors launch");
}
