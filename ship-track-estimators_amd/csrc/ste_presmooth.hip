// ste_presmooth.hip — observation preparation with SOG / COG smoothed before the rates and the measurements are formed.
//
// Device counterpart of what the reference does per ship between calculate_sog / calculate_cog and get_measurements /
// calculate_*_rate: utils.smooth (a centred moving average, reference cli/main_cli.py:99-104) or scipy's savgol_filter
// (reference examples/example_ukf_rts_smoother_savgol.py).  Both are linear, so the device has one form, ste_fir_f64: w
// interior taps, and h rows of edge weights over the first (mirrored: the last) w samples.  The tables are made on the host
// (track_estimators/batch.py: box_filter, savgol_filter_table); this file only applies them.
//
//   1. ste_track_prep_f64 with sog / cog redirected into the caller's raw_sog / raw_cog (the same kernel, the same bits)
//   2. fir_rows   one wave = 64 consecutive tracks of one row, both series in one launch; w coalesced row reads per output
//   3. rates_z    backward differences of the FILTERED series over gap[i-1], and z
//
// The arithmetic is plain IEEE: every tap is multiplied and added in tap order, nothing is skipped for a zero weight, so a
// non-finite raw value makes exactly the outputs whose window holds it non-finite.  Contraction is off for the whole file,
// as in ste_prep.hip: an unsmoothed series must give the rates of ste_track_prep_f64 bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/ste.h"
#include "ste_err.h"

#pragma clang fp contract(off)

namespace ste {
namespace {

constexpr int kFirMaxWindow = 128;

struct FirSeries {
    const double* src;   // [T][B] raw series
    double* dst;         // [T][B] filtered series
    const double* taps;  // [w], NULL: copy
    const double* edge;  // [h][w]
    int w, left, h, circular;
};

struct FirParams {
    int B, T;
    unsigned ntile;  // tiles of 64 tracks
    const int32_t* nobs;
    FirSeries s[2];
};

// d = delta - 360 rint(delta / 360): the difference of two courses as an angle in [-180, 180]
__device__ __forceinline__ double wrap_diff(double delta) { return delta - 360.0 * rint(delta / 360.0); }

template <bool kCircular>
__device__ __forceinline__ double fir_term(double acc, double c, double y, double centre) {
    return acc + c * (kCircular ? wrap_diff(y - centre) : y);
}

// Row i of track t.  Interior rows read y[i - left + k] (0 outside [0, n)) against taps[k]; with h > 0 row i < h is edge row i
// over y[0 .. w), row n - 1 - r (r < h) is edge row r reversed over y[n - w .. n).  The row is uniform over the wave and so is
// the interior / leading-edge choice; the trailing edge depends on the lane's n, so when any live lane of the wave is on an
// edge every lane takes its weights through its own pointer (kUniform = false); otherwise the taps are scalar loads.
template <bool kCircular, bool kUniform>
__device__ __forceinline__ double fir_row(const FirSeries& f, int B, int t, int i, int n, const double* cp, int cstep, int base) {
    const double centre = kCircular ? f.src[(size_t)i * B + t] : 0.0;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < f.w; ++k) {
        const int j = base + k;
        const bool in = j >= 0 && j < n;
        // the load is unconditional on a clamped row (n >= 1 here), so that the loads of an unrolled group go out together
        const double v = f.src[(size_t)min(max(j, 0), n - 1) * B + t];
        const double y = in ? v : (kCircular ? centre : 0.0);  // circular: a padded tap has d = 0
        const double c = kUniform ? f.taps[k] : cp[(ptrdiff_t)k * cstep];
        acc = fir_term<kCircular>(acc, c, y, centre);
    }
    if (kCircular) {
        double r = fmod(centre + acc, 360.0);
        if (r < 0.0) r += 360.0;
        if (r >= 360.0) r = 0.0;  // -tiny + 360 rounds to 360
        return r;
    }
    return acc;
}

// grid: x = (group of 4 rows) * ntile + tile of 64 tracks, y = series; block (64, 4): threadIdx.y picks the row, so each wave
// holds one row of 64 consecutive tracks.
__global__ void __launch_bounds__(256) fir_rows(FirParams p) {
    const FirSeries& f = p.s[blockIdx.y];
    const long long tt = (long long)(blockIdx.x % p.ntile) * 64 + threadIdx.x;
    const int i = (int)(blockIdx.x / p.ntile) * 4 + (int)threadIdx.y;
    if (i >= p.T) return;  // uniform over the wave
    const bool lane = tt < p.B;
    const int t = lane ? (int)tt : 0;
    const int n = lane ? (p.nobs ? min(max(p.nobs[t], 0), p.T) : p.T) : 0;
    const bool live = lane && i < n;
    double out = 0.0;
    if (f.taps == nullptr) {
        if (live) out = f.src[(size_t)i * p.B + t];
    } else {
        const bool lead = i < f.h, trail = !lead && i >= n - f.h;
        const bool on_edge = live && (lead || trail);
        if (__ballot(on_edge) == 0ull) {
            if (live)
                out = f.circular ? fir_row<true, true>(f, p.B, t, i, n, nullptr, 0, i - f.left)
                                 : fir_row<false, true>(f, p.B, t, i, n, nullptr, 0, i - f.left);
        } else if (live) {
            const double* cp = f.taps;
            int cstep = 1, base = i - f.left;
            if (lead) {
                cp = f.edge + (size_t)i * f.w;
                base = 0;
            } else if (trail) {
                cp = f.edge + (size_t)(n - 1 - i) * f.w + (f.w - 1);
                cstep = -1;
                base = n - f.w;
            }
            out = f.circular ? fir_row<true, false>(f, p.B, t, i, n, cp, cstep, base)
                             : fir_row<false, false>(f, p.B, t, i, n, cp, cstep, base);
        }
    }
    if (lane) f.dst[(size_t)i * p.B + t] = out;
}

struct RateParams {
    int B, T;
    const int32_t* nobs;
    const double *lon, *lat, *gap, *sog, *cog;
    double *sog_rate, *cog_rate, *z;
};

// The rules of track_prep (ste_prep.hip) on the filtered series: backward difference over gap[i-1], 0 at i = 0 and in rows
// at or past nobs.  (A track with fewer than 2 observations ends as 0 throughout, as there, though nothing here sees to it:
// the raw kernel writes 0 for it and a filter of zeros is 0.)
__global__ void __launch_bounds__(256) rates_z(RateParams p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.T * p.B) return;
    const int t = (int)(idx % p.B), i = (int)(idx / p.B);
    const int n = p.nobs ? min(p.nobs[t], p.T) : p.T;
    const double sog = p.sog[idx], cog = p.cog[idx];
    double sr = 0.0, cr = 0.0;
    if (i >= 1 && i < n) {
        const double g = p.gap[idx - p.B];
        sr = (sog - p.sog[idx - p.B]) / g;
        cr = (cog - p.cog[idx - p.B]) / g;
    }
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

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int check_fir(const ste_fir_f64* f, const char* which) {
    char msg[160];
    const char* what = nullptr;
    if (f->window < 2 || f->window > kFirMaxWindow)
        what = "window must be in 2..128";
    else if (f->left < 0 || f->left >= f->window)
        what = "left must be in 0..window-1";
    else if (f->nedge < 0 || 2 * f->nedge > f->window)
        what = "nedge must be in 0..window/2";
    else if (!f->taps)
        what = "taps is NULL";
    else if (f->nedge > 0 && !f->edge)
        what = "edge is NULL with nedge > 0";
    else if (f->circular != 0 && f->circular != 1)
        what = "circular must be 0 or 1";
    if (!what) return STE_OK;
    snprintf(msg, sizeof msg, "%s: %s", which, what);
    return abi_fail(STE_EINVAL, msg);
}

FirSeries series_of(const ste_fir_f64* f, const double* src, double* dst) {
    if (!f) return FirSeries{src, dst, nullptr, nullptr, 0, 0, 0, 0};
    return FirSeries{src, dst, f->taps, f->edge, f->window, f->left, f->nedge, f->circular};
}

}  // namespace
}  // namespace ste

extern "C" int ste_track_prep_smooth_f64(const ste_prep_batch_f64* b, const ste_fir_f64* fir_sog, const ste_fir_f64* fir_cog,
                                         double* raw_sog, double* raw_cog, void* stream) {
    using namespace ste;
    if (!b) return abi_fail(STE_EINVAL, "prep batch pointer is NULL");
    if (!raw_sog || !raw_cog) return abi_fail(STE_EINVAL, "raw_sog and raw_cog (workspace [Tmax][B]) are required");
    if (fir_sog) {
        int rc = check_fir(fir_sog, "fir_sog");
        if (rc) return rc;
    }
    if (fir_cog) {
        int rc = check_fir(fir_cog, "fir_cog");
        if (rc) return rc;
    }
    // checked here on the caller's struct: below ste_track_prep_f64 sees a copy whose sog / cog are the workspace
    if (b->B <= 0 || b->Tmax < 1) return abi_fail(STE_EINVAL, "B must be > 0 and Tmax >= 1");
    if (!b->sog || !b->cog) return abi_fail(STE_EINVAL, "sog and cog are required");
    {
        const size_t cells = (size_t)b->B * b->Tmax, bytes = sizeof(double) * cells;
        struct Range {
            const void* p;
            size_t n;
        };
        const Range others[] = {{b->sog, bytes},      {b->cog, bytes},
                                {b->sog_rate, bytes}, {b->cog_rate, bytes},
                                {b->z, 4 * bytes},    {b->lon, bytes},
                                {b->lat, bytes},      {b->gap, bytes - sizeof(double) * (size_t)b->B},
                                {b->nobs, sizeof(int32_t) * (size_t)b->B}};
        bool alias = overlaps(raw_sog, bytes, raw_cog, bytes);
        for (const Range& o : others) alias = alias || overlaps(raw_sog, bytes, o.p, o.n) || overlaps(raw_cog, bytes, o.p, o.n);
        if (alias) return abi_fail(STE_EINVAL, "raw_sog / raw_cog alias each other, an output or an input of the batch");
        if ((((size_t)b->B + 63) / 64) * (((size_t)b->Tmax + 3) / 4) > 0x7fffffffull)
            return abi_fail(STE_EINVAL, "B * Tmax is beyond what one launch covers");
    }
    // the raw series, by the kernel of ste_track_prep_f64 (which checks the batch and resets status); the rates it leaves in
    // b->sog_rate / b->cog_rate are overwritten below
    ste_prep_batch_f64 raw = *b;
    raw.sog = raw_sog;
    raw.cog = raw_cog;
    raw.z = nullptr;
    int rc = ste_track_prep_f64(&raw, stream);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned ntile = (unsigned)(((size_t)b->B + 63) / 64), nrowgroup = (unsigned)(((size_t)b->Tmax + 3) / 4);
    FirParams fp{b->B, b->Tmax, ntile, b->nobs, {series_of(fir_sog, raw_sog, b->sog), series_of(fir_cog, raw_cog, b->cog)}};
    hipLaunchKernelGGL(fir_rows, dim3(ntile * nrowgroup, 2), dim3(64, 4), 0, s, fp);
    rc = abi_check_hip(hipGetLastError(), "fir_rows launch");
    if (rc) return rc;
    RateParams rp{b->B, b->Tmax, b->nobs, b->lon, b->lat, b->gap, b->sog, b->cog, b->sog_rate, b->cog_rate, b->z};
    const size_t total = (size_t)b->B * b->Tmax;
    hipLaunchKernelGGL(rates_z, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rp);
    return abi_check_hip(hipGetLastError(), "rates_z launch");
}
