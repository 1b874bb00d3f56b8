// ste_candidates.hip — the broad phase of the encounter search (include/ste.h: CANDIDATES, ste_encounter_candidates_mask_f64,
// ste_encounter_candidates_list_f64): which pairs of tracks of a batch can have been within reach of each other at one
// instant.  The clock is cut into windows; every track gets, per window it lives in, a box around the unit vectors of its
// rows and the half length of its longest step; two tracks are NEAR in a window when the boxes are closer than the chord of
// the reach.  The header carries the rule and tests/candidate_cases.py restates it in NumPy.
//
//   cand_boxes   a lane per track, one in-order pass over its steps (the mapping of path_metrics).  A running box belongs to
//                the window the clock is in; it is stored when the clock leaves the window, so every (window, track) word has
//                one writer and is written once.  Only the windows wlo .. whi of a track are written; nothing else is read.
//   cand_mask    a wave per 64 x 64 tile of (i, j) on and above the diagonal.  A lane is a j and keeps its box of the current
//                window in registers; the 64 i-boxes are staged in LDS and read as broadcasts.  Windows outer, i inner: the
//                boxes of the next window are requested before the 64 tests of the current one.  64 ballots turn the lanes'
//                found-bits into one 64-bit word per (i, 64-block of j), stored by lane i.
//   cand_count   a wave per row: the popcount of its words (the tiles of a row are written by different blocks, and nothing
//                here adds into a shared word).
//   cand_list    a wave per row: walks the row's words and writes its pairs from the exclusive prefix of the row counts, in
//                (i, j) order; on request the first near window and the number of near windows, recomputed for these pairs.
//
// No atomics; every word has one writer; plain loads and stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ste.h"
#include "ste_err.h"
#include "ste_track.h"  // is_finite, wave_min, wave_max; it switches contraction off, and the pragma below says so here

#pragma clang fp contract(off)  // explicit fma() only (ste_math.h): every expression of the rule as written

namespace ste {
namespace {

constexpr double kPiD = 3.141592653589793;
constexpr double kSlack = 1e-7;  // radians, the slack of batch.candidate_pairs

struct CandParams {
    int B, Nmax, NW;
    size_t ld;              // tracks per row of states / dt (track_stride, or B)
    size_t nwords;          // 64-bit words per mask row: ceil(B / 64)
    const int32_t* nsteps;  // [B] or nullptr
    const double* dt;       // [Nmax][ld]
    const double* states;   // [Nmax+1][4][ld]
    const double* t0;       // [B] or nullptr
    const double* margin;   // [B] or nullptr, km
    double time0, window_h;
    double reach;           // reach_km / 6378.137
    // workspace
    double* boxes;          // [NW][7][B]: lo[3], hi[3], h
    uint64_t* mask;         // [B][nwords]
    int32_t* wlo;           // [B]
    int32_t* whi;           // [B]
    int32_t* count;         // [B]
    int32_t* status;        // [B]
    // list
    const int64_t* row_offset;  // [B]
    int64_t npairs;
    int32_t* pairs;         // [P][2]
    int32_t* wfirst;        // [P] or nullptr
    int32_t* nwin;          // [P] or nullptr
};

__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }

// win(x) and whether clamping changed it.  x is t0 + a sum of finite dt >= 0 with t0 finite: finite or +inf, never NaN.
__device__ __forceinline__ int window_of(double x, double time0, double W, int NW, bool& clipped) {
    const double f = floor((x - time0) / W);
    const double top = (double)(NW - 1);
    const double c = f < 0.0 ? 0.0 : (f > top ? top : f);
    clipped = clipped || c != f;
    return c == c ? (int)c : 0;
}

struct Box {
    double lo[3], hi[3], h;
};

__device__ __forceinline__ void box_empty(Box& b) {
    b.lo[0] = b.lo[1] = b.lo[2] = __builtin_inf();
    b.hi[0] = b.hi[1] = b.hi[2] = -__builtin_inf();
    b.h = 0.0;
}

__device__ __forceinline__ void box_store(const CandParams& p, int w, int t, const Box& b) {
    double* o = p.boxes + ((size_t)w * 7) * (size_t)p.B + (size_t)t;
    const size_t B = (size_t)p.B;
    o[0] = b.lo[0];
    o[B] = b.lo[1];
    o[2 * B] = b.lo[2];
    o[3 * B] = b.hi[0];
    o[4 * B] = b.hi[1];
    o[5 * B] = b.hi[2];
    o[6 * B] = b.h;
}

// The unit vector of a row; a row that is not finite belongs to no sound step and gets no trigonometry.  Not the
// unit_vector of ste_track.h: the boxes are made with sincos_fast, as tests/candidate_cases.py restates them.
__device__ __forceinline__ void box_vector(double lon, double lat, double (&u)[3]) {
    if (is_finite(lon) && is_finite(lat)) {
        double sl, cl, sp, cp;
        sincos_fast(lon * kDeg2Rad, sl, cl);
        sincos_fast(lat * kDeg2Rad, sp, cp);
        u[0] = cp * cl;
        u[1] = cp * sl;
        u[2] = sp;
    } else {
        u[0] = u[1] = u[2] = __builtin_nan("");
    }
}

__global__ __launch_bounds__(64) void cand_boxes(const CandParams p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.B) return;
    const size_t ld = p.ld;
    const int ns = track_steps(p, t);
    const double t0 = p.t0 ? p.t0[t] : 0.0;
    int status = 0;
    if (p.margin) {
        const double m = p.margin[t];
        if (!(m >= 0.0 && is_finite(m))) status |= STE_CAND_BAD_MARGIN;
    }
    int wlo = 0, whi = -1;
    const bool bad_t0 = !is_finite(t0);
    bool bad_dt = false, clipped = false, any_sound = false;
    if (!bad_t0) {
        const double* st = p.states + (size_t)t;  // row k, component c: st[(k * 4 + c) * ld]
        const double* dtp = p.dt + (size_t)t;
        double T = 0.0;
        int a = window_of(t0 + T, p.time0, p.window_h, p.NW, clipped);
        wlo = a;
        Box acc;
        box_empty(acc);
        double lon = 0.0, lat = 0.0, nlon = 0.0, nlat = 0.0, dtk = 0.0;
        double u[3] = {0.0, 0.0, 0.0}, v[3];
        if (ns > 0) {  // rows past nsteps are never read
            lon = st[0];
            lat = st[ld];
            nlon = st[4 * ld];
            nlat = st[5 * ld];
            dtk = dtp[0];
            box_vector(lon, lat, u);
        }
        for (int k = 0; k < ns; ++k) {
            // what the next step needs, in flight during this step's arithmetic
            double pdt = 0.0, plon = 0.0, plat = 0.0;
            if (k + 1 < ns) {
                const size_t r = (size_t)k + 2;
                pdt = dtp[(r - 1) * ld];
                plon = st[(r * 4) * ld];
                plat = st[(r * 4 + 1) * ld];
            }
            if (!(dtk >= 0.0 && is_finite(dtk))) {  // the track ends here: the walk of ENCOUNTERS goes no further either
                bad_dt = true;
                break;
            }
            T = T + dtk;
            const int b = window_of(t0 + T, p.time0, p.window_h, p.NW, clipped);
            box_vector(nlon, nlat, v);
            const double delta = wrap180(nlon - lon), dlat = nlat - lat;
            const bool sound = fabs(delta) < 90.0 && is_finite(lat) && is_finite(nlat);
            Box sb;
            box_empty(sb);
            if (sound) {
                any_sound = true;
                for (int c = 0; c < 3; ++c) {
                    sb.lo[c] = dmin(u[c], v[c]);
                    sb.hi[c] = dmax(u[c], v[c]);
                    acc.lo[c] = dmin(acc.lo[c], sb.lo[c]);
                    acc.hi[c] = dmax(acc.hi[c], sb.hi[c]);
                }
                sb.h = 0.5 * kDeg2Rad * sqrt(delta * delta + dlat * dlat);
                acc.h = dmax(acc.h, sb.h);
            }
            if (b > a) {  // the clock leaves window a: it is complete; the step alone fills the windows it passes over
                box_store(p, a, t, acc);
                for (int w = a + 1; w < b; ++w) box_store(p, w, t, sb);
                acc = sb;
                a = b;
            }
            lon = nlon;
            lat = nlat;
            u[0] = v[0];
            u[1] = v[1];
            u[2] = v[2];
            nlon = plon;
            nlat = plat;
            dtk = pdt;
        }
        box_store(p, a, t, acc);
        whi = a;
        if (clipped) status |= STE_CAND_CLIPPED;
        if (!any_sound) status |= STE_CAND_EMPTY;
    }
    if (bad_t0 || bad_dt) status |= STE_CAND_BAD_TIME;
    if (!any_sound || (status & STE_CAND_BAD_MARGIN)) {  // pairs with nothing: an empty window range
        wlo = 0;
        whi = -1;
    }
    p.wlo[t] = wlo;
    p.whi[t] = whi;
    p.status[t] = status;
}

// NEAR of the header.  rmm = (reach / 6378.137 + m_i) + m_j.  An empty box holds +inf / -inf: every gap is +inf, no NaN.
__device__ __forceinline__ bool near_test(double li0, double li1, double li2, double hi0, double hi1, double hi2, double h_i,
                                          double lj0, double lj1, double lj2, double hj0, double hj1, double hj2, double h_j,
                                          double rmm) {
    const bool both = li0 <= hi0 && lj0 <= hj0;
    const double g0 = dmax(dmax(0.0, li0 - hj0), lj0 - hi0);
    const double g1 = dmax(dmax(0.0, li1 - hj1), lj1 - hi1);
    const double g2 = dmax(dmax(0.0, li2 - hj2), lj2 - hi2);
    const double gg = (g0 * g0 + g1 * g1) + g2 * g2;
    const double th = dmin(((rmm + h_i) + h_j) + kSlack, kPiD);
    double s, cs;
    sincos_fast(th / 2.0, s, cs);
    const double c = 2.0 * s;
    return both && gg <= c * c;
}

__device__ __forceinline__ void box_load(const CandParams& p, int w, int t, bool in, double (&b)[7]) {
    if (in) {
        const double* o = p.boxes + ((size_t)w * 7) * (size_t)p.B + (size_t)t;
        for (int c = 0; c < 7; ++c) b[c] = o[(size_t)c * (size_t)p.B];
    } else {
        b[0] = b[1] = b[2] = __builtin_inf();
        b[3] = b[4] = b[5] = -__builtin_inf();
        b[6] = 0.0;
    }
}

__device__ __forceinline__ double margin_rad(const CandParams& p, int t) { return p.margin ? p.margin[t] / kEarthRadius : 0.0; }

__global__ __launch_bounds__(64) void cand_mask(const CandParams p) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;  // the upper triangle of tiles
    __shared__ double sbox[8][64];  // per i of the tile: lo[3], hi[3], h of the current window, and reach + m_i
    const int lane = threadIdx.x;
    const int i = ti * 64 + lane, j = tj * 64 + lane;
    const bool iok = i < p.B, jok = j < p.B;
    const int iwlo = iok ? p.wlo[i] : 0, iwhi = iok ? p.whi[i] : -1;
    const int jwlo = jok ? p.wlo[j] : 0, jwhi = jok ? p.whi[j] : -1;
    const bool ilive = iwlo <= iwhi, jlive = jwlo <= jwhi;
    const double mj = jlive ? margin_rad(p, j) : 0.0;
    sbox[7][lane] = p.reach + (ilive ? margin_rad(p, i) : 0.0);
    // the windows in which some i and some j of the tile both live
    const int wa = max(wave_min(ilive ? iwlo : 0x7fffffff), wave_min(jlive ? jwlo : 0x7fffffff));
    const int wb = min(wave_max(ilive ? iwhi : -1), wave_max(jlive ? jwhi : -1));
    const bool diag = ti == tj;
    const uint64_t below = ((uint64_t)1 << lane) - 1;  // the i of a diagonal tile with i < j
    const uint64_t irows = __ballot(ilive);  // by every lane, before anything depends on j
    const uint64_t want = jlive ? (irows & (diag ? below : ~(uint64_t)0)) : 0;  // what this lane can still find
    uint64_t found = 0;
    double bi[7], bj[7];
    if (wa <= wb) {
        box_load(p, wa, i, ilive && wa >= iwlo && wa <= iwhi, bi);
        box_load(p, wa, j, jlive && wa >= jwlo && wa <= jwhi, bj);
    }
    for (int w = wa; w <= wb; ++w) {
        __syncthreads();  // the tests of the window before are through with sbox
        for (int c = 0; c < 7; ++c) sbox[c][lane] = bi[c];
        const double lj0 = bj[0], lj1 = bj[1], lj2 = bj[2], hj0 = bj[3], hj1 = bj[4], hj2 = bj[5], h_j = bj[6];
        __syncthreads();
        if (w < wb) {  // the next window's boxes, in flight during this window's tests
            box_load(p, w + 1, i, ilive && w + 1 >= iwlo && w + 1 <= iwhi, bi);
            box_load(p, w + 1, j, jlive && w + 1 >= jwlo && w + 1 <= jwhi, bj);
        }
#pragma unroll 4
        for (int ii = 0; ii < 64; ++ii) {
            const bool nr = near_test(sbox[0][ii], sbox[1][ii], sbox[2][ii], sbox[3][ii], sbox[4][ii], sbox[5][ii], sbox[6][ii],
                                      lj0, lj1, lj2, hj0, hj1, hj2, h_j, sbox[7][ii] + mj);
            found |= (uint64_t)nr << ii;
        }
        if (!__any((found & want) != want)) break;  // every lane has its answer
    }
    found &= want;
    uint64_t mine = 0;
    for (int ii = 0; ii < 64; ++ii) {
        const uint64_t word = __ballot((found >> ii) & 1);
        if (lane == ii) mine = word;
    }
    if (iok) p.mask[(size_t)i * p.nwords + (size_t)tj] = mine;
}

__global__ __launch_bounds__(64) void cand_count(const CandParams p) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const uint64_t* row = p.mask + (size_t)i * p.nwords;
    int c = 0;
    for (size_t wd = (size_t)(i >> 6) + lane; wd < p.nwords; wd += 64) c += __popcll(row[wd]);
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if (lane == 0) p.count[i] = c;
}

template <bool kDetails>
__global__ __launch_bounds__(64) void cand_list(const CandParams p) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const uint64_t* row = p.mask + (size_t)i * p.nwords;
    int64_t off = p.row_offset[i];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    int iwlo = 0, iwhi = -1;
    double rm = 0.0;
    if constexpr (kDetails) {
        iwlo = p.wlo[i];
        iwhi = p.whi[i];
        rm = p.reach + margin_rad(p, i);
    }
    for (size_t wd = (size_t)(i >> 6); wd < p.nwords; ++wd) {
        const uint64_t word = row[wd];
        if (word == 0) continue;
        const int64_t q = off + __popcll(word & below);
        off += __popcll(word);
        const int j = (int)(wd * 64) + lane;
        // outside [0, npairs) or [0, B): a row_offset or a workspace that is not the mask call's; nothing is written
        if (!((word >> lane) & 1) || q < 0 || q >= p.npairs || j >= p.B) continue;
        p.pairs[2 * q] = i;
        p.pairs[2 * q + 1] = j;
        if constexpr (kDetails) {
            const int lo = max(iwlo, p.wlo[j]), hi = min(iwhi, p.whi[j]);
            const double rmm = rm + margin_rad(p, j);
            int first = -1, n = 0;
            for (int w = lo; w <= hi; ++w) {
                double a[7], b[7];
                box_load(p, w, i, true, a);
                box_load(p, w, j, true, b);
                if (near_test(a[0], a[1], a[2], a[3], a[4], a[5], a[6], b[0], b[1], b[2], b[3], b[4], b[5], b[6], rmm)) {
                    if (n == 0) first = w;
                    ++n;
                }
            }
            if (p.wfirst) p.wfirst[q] = first;
            if (p.nwin) p.nwin[q] = n;
        }
    }
}

size_t workspace_bytes(int64_t B, int64_t NW) {
    const size_t b = (size_t)B, nwords = (b + 63) / 64;
    return 8 * (7 * (size_t)NW * b + b * nwords) + 4 * 3 * b;
}

// the refusals the two calls share, and the parameters; returns STE_OK or the recorded failure
int cand_params(const Refusal& refuse, const ste_ukf_batch_f64* b, const ste_candidates_f64* c, CandParams& p) {
    if (!b) return refuse("batch pointer is NULL");
    if (!c) return refuse("the candidate arguments (c) are NULL");
    if (int rc = refuse.shape(b)) return rc;
    if (b->B > STE_CANDIDATES_MAX_TRACKS) return refuse("B is limited to STE_CANDIDATES_MAX_TRACKS (2^20) per call (the mask is B x B bits)");
    if (int rc = refuse.stride(b)) return rc;
    if (!c->states) return refuse("c->states is required");
    if (!b->dt) return refuse("the batch's dt is required (the clock is made of its sums)");
    if (!(std::isfinite(c->window_h) && c->window_h > 0.0)) return refuse("c->window_h must be finite and > 0");
    if (!std::isfinite(c->time0)) return refuse("c->time0 must be finite");
    if (c->nwindows < 1 || c->nwindows > STE_CANDIDATES_MAX_WINDOWS)
        return refuse("c->nwindows must be between 1 and STE_CANDIDATES_MAX_WINDOWS (4096)");
    if (!(std::isfinite(c->reach_km) && c->reach_km >= 0.0 && c->reach_km <= STE_CANDIDATES_MAX_REACH_KM))
        return refuse("c->reach_km must be finite and between 0 and STE_CANDIDATES_MAX_REACH_KM (20000)");
    if (c->flags != 0) return refuse("c->flags must be 0");
    if (c->reserved != 0) return refuse("c->reserved must be 0");
    if (!c->workspace) return refuse("c->workspace is required");
    if (c->workspace_bytes < workspace_bytes(b->B, c->nwindows))
        return refuse("c->workspace_bytes is below ste_encounter_candidates_workspace(B, nwindows)");
    if (((uintptr_t)c->workspace & 7) != 0) return refuse("c->workspace must be aligned to 8 bytes");
    p.B = b->B;
    p.Nmax = b->Nmax;
    p.NW = c->nwindows;
    p.ld = track_ld(b);
    p.nwords = ((size_t)b->B + 63) / 64;
    p.nsteps = b->nsteps;
    p.dt = b->dt;
    p.states = c->states;
    p.t0 = c->t0;
    p.margin = c->track_margin_km;
    p.time0 = c->time0;
    p.window_h = c->window_h;
    p.reach = c->reach_km / kEarthRadius;
    const size_t B = (size_t)b->B;
    p.boxes = static_cast<double*>(c->workspace);
    p.mask = reinterpret_cast<uint64_t*>(p.boxes + 7 * (size_t)c->nwindows * B);
    p.wlo = reinterpret_cast<int32_t*>(p.mask + B * p.nwords);
    p.whi = p.wlo + B;
    p.count = p.whi + B;
    p.status = c->track_status;
    p.row_offset = c->row_offset;
    p.npairs = c->npairs;
    p.pairs = c->pairs;
    p.wfirst = c->wfirst;
    p.nwin = c->nwin;
    return STE_OK;
}

}  // namespace
}  // namespace ste

extern "C" size_t ste_encounter_candidates_workspace(int32_t B, int32_t nwindows) {
    if (B <= 0 || nwindows < 1) return 0;
    return ste::workspace_bytes(B, nwindows);
}

extern "C" int ste_encounter_candidates_mask_f64(const ste_ukf_batch_f64* b, const ste_candidates_f64* c, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_encounter_candidates_mask_f64"};
    CandParams p;
    if (int rc = cand_params(refuse, b, c, p)) return rc;
    if (!c->track_status) return refuse("c->track_status is required");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned nt = (unsigned)p.nwords;
    hipLaunchKernelGGL(cand_boxes, dim3(nt), dim3(64), 0, s, p);
    hipLaunchKernelGGL(cand_mask, dim3(nt, nt), dim3(64), 0, s, p);
    hipLaunchKernelGGL(cand_count, dim3((unsigned)p.B), dim3(64), 0, s, p);
    return abi_check_hip(hipGetLastError(), "encounter candidates (boxes, mask, count) launch");
}

extern "C" int ste_encounter_candidates_list_f64(const ste_ukf_batch_f64* b, const ste_candidates_f64* c, void* stream) {
    using namespace ste;
    const Refusal refuse{"ste_encounter_candidates_list_f64"};
    CandParams p;
    if (int rc = cand_params(refuse, b, c, p)) return rc;
    if (!c->row_offset) return refuse("c->row_offset is required");
    if (!c->pairs) return refuse("c->pairs is required");
    if (c->npairs < 1 || c->npairs > STE_ENCOUNTER_MAX_PAIRS)
        return refuse("c->npairs must be between 1 and STE_ENCOUNTER_MAX_PAIRS (2^26)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->wfirst || c->nwin) hipLaunchKernelGGL(cand_list<true>, dim3((unsigned)p.B), dim3(64), 0, s, p);
    else hipLaunchKernelGGL(cand_list<false>, dim3((unsigned)p.B), dim3(64), 0, s, p);
    return abi_check_hip(hipGetLastError(), "cand_list launch");
}
