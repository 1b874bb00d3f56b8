/*
 * ste.h — C ABI of the MI355X-native batched UKF + URTSS path ("ship-track-estimators", ste).
 *
 * The reference (NOC-OI/ship-track-estimators) is pure Python and has no FFI of its own; its boundary for this path
 * is the Python API.  Each entry point below is the batched, device-resident counterpart of one
 * reference method and is what a reference-side binding (ctypes) would load:
 *
 *   ste_ukf_forward_f64      KalmanFilterBase.run            src/track_estimators/kalman_filters/kalman_filter.py:36-117
 *                            (+ UnscentedKalmanFilter.predict / .update, kalman_filters/unscented.py:144-265)
 *   ste_urtss_backward_f64   KalmanFilterBase.run_rts_smoother kalman_filter.py:119-137
 *                            (+ UnscentedKalmanFilter.rts_step, unscented.py:267-351)
 *   ste_ukf_urtss_f64        both, back to back on one stream (examples/example_ukf_rts_smoother_batch.py:75-87)
 *   ste_ukf_predict_f64      UnscentedKalmanFilter.predict (one step, many filters)   unscented.py:144-207
 *   ste_ukf_update_f64       UnscentedKalmanFilter.update  (one step, many filters)   unscented.py:209-265
 *   ste_geodetic_dynamics_f64  geodetic_dynamics              kalman_filters/non_linear_process.py:6-85
 *   ste_sigma_points_f64     UnscentedKalmanFilter.compute_sigma_points  unscented.py:76-107
 *   ste_track_prep_f64       ShipTrack.calculate_sog / _cog / _sog_rate / _cog_rate / get_measurements
 *                            src/track_estimators/ship_track.py:197-338 (distance / heading: utils.py:9-147)
 *   ste_track_prep_smooth_f64  the same with SOG / COG smoothed first: utils.smooth (utils.py:150-172, cli/main_cli.py:99-104)
 *                            or scipy's savgol_filter (examples/example_ukf_rts_smoother_savgol.py), as one table-driven filter
 *   ste_path_metrics_f64     distance sailed and line-crossing times of tracks that stay on the device (smoothed, filtered or
 *                            sampled): per-leg utils.haversine_formula / geographiclib_distance (utils.py:9-113), summed
 *   ste_region_metrics_f64   time inside a polygon, first entry, entries, distance inside and per-row flags of such tracks (no
 *                            counterpart in the reference: its callers would loop over a geometry library on a download)
 *   ste_grid_metrics_f64     ship-hours per cell of a regular lon / lat grid, summed over such tracks in exact integer ticks,
 *                            and entries per cell (no counterpart in the reference: a download and a host loop)
 *   ste_encounter_metrics_f64  closest approach and time within a radius of pairs of such tracks (no counterpart in the reference)
 *   ste_track_positions_f64  position, speed and heading of such tracks at given clock times, and the moments of the positions over
 *                            the samples for an error ellipse (no counterpart in the reference: a download, a search and a host loop)
 *   ste_site_metrics_f64     closest approach and time within a radius of such tracks at fixed sites (ports), a dense (sample, site,
 *                            track) block (no counterpart in the reference)
 *   ste_line_metrics_f64     closest approach and crossings of such tracks at polylines (coasts, cables, gates), a dense (sample,
 *                            line, track) block (no counterpart in the reference)
 *   ste_route_metrics_f64    discrete Frechet distance and time-warping cost of pairs of such tracks as curves without a clock
 *                            (the reference's performance_metrics.py compares two tracks row by row, which needs equal rows)
 *   ste_speed_metrics_f64    speed made good per step, its maximum, hours per speed band and runs at or below (above) a speed
 *                            threshold (stops, sustained speed) of such tracks: the per-leg distance of utils.py:9-113 over dt
 *   ste_track_errors_f64     error of such tracks against truth positions at the tracks' own rows, in km, split along and across
 *                            the true course and scored against the track's covariance (performance_metrics.py: rmse,
 *                            cum_abs_diff and abs_diff compare in degrees, one ship at a time, on downloaded arrays)
 *   ste_raster_metrics_f64   the values of a gridded field (land mask, depth, density) along such tracks: time with and without
 *                            data, the time-weighted sum, extremes and when, and excursions past a threshold, in exact integer
 *                            ticks (no counterpart in the reference: a download and a host loop)
 *   ste_track_simplify_f64   such tracks made smaller within a tolerance: the time-aware Douglas-Peucker rule (or the classic one
 *                            on shape alone), keep flags and the kept rows compacted into a fleet of their own (no counterpart in
 *                            the reference, whose callers download every row of every history)
 *   ste_ukf_noise_moments_f64 / ste_ukf_noise_mstep_f64   the measurement noise R of a track or a group of tracks fitted to the
 *                            data by EM, from the smoothed marginals on the device (no counterpart in the reference, where R is
 *                            an argument of UnscentedKalmanFilter, unscented.py:55-61)
 *   ste_field_values_f64     the values of a space-time gridded field (SST, pressure, wind, ice) where such tracks were at given
 *                            clock times, trilinear with no-data handling or nearest-node, and their count, moments and extremes
 *                            over the samples (no counterpart in the reference: a download of S x Q positions and a host loop)
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every array pointer is a DEVICE pointer unless marked HOST; the caller owns every buffer, the library never
 *     allocates outputs or frees inputs.
 *   - calls are asynchronous on `stream`; no global state except a thread-local error string (launch shape and lane
 *     mapping are per call: flags / tuning of the batch struct).
 *   - return 0 on success, a negative STE_E* code on argument / launch errors (message via ste_last_error()).
 *   - per-track numerical trouble never aborts a batch: it is reported in status[] (mirrors the batch example's
 *     try/except/continue, example_ukf_rts_smoother_batch.py:73-90).
 *   - state order [lon deg, lat deg, speed km/h, heading deg], time in hours (non_linear_process.py:54-57).
 *
 * Data layout in HBM: structure-of-arrays with the TRACK index fastest, so that consecutive lanes (= consecutive
 * tracks) read and write consecutive 8-byte words:
 *      per-step scalar   a[k][t]            -> a[k*B + t]
 *      per-step vector   v[k][c][t]         -> v[(k*4 + c)*B + t]
 *      per-step matrix   M[k][r][c][t]      -> M[(k*16 + r*4 + c)*B + t]
 */
#ifndef STE_H
#define STE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STE_VERSION 340 /* 0.3.4: posterior covariance on the GP path (ste_gp_predict_cov_f64).  Unnumbered addition:
                           the innovation log-likelihood of the forward pass (ste_ukf_loglik_f64,
                           ste_ukf_forward_loglik_f64).  Unnumbered addition: the posterior of the time derivative on the
                           GP path (ste_gp_predict_deriv_f64, ste_gp_predict_deriv_cov_f64).  Unnumbered addition: posterior tracks
                           sampled from the smoother (ste_urtss_sample_f64).  Unnumbered addition: path quantities of tracks on the
                           device (ste_path_metrics_f64).  Unnumbered addition: tracks on the device against a polygon
                           (ste_region_metrics_f64).  Unnumbered addition: tracks on the device on a lon / lat grid
                           (ste_grid_metrics_f64).  Unnumbered addition: pairs of tracks on the device against each other
                           (ste_encounter_metrics_f64).  Unnumbered addition: tracks on the device at given clock times
                           (ste_track_positions_f64).  Unnumbered addition: tracks on the device against fixed sites
                           (ste_site_metrics_f64).  Unnumbered addition: tracks on the device against polylines
                           (ste_line_metrics_f64).  Unnumbered addition: pairs of tracks on the device as curves
                           (ste_route_metrics_f64).  Unnumbered addition: speed made good, speed bands and stops of tracks on
                           the device (ste_speed_metrics_f64).  Unnumbered addition: errors of tracks on the device against
                           truth positions (ste_track_errors_f64).  Unnumbered addition: the values of a gridded field along
                           tracks on the device (ste_raster_metrics_f64).  Unnumbered addition: observation preparation with
                           SOG / COG smoothed first (ste_track_prep_smooth_f64).  Unnumbered addition: tracks on the device
                           simplified within a tolerance (ste_track_simplify_f64).  Unnumbered addition: measurement noise fitted
                           by EM on the device (ste_ukf_noise_moments_f64, ste_ukf_noise_mstep_f64).  Unnumbered addition: the
                           values of a space-time gridded field where tracks on the device were at given clock times
                           (ste_field_values_f64).  Unnumbered addition: the lag-one cross-covariance of the smoother and the
                           exact covariance of a position at a query time (ste_urtss_lag_one_f64, ste_track_position_cov_f64).
                           Unnumbered addition: the pair list of the encounter call found on the device
                           (ste_encounter_candidates_mask_f64, ste_encounter_candidates_list_f64).
                           0.3.3: Matern kernels (nu = 1/2, 3/2, 5/2) on the GP path (ste_gp_batch_f64.kernel, appended).
                           0.3.2: the forward passes of many windows as one scheduled launch (ste_ukf_forward_sched_f64,
                           ste_stream_wait_counter); 321: their smoothers as one launch too (ste_urtss_backward_sched_f64).  0.3.1: track_stride (windows of a resident fleet), sm_pos, forward pass in
                           time slices (step_begin / step_end).  0.3.0: rts_work rows of 30 doubles (+ B at the end); sigma
                           weights sum to one */

/* error codes */
#define STE_OK 0
#define STE_EINVAL (-1)   /* bad argument (NULL pointer, B <= 0, n != 4 ...) */
#define STE_ELAUNCH (-2)  /* HIP launch / runtime error */
#define STE_ENOGPU (-3)   /* no HIP device visible */

/* ste_ukf_batch_f64.flags */
#define STE_FLAG_SHARED_P0 0x1u        /* P0 is one 4x4 matrix [16] shared by all tracks (else [16][B]) */
#define STE_FLAG_NO_INITIAL_UPDATE 0x2u /* skip the update with z[:,0] that run() performs before the first predict */
#define STE_FLAG_LANES_1 0x10u /* forward pass with one lane per track for this call (default: chosen by batch size) */
#define STE_FLAG_LANES_4 0x20u /* forward pass with one DPP quad (4 lanes) per track for this call */
#define STE_FLAG_PACKED_COV 0x40u /* fwd_cov and sm_cov hold upper triangles, [Nmax+1][10][B] (row-major: 00 01 02 03 11 12 13
                                     22 23 33), instead of full matrices [Nmax+1][16][B]: the covariances are symmetric by
                                     construction, and 96 of the 828 bytes the two passes move per track-step go */
#define STE_FLAG_ROBUST 0x4u /* opt-in Mahalanobis robustification of every update (check_robustness, unscented.py:353-387;
                                the reference ships with its call site commented out, :228) */

#define STE_RTS_WORK_ROWS 30 /* doubles per (step, track) of ste_ukf_batch_f64.rts_work (+ one row at its end) */
#define STE_SLICE_ALIGN 64   /* time slices of the forward pass start and end on multiples of this many steps */

/* status[] bits (per track) */
#define STE_STATUS_NAN 0x1        /* a non-finite value reached the state or covariance */
#define STE_STATUS_CLAMPED 0x2    /* sigma fan: negative eigenvalue clamped to 0 (sqrtm went complex in the reference) */
#define STE_STATUS_NOCONV 0x4     /* Jacobi eigen-solve hit its sweep cap */
#define STE_STATUS_ROBUST_CAP 0x8 /* robust update: criterion still above chi_alpha after robust_max_iter rescalings */
#define STE_STATUS_HOST_INDEX 0x10 /* set by host-side packers, never by the library: the reference would raise IndexError
                                      for this track (update index past its last observation, kalman_filter.py:105) */
#define STE_STATUS_BAD_INDEX 0x20 /* upd_idx[k] >= Tmax at some step: that update was skipped (precondition below) */

/*
 * One batch of B independent tracks, padded to Nmax filter steps and Tmax observations.
 * n must be 4 (the reference hard-codes index 3 as the heading, unscented.py:250).
 */
typedef struct ste_ukf_batch_f64 {
    int32_t B;     /* number of tracks */
    int32_t Nmax;  /* padded number of filter steps (len(dt) in run()) */
    int32_t Tmax;  /* padded number of observations (columns of ShipTrack.z) */
    int32_t n;     /* state dimension, must be 4 */
    uint32_t flags;
    int32_t tuning; /* 0 = defaults.  Bit 8 (0x100): every smoother gain by the eigenvalue route (default: only where P_b is close
                       to singular).  Bits 9 / 10 (0x200 / 0x400): ste_urtss_backward_f64 in its two-kernel / one-kernel form
                       whatever the batch size (default: two kernels -- all gains at once, then a lean recurrence -- up to 4 096
                       tracks, where the smoother is a few waves running a latency chain; one kernel above; same bits either way).
                       Bit 11 (0x800): the lean recurrence of the two-kernel form with a lane per track instead of a DPP quad per
                       track (same bits; measurements).  Must not change between the backward calls made on one forward result.
                       Other bits are ignored */
#define STE_TUNING_EIG_GAINS 0x100           /* bit 8: every smoother gain by the eigenvalue route */
#define STE_TUNING_TWO_KERNEL_SMOOTHER 0x200 /* bit 9: the two-kernel smoother whatever the batch size */
#define STE_TUNING_ONE_KERNEL_SMOOTHER 0x400 /* bit 10: the one-kernel smoother whatever the batch size */
#define STE_TUNING_LANE_RECURRENCE 0x800     /* bit 11: the two-kernel form's recurrence with a lane per track */

    /* sigma-fan constants, computed by the host exactly as unscented.py:95,125,132 does (HOST values) */
    double fan_scale; /* n / (1 - W0) */
    double w0;        /* 1 - n/3 */
    double wi;        /* (1 - W0) / (2n) */

    /* shared 4x4 matrices, row-major, HOST pointers read at call time (unscented.py:55-61) */
    const double* H;
    const double* Q;
    const double* R;

    /* per-track inputs (device) */
    const int32_t* nsteps; /* [B] real step count of each track (<= Nmax); NULL = every track has Nmax steps */
    const double* x0;      /* [4][B]  prior mean */
    const double* P0;      /* [16][B] prior covariance, or [16] with STE_FLAG_SHARED_P0 */

    /* per-step inputs (device) */
    const double* dt;           /* [Nmax][B]  kalman_filter.py:88 */
    const double* sog_rate;     /* [Nmax][B]  rate used by predict at step k  (kalman_filter.py:93) */
    const double* cog_rate;     /* [Nmax][B]                                   (kalman_filter.py:94) */
    const double* sog_rate_rts; /* [Nmax][B]  rate used by the smoother at step k (unscented.py:287-292,310); NULL = sog_rate */
    const double* cog_rate_rts; /* [Nmax][B]  NULL = cog_rate */
    const int32_t* upd_idx;     /* [Nmax][B]  observation column consumed after step k, -1 = no update (kalman_filter.py:101-108);
                                   must be < Tmax: a larger value skips that update and sets STE_STATUS_BAD_INDEX */
    const double* z;            /* [Tmax][4][B] measurement matrix columns (ship_track.py:324-336) */

    /* recorded noise draws, already scaled; NULL = zero noise (unscented.py:198,232,320) */
    const double* noise_pred; /* [Nmax][4][B]   added to the predicted mean of step k */
    const double* noise_upd;  /* [Nmax+1][4][B] row 0: initial update; row k+1: update after step k */
    const double* noise_rts;  /* [Nmax][4][B]   added to the back-predicted mean of step k */

    /* outputs (device) */
    double* fwd_mean; /* [Nmax+1][4][B]  row 0 = prior (kalman_filter.py:76) */
    double* fwd_cov;  /* [Nmax+1][16][B]; [Nmax+1][10][B] with STE_FLAG_PACKED_COV */
    double* sm_mean;  /* [Nmax+1][4][B]  smoothed; row nsteps = filtered row nsteps */
    double* sm_cov;   /* [Nmax+1][16][B]; [Nmax+1][10][B] with STE_FLAG_PACKED_COV */
    int32_t* status;  /* [B] OR-ed STE_STATUS_* bits; the forward pass overwrites, the backward pass ORs */

    /*
     * Optional workspace of (Nmax * STE_RTS_WORK_ROWS + 1) * B doubles (device), caller-owned.  When it is non-NULL
     * ste_ukf_forward_f64 also evaluates what the smoother's step k needs of the sigma
     * fan of the filtered state of step k (unscented.py:297-330: back-prediction x_b, P_b, cross-covariance D) while it has
     * that fan in registers, and stores it here: row k = columns 0-1 of D (8) | x_b (4) | P_b upper triangle (10) |
     * columns 2-3 of D (8), each [B].  x_b and P_b are written only for the steps where they do not follow from rows k and
     * k + 1 of the filtered history (steps followed by an update, row 0 of a run that starts with one, runs with recorded
     * noise); columns 2-3 of D only at and after a track's first clamped / unconverged square root (elsewhere they are
     * 2 wi fan_scale times columns 2-3 of the filtered covariance); the last B words hold that step index per track.
     * ste_urtss_backward_f64 on the same batch then forms the gains K = D pinv(P_b) (:333) and runs the recurrence
     * (:337-349); it may be called again on the same forward result (the one-kernel form only reads the workspace; the
     * two-kernel form of small batches rewrites rows into gains once and marks the workspace as such).  Results are those
     * of the stand-alone smoother to rounding.  Smoother rates of its own (sog_rate_rts / cog_rate_rts) are no obstacle:
     * speed and heading pass through the process model as x + rate * dt, so they move x_b[2:4] -- and through it P_b,
     * which is taken about the filtered mean -- by a known amount and leave D alone.
     * NULL = the smoother recomputes everything from fwd_mean / fwd_cov (required when the forward history was not
     * produced by ste_ukf_forward_f64 on this batch).
     */
    double* rts_work;

    /* robust update (STE_FLAG_ROBUST): threshold chi_alpha (the reference hard-codes 50) and iteration cap (0 = 50) */
    double chi_alpha;
    int32_t robust_max_iter;
    int32_t reserved2;

    /* ---- 0.3.1 ---------------------------------------------------------------------------------------------------
     * A WINDOW of a larger resident batch ("fleet"): every per-track array above and below is addressed
     *      a[row * track_stride + t],   0 <= t < B,
     * i.e. the pointers name track 0 of the window inside arrays whose rows hold track_stride tracks.  0 = B (a batch of
     * its own).  The reference's batch dimension is its per-ship loop (examples/example_ukf_rts_smoother_batch.py:19-90);
     * windows are how a fleet of any size goes through the GPU in chip-sized pieces without copying or re-packing
     * (track_estimators.batch.run_fleet).  nsteps and status are [B] and simply point at the window's first entry; the
     * last row of rts_work (first bad step per track) sits after Nmax * STE_RTS_WORK_ROWS rows of track_stride. */
    int64_t track_stride;

    /* Optional output [Nmax+1][2][track_stride]: smoothed longitude / latitude, written by the smoother beside sm_mean
     * (rows 0 .. nsteps of every track; rows past a short track's end are left alone).  This is the tensor
     * BASELINE configs[2] exchanges between GPUs: with it the all-gather sends the smoother's own output. */
    double* sm_pos;

    /* The forward pass in time slices: ste_ukf_forward_f64 runs steps [step_begin, step_end) of every track (step_end = 0
     * means Nmax).  Both must be multiples of STE_SLICE_ALIGN (or 0 / Nmax); a call with step_begin = 0 starts from the
     * prior, a later one from history row step_begin, which the previous call left -- slices must therefore be issued in
     * order (one stream, or the caller's own ordering).  Histories, work rows and status are bit-identical to those of one
     * call over [0, Nmax): at multiples of STE_SLICE_ALIGN the warm start of the fan's eigen-solve restarts in a whole
     * pass too, so the history row is the complete filter state and only the launch boundary moves.  With the quad
     * mapping (STE_FLAG_LANES_4 or a small batch) slices need full covariance histories (no STE_FLAG_PACKED_COV).  The
     * smoother is not sliced.  What this is for: a forward launch is one indivisible wave per 64 tracks for the whole
     * pass; in slices, the waves of several batches re-balance over the chip at every boundary. */
    int32_t step_begin;
    int32_t step_end;
} ste_ukf_batch_f64;

int ste_version(void);

/* Thread-local message of the last failing call on this thread; valid until the next call on this thread. */
const char* ste_last_error(void);

/* Number of HIP devices visible (0 if none / runtime unavailable). Does not select a device. */
int ste_device_count(void);

/* Forward UKF over all steps of every track: writes fwd_mean, fwd_cov, status. */
int ste_ukf_forward_f64(const ste_ukf_batch_f64* b, void* stream);

/*
 * Innovation log-likelihood of the forward pass (the prediction-error decomposition), per track.  For every measurement
 * update the pass performs -- the initial one at z[:, 0] unless STE_FLAG_NO_INITIAL_UPDATE, then one per upd_idx[k] >= 0 --
 * with x-, P- the state it starts from (the predicted one, recorded noise_pred included; the prior for the initial update),
 * z its observation column (+ noise_upd), R_u its R (rescaled under STE_FLAG_ROBUST):
 *      S = H P- H^T + R_u,   y = z - H x-  with y[3] wrapped to [-180, 180) as the update wraps it,
 *      S^+ the update's own pseudo-inverse, keeping the r eigenvalues lambda_i with |lambda| > 1e-15 max |lambda|,
 *      nis_u = y^T S^+ y,    l_u = -1/2 (nis_u + sum_i log lambda_i + r log 2 pi)
 * l_u is the Gaussian log density of the part of y in the range of S (the part in its null space enters neither the gain
 * nor l_u; for H = diag(1, 1, 0, 0) that is y[2], y[3] and r = 2).  A kept eigenvalue <= 0 makes l_u NaN; a non-finite
 * observation that makes the update's state NaN makes the track's loglik NaN too.  r is the pseudo-inverse's own count: a NaN
 * eigenvalue (an S that is not finite, e.g. every update after such an observation) is not inverted, so it adds nothing to
 * dof, while the update still counts in nupd and its l_u is NaN.
 * Output arrays are indexed like status and nsteps: a window's pointers name its first track, rows hold track_stride.
 */
typedef struct ste_ukf_loglik_f64 {
    double*  loglik; /* [B] out, required: sum of l_u over the track's updates */
    int32_t* dof;    /* [B] out or NULL: sum of the ranks r (NaN eigenvalues not counted, see above) */
    int32_t* nupd;   /* [B] out or NULL: updates summed */
    double*  nis;    /* [Nmax+1][track_stride] out or NULL: nis_u of the update that produced history row k; NaN in rows
                        0..nsteps[t] without an update; rows past nsteps[t] are not written */
} ste_ukf_loglik_f64;

/* The forward pass of ste_ukf_forward_f64 with the lane-per-track mapping, plus the innovation log-likelihood above.
 *   - fwd_mean and fwd_cov both non-NULL: everything else the call writes (histories, rts_work, status) is bit-identical to
 *     ste_ukf_forward_f64 with flags | STE_FLAG_LANES_1, and ste_urtss_backward_f64 may follow it unchanged.
 *   - both NULL: the likelihood alone (no history is written; rts_work must be NULL).  One such call per candidate (Q, R)
 *     scores the candidates over a whole fleet (track_estimators.batch.log_likelihood_grid).
 * Recorded noise, STE_FLAG_ROBUST, STE_FLAG_NO_INITIAL_UPDATE, STE_FLAG_SHARED_P0, STE_FLAG_PACKED_COV, ragged nsteps and
 * windows are accepted.  Refused with STE_EINVAL before any launch: STE_FLAG_LANES_4, time slices (step_begin != 0 or
 * step_end not in {0, Nmax}), l or l->loglik NULL, exactly one of fwd_mean / fwd_cov NULL, rts_work without histories,
 * and whatever ste_ukf_forward_f64 refuses. */
int ste_ukf_forward_loglik_f64(const ste_ukf_batch_f64* b, const ste_ukf_loglik_f64* l, void* stream);

/*
 * Per-track process and measurement noise.  In the reference every ship has a filter object of its own
 * (UnscentedKalmanFilter(H=H, Q=Q, R=R, ...) inside the per-ship loop, examples/example_ukf_rts_smoother_batch.py:46-64,
 * unscented.py:55-61), so Q and R are per-track quantities there; the batch struct carries one shared pair.  This struct
 * travels beside it (an unnumbered addition, like ste_ukf_loglik_f64) and gives track t its own matrices:
 *   - Track t of a window reads Q[e * track_stride + t] (R likewise): the pointers name the window's first track, like every
 *     other per-track array.  Only the upper triangle exists, so the matrices are symmetric by construction.  b->H stays
 *     shared; b->Q / b->R are still required and are what a NULL member falls back on.
 *   - Route.  The closed-form update is taken when b->H == diag(1, 1, 0, 0) and R is confined to the leading 2 x 2 block: for a
 *     shared R (nz->R NULL) as in the plain calls, from b->R; for a per-track R when STE_NOISE_R_BLOCK2 is set -- the library
 *     cannot look into device memory before a launch, so this is the caller's promise (track_estimators.batch checks it when
 *     it packs).  With the promise the kernels read entries 00, 01, 11 of R only.  Without it every track takes the general
 *     4 x 4 route (where the pseudo-inverse's 2 x 2 shortcut is decided per track, not per wave, and taken only for an S
 *     that is exactly confined to the block; a non-finite S goes the 4 x 4 way, as in a shared launch with a general R).
 *   - The result for a track is the result of the plain call on a batch whose shared Q / R are that track's matrices, bit for
 *     bit, given the same route, the lane-per-track mapping and the same flags / tuning: histories, rts_work, status, sm_mean,
 *     sm_cov, sm_pos, and loglik / dof / nupd / nis.  A track's results do not depend on the other tracks' matrices.
 *   - Accepted: everything ste_ukf_forward_loglik_f64 accepts (recorded noise, STE_FLAG_ROBUST, STE_FLAG_NO_INITIAL_UPDATE,
 *     STE_FLAG_SHARED_P0, STE_FLAG_PACKED_COV, ragged nsteps, windows, the likelihood without histories), plus time slices
 *     (step_begin / step_end) when l == NULL; every smoother form ste_urtss_backward_f64 can pick (stand-alone without
 *     rts_work, one kernel from rts_work, two kernels with the quad or the lane recurrence -- tuning bits 0x200 / 0x400 /
 *     0x800 -- and smoother rates of their own).
 *   - Refused with STE_EINVAL and a message before any launch: nz NULL; nz->Q and nz->R both NULL (that is the plain call);
 *     STE_FLAG_LANES_4 (the quad forward kernel has no per-track noise; without a lane flag the call takes the lane-per-track
 *     mapping whatever the batch size, as the likelihood call does); unknown bits in nz->flags; and whatever the underlying
 *     plain call refuses.  The scheduled launches (ste_ukf_forward_sched_f64, ste_urtss_backward_sched_f64) have no
 *     per-track form.
 */
#define STE_NOISE_R_BLOCK2 0x1u /* caller's promise: every track's R is zero outside its leading 2 x 2 block */

typedef struct ste_ukf_noise_f64 {
    const double* Q;  /* DEVICE [10][track_stride]: upper triangles, row-major 00 01 02 03 11 12 13 22 23 33 (the order of
                         STE_FLAG_PACKED_COV), track index fastest; NULL = the batch's shared Q for every track */
    const double* R;  /* the same for R; NULL = the batch's shared R */
    uint32_t flags;   /* STE_NOISE_* */
    uint32_t reserved;
} ste_ukf_noise_f64;   /* 24 bytes */

/* ste_ukf_forward_f64 (l == NULL) or ste_ukf_forward_loglik_f64 (l != NULL) with track t using its own Q / R */
int ste_ukf_forward_noise_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_ukf_loglik_f64* l, void* stream);
/* ste_urtss_backward_f64 with track t's own Q (the smoother never reads R; nz->R is ignored) */
int ste_urtss_backward_noise_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, void* stream);
/* both, back to back on one stream */
int ste_ukf_urtss_noise_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, void* stream);

/*
 * Posterior TRACKS from the unscented smoother (an unnumbered addition, like ste_ukf_noise_f64).  sm_mean / sm_cov are the
 * marginals of every row; what carries a track's uncertainty into something downstream (distance sailed, the time of a
 * crossing) are whole tracks drawn from the joint posterior, in which neighbouring rows are tied together by the smoother
 * gains.  Backward simulation with the smoother's own per-step quantities (unscented.py:297-349; m_k, P_k the filtered row k,
 * x_b, P_b -- about the filtered mean, as there -- and K = D pinv(P_b) of step k), for a track of ns steps:
 *      row ns:  x_ns = m_ns + T_ns xi_ns,                                        T_ns = symsqrt(P_ns)
 *      row k :  y = x_{k+1} - x_b,  y[3] wrapped to [-180, 180);   x_k = (m_k + K y) + T_k xi_k,   T_k = symsqrt(P_k - K P_b K^T)
 *      x_k[3] = x_k[3] mod 360 (floored), row ns included
 * xi are the caller's standard normal draws; symsqrt is the symmetric square root of the sigma fan (eigenvalues below zero
 * clamped), which exists where the conditional covariance is only semi-definite (a Q with zero directions).  With xi = 0
 * the samples are sm_mean, bit for bit; the ensemble covariance of the samples is sm_cov (the recursion
 * Cov(x_k) = T_k T_k + K Cov(x_{k+1}) K^T is the smoother's own).
 *   - Precondition: a completed forward pass of this batch WITH rts_work.  The smoother may or may not have run, in either of
 *     its forms; samples are the same bits whichever state the work rows are in.  The calls only read the batch: rts_work, the
 *     histories and b->status are not written.
 *   - prepare turns the work rows into coefficients (K 16 | x_b 4 | T packed 10 per row) in `coef`; draw runs the recurrence from
 *     them and may be repeated with fresh draws; ste_urtss_sample_f64 is both.  nz: the per-track Q the forward pass ran with
 *     (NULL, or nz->Q NULL: the shared b->Q); nz->R and nz->flags are not read.
 *   - Ordering: the calls read rts_work.  A two-kernel smoother (ste_urtss_backward_f64 on a small batch) REWRITES the work rows
 *     into gains; when it runs on another stream the caller orders prepare before or after it, never beside it.
 *   - Windows: track_stride works like for every other per-track array -- samples and coef have rows of track_stride tracks
 *     and the pointers name the window's first track; status is [B] and points at the window's first entry.
 *   - Rows past nsteps[t] of samples (and of coef) are left as they were.
 *   - Refused with STE_EINVAL and a message before any launch: b, sm, sm->samples or sm->coef NULL; nsamples < 1 (or > 65535);
 *     flags != 0; rts_work, fwd_mean or fwd_cov NULL; step_begin / step_end naming a slice; and whatever
 *     ste_urtss_backward_f64 refuses (sm_mean / sm_cov NULL among it).  STE_FLAG_LANES_1 / _4 are ignored.
 */
typedef struct ste_ukf_sample_f64 {
    int32_t nsamples;  /* S >= 1 */
    uint32_t flags;    /* must be 0 */
    double* samples;   /* DEVICE [S][Nmax+1][4][track_stride]; in: N(0, 1) draws, out: sampled states */
    double* coef;      /* DEVICE workspace [Nmax+1][30][track_stride]: written by prepare, read by draw */
    int32_t* status;   /* DEVICE [B] out or NULL: overwritten by prepare with STE_STATUS_NAN (a non-finite coefficient),
                          STE_STATUS_CLAMPED (a negative eigenvalue of a conditional covariance was clamped), STE_STATUS_NOCONV */
} ste_ukf_sample_f64;  /* 32 bytes */

int ste_urtss_sample_prepare_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64* sm, void* stream);
/* the recurrence only, from a prepared coef; repeatable with fresh draws */
int ste_urtss_sample_draw_f64(const ste_ukf_batch_f64* b, const ste_ukf_sample_f64* sm, void* stream);
/* both, back to back on one stream */
int ste_urtss_sample_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_ukf_sample_f64* sm, void* stream);

/*
 * PATH QUANTITIES of tracks that stay on the device (an unnumbered addition, like ste_ukf_sample_f64): distance sailed and the
 * time at which a track first crosses a meridian or a parallel.  `states` holds S tracks per ship in the layout of the
 * sampler's output; sm_mean and fwd_mean have the layout of one sample ([Nmax+1][4][track_stride], S = 1), so the same call
 * serves a deterministic track.  Values are one or two doubles per (sample, ship): what carries a posterior over tracks into
 * a posterior over a distance or a crossing time without the samples leaving the device.
 *   - Leg.  Leg k of track t joins rows k and k + 1, for k < nsteps[t].  Its length in km is the distance ste_track_prep_f64
 *     computes for two observations under the same `model`: haversine on the 6378.137 km sphere (STE_PREP_SPHERE) or the
 *     WGS84 geodesic by Karney's algorithm (STE_PREP_WGS84) -- the same formulas, with the heading dropped.
 *   - Distance.  dist is the sum of the legs in step order, k = 0, 1, ...: a value's bits depend on nothing but that track's
 *     rows (not on S, the window, the other outputs asked for).  cumdist row 0 is 0, row k the first k legs; dist equals
 *     cumdist row nsteps[t] bit for bit.  A track with nsteps == 0 has distance 0 and no crossing.
 *   - Offset from the line, with v = line_value[t] in degrees.  A parallel (line_axis 1): a_k = lat_k - v.  A meridian
 *     (line_axis 0): a_k = wrap180(lon_k - v), wrap180(x) = floored_mod(x + 180, 360) - 180, in [-180, 180).
 *   - Crossing.  Step k crosses when (a_k < 0) != (a_{k+1} < 0); for a meridian also |a_{k+1} - a_k| < 180 must hold, which
 *     excludes passing the antipodal meridian.  ncross counts the crossing steps.
 *   - Crossing time.  cross_time is that of the FIRST crossing step k, in hours from row 0: T_k + dt_k a_k / (a_k - a_{k+1}),
 *     T_k the in-order sum dt_0 + ... + dt_{k-1} of that track; NaN when no step crosses.
 *   - Non-finite values.  A NaN coordinate makes dist (and cumdist from that leg on) NaN and counts as no crossing: a step
 *     with a non-finite offset at either end does not cross.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch, dt only when a line
 *     is given, and writes nothing of the batch.  Per-track arrays are addressed a[row * track_stride + t] with the pointers
 *     naming the window's first track, like the sampler's; nsteps and line_value point at the window's first entry.
 *   - Rows past nsteps[t] of states are not read; rows past nsteps[t] of cumdist are not written.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or pm NULL; states NULL; nstates < 1 or
 *     > 65535; an unknown model; line_axis outside {-1, 0, 1}; reserved != 0; a line without line_value or without b->dt;
 *     cross_time or ncross given without a line; every output NULL; B <= 0, Nmax < 0, or track_stride non-zero and below B.
 */
typedef struct ste_path_f64 {
    int32_t nstates;          /* S >= 1 tracks per ship in `states` */
    int32_t model;            /* STE_PREP_SPHERE or STE_PREP_WGS84: the leg function of ste_track_prep_f64 */
    const double* states;     /* DEVICE [S][Nmax+1][4][track_stride]; only components 0 (lon) and 1 (lat) are read */
    double* dist;             /* DEVICE [S][track_stride] out or NULL: km along rows 0..nsteps[t] */
    double* cumdist;          /* DEVICE [S][Nmax+1][track_stride] out or NULL: row 0 = 0, row k = first k legs; rows past nsteps[t] untouched */
    int32_t line_axis;        /* -1 = no line; 0 = a meridian (lon = line_value[t]); 1 = a parallel (lat = line_value[t]) */
    int32_t reserved;         /* must be 0 */
    const double* line_value; /* DEVICE [track_stride], degrees, per track; required when line_axis >= 0 */
    double* cross_time;       /* DEVICE [S][track_stride] out or NULL: hours from row 0 to the FIRST crossing, NaN = none */
    int32_t* ncross;          /* DEVICE [S][track_stride] out or NULL: number of crossing steps */
} ste_path_f64;               /* 64 bytes */

int ste_path_metrics_f64(const ste_ukf_batch_f64* b, const ste_path_f64* pm, void* stream);

/*
 * REGIONS: tracks that stay on the device against a polygon (an unnumbered addition, like ste_path_f64): the time a track
 * spends inside, when it first enters, how often it enters, the distance it sails inside and the inside flag of every row.
 * `states` is that of ste_path_f64.  The geometry is PLANAR in (lon, lat) degrees -- what a GeoJSON or shapefile polygon means --
 * and a position is linear in time inside a step, the convention of cross_time above.
 *   - Polygon.  V vertices, px[0..V) then py[0..V); edge i joins vertex i and vertex (i + 1) mod V.  Preconditions the library
 *     cannot check (the vertices are device memory; the Python front end checks them): the polygon is simple and
 *     counter-clockwise (signed area > 0), every coordinate is finite, every px lies within lon_ref +- 90.  bbox is the min / max
 *     of px and of py.
 *   - Unwrapping.  Row k sits at x_k = lon_ref + wrap180(lon_k - lon_ref), y_k = lat_k, wrap180 that of ste_path_f64.  Step k
 *     (k < nsteps[t]) runs from A = (x_k, y_k) to B = (x_k + delta, y_{k+1}), delta = wrap180(lon_{k+1} - lon_k).  Step k is
 *     BROKEN when |delta| < 90 is false or either latitude is not finite; every other step is sound.  With |delta| < 90 and a
 *     polygon within lon_ref +- 90 no periodic copy of the polygon can be met, so one copy is exact and stored longitudes may be
 *     wrapped or unwrapped.
 *   - Row inside.  A row whose (x, y) is not within bbox (closed comparisons, so NaN is outside) is outside.  Otherwise the
 *     even-odd ray test: edge i, from P = vertex i to Q = vertex i + 1, toggles when (P.y > y) != (Q.y > y) and
 *     x < P.x + (y - P.y) * (Q.x - P.x) / (Q.y - P.y).
 *   - Step fraction f of a sound step, i0 the inside flag of row k.  If the step's bounding box and bbox are disjoint (strict
 *     comparisons) f = i0 and there are no crossings.  Otherwise, for every edge in index order, with d = B - A, e = Q - P,
 *     w = P - A:  den = d.x e.y - d.y e.x,  u = (w.x e.y - w.y e.x) / den,  v = (w.x d.y - w.y d.x) / den.  A CROSSING exists
 *     when den != 0, 0 <= u < 1 and 0 <= v < 1; it is ENTERING when den < 0 and leaving otherwise.  Starting from i0, every
 *     entering crossing adds 1 - u and every leaving one subtracts it, in edge order; f is the result clamped to [0, 1].  No
 *     crossing is sorted.
 *   - Outputs, with T_k = dt_0 + ... + dt_{k-1} summed in order.  time_inside = sum of dt_k f_k over the sound steps, in step
 *     order.  dist_inside = sum of leg_k f_k over the sound steps with f_k > 0, in step order, leg_k the leg of
 *     ste_path_metrics_f64 for `model`.  ENTERING EVENTS are: row 0 inside, at time 0; every entering crossing of a sound step,
 *     at T_k + dt_k u; for a broken step, row k + 1 inside while row k is not, at T_{k+1}.  nenter counts them; first_entry is
 *     the earliest (within a step: T_k + dt_k times the smallest u), NaN when there is none.  nbroken counts the broken steps;
 *     a broken step adds nothing to time_inside or dist_inside.  inside holds the flags of rows 0 .. nsteps[t].  A track with
 *     nsteps == 0 gives 0, (0 or NaN), (1 or 0), 0, 0.
 *   - Every value's bits depend on that track's rows and the polygon alone: not on S, the window, track_stride, or which
 *     outputs were asked for.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_path_metrics_f64 (inside: inside[(s * (Nmax + 1) + row) * track_stride
 *     + t], one byte each).  Rows past nsteps[t] of states are not read.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or rg NULL; states or vert NULL; nstates < 1
 *     or > 65535; nvert < 3 or > STE_REGION_MAX_VERT; reserved != 0; a non-finite lon_ref; dist_inside with an unknown model;
 *     b->dt NULL when time_inside or first_entry is asked for; every output NULL; B <= 0, Nmax < 0, or track_stride non-zero
 *     and below B.
 */
#define STE_REGION_MAX_VERT 1024
typedef struct ste_region_f64 {
    int32_t nstates;        /* S >= 1 tracks per ship in `states` (<= 65535) */
    int32_t model;          /* STE_PREP_SPHERE / STE_PREP_WGS84: leg function for dist_inside; read only when dist_inside != NULL */
    const double* states;   /* DEVICE [S][Nmax+1][4][track_stride]; components 0 (lon) and 1 (lat) are read */
    int32_t nvert;          /* V, 3 <= V <= STE_REGION_MAX_VERT (1024) */
    int32_t reserved;       /* must be 0 */
    const double* vert;     /* DEVICE [2][V]: px[0..V), py[0..V) in degrees, shared by all tracks of the call */
    double lon_ref;         /* HOST value: the meridian the longitudes are unwrapped about (above) */
    double* time_inside;    /* DEVICE [S][track_stride] out or NULL: hours */
    double* first_entry;    /* DEVICE [S][track_stride] out or NULL: hours from row 0, NaN = never inside */
    int32_t* nenter;        /* DEVICE [S][track_stride] out or NULL */
    int32_t* nbroken;       /* DEVICE [S][track_stride] out or NULL */
    double* dist_inside;    /* DEVICE [S][track_stride] out or NULL: km sailed inside */
    uint8_t* inside;        /* DEVICE [S][Nmax+1][track_stride] out or NULL: 1 = row inside; rows past nsteps[t] untouched */
} ste_region_f64;           /* 88 bytes */

int ste_region_metrics_f64(const ste_ukf_batch_f64* b, const ste_region_f64* rg, void* stream);

/*
 * GRIDS: tracks that stay on the device on a regular lon / lat grid (an unnumbered addition, like ste_region_f64): the time
 * spent in every cell, SUMMED OVER THE TRACKS of the call, and how often a cell is entered.  `states` is that of ste_path_f64.
 * The geometry is PLANAR in (lon, lat) degrees and a position is linear in time inside a step, as for ste_region_f64.
 *   - Ticks.  Time is counted in integer ticks of 1 / STE_GRID_TICKS_PER_HOUR hours (2^-20 h = 3.4 ms).  Integer sums are exact
 *     and do not depend on the order of the additions, so the grid's bits do not depend on S, windows, sample chunks or launch
 *     order, which no floating-point sum over tracks could offer.  `ticks` and `entries` are ACCUMULATED (+=) with atomic
 *     adds: the caller zeroes them, and the grid after two calls is the sum of the grids of each.
 *   - Grid.  Cell (ix, iy), 0 <= ix < nx, 0 <= iy < ny, is [lon0 + ix dlon, lon0 + (ix + 1) dlon) x [lat0 + iy dlat,
 *     lat0 + (iy + 1) dlat), stored at [iy * nx + ix].  A position's grid coordinates are gx = (x - lon0) / dlon and
 *     gy = (lat - lat0) / dlat, and it lies in cell (floor gx, floor gy).  Without STE_GRID_PERIODIC_LON the grid must lie
 *     within lon_ref +- 90 (so it is at most 180 degrees wide and one copy of it is exact, by the argument of ste_region_f64);
 *     everything off the grid is one OUTSIDE cell.  With STE_GRID_PERIODIC_LON the grid is exactly 360 degrees wide
 *     ((double)nx * dlon == 360), the column is floor gx modulo nx (floored), and lon0 must lie within lon_ref +- 360.
 *   - Unwrapping.  Row k sits at x_k = lon_ref + wrap180(lon_k - lon_ref), wrap180 that of ste_path_f64.  Step k (k <
 *     nsteps[t]) runs from A = (x_k, lat_k) to B = (x_k + delta, lat_{k+1}), delta = wrap180(lon_{k+1} - lon_k).  Step k is
 *     SOUND when |delta| < 90, both latitudes are finite, dt_k >= 0 and dt_k * 2^20 < 2^52; every other step is BROKEN: it is
 *     counted in nbroken and adds no time anywhere.
 *   - Pieces.  A sound step has dtq = rint(dt_k * 2^20) ticks (rint: to nearest, ties to even).  It is split at the grid lines
 *     strictly between its ends: the x-lines i with parameter u = (i - gxA) / (gxB - gxA) and the y-lines j with
 *     u = (j - gyA) / (gyB - gyA), each u clamped to [0, 1], each set in the order met and the two merged by u, ties to x.  Without the
 *     periodic flag only the grid's own lines 0 .. nx (and always 0 .. ny) are taken: that is the clipping.  The line at u has
 *     the tick tq = max(rint(u * dtq), the previous line's tick); a piece is the difference of the ticks of its two ends (0 at
 *     the start, dtq at the end), so the pieces of a step sum to dtq exactly.  The first piece lies in the cell of A (indices
 *     clamped to -1 .. n, the outside, where not periodic); crossing x-line i eastwards leads to column i, westwards to i - 1,
 *     and likewise for rows.  A piece of 0 ticks is dropped.
 *   - Runs.  A track's RUN is a maximal stretch of consecutive pieces in one cell (or outside), across steps and across
 *     broken steps.  Each run adds its ticks to ticks[cell] once and 1 to entries[cell]; outside runs add to outside[s][t].
 *     total[s][t] is the sum of dtq over the sound steps.  EXACTLY: the track's ticks on the grid + outside = total.
 *     A track with nsteps == 0 adds nothing and gives 0, 0, 0.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_region_metrics_f64.  Rows past nsteps[t] of states are not read.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or g NULL; states NULL; nstates < 1 or
 *     > 65535; unknown flag bits; nx or ny < 1 or nx * ny > STE_GRID_MAX_CELLS; a non-finite lon0, lat0 or lon_ref; dlon or
 *     dlat not finite or < 1e-6; STE_GRID_PERIODIC_LON with (double)nx * dlon != 360 or with lon0 outside lon_ref +- 360;
 *     without the flag a grid that is not within lon_ref +- 90 (lon0 - lon_ref >= -90 and (lon0 + nx * dlon) - lon_ref <= 90);
 *     b->dt NULL; every output NULL; B <= 0, Nmax < 0, or track_stride non-zero and below B.
 */
#define STE_GRID_TICKS_PER_HOUR 1048576   /* 2^20: one tick = 3.4 ms */
#define STE_GRID_MAX_CELLS (1 << 26)
#define STE_GRID_PERIODIC_LON 0x1u        /* nx * dlon == 360 exactly: columns wrap */
typedef struct ste_grid_f64 {
    int32_t nstates;       /* S >= 1 tracks per ship in `states` (<= 65535) */
    uint32_t flags;        /* STE_GRID_* ; unknown bits refused */
    const double* states;  /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 / ste_region_f64 */
    int32_t nx, ny;        /* columns (lon) and rows (lat), >= 1, nx * ny <= STE_GRID_MAX_CELLS */
    double lon0, lat0;     /* HOST: west and south edge of cell (0, 0), degrees */
    double dlon, dlat;     /* HOST: cell size, finite, >= 1e-6 */
    double lon_ref;        /* HOST: meridian the longitudes are unwrapped about */
    int64_t* ticks;        /* DEVICE [ny][nx], ACCUMULATED (+=): the caller zeroes it; or NULL */
    int64_t* entries;      /* DEVICE [ny][nx], accumulated: runs of a track in the cell; or NULL */
    int64_t* outside;      /* DEVICE [S][track_stride] out or NULL: ticks of sound steps spent off the grid */
    int64_t* total;        /* DEVICE [S][track_stride] out or NULL: ticks of all sound steps */
    int32_t* nbroken;      /* DEVICE [S][track_stride] out or NULL */
} ste_grid_f64;            /* 104 bytes */

int ste_grid_metrics_f64(const ste_ukf_batch_f64* b, const ste_grid_f64* g, void* stream);

/*
 * ENCOUNTERS: PAIRS of tracks that stay on the device against each other (an unnumbered addition, like ste_grid_f64): how close
 * two ships came and when, and for how long, from when and how often they were within R km of each other.  `states` is that of
 * ste_path_f64; sample s of ship i is held against sample s of ship j.  Every ship has its own dt, so the two are walked on a
 * common clock.  A position is linear in time inside a step, in planar (lon, lat), and a step is broken by the rule of
 * ste_region_f64.  Below clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x), max(x, y) = x > y ? x : y, min(x, y) = x < y ? x : y, and
 * every expression is evaluated as written, left to right, without contraction.
 *   - Clock.  Track t has knots tau_t[k] = t0[t] + T_k, T_0 = 0, T_{k+1} = T_k + dt_k summed in order; the single addition of
 *     t0 is made at use.  t0 NULL is 0 for every track.
 *   - Walk.  For pair (i, j), ns_i = nsteps[i], ns_j = nsteps[j]: start with a = b = 0 and repeat while a < ns_i and b < ns_j:
 *     lo = max(tau_i[a], tau_j[b]), ea = tau_i[a+1], eb = tau_j[b+1], hi = min(ea, eb).  If hi > lo the PIECE (a, b, lo, hi) is
 *     examined.  Then a advances if ea <= eb and b advances if eb <= ea (both on a tie).  Pieces are examined in this order,
 *     which defines "first" below.
 *   - Bad clock.  A pair has a bad clock when t0 of either ship is not finite (checked before the walk: no comparison of the
 *     walk would be true and it would not end) or when a dt the walk reads -- dt_a of ship i and dt_b of ship j at the top of
 *     a repetition -- is not finite and >= 0.  A bad clock sets STE_ENC_BAD_TIME in status, ends the walk and gives min_dist,
 *     min_time and first_within = NaN and zero for every other output.
 *   - Bad index.  An index outside [0, B) sets STE_ENC_BAD_INDEX and gives the outputs of a bad clock; nothing of that pair is
 *     read.  A pair with i == j is valid and gives distance 0.
 *   - Soundness.  A step of a ship is BROKEN when |delta| < 90 is false, delta = wrap180(lon_{k+1} - lon_k), or either of its
 *     latitudes is not finite.  A piece on a broken step of either ship adds 1 to nbroken and nothing else, and closes an open
 *     run.  Every other piece is SOUND.
 *   - Positions in a piece.  Ship i on step a, dt = dt_a: u0 = clamp01((lo - tau_i[a]) / dt), u1 = clamp01((hi - tau_i[a]) / dt),
 *     x(u) = lon_a + u * delta, y(u) = lat_a + u * (lat_{a+1} - lat_a); (xi0, yi0) at u0 and (xi1, yi1) at u1.  Ship j on
 *     step b likewise.
 *   - Relative motion.  gx0 = wrap180(xj0 - xi0), gy0 = yj0 - yi0, gx1 = gx0 + ((xj1 - xj0) - (xi1 - xi0)) (continuous, never
 *     re-wrapped), gy1 = yj1 - yi1.  c = cos(0.25 * ((yi0 + yi1) + (yj0 + yj1)) * kDeg2Rad), Kd = 6378.137 * kDeg2Rad (one
 *     double), kc = Kd * c.  r0 = (kc * gx0, Kd * gy0), r1 = (kc * gx1, Kd * gy1), d = r1 - r0, dd = d.x * d.x + d.y * d.y,
 *     bq = r0.x * d.x + r0.y * d.y, r00 = r0.x * r0.x + r0.y * r0.y.  cos is the only operation here whose bits may differ
 *     between implementations.
 *   - Closest approach.  u* = dd > 0 ? clamp01(-bq / dd) : 0, m = (r0.x + u* * d.x, r0.y + u* * d.y), q = m.x * m.x + m.y * m.y.
 *     The piece becomes the best one when q < best_q (best_q starts at +inf; strict, so the first piece wins a tie).  It then
 *     records min_time = lo + u* * (hi - lo) and the two positions (xi0 + u* * (xi1 - xi0), yi0 + u* * (yi1 - yi0)) and likewise
 *     for j.  After the walk min_dist is the leg of ste_path_metrics_f64 for `model` between those two positions (NaN when a
 *     coordinate is not finite): the leg function runs once per (sample, pair).  Without a best piece min_dist and min_time
 *     are NaN.
 *   - Within R, R = radius_km.  If dd > 0: disc = bq * bq - dd * (r00 - R * R), and if disc >= 0: sq = sqrt(disc),
 *     ua = max((-bq - sq) / dd, 0), ub = min((-bq + sq) / dd, 1).  If dd == 0: ua = 0, ub = 1 iff r00 <= R * R.  Otherwise
 *     there is no interval.  If ub > ua: time_within += (ub - ua) * (hi - lo); a new RUN starts unless the run is open and
 *     ua == 0; a new run adds 1 to nwithin and the first one sets first_within = lo + ua * (hi - lo); after that the run is open
 *     iff ub == 1.  A piece without an interval, a broken piece and the end of the walk close the run.  No tolerance anywhere.
 *   - Overlap.  overlap is the sum of hi - lo over the sound pieces, in piece order.
 *   - Accuracy.  The planar metric is for ships close together: its relative error is about tan(lat) times half the latitude
 *     change over a piece (radians) plus (separation / 6378 km)^2.  On the test fleet (steps of about 0.1 degrees at 50 N,
 *     separations up to 90 km) sqrt(q) and min_dist differ by up to 1.6e-3 relative.  min_dist is a true distance (of `model`)
 *     at the time the planar distance is least; time_within, first_within and nwithin are planar, hence the limit on
 *     radius_km.
 *   - Every value's bits depend on the two tracks' rows, their dt, t0 and R alone: not on S, P, the place of the pair in the
 *     list, the window, or which outputs were asked for.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_path_metrics_f64, t0 like nsteps, pair indices count from the
 *     window's first track.  Rows past nsteps[t] of states are not read.  Outputs per pair are out[s * P + p]; status[p].
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or en NULL; states or pairs NULL; nstates < 1
 *     or > 65535; npairs < 1 or > STE_ENCOUNTER_MAX_PAIRS; an unknown model when min_dist is asked for; radius_km not finite,
 *     < 0 or > STE_ENCOUNTER_MAX_RADIUS_KM; flags or reserved non-zero; b->dt NULL; every output NULL; B <= 0, Nmax < 0, or
 *     track_stride non-zero and below B.
 */
#define STE_ENCOUNTER_MAX_PAIRS (1 << 26)
#define STE_ENCOUNTER_MAX_RADIUS_KM 1000.0
#define STE_ENC_BAD_INDEX 0x1  /* a pair index outside [0, B): nothing of that pair is read */
#define STE_ENC_BAD_TIME  0x2  /* a non-finite t0, or a dt met by the walk that is not finite and >= 0 */
typedef struct ste_encounter_f64 {
    int32_t nstates;       /* S >= 1 (<= 65535); sample s of ship i is held against sample s of ship j */
    int32_t model;         /* STE_PREP_SPHERE / STE_PREP_WGS84: leg function for min_dist only */
    const double* states;  /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 */
    int64_t npairs;        /* P, 1 .. STE_ENCOUNTER_MAX_PAIRS */
    const int32_t* pairs;  /* DEVICE [P][2]: (i, j), tracks of the window, 0 <= i, j < B */
    const double* t0;      /* DEVICE [track_stride] or NULL (= 0): clock time of row 0 of each track, hours */
    double radius_km;      /* HOST: R, finite, 0 <= R <= STE_ENCOUNTER_MAX_RADIUS_KM */
    uint32_t flags;        /* must be 0 */
    uint32_t reserved;     /* must be 0 */
    double* min_dist;      /* DEVICE [S][P] or NULL: km at the closest approach, NaN = no sound piece */
    double* min_time;      /* DEVICE [S][P] or NULL: its clock time, hours; NaN likewise */
    double* time_within;   /* DEVICE [S][P] or NULL: hours with planar distance <= R */
    double* first_within;  /* DEVICE [S][P] or NULL: clock time of the first run within R, NaN = none */
    int32_t* nwithin;      /* DEVICE [S][P] or NULL: runs within R */
    double* overlap;       /* DEVICE [S][P] or NULL: hours of sound pieces (common clock time examined) */
    int32_t* nbroken;      /* DEVICE [S][P] or NULL: pieces skipped because a step of either ship is broken */
    int32_t* status;       /* DEVICE [P] or NULL: STE_ENC_* bits (they do not depend on the sample) */
} ste_encounter_f64;       /* 120 bytes */

int ste_encounter_metrics_f64(const ste_ukf_batch_f64* b, const ste_encounter_f64* en, void* stream);

/*
 * CANDIDATES: the pair list of ste_encounter_f64, found on the device (an unnumbered addition, like ste_encounter_f64): which
 * pairs (i, j), i < j, of the tracks of a batch can have been within reach_km of each other AT ONE INSTANT.  The clock is cut
 * into windows; every track gets, per window it lives in, a box around the unit vectors of its rows; a pair is listed when
 * the two boxes of some window are closer than the chord of the reach.  `states` is ONE state set, [Nmax+1][4][track_stride]
 * (sm_mean, fwd_mean or one sample).  Below clamp(x, a, b) = x < a ? a : (x > b ? b : x), min and max as for ENCOUNTERS, and
 * every expression is evaluated as written, left to right, without contraction.
 *   - Clock.  As for ENCOUNTERS: tau_t[k] = t0[t] + T_k, T_0 = 0, T_{k+1} = T_k + dt_k summed in order; t0 NULL is 0.  A track
 *     has a BAD CLOCK when t0 is not finite or when a dt among its first nsteps is not finite and >= 0, and gets
 *     STE_CAND_BAD_TIME.  With a bad t0 it pairs with nothing (and gets no other clock bit).  A bad dt_k ENDS the track at
 *     knot k for this call: steps k and later do not exist, everything below speaks of the steps before it.  (The walk of
 *     ENCOUNTERS gives a pair nothing once it meets that dt, and a pair whose walk ends before it is met is served from the
 *     steps before it: the guarantee below has to hold for those.)
 *   - Windows.  time0, window_h = W > 0 and nwindows = NW are host values; window w covers [time0 + w W, time0 + (w + 1) W).
 *     win(x) = clamp(floor((x - time0) / W), 0, NW - 1).  Clamping merges whatever lies outside the range into the edge
 *     windows and never loses a pair; a track for which clamping changed an index of one of its knots 0 .. nsteps gets
 *     STE_CAND_CLIPPED.  win is monotone in x: if two ships are both on a step at one instant, that instant's window lies in
 *     the window ranges of both steps.
 *   - Sound steps.  The rule of ENCOUNTERS: step k is BROKEN when |wrap180(lon_{k+1} - lon_k)| < 90 is false or either of
 *     its latitudes is not finite.  Broken steps contribute nothing (a piece on one adds nothing to any within-R output of
 *     ste_encounter_metrics_f64).  A track with a finite t0 and no sound step (nsteps 0, or a bad dt_0, included) gets
 *     STE_CAND_EMPTY and pairs with nothing.
 *   - Boxes.  For (track, window w), over the sound steps k with win(tau[k]) <= w <= win(tau[k+1]): lo[3] and hi[3] are the
 *     componentwise min and max of the unit vectors (cos lat cos lon, cos lat sin lon, sin lat), angles times kDeg2Rad, of rows
 *     k and k + 1; h is the max over those steps of 0.5 * kDeg2Rad * sqrt(delta * delta + dlat * dlat), delta and dlat those
 *     of ENCOUNTERS: half the step's planar length in radians.  Every point of a step that is linear in (lon, lat) lies
 *     within that great-circle angle of one of its two rows.  Without such a step the box is EMPTY: lo = +inf, hi = -inf,
 *     h = 0.  sin and cos are the only operations whose bits may differ between implementations.
 *   - Near.  Tracks i and j are NEAR in window w when both boxes are non-empty and g2 <= c * c, with
 *     g_c = max(max(0, lo_i[c] - hi_j[c]), lo_j[c] - hi_i[c]) for c = 0, 1, 2, g2 = (g_0 * g_0 + g_1 * g_1) + g_2 * g_2,
 *     theta = min(((((reach_km / 6378.137 + m_i) + m_j) + h_i) + h_j) + 1e-7, pi), c = 2 * sin(theta / 2), and
 *     m_t = track_margin_km[t] / 6378.137 (0 when the array is NULL).  A track whose margin is negative or not finite gets
 *     STE_CAND_BAD_MARGIN and pairs with nothing.  1e-7 rad is a slack of 0.6 m for the roundings of the corners.
 *   - Output.  The pairs (i, j), i < j, that are near in at least one window, int32 [P][2] sorted by (i, j) (the order on
 *     which ste_encounter_metrics_f64 is fastest); on request per pair wfirst, the first near window, and nwin, the number of
 *     near windows: the pair can only be within reach inside those; track_status[B] with the STE_CAND_* bits.
 *   - GUARANTEE.  If ste_encounter_metrics_f64 on these states finds a sound piece of (i, j) whose TRUE angular separation
 *     at some instant is <= reach_km / 6378.137, then (i, j) is in the list: both ships are on sound steps at that instant,
 *     its window is in both steps' window ranges, each position is within h of a row inside its box, and the chord between
 *     two points is at least the gap between boxes that hold them.  Whole-track time overlap is implied and is no separate
 *     test.  The caller puts into reach_km (or track_margin_km) what the tested track does not show: the posterior spread
 *     when the list is used on samples, and the 0.2 % by which the planar distance of ENCOUNTERS may differ from the true one.
 *   - Determinism.  The list depends on the tracks' rows, dt, t0, the window parameters, the margins and reach_km alone: not
 *     on the fleet window it is read through, the stream, or an earlier call.  No atomics; every word has one writer.
 *   - Two calls and a workspace; the library never allocates.  ste_encounter_candidates_mask_f64 writes track_status and, into
 *     the workspace, the boxes, one bit per (i, j) and the number of pairs of every row.  The caller forms the exclusive
 *     prefix of those counts (row_offset, int64 [B]) and their sum P, provides pairs [P][2] and then
 *     ste_encounter_candidates_list_f64, with the same struct but for row_offset, npairs, pairs, wfirst and nwin, writes the
 *     list.  With P = 0 there is nothing to list.  The workspace holds, in this order: double boxes[NW][7][B] (lo[3], hi[3], h;
 *     only the windows wlo[t] .. whi[t] of track t are written and read), uint64 mask[B][ceil(B / 64)] (bit j % 64 of word
 *     j / 64 of row i; only words j / 64 >= i / 64 are written and read), int32 wlo[B], whi[B] (wlo > whi: the track pairs with
 *     nothing), count[B]; ste_encounter_candidates_workspace(B, nwindows) is its size in bytes, 0 for arguments out of range.
 *   - The calls read only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and write nothing of
 *     it; windows and addressing are those of ste_encounter_metrics_f64, t0, track_margin_km and track_status like nsteps;
 *     pair indices count from the window's first track.  Rows past nsteps[t] of states are not read.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or c NULL; states NULL; b->dt NULL; window_h
 *     not finite or <= 0; time0 not finite; nwindows < 1 or > STE_CANDIDATES_MAX_WINDOWS; reach_km not finite, < 0 or
 *     > STE_CANDIDATES_MAX_REACH_KM (theta reaches pi at 20 037 km, where every pair is near); flags or reserved non-zero;
 *     B <= 0 or > STE_CANDIDATES_MAX_TRACKS, Nmax < 0, track_stride non-zero and below B; workspace NULL, not aligned to 8
 *     bytes or workspace_bytes below the size above; the mask call without track_status; the list call without row_offset or
 *     pairs, or with npairs < 1 or > STE_ENCOUNTER_MAX_PAIRS.
 */
#define STE_CANDIDATES_MAX_WINDOWS 4096
#define STE_CANDIDATES_MAX_REACH_KM 20000.0
#define STE_CANDIDATES_MAX_TRACKS (1 << 20)
#define STE_CAND_BAD_TIME   0x1  /* a non-finite t0 (pairs with nothing), or a dt among the first nsteps that is not finite and
                                    >= 0 (the track ends there) */
#define STE_CAND_CLIPPED    0x2  /* a knot of the track lies outside [time0, time0 + NW W): merged into an edge window */
#define STE_CAND_EMPTY      0x4  /* a finite t0 and no sound step */
#define STE_CAND_BAD_MARGIN 0x8  /* track_margin_km[t] negative or not finite */
typedef struct ste_candidates_f64 {
    const double* states;          /* DEVICE [Nmax+1][4][track_stride]: one state set, as one sample of ste_path_f64 */
    const double* t0;              /* DEVICE [B] or NULL (= 0): clock time of row 0 of each track, hours */
    const double* track_margin_km; /* DEVICE [B] or NULL (= 0): added to the reach of every pair the track is in */
    double reach_km;               /* HOST: finite, 0 <= reach_km <= STE_CANDIDATES_MAX_REACH_KM */
    double time0;                  /* HOST: start of window 0, hours, finite */
    double window_h;               /* HOST: W, finite, > 0 */
    int32_t nwindows;              /* NW, 1 .. STE_CANDIDATES_MAX_WINDOWS */
    uint32_t flags;                /* must be 0 */
    uint32_t reserved;             /* must be 0 */
    int32_t reserved_pad;          /* not read */
    void* workspace;               /* DEVICE, 8-byte aligned, >= ste_encounter_candidates_workspace(B, nwindows) bytes */
    uint64_t workspace_bytes;
    int32_t* track_status;         /* DEVICE [B]: STE_CAND_* bits, written by the mask call */
    const int64_t* row_offset;     /* DEVICE [B]: exclusive prefix of the workspace's count[] (list call) */
    int64_t npairs;                /* P = sum of count[], 1 .. STE_ENCOUNTER_MAX_PAIRS (list call) */
    int32_t* pairs;                /* DEVICE [P][2], written by the list call */
    int32_t* wfirst;               /* DEVICE [P] or NULL: first near window (list call) */
    int32_t* nwin;                 /* DEVICE [P] or NULL: number of near windows (list call) */
} ste_candidates_f64;              /* 128 bytes */

size_t ste_encounter_candidates_workspace(int32_t B, int32_t nwindows);
int ste_encounter_candidates_mask_f64(const ste_ukf_batch_f64* b, const ste_candidates_f64* c, void* stream);
int ste_encounter_candidates_list_f64(const ste_ukf_batch_f64* b, const ste_candidates_f64* c, void* stream);

/*
 * POSITIONS: where tracks that stay on the device were AT GIVEN CLOCK TIMES (an unnumbered addition, like ste_encounter_f64):
 * longitude, latitude, speed and heading of every sample at a list of (track, time) queries, and the moments of the positions
 * OVER THE SAMPLES about an anchor, from which a caller makes a mean position and an error ellipse per query.  `states` is that
 * of ste_path_f64 and the clock that of ste_encounter_f64.  A position is linear in time inside a step, in planar (lon, lat), and
 * a step is broken by the rule of ste_region_f64.  Below clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x), wrap180 is that of
 * ste_path_f64, a % 360 is the floored modulus (NumPy's), and every expression is evaluated as written, left to right, without
 * contraction.  No operation here has bits that may differ between implementations: the library and a NumPy restatement agree
 * bit for bit.
 *   - Knots.  Track t, ns = nsteps[t]: T_0 = 0, T_{k+1} = T_k + dt_k for k < ns, summed in order.  The clock of a track is BAD when
 *     some dt_k, k < ns, is not finite and >= 0, or when t0[t] is not finite.  The call writes T_k into knots[k][t] for k <= ns
 *     (knots[k * track_stride + t]), with knots[0][t] = NaN marking a bad dt and 0 otherwise; rows past ns are left alone.  With
 *     STE_POS_REUSE_KNOTS it reads `knots` as a previous call on the same batch left them and does not read dt.
 *     tau_k = t0[t] + T_k: the single addition of t0 is made at use.  t0 NULL is 0 for every track.
 *   - Bad index.  qtrack[q] outside [0, B) sets STE_POS_BAD_INDEX; nothing of that query's track is read.
 *   - Bad time.  A bad clock or a non-finite qtime[q] sets STE_POS_BAD_TIME.
 *   - Locate, with tq = qtime[q].  (1) If tq == tau_0 the answer is ROW 0, for ns == 0 too.  (2) Otherwise, if ns == 0, or
 *     tq >= tau_0 is false, or tq <= tau_ns is false, the status is STE_POS_OUTSIDE: the call never extrapolates.  (3) Otherwise
 *     k is the smallest index in [0, ns) with tq <= tau_{k+1}; if tq == tau_{k+1} the answer is ROW k + 1.  tau is
 *     non-decreasing, so a bisection finds the k of a scan.  (4) Otherwise the query is INTERIOR to step k with
 *     u = clamp01((tq - tau_k) / (T_{k+1} - T_k)).  The divisor is the length of the step on the clock that was searched: it is
 *     dt_k rounded once (by the sum that made T_{k+1}), it is > 0 here because tau_k < tq < tau_{k+1}, and the call can form it
 *     from `knots` alone, which is what lets STE_POS_REUSE_KNOTS leave dt unread.  step[q] is the row of a knot hit or k, -1 when
 *     the query is not located; frac[q] is 0 on a knot hit or u, NaN when not located.
 *   - Knot hit on row j.  Per sample the outputs are the row itself: wrap180(lon_j), lat_j, speed_j, heading_j % 360.  A NaN
 *     stays a NaN; no step's soundness is consulted and no other row is read.
 *   - Interior.  delta = wrap180(lon_{k+1} - lon_k).  Step k is BROKEN when |delta| < 90 is false or either latitude is not
 *     finite, and then all four outputs are NaN.  Otherwise lon = wrap180(lon_k + u * delta), lat = lat_k + u * (lat_{k+1} -
 *     lat_k), speed = s_k + u * (s_{k+1} - s_k), heading = (h_k + u * wrap180(h_{k+1} - h_k)) % 360.
 *   - Not located.  A bad index, a bad time or an outside query gives NaN in every per-sample output and adds nothing to count
 *     or moments.
 *   - Moments.  For query q, for s = 0 .. S - 1 in order: dx = wrap180(lon - anchor[0][q]), dy = lat - anchor[1][q]; if both are
 *     finite, count[q] += 1 and the sums of dx, dy, dx * dx, dx * dy, dy * dy (moments[0..5)[q]) take one addition each.  The sums
 *     START FROM THE STORED VALUES and are stored once at the end, so a call with S samples equals a call with the first S1 and
 *     a call with the other S - S1 on the same accumulators, bit for bit.  The caller zeroes them before the first call.  The
 *     moments are in degrees.
 *   - Every value's bits depend on the track's rows, its dt, t0, the query and (the moments) the stored accumulators alone: not
 *     on Q, the place of the query in the list, S, the window, or which outputs were asked for.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_path_metrics_f64, t0 and the columns of knots like nsteps, qtrack counts
 *     from the window's first track.  Rows past nsteps[t] of states are not read.  Outputs per sample are out[s * Q + q].
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or po NULL; states, qtrack, qtime or knots
 *     NULL; nstates < 1 or > 65535; nqueries < 1 or > STE_POSITIONS_MAX_QUERIES; unknown flag bits; b->dt NULL without
 *     STE_POS_REUSE_KNOTS; count without moments or moments without count, or either without anchor; every output NULL; B <= 0,
 *     Nmax < 0, or track_stride non-zero and below B.
 */
#define STE_POSITIONS_MAX_QUERIES (1 << 26)
#define STE_POS_REUSE_KNOTS 0x1u /* `knots` holds what a previous call on this batch wrote: it is read, dt is not */
#define STE_POS_BAD_INDEX 0x1    /* qtrack outside [0, B): nothing of that query's track is read */
#define STE_POS_BAD_TIME  0x2    /* a non-finite t0 or qtime, or a dt of the track that is not finite and >= 0 */
#define STE_POS_OUTSIDE   0x4    /* the time lies before row 0 or after row nsteps of the track (or the track has no step) */
typedef struct ste_positions_f64 {
    int32_t nstates;        /* S >= 1 tracks per ship in `states` (<= 65535) */
    uint32_t flags;         /* STE_POS_REUSE_KNOTS; unknown bits refused */
    const double* states;   /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 */
    int64_t nqueries;       /* Q, 1 .. STE_POSITIONS_MAX_QUERIES */
    const int32_t* qtrack;  /* DEVICE [Q]: track of the window, 0 <= t < B */
    const double* qtime;    /* DEVICE [Q]: clock time, hours */
    const double* t0;       /* DEVICE [track_stride] or NULL (= 0): clock time of row 0 of each track, as ste_encounter_f64 */
    double* knots;          /* DEVICE [Nmax+1][track_stride] workspace, required, caller-owned: written, or read with the flag */
    const double* anchor;   /* DEVICE [2][Q]: lon then lat in degrees; required when count and moments are given */
    double* lon;            /* DEVICE [S][Q] or NULL: degrees in [-180, 180) */
    double* lat;            /* DEVICE [S][Q] or NULL */
    double* speed;          /* DEVICE [S][Q] or NULL: km/h */
    double* heading;        /* DEVICE [S][Q] or NULL: degrees in [0, 360] */
    int32_t* step;          /* DEVICE [Q] or NULL: row of a knot hit, or k; -1 = not located */
    double* frac;           /* DEVICE [Q] or NULL: 0 on a knot hit, or u; NaN = not located */
    int32_t* status;        /* DEVICE [Q] or NULL: STE_POS_* bits (step, frac and status do not depend on the sample) */
    int32_t* count;         /* DEVICE [Q], ACCUMULATED (+=), or NULL: samples with a finite dx and dy; with moments or not at all */
    double* moments;        /* DEVICE [5][Q], ACCUMULATED: sums of dx, dy, dx dx, dx dy, dy dy in degrees; or NULL */
} ste_positions_f64;        /* 136 bytes */

int ste_track_positions_f64(const ste_ukf_batch_f64* b, const ste_positions_f64* po, void* stream);

/*
 * SITES: tracks that stay on the device against FIXED POINTS (an unnumbered addition, like ste_positions_f64): how close every
 * ship came to every one of M sites (ports, anchorages, buoys, stations, wrecks) and when, and for how long, from when, how
 * often and for how long at a stretch it was within the site's own radius.  `states` is that of ste_path_f64.  A site is a ship
 * that does not move and has no clock: every rule below is the rule of ste_encounter_f64 specialised to that, so an encounter
 * call with one stationary one-step ship per site whose step spans every clock gives the same bits wherever no step has zero
 * length (tests/test_site_metrics.py holds the two against each other).  A position is linear in time inside a step, in planar
 * (lon, lat), and a step is broken by the rule of ste_region_f64.  Below clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x),
 * max(x, y) = x > y ? x : y, min(x, y) = x < y ? x : y, wrap180 is that of ste_path_f64, and every expression is evaluated as
 * written, left to right, without contraction.
 *   - Clock.  Track t has knots tau_k = t0[t] + T_k, T_0 = 0, T_{k+1} = T_k + dt_k summed in order; the single addition of t0 is
 *     made at use.  t0 NULL is 0 for every track.
 *   - Bad clock.  A track's clock is bad when t0[t] is not finite or when some dt_k, k < nsteps[t], is not finite or is negative.
 *     A bad clock sets STE_SITE_BAD_TIME in track_status[t] and gives min_dist, min_time and first_within = NaN and zero for
 *     every other output, for every site and sample of that track (sound_time and nbroken too).
 *   - Pieces.  Step k of track t, k < nsteps[t], is the PIECE (lo, hi) = (tau_k, tau_{k+1}).  It is examined when hi > lo: a
 *     step of zero length is skipped.  Pieces are examined in the order of k, which defines "first" below.
 *   - Soundness.  delta = wrap180(lon_{k+1} - lon_k).  The step is BROKEN when |delta| < 90 is false or either of its latitudes
 *     is not finite.  A broken examined step adds 1 to nbroken and nothing else, and closes every open run.  Every other
 *     examined step is SOUND.  sound_time is the sum of hi - lo over the sound examined steps, in order.
 *   - Bad site.  A site is bad when its lon or lat is not finite, or when its radius is not finite, is < 0 or is
 *     > STE_ENCOUNTER_MAX_RADIUS_KM.  A bad site sets STE_SITE_BAD_SITE in site_status[m] and gives min_dist, min_time and
 *     first_within = NaN and zero for time_within, longest and nwithin, for every track and sample.
 *   - Relative motion on a sound step, for the site (X, Y) with radius R.  x0 = lon_k, y0 = lat_k, x1 = x0 + delta,
 *     y1 = lat_{k+1}.  gx0 = wrap180(X - x0), gy0 = Y - y0, gx1 = gx0 - (x1 - x0) (continuous, never re-wrapped), gy1 = Y - y1.
 *     c = cos(0.25 * ((y0 + y1) + (Y + Y)) * kDeg2Rad), Kd = 6378.137 * kDeg2Rad (one double), kc = Kd * c.  r0 = (kc * gx0,
 *     Kd * gy0), r1 = (kc * gx1, Kd * gy1), d = r1 - r0, dd = d.x * d.x + d.y * d.y, bq = r0.x * d.x + r0.y * d.y,
 *     r00 = r0.x * r0.x + r0.y * r0.y.  cos is the only operation here whose bits may differ between implementations.
 *   - Closest approach.  u* = dd > 0 ? clamp01(-bq / dd) : 0, m = (r0.x + u* * d.x, r0.y + u* * d.y), q = m.x * m.x + m.y * m.y.
 *     The piece becomes the best one when q < best_q (best_q starts at +inf; strict, so the first piece wins a tie).  It then
 *     records min_time = lo + u* * (hi - lo) and the ship's position (x0 + u* * (x1 - x0), y0 + u* * (y1 - y0)).  After the last
 *     step min_dist is the leg of ste_path_metrics_f64 for `model` from that position to (X, Y): the leg function runs once per
 *     (sample, site, track).  Without a best piece min_dist and min_time are NaN.
 *   - Within R.  If dd > 0: disc = bq * bq - dd * (r00 - R * R), and if disc >= 0: sq = sqrt(disc), ua = max((-bq - sq) / dd, 0),
 *     ub = min((-bq + sq) / dd, 1).  If dd == 0: ua = 0, ub = 1 iff r00 <= R * R.  Otherwise there is no interval.  If ub > ua:
 *     time_within += (ub - ua) * (hi - lo); a new RUN starts unless the run is open and ua == 0; a new run adds 1 to nwithin and
 *     the first one sets first_within = lo + ua * (hi - lo); after that the run is open iff ub == 1.  The length of a run is the
 *     sum of (ub - ua) * (hi - lo) over its pieces, in order; longest is the largest length of a run, 0 without one.  A piece
 *     without an interval, a broken piece, a skipped piece (hi > lo false) and the end of the track close the run.  No
 *     tolerance anywhere.  (Only the skipped piece departs from ste_encounter_f64, whose walk passes over it with the run open.)
 *   - Accuracy.  That of ste_encounter_f64: the planar metric is for a ship near the site, min_dist is a true distance (of
 *     `model`) at the time the planar distance is least, the within-R outputs are planar, hence the limit on the radius.
 *   - Every value's bits depend on the track's rows, its dt and t0, and the site's three numbers alone: not on S, M, the site's
 *     place in the list, the window, or which outputs were asked for.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_path_metrics_f64, t0 and track_status like nsteps.  Rows past nsteps[t]
 *     of states are not read.  Outputs per (sample, site, track) are out[(s * M + m) * track_stride + t]; sound_time and nbroken
 *     out[s * track_stride + t] (track_stride = B where it is 0).
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or si NULL; states, sites or radius_km NULL;
 *     nstates < 1 or > 65535; nsites < 1 or > STE_SITES_MAX; an unknown model when min_dist is asked for; flags or reserved
 *     non-zero; b->dt NULL; every output NULL; B <= 0, Nmax < 0, or track_stride non-zero and below B; and a call whose
 *     ceil(B / 64) * ceil(nsites / ste_site_tile()) exceeds 2^31 - 1.
 */
#define STE_SITES_MAX 65536
#define STE_SITE_BAD_TIME 0x1  /* track_status: a non-finite t0, or a dt below nsteps that is not finite and >= 0 */
#define STE_SITE_BAD_SITE 0x1  /* site_status: a non-finite lon or lat, or a radius that is not finite, < 0 or above the limit */
typedef struct ste_site_f64 {
    int32_t nstates;         /* S >= 1 tracks per ship in `states` (<= 65535) */
    int32_t model;           /* STE_PREP_SPHERE / STE_PREP_WGS84: leg function for min_dist only */
    const double* states;    /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 */
    int32_t nsites;          /* M, 1 .. STE_SITES_MAX (four bytes of padding follow) */
    const double* sites;     /* DEVICE [2][M]: lon[0..M) then lat[0..M), degrees */
    const double* radius_km; /* DEVICE [M]: R per site, finite, 0 <= R <= STE_ENCOUNTER_MAX_RADIUS_KM, else the site is bad */
    const double* t0;        /* DEVICE [track_stride] or NULL (= 0): clock time of row 0 of each track, as ste_encounter_f64 */
    uint32_t flags;          /* must be 0 */
    uint32_t reserved;       /* must be 0 */
    double* min_dist;        /* DEVICE [S][M][track_stride] or NULL: km at the closest approach, NaN = no sound piece */
    double* min_time;        /* DEVICE [S][M][track_stride] or NULL: its clock time, hours; NaN likewise */
    double* time_within;     /* DEVICE [S][M][track_stride] or NULL: hours with planar distance <= R */
    double* first_within;    /* DEVICE [S][M][track_stride] or NULL: clock time at which the first run within R starts, NaN = none */
    double* longest;         /* DEVICE [S][M][track_stride] or NULL: hours of the longest run within R, 0 = none */
    int32_t* nwithin;        /* DEVICE [S][M][track_stride] or NULL: runs within R */
    double* sound_time;      /* DEVICE [S][track_stride] or NULL: hours of sound steps */
    int32_t* nbroken;        /* DEVICE [S][track_stride] or NULL: broken examined steps */
    int32_t* track_status;   /* DEVICE [track_stride] or NULL: STE_SITE_BAD_TIME (does not depend on the sample or the site) */
    int32_t* site_status;    /* DEVICE [M] or NULL: STE_SITE_BAD_SITE */
} ste_site_f64;              /* 136 bytes */

int ste_site_metrics_f64(const ste_ukf_batch_f64* b, const ste_site_f64* si, void* stream);
/* sites a wave holds in registers; M at and around its multiples is where the tiling of the sites shows */
int ste_site_tile(void);

/*
 * LINES: tracks that stay on the device against FIXED POLYLINES (an unnumbered addition, like ste_site_f64): how close every
 * ship came to every one of M lines (coasts, cables, planned routes, gates) and when, on which segment and where along it, and
 * how often, in which direction and when it crossed the line.  `states` is that of ste_path_f64, the clock that of
 * ste_site_f64, the frame that of ste_region_f64 (one per line) and the metric that of ste_site_f64.  The lines are a CSR list:
 * line m owns vertices first[m] .. first[m+1] - 1 of vert, L = first[m+1] - first[m] - 1 segments; segment j of the line joins
 * its vertices j and j + 1, P = vertex j and Q = vertex j + 1 below.  A position is linear in time inside a step, in planar
 * (lon, lat).  Below clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x), wrap180 is that of ste_path_f64, a . b = a.x * b.x + a.y * b.y,
 * and every expression is evaluated as written, left to right, without contraction.
 *   - Clock.  Track t has knots tau_k = t0[t] + T_k, T_0 = 0, T_{k+1} = T_k + dt_k summed in order; the single addition of t0 is
 *     made at use.  t0 NULL is 0 for every track.
 *   - Bad clock.  A track's clock is bad when t0[t] is not finite or when some dt_k, k < nsteps[t], is not finite or is negative.
 *     A bad clock sets STE_LINE_BAD_TIME in track_status[t] and gives min_dist, min_time, min_frac, first_cross and last_cross
 *     = NaN, min_seg = -1 and zero for every other output, for every line and sample of that track (sound_time and nbroken too).
 *   - Pieces.  Step k of track t, k < nsteps[t], is the PIECE (lo, hi) = (tau_k, tau_{k+1}).  It is examined when hi > lo: a
 *     step of zero length is skipped.  Pieces are examined in the order of k, and within a piece the segments in the order of
 *     j, which defines "first" below.
 *   - Soundness.  delta = wrap180(lon_{k+1} - lon_k).  The step is BROKEN when |delta| < 90 is false or either of its latitudes
 *     is not finite.  A broken examined step adds 1 to nbroken and nothing else.  Every other examined step is SOUND.
 *     sound_time is the sum of hi - lo over the sound examined steps, in order.
 *   - Frame of line m, ref = lon_ref[m].  Row k sits at x_k = ref + wrap180(lon_k - ref); the step runs from A = (x_k, lat_k) to
 *     B = (x_k + delta, lat_{k+1}).  Vertices are used as stored, so adjacent segments share a vertex's bits.  PRECONDITION:
 *     every vertex longitude of line m lies within ref +- 90; then, as for ste_region_f64, no periodic copy of the line can be
 *     met by a sound step and stored longitudes of the ships may be wrapped or not.  The library cannot refuse a violation (the
 *     vertices are device memory): the kernel marks the line bad, the Python front end raises before the call.
 *   - Bad line.  Line m is bad when first[m+1] - first[m] < 2, when its range leaves [0, V] (first[m] < 0 or first[m+1] > V),
 *     when lon_ref[m] is not finite, or when any of its vertices has a non-finite coordinate or a longitude with
 *     |lon - ref| <= 90 false.  A bad line sets STE_LINE_BAD_LINE in line_status[m] and gives min_dist, min_time, min_frac,
 *     first_cross and last_cross = NaN, min_seg = -1 and zero for ncross and net_cross, for every track and sample.  With a bad
 *     range nothing of the line is read.
 *   - Crossing, planar in degrees: the rule of ste_region_f64.  On a sound step, for segment j, with d = B - A, e = Q - P,
 *     w = P - A:  den = d.x * e.y - d.y * e.x,  u = (w.x * e.y - w.y * e.x) / den,  v = (w.x * d.y - w.y * d.x) / den.  A
 *     CROSSING exists when den != 0, 0 <= u < 1 and 0 <= v < 1 (so a track through a vertex shared by two segments crosses
 *     once).  It adds 1 to ncross, and +1 to net_cross when den < 0 and -1 otherwise (for a counter-clockwise ring +1 is
 *     ste_region_f64's ENTERING); its time is lo + u * (hi - lo).  first_cross is the earliest: of the first step that has a
 *     crossing, lo + umin * (hi - lo) with umin the smallest u of that step's crossings; last_cross likewise is the latest: of
 *     the last step that has one, with the largest u.  No crossing is sorted.  Without a crossing both are NaN.
 *   - Closest approach, planar in km, per (sound step, segment).  c = cos(0.25 * ((A.y + B.y) + (P.y + Q.y)) * kDeg2Rad),
 *     Kd = 6378.137 * kDeg2Rad (one double), kc = Kd * c.  a0 = (kc * w.x, Kd * w.y), a1 = (kc * (Q.x - A.x), Kd * (Q.y - A.y)),
 *     dk = (kc * d.x, Kd * d.y), ek = a1 - a0, dd = dk . dk, ee = ek . ek, b0 = a0 - dk.  cos is the only operation here whose
 *     bits may differ between implementations.  The CANDIDATES, each a (u, v, q) with q the squared norm of the difference
 *     vector g between the point of the segment at v and the ship's position at u, q = g.x * g.x + g.y * g.y, in this order:
 *       1. the crossing, when there is one: its (u, v), q = 0;
 *       2. P against the step: u = dd > 0 ? clamp01((a0 . dk) / dd) : 0, v = 0, g = (a0.x - u * dk.x, a0.y - u * dk.y);
 *       3. Q against the step: u = dd > 0 ? clamp01((a1 . dk) / dd) : 0, v = 1, g = (a1.x - u * dk.x, a1.y - u * dk.y);
 *       4. A against the segment: v = ee > 0 ? clamp01(-(a0 . ek) / ee) : 0, u = 0, g = (a0.x + v * ek.x, a0.y + v * ek.y);
 *       5. B against the segment: v = ee > 0 ? clamp01(-(b0 . ek) / ee) : 0, u = 1, g = (b0.x + v * ek.x, b0.y + v * ek.y).
 *     A candidate replaces the best one only when its q < best_q (best_q starts at +inf; strict, so the first candidate of the
 *     first segment of the first step wins a tie).  The best candidate records min_time = lo + u * (hi - lo), the ship's
 *     position (A.x + u * d.x, A.y + u * d.y), min_seg = j and min_frac = v.  After the last step min_dist is the leg of
 *     ste_path_metrics_f64 for `model` from that position to (P.x + v * (Q.x - P.x), P.y + v * (Q.y - P.y)) of the recorded
 *     segment: the leg function runs once per (sample, line, track).  Without a sound step min_dist, min_time and min_frac are
 *     NaN and min_seg is -1.
 *   - Accuracy.  That of ste_site_f64: the planar metric is for a ship near the line, and min_dist is a true distance (of
 *     `model`) between a point of the track and a point of the line, at the time the planar distance is least.  A step and a
 *     line more than 180 degrees apart in the frame (more than 90 degrees of true longitude between them) are compared in the
 *     wrong image; the planar metric means nothing there anyway, and min_dist, still a true distance between a point of the
 *     track and a point of the line, is an upper bound.
 *   - Every value's bits depend on the track's rows, its dt and t0, and the line's vertices and lon_ref alone: not on S, M, the
 *     line's place in the list or in vert, the window, or which outputs were asked for.
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_path_metrics_f64, t0 and track_status like nsteps.  Rows past nsteps[t]
 *     of states are not read.  Outputs per (sample, line, track) are out[(s * M + m) * track_stride + t]; sound_time and nbroken
 *     out[s * track_stride + t] (track_stride = B where it is 0).
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or li NULL; states, vert, first or lon_ref
 *     NULL; nstates < 1 or > 65535; nlines < 1 or > STE_LINES_MAX; nvert < 2 or > STE_LINE_MAX_VERT_TOTAL; an unknown model when
 *     min_dist is asked for; flags or reserved non-zero; b->dt NULL; every output NULL; B <= 0, Nmax < 0, or track_stride
 *     non-zero and below B; and a call whose ceil(B / 64) * nlines exceeds 2^31 - 1.
 */
#define STE_LINES_MAX 4096
#define STE_LINE_MAX_VERT_TOTAL (1 << 20)
#define STE_LINE_BAD_TIME 0x1  /* track_status: a non-finite t0, or a dt below nsteps that is not finite and >= 0 */
#define STE_LINE_BAD_LINE 0x1  /* line_status: fewer than 2 vertices, a range outside vert, a non-finite lon_ref or vertex, a vertex outside lon_ref +- 90 */
typedef struct ste_line_f64 {
    int32_t nstates;         /* S >= 1 tracks per ship in `states` (<= 65535) */
    int32_t model;           /* STE_PREP_SPHERE / STE_PREP_WGS84: leg function for min_dist only */
    const double* states;    /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 */
    int32_t nlines;          /* M, 1 .. STE_LINES_MAX */
    int32_t nvert;           /* V, 2 .. STE_LINE_MAX_VERT_TOTAL: vertices of all lines together */
    const double* vert;      /* DEVICE [2][V]: lon[0..V) then lat[0..V), degrees */
    const int32_t* first;    /* DEVICE [M+1]: line m owns vertices first[m] .. first[m+1] - 1 */
    const double* lon_ref;   /* DEVICE [M]: the meridian line m is unwrapped about */
    const double* t0;        /* DEVICE [track_stride] or NULL (= 0): clock time of row 0 of each track, as ste_site_f64 */
    uint32_t flags;          /* must be 0 */
    uint32_t reserved;       /* must be 0 */
    double* min_dist;        /* DEVICE [S][M][track_stride] or NULL: km at the closest approach, NaN = no sound step */
    double* min_time;        /* DEVICE [S][M][track_stride] or NULL: its clock time, hours; NaN likewise */
    int32_t* min_seg;        /* DEVICE [S][M][track_stride] or NULL: segment of the line that is closest, -1 = none */
    double* min_frac;        /* DEVICE [S][M][track_stride] or NULL: v on that segment, 0 at its first vertex, 1 at its second; NaN = none */
    int32_t* ncross;         /* DEVICE [S][M][track_stride] or NULL: crossings */
    int32_t* net_cross;      /* DEVICE [S][M][track_stride] or NULL: crossings with den < 0 minus the others */
    double* first_cross;     /* DEVICE [S][M][track_stride] or NULL: clock time of the earliest crossing, NaN = none */
    double* last_cross;      /* DEVICE [S][M][track_stride] or NULL: clock time of the latest crossing, NaN = none */
    double* sound_time;      /* DEVICE [S][track_stride] or NULL: hours of sound steps */
    int32_t* nbroken;        /* DEVICE [S][track_stride] or NULL: broken examined steps */
    int32_t* track_status;   /* DEVICE [track_stride] or NULL: STE_LINE_BAD_TIME (does not depend on the sample or the line) */
    int32_t* line_status;    /* DEVICE [M] or NULL: STE_LINE_BAD_LINE */
} ste_line_f64;              /* 160 bytes */

int ste_line_metrics_f64(const ste_ukf_batch_f64* b, const ste_line_f64* li, void* stream);
/* segments of a line the kernel stages at a time; line lengths at and around its multiples are where the staging shows */
int ste_line_chunk(void);

/*
 * ROUTES: pairs of tracks that stay on the device as CURVES, without a clock (an unnumbered addition, like ste_line_f64): did
 * two ships sail the same route, and where do the two curves differ most?  Per (sample, pair) the discrete Frechet distance
 * (the largest gap under the best monotone matching of rows) with the rows that attain it, and the dynamic-time-warping (DTW)
 * cost (the summed gap under the best matching) with the number of cells on its path.  `states` is that of ste_path_f64, the
 * pair list that of ste_encounter_f64.  No dt and no t0 is read: two ships on one lane a month apart have distance 0.  Below
 * kDeg2Rad is that of ste_path_f64, and every expression is evaluated as written, left to right, without contraction.
 *   - Curves.  Pair (i, j) holds sample s of ship i against sample s of ship j.  With ns = nsteps[t] (NULL = Nmax), track i
 *     gives the points a = 0 .. ns_i, its rows 0 .. ns_i; track j gives the points b = 0 .. ns_j: point b is row b, or row
 *     ns_j - b with STE_ROUTE_REVERSE_J.  A track with ns = 0 is one point and is valid.  i == j is valid (unreversed: 0).
 *   - Point.  lambda = lon * kDeg2Rad, phi = lat * kDeg2Rad, c = cos(phi), u = (c * cos(lambda), c * sin(lambda), sin(phi)).
 *   - Cell.  d = u_i(a) - u_j(b) componentwise, q(a, b) = (d.x * d.x + d.y * d.y) + d.z * d.z: the squared chord on the unit
 *     sphere, monotone in the great-circle distance.  A q that is not finite counts as +inf.  cos and sin are the only
 *     operations here whose bits may differ between implementations.
 *   - Cost (DTW only).  h = 0.5 * sqrt(q), h > 1 taken as 1; cost(a, b) = (2 * 6378.137) * asin(h): km on the sphere of
 *     ste_path_f64.  asin joins cos and sin as an operation whose bits may differ.
 *   - Band.  Cell (a, b) is ADMISSIBLE when band == 0 or |a - b| <= band (a Sakoe-Chiba band).  Every admissible cell but
 *     (0, 0) has an admissible predecessor: the diagonal one, or along row 0 / column 0 the one toward (0, 0).
 *   - Predecessor of (a, b) for a table T: of (a-1, b-1), (a-1, b), (a, b-1), in this order, among those that exist and are
 *     admissible, the first; a later one replaces it only when its T is strictly smaller.
 *   - Frechet table.  F(0, 0) = q(0, 0), at(0, 0) = (0, 0).  Otherwise m = F(predecessor by F); if q(a, b) >= m then
 *     F = q(a, b) and at = (a, b), else F = m and at = at(predecessor).
 *   - DTW tables.  D(0, 0) = cost(0, 0), L(0, 0) = 1.  Otherwise D = cost(a, b) + D(predecessor by D) and
 *     L = 1 + L(predecessor by D).
 *   - Bits.  min and max do not round and each D is one addition, so every value has the bits of the row-major recurrence
 *     whatever the order in which the device evaluates the cells.
 *   - Outputs, taken at (ns_i, ns_j).  frechet_at = at(ns_i, ns_j) as ROW indices of the two tracks (with reversal the second
 *     entry is ns_j - b).  frechet is the leg of ste_path_metrics_f64 for `model` between the positions of those two rows: the
 *     leg function runs once per (sample, pair).  dtw = D(ns_i, ns_j), dtw_len = L(ns_i, ns_j).
 *   - Status.  F(ns_i, ns_j) = +inf sets STE_ROUTE_NOT_FINITE: every coupling visits every row, so one row with a non-finite
 *     coordinate suffices.  STE_ROUTE_BAD_INDEX (a pair index outside [0, B)) and STE_ROUTE_NO_PATH (band > 0 and
 *     |ns_i - ns_j| > band: the last cell is not admissible) are decided before anything of the pair is read.  Any status bit
 *     gives frechet = dtw = NaN, frechet_at = (-1, -1) and dtw_len = 0.
 *   - Every value's bits depend on the two tracks' rows, band and the reverse flag alone: not on S, P, the pair's place in the
 *     list, the window, which outputs were asked for, or whether `work` was used.
 *   - The call reads only B, Nmax, track_stride and nsteps (NULL = Nmax for every track) of the batch and writes nothing of the
 *     batch; windows and addressing are those of ste_path_metrics_f64.  Rows past nsteps[t] of states are not read.  Outputs
 *     per (sample, pair) are out[s * P + p] (frechet_at: two of them).
 *   - Work.  A pair whose track j has more than ste_route_lds_cols() points keeps a row of the tables in `work`;
 *     ste_route_workspace(Nmax, nstates, npairs) is the number of bytes these sizes need, 0 while Nmax + 1 <= ste_route_lds_cols().
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or ro NULL; states or pairs NULL; nstates < 1
 *     or > 65535; npairs < 1 or > STE_ROUTE_MAX_PAIRS; an unknown model when frechet is asked for; band < 0; flags with any
 *     other bit than STE_ROUTE_REVERSE_J; every output NULL (each output is independent of the others); work NULL or work_bytes
 *     below ste_route_workspace(Nmax, nstates, npairs) when that is non-zero; B <= 0, Nmax < 0 or Nmax > 2^31 - 257, or
 *     track_stride non-zero and below B.
 */
#define STE_ROUTE_MAX_PAIRS (1 << 26)
#define STE_ROUTE_REVERSE_J 0x1u     /* flags: track j is read from its last row to its first */
#define STE_ROUTE_BAD_INDEX 0x1      /* status: a pair index outside [0, B): nothing of that pair is read */
#define STE_ROUTE_NO_PATH 0x2        /* status: band > 0 and |ns_i - ns_j| > band: nothing of that pair is read */
#define STE_ROUTE_NOT_FINITE 0x4     /* status: a coordinate of a row read is not finite */
typedef struct ste_route_f64 {
    int32_t nstates;         /* S >= 1 tracks per ship in `states` (<= 65535) */
    int32_t model;           /* STE_PREP_SPHERE / STE_PREP_WGS84: leg function for `frechet` only */
    const double* states;    /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 */
    int64_t npairs;          /* P, 1 .. STE_ROUTE_MAX_PAIRS */
    const int32_t* pairs;    /* DEVICE [P][2]: (i, j), tracks of the window */
    int32_t band;            /* >= 0, 0 = none */
    uint32_t flags;          /* STE_ROUTE_REVERSE_J or 0 */
    double* work;            /* DEVICE scratch of work_bytes, see ste_route_workspace; may be NULL when that is 0 */
    int64_t work_bytes;
    double* frechet;         /* DEVICE [S][P] or NULL: km */
    int32_t* frechet_at;     /* DEVICE [S][P][2] or NULL: (row of i, row of j) of the cell that attains it */
    double* dtw;             /* DEVICE [S][P] or NULL: km */
    int32_t* dtw_len;        /* DEVICE [S][P] or NULL: cells on the warping path */
    int32_t* status;         /* DEVICE [S][P] or NULL: STE_ROUTE_* bits */
} ste_route_f64;             /* 96 bytes */

int ste_route_metrics_f64(const ste_ukf_batch_f64* b, const ste_route_f64* ro, void* stream);
/* bytes of `work` these sizes need; may be 0 */
size_t ste_route_workspace(int32_t Nmax, int32_t nstates, int64_t npairs);
/* columns of track j whose boundary row the kernel keeps in LDS; a pair with more goes through `work` */
int ste_route_lds_cols(void);

/*
 * SPEEDS: how fast tracks that stay on the device went (an unnumbered addition, like ste_route_f64): the speed made good of every
 * step, its maximum and when, the hours spent in each of up to STE_SPEED_MAX_BANDS speed bands, and the RUNS of steps at or below
 * a speed threshold (stops, loitering) or, with STE_SPEED_ABOVE, at or above it (sustained speed): how often, for how long, from
 * when, and the longest.  `states` is that of ste_path_f64, the leg that of ste_path_metrics_f64 for `model`, the clock that of
 * ste_site_f64 without t0: times are hours from row 0, as cross_time is.  Every expression below is evaluated as written, left to
 * right, without contraction.
 *   - Clock.  T_0 = 0, T_{k+1} = T_k + dt_k, summed in order.
 *   - Bad clock, bad limit.  A track's clock is bad when some dt_k, k < nsteps[t], is not finite or is negative
 *     (STE_SPEED_BAD_TIME).  Its limit is bad when a run output is asked for and its threshold thr (threshold[t], or threshold_all
 *     where threshold is NULL) is not finite or is negative (STE_SPEED_BAD_LIMIT); a call without run outputs reads no threshold
 *     and never sets that bit.  Either bit gives NaN for vmax, vmax_time, first_run, longest_start and every speed row below
 *     nsteps[t], and zero for every other output of that track, for every sample.
 *   - Step.  Step k of track t, k < nsteps[t], is examined when dt_k > 0.  A SKIPPED step (dt_k == 0) writes NaN to speed and
 *     closes the run.  L_k is the leg of ste_path_metrics_f64 for `model` from row k to row k + 1, and v_k = L_k / dt_k.  An
 *     examined step is BROKEN when v_k is not finite (a coordinate that is not finite, or a quotient that overflows): it adds 1 to
 *     nbroken, writes NaN to speed, closes the run and adds nothing else.  Every other examined step is SOUND and writes
 *     speed = v_k.  Steps are examined in the order of k, which defines "first" below.
 *   - Sums.  dist and sound_time add L_k and dt_k over the sound steps, in order: where every step of a track is examined and
 *     sound, dist has the bits of ste_path_metrics_f64's dist.
 *   - Maximum.  A sound step becomes the best one when v_k > vmax (vmax starts below every speed; strict, so the first step wins
 *     a tie); it records vmax = v_k and vmax_time = T_k, the start of the step.  Without a sound step both are NaN.
 *   - Bands.  j = (number of i in 0 .. nbands with band_edges[i] <= v_k) - 1; a sound step adds dt_k to band_time of band j when
 *     0 <= j < nbands.  A speed below band_edges[0], or at or above band_edges[nbands], falls in no band.
 *   - Runs.  A sound step QUALIFIES when v_k <= thr, or with STE_SPEED_ABOVE when v_k >= thr; cond_time is the sum of dt_k over
 *     the qualifying steps, in order.  A RUN is a maximal sequence of consecutive qualifying steps: its length is the sum of their
 *     dt_k in order, its start T_k of its first step.  A step that does not qualify, a broken step, a skipped step and the end
 *     of the track close the run.  On closing, a run of length len >= min_run_h adds 1 to nruns and len to run_time, and the
 *     first such run sets first_run to its start; any run with len > longest (strict: the first of equal ones) sets longest = len
 *     and longest_start to its start, whether it reaches min_run_h or not.  No tolerance anywhere.
 *   - Every value's bits depend on the track's rows, its dt and its threshold, and on band_edges and min_run_h alone: not on S,
 *     the window, the lane, or which outputs were asked for (a bad limit excepted: it exists only with a run output).
 *   - The call reads only B, Nmax, track_stride, nsteps (NULL = Nmax for every track) and dt of the batch and writes nothing of
 *     the batch; windows and addressing are those of ste_path_metrics_f64, threshold and track_status like nsteps.  Rows past
 *     nsteps[t] of states are not read, and rows k >= nsteps[t] of speed are not written.  Per (sample, track) outputs are
 *     out[s * track_stride + t], speed is speed[(s * Nmax + k) * track_stride + t] and band_time is
 *     band_time[(s * nbands + j) * track_stride + t] (track_stride = B where it is 0).
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or sp NULL; states NULL; nstates < 1 or
 *     > 65535; an unknown model; flags with any other bit than STE_SPEED_ABOVE; nbands < 0 or > STE_SPEED_MAX_BANDS; band_edges
 *     NULL with nbands > 0, or given with nbands == 0; an edge that is not finite, is negative or does not ascend strictly;
 *     band_time given with nbands == 0; min_run_h not finite or negative; a run output (cond_time, run_time, first_run, longest,
 *     longest_start, nruns) given while threshold is NULL and threshold_all is not finite or is negative; b->dt NULL; every
 *     output NULL; B <= 0, Nmax < 0, or track_stride non-zero and below B.
 */
#define STE_SPEED_MAX_BANDS 32
#define STE_SPEED_ABOVE 0x1u      /* flags: a step qualifies when v >= threshold (sustained speed); default v <= threshold (stops) */
#define STE_SPEED_BAD_TIME 0x1    /* track_status: a dt below nsteps that is not finite and >= 0 */
#define STE_SPEED_BAD_LIMIT 0x2   /* track_status: the track's threshold is not finite or is < 0 */
typedef struct ste_speed_f64 {
    int32_t nstates;         /* S >= 1 tracks per ship in `states` (<= 65535) */
    int32_t model;           /* STE_PREP_SPHERE / STE_PREP_WGS84: the leg function */
    const double* states;    /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64; components 0 and 1 are read */
    uint32_t flags;          /* STE_SPEED_ABOVE or 0 */
    int32_t nbands;          /* 0 .. STE_SPEED_MAX_BANDS */
    const double* band_edges;/* HOST [nbands + 1]: km/h, finite, >= 0, strictly ascending; NULL iff nbands == 0 */
    const double* threshold; /* DEVICE [track_stride]: km/h per track, or NULL: threshold_all for every track */
    double threshold_all;    /* km/h; NaN = no run output may be asked for */
    double min_run_h;        /* hours, finite, >= 0: a run QUALIFIES when its length >= min_run_h */
    double* speed;           /* DEVICE [S][Nmax][track_stride] or NULL: km/h of step k; NaN for a skipped or broken step */
    double* dist;            /* DEVICE [S][track_stride] or NULL: km over the sound steps, in order */
    double* sound_time;      /* DEVICE [S][track_stride] or NULL: hours of the sound steps, in order */
    double* vmax;            /* DEVICE [S][track_stride] or NULL: the largest speed of a sound step; NaN = none */
    double* vmax_time;       /* DEVICE [S][track_stride] or NULL: T_k of that step (hours from row 0, its start); NaN = none */
    double* band_time;       /* DEVICE [S][nbands][track_stride] or NULL: hours of sound steps with edges[j] <= v < edges[j+1] */
    double* cond_time;       /* DEVICE [S][track_stride] or NULL: hours of qualifying steps, whatever their run */
    double* run_time;        /* DEVICE [S][track_stride] or NULL: hours inside qualifying runs */
    double* first_run;       /* DEVICE [S][track_stride] or NULL: T at the start of the first qualifying run; NaN = none */
    double* longest;         /* DEVICE [S][track_stride] or NULL: length of the longest run, qualifying or not; 0 = none */
    double* longest_start;   /* DEVICE [S][track_stride] or NULL: T at its start; NaN = none */
    int32_t* nruns;          /* DEVICE [S][track_stride] or NULL: qualifying runs */
    int32_t* nbroken;        /* DEVICE [S][track_stride] or NULL: broken examined steps */
    int32_t* track_status;   /* DEVICE [track_stride] or NULL: STE_SPEED_BAD_* (does not depend on the sample) */
} ste_speed_f64;             /* 168 bytes */

int ste_speed_metrics_f64(const ste_ukf_batch_f64* b, const ste_speed_f64* sp, void* stream);

/*
 * ERRORS: how far tracks that stay on the device are from where the ship really was (an unnumbered addition, like ste_speed_f64):
 * the distance of every row from a truth position of that row, in km, its sums, its split along and across the true course, and its
 * score against the track's own covariance (NEES and coverage).  `states` is that of ste_path_f64.  Every expression below is
 * evaluated as written, left to right, without contraction.
 *   - Rows.  Row k of track t, 0 <= k <= nsteps[t], is TRUTHED when both coordinates of truth row k are finite.  A truthed row is
 *     BROKEN when the state's lon or lat is not finite, or when the leg below is not finite: it adds 1 to nbroken, writes NaN to
 *     the row outputs err, along, cross and nees, and adds nothing else.  Every other truthed row is SOUND.  Rows are taken in the
 *     order of k, which defines "first" below.
 *   - Error.  e_k is the distance of the leg of `model` FROM the truth (point 1) TO the state (point 2), km, and h_k that leg's
 *     initial heading, degrees in [0, 360): sphere_leg / wgs84_leg of ste_geodesy.h, what ste_track_prep_f64 computes for two
 *     observations (WGS84: 0 and 0 for points closer than 1e-8 degrees in both coordinates).
 *   - Sums over the sound rows, in order: n counts them, sum_err adds e_k, sum_sq adds e_k * e_k.  A sound row becomes the worst
 *     one when e_k > max_err (strict, so the first row wins a tie); it records max_err = e_k and max_row = k.  With no sound row
 *     max_err is NaN and max_row is -1.  cumerr row k is sum_err after row k; rows that are not sound carry the running value, so
 *     sum_err equals cumerr row nsteps[t] bit for bit (cum_abs_diff in km; rmse is sqrt(sum_sq / n)).
 *   - Along and cross (with `course`).  A sound row is COURSED when course row k is finite.  theta = (h_k - course_k) * kDeg2Rad
 *     (0.017453292519943295), along_k = e_k * cos(theta), positive when the state is ahead of the truth, cross_k =
 *     e_k * sin(theta), positive to starboard.  ncoursed counts the coursed rows; sum_along, sum_along_sq, sum_cross and
 *     sum_cross_sq add along_k, along_k * along_k, cross_k and cross_k * cross_k over them, in order.  A sound row without a
 *     course writes NaN to along and cross and adds nothing to these sums.
 *   - NEES (with `cov`).  dx = wrap180(lon - lon_t), dy = lat - lat_t, degrees, wrap180(y) = floored_mod(y + 180, 360) - 180;
 *     a, b, c are entries 00, 01 and 11 of the covariance of row k (rows 0, 1, 5 of 16, rows 0, 1, 4 of 10);
 *     det = a * c - b * b; q_k = (c * dx * dx - 2.0 * b * dx * dy + a * dy * dy) / det.  A sound row is SCORED when a, b, c and
 *     q_k are finite, a > 0 and det > 0.  nscored counts the scored rows, sum_nees adds q_k over them in order, ninside counts
 *     those with q_k <= nees_limit (coverage is ninside / nscored; -2 ln(1 - p) is the chi-square quantile for 2 degrees of
 *     freedom).  A row that is not scored writes NaN to nees.
 *   - Row outputs.  err, along, cross and nees of a row k <= nsteps[t] that is not truthed, or not sound, are NaN; cumerr of
 *     such a row is the running value.  Rows past nsteps[t] of every row output are not written.  No tolerance anywhere.
 *   - Every value's bits depend on the track's rows, truth, course and covariance, and on nees_limit alone: not on S, the window,
 *     the lane, or which outputs were asked for.
 *   - The call reads only B, Nmax, track_stride and nsteps (NULL = Nmax for every track) of the batch, no dt, and writes nothing
 *     of the batch; windows and addressing are those of ste_path_metrics_f64: truth, course and cov are rows of track_stride tracks
 *     like the batch's own arrays and do not depend on the sample.  Rows past nsteps[t] are not read.  Per (sample, track)
 *     outputs are out[s * track_stride + t], row outputs out[(s * (Nmax + 1) + k) * track_stride + t] (track_stride = B where it
 *     is 0).
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or er NULL; states or truth NULL; nstates < 1
 *     or > 65535; an unknown model; cov_rows not 16 or 10 while cov is given; cov with nstates > 1 (a covariance belongs to one
 *     track, not to its samples); nees_limit not finite or <= 0 while cov is given; an along / cross output (sum_along,
 *     sum_along_sq, sum_cross, sum_cross_sq, ncoursed, along, cross) without course; a NEES output (sum_nees, nscored, ninside,
 *     nees) without cov; reserved != 0; every output NULL; B <= 0, Nmax < 0, or track_stride non-zero and below B.
 */
#define STE_ERRORS_COV_FULL 16    /* cov_rows: full 4 x 4 matrices, row-major (sm_cov without STE_FLAG_PACKED_COV) */
#define STE_ERRORS_COV_PACKED 10  /* cov_rows: upper triangles 00 01 02 03 11 12 13 22 23 33 (STE_FLAG_PACKED_COV) */
typedef struct ste_errors_f64 {
    int32_t nstates;         /* S >= 1 tracks per ship in `states` (<= 65535) */
    int32_t model;           /* STE_PREP_SPHERE / STE_PREP_WGS84: the leg function */
    const double* states;    /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64; components 0 and 1 are read */
    const double* truth;     /* DEVICE [Nmax+1][2][track_stride]: lon, lat in degrees; a row that is not finite has no truth */
    const double* course;    /* DEVICE [Nmax+1][track_stride] or NULL: the true course over ground, degrees */
    const double* cov;       /* DEVICE [Nmax+1][cov_rows][track_stride] or NULL: the track's covariance (sm_cov, fwd_cov); S == 1 */
    int32_t cov_rows;        /* STE_ERRORS_COV_FULL or STE_ERRORS_COV_PACKED; read only with cov */
    int32_t reserved;        /* 0 */
    double nees_limit;       /* q_k <= nees_limit counts as inside; finite and > 0; read only with cov */
    double* sum_err;         /* DEVICE [S][track_stride] or NULL: km, the sum of e_k over the sound rows */
    double* sum_sq;          /* DEVICE [S][track_stride] or NULL: km^2 */
    double* max_err;         /* DEVICE [S][track_stride] or NULL: the largest e_k; NaN = no sound row */
    double* sum_along;       /* DEVICE [S][track_stride] or NULL: km over the coursed rows */
    double* sum_along_sq;    /* DEVICE [S][track_stride] or NULL */
    double* sum_cross;       /* DEVICE [S][track_stride] or NULL */
    double* sum_cross_sq;    /* DEVICE [S][track_stride] or NULL */
    double* sum_nees;        /* DEVICE [S][track_stride] or NULL: the sum of q_k over the scored rows */
    int32_t* n;              /* DEVICE [S][track_stride] or NULL: sound rows */
    int32_t* max_row;        /* DEVICE [S][track_stride] or NULL: the row of max_err; -1 = none */
    int32_t* nbroken;        /* DEVICE [S][track_stride] or NULL: broken rows */
    int32_t* ncoursed;       /* DEVICE [S][track_stride] or NULL: coursed rows */
    int32_t* nscored;        /* DEVICE [S][track_stride] or NULL: scored rows */
    int32_t* ninside;        /* DEVICE [S][track_stride] or NULL: scored rows with q_k <= nees_limit */
    double* err;             /* DEVICE [S][Nmax+1][track_stride] or NULL: e_k; NaN for a row without truth and for a broken row */
    double* cumerr;          /* DEVICE [S][Nmax+1][track_stride] or NULL: sum_err after row k */
    double* along;           /* DEVICE [S][Nmax+1][track_stride] or NULL: NaN unless coursed */
    double* cross;           /* DEVICE [S][Nmax+1][track_stride] or NULL: NaN unless coursed */
    double* nees;            /* DEVICE [S][Nmax+1][track_stride] or NULL: q_k; NaN unless scored */
} ste_errors_f64;            /* 208 bytes */

int ste_track_errors_f64(const ste_ukf_batch_f64* b, const ste_errors_f64* er, void* stream);

/*
 * RASTERS: tracks that stay on the device against a GRIDDED FIELD (an unnumbered addition, like ste_grid_f64): a land mask,
 * bathymetry, an ice concentration, a climatology, or the ship-hours map that ste_grid_metrics_f64 itself made of a fleet.
 * ste_grid_metrics_f64 walks a track's pieces through the cells and ADDS to every cell; this call walks the same pieces and
 * READS every cell.  `states` is that of ste_path_f64.
 *   - Raster.  The grid is that of ste_grid_f64 (GRIDS: Grid.), member for member: nx, ny, lon0, lat0, dlon, dlat, lon_ref,
 *     STE_GRID_PERIODIC_LON in `flags` with the same conditions, at most STE_GRID_MAX_CELLS cells.  `values` is a DEVICE array
 *     double [ny][nx], one value per cell, constant over the cell, cell (ix, iy) at [iy * nx + ix].  NaN means NO DATA; +-inf
 *     are values.
 *   - Track.  Everything about the track is the grid call's, word for word (GRIDS: Unwrapping., Pieces., Runs.): unwrapping
 *     about lon_ref, SOUND and BROKEN steps, dtq = rint(dt_k * 2^20), the split of a sound step at the grid lines strictly
 *     between its ends (x-lines and y-lines merged by u, ties to x, tq = max(rint(u * dtq), the previous line's tick)), the
 *     clipping by clamped line indices, and the dropped pieces of 0 ticks.
 *   - Runs.  A RUN is the grid's: a maximal stretch of consecutive non-empty pieces in one cell (or outside), across steps and
 *     across broken steps.  It has its cell, its ticks q, its START -- the ticks of the track's sound steps before its first
 *     piece: the tick clock, which broken steps do not advance -- and its value v = values[cell].  A run outside has no value.
 *     A run is VALID when it is on the grid and v is not NaN.
 *   - total, outside, nbroken: as in ste_grid_metrics_f64, the same bits.  valid: the ticks of the valid runs.  nodata: the
 *     ticks of the runs on the grid whose value is NaN.  EXACTLY: valid + nodata + outside = total.
 *   - wsum = the sum over the valid runs, in track order, of (double)q * v, from 0.0: one multiplication and one addition per
 *     run, not contracted.  The mean of the field along the track is wsum / valid.
 *   - vmin, vmax: the least and the greatest value over the valid runs; tmin, tmax: the start of the FIRST run that attains
 *     it.  From vmin = vmax = NaN, tmin = tmax = -1, in track order: if (!(vmin <= v)) { vmin = v; tmin = start; } and
 *     if (!(vmax >= v)) { vmax = v; tmax = start; }.  A track without a valid run gives NaN and -1.
 *   - Threshold.  A valid run is a HIT when v >= threshold, or v <= threshold with STE_RASTER_BELOW.  With
 *     STE_RASTER_NO_THRESHOLD nothing is a hit, threshold and min_ticks are not looked at and the hit outputs must be NULL.  An
 *     EXCURSION is a maximal stretch of consecutive runs that are all hits: a run that is no hit (a miss, no data, outside)
 *     ends it, a broken step does not.  hit_ticks: the ticks of all hits.  hit_first: the start of the first hit, -1 = never.
 *     nhit: the number of excursions.  nhit_long: those of at least min_ticks ticks.  hit_longest: the ticks of the longest
 *     excursion, 0 without one.
 *   - row_value[s][k][t], k <= nsteps[t]: the value of the cell that row k itself lies in, (floor((x_k - lon0) / dlon),
 *     floor((lat_k - lat0) / dlat)), the column taken modulo nx (floored) when periodic; NaN where the row is off the grid or
 *     its lon or lat is not finite.  Whether the steps about the row are sound does not matter.  Rows past nsteps[t] are not
 *     written.
 *   - A track with nsteps == 0 gives zeros, NaN and -1 as above, and its row 0 in row_value.
 *   - Every per-track output is [S][track_stride] like outside / total of ste_grid_f64, and may be NULL; at least one output is
 *     required.  The call reads the batch exactly as ste_grid_metrics_f64 does (B, Nmax, track_stride, nsteps, dt; windows)
 *     and writes nothing of it.  Every value depends on its own track's rows and the raster alone, and every sum takes its
 *     terms in track order: windows, sample slices and the outputs asked for cannot move a bit.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: every refusal of ste_grid_metrics_f64 (b or r
 *     NULL; states NULL; nstates < 1 or > 65535; nx or ny < 1 or nx * ny > STE_GRID_MAX_CELLS; a non-finite lon0, lat0 or
 *     lon_ref; dlon or dlat not finite or < 1e-6; the conditions of STE_GRID_PERIODIC_LON and of a grid without it; b->dt
 *     NULL; B <= 0, Nmax < 0, or track_stride non-zero and below B); values NULL; unknown flag bits; a NaN threshold without
 *     STE_RASTER_NO_THRESHOLD; min_ticks < 0; a hit output together with STE_RASTER_NO_THRESHOLD; every output NULL.
 */
#define STE_RASTER_BELOW 0x2u         /* a hit is v <= threshold (default: v >= threshold) */
#define STE_RASTER_NO_THRESHOLD 0x4u  /* no threshold: the hit outputs must be NULL */
typedef struct ste_raster_f64 {
    int32_t nstates;       /* S >= 1 tracks per ship in `states` (<= 65535) */
    uint32_t flags;        /* STE_GRID_PERIODIC_LON | STE_RASTER_* ; unknown bits refused */
    const double* states;  /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64 / ste_grid_f64 */
    int32_t nx, ny;        /* columns (lon) and rows (lat), >= 1, nx * ny <= STE_GRID_MAX_CELLS */
    double lon0, lat0;     /* HOST: west and south edge of cell (0, 0), degrees */
    double dlon, dlat;     /* HOST: cell size, finite, >= 1e-6 */
    double lon_ref;        /* HOST: meridian the longitudes are unwrapped about */
    const double* values;  /* DEVICE [ny][nx]: the field, a value per cell; NaN = no data */
    double threshold;      /* HOST: not NaN, unless STE_RASTER_NO_THRESHOLD */
    int64_t min_ticks;     /* HOST: >= 0; an excursion of at least this many ticks counts in nhit_long */
    int64_t* total;        /* DEVICE [S][track_stride] out or NULL: ticks of all sound steps */
    int64_t* outside;      /* DEVICE [S][track_stride] out or NULL: ticks spent off the grid */
    int32_t* nbroken;      /* DEVICE [S][track_stride] out or NULL */
    int64_t* valid;        /* DEVICE [S][track_stride] out or NULL: ticks of runs with a value */
    int64_t* nodata;       /* DEVICE [S][track_stride] out or NULL: ticks of runs on the grid whose value is NaN */
    double* wsum;          /* DEVICE [S][track_stride] out or NULL: sum of (double)q * v over the valid runs */
    double* vmin;          /* DEVICE [S][track_stride] out or NULL: NaN without a valid run */
    double* vmax;          /* DEVICE [S][track_stride] out or NULL */
    int64_t* tmin;         /* DEVICE [S][track_stride] out or NULL: start of the first run at vmin, -1 without one */
    int64_t* tmax;         /* DEVICE [S][track_stride] out or NULL */
    int64_t* hit_ticks;    /* DEVICE [S][track_stride] out or NULL: ticks of all hits */
    int64_t* hit_first;    /* DEVICE [S][track_stride] out or NULL: start of the first hit, -1 = never */
    int32_t* nhit;         /* DEVICE [S][track_stride] out or NULL: excursions */
    int32_t* nhit_long;    /* DEVICE [S][track_stride] out or NULL: excursions of at least min_ticks ticks */
    int64_t* hit_longest;  /* DEVICE [S][track_stride] out or NULL: ticks of the longest excursion */
    double* row_value;     /* DEVICE [S][Nmax+1][track_stride] out or NULL; rows past nsteps[t] untouched */
} ste_raster_f64;          /* 216 bytes */

int ste_raster_metrics_f64(const ste_ukf_batch_f64* b, const ste_raster_f64* r, void* stream);

/*
 * SIMPLIFICATION: tracks that stay on the device made SMALLER within a tolerance (an unnumbered addition, like ste_raster_f64):
 * the time-aware Douglas-Peucker rule (TD-TR, "synchronised Euclidean distance"), which drops a row when the position
 * interpolated AT THAT ROW'S OWN TIME on the chord between the surviving neighbours is within the tolerance of the row, so that
 * ste_track_positions_f64 on the simplified track stays within the tolerance of the original at every row time; and, with
 * STE_SIMPLIFY_SHAPE, the classic rule on the perpendicular distance, for questions without a clock (routes, lines).  `states` is
 * that of ste_path_f64; components 0 and 1 are read.  Every expression below is evaluated as written, left to right,
 * without contraction, and no transcendental function appears in any decision: a restatement in IEEE doubles (tests/simplify_cases.py)
 * reproduces every output bit for bit.  For track t of sample s let ns = nsteps[t] (NULL = Nmax), rows 0 .. ns.
 *   - Clock.  T_0 = 0, T_{k+1} = T_k + dt_k, summed in order.  The clock is bad when some dt_k, k < ns, is not finite or is
 *     negative (STE_SIMPLIFY_BAD_TIME).  With STE_SIMPLIFY_SHAPE there is no clock: no T is formed and the bit is never set.
 *   - Unwrapped longitude.  X_0 = lon_0, X_{k+1} = X_k + wrap180(lon_{k+1} - lon_k), summed in order, wrap180 that of
 *     ste_path_f64; Y_k = lat_k.  The track is BROKEN when for some k < ns |wrap180(lon_{k+1} - lon_k)| < 90 is false, or when a
 *     latitude of rows 0 .. ns is not finite (STE_SIMPLIFY_BROKEN; it depends on the sample, the other two bits do not).
 *   - Metric.  c = lon_scale[t], or lon_scale_all where lon_scale is NULL; tol = tolerance[t], or tolerance_all where tolerance
 *     is NULL, in degrees of a great circle.  A per-track c or tol that is not finite or is negative sets
 *     STE_SIMPLIFY_BAD_LIMIT; a scalar with that defect is refused.  tol2 = tol * tol.
 *   - Deviation of row k from the chord (i, j), i < k < j.  xk = (X_k - X_i) * c, yk = Y_k - Y_i, xj = (X_j - X_i) * c,
 *     yj = Y_j - Y_i.  With the clock (the default): den = T_j - T_i and u = den > 0 ? (T_k - T_i) / den : 0.  With
 *     STE_SIMPLIFY_SHAPE: den = xj * xj + yj * yj and u = den > 0 ? clamp01((xk * xj + yk * yj) / den) : 0, clamp01(x) =
 *     x < 0 ? 0 : (x > 1 ? 1 : x).  Then ex = xk - u * xj, ey = yk - u * yj, d2 = ex * ex + ey * ey.
 *   - Rule.  Rows 0 and ns are kept.  A range (i, j) with j > i + 1 takes best = -1; its winner is the SMALLEST k with
 *     d2 > best, scanning k upwards (strict: the first of equal rows wins and a NaN never wins).  If best > tol2 (strict), row k
 *     is kept and (i, k) and (k, j) are ranges.  Otherwise no row inside the range is kept, and if best > worst_sq then
 *     worst_sq = best; worst_sq starts at 0.0.  The result does not depend on the order in which ranges are taken.
 *   - A (sample, track) with any of the three bits keeps every row 0 .. ns (the identity, lossless): nkeep = ns + 1 and
 *     worst_sq = NaN.  ns = 0: row 0 is kept, nkeep = 1, worst_sq = 0.
 *   - Outputs, each may be NULL but not all of them.  keep is 1 or 0 for rows 0 .. ns, keep[(s * (Nmax + 1) + k) * track_stride
 *     + t]; rows past ns are untouched.  nkeep, worst_sq (deg^2 in the scaled plane) and status are out[s * track_stride + t].
 *   - Compaction.  cap is the number of rows the three arrays rows, out_states and out_dt hold, 1 <= cap <= Nmax + 1, read only
 *     when one of them is given.  rows[(s * cap + m) * track_stride + t] is the m-th kept row r_m; out_states[((s * cap + m) * 4
 *     + c) * track_stride + t] holds the four components of that row, its bits; out_dt[(s * (cap - 1) + m) * track_stride + t]
 *     is dt_{r_m} + dt_{r_m + 1} + ... + dt_{r_{m+1} - 1}, summed in order STARTING FROM THE FIRST TERM, so adjacent kept rows
 *     give dt's own bits and the identity reproduces the batch.  Entries at and past nkeep (out_dt: nkeep - 1) are untouched.
 *     When nkeep > cap the first cap kept rows are written, STE_SIMPLIFY_TRUNCATED is set and nkeep stays the true count.  A
 *     compacted block is itself a resident fleet: a batch struct with B, Nmax = cap - 1, nsteps = nkeep - 1 and dt = out_dt is
 *     all a ste_*_metrics_f64 call reads of a batch.
 *   - Every value's bits depend on the track's rows, its dt, c, tol and the flag alone: not on S, the window, which outputs
 *     were asked for, or whether `work` was used.
 *   - The call reads only B, Nmax, track_stride, nsteps and dt of the batch and writes nothing of the batch; windows and
 *     addressing are those of ste_path_metrics_f64, tolerance and lon_scale like nsteps.  Rows past nsteps[t] of states are not
 *     read.  b->dt is required unless STE_SIMPLIFY_SHAPE is set and out_dt is NULL.
 *   - Work.  A track with more than ste_track_simplify_lds_rows() rows keeps X, Y, T and its flags in `work`;
 *     ste_track_simplify_workspace(Nmax, nstates, B) is the number of bytes these sizes need, 0 while Nmax + 1 <=
 *     ste_track_simplify_lds_rows().
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or sf NULL; states NULL; nstates < 1 or
 *     > 65535; flags with any other bit than STE_SIMPLIFY_SHAPE; reserved != 0; tolerance NULL and tolerance_all not finite or
 *     negative; lon_scale NULL and lon_scale_all not finite or negative; rows, out_states or out_dt given with cap == 0, or with
 *     cap outside 1 .. Nmax + 1; b->dt NULL where it is read; work NULL or work_bytes below ste_track_simplify_workspace(Nmax,
 *     nstates, B) when that is non-zero; every output NULL; B <= 0, Nmax < 0 or Nmax > 2^31 - 257, or track_stride non-zero and
 *     below B.
 */
#define STE_SIMPLIFY_SHAPE 0x1u       /* flags: the perpendicular distance to the chord, no clock (default: at the row's own time) */
#define STE_SIMPLIFY_BAD_TIME 0x1     /* status: a dt below nsteps that is not finite and >= 0 (clock mode) */
#define STE_SIMPLIFY_BAD_LIMIT 0x2    /* status: the track's tolerance or lon_scale is not finite or is < 0 */
#define STE_SIMPLIFY_BROKEN 0x4       /* status: a step of 90 degrees of longitude or more, or a latitude that is not finite */
#define STE_SIMPLIFY_TRUNCATED 0x8    /* status: nkeep > cap: the first cap kept rows were written */
typedef struct ste_simplify_f64 {
    int32_t nstates;         /* S >= 1 tracks per ship in `states` (<= 65535) */
    uint32_t flags;          /* STE_SIMPLIFY_SHAPE or 0 */
    int32_t cap;             /* rows of `rows`, `out_states` and `out_dt` (cap - 1); 1 .. Nmax + 1; read with one of them only */
    int32_t reserved;        /* must be 0 */
    const double* states;    /* DEVICE [S][Nmax+1][4][track_stride], as ste_path_f64; components 0 and 1 decide */
    const double* tolerance; /* DEVICE [track_stride]: degrees per track, or NULL: tolerance_all for every track */
    double tolerance_all;    /* degrees of a great circle, finite, >= 0 */
    const double* lon_scale; /* DEVICE [track_stride]: c per track, or NULL: lon_scale_all for every track */
    double lon_scale_all;    /* finite, >= 0; 1 = plain degrees, cos(lat) = a local equirectangular plane */
    double* work;            /* DEVICE scratch of work_bytes, see ste_track_simplify_workspace; may be NULL when that is 0 */
    int64_t work_bytes;
    uint8_t* keep;           /* DEVICE [S][Nmax+1][track_stride] or NULL: 1 / 0 for rows 0 .. nsteps[t] */
    int32_t* nkeep;          /* DEVICE [S][track_stride] or NULL: kept rows (the true count, also when truncated) */
    double* worst_sq;        /* DEVICE [S][track_stride] or NULL: the largest d2 of a range that was closed; NaN = identity */
    int32_t* status;         /* DEVICE [S][track_stride] or NULL: STE_SIMPLIFY_* bits */
    int32_t* rows;           /* DEVICE [S][cap][track_stride] or NULL: the m-th kept row */
    double* out_states;      /* DEVICE [S][cap][4][track_stride] or NULL: that row of states */
    double* out_dt;          /* DEVICE [S][cap-1][track_stride] or NULL: hours from kept row m to kept row m + 1 */
} ste_simplify_f64;          /* 128 bytes */

int ste_track_simplify_f64(const ste_ukf_batch_f64* b, const ste_simplify_f64* sf, void* stream);
/* bytes of `work` these sizes need; may be 0 */
size_t ste_track_simplify_workspace(int32_t Nmax, int32_t nstates, int32_t B);
/* rows of a track the kernel keeps in LDS; a track with more goes through `work` */
int ste_track_simplify_lds_rows(void);

/*
 * NOISE FIT: the measurement noise R of a track, or of a group of tracks, estimated from the data by EM (an unnumbered
 * addition, like ste_ukf_noise_f64, whose R stack it fills).  The E-step is a forward pass and a smoother; the M-step is
 *      R_new = 1/n sum_u [ (z_u - H m^s)(z_u - H m^s)^T + H P^s H^T ]
 * over the updates u of the track (group), m^s, P^s the smoothed row the update produced, followed by a projection onto the
 * structure R may have.  Two calls: the per-track sums of the terms, and the deterministic sum over a group with the projection.
 *
 * ste_ukf_noise_moments_f64 -- per-track sums, from a completed forward pass and smoother of the batch.
 *   - Updates.  An update is a step k < nsteps[t] with 0 <= upd_idx[k] < Tmax; its row is k + 1 and its observation column
 *     upd_idx[k] of z.  The initial update never counts: row 0 of the histories is the prior (kalman_filter.py:76), not the
 *     state that update produced.
 *   - Term of an update, every expression evaluated as written, left to right, without contraction (no fma):
 *         (Hm)_r = ((H_r0 m_0 + H_r1 m_1) + H_r2 m_2) + H_r3 m_3,   v = z - Hm,   v_3 = wrap180(v_3) (that of ste_path_f64)
 *         G_rc   = ((H_r0 P_0c + H_r1 P_1c) + H_r2 P_2c) + H_r3 P_3c,   P_ic the stored entry (min(i, c), max(i, c)) of sm_cov
 *         (GH)_rc = ((G_r0 H_c0 + G_r1 H_c1) + G_r2 H_c2) + G_r3 H_c3   for r <= c
 *         term_rc = v_r v_c + (GH)_rc                                    for r <= c, the ten entries in the order of STE_FLAG_PACKED_COV
 *     moments holds the sums of the terms, vsum the sums of v (the bias of the observations against the smoothed track), both
 *     starting from 0.0 and adding in ascending step order; count the number of updates summed.  A track's bits depend on
 *     its own rows only.
 *   - Unusable tracks have count 0 and zero sums: a track whose b->status carries STE_STATUS_NAN (STE_NOISE_TRACK_NAN; its
 *     rows are not read; b->status NULL = no track does), and a track with a non-finite term (STE_NOISE_TRACK_NOT_FINITE).
 *   - The call reads B, Nmax, Tmax, track_stride, flags (STE_FLAG_PACKED_COV), H (HOST, read at call time), nsteps (NULL =
 *     Nmax for every track), upd_idx, z, sm_mean, sm_cov and status of the batch and writes nothing of it.  Per-track arrays
 *     are addressed a[row * track_stride + t] with the pointers naming the window's first track; track_status is [B].
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or nm NULL; moments or count NULL; H, sm_mean,
 *     sm_cov, z or upd_idx NULL; STE_FLAG_ROBUST (the filter rescales R per update, and the M-step above is not defined);
 *     recorded noise (noise_upd non-NULL: the update saw z + noise); a time slice (step_begin != 0 or step_end not 0 or Nmax);
 *     nm->flags or nm->reserved non-zero; B <= 0, Nmax < 0, Tmax < 1, or track_stride non-zero and below B.
 */
#define STE_NOISE_TRACK_NAN 0x1        /* track_status: the batch's status carries STE_STATUS_NAN for this track */
#define STE_NOISE_TRACK_NOT_FINITE 0x2 /* track_status: a term of this track was not finite */
typedef struct ste_noise_moments_f64 {
    double* moments;       /* DEVICE [10][track_stride] out, required */
    int32_t* count;        /* DEVICE [track_stride] out, required: updates summed */
    double* vsum;          /* DEVICE [4][track_stride] out or NULL: sum of v */
    int32_t* track_status; /* DEVICE [B] out or NULL: STE_NOISE_TRACK_* bits (overwritten) */
    uint32_t flags;        /* must be 0 */
    uint32_t reserved;     /* must be 0 */
} ste_noise_moments_f64;   /* 40 bytes */

int ste_ukf_noise_moments_f64(const ste_ukf_batch_f64* b, const ste_noise_moments_f64* nm, void* stream);

/*
 * ste_ukf_noise_mstep_f64 -- the sums of a group's tracks, divided by the group's count and projected.  The order of the
 * additions is part of the definition, so R has the same bits in every run (an atomic sum over tracks would not).
 *   - Groups come as CSR: group g has the members group_members[group_offsets[g] .. group_offsets[g + 1]), indices of tracks
 *     in [0, ntracks); a track is a member of at most one group (the caller's promise; a track that is a member of none keeps
 *     its R).  nmembers is group_offsets[ngroups] as the host knows it; offsets are clamped to [0, nmembers], and a member
 *     outside [0, ntracks) is skipped and sets STE_NOISE_GROUP_BAD_MEMBER.  Both pointers NULL: every track is a group of its
 *     own (ngroups == ntracks, nmembers == 0).
 *   - Sums, for entries 00, 01 and 11 of moments (the others enter no structure and are not summed) and for count: a wave per
 *     group; lane l starts from 0.0 (0) and adds members l, l + 64, l + 128, ... of the group in that order; then for
 *     off = 32, 16, 8, 4, 2, 1 lane l < off adds lane l + off's value to its own; lane 0 holds the sums M and n.  With NULL
 *     groups a lane per track: 0.0 + the track's value.
 *   - Projection, with M_e = sum_e / (double)n.  Every structure confines R to the leading 2 x 2 block, so
 *     STE_NOISE_R_BLOCK2 holds for the result:
 *         STE_NOISE_FIT_SCALAR   r diag(1, 1, 0, 0), r = (M_00 + M_11) / 2.0
 *         STE_NOISE_FIT_DIAG2    diag(M_00, M_11, 0, 0)
 *         STE_NOISE_FIT_BLOCK2   entries 00, 01, 11 = M_00, M_01, M_11, the rest 0
 *   - Outputs.  R_group holds the projected triangle and n_group the count of every group, whatever its status (n = 0 gives
 *     NaN).  R_tracks receives the group's triangle for every member -- unless the group is EMPTY (n = 0) or has a BAD_VARIANCE
 *     (entry 00 or 11 of the projection not finite or <= 0, or entry 01 not finite): then group_status says so and the
 *     members' R_tracks keep their values.  Every output has one writer: plain vector stores.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: ms NULL; moments, count, R_group, n_group,
 *     group_status or R_tracks NULL; exactly one of group_offsets / group_members NULL; an unknown structure; reserved != 0;
 *     ntracks <= 0, ngroups <= 0 or nmembers < 0; ld non-zero and below ntracks; NULL groups with ngroups != ntracks.
 */
#define STE_NOISE_FIT_SCALAR 0
#define STE_NOISE_FIT_DIAG2 1
#define STE_NOISE_FIT_BLOCK2 2
#define STE_NOISE_GROUP_EMPTY 0x1        /* group_status: n = 0, nothing to divide by */
#define STE_NOISE_GROUP_BAD_VARIANCE 0x2 /* group_status: the projection is not a usable R */
#define STE_NOISE_GROUP_BAD_MEMBER 0x4   /* group_status: a member index outside [0, ntracks) was skipped */
typedef struct ste_noise_mstep_f64 {
    int32_t ntracks;              /* tracks in a row of moments / count / R_tracks */
    int32_t ngroups;              /* G */
    int32_t nmembers;             /* group_offsets[G]; 0 with NULL groups */
    int32_t structure;            /* STE_NOISE_FIT_* */
    int64_t ld;                   /* tracks per row of moments and R_tracks (the track_stride of call 1); 0 = ntracks */
    const double* moments;        /* DEVICE [10][ld], from ste_ukf_noise_moments_f64 */
    const int32_t* count;         /* DEVICE [ld] */
    const int32_t* group_offsets; /* DEVICE [G + 1] or NULL */
    const int32_t* group_members; /* DEVICE [nmembers] or NULL */
    double* R_group;              /* DEVICE [10][G] out */
    int32_t* n_group;             /* DEVICE [G] out */
    int32_t* group_status;        /* DEVICE [G] out: STE_NOISE_GROUP_* bits (overwritten) */
    double* R_tracks;             /* DEVICE [10][ld] in / out: ste_ukf_noise_f64.R of the batch */
    int64_t reserved;             /* must be 0 */
} ste_noise_mstep_f64;            /* 96 bytes */

int ste_ukf_noise_mstep_f64(const ste_noise_mstep_f64* ms, void* stream);

/*
 * FIELDS: the values of a SPACE-TIME GRIDDED FIELD (SST, pressure, wind, ice: [nt][ny][nx]) where tracks that stay on the
 * device were AT GIVEN CLOCK TIMES (an unnumbered addition, like ste_positions_f64): per (sample, query) the position of
 * POSITIONS is formed and the field is read there, trilinear in (time, lat, lon) with no-data handling or at the nearest node,
 * and the count, the moments and the extremes of the value OVER THE SAMPLES about an anchor are continued from call to call.
 * `states`, `nqueries`, `qtrack`, `qtime` and `t0` are those of ste_positions_f64.  wrap180, clamp01 and % are those of
 * POSITIONS, floor is the floor of a double, and every expression is evaluated as written, left to right, without contraction and
 * without transcendentals: the library and a NumPy restatement agree bit for bit.
 *   - Knots.  `knots` is what a previous ste_track_positions_f64 on this batch left in its workspace ([Nmax+1][track_stride]);
 *     it is read only, and this call never reads b->dt.  knots[0][t] = NaN marks a bad clock, as there.
 *   - Locate.  POSITIONS word for word: Bad index, Bad time, Locate, Knot hit, Interior and the BROKEN step, which give (lon, lat)
 *     per sample -- wrap180(lon_j), lat_j on a knot hit; wrap180(lon_k + u * delta), lat_k + u * (lat_{k+1} - lat_k) inside a
 *     sound step; NaN, NaN inside a broken one -- and the STE_POS_* bits of status[q] with their meaning.  A query that is not
 *     located gives NaN in value and cover of every sample and adds nothing to any accumulator.
 *   - Time, with tq = qtime[q].  Slab j of the field is valid at time0 + j * dtime.  With nt == 1 the field is static: it0 = it1 =
 *     0, ft = 0, and time is never outside.  Otherwise gt = (tq - time0) / dtime, and a located query for which
 *     gt >= 0 && gt <= nt - 1 is false gets STE_FLD_TIME_OUTSIDE: value and cover of every sample are NaN and nothing is
 *     counted; there is no extrapolation in time.  it = floor(gt); if it >= nt - 1 then it0 = it1 = nt - 1 and ft = 0, otherwise
 *     it0 = it, it1 = it + 1 and ft = gt - it.
 *   - Space.  Values sit at CELL CENTRES of the grid of ste_grid_f64 (GRIDS: Grid.): node (ix, iy) of slab j lies at
 *     (lon0 + (ix + 0.5) dlon, lat0 + (iy + 0.5) dlat) and is stored at values[(j * ny + iy) * nx + ix].  x = lon_ref +
 *     wrap180(lon - lon_ref), gx = (x - lon0) / dlon, gy = (lat - lat0) / dlat.  A sample whose lon or lat is not finite counts
 *     NOWHERE: value and cover are NaN.  A finite sample is ON THE GRID by the raster's cell test, 0 <= gy < ny and without
 *     STE_GRID_PERIODIC_LON also 0 <= gx < nx; a finite sample OFF THE GRID gives value NaN and cover 0 and adds 1 to count[2].
 *     On the grid hx = gx - 0.5, ix = floor(hx), fx = hx - ix.  Not periodic: ix < 0 puts both columns at 0 with fx = 0, and
 *     ix >= nx - 1 puts both at nx - 1 with fx = 0 (the outer half cell is a constant continuation).  Periodic: the columns are
 *     ix and ix + 1 modulo nx (floored).  Rows: hy = gy - 0.5, iy = floor(hy), fy = hy - iy, always by the non-periodic rule.
 *   - Value.  Corner c = 4 e + 2 b + a (e: slab it0 / it1, b: row, a: column) has the weight w = (wt_e * wy_b) * wx_a with
 *     wx_0 = 1 - fx, wx_1 = fx, wy_0 = 1 - fy, wy_1 = fy, wt_0 = 1 - ft, wt_1 = ft.  A corner with w == 0, or whose value is NaN, is
 *     skipped; for the others, in corner order from num = den = 0.0: num = num + w * v, den = den + w.  cover = den, and
 *     value = (den > 0 && den >= min_cover) ? num / den : NaN.  +-inf are values.  A sample on the grid whose value comes out NaN
 *     adds 1 to count[1].  A float field (STE_FLD_VALUES_F32) is converted to double, exactly, when it is read.
 *   - Nearest.  With STE_FLD_NEAREST the value is that of one node: the node of the cell (floor gx, floor gy) the sample lies in
 *     (the column modulo nx where periodic), exactly the cell of ste_raster_f64's row_value, in slab min(floor(gt + 0.5), nt - 1)
 *     (slab 0 when nt == 1).  cover is 1, or 0 where the node is NaN; min_cover is not consulted.
 *   - Moments.  For query q, for s = 0 .. S - 1 in order: if value is finite and d = value - vanchor[q] is finite, then
 *     count[0][q] += 1, moments[0][q] += d, moments[1][q] += d * d, if (!(vmin[q] <= value)) vmin[q] = value and
 *     if (!(vmax[q] >= value)) vmax[q] = value.  count, moments, vmin and vmax START FROM THE STORED VALUES and are stored once
 *     at the end: the caller zeroes the sums and puts NaN into vmin and vmax before the first call, and a call with S samples
 *     equals a call with the first S1 and a call with the other S - S1 on the same accumulators, bit for bit.
 *   - Every value's bits depend on its own track's rows, the knots, t0, the query, the field and (the accumulators) the stored
 *     values alone: not on Q, the place of the query in the list, S, the window, or which outputs were asked for.
 *   - The call reads only B, Nmax, track_stride and nsteps (NULL = Nmax for every track) of the batch and writes nothing of it;
 *     windows and addressing are those of ste_track_positions_f64.  Rows past nsteps[t] of states are not read.  Outputs per
 *     sample are out[s * Q + q]; count is [3][Q] (valid, nodata, off) and moments [2][Q].
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or f NULL; B <= 0, Nmax < 0, or track_stride
 *     non-zero and below B; states, qtrack, qtime, knots or values NULL; nstates < 1 or > 65535; nqueries < 1 or >
 *     STE_POSITIONS_MAX_QUERIES; unknown flag bits; the reserved word not 0; the grid refusals of ste_grid_metrics_f64 (nx, ny,
 *     the cells, lon0, lat0, lon_ref, dlon, dlat, the periodic and the non-periodic condition); nt < 1 or > STE_FIELD_MAX_SLABS;
 *     a non-finite time0; dtime not finite or <= 0 when nt > 1; min_cover not in [0, 1]; any of count, moments, vmin, vmax without
 *     vanchor; every output NULL.
 */
#define STE_FIELD_MAX_SLABS 65536
#define STE_FLD_NEAREST 0x2u       /* the value of the nearest node instead of the trilinear one */
#define STE_FLD_VALUES_F32 0x4u    /* `values` is float[nt][ny][nx] instead of double */
#define STE_FLD_TIME_OUTSIDE 0x8   /* status: the query is located but its time lies off the field's time axis */
typedef struct ste_field_f64 {
    int32_t nstates;        /* S >= 1 tracks per ship in `states` (<= 65535) */
    uint32_t flags;         /* STE_GRID_PERIODIC_LON | STE_FLD_NEAREST | STE_FLD_VALUES_F32; unknown bits refused */
    const double* states;   /* DEVICE [S][Nmax+1][4][track_stride], as ste_positions_f64 */
    int64_t nqueries;       /* Q, 1 .. STE_POSITIONS_MAX_QUERIES */
    const int32_t* qtrack;  /* DEVICE [Q]: track of the window, 0 <= t < B */
    const double* qtime;    /* DEVICE [Q]: clock time, hours */
    const double* t0;       /* DEVICE [track_stride] or NULL (= 0): clock time of row 0 of each track */
    const double* knots;    /* DEVICE [Nmax+1][track_stride], read only: what ste_track_positions_f64 left there */
    int32_t nx, ny;         /* columns (lon) and rows (lat), >= 1, nx * ny <= STE_GRID_MAX_CELLS */
    int32_t nt;             /* slabs, 1 .. STE_FIELD_MAX_SLABS; 1 = a static field */
    uint32_t reserved;      /* must be 0 */
    double lon0, lat0;      /* HOST: west and south edge of cell (0, 0), degrees, as ste_grid_f64 */
    double dlon, dlat;      /* HOST: cell size, finite, >= 1e-6 */
    double lon_ref;         /* HOST: meridian the longitudes are unwrapped about */
    double time0, dtime;    /* HOST: slab j is valid at time0 + j * dtime hours on the queries' clock; dtime > 0 when nt > 1 */
    double min_cover;       /* HOST: in [0, 1]: the least weight of valid corners a value needs */
    const void* values;     /* DEVICE [nt][ny][nx]: double, or float with STE_FLD_VALUES_F32; NaN = no data */
    const double* vanchor;  /* DEVICE [Q]: required with count, moments, vmin or vmax */
    double* value;          /* DEVICE [S][Q] or NULL */
    double* cover;          /* DEVICE [S][Q] or NULL: the weight of the valid corners, 0 off the grid */
    int32_t* status;        /* DEVICE [Q] or NULL: STE_POS_* bits and STE_FLD_TIME_OUTSIDE */
    int32_t* count;         /* DEVICE [3][Q], ACCUMULATED (+=), or NULL: samples that are valid, nodata, off the grid */
    double* moments;        /* DEVICE [2][Q], ACCUMULATED, or NULL: sums of d and d * d, d = value - vanchor */
    double* vmin;           /* DEVICE [Q], continued from the stored value (NaN = none yet), or NULL */
    double* vmax;           /* DEVICE [Q], continued likewise, or NULL */
} ste_field_f64;            /* 208 bytes */

int ste_field_values_f64(const ste_ukf_batch_f64* b, const ste_field_f64* f, void* stream);

/*
 * LAG-ONE COVARIANCE of the unscented smoother (an unnumbered addition, like ste_ukf_sample_f64).  sm_mean / sm_cov are the
 * marginals of every row; what two NEIGHBOURING rows have in common is the third output of an RTS smoother (Shumway-Stoffer):
 *      L_k = Cov(x_k, x_{k+1} | all data) = K_k P^s_{k+1},      k = 0 .. nsteps - 1
 * with K_k = D pinv(P_b) the gain of step k exactly as the smoother forms it and P^s_{k+1} row k + 1 of sm_cov.  Under the
 * sampler's recursion x_k = (m_k + K y) + T xi this is the cross-covariance of rows k and k + 1 of the sampled tracks.  The
 * product is formed entry by entry, L[r][c]: acc = K[r][0] * P[0][c]; acc = fma(K[r][i], P[i][c], acc) for i = 1, 2, 3, with
 * P[i][c] read from the upper triangle of the stored row; nothing else is contracted.
 *   - lag1: entry 4 r + c of row k holds L_k[r][c] (L is not symmetric: all 16).  With STE_LAG1_POSITION a row has 4 entries,
 *     L[0][0], L[0][1], L[1][0], L[1][1] -- all the covariance of a position needs, a quarter of the memory -- with the bits of the
 *     same entries of the full form.  Rows k >= nsteps[t] are left as they were.
 *   - Precondition: a completed forward pass of this batch WITH rts_work, and a completed smoother (sm_cov holds the smoothed
 *     covariances), in either of its forms.  The call only reads the batch: rts_work, the histories and b->status are not written.
 *     nz: the per-track Q the forward pass ran with (NULL, or nz->Q NULL: the shared b->Q); nz->R and nz->flags are not read.
 *   - Ordering: the call reads rts_work.  A two-kernel smoother (ste_urtss_backward_f64 on a small batch) REWRITES the work rows
 *     into gains; when it runs on another stream the caller orders this call before or after it, never beside it -- and after
 *     whatever writes sm_cov.
 *   - Windows: track_stride works like for every other per-track array -- lag1 has rows of track_stride tracks and the pointer
 *     names the window's first track; status is [B] and points at the window's first entry.
 *   - Refused with STE_EINVAL and a message before any launch: b, lg or lg->lag1 NULL; unknown flag bits; reserved != 0; rts_work,
 *     fwd_mean or fwd_cov NULL; step_begin / step_end naming a slice; and whatever ste_urtss_backward_f64 refuses (sm_mean /
 *     sm_cov NULL among it).  STE_FLAG_LANES_1 / _4 are ignored.
 */
#define STE_LAG1_POSITION 0x1u /* lag1 rows hold the 4 entries of the lon / lat block instead of all 16 */
typedef struct ste_lag_one_f64 {
    double* lag1;      /* DEVICE [Nmax][16][track_stride] out; [Nmax][4][track_stride] with STE_LAG1_POSITION */
    int32_t* status;   /* DEVICE [B] out or NULL: cleared, then STE_STATUS_NAN (a non-finite entry of L) and what the gain solve
                          reports (STE_STATUS_NOCONV) are ORed in */
    uint32_t flags;    /* STE_LAG1_POSITION; unknown bits refused */
    uint32_t reserved; /* must be 0 */
} ste_lag_one_f64;     /* 24 bytes */

int ste_urtss_lag_one_f64(const ste_ukf_batch_f64* b, const ste_ukf_noise_f64* nz, const ste_lag_one_f64* lg, void* stream);

/*
 * POSITION COVARIANCE: how well the position of ste_track_positions_f64 is known, WITHOUT SAMPLES (an unnumbered addition, like
 * ste_lag_one_f64).  POSITIONS interpolates linearly inside a step, so the covariance of the interpolated state at fraction u of
 * step k follows from rows k and k + 1 of the smoothed covariance and the lag-one block between them:
 *      P(u) = (1 - u)^2 P^s_k + u^2 P^s_{k+1} + (1 - u) u (L_k + L_k^T)
 * `nqueries`, `qtrack`, `qtime`, `t0` are those of ste_positions_f64 and `knots` is that of ste_field_f64: what a previous
 * ste_track_positions_f64 on this batch left in its workspace, read only.  The call reads no states.
 *   - Locate.  POSITIONS word for word: Bad index, Bad time, Locate; the same step[q], frac[q] and STE_POS_* bits of status[q].
 *     The call never extrapolates.
 *   - cov has the layout of the batch's histories: [Nmax+1][16][track_stride], or upper triangles [Nmax+1][10][track_stride] with
 *     STE_FLAG_PACKED_COV in b->flags; of a full matrix the entries with r <= c are read.  sm_cov is what a caller passes.
 *     lag1 is what ste_urtss_lag_one_f64 wrote, in either form; STE_PCOV_LAG1_POSITION says it is the 4-entry one.
 *   - Interior, with w1 = u, w0 = 1 - u, A row step[q] of cov, B row step[q] + 1 and L row step[q] of lag1:
 *          P_rc = ((w0 * w0) * A_rc + (w1 * w1) * B_rc) + (w0 * w1) * (L_rc + L_cr)
 *     evaluated as written, without contraction: the library and a NumPy restatement agree bit for bit.
 *   - Knot hit on row j: P_rc = A_rc of row j, copied; the neighbouring row and lag1 are not read.
 *   - Not located (a bad index, a bad time, outside): NaN in every entry.  A broken step (POSITIONS: Interior) is a property of
 *     the states, which this call does not read: the caller masks with the position's own NaN.
 *   - pcov is [3][Q]: lon-lon, lon-lat, lat-lat in degrees squared, pcov[e * Q + q].  With STE_PCOV_FULL it is [10][Q], the upper
 *     triangle of the 4 x 4 in the order of STE_FLAG_PACKED_COV; that needs the 16-entry lag1.  The three entries the two forms
 *     share (0 / 0, 1 / 1, 2 / 4) have the same bits.
 *   - Every value's bits depend on the track's rows of cov and lag1, the knots, t0 and the query alone: not on Q, the place of the
 *     query in the list, the window, the layout of cov or lag1, or which outputs were asked for.  Every output word has one
 *     writer; there are no atomics.
 *   - The call reads only B, Nmax, track_stride, flags (STE_FLAG_PACKED_COV) and nsteps (NULL = Nmax for every track) of the
 *     batch and writes nothing of it; windows and addressing are those of ste_track_positions_f64, with cov and lag1 in rows of
 *     track_stride tracks and their pointers at the window's first track.  Rows past nsteps[t] of cov and lag1 are not read.
 *   - Refused with STE_EINVAL and a message naming the call, before any launch: b or pc NULL; B <= 0, Nmax < 0, or track_stride
 *     non-zero and below B; qtrack, qtime or knots NULL; nqueries < 1 or > STE_POSITIONS_MAX_QUERIES; unknown flag bits; reserved
 *     != 0; STE_PCOV_FULL together with STE_PCOV_LAG1_POSITION; every output NULL; pcov without cov, or without lag1 when Nmax > 0.
 */
#define STE_PCOV_FULL 0x1u          /* pcov is [10][Q], the whole 4 x 4 (upper triangle); needs the 16-entry lag1 */
#define STE_PCOV_LAG1_POSITION 0x2u /* lag1 is the 4-entry form (STE_LAG1_POSITION) */
typedef struct ste_position_cov_f64 {
    uint32_t flags;         /* STE_PCOV_FULL | STE_PCOV_LAG1_POSITION; unknown bits refused */
    uint32_t reserved;      /* must be 0 */
    int64_t nqueries;       /* Q, 1 .. STE_POSITIONS_MAX_QUERIES */
    const int32_t* qtrack;  /* DEVICE [Q]: track of the window, 0 <= t < B */
    const double* qtime;    /* DEVICE [Q]: clock time, hours */
    const double* t0;       /* DEVICE [track_stride] or NULL (= 0): clock time of row 0 of each track */
    const double* knots;    /* DEVICE [Nmax+1][track_stride], read only: what ste_track_positions_f64 left there */
    const double* cov;      /* DEVICE [Nmax+1][16 or 10][track_stride]: sm_cov, in the layout b->flags names; required with pcov */
    const double* lag1;     /* DEVICE [Nmax][16 or 4][track_stride]: what ste_urtss_lag_one_f64 wrote; required with pcov */
    double* pcov;           /* DEVICE [3][Q] or NULL; [10][Q] with STE_PCOV_FULL: degrees squared (and the other units) */
    int32_t* step;          /* DEVICE [Q] or NULL: row of a knot hit, or k; -1 = not located */
    double* frac;           /* DEVICE [Q] or NULL: 0 on a knot hit, or u; NaN = not located */
    int32_t* status;        /* DEVICE [Q] or NULL: STE_POS_* bits */
} ste_position_cov_f64;     /* 96 bytes */

int ste_track_position_cov_f64(const ste_ukf_batch_f64* b, const ste_position_cov_f64* pc, void* stream);

/* ---- 0.3.2 -------------------------------------------------------------------------------------------------------
 * The forward passes of MANY windows (or batches) as ONE launch.  The reference's batch dimension is its per-ship loop
 * (examples/example_ukf_rts_smoother_batch.py:19-90); a fleet goes through the GPU as windows (track_stride above), and
 * with one launch per window a forward wave -- 64 tracks for the whole pass -- is indivisible: W windows of T tiles on S
 * SIMDs cost ceil(W T / S) pass times for W T / S pass times of work.  Here the unit is a (64-track tile, time slice) item,
 * the launch is `nwaves` resident waves (one per SIMD the stream may use), and `items` says which item every wave runs in
 * every round.  A tile's slices may run on different waves: each slice starts from the history row the one before it
 * left (the slices of ste_ukf_forward_f64: same bits as a whole pass); where a tile changes waves the finished slice
 * publishes the tile's slice count once its rows are in memory (release, agent scope) and the next slice waits for that
 * count (acquire) -- always an item of an EARLIER round; slices that follow one another on one wave are run as ONE item over
 * the whole step range, with no hand-over at all (the library finds those runs in the table).  The library checks the table
 * (every tile of every window runs all its slices, in order, at most one per round) before anything is launched, and
 * every in-kernel wait is bounded: a launch that cannot progress sets *error and ends.
 *
 * window_done[w] counts the finished tiles of window w: ste_stream_wait_counter(window_done + w, tiles of w, ...) on another
 * stream holds that stream until the window's forward pass is complete (its smoother goes behind it).
 *
 * All windows must take the same kernel (same H / R structure, robust flag, rts_work present or not); lane-per-track
 * mapping only.  host_ws should be page-locked (hipHostMalloc / hipHostRegister): a kernel on `stream` then reads the table
 * from it in place, and nothing but kernels sits between two launches; pageable memory goes through a staged copy.  Either
 * way it must stay untouched until the launch has started; dev_ws is filled by the call's own stream operations.  window_done,
 * error and started must be ZERO when the launch starts: the caller clears them on `stream` before the call (and orders
 * every stream that will wait on a counter behind that clearing), the call does not.
 *
 * Residency.  A wave may wait for any other wave of its launch, so all `nwaves` must be on the chip together.  One such
 * launch at a time gets there by itself; two that are dispatched together can each take part of the SIMDs and wait for
 * the rest until their bounds expire.  `started` (optional) counts the waves of this launch that have begun: put
 * ste_stream_wait_counter(started of the launch before, its nwaves, ...) on the stream in front of the next call and the
 * next launch is not dispatched before the one before it is resident (SmootherPipeline does, across pipelines of a process;
 * launches of different processes on one device are the caller's to keep apart). */
typedef struct ste_fwd_sched_f64 {
    int32_t nwindows;
    const ste_ukf_batch_f64* windows; /* HOST [nwindows]; step_begin = step_end = 0 */
    int32_t slice_steps;              /* steps per time slice, a multiple of STE_SLICE_ALIGN; 0 = STE_SLICE_ALIGN */
    int32_t nwaves;                   /* waves of the launch; all must be resident at once: <= SIMDs the stream may use */
    int32_t nrounds;
    const int32_t* items;             /* HOST [nrounds][nwaves][2]: (window, tile of that window), window < 0 = idle */
    void* host_ws;                    /* HOST scratch (page-locked if possible), ws_bytes (ste_ukf_forward_sched_workspace) */
    void* dev_ws;                     /* DEVICE scratch, ws_bytes */
    size_t ws_bytes;
    int32_t* window_done;             /* DEVICE [nwindows], zero at launch */
    int32_t* error;                   /* DEVICE [1], zero at launch: 1 = a forward wait timed out, 2 = a gate (wait_counter) did */
    double timeout_s;                 /* bound of one in-kernel wait; 0 = 2 s */
    int32_t* started;                 /* DEVICE [1] or NULL, zero at launch: waves of this launch that have begun */
} ste_fwd_sched_f64;

/* bytes of host_ws / dev_ws for a schedule of that shape (max_slices = largest ceil(Nmax / slice_steps) over the windows, at
 * least 1).  The launch lays its workspace out by these five numbers alone -- room for max_slices (max_slices + 1) / 2
 * parameter blocks for EVERY window, the item table, the per-tile counters -- whether or not the windows all have max_slices
 * slices: a ws_bytes below this size is refused, and the counters sit at ste_ukf_forward_sched_progress_offset (below) of the
 * same five numbers for any mix of window lengths. */
size_t ste_ukf_forward_sched_workspace(int32_t nwindows, int32_t max_slices, int64_t ntiles_total, int32_t nrounds,
                                       int32_t nwaves);
int ste_ukf_forward_sched_f64(const ste_fwd_sched_f64* sc, void* stream);

/* Holds `stream` (a one-wave kernel) until *counter >= need; after timeout_s (0 = 2 s) it gives up and sets *error = 2. */
int ste_stream_wait_counter(const int32_t* counter, int32_t need, int32_t* error, double timeout_s, void* stream);

/* The smoothers of every window of a scheduled forward launch as ONE launch: a wave per (window, 64-track tile) that waits
 * (bounded; *error = 2) until the forward launch has finished THAT tile's last slice and then smooths it -- the reference's
 * run_rts_smoother (kalman_filter.py:119-137) per track, started as soon as the track's forward pass is complete instead of
 * when its whole window's is.  `items` lists every tile of every window once, in the order the forward schedule finishes
 * them (waves are dispatched in that order).  `progress` is the forward launch's per-tile slice counter array: dev_ws of that
 * launch + ste_ukf_forward_sched_progress_offset(same arguments as ste_ukf_forward_sched_workspace) -- that is where the
 * forward launch zeroes and counts, for windows of equal and of unequal slice counts alike; int32 [ntiles_total], window by
 * window, each ending at its window's slice count.  Every window must take
 * the one-kernel smoother (rts_work; more than 4096 tracks, or tuning bit 10) and agree on sog_rate_rts / cog_rate_rts.
 * Waiting waves hold a wave slot each: put ste_stream_wait_counter(started of the forward launch, its nwaves, ...) on `stream`
 * in front of this call, so that every forward wave has its SIMD before a waiting smoother wave could be in its way.  Results
 * are those of ste_urtss_backward_f64 on every window, bit for bit. */
typedef struct ste_bwd_sched_f64 {
    int32_t nwindows;
    const ste_ukf_batch_f64* windows; /* HOST [nwindows], the forward launch's windows */
    int32_t slice_steps;              /* as in the forward launch */
    int32_t nitems;                   /* tiles of all windows */
    const int32_t* items;             /* HOST [nitems][2]: (window, tile of that window) */
    void* host_ws;                    /* HOST scratch (page-locked if possible), ws_bytes (ste_urtss_backward_sched_workspace) */
    void* dev_ws;                     /* DEVICE scratch, ws_bytes */
    size_t ws_bytes;
    const int32_t* progress;          /* DEVICE: the forward launch's per-tile slice counters */
    int32_t* error;                   /* DEVICE [1]: the forward launch's error word */
    double timeout_s;                 /* bound of a wave's wait; 0 = 2 s */
} ste_bwd_sched_f64;

/* byte offset of the forward launch's per-tile counters in its dev_ws: ste_ukf_forward_sched_workspace of the same arguments
 * less the counters themselves (4 bytes per tile, rounded up to 16) */
size_t ste_ukf_forward_sched_progress_offset(int32_t nwindows, int32_t max_slices, int64_t ntiles_total, int32_t nrounds,
                                             int32_t nwaves);
size_t ste_urtss_backward_sched_workspace(int32_t nwindows, int64_t ntiles_total);
int ste_urtss_backward_sched_f64(const ste_bwd_sched_f64* sc, void* stream);

/* Unscented RTS smoother: reads fwd_mean/fwd_cov, writes sm_mean/sm_cov, ORs status. */
int ste_urtss_backward_f64(const ste_ukf_batch_f64* b, void* stream);

/* Forward then backward on the same stream. */
int ste_ukf_urtss_f64(const ste_ukf_batch_f64* b, void* stream);

/*
 * Great-circle process model on `count` independent states.
 * x, out: [4][count]; dt, sog_rate, cog_rate: [count].
 */
int ste_geodetic_dynamics_f64(int64_t count, const double* x, const double* dt, const double* sog_rate,
                              const double* cog_rate, double* out, void* stream);

/*
 * One UKF predict on `count` independent (x, P) pairs.  x, x_out: [4][count]; P, P_out: [16][count];
 * dt, sog_rate, cog_rate: [count]; noise: [4][count] or NULL; Q: HOST 4x4; status: [count] or NULL.
 */
int ste_ukf_predict_f64(int64_t count, const double* x, const double* P, const double* dt, const double* sog_rate,
                        const double* cog_rate, const double* noise, const double* Q, double fan_scale, double w0,
                        double wi, double* x_out, double* P_out, int32_t* status, void* stream);

/*
 * One linear-KF update (pinv gain, heading wrap, Joseph form) on `count` independent (x, P) pairs with observations
 * z: [4][count]; noise: [4][count] or NULL (added to z); H, R: HOST 4x4.
 */
int ste_ukf_update_f64(int64_t count, const double* x, const double* P, const double* z, const double* noise,
                       const double* H, const double* R, double* x_out, double* P_out, int32_t* status, void* stream);

/*
 * Terms of the robustification helpers for `count` independent (x, P, z) triples, with y = z - x as the reference
 * writes it: gamma = |y^T (H P H^T + R)^+ y| (criterion_index, unscented.py:389-428) and
 * denom = y^T S^+ R S^+ y (update_lambda_factor, :468-478).  H, R: HOST 4x4.
 */
int ste_ukf_robust_terms_f64(int64_t count, const double* x, const double* P, const double* z, const double* H,
                             const double* R, double* gamma, double* denom, void* stream);

/*
 * Sigma fans of `count` (x, P) pairs: out[j][c][i] for sigma point j in 0..8, component c, pair i.
 * x: [4][count]; P: [16][count]; out: [9][4][count].  scale = n/(1-W0) (n when weights were never computed).
 */
int ste_sigma_points_f64(int64_t count, const double* x, const double* P, double scale, double* out, void* stream);

/*
 * Same for a general state dimension 1 <= n <= 16 (the reference's constructor and compute_sigma_points accept any n;
 * its unit tests use n = 2).  x: [n][count]; P: [n*n][count]; out: [2n+1][n][count].  Not a hot path.
 */
int ste_sigma_points_generic_f64(int32_t n, int64_t count, const double* x, const double* P, double scale, double* out,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Second kernel set: Gaussian-process regression (reference: src/track_estimators/gaussian_processes/
 * gaussian_process.py:28-89, a wrapper over scikit-learn's GaussianProcessRegressor).  One batch = B independent tracks;
 * track b has n[b] observations at 1-D inputs x (cumulative time, gaussian_process.py:53-58) with nout outputs
 * (lon, lat: :66) and its own kernel hyper-parameters theta = log(constant, length_scale, noise) of
 * ConstantKernel * K + WhiteKernel, K = RBF (examples/example_gaussian_process_batch.py:41) or a Matern kernel with
 * nu = 1/2, 3/2, 5/2 (scikit-learn's Matern), the same K for the whole batch (ste_gp_batch_f64.kernel).
 * Matrices are row-major [B][ld][ld] with ld = 64 * ceil(nmax / 64) + STE_GP_LD_PAD (the pad keeps consecutive rows off
 * the same HBM channel when 64 * ceil(nmax / 64) is a power of two); all buffers are caller-owned device memory.
 * ------------------------------------------------------------------------------------------------------------- */
#define STE_GP_LD_PAD 16
#define STE_GP_INVERSE_AUTO 0 /* column order (one workgroup per matrix) when B >= 128, else row order (nb workgroups per matrix) */
#define STE_GP_INVERSE_ROWS 1
#define STE_GP_INVERSE_COLS 2
/* ste_gp_batch_f64.kernel, with d = |xi - xj| / length_scale:                                     d k / d log(length_scale):
 *   RBF       exp(-d^2/2)                                                                          d^2 exp(-d^2/2)
 *   MATERN12  exp(-d)                                                                              d exp(-d)
 *   MATERN32  (1 + sqrt(3) d) exp(-sqrt(3) d)                                                      3 d^2 exp(-sqrt(3) d)
 *   MATERN52  (1 + sqrt(5) d + 5 d^2/3) exp(-sqrt(5) d)                                            (5/3) d^2 (1 + sqrt(5) d) exp(-sqrt(5) d) */
#define STE_GP_KERNEL_RBF 0
#define STE_GP_KERNEL_MATERN12 1
#define STE_GP_KERNEL_MATERN32 2
#define STE_GP_KERNEL_MATERN52 3

typedef struct ste_gp_batch_f64 {
    int32_t B;     /* number of tracks */
    int32_t nmax;  /* padded number of observations */
    int32_t nout;  /* output columns of y (2: lon, lat) */
    int32_t inverse_order; /* which kernel forms U = L^-T: STE_GP_INVERSE_AUTO (0: by B, see below), _ROWS (1), _COLS (2).  The two
                              sum in different orders, so objectives that must agree bit for bit (a track's first start and
                              its restarts in a replicated batch) have to name the same one */
    double jitter; /* added to the diagonal of K (GaussianProcessRegressor alpha, 1e-10) */
    const int32_t* n;    /* [B] observations per track */
    const double* x;     /* [B][nmax] */
    const double* y;     /* [B][nout][nmax] */
    const double* theta; /* [B][3] log(constant), log(length_scale), log(noise) */
    double* K;      /* [B][ld][ld]  K(X,X) + (noise + jitter) I (ste_gp_rbf_kmatrix_f64), then its Cholesky factor L (lower triangle,
                       diagonal included; what is above the diagonal is not defined).  ste_gp_lml_f64 evaluates the kernel
                       function inside the factorisation and leaves L here without K ever being stored */
    double* U;      /* [B][ld][ld]  workspace: L^-T (upper triangle) */
    double* Dinv;   /* [B][(ld-16)/64][64][64] workspace: inverses of the diagonal blocks of L */
    double* Kinv;   /* [B][ld][ld] K^-1 (both triangles) when non-NULL; needed by ste_gp_predict_f64 and ste_gp_predict_cov_f64 */
    double* alpha;  /* [B][nout][nmax] out: K^-1 y (after ste_gp_potrf_f64 alone: the forward substitution L^-1 y, which rides along
                       with the factorisation) */
    double* lml;    /* [B] out: log marginal likelihood summed over outputs */
    double* grad;   /* [B][3] out: d lml / d theta, or NULL to skip the gradient */
    double* tr;     /* [B][3][nt] workspace, nt = nb(nb + 1)/2 with nb = ceil(nmax/64): per-tile partial traces (summed in tile order) */
    int32_t* status; /* [B] out: 0 ok, 1 = K not positive definite */
    int32_t kernel;  /* 0.3.3: STE_GP_KERNEL_* (0, RBF, in a zero-initialised struct); any other value is refused with STE_EINVAL */
} ste_gp_batch_f64;

const char* ste_gp_last_error(void);

/* K(X,X) build only (lower 64x64 tiles + identity padding) -- sklearn kernel __call__.  Despite the name it builds whichever
 * kernel `kernel` names (RBF: exp(-pdist^2/2)). */
int ste_gp_rbf_kmatrix_f64(const ste_gp_batch_f64* b, void* stream);

/* In-place blocked Cholesky of the K that ste_gp_rbf_kmatrix_f64 left in the buffer (scipy.linalg.cholesky(K, lower=True) in
 * GaussianProcessRegressor); also writes L^-1 y to alpha and the inverted diagonal blocks to Dinv. */
int ste_gp_potrf_f64(const ste_gp_batch_f64* b, void* stream);

/*
 * One objective evaluation per track (GaussianProcessRegressor.log_marginal_likelihood(theta, eval_gradient=True)):
 * Cholesky of K (the kernel function evaluated in place of a stored K; same values as ste_gp_rbf_kmatrix_f64), L^-T, alpha,
 * lml, and -- when grad != NULL -- the gradient via K^-1 = L^-T L^-1 reduced against dK/dtheta on the fly.
 */
int ste_gp_lml_f64(const ste_gp_batch_f64* b, void* stream);

/* The same evaluation for `count` of the batch's matrices only: active[count] (DEVICE int32, distinct indices in
 * [0, B)) names them.  Outputs of the other matrices are left untouched.  This is what a lock-step batched optimiser
 * uses once some of its tracks have converged (scipy's L-BFGS-B stops per track, gaussian_process.py:63-66 via
 * scikit-learn's _constrained_optimization); per-matrix results do not depend on which other matrices are listed. */
int ste_gp_lml_subset_f64(const ste_gp_batch_f64* b, int32_t count, const int32_t* active, void* stream);

/*
 * Posterior mean [B][nout][mmax] and variance [B][mmax] at m[b] new inputs xs [B][mmax]
 * (GaussianProcessRegressor.predict(return_std=True); std = sqrt(max(var, 0)) is left to the caller).
 * Needs alpha and Kinv from a preceding ste_gp_lml_f64 on the same batch.  Kstar: workspace [B][64*ceil(mmax/64)][ld].
 */
int ste_gp_predict_f64(const ste_gp_batch_f64* b, int32_t mmax, const int32_t* m, const double* xs, double* Kstar,
                       double* mean, double* var, void* stream);

/*
 * Posterior mean [B][nout][mmax] and covariance [B][mmax][mmax] at m[b] new inputs xs [B][mmax]
 * (GaussianProcessRegressor.predict(return_cov=True)):
 *   cov = c k(xs_i - xs_j) + s [i == j] - Kstar K^-1 Kstar^T      (the WhiteKernel adds s on the diagonal only)
 * Needs alpha and Kinv from a preceding ste_gp_lml_f64 on the same batch.  Kstar, W: workspaces [B][64*ceil(mmax/64)][ld].
 * The mean is ste_gp_predict_f64's, bit for bit; mean rows >= m[b] are not written.  Every element of a track's
 * [mmax][mmax] block of cov is written: both triangles (the upper one mirrors the lower one bit for bit), 0 in rows and
 * columns >= m[b].  Per-track results do not depend on the other tracks of the batch.
 */
int ste_gp_predict_cov_f64(const ste_gp_batch_f64* b, int32_t mmax, const int32_t* m, const double* xs, double* Kstar,
                           double* W, double* mean, double* cov, void* stream);

/*
 * Posterior of the time derivative f'(t) of the latent function (the velocity of a track: deg/h for lon / lat against
 * hours) at m[b] new inputs xs [B][mmax].  The derivative of a GP is a GP; with c, l, s = exp(theta), d = (t - x) / l and
 * k(t, x) = c kappa(d) for the batch's kernel function:
 *   kind        kappa'(d)                                         q = -kappa''(0)   -kappa''(d)
 *   RBF         -d exp(-d^2/2)                                    1                 (1 - d^2) exp(-d^2/2)
 *   MATERN32    -3 d exp(-sqrt(3) |d|)                            3                 3 (1 - sqrt(3) |d|) exp(-sqrt(3) |d|)
 *   MATERN52    -(5/3) d (1 + sqrt(5) |d|) exp(-sqrt(5) |d|)      5/3               (5/3) (1 + sqrt(5) |d| - 5 d^2) exp(-sqrt(5) |d|)
 *   MATERN12    not differentiable: refused with STE_EINVAL
 *   K'*[j][i] = (c / l) kappa'((xs_j - x_i) / l)      (0 in padding columns i >= n[b] and rows j >= m[b], as Kstar)
 *   dmean     = K'* alpha                              [B][nout][mmax], per output
 *   dvar_j    = c q / l^2 - (K'* K^-1 K'*^T)_jj       [B][mmax]
 *   dcov_ij   = (c / l^2) (-kappa''((xs_i - xs_j) / l)) - (K'* K^-1 K'*^T)_ij
 * This is the latent derivative: the WhiteKernel adds nothing (no + s, unlike the position variance).
 * Layouts, workspaces and preconditions are those of ste_gp_predict_f64 / ste_gp_predict_cov_f64 (Kinv and alpha from a
 * preceding ste_gp_lml_f64; Kstar and W are the same workspaces and hold K'* and K'* K^-1 afterwards).  Rows >= m[b] of
 * dmean and dvar are not written; every element of a track's [mmax][mmax] block of dcov is written, both triangles
 * mirrored bit for bit, 0 outside [0, m[b])^2.  The two calls' dmean agree bit for bit, and per-track results do not
 * depend on the other tracks of the batch.  Every argument the position calls refuse, and kernel == MATERN12, is refused
 * with STE_EINVAL before any launch.
 */
int ste_gp_predict_deriv_f64(const ste_gp_batch_f64* b, int32_t mmax, const int32_t* m, const double* xs, double* Kstar,
                             double* dmean, double* dvar, void* stream);
int ste_gp_predict_deriv_cov_f64(const ste_gp_batch_f64* b, int32_t mmax, const int32_t* m, const double* xs,
                                 double* Kstar, double* W, double* dmean, double* dcov, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Observation preparation: speed / course over ground and their rates for a batch of tracks, the
 * device counterpart of ShipTrack.calculate_sog (ship_track.py:197-224), calculate_sog_rate (:226-250),
 * calculate_cog (:252-278), calculate_cog_rate (:280-304) and get_measurements(include_sog=True, include_cog=True)
 * (:306-338).  Arrays are [Tmax][B], track index fastest; observation i >= nobs[t] of a short track is written as 0.
 *   sog[i]      = distance(i, i+1) / gap[i]   (km/h), last value repeated;  gap = 0 gives inf / NaN as in the reference
 *   cog[i]      = heading(i, i+1)             (degrees in [0, 360)), last value repeated
 *   *_rate[i]   = (v[i] - v[i-1]) / gap[i-1], 0 for i = 0
 *   z[i][0..3]  = lon, lat, sog, cog          (optional; the layout ste_ukf_batch_f64.z consumes)
 * A track with fewer than 2 observations has no leg: all outputs 0 (the reference raises IndexError there).
 * ------------------------------------------------------------------------------------------------------------- */
#define STE_PREP_SPHERE 0 /* haversine_formula + heading on the 6378.137 km sphere (utils.py:75-147) */
#define STE_PREP_STATUS_NOCONV 0x1 /* reserved: up to 0.3.0 the WGS84 model used Vincenty's iteration, which does not converge
                                      for nearly antipodal points, and flagged such legs here; Karney's solver (0.3.1) solves
                                      every leg and never sets it */
#define STE_PREP_WGS84 1  /* geographiclib_distance + geographiclib_heading semantics (utils.py:9-72): WGS84 inverse
                             geodesic by Karney's algorithm (J. Geodesy 87, 2013), what geographiclib implements */

typedef struct ste_prep_batch_f64 {
    int32_t B;            /* tracks */
    int32_t Tmax;         /* observations per track (padded) */
    int32_t model;        /* STE_PREP_* */
    int32_t reserved;
    const int32_t* nobs;  /* [B] observations per track, NULL = Tmax for all */
    const double* lon;    /* [Tmax][B] degrees */
    const double* lat;    /* [Tmax][B] degrees */
    const double* gap;    /* [Tmax-1][B] hours between observation i and i+1 (ShipTrack.dts) */
    double* sog;          /* [Tmax][B] out */
    double* cog;          /* [Tmax][B] out */
    double* sog_rate;     /* [Tmax][B] out */
    double* cog_rate;     /* [Tmax][B] out */
    double* z;            /* [Tmax][4][B] out, may be NULL */
    int32_t* status;      /* [B] out, may be NULL: STE_PREP_STATUS_* bits per track (reset by the call) */
} ste_prep_batch_f64;

int ste_track_prep_f64(const ste_prep_batch_f64* b, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Pre-smoothing: the same preparation with SOG and / or COG smoothed BEFORE the rates and z are formed,
 * the device counterpart of utils.smooth in the reference's CLI (cli/main_cli.py:99-104: "smooth": k of input.json) and of
 * scipy.signal.savgol_filter in examples/example_ukf_rts_smoother_savgol.py.  Both are linear filters, and the device has
 * one form that covers them; the tables are made on the host (track_estimators.batch.box_filter, savgol_filter_table).
 *   interior    out[i] = sum_k taps[k] y[i - left + k], k < window; samples outside [0, nobs) count as 0
 *   edges       with nedge = h > 0, row i < h is sum_k edge[i][k] y[k] over the first `window` samples and row
 *               nobs - 1 - r (r < h) its mirror image over the last: sum_k edge[r][window - 1 - k] y[nobs - window + k].
 *               h <= window / 2, so with nobs >= window the two edges never meet.
 *   circular    (for courses) the filter runs on differences from the row's own value, wrapped into [-180, 180]:
 *               d_k = delta - 360 rint(delta / 360) with delta = y[j] - y[i] (d_k = 0 for a sample outside [0, nobs)),
 *               out[i] = (y[i] + sum_k c_k d_k) mod 360 in [0, 360).  With circular = 0 courses are averaged as plain
 *               numbers, as the reference does (359 and 1 give 180).
 * Every tap is multiplied and added in order of k without contraction, none is skipped for a zero weight: a non-finite raw
 * value (gap = 0) makes exactly the outputs whose window holds it non-finite.
 *
 * ste_track_prep_smooth_f64 computes the raw series as ste_track_prep_f64 does (the same kernel) into raw_sog / raw_cog
 * [Tmax][B] (required workspace that doubles as output; must not overlap each other, any output or any input of the batch), filters each
 * over [0, nobs[t]) into b->sog / b->cog, and builds sog_rate, cog_rate and z from the FILTERED series by the rules above
 * (backward difference over gap[i-1], 0 for i = 0; rows >= nobs[t] are 0).  A NULL descriptor leaves that series unsmoothed:
 * its values and rates are then those of ste_track_prep_f64 bit for bit.  b->status is reset as there.
 * STE_EINVAL before any launch: NULL workspace, NULL b->sog or b->cog, aliasing, window outside 2..128, left outside 0..window-1, nedge outside
 * 0..window/2, NULL taps, NULL edge with nedge > 0, circular not 0 or 1, and whatever ste_track_prep_f64 refuses.
 * With nedge > 0 every track needs nobs >= window.  THE CALLER GUARANTEES THIS: nobs is device memory and the call stays
 * asynchronous, so it is not checked here (track_estimators.batch.prepare_observations checks it on the host and raises).
 * A shorter track is safe for memory -- no read or write leaves [0, nobs) of its columns -- but its values are unspecified.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct ste_fir_f64 {
    int32_t window;      /* w taps, 2..128 */
    int32_t left;        /* tap k of interior row i reads y[i - left + k]; 0..w-1 */
    int32_t nedge;       /* h edge rows at either end, 0..w/2; 0 = zero padding */
    int32_t circular;    /* 1: filter wrapped differences (courses in degrees); 0: plain numbers */
    const double* taps;  /* DEVICE [w] */
    const double* edge;  /* DEVICE [h][w], may be NULL when h = 0 */
} ste_fir_f64;

int ste_track_prep_smooth_f64(const ste_prep_batch_f64* b, const ste_fir_f64* fir_sog, const ste_fir_f64* fir_cog,
                              double* raw_sog, double* raw_cog, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Stream partitioning for pipelined batches.  At the batch sizes of BASELINE configs[1..2] the forward kernel is a few
 * hundred long-running waves (10 000 tracks = 625 waves on 1 024 SIMDs) and the smoother is latency-bound, so the
 * smoother of batch i can run beside the forward pass of batch i+1 -- provided they do not share SIMDs, where each
 * would take the other's issue slots.  These two calls create / destroy a HIP stream restricted to the compute units
 * [first_cu, first_cu + num_cus) of the current device (hipExtStreamCreateWithCUMask; on MI355X mask bit n is CU n/8
 * of XCD n%8, so a contiguous range is spread evenly over the eight XCDs).  Every entry point above accepts such a
 * stream.  Host plumbing only: nothing of the reference corresponds to it (the reference runs ships one at a time,
 * examples/example_ukf_rts_smoother_batch.py:19-90).
 * ------------------------------------------------------------------------------------------------------------- */
int ste_stream_create_cu_range(int32_t first_cu, int32_t num_cus, void** stream);
int ste_stream_destroy(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STE_H */
