"""
ctypes binding of the C ABI declared in include/ste.h (libste_hip.so, built in-tree by ``__graft_entry__.build()``).

There is deliberately no CPU fallback: if the shared library is missing, or no MI355X is visible when a compute entry
point is called, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))  # .../ship-track-estimators_amd
# STE_LIB_PATH: developer override to A/B an experimental build of the same ABI
LIB_PATH = os.environ.get("STE_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libste_hip.so")

STE_FLAG_SHARED_P0 = 0x1
STE_FLAG_NO_INITIAL_UPDATE = 0x2
STE_FLAG_ROBUST = 0x4
STE_FLAG_LANES_1 = 0x10
STE_FLAG_LANES_4 = 0x20
STE_FLAG_PACKED_COV = 0x40

# ste_ukf_batch_f64.tuning
STE_TUNING_EIG_GAINS = 0x100  # every smoother gain by the eigenvalue route
STE_TUNING_TWO_KERNEL_SMOOTHER = 0x200  # the two-kernel smoother whatever the batch size
STE_TUNING_ONE_KERNEL_SMOOTHER = 0x400  # the one-kernel smoother whatever the batch size
STE_TUNING_LANE_RECURRENCE = 0x800  # the two-kernel form's recurrence with a lane instead of a quad per track

STE_NOISE_R_BLOCK2 = 0x1  # ste_ukf_noise_f64.flags: every track's R is zero outside its leading 2 x 2 block

STE_RTS_WORK_ROWS = 30  # doubles per (step, track) of ste_ukf_batch_f64.rts_work
STE_SLICE_ALIGN = 64  # time slices of the forward pass start and end on multiples of this many steps

STE_STATUS_NAN = 0x1
STE_STATUS_CLAMPED = 0x2
STE_STATUS_NOCONV = 0x4
STE_STATUS_ROBUST_CAP = 0x8
STE_STATUS_HOST_INDEX = 0x10
STE_STATUS_BAD_INDEX = 0x20

_dp = C.c_void_p  # device / host pointers travel as integers


class SteUkfBatchF64(C.Structure):
    """Mirror of ``struct ste_ukf_batch_f64`` (include/ste.h)."""

    _fields_ = [
        ("B", C.c_int32),
        ("Nmax", C.c_int32),
        ("Tmax", C.c_int32),
        ("n", C.c_int32),
        ("flags", C.c_uint32),
        ("tuning", C.c_int32),
        ("fan_scale", C.c_double),
        ("w0", C.c_double),
        ("wi", C.c_double),
        ("H", _dp),
        ("Q", _dp),
        ("R", _dp),
        ("nsteps", _dp),
        ("x0", _dp),
        ("P0", _dp),
        ("dt", _dp),
        ("sog_rate", _dp),
        ("cog_rate", _dp),
        ("sog_rate_rts", _dp),
        ("cog_rate_rts", _dp),
        ("upd_idx", _dp),
        ("z", _dp),
        ("noise_pred", _dp),
        ("noise_upd", _dp),
        ("noise_rts", _dp),
        ("fwd_mean", _dp),
        ("fwd_cov", _dp),
        ("sm_mean", _dp),
        ("sm_cov", _dp),
        ("status", _dp),
        ("rts_work", _dp),
        ("chi_alpha", C.c_double),
        ("robust_max_iter", C.c_int32),
        ("reserved2", C.c_int32),
        ("track_stride", C.c_int64),
        ("sm_pos", _dp),
        ("step_begin", C.c_int32),
        ("step_end", C.c_int32),
    ]


class SteUkfLoglikF64(C.Structure):
    """Mirror of ``struct ste_ukf_loglik_f64`` (include/ste.h)."""

    _fields_ = [
        ("loglik", _dp),
        ("dof", _dp),
        ("nupd", _dp),
        ("nis", _dp),
    ]


class SteUkfNoiseF64(C.Structure):
    """Mirror of ``struct ste_ukf_noise_f64`` (include/ste.h): per-track Q / R, upper triangles [10][track_stride]."""

    _fields_ = [
        ("Q", _dp),
        ("R", _dp),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SteUkfSampleF64(C.Structure):
    """Mirror of ``struct ste_ukf_sample_f64`` (include/ste.h): posterior tracks sampled from the smoother."""

    _fields_ = [
        ("nsamples", C.c_int32),
        ("flags", C.c_uint32),
        ("samples", _dp),
        ("coef", _dp),
        ("status", _dp),
    ]


STE_SAMPLE_COEF_ROWS = 30  # doubles per (row, track) of ste_ukf_sample_f64.coef


class StePathF64(C.Structure):
    """Mirror of ``struct ste_path_f64`` (include/ste.h): distance sailed and line-crossing times of tracks on the device."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("dist", _dp),
        ("cumdist", _dp),
        ("line_axis", C.c_int32),
        ("reserved", C.c_int32),
        ("line_value", _dp),
        ("cross_time", _dp),
        ("ncross", _dp),
    ]


STE_REGION_MAX_VERT = 1024


class SteRegionF64(C.Structure):
    """Mirror of ``struct ste_region_f64`` (include/ste.h): tracks on the device against a polygon."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("nvert", C.c_int32),
        ("reserved", C.c_int32),
        ("vert", _dp),
        ("lon_ref", C.c_double),
        ("time_inside", _dp),
        ("first_entry", _dp),
        ("nenter", _dp),
        ("nbroken", _dp),
        ("dist_inside", _dp),
        ("inside", _dp),
    ]


STE_GRID_TICKS_PER_HOUR = 1048576
STE_GRID_MAX_CELLS = 1 << 26
STE_GRID_PERIODIC_LON = 0x1


class SteGridF64(C.Structure):
    """Mirror of ``struct ste_grid_f64`` (include/ste.h): tracks on the device on a regular lon / lat grid."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("flags", C.c_uint32),
        ("states", _dp),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("lon0", C.c_double),
        ("lat0", C.c_double),
        ("dlon", C.c_double),
        ("dlat", C.c_double),
        ("lon_ref", C.c_double),
        ("ticks", _dp),
        ("entries", _dp),
        ("outside", _dp),
        ("total", _dp),
        ("nbroken", _dp),
    ]


STE_RASTER_BELOW = 0x2
STE_RASTER_NO_THRESHOLD = 0x4


class SteRasterF64(C.Structure):
    """Mirror of ``struct ste_raster_f64`` (include/ste.h): tracks on the device against a gridded field."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("flags", C.c_uint32),
        ("states", _dp),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("lon0", C.c_double),
        ("lat0", C.c_double),
        ("dlon", C.c_double),
        ("dlat", C.c_double),
        ("lon_ref", C.c_double),
        ("values", _dp),
        ("threshold", C.c_double),
        ("min_ticks", C.c_int64),
        ("total", _dp),
        ("outside", _dp),
        ("nbroken", _dp),
        ("valid", _dp),
        ("nodata", _dp),
        ("wsum", _dp),
        ("vmin", _dp),
        ("vmax", _dp),
        ("tmin", _dp),
        ("tmax", _dp),
        ("hit_ticks", _dp),
        ("hit_first", _dp),
        ("nhit", _dp),
        ("nhit_long", _dp),
        ("hit_longest", _dp),
        ("row_value", _dp),
    ]


STE_ENCOUNTER_MAX_PAIRS = 1 << 26
STE_ENCOUNTER_MAX_RADIUS_KM = 1000.0
STE_ENC_BAD_INDEX = 0x1
STE_ENC_BAD_TIME = 0x2


class SteEncounterF64(C.Structure):
    """Mirror of ``struct ste_encounter_f64`` (include/ste.h): pairs of tracks on the device against each other."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("npairs", C.c_int64),
        ("pairs", _dp),
        ("t0", _dp),
        ("radius_km", C.c_double),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("min_dist", _dp),
        ("min_time", _dp),
        ("time_within", _dp),
        ("first_within", _dp),
        ("nwithin", _dp),
        ("overlap", _dp),
        ("nbroken", _dp),
        ("status", _dp),
    ]


STE_CANDIDATES_MAX_WINDOWS = 4096
STE_CANDIDATES_MAX_REACH_KM = 20000.0
STE_CANDIDATES_MAX_TRACKS = 1 << 20
STE_CAND_BAD_TIME = 0x1
STE_CAND_CLIPPED = 0x2
STE_CAND_EMPTY = 0x4
STE_CAND_BAD_MARGIN = 0x8


class SteCandidatesF64(C.Structure):
    """Mirror of ``struct ste_candidates_f64`` (include/ste.h): the pair list of the encounter call, found on the device."""

    _fields_ = [
        ("states", _dp),
        ("t0", _dp),
        ("track_margin_km", _dp),
        ("reach_km", C.c_double),
        ("time0", C.c_double),
        ("window_h", C.c_double),
        ("nwindows", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("reserved_pad", C.c_int32),
        ("workspace", _dp),
        ("workspace_bytes", C.c_uint64),
        ("track_status", _dp),
        ("row_offset", _dp),
        ("npairs", C.c_int64),
        ("pairs", _dp),
        ("wfirst", _dp),
        ("nwin", _dp),
    ]


STE_POSITIONS_MAX_QUERIES = 1 << 26
STE_POS_REUSE_KNOTS = 0x1
STE_POS_BAD_INDEX = 0x1
STE_POS_BAD_TIME = 0x2
STE_POS_OUTSIDE = 0x4


class StePositionsF64(C.Structure):
    """Mirror of ``struct ste_positions_f64`` (include/ste.h): tracks on the device at given clock times."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("flags", C.c_uint32),
        ("states", _dp),
        ("nqueries", C.c_int64),
        ("qtrack", _dp),
        ("qtime", _dp),
        ("t0", _dp),
        ("knots", _dp),
        ("anchor", _dp),
        ("lon", _dp),
        ("lat", _dp),
        ("speed", _dp),
        ("heading", _dp),
        ("step", _dp),
        ("frac", _dp),
        ("status", _dp),
        ("count", _dp),
        ("moments", _dp),
    ]


STE_FIELD_MAX_SLABS = 65536
STE_FLD_NEAREST = 0x2
STE_FLD_VALUES_F32 = 0x4
STE_FLD_TIME_OUTSIDE = 0x8


class SteFieldF64(C.Structure):
    """Mirror of ``struct ste_field_f64`` (include/ste.h): a space-time gridded field where tracks on the device were at given
    clock times."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("flags", C.c_uint32),
        ("states", _dp),
        ("nqueries", C.c_int64),
        ("qtrack", _dp),
        ("qtime", _dp),
        ("t0", _dp),
        ("knots", _dp),
        ("nx", C.c_int32),
        ("ny", C.c_int32),
        ("nt", C.c_int32),
        ("reserved", C.c_uint32),
        ("lon0", C.c_double),
        ("lat0", C.c_double),
        ("dlon", C.c_double),
        ("dlat", C.c_double),
        ("lon_ref", C.c_double),
        ("time0", C.c_double),
        ("dtime", C.c_double),
        ("min_cover", C.c_double),
        ("values", _dp),
        ("vanchor", _dp),
        ("value", _dp),
        ("cover", _dp),
        ("status", _dp),
        ("count", _dp),
        ("moments", _dp),
        ("vmin", _dp),
        ("vmax", _dp),
    ]


STE_LAG1_POSITION = 0x1
STE_LAG1_ROWS, STE_LAG1_POSITION_ROWS = 16, 4  # doubles per (step, track) of ste_lag_one_f64.lag1 in its two forms


class SteLagOneF64(C.Structure):
    """Mirror of ``struct ste_lag_one_f64`` (include/ste.h): the lag-one cross-covariance of the smoother."""

    _fields_ = [
        ("lag1", _dp),
        ("status", _dp),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


STE_PCOV_FULL = 0x1
STE_PCOV_LAG1_POSITION = 0x2


class StePositionCovF64(C.Structure):
    """Mirror of ``struct ste_position_cov_f64`` (include/ste.h): the covariance of tracks on the device at given clock times."""

    _fields_ = [
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("nqueries", C.c_int64),
        ("qtrack", _dp),
        ("qtime", _dp),
        ("t0", _dp),
        ("knots", _dp),
        ("cov", _dp),
        ("lag1", _dp),
        ("pcov", _dp),
        ("step", _dp),
        ("frac", _dp),
        ("status", _dp),
    ]


STE_SITES_MAX = 65536
STE_SITE_BAD_TIME = 0x1
STE_SITE_BAD_SITE = 0x1


class SteSiteF64(C.Structure):
    """Mirror of ``struct ste_site_f64`` (include/ste.h): tracks on the device against fixed sites."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("nsites", C.c_int32),
        ("sites", _dp),
        ("radius_km", _dp),
        ("t0", _dp),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("min_dist", _dp),
        ("min_time", _dp),
        ("time_within", _dp),
        ("first_within", _dp),
        ("longest", _dp),
        ("nwithin", _dp),
        ("sound_time", _dp),
        ("nbroken", _dp),
        ("track_status", _dp),
        ("site_status", _dp),
    ]


STE_LINES_MAX = 4096
STE_LINE_MAX_VERT_TOTAL = 1 << 20
STE_LINE_BAD_TIME = 0x1
STE_LINE_BAD_LINE = 0x1


class SteLineF64(C.Structure):
    """Mirror of ``struct ste_line_f64`` (include/ste.h): tracks on the device against polylines."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("nlines", C.c_int32),
        ("nvert", C.c_int32),
        ("vert", _dp),
        ("first", _dp),
        ("lon_ref", _dp),
        ("t0", _dp),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("min_dist", _dp),
        ("min_time", _dp),
        ("min_seg", _dp),
        ("min_frac", _dp),
        ("ncross", _dp),
        ("net_cross", _dp),
        ("first_cross", _dp),
        ("last_cross", _dp),
        ("sound_time", _dp),
        ("nbroken", _dp),
        ("track_status", _dp),
        ("line_status", _dp),
    ]


STE_ROUTE_MAX_PAIRS = 1 << 26
STE_ROUTE_REVERSE_J = 0x1
STE_ROUTE_BAD_INDEX = 0x1
STE_ROUTE_NO_PATH = 0x2
STE_ROUTE_NOT_FINITE = 0x4


class SteRouteF64(C.Structure):
    """Mirror of ``struct ste_route_f64`` (include/ste.h): pairs of tracks on the device as curves."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("npairs", C.c_int64),
        ("pairs", _dp),
        ("band", C.c_int32),
        ("flags", C.c_uint32),
        ("work", _dp),
        ("work_bytes", C.c_int64),
        ("frechet", _dp),
        ("frechet_at", _dp),
        ("dtw", _dp),
        ("dtw_len", _dp),
        ("status", _dp),
    ]


STE_SPEED_MAX_BANDS = 32
STE_SPEED_ABOVE = 0x1
STE_SPEED_BAD_TIME = 0x1
STE_SPEED_BAD_LIMIT = 0x2


class SteSpeedF64(C.Structure):
    """Mirror of ``struct ste_speed_f64`` (include/ste.h): speeds, speed bands and runs of tracks on the device."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("flags", C.c_uint32),
        ("nbands", C.c_int32),
        ("band_edges", _dp),
        ("threshold", _dp),
        ("threshold_all", C.c_double),
        ("min_run_h", C.c_double),
        ("speed", _dp),
        ("dist", _dp),
        ("sound_time", _dp),
        ("vmax", _dp),
        ("vmax_time", _dp),
        ("band_time", _dp),
        ("cond_time", _dp),
        ("run_time", _dp),
        ("first_run", _dp),
        ("longest", _dp),
        ("longest_start", _dp),
        ("nruns", _dp),
        ("nbroken", _dp),
        ("track_status", _dp),
    ]


STE_ERRORS_COV_FULL = 16
STE_ERRORS_COV_PACKED = 10


class SteErrorsF64(C.Structure):
    """Mirror of ``struct ste_errors_f64`` (include/ste.h): errors of tracks on the device against truth positions."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("model", C.c_int32),
        ("states", _dp),
        ("truth", _dp),
        ("course", _dp),
        ("cov", _dp),
        ("cov_rows", C.c_int32),
        ("reserved", C.c_int32),
        ("nees_limit", C.c_double),
        ("sum_err", _dp),
        ("sum_sq", _dp),
        ("max_err", _dp),
        ("sum_along", _dp),
        ("sum_along_sq", _dp),
        ("sum_cross", _dp),
        ("sum_cross_sq", _dp),
        ("sum_nees", _dp),
        ("n", _dp),
        ("max_row", _dp),
        ("nbroken", _dp),
        ("ncoursed", _dp),
        ("nscored", _dp),
        ("ninside", _dp),
        ("err", _dp),
        ("cumerr", _dp),
        ("along", _dp),
        ("cross", _dp),
        ("nees", _dp),
    ]


STE_SIMPLIFY_SHAPE = 0x1
STE_SIMPLIFY_BAD_TIME = 0x1
STE_SIMPLIFY_BAD_LIMIT = 0x2
STE_SIMPLIFY_BROKEN = 0x4
STE_SIMPLIFY_TRUNCATED = 0x8


class SteSimplifyF64(C.Structure):
    """Mirror of ``struct ste_simplify_f64`` (include/ste.h): tracks on the device simplified within a tolerance."""

    _fields_ = [
        ("nstates", C.c_int32),
        ("flags", C.c_uint32),
        ("cap", C.c_int32),
        ("reserved", C.c_int32),
        ("states", _dp),
        ("tolerance", _dp),
        ("tolerance_all", C.c_double),
        ("lon_scale", _dp),
        ("lon_scale_all", C.c_double),
        ("work", _dp),
        ("work_bytes", C.c_int64),
        ("keep", _dp),
        ("nkeep", _dp),
        ("worst_sq", _dp),
        ("status", _dp),
        ("rows", _dp),
        ("out_states", _dp),
        ("out_dt", _dp),
    ]


STE_NOISE_TRACK_NAN = 0x1
STE_NOISE_TRACK_NOT_FINITE = 0x2
STE_NOISE_FIT_SCALAR, STE_NOISE_FIT_DIAG2, STE_NOISE_FIT_BLOCK2 = 0, 1, 2
STE_NOISE_GROUP_EMPTY = 0x1
STE_NOISE_GROUP_BAD_VARIANCE = 0x2
STE_NOISE_GROUP_BAD_MEMBER = 0x4


class SteNoiseMomentsF64(C.Structure):
    """Mirror of ``struct ste_noise_moments_f64`` (include/ste.h): per-track sums of the M-step for R."""

    _fields_ = [
        ("moments", _dp),
        ("count", _dp),
        ("vsum", _dp),
        ("track_status", _dp),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SteNoiseMstepF64(C.Structure):
    """Mirror of ``struct ste_noise_mstep_f64`` (include/ste.h): group sums and the projection of the M-step for R."""

    _fields_ = [
        ("ntracks", C.c_int32),
        ("ngroups", C.c_int32),
        ("nmembers", C.c_int32),
        ("structure", C.c_int32),
        ("ld", C.c_int64),
        ("moments", _dp),
        ("count", _dp),
        ("group_offsets", _dp),
        ("group_members", _dp),
        ("R_group", _dp),
        ("n_group", _dp),
        ("group_status", _dp),
        ("R_tracks", _dp),
        ("reserved", C.c_int64),
    ]


class SteFwdSchedF64(C.Structure):
    """Mirror of ``struct ste_fwd_sched_f64`` (include/ste.h)."""

    _fields_ = [
        ("nwindows", C.c_int32),
        ("windows", _dp),
        ("slice_steps", C.c_int32),
        ("nwaves", C.c_int32),
        ("nrounds", C.c_int32),
        ("items", _dp),
        ("host_ws", _dp),
        ("dev_ws", _dp),
        ("ws_bytes", C.c_size_t),
        ("window_done", _dp),
        ("error", _dp),
        ("timeout_s", C.c_double),
        ("started", _dp),
    ]


class SteBwdSchedF64(C.Structure):
    """Mirror of ``struct ste_bwd_sched_f64`` (include/ste.h)."""

    _fields_ = [
        ("nwindows", C.c_int32),
        ("windows", _dp),
        ("slice_steps", C.c_int32),
        ("nitems", C.c_int32),
        ("items", _dp),
        ("host_ws", _dp),
        ("dev_ws", _dp),
        ("ws_bytes", C.c_size_t),
        ("progress", _dp),
        ("error", _dp),
        ("timeout_s", C.c_double),
    ]


class SteGpBatchF64(C.Structure):
    """Mirror of ``struct ste_gp_batch_f64`` (include/ste.h)."""

    _fields_ = [
        ("B", C.c_int32),
        ("nmax", C.c_int32),
        ("nout", C.c_int32),
        ("inverse_order", C.c_int32),
        ("jitter", C.c_double),
        ("n", _dp),
        ("x", _dp),
        ("y", _dp),
        ("theta", _dp),
        ("K", _dp),
        ("U", _dp),
        ("Dinv", _dp),
        ("Kinv", _dp),
        ("alpha", _dp),
        ("lml", _dp),
        ("grad", _dp),
        ("tr", _dp),
        ("status", _dp),
        ("kernel", C.c_int32),  # 0.3.3: STE_GP_KERNEL_*
    ]


class StePrepBatchF64(C.Structure):
    """Mirror of ``struct ste_prep_batch_f64`` (include/ste.h)."""

    _fields_ = [
        ("B", C.c_int32),
        ("Tmax", C.c_int32),
        ("model", C.c_int32),
        ("reserved", C.c_int32),
        ("nobs", _dp),
        ("lon", _dp),
        ("lat", _dp),
        ("gap", _dp),
        ("sog", _dp),
        ("cog", _dp),
        ("sog_rate", _dp),
        ("cog_rate", _dp),
        ("z", _dp),
        ("status", _dp),
    ]


class SteFirF64(C.Structure):
    """Mirror of ``struct ste_fir_f64`` (include/ste.h)."""

    _fields_ = [
        ("window", C.c_int32),
        ("left", C.c_int32),
        ("nedge", C.c_int32),
        ("circular", C.c_int32),
        ("taps", _dp),
        ("edge", _dp),
    ]


STE_GP_INVERSE_AUTO, STE_GP_INVERSE_ROWS, STE_GP_INVERSE_COLS = 0, 1, 2
STE_GP_KERNEL_RBF, STE_GP_KERNEL_MATERN12, STE_GP_KERNEL_MATERN32, STE_GP_KERNEL_MATERN52 = 0, 1, 2, 3
STE_PREP_SPHERE = 0
STE_PREP_WGS84 = 1
STE_PREP_STATUS_NOCONV = 0x1

# every symbol include/ste.h declares: (restype, argtypes)
SYMBOLS = {
    "ste_version": (C.c_int, []),
    "ste_last_error": (C.c_char_p, []),
    "ste_device_count": (C.c_int, []),
    "ste_ukf_forward_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.c_void_p]),
    "ste_ukf_forward_loglik_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfLoglikF64), C.c_void_p]),
    "ste_ukf_forward_noise_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfNoiseF64), C.POINTER(SteUkfLoglikF64),
                                            C.c_void_p]),
    "ste_urtss_backward_noise_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfNoiseF64), C.c_void_p]),
    "ste_ukf_urtss_noise_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfNoiseF64), C.c_void_p]),
    "ste_urtss_sample_prepare_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfNoiseF64), C.POINTER(SteUkfSampleF64),
                                               C.c_void_p]),
    "ste_urtss_sample_draw_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfSampleF64), C.c_void_p]),
    "ste_urtss_sample_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfNoiseF64), C.POINTER(SteUkfSampleF64),
                                       C.c_void_p]),
    "ste_path_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(StePathF64), C.c_void_p]),
    "ste_region_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteRegionF64), C.c_void_p]),
    "ste_grid_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteGridF64), C.c_void_p]),
    "ste_encounter_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteEncounterF64), C.c_void_p]),
    "ste_encounter_candidates_workspace": (C.c_size_t, [C.c_int32, C.c_int32]),
    "ste_encounter_candidates_mask_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteCandidatesF64), C.c_void_p]),
    "ste_encounter_candidates_list_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteCandidatesF64), C.c_void_p]),
    "ste_track_positions_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(StePositionsF64), C.c_void_p]),
    "ste_site_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteSiteF64), C.c_void_p]),
    "ste_site_tile": (C.c_int, []),
    "ste_line_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteLineF64), C.c_void_p]),
    "ste_line_chunk": (C.c_int, []),
    "ste_route_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteRouteF64), C.c_void_p]),
    "ste_route_workspace": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64]),
    "ste_route_lds_cols": (C.c_int, []),
    "ste_speed_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteSpeedF64), C.c_void_p]),
    "ste_track_errors_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteErrorsF64), C.c_void_p]),
    "ste_raster_metrics_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteRasterF64), C.c_void_p]),
    "ste_track_simplify_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteSimplifyF64), C.c_void_p]),
    "ste_track_simplify_workspace": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ste_track_simplify_lds_rows": (C.c_int, []),
    "ste_ukf_noise_moments_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteNoiseMomentsF64), C.c_void_p]),
    "ste_ukf_noise_mstep_f64": (C.c_int, [C.POINTER(SteNoiseMstepF64), C.c_void_p]),
    "ste_field_values_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteFieldF64), C.c_void_p]),
    "ste_urtss_lag_one_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(SteUkfNoiseF64), C.POINTER(SteLagOneF64), C.c_void_p]),
    "ste_track_position_cov_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.POINTER(StePositionCovF64), C.c_void_p]),
    "ste_urtss_backward_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.c_void_p]),
    "ste_ukf_urtss_f64": (C.c_int, [C.POINTER(SteUkfBatchF64), C.c_void_p]),
    "ste_ukf_forward_sched_workspace": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "ste_ukf_forward_sched_f64": (C.c_int, [C.POINTER(SteFwdSchedF64), C.c_void_p]),
    "ste_stream_wait_counter": (C.c_int, [_dp, C.c_int32, _dp, C.c_double, C.c_void_p]),
    "ste_ukf_forward_sched_progress_offset": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "ste_urtss_backward_sched_workspace": (C.c_size_t, [C.c_int32, C.c_int64]),
    "ste_urtss_backward_sched_f64": (C.c_int, [C.POINTER(SteBwdSchedF64), C.c_void_p]),
    "ste_geodetic_dynamics_f64": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, _dp, C.c_void_p]),
    "ste_ukf_predict_f64": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double,
                                      _dp, _dp, _dp, C.c_void_p]),
    "ste_ukf_update_f64": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_void_p]),
    "ste_ukf_robust_terms_f64": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_void_p]),
    "ste_sigma_points_f64": (C.c_int, [C.c_int64, _dp, _dp, C.c_double, _dp, C.c_void_p]),
    "ste_sigma_points_generic_f64": (C.c_int, [C.c_int32, C.c_int64, _dp, _dp, C.c_double, _dp, C.c_void_p]),
    "ste_track_prep_f64": (C.c_int, [C.POINTER(StePrepBatchF64), C.c_void_p]),
    "ste_track_prep_smooth_f64": (C.c_int, [C.POINTER(StePrepBatchF64), C.POINTER(SteFirF64), C.POINTER(SteFirF64), _dp, _dp,
                                            C.c_void_p]),
    "ste_gp_last_error": (C.c_char_p, []),
    "ste_gp_rbf_kmatrix_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_void_p]),
    "ste_gp_potrf_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_void_p]),
    "ste_gp_lml_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_void_p]),
    "ste_gp_lml_subset_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_int32, _dp, C.c_void_p]),
    "ste_gp_predict_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_void_p]),
    "ste_gp_predict_cov_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, C.c_void_p]),
    "ste_gp_predict_deriv_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_void_p]),
    "ste_gp_predict_deriv_cov_f64": (C.c_int, [C.POINTER(SteGpBatchF64), C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp,
                                               C.c_void_p]),
    "ste_stream_create_cu_range": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "ste_stream_destroy": (C.c_int, [C.c_void_p]),
}


class SteError(RuntimeError):
    pass


_lib = None


def load():
    """Load libste_hip.so (once) and bind every declared symbol; raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SteError(
            f"HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "from the repo root (hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    # PyTorch (device memory / streams / RCCL plumbing) bundles its own HIP runtime under the same soname as the
    # system one.  Whichever is loaded first serves the whole process, and torch finds no GPU when the system copy won
    # the race -- so make sure torch's copy is resident before libste_hip.so pulls in libamdhip64.so.7.
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        lib = load()
        msg = lib.ste_gp_last_error() if what.startswith("ste_gp") else lib.ste_last_error()
        raise SteError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def require_gpu():
    lib = load()
    if lib.ste_device_count() < 1:
        raise SteError("no HIP device visible: the UKF/URTSS path runs only on an MI355X (gfx950); no CPU fallback")
    return lib
