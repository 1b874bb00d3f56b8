"""NumPy restatement of the path quantities (include/ste.h: ste_path_metrics_f64; DESIGN.md, "Path quantities") and the small
batches its tests share.

For track t of sample s, with ns = nsteps[t] and rows 0 .. ns of (lon, lat):
    leg k (k < ns)   utils.haversine_formula(row k, row k+1) on the sphere, geodesic.inverse(...) on WGS84 (0 for points closer
                     than 1e-8 degrees in both coordinates, as utils.geographiclib_distance has it)
    distance         the legs summed in step order; cumulative[k] = the first k legs
    offset           a_k = lat_k - v (a parallel) or wrap180(lon_k - v) (a meridian), wrap180 of tests/track_sampling_cases
    crossing         step k crosses when (a_k < 0) != (a_{k+1} < 0), for a meridian also |a_{k+1} - a_k| < 180; a step with a
                     non-finite offset does not cross
    cross_time       of the FIRST crossing step: T_k + dt_k a_k / (a_k - a_{k+1}), T_k = dt_0 + ... + dt_{k-1} in order; NaN = none
"""
import numpy as np
from track_sampling_cases import wrap180

DIST_RTOL, DIST_ATOL = 1e-10, 1e-12  # tests/test_track_prep.py::compare, for the same leg functions; a sum of non-negative
#                                      legs keeps the relative error
TIME_RTOL = 1e-12  # of the track's total time: a handful of roundings, no cancellation (a_k and a_{k+1} differ in sign)
KM_PER_DEG_EQUATOR = 6378.137 * np.pi / 180.0


def leg_km(model, lon1, lat1, lon2, lat2):
    from track_estimators import geodesic, utils

    if model == "sphere":
        return float(utils.haversine_formula(lon1, lat1, lon2, lat2))
    if abs(lat1 - lat2) < 1e-8 and abs(lon1 - lon2) < 1e-8:
        return 0.0
    return geodesic.inverse(lat1, lon1, lat2, lon2)[0] * 1e-3


def path_metrics(states, nsteps, dt=None, model="sphere", line_axis=None, line_value=None):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B), ``line_value`` (B,) ->
    dict(distance (S, B), cumulative (S, N+1, B) with NaN past nsteps, cross_time (S, B), ncross (S, B) int32,
    total_time (B,))."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    out = {"distance": np.zeros((S, B)), "cumulative": np.full((S, rows, B), np.nan)}
    if line_axis is not None:
        out["cross_time"] = np.full((S, B), np.nan)
        out["ncross"] = np.zeros((S, B), dtype=np.int32)
        out["total_time"] = np.zeros((B,))
        line_value = np.broadcast_to(np.asarray(line_value, dtype=np.float64), (B,))
    for s in range(S):
        for t in range(B):
            ns = int(nsteps[t])
            lon, lat = states[s, :, 0, t], states[s, :, 1, t]
            d = 0.0
            out["cumulative"][s, 0, t] = 0.0
            for k in range(ns):
                d = d + leg_km(model, lon[k], lat[k], lon[k + 1], lat[k + 1])
                out["cumulative"][s, k + 1, t] = d
            out["distance"][s, t] = d
            if line_axis is None:
                continue
            v = line_value[t]
            a = (lat[: ns + 1] - v) if line_axis == "lat" else wrap180(lon[: ns + 1] - v)
            T, nc = 0.0, 0
            for k in range(ns):
                a0, a1 = a[k], a[k + 1]
                cross = ((a0 < 0.0) != (a1 < 0.0)) and np.isfinite(a0 - a1)
                if line_axis == "lon":
                    cross = cross and abs(a1 - a0) < 180.0
                if cross:
                    if nc == 0:
                        out["cross_time"][s, t] = T + dt[k, t] * a0 / (a0 - a1)
                    nc += 1
                T = T + dt[k, t]
            out["ncross"][s, t] = nc
            out["total_time"][t] = T
    return out


def states_of(tracks):
    """Hand-made tracks, a list of (rows, 2) lon / lat arrays of one length -> (1, rows, 4, B) with zero speed and heading."""
    tracks = [np.asarray(t, dtype=np.float64) for t in tracks]
    st = np.zeros((1, tracks[0].shape[0], 4, len(tracks)))
    for b, t in enumerate(tracks):
        st[0, :, :2, b] = t
    return st


def equator_track(n, lon0=0.0):
    """n legs of one degree along the equator, eastwards from lon0."""
    return np.stack([lon0 + np.arange(n + 1.0), np.zeros(n + 1)], axis=1)


def bare_batch(nsteps, dt):
    """A HostBatch that carries nothing but what ste_path_metrics_f64 reads of a batch: B, Nmax, nsteps and dt (Nmax, B)."""
    from track_estimators import batch

    dt = np.ascontiguousarray(dt, dtype=np.float64)
    N, B = dt.shape
    z = np.zeros((N, B))
    return batch.HostBatch(B=B, Nmax=N, Tmax=1, H=np.eye(4), Q=np.eye(4), R=np.eye(4), nsteps=np.asarray(nsteps, dtype=np.int32),
                           x0=np.zeros((4, B)), P0=np.eye(4).reshape(16), dt=dt, sog_rate=z, cog_rate=z.copy(), sog_rate_rts=None,
                           cog_rate_rts=None, upd_idx=np.full((N, B), -1, dtype=np.int32), z=np.zeros((1, 4, B)))


# ---- the random-walk fleet of the mapping tests: S = 5, Nmax = 8, B = 130 (two full waves plus two lanes) -------------------
WALK_S, WALK_N, WALK_B, WALK_SEED = 5, 8, 130, 7
WALK_WINDOW = (3, 70)
_CACHE = {}


def walk():
    """dict(states (5, 9, 4, 130), nsteps (every length 0 .. 8, so 0, 1 and Nmax are there), dt (8, 130), lat_line, lon_line
    (130,)).  Steps of a few tenths of a degree; tracks 0 .. 9 start within a degree of the antimeridian and are kept
    unwrapped (longitudes past 180).  Line values: for three tracks in four the track's own mid-row position of sample 0 (so
    that sample crosses), for every fourth one 40 degrees away (no sample gets there)."""
    if "walk" in _CACHE:
        return _CACHE["walk"]
    rng = np.random.default_rng(WALK_SEED)
    S, N, B = WALK_S, WALK_N, WALK_B
    st = np.zeros((S, N + 1, 4, B))
    lon0 = rng.uniform(-170.0, 170.0, B)
    lon0[:10] = 179.0 + rng.uniform(0.0, 1.0, 10)
    lat0 = rng.uniform(-60.0, 60.0, B)
    drift = rng.normal(0.0, 0.3, (2, B))
    steps = drift[None, None] + rng.normal(0.0, 0.1, (S, N, 2, B))
    st[:, 0, 0], st[:, 0, 1] = lon0, lat0
    st[:, 1:, :2] = np.stack([lon0, lat0])[None, None] + np.cumsum(steps, axis=1)
    st[:, :, 2:] = rng.normal(0.0, 1.0, (S, N + 1, 2, B))  # speed and heading: not read
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    dt = rng.uniform(0.2, 1.5, (N, B))
    mid = np.maximum(nsteps // 2, 0)
    far = np.arange(B) % 4 == 3
    lines = {}
    for name, c in (("lon", 0), ("lat", 1)):
        a, b = st[0, mid, c, np.arange(B)], st[0, np.minimum(mid + 1, N), c, np.arange(B)]
        lines[name] = np.where(far, a + 40.0, 0.5 * (a + b))
    _CACHE["walk"] = dict(states=st, nsteps=nsteps, dt=dt, lon_line=lines["lon"], lat_line=lines["lat"])
    return _CACHE["walk"]


def walk_reference(model, line_axis):
    """The restatement on the random-walk fleet, computed once per (model, axis)."""
    key = ("ref", model, line_axis)
    if key not in _CACHE:
        w = walk()
        _CACHE[key] = path_metrics(w["states"], w["nsteps"], w["dt"], model, line_axis,
                                   None if line_axis is None else w[line_axis + "_line"])
    return _CACHE[key]
