"""Python restatement of the grid quantities (include/ste.h: ste_grid_metrics_f64; DESIGN.md, "Grids"), operation for operation,
and the small batches its tests share.

A grid is the tuple (lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref) (``grid_tuple`` makes one of a
track_estimators.batch.TrackGrid).  Time is counted in integer ticks of 2^-20 h.  For one track, ns = nsteps[t], rows 0 .. ns:
    row        x_k = lon_ref + wrap180(lon_k - lon_ref)
    step k     from A = (x_k, lat_k) to B = (x_k + delta, lat_{k+1}), delta = wrap180(lon_{k+1} - lon_k); SOUND when |delta| < 90,
               both latitudes are finite, dt_k >= 0 and dt_k 2^20 < 2^52; else BROKEN: counted, and no time anywhere
    pieces     dtq = rint(dt_k 2^20) split at the grid lines strictly between A and B: x-lines and y-lines merged by their
               parameter u, ties to x; a piece is the difference of the rounded ticks of its ends, so a step's pieces sum to dtq
    clipping   the line indices are clamped to the grid's own lines (not in x on a periodic grid); everything off the grid is
               one "outside" cell
    runs       a maximal stretch of consecutive non-empty pieces in one cell, across steps and broken steps, adds its ticks to
               ticks[cell] once and 1 to entries[cell]
"""
import math

import numpy as np
import path_metrics_cases as pmc
import region_metrics_cases as rmc

TICKS_PER_HOUR = 1048576.0


def wrap180(x): return np.mod(x + 180.0, 360.0) - 180.0
def _lines(gA, gB, n, periodic):   # grid lines strictly between gA and gB, in the order met: (first, last, direction)
    if gB > gA:
        lo, hi = math.floor(gA) + 1.0, math.ceil(gB) - 1.0
        if not periodic: lo, hi = max(lo, 0.0), min(hi, float(n))
        return (int(lo), int(hi), 1) if lo <= hi else (0, -1, 1)
    if gB < gA:
        hi, lo = math.ceil(gA) - 1.0, math.floor(gB) + 1.0
        if not periodic: lo, hi = max(lo, 0.0), min(hi, float(n))
        return (int(hi), int(lo), -1) if lo <= hi else (0, 1, -1)
    return (0, -1, 1)
def _start(g, n, periodic):
    f = math.floor(g)
    return int(f) if periodic else int(min(max(f, -1.0), float(n)))
def grid_track(lon, lat, dt, ns, grid):
    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = grid
    ticks, entries = {}, {}
    state = {"cur": "start", "acc": 0, "outside": 0}
    def flush():
        if state["cur"] is None: state["outside"] += state["acc"]
        elif state["cur"] != "start": ticks[state["cur"]] = ticks.get(state["cur"], 0) + state["acc"]
    def add(ix, iy, q):
        if q == 0: return                      # a piece of no ticks adds nothing and is no entry
        if periodic: ix = ix % nx
        c = (iy, ix) if 0 <= ix < nx and 0 <= iy < ny else None
        if c != state["cur"]:
            flush(); state["cur"], state["acc"] = c, 0
            if c is not None: entries[c] = entries.get(c, 0) + 1
        state["acc"] += q
    total = nbroken = 0
    ax = lon_ref + wrap180(lon[0] - lon_ref)
    for k in range(ns):
        x1 = lon_ref + wrap180(lon[k + 1] - lon_ref)
        delta = wrap180(lon[k + 1] - lon[k]); d = dt[k]
        sound = (abs(delta) < 90.0 and lat[k] * 0.0 == 0.0 and lat[k + 1] * 0.0 == 0.0
                 and d >= 0.0 and d * TICKS_PER_HOUR < 4503599627370496.0)
        if not sound:
            nbroken += 1; ax = x1; continue
        dtq = int(np.rint(d * TICKS_PER_HOUR)); total += dtq
        gxA, gyA = (ax - lon0) / dlon, (lat[k] - lat0) / dlat
        gxB, gyB = ((ax + delta) - lon0) / dlon, (lat[k + 1] - lat0) / dlat
        dgx, dgy = gxB - gxA, gyB - gyA
        i, iend, sx = _lines(gxA, gxB, nx, periodic)
        j, jend, sy = _lines(gyA, gyB, ny, False)
        ix, iy = _start(gxA, nx, periodic), _start(gyA, ny, False)
        tprev = 0
        while True:
            morex, morey = (i - iend) * sx <= 0, (j - jend) * sy <= 0
            if not (morex or morey): break
            ux = min(max((float(i) - gxA) / dgx, 0.0), 1.0) if morex else 2.0
            uy = min(max((float(j) - gyA) / dgy, 0.0), 1.0) if morey else 2.0
            takex = ux <= uy
            tq = max(int(np.rint((ux if takex else uy) * float(dtq))), tprev)
            add(ix, iy, tq - tprev); tprev = tq
            if takex: ix = i if sx > 0 else i - 1; i += sx
            else:     iy = j if sy > 0 else j - 1; j += sy
        add(ix, iy, dtq - tprev)
        ax = x1
    flush()
    return ticks, entries, state["outside"], total, nbroken


# ---- the call: every track of every sample on one grid -----------------------------------------------------------------------
def grid_tuple(g):
    """The restatement's grid of a track_estimators.batch.TrackGrid."""
    return (g.lon0, g.lat0, g.dlon, g.dlat, g.nx, g.ny, g.periodic, g.lon_ref)


def grid_metrics(states, nsteps, dt, grid, tracks=False):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B), ``grid`` a tuple as above ->
    dict(ticks, entries (ny, nx) int64 summed over all tracks, outside, total (S, B) int64, nbroken (S, B) int32); with
    ``tracks`` also per_track[s][t] = (ticks, entries) of that track, dicts keyed (iy, ix)."""
    states = np.asarray(states, dtype=np.float64)
    S, _, _, B = states.shape
    nx, ny = grid[4], grid[5]
    out = {"ticks": np.zeros((ny, nx), dtype=np.int64), "entries": np.zeros((ny, nx), dtype=np.int64),
           "outside": np.zeros((S, B), dtype=np.int64), "total": np.zeros((S, B), dtype=np.int64),
           "nbroken": np.zeros((S, B), dtype=np.int32)}
    per = [[None] * B for _ in range(S)]
    with np.errstate(all="ignore"):
        for s in range(S):
            for t in range(B):
                ns = int(nsteps[t])
                lon = [float(v) for v in states[s, : ns + 1, 0, t]]
                lat = [float(v) for v in states[s, : ns + 1, 1, t]]
                tk, en, outside, total, nbrk = grid_track(lon, lat, [float(v) for v in dt[:ns, t]], ns, grid)
                for c, v in tk.items():
                    out["ticks"][c] += v
                for c, v in en.items():
                    out["entries"][c] += v
                out["outside"][s, t], out["total"][s, t], out["nbroken"][s, t] = outside, total, nbrk
                per[s][t] = (tk, en)
    if tracks:
        out["per_track"] = per
    return out


def conserved(r):
    """The identity on a result of the call (restatement or device): the grid's ticks and the tracks' outside ticks sum to the
    tracks' total ticks.  (Per track it is asserted on the restatement, which has per-track grids.)"""
    return int(r["ticks"].sum()) + int(r["outside"].sum()) == int(r["total"].sum())


# ---- hand-made tracks: the equator at one degree an hour over a row of ten one-degree cells -----------------------------------
T20, T19 = 1 << 20, 1 << 19


def hand_cases():
    """name -> (grid arguments for batch.track_grid, states (1, rows, 4, 1), nsteps, dt (N, 1), ticks expected in columns
    0 .. 9 of row 0, ticks expected outside, ticks expected in column 10 (periodic: the grid has no outside in longitude)).
      one: from lon 0.5 in ten steps of an hour: cell 0 for half an hour, cells 1 .. 9 for an hour each, half an hour outside
      two: the same line from 0.25 in four steps of 2.5 hours: cell 0 for 0.75 h, 0.25 h outside
    each also moved to 175 .. 185 and stored wrapped, and through a periodic 360 x 1 grid from lon 0."""
    cases = {}
    for name, start, n, step in (("one", 0.5, 10, 1.0), ("two", 0.25, 4, 2.5)):
        first = int((1.0 - start) * T20)
        want, outside = [first] + [T20] * 9, int(start * T20)
        for where, shift, wrapped, args in (("", 0.0, False, (0.0, -0.5, 1.0, 1.0, 10, 1)),
                                            ("/antimeridian", 175.0, True, (175.0, -0.5, 1.0, 1.0, 10, 1)),
                                            ("/periodic", 0.0, False, (0.0, -0.5, 1.0, 1.0, 360, 1))):
            trk = np.stack([shift + start + step * np.arange(n + 1.0), np.zeros(n + 1)], axis=1)
            st = pmc.states_of([trk])
            if wrapped:
                st[:, :, 0] = wrap180(st[:, :, 0])
            periodic = where == "/periodic"
            cases[name + where] = (args, st, np.array([n], dtype=np.int32), np.full((n, 1), step), want,
                                   0 if periodic else outside, outside if periodic else None)
    return cases


# ---- random ragged tracks about the antimeridian, for the restatement against sampling ----------------------------------------
SAMPLING_GRIDS = {"half-degree": (172.0, -3.0, 0.5, 0.25, 32, 24), "global 5": (-180.0, -90.0, 5.0, 5.0, 72, 36),
                  "one cell": (170.0, -5.0, 20.0, 10.0, 1, 1)}
_CACHE = {}


def random_tracks():
    """300 tracks of up to N = 8 steps (states (1, 9, 4, 300), nsteps in 0 .. 8, dt (8, 300) in [0.2, 1.5]): starts within 6
    degrees of lon 179 and 3 of the equator (the latitudes of the first grid), steps N(0, 1.2) x N(0, 0.6) degrees, longitudes stored wrapped."""
    if "random" not in _CACHE:
        rng = np.random.default_rng(5)
        N, B = 8, 300
        st = np.zeros((1, N + 1, 4, B))
        start = np.stack([179.0 + rng.uniform(-6.0, 6.0, B), rng.uniform(-3.0, 3.0, B)])
        steps = rng.normal(0.0, 1.0, (N, 2, B)) * np.array([1.2, 0.6])[None, :, None]
        st[0, 0, :2] = start
        st[0, 1:, :2] = start[None] + np.cumsum(steps, axis=0)
        st[:, :, 0] = wrap180(st[:, :, 0])
        nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
        _CACHE["random"] = dict(states=st, nsteps=nsteps, dt=rng.uniform(0.2, 1.5, (N, B)))
    return _CACHE["random"]


# ---- the mapping fleet: that of the region tests (S = 5, Nmax = 8, B = 130, about (179.6, 10)), garbage rows planted ------------
FLEET_S, FLEET_N, FLEET_B, FLEET_WINDOW = rmc.FLEET_S, rmc.FLEET_N, rmc.FLEET_B, rmc.FLEET_WINDOW
HUGE_LAT_TRACK, NAN_LON_TRACK, INF_LAT_TRACK, NEG_DT_TRACK, NAN_DT_TRACK = 26, 35, 44, 53, 62  # all have nsteps = Nmax
# the first and second grids of the sampling test (the fleet sails north of the first: nearly all of it is outside), and the
# first moved north to lie under the fleet
FLEET_GRIDS = {"half-degree": SAMPLING_GRIDS["half-degree"], "global 5": SAMPLING_GRIDS["global 5"],
               "half-degree north": (172.0, 7.0, 0.5, 0.25, 32, 24)}


def plant_garbage(states, dt):
    """Copies of (states, dt) with: latitude 1e300 in row 3 of HUGE_LAT_TRACK (finite: two sound steps that run off the grid);
    NaN longitude in row 4 of NAN_LON_TRACK and inf latitude in row 2 of INF_LAT_TRACK (two broken steps each); dt = -1 in step
    5 of NEG_DT_TRACK and NaN in step 1 of NAN_DT_TRACK (one broken step each)."""
    st, dt = states.copy(), dt.copy()
    st[:, 3, 1, HUGE_LAT_TRACK] = 1e300
    st[:, 4, 0, NAN_LON_TRACK] = np.nan
    st[:, 2, 1, INF_LAT_TRACK] = np.inf
    dt[5, NEG_DT_TRACK] = -1.0
    dt[1, NAN_DT_TRACK] = np.nan
    return st, dt


def fleet():
    """dict(states (5, 9, 4, 130), nsteps (every length 0 .. 8), dt (8, 130)): the fleet of tests/region_metrics_cases.py (its
    NaN-latitude track and its 120-degree jump included) with the rows of ``plant_garbage``."""
    if "fleet" not in _CACHE:
        w = rmc.fleet()
        st, dt = plant_garbage(w["states"], w["dt"])
        for b in (HUGE_LAT_TRACK, NAN_LON_TRACK, INF_LAT_TRACK, NEG_DT_TRACK, NAN_DT_TRACK):
            assert w["nsteps"][b] == FLEET_N
        _CACHE["fleet"] = dict(states=st, nsteps=w["nsteps"], dt=dt)
    return _CACHE["fleet"]


def fleet_reference(name, args=None):
    """The restatement on the mapping fleet for the grid batch.track_grid(*args) (default: FLEET_GRIDS[name]), computed once."""
    from track_estimators import batch

    key = ("ref", name)
    if key not in _CACHE:
        w = fleet()
        g = batch.track_grid(*(FLEET_GRIDS[name] if args is None else args))
        _CACHE[key] = grid_metrics(w["states"], w["nsteps"], w["dt"], grid_tuple(g))
    return _CACHE[key]
