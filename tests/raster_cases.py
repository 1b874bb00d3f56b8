"""Python restatement of the raster quantities (include/ste.h: ste_raster_metrics_f64; DESIGN.md, "Rasters"), operation for
operation, and the rasters its tests share.  Ticks are Python integers throughout.

A grid is the tuple of tests/grid_metrics_cases.py, (lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref), and the track is
the grid call's, word for word.  For one track:
    pieces     the non-empty pieces of its sound steps in the order sailed, (cell, q): cell = (iy, ix) after wrapping, None
               off the grid; q > 0 ticks (`pieces`)
    runs       maximal stretches of consecutive pieces in one cell, across steps and broken steps: (cell, q, start), start =
               the ticks of all pieces before it (`runs`)
    outputs    from the runs and the raster's values alone (`outputs`)
"""
import math

import grid_metrics_cases as gmc
import numpy as np

TICKS_PER_HOUR = gmc.TICKS_PER_HOUR
NAN = float("nan")


def pieces(lon, lat, dt, ns, grid, tally=None):
    """The non-empty pieces (cell, q) of a track, in order.  ``tally``, a dict, gets ``total`` (the ticks of the sound steps)
    and ``nbroken`` when the generator is exhausted.  The walk is that of grid_metrics_cases.grid_track."""
    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = grid
    total = nbroken = 0

    def cell(ix, iy):
        if periodic:
            ix = ix % nx
        return (iy, ix) if 0 <= ix < nx and 0 <= iy < ny else None

    ax = lon_ref + gmc.wrap180(lon[0] - lon_ref) if ns > 0 else 0.0
    for k in range(ns):
        x1 = lon_ref + gmc.wrap180(lon[k + 1] - lon_ref)
        delta = gmc.wrap180(lon[k + 1] - lon[k])
        d = dt[k]
        sound = (abs(delta) < 90.0 and lat[k] * 0.0 == 0.0 and lat[k + 1] * 0.0 == 0.0
                 and d >= 0.0 and d * TICKS_PER_HOUR < 4503599627370496.0)
        if not sound:
            nbroken += 1
            ax = x1
            continue
        dtq = int(np.rint(d * TICKS_PER_HOUR))
        total += dtq
        gxA, gyA = (ax - lon0) / dlon, (lat[k] - lat0) / dlat
        gxB, gyB = ((ax + delta) - lon0) / dlon, (lat[k + 1] - lat0) / dlat
        dgx, dgy = gxB - gxA, gyB - gyA
        i, iend, sx = gmc._lines(gxA, gxB, nx, periodic)
        j, jend, sy = gmc._lines(gyA, gyB, ny, False)
        ix, iy = gmc._start(gxA, nx, periodic), gmc._start(gyA, ny, False)
        tprev = 0
        while True:
            morex, morey = (i - iend) * sx <= 0, (j - jend) * sy <= 0
            if not (morex or morey):
                break
            ux = min(max((float(i) - gxA) / dgx, 0.0), 1.0) if morex else 2.0
            uy = min(max((float(j) - gyA) / dgy, 0.0), 1.0) if morey else 2.0
            takex = ux <= uy
            tq = max(int(np.rint((ux if takex else uy) * float(dtq))), tprev)
            if tq > tprev:
                yield cell(ix, iy), tq - tprev
            tprev = tq
            if takex:
                ix = i if sx > 0 else i - 1
                i += sx
            else:
                iy = j if sy > 0 else j - 1
                j += sy
        if dtq > tprev:
            yield cell(ix, iy), dtq - tprev
        ax = x1
    if tally is not None:
        tally["total"], tally["nbroken"] = total, nbroken


def runs(pcs):
    """[(cell, q, start)] of an iterable of pieces: consecutive pieces in one cell joined, start = the ticks before the run."""
    out, clock = [], 0
    for c, q in pcs:
        if out and out[-1][0] == c:
            out[-1][1] += q
        else:
            out.append([c, q, clock])
        clock += q
    return [tuple(r) for r in out]


def outputs(rns, values, threshold=None, below=False, min_ticks=0):
    """The per-track outputs of the header from a track's runs and ``values`` (ny, nx)."""
    o = dict(outside=0, valid=0, nodata=0, wsum=0.0, vmin=NAN, vmax=NAN, tmin=-1, tmax=-1, hit_ticks=0, hit_first=-1, nhit=0,
             nhit_long=0, hit_longest=0)
    exc = None  # the ticks of the excursion that is open

    def end():
        nonlocal exc
        if exc is not None:
            if exc >= min_ticks:
                o["nhit_long"] += 1
            o["hit_longest"] = max(o["hit_longest"], exc)
            exc = None

    for c, q, start in rns:
        hit = False
        if c is None:
            o["outside"] += q
        else:
            v = float(values[c])
            if v != v:
                o["nodata"] += q
            else:
                o["valid"] += q
                o["wsum"] = o["wsum"] + float(q) * v
                if not (o["vmin"] <= v):
                    o["vmin"], o["tmin"] = v, start
                if not (o["vmax"] >= v):
                    o["vmax"], o["tmax"] = v, start
                hit = threshold is not None and (v <= threshold if below else v >= threshold)
        if hit:
            o["hit_ticks"] += q
            if o["hit_first"] < 0:
                o["hit_first"] = start
            if exc is None:
                exc = 0
                o["nhit"] += 1
            exc += q
        else:
            end()
    end()
    return o


def row_value(lon_k, lat_k, grid, values):
    """The value of the cell a row itself lies in; NaN off the grid or for a lon or lat that is not finite."""
    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = grid
    gx = ((lon_ref + gmc.wrap180(lon_k - lon_ref)) - lon0) / dlon
    gy = (lat_k - lat0) / dlat
    if not (math.isfinite(gx) and math.isfinite(gy)):
        return NAN
    fx, fy = math.floor(gx), math.floor(gy)
    if periodic:
        fx %= nx
    return float(values[fy, fx]) if 0 <= fx < nx and 0 <= fy < ny else NAN


INT64 = ("total", "outside", "valid", "nodata", "tmin", "tmax", "hit_ticks", "hit_first", "hit_longest")
INT32 = ("nbroken", "nhit", "nhit_long")
FLOAT = ("wsum", "vmin", "vmax")
HIT = ("hit_ticks", "hit_first", "nhit", "nhit_long", "hit_longest")


def raster_metrics(states, nsteps, dt, grid, values, threshold=None, below=False, min_ticks=0, tracks=False):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B) -> dict of (S, B) arrays with the dtypes
    of the call, ``row_value`` (S, N+1, B) with NaN past nsteps, and with ``tracks`` per_track[s][t] = the track's runs."""
    states = np.asarray(states, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    S, rows, _, B = states.shape
    out = {k: np.zeros((S, B), dtype=np.int64) for k in INT64}
    out.update({k: np.zeros((S, B), dtype=np.int32) for k in INT32})
    out.update({k: np.zeros((S, B)) for k in FLOAT})
    out["row_value"] = np.full((S, rows, B), np.nan)
    per = [[None] * B for _ in range(S)]
    with np.errstate(all="ignore"):
        for s in range(S):
            for t in range(B):
                ns = int(nsteps[t])
                lon = [float(v) for v in states[s, : ns + 1, 0, t]]
                lat = [float(v) for v in states[s, : ns + 1, 1, t]]
                tally = {"total": 0, "nbroken": 0}
                rns = runs(pieces(lon, lat, [float(v) for v in dt[:ns, t]], ns, grid, tally))
                o = outputs(rns, values, threshold, below, min_ticks)
                o.update(tally)
                for k, v in o.items():
                    out[k][s, t] = v
                for k in range(ns + 1):
                    out["row_value"][s, k, t] = row_value(lon[k], lat[k], grid, values)
                per[s][t] = rns
    if tracks:
        out["per_track"] = per
    return out


# ---- the rasters of the tests -------------------------------------------------------------------------------------------------
THRESHOLD, MIN_TICKS, MIN_HOURS = 3.0, 1 << 18, 0.25
FINE_GRID = (179.0, 9.5, 0.01, 0.01, 128, 128)  # lon_ref 179.64: every step of the fleet crosses tens of its lines
# the fleet's rasters: one cell; either side of 256 cells (the size up to which the grid kernel keeps a copy in LDS); the
# periodic 72 x 36 grid; half-degree cells under the fleet; the fine grid
FLEET_RASTERS = {"one cell": (178.0, 9.0, 4.0, 2.0, 1, 1), "256 cells": (176.0, 6.0, 0.5, 0.5, 16, 16),
                 "272 cells": (176.0, 6.0, 0.5, 0.5, 17, 16), "global 5": gmc.FLEET_GRIDS["global 5"],
                 "half-degree north": gmc.FLEET_GRIDS["half-degree north"], "fine": FINE_GRID}
_CACHE = {}


def raster_values(ny, nx, nodata=True):
    """Integers in -8 .. 8 from default_rng(11), a tenth of the cells NaN (``nodata=False``: 0 there)."""
    rng = np.random.default_rng(11)
    v = rng.integers(-8, 9, (ny, nx)).astype(np.float64)
    v[rng.random((ny, nx)) < 0.1] = np.nan if nodata else 0.0
    return v


def fleet_reference(name):
    """The restatement on the mapping fleet of the grid tests for FLEET_RASTERS[name] with ``raster_values``, THRESHOLD and
    MIN_TICKS, computed once: (TrackGrid, values, result)."""
    from track_estimators import batch

    if name not in _CACHE:
        w = gmc.fleet()
        g = batch.track_grid(*FLEET_RASTERS[name])
        values = raster_values(g.ny, g.nx)
        _CACHE[name] = (g, values, raster_metrics(w["states"], w["nsteps"], w["dt"], gmc.grid_tuple(g), values, THRESHOLD,
                                                  False, MIN_TICKS))
    return _CACHE[name]
