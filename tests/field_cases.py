"""NumPy restatement of the values of a space-time gridded field at track positions and times (include/ste.h:
ste_field_values_f64; DESIGN.md, "Fields"), operation for operation, and the fields its tests share.  The positions are those
of tests/position_cases.py (``positions``), so locating is not restated twice.

A grid is the tuple of tests/grid_metrics_cases.py, (lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref); a field is
dict(grid, values (nt, ny, nx) float64 or float32, time0, dtime).  For a located query at tq and a sample at (lon, lat):
    time       nt == 1: it0 = it1 = 0, ft = 0.  Else gt = (tq - time0) / dtime; gt >= 0 and gt <= nt - 1 false -> TIME_OUTSIDE,
               NaN, nothing counted; it = floor(gt); it >= nt - 1 -> both slabs nt - 1, ft = 0; else it, it + 1, ft = gt - it
    space      x = lon_ref + wrap180(lon - lon_ref), gx = (x - lon0) / dlon, gy = (lat - lat0) / dlat; a non-finite lon or lat
               counts nowhere (NaN, NaN); off the grid (the raster's cell test) -> value NaN, cover 0, count[2] += 1; else
               hx = gx - 0.5, ix = floor(hx), fx = hx - ix, clamped at the borders (periodic: columns ix, ix + 1 modulo nx)
    value      w = (wt_e * wy_b) * wx_a in the order c = 4 e + 2 b + a; corners with w == 0 or a NaN value are skipped;
               num += w * v, den += w; cover = den; value = num / den if den > 0 and den >= min_cover else NaN
    nearest    the node of cell (floor gx, floor gy), slab min(floor(gt + 0.5), nt - 1); cover 1 or 0
    moments    for s in order, value and d = value - vanchor finite: count[0] += 1, sums of d and d d, vmin, vmax
"""
import math

import numpy as np
import position_cases as pc
from track_sampling_cases import wrap180

TIME_OUTSIDE = 0x8
NOWHERE, ON_GRID, OFF_GRID = 0, 1, 2
NAN = float("nan")
_CACHE = {}


def _axis(h, n):
    """The two nodes and the fraction at h = g - 0.5 on an axis of n nodes, by the non-periodic rule."""
    fl = math.floor(h)
    if fl < 0:
        return 0, 0, 0.0
    if fl >= n - 1:
        return n - 1, n - 1, 0.0
    return fl, fl + 1, h - fl


def time_axis(tq, nt, time0, dtime, nearest=False):
    """-> (inside, it0, it1, ft)."""
    if nt == 1:
        return True, 0, 0, 0.0
    gt = (float(tq) - time0) / dtime
    if not (gt >= 0.0 and gt <= nt - 1):
        return False, 0, 0, 0.0
    if nearest:
        it = min(math.floor(gt + 0.5), nt - 1)
        return True, it, it, 0.0
    it = math.floor(gt)
    if it >= nt - 1:
        return True, nt - 1, nt - 1, 0.0
    return True, it, it + 1, gt - it


def sample_value(lon, lat, it0, it1, ft, grid, values, nearest=False, min_cover=0.0):
    """One sample -> (value, cover, where, info): info = dict(nvalid corners of weight > 0, ncorners of weight > 0, cols,
    rows) on the grid, else None."""
    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = grid
    lon, lat = float(lon), float(lat)
    if not (math.isfinite(lon) and math.isfinite(lat)):
        return NAN, NAN, NOWHERE, None
    x = lon_ref + float(wrap180(lon - lon_ref))
    gx, gy = (x - lon0) / dlon, (lat - lat0) / dlat
    if not ((periodic or (gx >= 0.0 and gx < nx)) and gy >= 0.0 and gy < ny):
        return NAN, 0.0, OFF_GRID, None
    if nearest:
        ix, iy = math.floor(gx), math.floor(gy)
        if periodic:
            ix %= nx
        v = float(values[it0, iy, ix])
        return v, (1.0 if v == v else 0.0), ON_GRID, dict(cols=(ix, ix), rows=(iy, iy))
    hx = gx - 0.5
    if periodic:
        fl = math.floor(hx)
        fx = hx - fl
        ix0 = fl % nx
        ix1 = (ix0 + 1) % nx
    else:
        ix0, ix1, fx = _axis(hx, nx)
    iy0, iy1, fy = _axis(gy - 0.5, ny)
    wx, wy, wt = (1.0 - fx, fx), (1.0 - fy, fy), (1.0 - ft, ft)
    cols, rws, slabs = (ix0, ix1), (iy0, iy1), (it0, it1)
    num = den = 0.0
    nvalid = ncorner = 0
    with np.errstate(all="ignore"):
        for c in range(8):
            e, b, a = c >> 2, (c >> 1) & 1, c & 1
            w = (wt[e] * wy[b]) * wx[a]
            v = float(values[slabs[e], rws[b], cols[a]])
            ncorner += w != 0.0
            if w != 0.0 and v == v:
                nvalid += 1
                num = float(np.float64(num) + np.float64(w) * np.float64(v))
                den = den + w
        value = float(np.float64(num) / np.float64(den)) if den > 0.0 and den >= min_cover else NAN
    return value, den, ON_GRID, dict(nvalid=nvalid, ncorner=ncorner, cols=cols, rows=rws)


def field_values(pos, qtime, field, nearest=False, min_cover=0.0, vanchor=None, acc=None, details=False):
    """``pos``: what ``position_cases.positions`` returned for the queries; -> dict(value, cover (S, Q), status (Q,) int32;
    with ``vanchor`` (Q,) also count (3, Q) int32, moments (2, Q), vmin, vmax (Q,), continued from ``acc`` (a dict of those
    four) when given; with ``details`` where (S, Q) and info, a dict (s, q) -> info of the samples on the grid)."""
    grid, values = field["grid"], field["values"]
    nt = values.shape[0]
    S, Q = pos["lon"].shape
    out = dict(value=np.full((S, Q), np.nan), cover=np.full((S, Q), np.nan), status=np.array(pos["status"], dtype=np.int32))
    where, info = np.zeros((S, Q), dtype=np.int8), {}
    if vanchor is not None:
        vanchor = np.asarray(vanchor, dtype=np.float64)
        out["count"] = np.zeros((3, Q), dtype=np.int32) if acc is None else np.array(acc["count"], dtype=np.int32)
        out["moments"] = np.zeros((2, Q)) if acc is None else np.array(acc["moments"], dtype=np.float64)
        out["vmin"] = np.full(Q, np.nan) if acc is None else np.array(acc["vmin"], dtype=np.float64)
        out["vmax"] = np.full(Q, np.nan) if acc is None else np.array(acc["vmax"], dtype=np.float64)
    with np.errstate(all="ignore"):
        for q in range(Q):
            if not pos["located"][q]:
                continue
            inside, it0, it1, ft = time_axis(qtime[q], nt, field["time0"], field["dtime"], nearest)
            if not inside:
                out["status"][q] = TIME_OUTSIDE
                continue
            if vanchor is not None:
                cnt = [int(v) for v in out["count"][:, q]]
                m0, m1 = np.float64(out["moments"][0, q]), np.float64(out["moments"][1, q])
                lo, hi, va = np.float64(out["vmin"][q]), np.float64(out["vmax"][q]), np.float64(vanchor[q])
            for s in range(S):
                v, c, w, inf = sample_value(pos["lon"][s, q], pos["lat"][s, q], it0, it1, ft, grid, values, nearest, min_cover)
                out["value"][s, q], out["cover"][s, q], where[s, q] = v, c, w
                if inf is not None:
                    info[(s, q)] = inf
                if vanchor is None:
                    continue
                if w == OFF_GRID:
                    cnt[2] += 1
                if w == ON_GRID and v != v:
                    cnt[1] += 1
                d = np.float64(v) - va
                if math.isfinite(v) and math.isfinite(d):
                    cnt[0] += 1
                    m0, m1 = m0 + d, m1 + d * d
                    if not (lo <= v):
                        lo = np.float64(v)
                    if not (hi >= v):
                        hi = np.float64(v)
            if vanchor is not None:
                out["count"][:, q], out["moments"][:, q], out["vmin"][q], out["vmax"][q] = cnt, (m0, m1), lo, hi
    if details:
        out["where"], out["info"] = where, info
    return out


# ---- hand-made: a 4 x 3 grid of unit cells, three slabs two hours apart, v = 100 j + 10 iy + ix ----------------------------
HAND_GRID = (0.0, 0.0, 1.0, 1.0, 4, 3, False, 2.0)
HAND_TIME0, HAND_DTIME = 0.0, 2.0


def hand_values():
    j, iy, ix = np.meshgrid(np.arange(3.0), np.arange(3.0), np.arange(4.0), indexing="ij")
    return 100.0 * j + 10.0 * iy + ix


def hand_field(kind="full"):
    """"full"; "one nan": node (1, 1) of every slab is NaN; "all nan": the four nodes about (1.0, 1.0) are."""
    v = hand_values()
    if kind == "one nan":
        v[:, 1, 1] = np.nan
    elif kind == "all nan":
        v[:, :2, :2] = np.nan
    return dict(grid=HAND_GRID, values=v, time0=HAND_TIME0, dtime=HAND_DTIME)


def hand_batch():
    """Two tracks of four steps, S = 1.  "walk": an hour a step from t0 = 0 through (0.5, 0.5), (1.5, 1.5), (2.5, 2.75),
    (3.9, 0.1), (4.5, 0.5); "buoy": at (1.0, 1.0) throughout, steps of 1.5 h from t0 = -1 (knots -1, 0.5, 2, 3.5, 5)."""
    st = np.zeros((1, 5, 4, 2))
    st[0, :, 0, 0] = [0.5, 1.5, 2.5, 3.9, 4.5]
    st[0, :, 1, 0] = [0.5, 1.5, 2.75, 0.1, 0.5]
    st[0, :, 0, 1] = st[0, :, 1, 1] = 1.0
    dt = np.stack([np.ones(4), np.full(4, 1.5)], axis=1)
    queries = [("knot on a node", 0, 0.0), ("mid-point of four nodes", 0, 0.5), ("node hit between slabs", 0, 1.0),
               ("border half row", 0, 2.0), ("border corner", 0, 3.0), ("off the grid", 0, 4.0), ("after the track", 0, 4.5),
               ("first slab", 1, 0.0), ("last slab", 1, 4.0), ("past the last slab", 1, 4.5), ("before the first slab", 1, -0.5),
               ("bad index", 2, 1.0)]
    return dict(states=st, nsteps=np.array([4, 4], dtype=np.int32), dt=dt, t0=np.array([0.0, -1.0]),
                names=[q[0] for q in queries], qtrack=np.array([q[1] for q in queries], dtype=np.int32),
                qtime=np.array([q[2] for q in queries], dtype=np.float64))


# name -> (status, value, cover) on hand_field("full"); None = NaN
HAND_ANSWERS = {
    "knot on a node": (0, 0.0, 1.0), "mid-point of four nodes": (0, 30.5, 1.0),  # 0.75 * 5.5 + 0.25 * 105.5
    "node hit between slabs": (0, 61.0, 1.0), "border half row": (0, 122.0, 1.0), "border corner": (0, 153.0, 1.0),
    "off the grid": (0, None, 0.0), "after the track": (pc.OUTSIDE, None, None),
    "first slab": (0, 5.5, 1.0), "last slab": (0, 205.5, 1.0), "past the last slab": (TIME_OUTSIDE, None, None),
    "before the first slab": (TIME_OUTSIDE, None, None), "bad index": (pc.BAD_INDEX, None, None),
}


def hand_positions():
    h = hand_batch()
    return pc.positions(h["states"], h["nsteps"], h["dt"], h["qtrack"], h["qtime"], h["t0"])


def check_hand_answers(r, what):
    h = hand_batch()
    assert set(h["names"]) == set(HAND_ANSWERS)
    for q, name in enumerate(h["names"]):
        status, value, cover = HAND_ANSWERS[name]
        assert int(r["status"][q]) == status, (what, name, int(r["status"][q]))
        for label, g, w in (("value", r["value"][0, q], value), ("cover", r["cover"][0, q], cover)):
            assert (np.isnan(g) if w is None else g == w), (what, name, label, g, w)


# ---- the fleet's two fields ------------------------------------------------------------------------------------------------
GLOBAL_GRID = (-180.0, -90.0, 0.5, 0.5, 720, 360, True, 0.0)
STRIP_GRID = (179.5, -30.0, 0.25, 4.0, 4, 15, False, 180.0)
FIELD_SPECS = {"global": (GLOBAL_GRID, 5, -36.0, 18.0, 101), "strip": (STRIP_GRID, 3, -40.0, 40.0, 202)}  # ..., mask seed


def fleet_field(name):
    """dict(grid, values (nt, ny, nx), time0, dtime): smooth values plus noise; no data in 4 x 4-node blocks at 20 %, shared by
    all slabs, and in 5 % single nodes per slab."""
    if ("field", name) in _CACHE:
        return _CACHE[("field", name)]
    grid, nt, time0, dtime, seed = FIELD_SPECS[name]
    nx, ny = grid[4], grid[5]
    rng = np.random.default_rng(seed)
    j, iy, ix = np.meshgrid(np.arange(nt), np.arange(ny), np.arange(nx), indexing="ij")
    values = 15.0 + 10.0 * np.cos(iy * (np.pi / ny)) + 0.01 * ix + 0.5 * j + rng.normal(0.0, 0.3, (nt, ny, nx))
    blocks = rng.uniform(size=((ny + 3) // 4, (nx + 3) // 4)) < 0.2
    values[:, np.kron(blocks, np.ones((4, 4), dtype=bool))[:ny, :nx]] = np.nan
    values[rng.uniform(size=values.shape) < 0.05] = np.nan
    values.setflags(write=False)
    _CACHE[("field", name)] = dict(grid=grid, values=values, time0=time0, dtime=dtime)
    return _CACHE[("field", name)]


def fleet_vanchor(name):
    """(Q,): sample 0's own value at each query (0 where it has none), rounded to 1e-2."""
    if ("vanchor", name) not in _CACHE:
        w = pc.fleet()
        r = field_values({k: (v[:1] if k in pc.PER_SAMPLE else v) for k, v in pc.fleet_reference().items()}, w["qtime"], fleet_field(name))
        _CACHE[("vanchor", name)] = np.round(np.nan_to_num(r["value"][0]), 2)
    return _CACHE[("vanchor", name)]


def fleet_reference(name, nearest=False):
    """The restatement on the fleet with accumulators about ``fleet_vanchor(name)`` from zero, with details, computed once;
    read-only."""
    key = ("ref", name, nearest)
    if key not in _CACHE:
        w = pc.fleet()
        ref = field_values(pc.fleet_reference(), w["qtime"], fleet_field(name), nearest=nearest, vanchor=fleet_vanchor(name), details=True)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]
