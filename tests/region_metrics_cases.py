"""NumPy restatement of the region quantities (include/ste.h: ste_region_metrics_f64; DESIGN.md, "Regions"), operation for
operation, and the small batches its tests share.

The polygon is (2, V): px then py, counter-clockwise, every px within lon_ref +- 90 (track_estimators.batch.region_polygon makes
one).  Edge i joins P = vertex i and Q = vertex (i + 1) mod V.  For track t of sample s, ns = nsteps[t], rows 0 .. ns:
    row              x_k = lon_ref + wrap180(lon_k - lon_ref), y_k = lat_k
    row inside       outside unless xmin <= x <= xmax and ymin <= y <= ymax; else the parity of the edges with
                     (P.y > y) != (Q.y > y) and x < P.x + (y - P.y) * (Q.x - P.x) / (Q.y - P.y)
    step k           from A = (x_k, y_k) to B = (x_k + delta, y_{k+1}), delta = wrap180(lon_{k+1} - lon_k); BROKEN unless
                     |delta| < 90 and both latitudes are finite
    crossings        none if the step's box misses the polygon's (strict); else per edge d = B - A, e = Q - P, w = P - A,
                     den = d.x e.y - d.y e.x, u = (w.x e.y - w.y e.x) / den, v = (w.x d.y - w.y d.x) / den; a crossing when
                     den != 0, 0 <= u < 1, 0 <= v < 1; entering when den < 0
    fraction         acc = i0; in edge order acc += 1 - u (entering) or acc -= 1 - u (leaving); f = clamp(acc, 0, 1)
    time_inside      acc += dt_k * f_k over the sound steps in step order
    dist_inside      acc += leg_k * f_k over the sound steps with f_k > 0, leg_k of tests/path_metrics_cases.leg_km
    entering events  row 0 inside (time 0); entering crossings (T_k + dt_k * u, the smallest u of a step first); a broken step
                     whose row k + 1 is inside while row k is not (T_k + dt_k)
"""
import numpy as np
import path_metrics_cases as pmc
from track_sampling_cases import wrap180


def star(centre, radii, nvert, wrapped=True):
    """(nvert, 2) ring about ``centre``, counter-clockwise, vertex i at angle 2 pi i / nvert and radius radii[i % len(radii)];
    longitudes wrapped to [-180, 180) when ``wrapped``."""
    th = 2.0 * np.pi * np.arange(nvert) / nvert
    r = np.asarray(radii, dtype=np.float64)[np.arange(nvert) % len(radii)]
    lon = centre[0] + r * np.cos(th)
    if wrapped:
        lon = wrap180(lon)
    return np.stack([lon, centre[1] + r * np.sin(th)], axis=1)


def row_inside(vert, box, x, y):
    xmin, xmax, ymin, ymax = box
    if not (x >= xmin and x <= xmax and y >= ymin and y <= ymax):
        return False
    px, py = vert
    qx, qy = np.roll(px, -1), np.roll(py, -1)
    with np.errstate(all="ignore"):
        hit = ((py > y) != (qy > y)) & (x < px + (y - py) * (qx - px) / (qy - py))
    return bool(np.count_nonzero(hit) & 1)


def region_metrics(states, nsteps, dt, vert, lon_ref, model=None):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B), ``vert`` (2, V) and ``lon_ref`` of a
    normalised polygon -> dict(time_inside, first_entry (S, B), nenter, nbroken (S, B) int32, inside (S, N+1, B) uint8 with 0
    past nsteps, ncrossings (S, B) int32: crossings of either kind, total_time (B,)); with ``model`` also dist_inside and
    total_dist (S, B), the legs of the sound steps summed."""
    states = np.asarray(states, dtype=np.float64)
    vert = np.asarray(vert, dtype=np.float64)
    lon_ref = np.float64(lon_ref)
    S, rows, _, B = states.shape
    px, py = vert
    qx, qy = np.roll(px, -1), np.roll(py, -1)
    ex, ey = qx - px, qy - py
    box = (px.min(), px.max(), py.min(), py.max())
    xmin, xmax, ymin, ymax = box
    out = {"time_inside": np.zeros((S, B)), "first_entry": np.full((S, B), np.nan), "nenter": np.zeros((S, B), dtype=np.int32),
           "nbroken": np.zeros((S, B), dtype=np.int32), "inside": np.zeros((S, rows, B), dtype=np.uint8),
           "ncrossings": np.zeros((S, B), dtype=np.int32), "total_time": np.zeros((B,))}
    if model is not None:
        out["dist_inside"], out["total_dist"] = np.zeros((S, B)), np.zeros((S, B))
    for s in range(S):
        for t in range(B):
            ns = int(nsteps[t])
            lon, lat = states[s, : ns + 1, 0, t], states[s, : ns + 1, 1, t]
            x = lon_ref + wrap180(lon - lon_ref)
            i0 = row_inside(vert, box, x[0], lat[0])
            out["inside"][s, 0, t] = i0
            T = tin = din = total = np.float64(0.0)
            first, nent, nbrk, ncr = (0.0 if i0 else np.nan), int(i0), 0, 0
            for k in range(ns):
                ax, ay, by, dtk = x[k], lat[k], lat[k + 1], np.float64(dt[k, t])
                delta = wrap180(lon[k + 1] - lon[k])
                bx = ax + delta
                i1 = row_inside(vert, box, x[k + 1], by)
                out["inside"][s, k + 1, t] = i1
                if abs(delta) < 90.0 and np.isfinite(ay) and np.isfinite(by):
                    acc, umin, ent = np.float64(1.0 if i0 else 0.0), None, 0
                    if not (max(ax, bx) < xmin or min(ax, bx) > xmax or max(ay, by) < ymin or min(ay, by) > ymax):
                        dx, dy = bx - ax, by - ay
                        wx, wy = px - ax, py - ay
                        with np.errstate(all="ignore"):
                            den = dx * ey - dy * ex
                            u = (wx * ey - wy * ex) / den
                            v = (wx * dy - wy * dx) / den
                        for i in np.flatnonzero((den != 0.0) & (u >= 0.0) & (u < 1.0) & (v >= 0.0) & (v < 1.0)):
                            ncr += 1
                            if den[i] < 0.0:
                                acc = acc + (1.0 - u[i])
                                ent += 1
                                umin = u[i] if umin is None or u[i] < umin else umin
                            else:
                                acc = acc - (1.0 - u[i])
                    f = np.float64(min(max(acc, 0.0), 1.0))
                    if ent > 0 and nent == 0:
                        first = T + dtk * umin
                    nent += ent
                    tin = tin + dtk * f
                    if model is not None:
                        leg = pmc.leg_km(model, lon[k], ay, lon[k + 1], by)
                        total = total + leg
                        if f > 0.0:
                            din = din + leg * f
                else:
                    nbrk += 1
                    if i1 and not i0:
                        if nent == 0:
                            first = T + dtk
                        nent += 1
                T = T + dtk
                i0 = i1
            out["time_inside"][s, t], out["first_entry"][s, t] = tin, first
            out["nenter"][s, t], out["nbroken"][s, t], out["ncrossings"][s, t] = nent, nbrk, ncr
            out["total_time"][t] = T
            if model is not None:
                out["dist_inside"][s, t], out["total_dist"][s, t] = din, total
    return out


# ---- hand-made tracks: the equator at one degree an hour against the square [2.5, 6.5] x [-1, 1] ------------------------------
HAND_N = 10
SQUARE = np.array([[2.5, -1.0], [6.5, -1.0], [6.5, 1.0], [2.5, 1.0]])


def hand_polygons():
    """name -> (ring as a caller would give it, shift in longitude of the tracks that go with it, tracks stored wrapped?): the
    square counter-clockwise; clockwise with a repeated closing vertex; moved to [178, 182] x [-1, 1] across the antimeridian,
    its longitudes and the tracks' wrapped to [-180, 180)."""
    cw_closed = np.concatenate([SQUARE[::-1], SQUARE[-1:]])
    anti = SQUARE + np.array([175.5, 0.0])
    anti[:, 0] = wrap180(anti[:, 0])
    return {"ccw": (SQUARE, 0.0, False), "cw+closing": (cw_closed, 0.0, False), "antimeridian": (anti, 175.5, True)}


def hand_tracks(shift=0.0, wrapped=False):
    """(states (1, 11, 4, 3), nsteps, dt): the equator from lon 0 to 10 (inside from 2.5 h to 6.5 h); the same rows cut after
    two steps (never inside); the equator from lon 4 for one step (starts inside)."""
    st = pmc.states_of([pmc.equator_track(HAND_N, shift), pmc.equator_track(HAND_N, shift), pmc.equator_track(HAND_N, shift + 4.0)])
    if wrapped:
        st[:, :, 0] = wrap180(st[:, :, 0])
    return st, np.array([HAND_N, 2, 1], dtype=np.int32), np.ones((HAND_N, 3))


HAND_TIME, HAND_FIRST, HAND_NENTER = [4.0, 0.0, 1.0], [2.5, np.nan, 0.0], [1, 0, 1]

# ---- the mapping fleet: S = 5, Nmax = 8, B = 130 (two full waves plus two lanes) about a star across the antimeridian ----------
FLEET_S, FLEET_N, FLEET_B, FLEET_SEED = 5, 8, 130, 11
FLEET_WINDOW = (3, 70)
CENTRE = (179.6, 10.0)
NAN_TRACK, JUMP_TRACK = 8, 17  # two of the tracks with nsteps = Nmax
_CACHE = {}


def star12(east=0.0):
    """The concave 12-vertex star, radii 1.2 and 0.45 alternating, about (179.6 + east, 10): it straddles the antimeridian."""
    return star((CENTRE[0] + east, CENTRE[1]), (1.2, 0.45), 12)


def fleet():
    """dict(states (5, 9, 4, 130), nsteps (every length 0 .. 8), dt (8, 130)).  Starts uniform within 2 degrees of the star's
    centre, a per-track drift N(0, 0.45) plus per-step noise N(0, 0.25) degrees, longitudes wrapped to [-180, 180).  Track
    NAN_TRACK waits west of the star, has a NaN latitude in row 4 and sits at the centre from row 5 on; track JUMP_TRACK sits
    120 degrees west of the centre up to row 3 and at the centre from row 4 on."""
    if "fleet" in _CACHE:
        return _CACHE["fleet"]
    rng = np.random.default_rng(FLEET_SEED)
    S, N, B = FLEET_S, FLEET_N, FLEET_B
    st = np.zeros((S, N + 1, 4, B))
    start = np.stack([CENTRE[0] + rng.uniform(-2.0, 2.0, B), CENTRE[1] + rng.uniform(-2.0, 2.0, B)])
    drift = rng.normal(0.0, 0.45, (2, B))
    steps = drift[None, None] + rng.normal(0.0, 0.25, (S, N, 2, B))
    st[:, 0, :2] = start
    st[:, 1:, :2] = start[None, None] + np.cumsum(steps, axis=1)
    st[:, :, 2:] = rng.normal(0.0, 1.0, (S, N + 1, 2, B))  # speed and heading: not read
    st[:, :, 0, NAN_TRACK], st[:, :, 1, NAN_TRACK] = CENTRE[0] - 3.0, CENTRE[1]
    st[:, 4, 1, NAN_TRACK] = np.nan
    st[:, 5:, 0, NAN_TRACK] = CENTRE[0]
    st[:, :, 0, JUMP_TRACK], st[:, :, 1, JUMP_TRACK] = CENTRE[0] - 120.0, CENTRE[1]
    st[:, 4:, 0, JUMP_TRACK] = CENTRE[0]
    st[:, :, 0] = wrap180(st[:, :, 0])
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    assert nsteps[NAN_TRACK] == N and nsteps[JUMP_TRACK] == N
    _CACHE["fleet"] = dict(states=st, nsteps=nsteps, dt=rng.uniform(0.2, 1.5, (N, B)))
    return _CACHE["fleet"]


def fleet_reference(name, ring, model=None):
    """The restatement on the mapping fleet for a ring as a caller gives it (normalised by batch.region_polygon), computed once
    per (name, model)."""
    from track_estimators import batch

    key = ("ref", name, model)
    if key not in _CACHE:
        w, poly = fleet(), ring if isinstance(ring, batch.RegionPolygon) else batch.region_polygon(ring)
        _CACHE[key] = region_metrics(w["states"], w["nsteps"], w["dt"], poly.vert, poly.lon_ref, model)
    return _CACHE[key]
