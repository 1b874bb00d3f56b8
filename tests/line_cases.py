"""NumPy restatement of the line quantities (include/ste.h: ste_line_metrics_f64; DESIGN.md, "Lines"), operation for operation,
and the small batches its tests share.  The clock, the pieces and the soundness are those of site_cases, the frame and the
crossing rule those of region_metrics_cases, the metric that of site_cases.

The lines are a CSR list: ``vert`` (2, V) lon then lat, ``first`` (M + 1,), ``lon_ref`` (M,).  Line m owns vertices first[m] ..
first[m+1] - 1; segment j joins P = vertex j and Q = vertex j + 1.  For track t of sample s, tau_k = t0[t] + T_k:
    bad clock        a non-finite t0 or a dt_k, k < nsteps, that is not finite and >= 0: BAD_TIME, NaN / -1 / 0 for every line
    bad line         fewer than 2 vertices, a range outside [0, V], a non-finite lon_ref or vertex, a vertex with
                     |lon - lon_ref| <= 90 false: BAD_LINE, NaN / -1 / 0 for every track; with a bad range nothing is read
    piece            step k is (lo, hi) = (tau_k, tau_{k+1}), examined when hi > lo
    broken           |wrap180(lon_{k+1} - lon_k)| < 90 false or a non-finite latitude: nbroken += 1
    frame            x_k = ref + wrap180(lon_k - ref), A = (x_k, lat_k), B = (x_k + delta, lat_{k+1}), d = B - A
    crossing         e = Q - P, w = P - A, den = d.x e.y - d.y e.x, u = (w.x e.y - w.y e.x) / den, v = (w.x d.y - w.y d.x) / den;
                     one when den != 0, 0 <= u < 1, 0 <= v < 1; +1 in net_cross when den < 0, else -1; time lo + u (hi - lo)
    closest          kc = Kd cos(0.25 ((A.y + B.y) + (P.y + Q.y)) deg2rad); a0 = (kc w.x, Kd w.y), a1 likewise for Q,
                     dk = (kc d.x, Kd d.y), ek = a1 - a0, b0 = a0 - dk; candidates in order: the crossing (q = 0), P against the
                     step, Q against the step, A against the segment, B against the segment; the first smallest q wins;
                     min_dist is path_metrics_cases.leg_km from the ship's position at u to P + v (Q - P)
"""
import numpy as np
import path_metrics_cases as pmc
import site_cases as sc
from track_sampling_cases import wrap180

DEG2RAD, KD = sc.DEG2RAD, sc.KD
BAD_TIME, BAD_LINE = 0x1, 0x1
FLOAT_OUTPUTS = ("min_dist", "min_time", "min_frac", "first_cross", "last_cross")  # (S, M, B)
INT_OUTPUTS = ("min_seg", "ncross", "net_cross")
TRACK_OUTPUTS = ("sound_time", "nbroken")  # (S, B)
NAN_OUTPUTS = FLOAT_OUTPUTS  # NaN where there is nothing; min_seg is -1 and the counts are 0
_CACHE = {}
_finite = sc._finite


def pack(lines):
    """A list of (n_i, 2) lon / lat arrays as stored -> (vert (2, V), first (M + 1,) int32): no unwrapping, no checks."""
    lines = [np.asarray(ln, dtype=np.float64).reshape(-1, 2) for ln in lines]
    first = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(lines).T), first


def line_is_bad(vert, first, lon_ref, m):
    """(bad, range is good)."""
    V = vert.shape[1]
    f0, f1 = int(first[m]), int(first[m + 1])
    if not (f0 >= 0 and f1 <= V and f1 >= f0 + 2):
        return True, False
    ref = np.float64(lon_ref[m])
    x, y = vert[0, f0:f1], vert[1, f0:f1]
    with np.errstate(invalid="ignore"):
        good = _finite(ref) and bool(np.all((x * 0.0 == 0.0) & (y * 0.0 == 0.0) & (np.abs(x - ref) <= 90.0)))
    return not good, True


def _clamp01(x):
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def _pairs(x0, y0, dx, dy, ysum, px, py, qx, qy):
    """One sound step against every segment of a line at once: (cq, cu, cv, crossing, den, u, v, other) per segment; ``other`` is
    the smallest q of a candidate that is no crossing and is not the winner's own point: a candidate with the winner's u and
    either its v (a knot against a vertex is reached by two candidates, whose q differ by a rounding and whose record is the
    same) or its q to the bit (a segment of zero length: the same operands)."""
    inf = np.inf
    ex, ey = qx - px, qy - py
    wx, wy = px - x0, py - y0
    den = dx * ey - dy * ex
    u = (wx * ey - wy * ex) / den
    v = (wx * dy - wy * dx) / den
    cr = (den != 0.0) & (u >= 0.0) & (u < 1.0) & (v >= 0.0) & (v < 1.0)
    kc = KD * np.cos(0.25 * (ysum + (py + qy)) * DEG2RAD)
    a0x, a0y = kc * wx, KD * wy
    a1x, a1y = kc * (qx - x0), KD * (qy - y0)
    dkx, dky = kc * dx, KD * dy
    ekx, eky = a1x - a0x, a1y - a0y
    dd, ee = dkx * dkx + dky * dky, ekx * ekx + eky * eky
    b0x, b0y = a0x - dkx, a0y - dky
    zero, one = np.zeros_like(px), np.ones_like(px)
    u2 = np.where(dd > 0.0, _clamp01((a0x * dkx + a0y * dky) / dd), 0.0)
    gx, gy = a0x - u2 * dkx, a0y - u2 * dky
    q2 = gx * gx + gy * gy
    u3 = np.where(dd > 0.0, _clamp01((a1x * dkx + a1y * dky) / dd), 0.0)
    gx, gy = a1x - u3 * dkx, a1y - u3 * dky
    q3 = gx * gx + gy * gy
    v4 = np.where(ee > 0.0, _clamp01(-(a0x * ekx + a0y * eky) / ee), 0.0)
    gx, gy = a0x + v4 * ekx, a0y + v4 * eky
    q4 = gx * gx + gy * gy
    v5 = np.where(ee > 0.0, _clamp01(-(b0x * ekx + b0y * eky) / ee), 0.0)
    gx, gy = b0x + v5 * ekx, b0y + v5 * eky
    q5 = gx * gx + gy * gy
    Q = np.stack([np.where(cr, 0.0, inf), q2, q3, q4, q5])
    U = np.stack([np.where(cr, u, 0.0), u2, u3, zero, one])
    W = np.stack([np.where(cr, v, 0.0), zero, one, v4, v5])
    win = np.argmin(Q, axis=0)  # the first of equal ones: a later candidate replaces an earlier one only when it is closer
    j = np.arange(px.shape[0])
    cq, cu, cv = Q[win, j], U[win, j], W[win, j]
    same = (U == cu[None]) & ((W == cv[None]) | (Q == cq[None]))
    same[0] = True  # a crossing is decided without cos: it is nobody's runner-up
    other = np.where(same, inf, Q).min(axis=0)
    return cq, cu, cv, cr, den, u, v, other


def _track_line(lon, lat, dt, ns, t0, px, py, qx, qy, ref, model):
    """One (sample, line, track) of a good line and a finite t0 -> dict."""
    nan, inf = np.float64(np.nan), np.float64(np.inf)
    T = np.float64(0.0)
    best_q, runner, margin = inf, inf, inf
    min_time, pos, seg, frac = nan, None, -1, nan
    ncross = net = nbroken = 0
    first, last, sound_time, bad = nan, nan, np.float64(0.0), False
    L = px.shape[0]
    for k in range(ns):
        dtk = np.float64(dt[k])
        if not (dtk >= 0.0 and _finite(dtk)):
            bad = True
        lo, T1 = t0 + T, T + dtk
        hi = t0 + T1
        T = T1
        if not hi > lo:
            continue
        delta = wrap180(lon[k + 1] - lon[k])
        if not (bool(abs(delta) < 90.0) and _finite(lat[k]) and _finite(lat[k + 1])):
            nbroken += 1
            continue
        ln = hi - lo
        sound_time = sound_time + ln
        if L == 0:
            continue
        x0, y0, y1 = ref + wrap180(lon[k] - ref), lat[k], lat[k + 1]
        x1 = x0 + delta
        dx, dy, ysum = x1 - x0, y1 - y0, y0 + y1
        cq, cu, cv, cr, den, u, v, other = _pairs(x0, y0, dx, dy, ysum, px, py, qx, qy)
        if cr.any():
            ncross += int(cr.sum())
            net += int((den[cr] < 0.0).sum()) - int((den[cr] >= 0.0).sum())
            if not first == first:
                first = lo + u[cr].min() * ln
            last = lo + u[cr].max() * ln
        # how close a knot or a vertex is to deciding a crossing: u against 0 and 1 where v is in reach, and v likewise
        ok = den != 0.0
        eu, ev = np.minimum(np.abs(u), np.abs(u - 1.0)), np.minimum(np.abs(v), np.abs(v - 1.0))
        near_v, near_u = ok & (v >= -1e-9) & (v <= 1.0 + 1e-9), ok & (u >= -1e-9) & (u <= 1.0 + 1e-9)
        margin = min(margin, eu[near_v].min() if near_v.any() else inf, ev[near_u].min() if near_u.any() else inf)
        j = int(np.argmin(cq))  # the first of equal ones
        rest = np.where(cr, other, np.minimum(cq, other))  # per segment: the smallest q that is no crossing ...
        rest[j] = other[j]                                 # ... and, for the winner, not its own point
        step_runner = rest.min()
        if cq[j] < best_q:
            runner = min(best_q, step_runner)
            best_q = cq[j]
            min_time = lo + cu[j] * ln
            pos = (x0 + cu[j] * dx, y0 + cu[j] * dy)
            seg, frac = j, cv[j]
        else:
            runner = min(runner, step_runner, cq[j] if not cr[j] else inf)
    min_dist = nan
    if pos is not None:
        min_dist = pmc.leg_km(model, pos[0], pos[1], px[seg] + frac * (qx[seg] - px[seg]), py[seg] + frac * (qy[seg] - py[seg]))
    return dict(min_dist=min_dist, min_time=min_time, min_seg=seg, min_frac=frac, ncross=ncross, net_cross=net, first_cross=first,
                last_cross=last, sound_time=sound_time, nbroken=nbroken, bad=bad, best_q=best_q, runner_up_q=runner,
                knot_margin=margin)


def line_metrics(states, nsteps, dt, vert, first, lon_ref, t0=None, model="sphere"):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B), ``vert`` (2, V), ``first`` (M + 1,),
    ``lon_ref`` (M,), ``t0`` (B,) or None -> dict(min_dist, min_time, min_frac, first_cross, last_cross (S, M, B); min_seg,
    ncross, net_cross (S, M, B) int32; sound_time (S, B); nbroken (S, B) int32; track_status (B,) and line_status (M,) int32; and,
    beyond the kernel's outputs, best_q and runner_up_q (S, M, B), the smallest q and the smallest q of any other candidate that
    is no crossing (inf where there is none), and knot_margin (S, M, B), the least distance of a u or v from 0 or 1 where the
    other parameter is in reach of [0, 1])."""
    states = np.asarray(states, dtype=np.float64)
    vert = np.asarray(vert, dtype=np.float64)
    S, rows, _, B = states.shape
    M = len(lon_ref)
    t0 = np.zeros(B) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), (B,))
    out = {k: np.full((S, M, B), np.nan) for k in FLOAT_OUTPUTS}
    out.update({k: np.full((S, M, B), np.inf) for k in ("best_q", "runner_up_q", "knot_margin")})
    out.update({k: np.zeros((S, M, B), dtype=np.int32) for k in INT_OUTPUTS})
    out["min_seg"][:] = -1
    out["sound_time"], out["nbroken"] = np.zeros((S, B)), np.zeros((S, B), dtype=np.int32)
    out["track_status"], out["line_status"] = np.zeros((B,), dtype=np.int32), np.zeros((M,), dtype=np.int32)
    empty = np.zeros(0)
    geom = []
    for m in range(M):
        bad, _ = line_is_bad(vert, first, lon_ref, m)
        if bad:
            out["line_status"][m] = BAD_LINE
            geom.append(None)
        else:
            x, y = vert[0, first[m]:first[m + 1]], vert[1, first[m]:first[m + 1]]
            geom.append((x[:-1], y[:-1], x[1:], y[1:], np.float64(lon_ref[m])))
    with np.errstate(all="ignore"):
        for b in range(B):
            ns = min(max(int(nsteps[b]), 0), rows - 1)
            tb = np.float64(t0[b])
            if not _finite(tb) or not all(v >= 0.0 and _finite(v) for v in dt[:ns, b]):
                out["track_status"][b] = BAD_TIME
                continue
            for s in range(S):
                for m in range(M):
                    # a bad line is walked without segments for the track's own outputs, which do not depend on the line
                    g = geom[m] if geom[m] is not None else (empty, empty, empty, empty, np.float64(0.0))
                    r = _track_line(states[s, :, 0, b], states[s, :, 1, b], dt[:, b], ns, tb, *g, model)
                    out["sound_time"][s, b], out["nbroken"][s, b] = r["sound_time"], r["nbroken"]
                    if geom[m] is not None:
                        for k in FLOAT_OUTPUTS + INT_OUTPUTS + ("best_q", "runner_up_q", "knot_margin"):
                            out[k][s, m, b] = r[k]
    return out


def near_tie(ref):
    """(S, M, B) bool: another candidate's q is within 1e-9 relative of the best one's, so the time, the segment and the
    fraction may come from either."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(ref["best_q"]) & (ref["runner_up_q"] <= ref["best_q"] * (1.0 + 1e-9))


def knot_decides(ref):
    """(S, M, B) bool: a knot or a vertex within 1e-9 of deciding a crossing."""
    return ref["knot_margin"] < 1e-9


def clock_span(nsteps, dt):
    return sc.clock_span(nsteps, dt, None)


# ---- hand-made ships: one batch of 14 ships, Nmax = 6; every coordinate is a dyadic number ------------------------------------
HAND_B, HAND_N = 14, 6
HAND_SHIPS = ["equator", "zigzag", "stationary", "antimeridian", "broken", "no steps", "one step", "negative dt", "nan dt",
              "nan dt past nsteps", "nan t0", "zero step", "corner", "from the corner"]
HAND_LINES = {
    "bad start": ([(2.5, 1.0), (2.5, -1.0)], 2.5),            # first[0] is set to -1 below: line 0, whose block walks the tracks
    "gate": ([(2.5, 1.0), (2.5, -1.0)], 2.5),                 # the equator ship crosses it in the middle of step 2: +1
    "gate reversed": ([(2.5, -1.0), (2.5, 1.0)], 2.5),        # -1
    "bend": ([(2.0, -1.0), (2.5, 0.0), (2.0, 1.0)], 2.0),     # the equator ship crosses at the shared vertex: once
    "parallel": ([(1.0, 0.125), (5.0, 0.125)], 3.0),          # 0.125 degrees north of the equator ship
    "pier": ([(2.5, 0.25), (2.5, 1.25)], 2.5),                # its first vertex is closest (candidate 2)
    "pier reversed": ([(2.5, 1.25), (2.5, 0.25)], 2.5),       # its second vertex (candidate 3)
    "equator line": ([(0.0, 0.0), (8.0, 0.0)], 4.0),          # the zigzag crosses it three times; the corner ships' knots are closest
    "near the buoy": ([(39.0, 0.125), (41.0, 0.125)], 40.0),  # the stationary ships lie 0.125 degrees south of its middle
    "across 180": ([(180.125, 1.0), (180.125, -1.0)], 180.125),     # ship 3 is stored wrapped
    "across -180": ([(-179.875, 1.0), (-179.875, -1.0)], -179.875),  # the same gate under its other name
    "doubled vertex": ([(2.5, 1.25), (2.5, 0.25), (2.5, 0.25), (3.5, 0.25)], 3.0),  # a segment of zero length
    "one vertex": ([(2.5, 0.0)], 2.5),
    "nan lon_ref": ([(2.5, 1.0), (2.5, -1.0)], np.nan),
    "nan vertex": ([(2.5, 1.0), (np.nan, 0.0), (2.5, -1.0)], 2.5),
    "inf latitude": ([(2.5, 1.0), (2.5, np.inf)], 2.5),
    "too wide": ([(2.5, 1.0), (93.0, -1.0)], 2.5),            # 90.5 degrees from its lon_ref
    "bad end": ([(2.5, 1.0), (2.5, -1.0)], 2.5),              # first[M] is set to V + 1 below
}
HAND_BAD = ("bad start", "one vertex", "nan lon_ref", "nan vertex", "inf latitude", "too wide", "bad end")


def hand_batch():
    """dict(states (1, 7, 4, 14), nsteps, dt (6, 14), t0 (14,), vert, first, lon_ref)."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    B, N = HAND_B, HAND_N
    k = np.arange(N + 1.0)
    lon, lat = np.zeros((N + 1, B)), np.zeros((N + 1, B))
    dt = np.ones((N, B))
    nsteps = np.full(B, 4, dtype=np.int32)
    t0 = np.zeros(B)
    for b in (0, 5, 6, 7, 8, 9, 10):  # one degree an hour along the equator
        lon[:, b] = k
    nsteps[[0, 1]] = 6
    lon[:, 1], lat[:, 1] = 1.0 + k, np.array([-0.5, 0.5, -0.5, 0.5, 0.5, 0.5, 0.5])
    t0[1] = 0.25
    lon[:, [2, 11]] = 40.0
    t0[2] = 0.5
    lon[:, 3] = wrap180(179.75 + 0.25 * k)
    lon[:, 4], lat[:, 4] = 2.0 + 0.25 * k, 0.0  # over the gate in the middle of step 2, which a NaN latitude in row 2 breaks
    lat[2, 4] = np.nan
    nsteps[5], nsteps[6] = 0, 1
    dt[0, 7], dt[1, 8], dt[5, 9], t0[10] = -1.0, np.nan, np.nan, np.nan
    dt[1, 11] = 0.0
    lon[:, 12], lat[:, 12] = np.array([1.0, 2.0, 3.0, 3.0, 3.0, 3.0, 3.0]), np.array([1.0, 0.25, 1.0, 1.0, 1.0, 1.0, 1.0])
    lon[:, 13], lat[:, 13] = np.array([2.0, 3.0, 4.0, 4.0, 4.0, 4.0, 4.0]), np.array([0.25, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    t0[13] = 0.75
    st = np.zeros((1, N + 1, 4, B))
    st[0, :, 0], st[0, :, 1] = lon, lat
    vert, first = pack([v[0] for v in HAND_LINES.values()])
    first[0], first[-1] = -1, vert.shape[1] + 1
    lon_ref = np.array([v[1] for v in HAND_LINES.values()])
    _CACHE["hand"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, vert=vert, first=first, lon_ref=lon_ref)
    return _CACHE["hand"]


def check_hand_answers(r, what, model="sphere"):
    """The known answers of the hand-made ships, for the restatement and for the device alike."""
    ships, lines = HAND_SHIPS, list(HAND_LINES)
    names = FLOAT_OUTPUTS + INT_OUTPUTS

    def at(ship, line):
        b, m = ships.index(ship), lines.index(line)
        v = {k: r[k][0, m, b] for k in names}
        v.update({k: r[k][0, b] for k in TRACK_OUTPUTS})
        return v

    def close(got, want, tol, name):
        assert abs(got - want) <= tol, (what, name, got, want)

    def leg(*a):
        return pmc.leg_km(model, *a)

    def none(v):
        return np.isnan([v[k] for k in NAN_OUTPUTS]).all() and (v["min_seg"], v["ncross"], v["net_cross"]) == (-1, 0, 0)

    assert r["track_status"].tolist() == [BAD_TIME if s in ("negative dt", "nan dt", "nan t0") else 0 for s in ships], what
    assert r["line_status"].tolist() == [BAD_LINE if s in HAND_BAD else 0 for s in lines], what
    # a gate crossed in the middle of step 2: 0 km at 2.5 h, +1; -1 for the reversed line
    for line, sign in (("gate", 1), ("gate reversed", -1)):
        v = at("equator", line)
        assert (v["ncross"], v["net_cross"], v["min_seg"], v["nbroken"], v["sound_time"]) == (1, sign, 0, 0, 6.0), (what, line, v)
        assert (v["first_cross"], v["last_cross"], v["min_time"], v["min_frac"]) == (2.5, 2.5, 2.5, 0.5), (what, line, v)
        assert v["min_dist"] <= 1e-9, (what, line, v)
    # through the vertex the two segments share: v = 1 on the first is no crossing, v = 0 on the second is one; the closest
    # point is that vertex as the second one of segment 0 (candidate 3, q = 0), which the crossing ties with and loses to
    v = at("equator", "bend")
    assert (v["ncross"], v["net_cross"], v["min_seg"], v["min_frac"], v["first_cross"], v["min_time"]) == (1, -1, 0, 1.0, 2.5, 2.5), (what, v)
    assert v["min_dist"] <= 1e-9
    v = at("equator", "parallel")  # the end of step 0 is the first moment at the offset; every later one ties and loses
    assert (v["ncross"], v["min_seg"], v["min_frac"], v["min_time"]) == (0, 0, 0.0, 1.0) and np.isnan(v["first_cross"]), (what, v)
    close(v["min_dist"], leg(1.0, 0.0, 1.0, 0.125), 1e-10, "parallel")
    close(v["min_dist"], 0.125 * pmc.KM_PER_DEG_EQUATOR, 7e-3 * 0.125 * pmc.KM_PER_DEG_EQUATOR, "parallel")
    for line, fr in (("pier", 0.0), ("pier reversed", 1.0)):  # a vertex against the inside of step 2
        v = at("equator", line)
        assert (v["ncross"], v["min_seg"], v["min_frac"]) == (0, 0, fr), (what, line, v)
        close(v["min_time"], 2.5, 1e-12, line)
        close(v["min_dist"], leg(2.5, 0.0, 2.5, 0.25), 1e-10, line)
    v = at("equator", "doubled vertex")  # the pier again as the second vertex of segment 0: the zero-length segment ties and loses
    assert (v["ncross"], v["min_seg"], v["min_frac"]) == (0, 0, 1.0), (what, v)
    close(v["min_time"], 2.5, 1e-12, "doubled vertex")
    close(v["min_dist"], leg(2.5, 0.0, 2.5, 0.25), 1e-10, "doubled vertex")
    v = at("zigzag", "equator line")  # three crossings, in the middle of steps 0, 1 and 2, from t0 = 0.25
    assert (v["ncross"], v["net_cross"], v["first_cross"], v["last_cross"]) == (3, 1, 0.75, 2.75), (what, v)
    assert v["min_time"] == 0.75 and v["min_seg"] == 0 and v["min_frac"] == 1.5 / 8.0 and v["min_dist"] <= 1e-9, (what, v)
    v = at("stationary", "near the buoy")  # dd == 0: the start of the first step, and no crossing whatever den is
    assert (v["ncross"], v["min_seg"], v["min_frac"], v["min_time"], v["sound_time"]) == (0, 0, 0.5, 0.5, 4.0), (what, v)
    close(v["min_dist"], leg(40.0, 0.0, 40.0, 0.125), 1e-10, "stationary")
    a, b = at("antimeridian", "across 180"), at("antimeridian", "across -180")  # stored wrapped, over the gate in the middle of step 1
    assert (a["ncross"], a["net_cross"], a["first_cross"], a["min_time"], a["min_frac"]) == (1, 1, 1.5, 1.5, 0.5), (what, a)
    assert a["min_dist"] <= 1e-9 and b["min_dist"] <= 1e-9
    for k in names[1:]:  # one gate under two names: the same bits in everything planar
        assert np.array_equal(np.float64(a[k]).view(np.uint64), np.float64(b[k]).view(np.uint64)), (what, k, "180 against -180")
    v = at("broken", "gate")  # steps 1 and 2 touch the NaN row: the crossing is not seen, the end of step 0 is closest
    assert (v["nbroken"], v["sound_time"], v["ncross"], v["min_time"], v["min_frac"]) == (2, 2.0, 0, 1.0, 0.5), (what, v)
    close(v["min_dist"], leg(2.25, 0.0, 2.5, 0.0), 1e-10, "broken")
    for line in lines:
        if line in HAND_BAD:
            continue
        v = at("no steps", line)
        assert none(v) and (v["sound_time"], v["nbroken"]) == (0.0, 0), (what, line, v)
    v = at("one step", "gate")  # the first step of the equator ship alone: its end is closest
    assert (v["ncross"], v["min_time"], v["sound_time"]) == (0, 1.0, 1.0), (what, v)
    close(v["min_dist"], leg(1.0, 0.0, 2.5, 0.0), 1e-10, "one step")
    for ship in ("negative dt", "nan dt", "nan t0"):
        for line in lines:
            v = at(ship, line)
            assert none(v) and (v["sound_time"], v["nbroken"]) == (0.0, 0), (what, ship, line, v)
    p, q = at("nan dt past nsteps", "gate"), at("equator", "gate")  # four steps of the same course
    assert p["sound_time"] == 4.0 and all(p[k] == q[k] for k in names), (what, p, q)
    v = at("zero step", "near the buoy")  # a step of no length is skipped
    assert (v["sound_time"], v["nbroken"], v["min_time"], v["min_frac"]) == (3.0, 0, 0.0, 0.5), (what, v)
    v = at("corner", "equator line")  # the knot (2, 0.25) is closest: as the end of step 0 (candidate 5); the start of step 1 ties
    assert (v["ncross"], v["min_seg"], v["min_frac"], v["min_time"]) == (0, 0, 0.25, 1.0), (what, v)
    close(v["min_dist"], leg(2.0, 0.25, 2.0, 0.0), 1e-10, "corner")
    v = at("from the corner", "equator line")  # the same knot as the start of step 0 (candidate 4), at t0 = 0.75
    assert (v["ncross"], v["min_seg"], v["min_frac"], v["min_time"]) == (0, 0, 0.25, 0.75), (what, v)
    close(v["min_dist"], leg(2.0, 0.25, 2.0, 0.0), 1e-10, "from the corner")
    for line in HAND_BAD:  # a bad line gives NaN / -1 / 0 for every ship, and leaves the ships' own outputs alone
        m = lines.index(line)
        for k in NAN_OUTPUTS:
            assert np.isnan(r[k][0, m]).all(), (what, line, k)
        assert (r["min_seg"][0, m] == -1).all() and not r["ncross"][0, m].any() and not r["net_cross"][0, m].any(), (what, line)
    assert r["sound_time"][0].tolist() == [6.0, 6.0, 4.0, 4.0, 2.0, 0.0, 1.0, 0.0, 0.0, 4.0, 0.0, 3.0, 4.0, 4.0], what


# ---- the line fleet: S = 3, Nmax = 8, B = 130 (two waves plus two lanes), M = 9; dt and t0 are multiples of 2^-6 h ------------
FLEET_S, FLEET_N, FLEET_B, FLEET_M, FLEET_SEED = 3, 8, 130, 9, 1  # the seed: no near tie and no deciding knot (the tests assert it)
FLEET_WINDOW = (3, 70)
RING = 7  # the line that is a closed counter-clockwise ring


def fleet(chunk=64):
    """dict(states (3, 9, 4, 130), nsteps, dt (8, 130), t0 (130,), lines, vert, first, lon_ref, ring (12, 2)).  The ships are those of
    the port fleet's recipe: ships 0 .. 15 start at lon 179.6 .. 180.4, lat -20 +- 0.3, have full length, and the first eight are
    stored wrapped; ships 16 .. 129 start within 0.6 degrees of longitude and 0.4 of latitude of (10, 50) and have nsteps =
    b % 9; a drift of N(0, 0.12) degrees per step per ship plus N(0, 0.04) noise; dt a multiple of 2^-6 h in [0.3, 1.2], t0 one
    in [0, 2]; samples 1 and 2 are sample 0 plus N(0, 0.02) degrees; the rows past nsteps hold garbage.  Nine lines, of 1, 2, 3,
    c - 1, c, c + 1 and 2 c + 1 segments (c = ``chunk``, the kernel's), a closed 12-vertex star and a line with a doubled
    vertex: random walks of N(0, 0.03)-degree segments with a drift through the ships' waters, lines 1, 4 and 8 across the
    antimeridian (line 8 stored as -180 ..), the others about (10, 50)."""
    key = ("fleet", chunk)
    if key in _CACHE:
        return _CACHE[key]
    import region_metrics_cases as rmc

    rng = np.random.default_rng(FLEET_SEED)
    S, N, B = FLEET_S, FLEET_N, FLEET_B
    start = np.stack([10.0 + rng.uniform(-0.6, 0.6, B), 50.0 + rng.uniform(-0.4, 0.4, B)])
    start[0, :16], start[1, :16] = np.linspace(179.6, 180.4, 16), -20.0 + rng.uniform(-0.3, 0.3, 16)
    drift = rng.normal(0.0, 0.12, (2, B))
    steps = drift[None] + rng.normal(0.0, 0.04, (N, 2, B))
    st = np.zeros((S, N + 1, 4, B))
    st[0, 0, :2] = start
    st[0, 1:, :2] = start[None] + np.cumsum(steps, axis=0)
    st[1:, :, :2] = st[0, :, :2][None] + rng.normal(0.0, 0.02, (S - 1, N + 1, 2, B))
    st[:, :, 0, :8] = wrap180(st[:, :, 0, :8])
    st[:, :, 2:] = rng.normal(0.0, 1.0, (S, N + 1, 2, B))  # speed and heading: not read
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    nsteps[:16] = N
    dt = np.round(rng.uniform(0.3, 1.2, (N, B)) * 64.0) / 64.0
    t0 = np.round(rng.uniform(0.0, 2.0, B) * 64.0) / 64.0
    garbage = rng.normal(0.0, 1e3, st.shape)
    for b in range(B):
        st[:, nsteps[b] + 1:, :, b] = garbage[:, nsteps[b] + 1:, :, b]
    nseg = [1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, None, 3]
    lines = []
    for m, n in enumerate(nseg):
        centre = np.array([180.0, -20.0]) if m in (1, 4, 8) else np.array([10.0, 50.0])
        if n is None:
            # twelve radii of their own: in a symmetric star the two segments at a tip have the same mean latitude, and which
            # of them owns the tip would be decided by a rounding
            radii = (0.7, 0.3, 0.65, 0.35, 0.75, 0.28, 0.6, 0.33, 0.72, 0.31, 0.68, 0.36)
            lines.append(rmc.star((10.1, 50.1), radii, 12, wrapped=False))
            lines[-1] = np.concatenate([lines[-1], lines[-1][:1]])  # closed: the last vertex repeats the first
            continue
        span = 1.6
        th = rng.uniform(0.0, 2.0 * np.pi)
        way = np.array([np.cos(th), np.sin(th)])
        seg = way[None] * (span / n) + rng.normal(0.0, 0.3 * span / n, (n, 2))
        pts = np.concatenate([np.zeros((1, 2)), np.cumsum(seg, axis=0)])
        pts = pts - pts.mean(axis=0) + centre + rng.normal(0.0, 0.1, 2)
        if m == 8:
            pts = np.concatenate([pts[:2], pts[1:]])  # a doubled vertex: a segment of zero length
            pts[:, 0] = wrap180(pts[:, 0])
        lines.append(pts)
    vert, first = pack(lines)
    lon_ref = np.array([ln[0, 0] + 0.5 * (wrap180(ln[:, 0] - ln[0, 0]).min() + wrap180(ln[:, 0] - ln[0, 0]).max()) for ln in lines])
    for m, ln in enumerate(lines):  # as batch.track_lines stores them: unwrapped from the first vertex
        ln[:, 0] = ln[0, 0] + wrap180(ln[:, 0] - ln[0, 0])
    vert, first = pack(lines)
    _CACHE[key] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, lines=lines, vert=vert, first=first, lon_ref=lon_ref)
    return _CACHE[key]


def fleet_reference(model="sphere", chunk=64):
    """The restatement on the line fleet, computed once per model."""
    key = ("fleet", model, chunk)
    if key not in _CACHE:
        w = fleet(chunk)
        _CACHE[key] = line_metrics(w["states"], w["nsteps"], w["dt"], w["vert"], w["first"], w["lon_ref"], w["t0"], model)
    return _CACHE[key]
