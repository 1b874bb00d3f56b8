"""NumPy restatement of the site quantities (include/ste.h: ste_site_metrics_f64; DESIGN.md, "Sites"), operation for operation,
and the small batches its tests share.  A site is a ship that does not move and has no clock: the rules are those of
encounter_cases specialised to that, and ``as_encounters`` turns a batch and its sites into the encounter call that must give the
same bits.

For track t of sample s and site (X, Y, R), with tau_k = t0[t] + T_k, T_{k+1} = T_k + dt_k:
    bad clock        a non-finite t0 or a dt_k, k < nsteps, that is not finite and >= 0: BAD_TIME, NaN for min_dist, min_time and
                     first_within, 0 for the rest, for every site
    bad site         a non-finite X or Y, or R not finite, < 0 or > 1000: BAD_SITE, NaN / 0 for every track
    piece            step k is (lo, hi) = (tau_k, tau_{k+1}), examined when hi > lo; a skipped step closes every run
    broken           |wrap180(lon_{k+1} - lon_k)| < 90 false or a non-finite latitude: nbroken += 1, the runs are closed
    relative         x1 = x0 + delta, gx0 = wrap180(X - x0), gx1 = gx0 - (x1 - x0), gy = Y - y, scaled by Kd cos(mean lat) and Kd:
                     r0, r1, d = r1 - r0, dd = d.d, bq = r0.d, r00 = r0.r0
    closest          u* = clamp01(-bq / dd) (0 when dd is not > 0), q = |r0 + u* d|^2, the first smallest q wins; min_dist is
                     path_metrics_cases.leg_km from the ship's position at u* to the site
    within R         the roots of |r0 + u d|^2 = R^2 clipped to [0, 1]; runs are joined across steps when ua == 0; longest is
                     the largest sum of a run's pieces
"""
import encounter_cases as enc
import numpy as np
import path_metrics_cases as pmc
from track_sampling_cases import wrap180

DEG2RAD = enc.DEG2RAD
KD = enc.KD
BAD_TIME, BAD_SITE = 0x1, 0x1
MAX_RADIUS_KM = 1000.0
FLOAT_OUTPUTS = ("min_dist", "min_time", "time_within", "first_within", "longest")  # (S, M, B)
INT_OUTPUTS = ("nwithin",)
TRACK_OUTPUTS = ("sound_time", "nbroken")  # (S, B)
_CACHE = {}
clamp01, _finite = enc.clamp01, enc._finite


def site_is_bad(X, Y, R):
    return not (_finite(X) and _finite(Y) and R >= 0.0 and R <= MAX_RADIUS_KM)


def _track_site(lon, lat, dt, ns, t0, X, Y, R, model):
    """One (sample, site, track) of a good site and a finite t0: (min_dist, min_time, time_within, first_within, longest,
    nwithin, sound_time, nbroken, bad clock, best_q, runner_up_q, knot_margin)."""
    nan, inf = np.float64(np.nan), np.float64(np.inf)
    R2 = R * R
    T = np.float64(0.0)
    best_q, runner, min_time, pos = inf, inf, nan, None
    within, first, longest, run, sound_time = np.float64(0.0), nan, np.float64(0.0), np.float64(0.0), np.float64(0.0)
    nwithin = nbroken = 0
    open_, bad, margin = False, False, inf

    def close():
        nonlocal open_, longest, run
        if run > longest:
            longest = run
        open_, run = False, np.float64(0.0)

    for k in range(ns):
        dtk = np.float64(dt[k])
        if not (dtk >= 0.0 and _finite(dtk)):
            bad = True
        lo, T1 = t0 + T, T + dtk
        hi = t0 + T1
        T = T1
        if not hi > lo:
            close()
            continue
        delta = wrap180(lon[k + 1] - lon[k])
        if not (bool(abs(delta) < 90.0) and _finite(lat[k]) and _finite(lat[k + 1])):
            nbroken += 1
            close()
            continue
        ln = hi - lo
        sound_time = sound_time + ln
        x0, y0, y1 = lon[k], lat[k], lat[k + 1]
        x1 = x0 + delta
        gx0, gy0 = wrap180(X - x0), Y - y0
        gx1, gy1 = gx0 - (x1 - x0), Y - y1
        kc = KD * np.cos(0.25 * ((y0 + y1) + (Y + Y)) * DEG2RAD)
        r0x, r0y, r1x, r1y = kc * gx0, KD * gy0, kc * gx1, KD * gy1
        dx, dy = r1x - r0x, r1y - r0y
        dd, bq, r00 = dx * dx + dy * dy, r0x * dx + r0y * dy, r0x * r0x + r0y * r0y
        us = clamp01(-bq / dd) if dd > 0.0 else 0.0
        mx, my = r0x + us * dx, r0y + us * dy
        q = mx * mx + my * my
        if q < best_q:
            runner, best_q = best_q, q
            min_time = lo + us * ln
            pos = (x0 + us * (x1 - x0), y0 + us * (y1 - y0))
        elif q < runner:
            runner = q
        if R > 0.0:  # how far, relative to R, the ends of the piece are from the circle: a knot on it decides a run by a rounding
            for e in (r00, r1x * r1x + r1y * r1y):
                margin = min(margin, abs(np.sqrt(e) - R) / R)
        ua = ub = 0.0
        if dd > 0.0:
            disc = bq * bq - dd * (r00 - R2)
            if disc >= 0.0:
                sq = np.sqrt(disc)
                va, vb = (-bq - sq) / dd, (-bq + sq) / dd
                ua = va if va > 0.0 else 0.0
                ub = vb if vb < 1.0 else 1.0
        elif dd == 0.0 and r00 <= R2:
            ub = 1.0
        if ub > ua:
            w = (ub - ua) * ln
            within = within + w
            if not (open_ and ua == 0.0):
                close()
                if nwithin == 0:
                    first = lo + ua * ln
                nwithin += 1
                run = w
            else:
                run = run + w
            open_ = True
            if not ub == 1.0:
                close()
        else:
            close()
    close()
    min_dist = nan if pos is None else pmc.leg_km(model, pos[0], pos[1], X, Y)
    return min_dist, min_time, within, first, longest, nwithin, sound_time, nbroken, bad, best_q, runner, margin


def site_metrics(states, nsteps, dt, sites, radius_km, t0=None, model="sphere"):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B), ``sites`` (M, 2) lon / lat, ``radius_km`` a
    scalar or (M,), ``t0`` (B,) or None -> dict(min_dist, min_time, time_within, first_within, longest (S, M, B); nwithin (S, M, B)
    int32; sound_time (S, B); nbroken (S, B) int32; track_status (B,) and site_status (M,) int32; and, beyond the kernel's
    outputs, best_q and runner_up_q (S, M, B), the smallest and the second smallest q of the sound pieces (inf where there is
    none), and knot_margin (S, M, B), the least |distance - R| / R over the ends of the sound pieces)."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    sites = np.asarray(sites, dtype=np.float64)
    M = sites.shape[0]
    radius = np.broadcast_to(np.asarray(radius_km, dtype=np.float64), (M,))
    t0 = np.zeros(B) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), (B,))
    out = {k: np.zeros((S, M, B)) for k in FLOAT_OUTPUTS}
    out.update({k: np.full((S, M, B), np.inf) for k in ("best_q", "runner_up_q", "knot_margin")})
    out["nwithin"] = np.zeros((S, M, B), dtype=np.int32)
    out["sound_time"], out["nbroken"] = np.zeros((S, B)), np.zeros((S, B), dtype=np.int32)
    out["track_status"], out["site_status"] = np.zeros((B,), dtype=np.int32), np.zeros((M,), dtype=np.int32)
    for k in ("min_dist", "min_time", "first_within"):
        out[k][:] = np.nan
    with np.errstate(all="ignore"):
        for m in range(M):
            if site_is_bad(sites[m, 0], sites[m, 1], radius[m]):
                out["site_status"][m] = BAD_SITE
        for b in range(B):
            ns = min(max(int(nsteps[b]), 0), rows - 1)
            tb = np.float64(t0[b])
            if not _finite(tb) or not all(v >= 0.0 and _finite(v) for v in dt[:ns, b]):
                out["track_status"][b] = BAD_TIME
                continue
            for s in range(S):
                for m in range(M):
                    # a bad site is walked with a radius of 0 for the track's own outputs, which do not depend on the site
                    good = not out["site_status"][m]
                    r = _track_site(states[s, :, 0, b], states[s, :, 1, b], dt[:, b], ns, tb,
                                    np.float64(sites[m, 0]) if good else np.float64(0.0),
                                    np.float64(sites[m, 1]) if good else np.float64(0.0),
                                    np.float64(radius[m]) if good else np.float64(0.0), model)
                    out["sound_time"][s, b], out["nbroken"][s, b] = r[6], r[7]
                    if good:
                        for k, v in zip(FLOAT_OUTPUTS + INT_OUTPUTS, r[:6]):
                            out[k][s, m, b] = v
                        out["best_q"][s, m, b], out["runner_up_q"][s, m, b], out["knot_margin"][s, m, b] = r[9], r[10], r[11]
    return out


def near_tie(ref):
    """(S, M, B) bool: encounter_cases.near_tie."""
    return enc.near_tie(ref)


def grazing(ref, radius_km):
    """(S, M, B) bool: encounter_cases.grazing with the site's own radius, or an end of a sound piece within 1e-9 relative of the
    circle (whether a run goes on into the next step is then decided by a rounding)."""
    R = np.broadcast_to(np.asarray(radius_km, dtype=np.float64), (ref["best_q"].shape[1],))[None, :, None]
    with np.errstate(invalid="ignore"):
        return enc.grazing(ref, R) | (ref["knot_margin"] < 1e-9)


def clock_span(nsteps, dt, t0):
    """(B,) hours from row 0 to row nsteps of each track: the scale of a time's tolerance."""
    B = dt.shape[1]
    return np.array([dt[: int(nsteps[b]), b].sum() for b in range(B)])


def as_encounters(states, nsteps, dt, t0, sites):
    """The batch with one stationary ship per site appended (nsteps = 1, t0 = the smallest t0 - 1, dt = the largest span + 2, so its
    one step holds every clock) and the full list of (track, site) pairs, sorted by (track, site): dict(states, nsteps, dt, t0,
    pairs) for encounter_cases.encounter_metrics or the device's encounter call.  Pair b * M + m is track b against site m."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    M = len(sites)
    end = t0 + np.array([dt[: int(nsteps[b]), b].sum() for b in range(B)])
    st = np.zeros((S, rows, 4, B + M))
    st[..., :B] = states
    st[:, :, 0, B:], st[:, :, 1, B:] = sites[:, 0], sites[:, 1]
    dt2 = np.ones((dt.shape[0], B + M))
    dt2[:, :B] = dt
    dt2[0, B:] = (end.max() - t0.min()) + 2.0
    pairs = np.array([(b, B + m) for b in range(B) for m in range(M)], dtype=np.int32)
    return dict(states=st, nsteps=np.concatenate([nsteps, np.ones(M, dtype=np.int32)]).astype(np.int32), dt=dt2,
                t0=np.concatenate([t0, np.full(M, t0.min() - 1.0)]), pairs=pairs)


# ---- hand-made ships: one batch of 12 ships, Nmax = 6, against 15 sites; every coordinate is a dyadic number ------------------
HAND_R = 30.0
HAND_B, HAND_N = 12, 6
HAND_SHIPS = ["crossing", "zigzag", "stationary", "antimeridian", "broken", "no steps", "one step", "negative dt", "nan dt",
              "nan dt past nsteps", "nan t0", "zero step"]
HAND_SITES = {
    "on the equator": (2.5, 0.0, HAND_R),      # ship 0 sails over it in the middle of step 2
    "off the course": (2.5, 0.125, HAND_R),    # ship 0 passes it 0.125 degrees of latitude away
    "harbour": (20.0, 0.0, HAND_R),            # the zigzag pauses next to it, leaves and comes back
    "near buoy": (40.0, 0.125, HAND_R),        # the stationary ships lie 0.125 degrees from it ...
    "far buoy": (40.0, 1.0, HAND_R),           # ... and a degree from this one
    "across 180": (180.125, 0.0, HAND_R),      # ship 3 is stored wrapped
    "at 180": (180.0, 0.0625, HAND_R),
    "at -180": (-180.0, 0.0625, HAND_R),       # the same point: the same bits
    "anchorage": (30.25, 0.125, HAND_R),       # ship 4 stays within R of it throughout; its row 2 has a NaN latitude
    "small": (0.5, 0.0, 10.0),                 # a radius of its own
    "nan lon": (np.nan, 0.0, HAND_R),
    "nan lat": (2.5, np.nan, HAND_R),
    "nan radius": (2.5, 0.0, np.nan),
    "negative radius": (2.5, 0.0, -1.0),
    "radius above the limit": (2.5, 0.0, 1000.5),
}


def hand_batch():
    """dict(states (1, 7, 4, 12), nsteps, dt (6, 12), t0 (12,), sites (15, 2), radius (15,))."""
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
    lon[:, 1], lat[:, 1] = 20.0 + np.array([-1.0, 0.0, 0.0, 1.0, 1.0, 0.0, -1.0]), 0.125
    lon[:, [2, 11]] = 40.0
    t0[2] = 0.5
    lon[:, 3] = wrap180(179.75 + 0.25 * k)
    lon[:, 4], lat[:, 4] = 30.0 + 0.125 * k, 0.125
    lat[2, 4] = np.nan
    nsteps[5], nsteps[6] = 0, 1
    dt[0, 7], dt[1, 8], dt[5, 9], t0[10] = -1.0, np.nan, np.nan, np.nan
    dt[1, 11] = 0.0
    st = np.zeros((1, N + 1, 4, B))
    st[0, :, 0], st[0, :, 1] = lon, lat
    sites = np.array([v[:2] for v in HAND_SITES.values()])
    radius = np.array([v[2] for v in HAND_SITES.values()])
    _CACHE["hand"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, sites=sites, radius=radius)
    return _CACHE["hand"]


def check_hand_answers(r, what, model="sphere"):
    """The known answers of the hand-made ships, for the restatement and for the device alike."""
    ships, sites = HAND_SHIPS, list(HAND_SITES)
    km = pmc.KM_PER_DEG_EQUATOR
    names = FLOAT_OUTPUTS + INT_OUTPUTS

    def at(ship, site):
        b, m = ships.index(ship), sites.index(site)
        v = {k: r[k][0, m, b] for k in names}
        v.update({k: r[k][0, b] for k in TRACK_OUTPUTS})
        return v

    def close(got, want, tol, name):
        assert abs(got - want) <= tol, (what, name, got, want)

    def leg(*a):
        return pmc.leg_km(model, *a)

    assert r["track_status"].tolist() == [BAD_TIME if s in ("negative dt", "nan dt", "nan t0") else 0 for s in ships], what
    assert r["site_status"].tolist() == [BAD_SITE if s.startswith(("nan", "negative", "radius above")) else 0 for s in sites], what
    v = at("crossing", "on the equator")  # a degree an hour over the site: 0 km at 2.5 h, 2 R / speed within
    assert v["min_dist"] <= 1e-9 and v["nwithin"] == 1 and v["nbroken"] == 0 and v["sound_time"] == 6.0, (what, v)
    close(v["min_time"], 2.5, 1e-12, "crossing")
    close(v["time_within"], 2.0 * HAND_R / km, 1e-12, "crossing")
    close(v["first_within"], 2.5 - HAND_R / km, 1e-12, "crossing")
    assert v["longest"] == v["time_within"]
    half = np.sqrt(HAND_R ** 2 - (0.125 * km) ** 2) / (km * np.cos(np.radians(0.0625)))  # half a chord, in hours at a degree an hour
    v = at("crossing", "off the course")
    close(v["min_dist"], leg(2.5, 0.0, 2.5, 0.125), 1e-10, "pass at distance")
    close(v["min_dist"], 0.125 * km, 7e-3 * 0.125 * km, "pass at distance")
    close(v["min_time"], 2.5, 1e-12, "pass at distance")
    close(v["time_within"], 2.0 * half, 1e-12, "pass at distance")
    close(v["first_within"], 2.5 - half, 1e-12, "pass at distance")
    assert v["nwithin"] == 1 and v["longest"] == v["time_within"]
    v = at("crossing", "small")
    close(v["time_within"], 2.0 * 10.0 / km, 1e-12, "a radius of its own")
    close(v["min_time"], 0.5, 1e-12, "a radius of its own")
    v = at("zigzag", "harbour")  # in over step 0, a pause of an hour beside it, out over step 2; away; in and out again
    assert v["nwithin"] == 2 and v["nbroken"] == 0 and v["sound_time"] == 6.0, (what, v)
    close(v["time_within"], 1.0 + 4.0 * half, 1e-12, "zigzag")
    close(v["longest"], 1.0 + 2.0 * half, 1e-12, "zigzag")
    close(v["first_within"], 1.0 - half, 1e-12, "zigzag")
    close(v["min_dist"], leg(20.0, 0.125, 20.0, 0.0), 1e-10, "zigzag")
    assert v["min_time"] == 1.0
    v = at("stationary", "near buoy")  # dd == 0 inside R: the whole clock, from t0 = 0.5
    assert (v["time_within"], v["longest"], v["nwithin"], v["first_within"], v["min_time"], v["sound_time"]) == (4.0, 4.0, 1, 0.5, 0.5, 4.0), (what, v)
    close(v["min_dist"], leg(40.0, 0.0, 40.0, 0.125), 1e-10, "stationary, inside")
    v = at("stationary", "far buoy")  # dd == 0 outside R
    assert (v["time_within"], v["longest"], v["nwithin"], v["min_time"]) == (0.0, 0.0, 0, 0.5) and np.isnan(v["first_within"]), (what, v)
    close(v["min_dist"], leg(40.0, 0.0, 40.0, 1.0), 1e-10, "stationary, outside")
    v = at("antimeridian", "across 180")  # a quarter of a degree an hour over the site in the middle of step 1, stored wrapped
    assert v["min_dist"] <= 1e-9 and v["nwithin"] == 1 and v["nbroken"] == 0, (what, v)
    close(v["min_time"], 1.5, 1e-12, "antimeridian")
    close(v["time_within"], 2.0 * HAND_R / (0.25 * km), 1e-12, "antimeridian")
    close(v["first_within"], 1.5 - HAND_R / (0.25 * km), 1e-12, "antimeridian")
    close(v["longest"], v["time_within"], 1e-12, "antimeridian")
    a, b = sites.index("at 180"), sites.index("at -180")
    for k in names[1:]:  # one point under two names: the same bits in everything planar
        assert np.array_equal(r[k][0, a].view(np.uint64) if r[k].dtype == np.float64 else r[k][0, a],
                              r[k][0, b].view(np.uint64) if r[k].dtype == np.float64 else r[k][0, b]), (what, k, "180 against -180")
    # min_dist is the leg function on the longitude as given.  For the ship that sails past the point the two names give the
    # same bits there too; for ships a hemisphere away (15 585 km: a haversine of a longitude difference of 140 against -220
    # degrees) the same distance within the leg's own tolerance, 3 ulp apart in NumPy
    da, db = r["min_dist"][0, a], r["min_dist"][0, b]
    assert np.array_equal(np.isnan(da), np.isnan(db)), (what, "180 against -180")
    near = ships.index("antimeridian")
    assert da[near].tobytes() == db[near].tobytes() and da[near] > 0.0, (what, "min_dist", "180 against -180", da[near], db[near])
    assert np.allclose(da, db, rtol=pmc.DIST_RTOL, atol=pmc.DIST_ATOL, equal_nan=True), (what, "min_dist", "180 against -180")
    assert at("antimeridian", "at 180")["nwithin"] == 1 and at("antimeridian", "at 180")["min_time"] == 1.0
    v = at("broken", "anchorage")  # within R throughout; steps 1 and 2 touch the NaN row: the run is cut in two
    assert (v["nbroken"], v["nwithin"], v["sound_time"], v["time_within"], v["longest"], v["first_within"]) == (2, 2, 2.0, 2.0, 1.0, 0.0), (what, v)
    assert v["min_time"] == 1.0  # the end of step 0 and the start of step 3 are equally far: the first wins
    close(v["min_dist"], leg(30.125, 0.125, 30.25, 0.125), 1e-10, "broken")
    for site in sites:
        if r["site_status"][sites.index(site)]:
            continue
        v = at("no steps", site)
        assert np.isnan([v["min_dist"], v["min_time"], v["first_within"]]).all(), (what, site, v)
        assert (v["time_within"], v["longest"], v["nwithin"], v["sound_time"], v["nbroken"]) == (0.0, 0.0, 0, 0.0, 0), (what, site, v)
    v = at("one step", "small")  # the first step of the crossing ship alone
    assert v["min_dist"] <= 1e-9 and v["nwithin"] == 1 and v["sound_time"] == 1.0, (what, v)
    close(v["min_time"], 0.5, 1e-12, "one step")
    v = at("one step", "on the equator")
    assert v["min_time"] == 1.0 and v["nwithin"] == 0
    close(v["min_dist"], leg(1.0, 0.0, 2.5, 0.0), 1e-10, "one step")
    for ship in ("negative dt", "nan dt", "nan t0"):
        for site in sites:
            v = at(ship, site)
            assert np.isnan([v["min_dist"], v["min_time"], v["first_within"]]).all(), (what, ship, site, v)
            assert (v["time_within"], v["longest"], v["nwithin"], v["sound_time"], v["nbroken"]) == (0.0, 0.0, 0, 0.0, 0), (what, ship, v)
    p, q = at("nan dt past nsteps", "on the equator"), at("crossing", "on the equator")  # four steps of the same course
    assert p["sound_time"] == 4.0 and all(p[k] == q[k] for k in names), (what, p, q)
    v = at("zero step", "near buoy")  # a stay of three hours with a step of no length after the first: two runs
    assert (v["time_within"], v["longest"], v["nwithin"], v["first_within"], v["sound_time"], v["nbroken"]) == (3.0, 2.0, 2, 0.0, 3.0, 0), (what, v)
    for site in sites:  # a bad site gives NaN / 0 for every ship, and leaves the ships' own outputs alone
        if r["site_status"][sites.index(site)]:
            m = sites.index(site)
            assert np.isnan(r["min_dist"][0, m]).all() and np.isnan(r["min_time"][0, m]).all() and np.isnan(r["first_within"][0, m]).all()
            assert not r["time_within"][0, m].any() and not r["longest"][0, m].any() and not r["nwithin"][0, m].any(), (what, site)
    assert r["sound_time"][0].tolist() == [6.0, 6.0, 4.0, 4.0, 2.0, 0.0, 1.0, 0.0, 0.0, 4.0, 0.0, 3.0], what


# ---- the port fleet: S = 5, Nmax = 8, B = 130 (two waves plus two lanes), M = 37; dt and t0 are multiples of 2^-6 h -----------
FLEET_S, FLEET_N, FLEET_B, FLEET_M, FLEET_SEED = 5, 8, 130, 37, 10  # the seed: no grazing value and no near tie (the tests assert it)
FLEET_RADII = (12.0, 20.0, 30.0)
FLEET_WINDOW = (3, 70)


def fleet():
    """dict(states (5, 9, 4, 130), nsteps, dt (8, 130), t0 (130,), sites (37, 2), radius (37,)).  Ships 0 .. 15 start at lon
    179.6 .. 180.4, lat -20 +- 0.3, have full length, and the first eight are stored wrapped; ships 16 .. 129 start within 0.6
    degrees of longitude and 0.4 of latitude of (10, 50) and have nsteps = b % 9.  A drift of N(0, 0.12) degrees per step per
    ship plus N(0, 0.04) noise; dt a multiple of 2^-6 h in [0.3, 1.2], t0 one in [0, 2]: every knot of every clock is exact;
    samples 1 .. 4 are sample 0 plus N(0, 0.02) degrees; the rows past nsteps hold garbage.  A site lies N(0, 0.05) degrees from
    a row of sample 0 of some ship: the first ten among the sixteen, given east of 180, the rest among the others; radius
    12, 20 or 30 km by m % 3."""
    if "fleet" in _CACHE:
        return _CACHE["fleet"]
    rng = np.random.default_rng(FLEET_SEED)
    S, N, B, M = FLEET_S, FLEET_N, FLEET_B, FLEET_M
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
    sites = np.zeros((M, 2))
    for m in range(M):
        b = int(rng.integers(0, 16)) if m < 10 else int(rng.integers(16, B))
        while nsteps[b] < 2:
            b = int(rng.integers(16, B))
        row = int(rng.integers(0, nsteps[b] + 1))
        sites[m] = st[0, row, :2, b] + rng.normal(0.0, 0.05, 2)
        if m < 10:
            sites[m, 0] = sites[m, 0] % 360.0  # 179.x or 180.x: never wrapped
    garbage = rng.normal(0.0, 1e3, st.shape)
    for b in range(B):
        st[:, nsteps[b] + 1:, :, b] = garbage[:, nsteps[b] + 1:, :, b]
    radius = np.array([FLEET_RADII[m % 3] for m in range(M)])
    _CACHE["fleet"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, sites=sites, radius=radius)
    return _CACHE["fleet"]


def fleet_reference(model="sphere"):
    """The restatement on the port fleet, computed once per model."""
    key = ("fleet", model)
    if key not in _CACHE:
        w = fleet()
        _CACHE[key] = site_metrics(w["states"], w["nsteps"], w["dt"], w["sites"], w["radius"], w["t0"], model)
    return _CACHE[key]
