"""NumPy restatement of the encounter quantities (include/ste.h: ste_encounter_metrics_f64; DESIGN.md, "Encounters"), operation
for operation, and the small batches its tests share.

For pair (i, j) of sample s, with tau_t[k] = t0[t] + T_k, T_{k+1} = T_k + dt_k:
    walk             a = b = 0; while a < ns_i and b < ns_j: lo = max(tau_i[a], tau_j[b]), hi = min(tau_i[a+1], tau_j[b+1]); the
                     PIECE is examined when hi > lo; the ship whose step ends first advances, both on a tie
    bad clock        a non-finite t0 (before the walk) or a dt read at the top of a repetition that is not finite and >= 0:
                     STE_ENC_BAD_TIME, NaN for min_dist, min_time and first_within, 0 for the rest; a bad index likewise
    broken           a piece on a step with |wrap180(lon_{k+1} - lon_k)| < 90 false or a non-finite latitude: nbroken += 1, the
                     run is closed, nothing else
    positions        u = clamp01((t - tau[k]) / dt_k) at lo and hi, x = lon_k + u delta, y = lat_k + u (lat_{k+1} - lat_k)
    relative         gx0 = wrap180(xj0 - xi0), gx1 = gx0 + ((xj1 - xj0) - (xi1 - xi0)), gy = yj - yi, scaled by Kd cos(mean lat)
                     and Kd: r0, r1, d = r1 - r0, dd = d.d, bq = r0.d, r00 = r0.r0
    closest          u* = clamp01(-bq / dd) (0 when dd is not > 0), q = |r0 + u* d|^2, the first smallest q wins; min_dist is
                     path_metrics_cases.leg_km between the two positions at u*
    within R         the roots of |r0 + u d|^2 = R^2 clipped to [0, 1]; runs are joined across pieces when ua == 0
"""
import numpy as np
import path_metrics_cases as pmc
from track_sampling_cases import wrap180

DEG2RAD = 0.017453292519943295
KD = 6378.137 * DEG2RAD  # km per degree of a great circle: one double, as in the kernel
BAD_INDEX, BAD_TIME = 0x1, 0x2
FLOAT_OUTPUTS = ("min_dist", "min_time", "time_within", "first_within", "overlap")
INT_OUTPUTS = ("nwithin", "nbroken")
_CACHE = {}


def clamp01(x):
    return 0.0 if x < 0.0 else (1.0 if x > 1.0 else x)


def _finite(x):
    return x * 0.0 == 0.0


def _step(lon, lat, k):
    """(lon_k, lat_k, delta, dlat, sound) of step k."""
    delta = wrap180(lon[k + 1] - lon[k])
    sound = bool(abs(delta) < 90.0) and _finite(lat[k]) and _finite(lat[k + 1])
    return lon[k], lat[k], delta, lat[k + 1] - lat[k], sound


def _pair(lon_i, lat_i, dt_i, ns_i, t0i, lon_j, lat_j, dt_j, ns_j, t0j, R2, model):
    """One (sample, pair): (min_dist, min_time, time_within, first_within, nwithin, overlap, nbroken, status, best_q,
    runner_up_q, npieces)."""
    nan, inf = np.float64(np.nan), np.float64(np.inf)
    bad = (nan, nan, 0.0, nan, 0, 0.0, 0, BAD_TIME, inf, inf, 0)
    if not (_finite(t0i) and _finite(t0j)):
        return bad
    a = b = 0
    Ta = Tb = np.float64(0.0)
    best_q, runner, min_time, pos = inf, inf, nan, None
    within, first, overlap = np.float64(0.0), nan, np.float64(0.0)
    nwithin = nbroken = npieces = 0
    open_ = False
    while a < ns_i and b < ns_j:
        dta, dtb = np.float64(dt_i[a]), np.float64(dt_j[b])
        if not (dta >= 0.0 and _finite(dta) and dtb >= 0.0 and _finite(dtb)):
            return bad
        ta, Ta1 = t0i + Ta, Ta + dta
        ea = t0i + Ta1
        tb, Tb1 = t0j + Tb, Tb + dtb
        eb = t0j + Tb1
        lo = ta if ta > tb else tb
        hi = ea if ea < eb else eb
        adva, advb = ea <= eb, eb <= ea
        if hi > lo:
            npieces += 1
            lon_a, lat_a, delta_a, dlat_a, sound_a = _step(lon_i, lat_i, a)
            lon_b, lat_b, delta_b, dlat_b, sound_b = _step(lon_j, lat_j, b)
            if not (sound_a and sound_b):
                nbroken += 1
                open_ = False
            else:
                ln = hi - lo
                overlap = overlap + ln
                u0a, u1a = clamp01((lo - ta) / dta), clamp01((hi - ta) / dta)
                u0b, u1b = clamp01((lo - tb) / dtb), clamp01((hi - tb) / dtb)
                xi0, xi1 = lon_a + u0a * delta_a, lon_a + u1a * delta_a
                yi0, yi1 = lat_a + u0a * dlat_a, lat_a + u1a * dlat_a
                xj0, xj1 = lon_b + u0b * delta_b, lon_b + u1b * delta_b
                yj0, yj1 = lat_b + u0b * dlat_b, lat_b + u1b * dlat_b
                gx0, gy0 = wrap180(xj0 - xi0), yj0 - yi0
                gx1, gy1 = gx0 + ((xj1 - xj0) - (xi1 - xi0)), yj1 - yi1
                kc = KD * np.cos(0.25 * ((yi0 + yi1) + (yj0 + yj1)) * DEG2RAD)
                r0x, r0y, r1x, r1y = kc * gx0, KD * gy0, kc * gx1, KD * gy1
                dx, dy = r1x - r0x, r1y - r0y
                dd, bq, r00 = dx * dx + dy * dy, r0x * dx + r0y * dy, r0x * r0x + r0y * r0y
                us = clamp01(-bq / dd) if dd > 0.0 else 0.0
                mx, my = r0x + us * dx, r0y + us * dy
                q = mx * mx + my * my
                if q < best_q:
                    runner, best_q = best_q, q
                    min_time = lo + us * ln
                    pos = (xi0 + us * (xi1 - xi0), yi0 + us * (yi1 - yi0), xj0 + us * (xj1 - xj0), yj0 + us * (yj1 - yj0))
                elif q < runner:
                    runner = q
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
                    within = within + (ub - ua) * ln
                    if not (open_ and ua == 0.0):
                        if nwithin == 0:
                            first = lo + ua * ln
                        nwithin += 1
                    open_ = ub == 1.0
                else:
                    open_ = False
        if adva:
            a, Ta = a + 1, Ta1
        if advb:
            b, Tb = b + 1, Tb1
    min_dist = nan
    if pos is not None:
        min_dist = pmc.leg_km(model, *pos) if all(_finite(v) for v in pos) else nan
    return min_dist, min_time, within, first, nwithin, overlap, nbroken, 0, best_q, runner, npieces


def encounter_metrics(states, nsteps, dt, pairs, radius_km, t0=None, model="sphere"):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``dt`` (N, B), ``pairs`` (P, 2), ``t0`` (B,) or None ->
    dict(min_dist, min_time, time_within, first_within, overlap (S, P); nwithin, nbroken (S, P) int32; status (P,) int32; and,
    beyond the kernel's outputs, best_q and runner_up_q (S, P), the smallest and the second smallest q of the pair's sound
    pieces (inf where there is none), and npieces (P,))."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    pairs = np.asarray(pairs)
    P = pairs.shape[0]
    t0 = np.zeros(B) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), (B,))
    R2 = np.float64(radius_km) * np.float64(radius_km)
    out = {k: np.zeros((S, P)) for k in FLOAT_OUTPUTS + ("best_q", "runner_up_q")}
    out.update({k: np.zeros((S, P), dtype=np.int32) for k in INT_OUTPUTS})
    out["status"], out["npieces"] = np.zeros((P,), dtype=np.int32), np.zeros((P,), dtype=np.int32)
    nan, inf = np.nan, np.inf
    with np.errstate(all="ignore"):
        for p in range(P):
            i, j = int(pairs[p, 0]), int(pairs[p, 1])
            for s in range(S):
                if not (0 <= i < B and 0 <= j < B):
                    r = (nan, nan, 0.0, nan, 0, 0.0, 0, BAD_INDEX, inf, inf, 0)
                else:
                    r = _pair(states[s, :, 0, i], states[s, :, 1, i], dt[:, i], min(max(int(nsteps[i]), 0), rows - 1), np.float64(t0[i]),
                              states[s, :, 0, j], states[s, :, 1, j], dt[:, j], min(max(int(nsteps[j]), 0), rows - 1), np.float64(t0[j]),
                              R2, model)
                for k, v in zip(("min_dist", "min_time", "time_within", "first_within", "nwithin", "overlap", "nbroken"), r):
                    out[k][s, p] = v
                out["status"][p] = r[7]
                out["best_q"][s, p], out["runner_up_q"][s, p], out["npieces"][p] = r[8], r[9], r[10]
    return out


def near_tie(ref):
    """(S, P) bool: the runner-up piece's q is within 1e-9 relative of the best one's, so min_time may come from either."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(ref["best_q"]) & (ref["runner_up_q"] <= ref["best_q"] * (1.0 + 1e-9))


def grazing(ref, radius_km):
    """(S, P) bool: the closest approach is within 1e-9 relative of R, so a rounding decides whether the pair came within."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(ref["best_q"]) & (np.abs(np.sqrt(ref["best_q"]) - radius_km) < 1e-9 * radius_km)


def clock_span(nsteps, dt, t0, pairs):
    """(P,) hours from the earlier start to the later end of the two tracks of each pair: the scale of a time's tolerance."""
    B = dt.shape[1]
    t0 = np.zeros(B) if t0 is None else np.asarray(t0, dtype=np.float64)
    end = t0 + np.array([dt[: int(nsteps[b]), b].sum() for b in range(B)])
    i, j = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
    return np.maximum(end[i], end[j]) - np.minimum(t0[i], t0[j])


# ---- hand-made tracks: one batch of 16 ships, Nmax = 6, R = 30 km ---------------------------------------------------------
HAND_R = 30.0
HAND_B, HAND_N = 16, 6
HAND_PAIRS = {
    "meeting": (0, 1),            # towards each other on the equator, meeting mid-step at 2.5 h
    "parallel": (2, 3),           # 0.1 degrees of latitude apart, own dt grids and t0
    "zigzag": (4, 5),             # past a stationary ship, pausing next to it and away from it: two runs, dd == 0
    "antimeridian": (6, 7),       # 0.2 degrees apart astride 180, ship 7 stored wrapped
    "disjoint clocks": (5, 8),    # ship 8 starts at 100 h
    "broken": (9, 10),            # a NaN latitude in row 2 of ship 9: two broken pieces split the run
    "same ship": (3, 3),
    "no steps": (10, 11),         # nsteps 0
    "no steps, bad dt": (11, 13),  # nothing is read of a walk that has no repetition
    "one step": (10, 12),         # nsteps 1: a copy of ship 10's first step
    "one step, dt past it": (12, 13),  # the NaN dt of ship 13's step 1 is never met
    "nan dt": (10, 13),
    "negative dt": (14, 10),
    "nan t0": (10, 15),
    "index past B": (0, 16),
    "negative index": (-1, 0),
}


def hand_batch():
    """dict(states (1, 7, 4, 16), nsteps, dt (6, 16), t0 (16,), pairs (16, 2) int32, names)."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    B, N = HAND_B, HAND_N
    k = np.arange(N + 1.0)
    lon, lat = np.zeros((N + 1, B)), np.zeros((N + 1, B))
    dt = np.ones((N, B))
    nsteps = np.full(B, 4, dtype=np.int32)
    t0 = np.zeros(B)
    lon[:, 0], lon[:, 1] = k, 5.0 - k
    dt[:, 2], dt[:, 3] = 0.5, [0.7, 0.3, 1.1, 0.4, 0.6, 0.2]
    t0[3] = 0.25
    nsteps[[2, 3, 4, 5, 8]] = 6
    lon[:, 2] = 10.0 + np.concatenate([[0.0], np.cumsum(dt[:, 2])])  # one degree an hour, both
    lon[:, 3] = 10.0 + (t0[3] + np.concatenate([[0.0], np.cumsum(dt[:, 3])]))
    lat[:, 3] = 0.1
    lon[:, 4], lat[:, 4] = 20.0 + np.array([-1.0, 0.0, 0.0, 1.0, 1.0, 0.0, -1.0]), 0.1
    lon[:, 5] = lon[:, 8] = 20.0
    t0[8] = 100.0
    lon[:, 6] = 179.6 + 0.2 * k
    lon[:, 7] = wrap180(179.8 + 0.2 * k)
    for b in (9, 10, 11, 12, 13, 14, 15):
        lon[:, b] = 30.0 + 0.1 * k
    lat[:, [10, 12]] = 0.1
    lat[2, 9] = np.nan
    nsteps[11], nsteps[12] = 0, 1
    dt[1, 13], dt[0, 14], t0[15] = np.nan, -1.0, np.nan
    st = np.zeros((1, N + 1, 4, B))
    st[0, :, 0], st[0, :, 1] = lon, lat
    _CACHE["hand"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, pairs=np.array(list(HAND_PAIRS.values()), dtype=np.int32),
                          names=list(HAND_PAIRS))
    return _CACHE["hand"]


def check_hand_answers(r, what):
    """The known answers of the hand-made pairs, for the restatement and for the device alike."""
    names = list(HAND_PAIRS)
    km = pmc.KM_PER_DEG_EQUATOR
    v = {n: {k: r[k][0, names.index(n)] for k in FLOAT_OUTPUTS + INT_OUTPUTS} for n in names}
    status = dict(zip(names, r["status"].tolist()))

    def close(got, want, tol, name):
        assert abs(got - want) <= tol, (what, name, got, want)

    m = v["meeting"]  # x = t against x = 5 - t: they meet at 2.5 h; the gap closes at 2 degrees an hour
    assert m["min_dist"] <= 1e-9 and m["nwithin"] == 1 and m["nbroken"] == 0 and m["overlap"] == 4.0, (what, m)
    close(m["min_time"], 2.5, 1e-12, "meeting")
    close(m["time_within"], HAND_R / km, 1e-12, "meeting")
    close(m["first_within"], 2.5 - 0.5 * HAND_R / km, 1e-12, "meeting")
    for name, gap in (("parallel", 0.1), ("antimeridian", 0.2)):  # a constant distance below R
        m = v[name]
        close(m["min_dist"], gap * km, 1e-9 * gap * km, name)
        assert m["time_within"] == m["overlap"] and m["nwithin"] == 1 and m["nbroken"] == 0, (what, name, m)
    close(v["parallel"]["overlap"], 2.75, 1e-12, "parallel")
    close(v["parallel"]["first_within"], 0.25, 0.0, "parallel")
    assert 0.25 <= v["parallel"]["min_time"] <= 3.0  # every piece has the same q but for roundings: any of them may win
    assert v["antimeridian"]["overlap"] == 4.0 and v["antimeridian"]["first_within"] == 0.0
    m = v["zigzag"]  # half a chord of the circle of R about the stationary ship at 0.1 degrees of latitude, in hours
    half = np.sqrt(HAND_R ** 2 - (0.1 * km) ** 2) / (km * np.cos(np.radians(0.05)))
    assert m["nwithin"] == 2 and m["nbroken"] == 0 and m["overlap"] == 6.0, (what, m)
    close(m["time_within"], 1.0 + 4.0 * half, 1e-12, "zigzag")
    close(m["first_within"], 1.0 - half, 1e-12, "zigzag")
    close(m["min_dist"], 0.1 * km, 1e-10, "zigzag")
    assert m["min_time"] == 1.0
    for name in ("disjoint clocks", "no steps", "no steps, bad dt"):
        m = v[name]
        assert status[name] == 0 and np.isnan([m["min_dist"], m["min_time"], m["first_within"]]).all(), (what, name, m)
        assert m["time_within"] == 0.0 and m["overlap"] == 0.0 and m["nwithin"] == 0 and m["nbroken"] == 0, (what, name, m)
    m = v["broken"]  # pieces 1 and 2 touch the NaN row: the run within R is cut in two
    assert (m["nbroken"], m["nwithin"], m["overlap"], m["time_within"], m["first_within"]) == (2, 2, 2.0, 2.0, 0.0), (what, m)
    close(m["min_dist"], 0.1 * km, 1e-10, "broken")
    m = v["same ship"]
    assert m["min_dist"] == 0.0 and m["time_within"] == m["overlap"] and m["nwithin"] == 1, (what, m)
    close(m["overlap"], 3.3, 1e-12, "same ship")
    close(m["min_time"], 0.25, 0.0, "same ship")
    for name in ("one step", "one step, dt past it"):
        m = v[name]
        assert status[name] == 0 and (m["overlap"], m["time_within"], m["nwithin"], m["nbroken"]) == (1.0, 1.0, 1, 0), (what, name, m)
        assert m["min_time"] == 0.0 and m["first_within"] == 0.0, (what, name, m)
    assert v["one step"]["min_dist"] == 0.0  # ship 12 is ship 10's first step; ship 13 sails 0.1 degrees south of it
    close(v["one step, dt past it"]["min_dist"], 0.1 * km, 1e-10, "one step, dt past it")
    for name, bit in (("nan dt", BAD_TIME), ("negative dt", BAD_TIME), ("nan t0", BAD_TIME), ("index past B", BAD_INDEX),
                      ("negative index", BAD_INDEX)):
        m = v[name]
        assert status[name] == bit and np.isnan([m["min_dist"], m["min_time"], m["first_within"]]).all(), (what, name, m)
        assert m["time_within"] == 0.0 and m["overlap"] == 0.0 and m["nwithin"] == 0 and m["nbroken"] == 0, (what, name, m)
    assert sum(status.values()) == 3 * BAD_TIME + 2 * BAD_INDEX


# ---- the meeting fleet: S = 5, Nmax = 8, B = 70, P = 130 (two waves plus two lanes), R = 30 km ------------------------------
FLEET_S, FLEET_N, FLEET_B, FLEET_P, FLEET_SEED, PAIR_SEED = 5, 8, 70, 130, 11, 5
FLEET_R = 30.0
FLEET_WINDOW = (3, 70)


def fleet():
    """dict(states (5, 9, 4, 70), nsteps, dt (8, 70), t0 (70,), pairs (130, 2) int32).  Ships 0 .. 7 start at lon 179.7 ..
    180.3, lat -20 +- 0.3, have full length, and the first four are stored wrapped; ships 8 .. 69 start within 0.6 degrees of
    longitude and 0.4 of latitude of (10, 50) and have nsteps = b % 9.  A drift of N(0, 0.12) degrees per step per ship plus
    N(0, 0.04) noise; dt U(0.3, 1.2), t0 U(0, 2); samples 1 .. 4 are sample 0 plus N(0, 0.02) degrees.  The pairs are drawn
    within the two groups; the last ten are four reversed copies of earlier pairs, one (i, i) and five pairs of the eight."""
    if "fleet" in _CACHE:
        return _CACHE["fleet"]
    rng = np.random.default_rng(FLEET_SEED)
    S, N, B = FLEET_S, FLEET_N, FLEET_B
    start = np.stack([10.0 + rng.uniform(-0.6, 0.6, B), 50.0 + rng.uniform(-0.4, 0.4, B)])
    start[0, :8], start[1, :8] = np.linspace(179.7, 180.3, 8), -20.0 + rng.uniform(-0.3, 0.3, 8)
    drift = rng.normal(0.0, 0.12, (2, B))
    steps = drift[None] + rng.normal(0.0, 0.04, (N, 2, B))
    st = np.zeros((S, N + 1, 4, B))
    st[0, 0, :2] = start
    st[0, 1:, :2] = start[None] + np.cumsum(steps, axis=0)
    st[1:, :, :2] = st[0, :, :2][None] + rng.normal(0.0, 0.02, (S - 1, N + 1, 2, B))
    st[:, :, 0, :4] = wrap180(st[:, :, 0, :4])
    st[:, :, 2:] = rng.normal(0.0, 1.0, (S, N + 1, 2, B))  # speed and heading: not read
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    nsteps[:8] = N
    dt = rng.uniform(0.3, 1.2, (N, B))
    t0 = rng.uniform(0.0, 2.0, B)
    prng = np.random.default_rng(PAIR_SEED)
    pairs = []
    while len(pairs) < FLEET_P - 10:
        i, j = (int(v) for v in prng.integers(8, B, 2))
        if i != j:
            pairs.append((i, j))
    pairs += [(pairs[k][1], pairs[k][0]) for k in (0, 7, 31, 64)] + [(21, 21)] + [(0, 5), (1, 2), (3, 4), (6, 2), (7, 0)]
    _CACHE["fleet"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, pairs=np.array(pairs, dtype=np.int32))
    return _CACHE["fleet"]


REVERSED = ((FLEET_P - 10, 0), (FLEET_P - 9, 7), (FLEET_P - 8, 31), (FLEET_P - 7, 64))  # (reversed copy, original)


def fleet_reference(model="sphere"):
    """The restatement on the meeting fleet, computed once per model."""
    key = ("fleet", model)
    if key not in _CACHE:
        w = fleet()
        _CACHE[key] = encounter_metrics(w["states"], w["nsteps"], w["dt"], w["pairs"], FLEET_R, w["t0"], model)
    return _CACHE[key]
