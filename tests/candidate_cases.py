"""NumPy restatement of the candidate rule (include/ste.h: CANDIDATES; DESIGN.md, "Candidates"), written from the rule and not
from the kernels' order of work, and the small batches its tests share.

    clock       tau_t[k] = t0[t] + T_k, T_{k+1} = T_k + dt_k in order; a non-finite t0: BAD_TIME, the track pairs with nothing; a
                dt among the first nsteps that is not finite and >= 0: BAD_TIME, the track ends at that knot
    windows     win(x) = clamp(floor((x - time0) / W), 0, NW - 1); CLIPPED when clamping changed the index of a knot
    sound step  |wrap180(lon_{k+1} - lon_k)| < 90 and both latitudes finite; no sound step: EMPTY
    boxes       per (track, window w), over the sound steps with win(tau[k]) <= w <= win(tau[k+1]): min and max of the unit
                vectors of rows k, k + 1, and h = max of 0.5 * kDeg2Rad * sqrt(delta^2 + dlat^2); else lo = +inf, hi = -inf, h = 0
    near        both boxes non-empty and g2 <= c^2, g_c = max(max(0, lo_i - hi_j), lo_j - hi_i), g2 = (g_0^2 + g_1^2) + g_2^2,
                theta = min(((((reach / 6378.137 + m_i) + m_j) + h_i) + h_j) + 1e-7, pi), c = 2 sin(theta / 2)
"""
import encounter_cases as enc
import numpy as np
from track_sampling_cases import wrap180

DEG2RAD = enc.DEG2RAD
EARTH_KM = 6378.137
SLACK = 1e-7
BAD_TIME, CLIPPED, EMPTY, BAD_MARGIN = 0x1, 0x2, 0x4, 0x8
CORNER_ATOL = 1.4e-15  # a box corner: a product of two sines / cosines, the device held to 1.5 ulp each and libm to 1
GRAZE_RTOL = 1e-9      # |g2 - c^2| <= 1e-9 c^2: a rounding of a corner decides the test
_CACHE = {}


def _finite(x):
    return x * 0.0 == 0.0


def window_of(x, time0, W, NW):
    """(win(x), clamping changed it)."""
    with np.errstate(all="ignore"):
        f = np.floor((np.float64(x) - np.float64(time0)) / np.float64(W))
    top = np.float64(NW - 1)
    c = 0.0 if f < 0.0 else (top if f > top else f)
    return int(c), bool(c != f)


def boxes(states, nsteps, dt, t0, time0, W, NW, margin=None):
    """``states`` (N+1, 4, B) -> dict(box (NW, 7, B): lo[3], hi[3], h; wlo, whi (B,) int32, wlo > whi for a track that pairs
    with nothing; status (B,) int32)."""
    states = np.asarray(states, dtype=np.float64)
    rows, _, B = states.shape
    t0 = np.zeros(B) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), (B,))
    box = np.zeros((NW, 7, B))
    box[:, 0:3], box[:, 3:6] = np.inf, -np.inf
    wlo, whi = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    with np.errstate(all="ignore"):
        lon, lat = states[:, 0], states[:, 1]
        lonr, latr = lon * DEG2RAD, lat * DEG2RAD
        unit = np.stack([np.cos(latr) * np.cos(lonr), np.cos(latr) * np.sin(lonr), np.sin(latr)])  # (3, rows, B)
        for t in range(B):
            ns = min(max(int(nsteps[t]), 0), rows - 1)
            if margin is not None and not (margin[t] >= 0.0 and _finite(margin[t])):
                status[t] |= BAD_MARGIN
            if not _finite(t0[t]):
                status[t] |= BAD_TIME
                continue
            badk = [k for k in range(ns) if not (dt[k, t] >= 0.0 and _finite(dt[k, t]))]
            if badk:  # the track ends at its first bad dt
                status[t] |= BAD_TIME
                ns = badk[0]
            T, wins, clipped = np.float64(0.0), [], False
            for k in range(ns + 1):
                w, c = window_of(t0[t] + T, time0, W, NW)
                wins.append(w)
                clipped = clipped or c
                if k < ns:
                    T = T + np.float64(dt[k, t])
            if clipped:
                status[t] |= CLIPPED
            any_sound = False
            for k in range(ns):
                delta, dlat = wrap180(lon[k + 1, t] - lon[k, t]), lat[k + 1, t] - lat[k, t]
                if not (abs(delta) < 90.0 and _finite(lat[k, t]) and _finite(lat[k + 1, t])):
                    continue
                any_sound = True
                h = 0.5 * DEG2RAD * np.sqrt(delta * delta + dlat * dlat)
                lo, hi = np.minimum(unit[:, k, t], unit[:, k + 1, t]), np.maximum(unit[:, k, t], unit[:, k + 1, t])
                for w in range(wins[k], wins[k + 1] + 1):
                    box[w, 0:3, t] = np.minimum(box[w, 0:3, t], lo)
                    box[w, 3:6, t] = np.maximum(box[w, 3:6, t], hi)
                    box[w, 6, t] = max(box[w, 6, t], h)
            if not any_sound:
                status[t] |= EMPTY
            elif not status[t] & BAD_MARGIN:
                wlo[t], whi[t] = wins[0], wins[-1]
    dead = wlo > whi
    box[:, 0:3, dead], box[:, 3:6, dead], box[:, 6, dead] = np.inf, -np.inf, 0.0  # such a track's boxes are never read
    return dict(box=box, wlo=wlo, whi=whi, status=status)


def candidates(states, nsteps, dt, reach_km, W, time0, NW, t0=None, margin=None):
    """The restated list: dict(pairs (P, 2) int32 sorted by (i, j); wfirst, nwin (P,) int32; status, wlo, whi (B,); box;
    ngrazing: the pair-windows (i < j, both boxes non-empty) with |g2 - c^2| <= 1e-9 c^2; ntests: those examined)."""
    bx = boxes(states, nsteps, dt, t0, time0, W, NW, margin)
    box = bx["box"]
    B = box.shape[2]
    m = np.zeros(B) if margin is None else np.where(bx["wlo"] <= bx["whi"], np.asarray(margin, dtype=np.float64), 0.0) / EARTH_KM
    nwin = np.zeros((B, B), dtype=np.int32)
    wfirst = np.full((B, B), -1, dtype=np.int32)
    upper = np.arange(B)[:, None] < np.arange(B)[None, :]
    ngrazing = ntests = 0
    with np.errstate(all="ignore"):
        rmm = (np.float64(reach_km) / EARTH_KM + m[:, None]) + m[None, :]
        for w in range(NW):
            lo, hi, h = box[w, 0:3], box[w, 3:6], box[w, 6]
            full = lo[0] <= hi[0]
            both = full[:, None] & full[None, :] & upper
            if not both.any():
                continue
            g = [np.maximum(np.maximum(0.0, lo[c][:, None] - hi[c][None, :]), lo[c][None, :] - hi[c][:, None]) for c in range(3)]
            g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
            theta = np.minimum(((rmm + h[:, None]) + h[None, :]) + SLACK, np.pi)
            c = 2.0 * np.sin(theta / 2.0)
            cc = c * c
            near = both & (g2 <= cc)
            ngrazing += int((both & (np.abs(g2 - cc) <= GRAZE_RTOL * cc)).sum())
            ntests += int(both.sum())
            wfirst[near & (nwin == 0)] = w
            nwin += near
    i, j = np.nonzero(nwin > 0)  # row-major: sorted by (i, j)
    return dict(pairs=np.stack([i, j], axis=1).astype(np.int32), wfirst=wfirst[i, j], nwin=nwin[i, j], status=bx["status"],
                wlo=bx["wlo"], whi=bx["whi"], box=box, ngrazing=ngrazing, ntests=ntests)


def clock_windows(nsteps, dt, t0, W):
    """(time0, NW) that cover the sound clocks: the earliest start and the window of the latest end."""
    B = dt.shape[1]
    t0 = np.zeros(B) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), (B,))
    with np.errstate(all="ignore"):
        d = [dt[: int(nsteps[b]), b] for b in range(B)]
        end = t0 + np.array([x.sum() for x in d])
        ok = np.isfinite(t0) & np.isfinite(end) & np.array([bool((np.isfinite(x) & (x >= 0.0)).all()) for x in d])
    if not ok.any():
        return 0.0, 1
    time0 = float(t0[ok].min())
    return time0, int(max(np.floor((end[ok].max() - time0) / W), 0.0)) + 1


def pair_keys(pairs, B):
    p = np.asarray(pairs).astype(np.int64)
    return p[:, 0] * B + p[:, 1]


# ---- hand-made ships: B = 17, Nmax = 24, dt = 2 h, reach 30.3 km, windows of 6 h from 0 ---------------------------------------
HAND_B, HAND_N, HAND_REACH, HAND_W, HAND_NW = 17, 24, 30.3, 6.0, 18
# what the rule gives at W = 6 h, time0 = 0, NW = 18 without margins, by hand (hand_batch's docstring)
HAND_GROUP = (6, 7, 11, 12, 13, 14, 16)
HAND_PAIRS = sorted([(0, 8), (2, 3), (4, 5), (6, 9)] + [(a, b) for a in HAND_GROUP for b in HAND_GROUP if a < b])
HAND_STATUS = {8: CLIPPED, 9: CLIPPED, 10: EMPTY, 13: BAD_TIME, 15: BAD_TIME}


def hand_batch():
    """dict(states (1, 25, 4, 17), nsteps, dt (24, 17), t0, margin).  Every ship has 24 steps of 2 h unless said otherwise.
      0, 1    one lane along the equator at 0.1 degrees an hour, ship 1 a day behind: 267 km apart at any instant, clocks
              [0, 48] and [24, 72] overlap and the tracks coincide, so the cap list has the pair; windows of 6 h do not
      2, 3    11 km apart astride the antimeridian, ship 2 stored unwrapped (past 180), ship 3 wrapped
      4, 5    22 to 11 km apart across the north pole, on the meridians 0 and 180
      6       at anchor at (40, 20) with one step of 60 h = 10 W: clock [0, 106], windows 0 .. 17
      7       at anchor 11 km north of it from 30 h to 78 h = 13 W exactly: windows 5 .. 13, the last one by its boundary alone
      8       near the start of ship 0 a hundred hours before time0: CLIPPED into window 0, where it pairs with ship 0
      9       beside ship 6, five hundred hours on: CLIPPED into window 17, where only ship 6 still is
      10      nsteps 0: EMPTY;  11: nsteps 1, from 30 h
      12      from 30 h with a NaN latitude in row 10: steps 9 and 10 are broken, window 8 keeps the steps around them
      13      from 30 h with a NaN dt at step 7: BAD_TIME, and the seven steps before it (30 .. 44 h, windows 5 .. 7) still pair
      14      nsteps 5 and the NaN dt past them;  15: a NaN t0: BAD_TIME, pairs with nothing
      16      from 30 h; its margin is negative in ``margin`` (zeros elsewhere): BAD_MARGIN when the margins are given
    Ships 6, 7, 9 .. 16 lie within 22 km of each other."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    B, N = HAND_B, HAND_N
    k = np.arange(N + 1.0)
    lon, lat = np.zeros((N + 1, B)), np.zeros((N + 1, B))
    dt = np.full((N, B), 2.0)
    nsteps = np.full(B, N, dtype=np.int32)
    t0 = np.zeros(B)
    lon[:, 0] = lon[:, 1] = 0.2 * k
    t0[1] = 24.0
    lon[:, 2], lat[:, 2] = 179.0 + 0.05 * k, 10.0
    lon[:, 3], lat[:, 3] = wrap180(179.1 + 0.05 * k), 10.0
    lon[:, 5] = 180.0
    lat[:, 4] = lat[:, 5] = 89.9 + 0.05 * k / N
    lon[:, 6:], lat[:, 6:] = 40.0, 20.0 + 0.01 * (np.arange(6, B) - 6.0)[None, :]
    lat[:, 7] = 20.1
    dt[3, 6] = 60.0
    t0[[7, 11, 12, 13, 14, 15, 16]] = 30.0
    lon[:, 8], lat[:, 8], t0[8] = 0.1, 0.05, -100.0
    t0[9] = 500.0
    nsteps[10], nsteps[11], nsteps[14] = 0, 1, 5
    lat[10, 12] = np.nan
    dt[7, 13], dt[10, 14], t0[15] = np.nan, np.nan, np.nan
    margin = np.zeros(B)
    margin[16] = -1.0
    st = np.zeros((1, N + 1, 4, B))
    st[0, :, 0], st[0, :, 1] = lon, lat
    _CACHE["hand"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, margin=margin)
    return _CACHE["hand"]


def check_hand_answers(r, what):
    """The answers known by hand at W = 6 h, time0 = 0, NW = 18, reach 30.3 km, no margins; ``r``: dict(pairs, wfirst, nwin,
    status) of the restatement or of the device."""
    pairs = [tuple(int(v) for v in p) for p in np.asarray(r["pairs"])]
    assert pairs == HAND_PAIRS, (what, sorted(set(pairs) ^ set(HAND_PAIRS)))
    assert (0, 1) not in pairs and all(i < j for i, j in pairs)
    status = np.asarray(r["status"]).tolist()
    assert status == [HAND_STATUS.get(t, 0) for t in range(HAND_B)], (what, status)
    first = dict(zip(pairs, np.asarray(r["wfirst"]).tolist()))
    n = dict(zip(pairs, np.asarray(r["nwin"]).tolist()))
    assert (first[(6, 7)], n[(6, 7)]) == (5, 9), (what, "the step of 10 W, and 78 h = 13 W on the boundary")
    assert (first[(7, 12)], n[(7, 12)]) == (5, 9), (what, "window 8 survives the two broken steps")
    assert (first[(0, 8)], n[(0, 8)]) == (0, 1) and (first[(6, 9)], n[(6, 9)]) == (17, 1), (what, "edge windows")
    assert (first[(6, 11)], n[(6, 11)]) == (5, 1) and (first[(7, 14)], n[(7, 14)]) == (5, 2), (what, "nsteps 1 and 5")
    assert (first[(7, 13)], n[(7, 13)]) == (5, 3), (what, "the steps before the NaN dt")
    assert n[(2, 3)] == 9 and n[(4, 5)] == 9 and first[(2, 3)] == first[(4, 5)] == 0, (what, "antimeridian and pole: [0, 48] h")


# ---- the meeting fleet of encounter_cases, widened to any B ---------------------------------------------------------------------
def wide_fleet(B, seed=enc.FLEET_SEED):
    """encounter_cases.fleet()'s generator for B ships (sample 0 alone): dict(states (1, 9, 4, B), nsteps, dt (8, B), t0)."""
    key = ("wide", B, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    N = enc.FLEET_N
    start = np.stack([10.0 + rng.uniform(-0.6, 0.6, B), 50.0 + rng.uniform(-0.4, 0.4, B)])
    n8 = min(8, B)
    start[0, :n8], start[1, :n8] = np.linspace(179.7, 180.3, 8)[:n8], -20.0 + rng.uniform(-0.3, 0.3, 8)[:n8]
    drift = rng.normal(0.0, 0.12, (2, B))
    steps = drift[None] + rng.normal(0.0, 0.04, (N, 2, B))
    st = np.zeros((1, N + 1, 4, B))
    st[0, 0, :2] = start
    st[0, 1:, :2] = start[None] + np.cumsum(steps, axis=0)
    st[0, :, 0, : min(4, B)] = wrap180(st[0, :, 0, : min(4, B)])
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    nsteps[:n8] = N
    _CACHE[key] = dict(states=st, nsteps=nsteps, dt=rng.uniform(0.3, 1.2, (N, B)), t0=rng.uniform(0.0, 2.0, B))
    return _CACHE[key]


def dense_batch():
    """66 ships, 3 steps of 1 h: ships 0 .. 64 within 2 km of (10, 50) -- every pair of them is near, so rows 0 .. 63 are
    full -- and ship 65 on the other side of the Earth: rows 64 and 65 have no pair.  P = 65 * 64 / 2 = 2080."""
    B, N = 66, 3
    rng = np.random.default_rng(2)
    st = np.zeros((1, N + 1, 4, B))
    st[0, :, 0], st[0, :, 1] = 10.0 + rng.uniform(-0.01, 0.01, (N + 1, B)), 50.0 + rng.uniform(-0.01, 0.01, (N + 1, B))
    st[0, :, 0, 65], st[0, :, 1, 65] = -170.0, -50.0
    return dict(states=st, nsteps=np.full(B, N, dtype=np.int32), dt=np.ones((N, B)), t0=np.zeros(B))


# ---- the voyage fleet: ships that cross oceans ------------------------------------------------------------------------------------
def voyage_fleet(B, N, seed=1):
    """dict(states (1, N+1, 4, B), nsteps, dt (N, B), t0): departures over ten days from anywhere between 50 S and 50 N, 15
    to 30 km/h on a fixed heading with a random walk in longitude, steps of 0.5 to 1.5 h."""
    rng = np.random.default_rng(seed)
    dt = rng.uniform(0.5, 1.5, (N, B))
    t0 = rng.uniform(0.0, 240.0, B)
    lon0 = rng.uniform(-180.0, 180.0, B)
    lat0 = rng.uniform(-50.0, 50.0, B)
    hd = rng.uniform(0.0, 2.0 * np.pi, B)
    v = rng.uniform(15.0, 30.0, B) / 111.0
    T = np.concatenate([np.zeros((1, B)), np.cumsum(dt, axis=0)])
    lon = wrap180(lon0 + np.cos(hd) * v * T + 0.02 * rng.standard_normal((N + 1, B)).cumsum(0))
    lat = np.clip(lat0 + 0.4 * np.sin(hd) * v * T, -80.0, 80.0)
    st = np.zeros((1, N + 1, 4, B))
    st[0, :, 0], st[0, :, 1] = lon, lat
    return dict(states=st, nsteps=np.full(B, N, dtype=np.int32), dt=dt, t0=t0)
