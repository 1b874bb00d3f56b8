"""NumPy restatement of the positions of tracks at query times (include/ste.h: ste_track_positions_f64; DESIGN.md, "Positions"),
operation for operation, and the small batches its tests share.

For query q on track t, tq = qtime[q], tau_k = t0[t] + T_k, T_0 = 0, T_{k+1} = T_k + dt_k summed in order, ns = nsteps[t]:
    bad index        qtrack outside [0, B): BAD_INDEX, nothing of the track is read
    bad time         a dt_k, k < ns, that is not finite and >= 0, a non-finite t0 or a non-finite tq: BAD_TIME
    locate           tq == tau_0 -> row 0 (also for ns == 0); else ns == 0, tq >= tau_0 false or tq <= tau_ns false -> OUTSIDE;
                     else k = the smallest index in [0, ns) with tq <= tau_{k+1} (a plain scan here, a bisection on the device);
                     tq == tau_{k+1} -> row k + 1; else interior with u = clamp01((tq - tau_k) / (T_{k+1} - T_k))
    knot hit         wrap180(lon_j), lat_j, speed_j, heading_j % 360
    interior         delta = wrap180(lon_{k+1} - lon_k); broken (|delta| < 90 false, or a non-finite latitude) -> four NaN; else
                     wrap180(lon_k + u delta), lat_k + u (lat_{k+1} - lat_k), s_k + u (s_{k+1} - s_k),
                     (h_k + u wrap180(h_{k+1} - h_k)) % 360
    moments          for s in order: dx = wrap180(lon - anchor lon), dy = lat - anchor lat; both finite -> count += 1 and the
                     sums of dx, dy, dx dx, dx dy, dy dy take one addition each, starting from the stored values
Nothing here has bits that may differ between implementations, so the device is held to this bit for bit.
"""
import numpy as np
from track_sampling_cases import wrap180

BAD_INDEX, BAD_TIME, OUTSIDE = 0x1, 0x2, 0x4
PER_SAMPLE = ("lon", "lat", "speed", "heading")
PER_QUERY = ("step", "frac", "status")
_CACHE = {}


def clamp01(x):
    return 0.0 if x < 0.0 else (1.0 if x > 1.0 else x)


def _finite(x):
    return x * 0.0 == 0.0


def knot_times(nsteps, dt):
    """-> (T (Nmax+1, B): the in-order sums, row 0 = NaN for a track with a bad dt, NaN past nsteps (the device leaves those
    rows alone), bad (B,))."""
    dt = np.asarray(dt, dtype=np.float64)
    N, B = dt.shape
    T = np.full((N + 1, B), np.nan)
    for t in range(B):
        ns = int(nsteps[t])
        acc, bad = np.float64(0.0), False
        for k in range(ns):
            d = dt[k, t]
            bad = bad or not (d >= 0.0 and _finite(d))
            acc = acc + d
            T[k + 1, t] = acc
        T[0, t] = np.nan if bad else 0.0
    return T


def locate(tq, t0, T, ns, method="scan"):
    """One query on one track's knots T[0 .. ns] (T[0] NaN = bad dt) -> (status, row, u, interior)."""
    nan = np.float64(np.nan)
    if not (_finite(t0) and T[0] == T[0] and _finite(tq)):
        return BAD_TIME, -1, nan, False
    tau0 = t0 + T[0]
    if tq == tau0:
        return 0, 0, np.float64(0.0), False
    if ns == 0 or not (tq >= tau0) or not (tq <= t0 + T[ns]):
        return OUTSIDE, -1, nan, False
    if method == "scan":
        k = 0
        while not (tq <= t0 + T[k + 1]):
            k += 1
    else:  # the bisection of the kernel: the smallest j in [1, ns] with tq <= tau_j
        lo, hi = 1, ns
        while lo < hi:
            mid = (lo + hi) >> 1
            if tq <= t0 + T[mid]:
                hi = mid
            else:
                lo = mid + 1
        k = lo - 1
    if tq == t0 + T[k + 1]:
        return 0, k + 1, np.float64(0.0), False
    return 0, k, np.float64(clamp01((tq - (t0 + T[k])) / (T[k + 1] - T[k]))), True


def positions(states, nsteps, dt, qtrack, qtime, t0=None, anchor=None, count=None, moments=None, method="scan"):
    """The restatement: states (S, N+1, 4, B) -> dict(lon, lat, speed, heading (S, Q); step, frac, status (Q,); knots
    (N+1, B); interior, located (Q,) bool; with ``anchor`` (2, Q) also count (Q,) int32 and moments (5, Q), continued from
    ``count`` / ``moments`` when given)."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    qtrack, qtime = np.asarray(qtrack), np.asarray(qtime, dtype=np.float64)
    Q = len(qtrack)
    T = knot_times(nsteps, dt)
    out = {k: np.full((S, Q), np.nan) for k in PER_SAMPLE}
    out.update(step=np.full(Q, -1, dtype=np.int32), frac=np.full(Q, np.nan), status=np.zeros(Q, dtype=np.int32), knots=T,
               interior=np.zeros(Q, dtype=bool), located=np.zeros(Q, dtype=bool))
    if anchor is not None:
        anchor = np.asarray(anchor, dtype=np.float64)
        out["count"] = np.zeros(Q, dtype=np.int32) if count is None else np.array(count, dtype=np.int32)
        out["moments"] = np.zeros((5, Q)) if moments is None else np.array(moments, dtype=np.float64)
    with np.errstate(all="ignore"):
        for q in range(Q):
            t = int(qtrack[q])
            if t < 0 or t >= B:
                out["status"][q] = BAD_INDEX
                continue
            ns = int(nsteps[t])
            t0v = np.float64(0.0) if t0 is None else np.float64(t0[t])
            status, row, u, interior = locate(qtime[q], t0v, T[:, t], ns, method)
            out["status"][q], out["step"][q], out["frac"][q] = status, row, u
            out["interior"][q], out["located"][q] = interior, row >= 0
            if row < 0:
                continue
            a = states[:, row, :, t]  # (S, 4)
            if not interior:
                lon, lat, speed, heading = wrap180(a[:, 0]), a[:, 1].copy(), a[:, 2].copy(), a[:, 3] % 360.0
            else:
                b = states[:, row + 1, :, t]
                delta = wrap180(b[:, 0] - a[:, 0])
                sound = (np.abs(delta) < 90.0) & _finite(a[:, 1]) & _finite(b[:, 1])
                lon = np.where(sound, wrap180(a[:, 0] + u * delta), np.nan)
                lat = np.where(sound, a[:, 1] + u * (b[:, 1] - a[:, 1]), np.nan)
                speed = np.where(sound, a[:, 2] + u * (b[:, 2] - a[:, 2]), np.nan)
                heading = np.where(sound, (a[:, 3] + u * wrap180(b[:, 3] - a[:, 3])) % 360.0, np.nan)
            out["lon"][:, q], out["lat"][:, q], out["speed"][:, q], out["heading"][:, q] = lon, lat, speed, heading
            if anchor is not None:
                cnt, m = int(out["count"][q]), [np.float64(v) for v in out["moments"][:, q]]
                for s in range(S):
                    dx, dy = wrap180(lon[s] - anchor[0, q]), lat[s] - anchor[1, q]
                    if _finite(dx) and _finite(dy):
                        cnt += 1
                        m = [m[0] + dx, m[1] + dy, m[2] + dx * dx, m[3] + dx * dy, m[4] + dy * dy]
                out["count"][q], out["moments"][:, q] = cnt, m
    return out


# ---- hand-made tracks: Nmax = 4, S = 2 (sample 1 = sample 0 moved 0.25 degrees north) -----------------------------------------
HAND_N, HAND_S = 4, 2
HAND_TRACKS = ("equator", "antimeridian", "pauses", "empty", "nan dt", "negative dt", "nan t0", "nan latitude")
HAND_B = len(HAND_TRACKS)


def hand_batch():
    """dict(states (2, 5, 4, 8), nsteps, dt (4, 8), t0 (8,), qtrack, qtime, names): the queries are named, and
    ``check_hand_answers`` knows what each must give."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    N, B = HAND_N, HAND_B
    st = np.zeros((1, N + 1, 4, B))
    nsteps = np.array([4, 2, 4, 0, 4, 4, 4, 4], dtype=np.int32)
    dt = np.ones((N, B))
    t0 = np.array([10.0, -3.0, 0.0, 5.0, 0.0, 0.0, np.nan, 100.0])
    # equator: a degree an hour eastwards, speed 10 .. 18, heading 350 -> 10 -> 30 -> 20 -> 730 (= 10)
    st[0, :, 0, 0] = np.arange(5.0)
    st[0, :, 2, 0] = 10.0 + 2.0 * np.arange(5)
    st[0, :, 3, 0] = [350.0, 10.0, 30.0, 20.0, 730.0]
    # antimeridian: 179.5 -> -179.5 (stored wrapped) -> 181.5 (stored unwrapped), two steps of 2 h; rows 3, 4 are not the track's
    st[0, :, 0, 1] = [179.5, -179.5, 181.5, np.nan, np.nan]
    st[0, :, 1, 1] = [10.0, 11.0, 12.0, np.nan, np.nan]
    dt[:, 1] = 2.0
    # pauses: dt = 1, 0, 0, 1: rows 1, 2 and 3 share a clock time and the smallest wins
    dt[:, 2] = [1.0, 0.0, 0.0, 1.0]
    st[0, :, 0, 2] = [20.0, 21.0, 22.0, 23.0, 24.0]
    st[0, :, 1, 2] = [-5.0, -5.5, -6.0, -6.5, -7.0]
    # empty: one row
    st[0, 0, :, 3] = [45.0, 45.0, 7.0, 90.0]
    st[0, 1:, :, 3] = np.nan
    for b in (4, 5, 6):
        st[0, :, 0, b], st[0, :, 1, b] = 30.0 + np.arange(5.0), 1.0
    dt[1, 4], dt[2, 5] = np.nan, -0.5
    # nan latitude at row 2: steps 1 and 2 are broken, the rows beside it still answer
    st[0, :, 0, 7] = [-60.0, -59.0, -58.0, -57.0, -56.0]
    st[0, :, 1, 7] = [40.0, 41.0, np.nan, 43.0, 44.0]
    st[0, :, 2, 7] = 5.0
    st[0, :, 3, 7] = 180.0
    states = np.concatenate([st, st], axis=0)
    states[1, :, 1] += 0.25
    queries = [("eq at t0", 0, 10.0), ("eq knot 1", 0, 11.0), ("eq knot 2", 0, 12.0), ("eq knot 3", 0, 13.0),
               ("eq last knot", 0, 14.0), ("eq mid step 0", 0, 10.5), ("eq quarter step 0", 0, 10.25), ("eq in step 3", 0, 13.75),
               ("eq before", 0, 9.5), ("eq after", 0, 14.5), ("eq nan time", 0, np.nan), ("eq inf time", 0, np.inf),
               ("am mid step 0", 1, -2.0), ("am knot 1", 1, -1.0), ("am in step 1", 1, 0.5), ("am last knot", 1, 1.0),
               ("am past its steps", 1, 2.0),
               ("pause at 1", 2, 1.0), ("pause mid step 0", 2, 0.5), ("pause mid step 3", 2, 1.5), ("pause last", 2, 2.0),
               ("empty at t0", 3, 5.0), ("empty off t0", 3, 5.5),
               ("nan dt", 4, 0.5), ("negative dt", 5, 0.0), ("nan t0", 6, 1.0),
               ("index -1", -1, 1.0), ("index B", HAND_B, 1.0),
               ("nl knot 1", 7, 101.0), ("nl step 1", 7, 101.5), ("nl knot 2", 7, 102.0), ("nl step 2", 7, 102.5),
               ("nl knot 3", 7, 103.0), ("nl step 0", 7, 100.5), ("nl step 3", 7, 103.5)]
    _CACHE["hand"] = dict(states=states, nsteps=nsteps, dt=dt, t0=t0, names=[q[0] for q in queries],
                          qtrack=np.array([q[1] for q in queries], dtype=np.int32),
                          qtime=np.array([q[2] for q in queries], dtype=np.float64))
    return _CACHE["hand"]


# name -> (status, step, frac, lon, lat, speed, heading) of sample 0; None = NaN
HAND_ANSWERS = {
    "eq at t0": (0, 0, 0.0, 0.0, 0.0, 10.0, 350.0), "eq knot 1": (0, 1, 0.0, 1.0, 0.0, 12.0, 10.0),
    "eq knot 2": (0, 2, 0.0, 2.0, 0.0, 14.0, 30.0), "eq knot 3": (0, 3, 0.0, 3.0, 0.0, 16.0, 20.0),
    "eq last knot": (0, 4, 0.0, 4.0, 0.0, 18.0, 10.0),  # 730 % 360
    "eq mid step 0": (0, 0, 0.5, 0.5, 0.0, 11.0, 0.0),  # 350 + 0.5 * 20 = 360: through north, not through 180
    "eq quarter step 0": (0, 0, 0.25, 0.25, 0.0, 10.5, 355.0),
    "eq in step 3": (0, 3, 0.75, 3.75, 0.0, 17.5, 12.5),  # 20 + 0.75 * wrap180(710) = 20 - 7.5
    "eq before": (OUTSIDE, -1, None, None, None, None, None), "eq after": (OUTSIDE, -1, None, None, None, None, None),
    "eq nan time": (BAD_TIME, -1, None, None, None, None, None), "eq inf time": (BAD_TIME, -1, None, None, None, None, None),
    "am mid step 0": (0, 0, 0.5, -180.0, 10.5, 0.0, 0.0),  # 179.5 + 0.5 * 1 = 180 -> -180: the result lies in [-180, 180)
    "am knot 1": (0, 1, 0.0, -179.5, 11.0, 0.0, 0.0),
    "am in step 1": (0, 1, 0.75, -178.75, 11.75, 0.0, 0.0),
    "am last knot": (0, 2, 0.0, -178.5, 12.0, 0.0, 0.0),  # wrap180(181.5)
    "am past its steps": (OUTSIDE, -1, None, None, None, None, None),
    "pause at 1": (0, 1, 0.0, 21.0, -5.5, 0.0, 0.0),  # rows 1, 2, 3 share the time: the smallest
    "pause mid step 0": (0, 0, 0.5, 20.5, -5.25, 0.0, 0.0), "pause mid step 3": (0, 3, 0.5, 23.5, -6.75, 0.0, 0.0),
    "pause last": (0, 4, 0.0, 24.0, -7.0, 0.0, 0.0),
    "empty at t0": (0, 0, 0.0, 45.0, 45.0, 7.0, 90.0), "empty off t0": (OUTSIDE, -1, None, None, None, None, None),
    "nan dt": (BAD_TIME, -1, None, None, None, None, None), "negative dt": (BAD_TIME, -1, None, None, None, None, None),
    "nan t0": (BAD_TIME, -1, None, None, None, None, None),
    "index -1": (BAD_INDEX, -1, None, None, None, None, None), "index B": (BAD_INDEX, -1, None, None, None, None, None),
    "nl knot 1": (0, 1, 0.0, -59.0, 41.0, 5.0, 180.0), "nl step 1": (0, 1, 0.5, None, None, None, None),
    "nl knot 2": (0, 2, 0.0, -58.0, None, 5.0, 180.0), "nl step 2": (0, 2, 0.5, None, None, None, None),
    "nl knot 3": (0, 3, 0.0, -57.0, 43.0, 5.0, 180.0), "nl step 0": (0, 0, 0.5, -59.5, 40.5, 5.0, 180.0),
    "nl step 3": (0, 3, 0.5, -56.5, 43.5, 5.0, 180.0),
}


def check_hand_answers(r, what):
    """``r``: the outputs for ``hand_batch()`` (restatement or device).  Every value of HAND_ANSWERS is exact in binary, so
    the comparison is exact; sample 1 lies 0.25 degrees north of sample 0 and is otherwise the same."""
    h = hand_batch()
    assert set(h["names"]) == set(HAND_ANSWERS)
    for q, name in enumerate(h["names"]):
        status, step, frac, *vals = HAND_ANSWERS[name]
        assert int(r["status"][q]) == status and int(r["step"][q]) == step, (what, name, int(r["status"][q]), int(r["step"][q]))
        got = [r["frac"][q]] + [r[k][0, q] for k in PER_SAMPLE]
        for label, g, w in zip(("frac",) + PER_SAMPLE, got, [frac] + vals):
            assert (np.isnan(g) if w is None else g == w), (what, name, label, g, w)
        for k in PER_SAMPLE:
            a, b = r[k][0, q], r[k][1, q]
            assert (np.isnan(a) and np.isnan(b)) or b == (a + 0.25 if k == "lat" else a), (what, name, k, "sample 1")
    lon = r["lon"][np.isfinite(r["lon"])]
    assert (lon >= -180.0).all() and (lon < 180.0).all()


# ---- the fleet: S = 5, Nmax = 9, B = 70 (a wave plus six lanes), ragged, half the ships astride the antimeridian ------------
FLEET_S, FLEET_N, FLEET_B, FLEET_SEED = 5, 9, 70, 11
FLEET_WINDOW = (3, 70)
FLEET_BAD = {11: "nan dt", 23: "negative dt", 37: "nan t0"}
FLEET_BROKEN = (0, 5, 4, 1)  # (sample, track, row, component): a NaN latitude that an interior query meets


def fleet():
    """dict(states (5, 10, 4, 70), nsteps (t % 10: every length 0 .. 9), dt (9, 70) with steps of 0 hours among them, t0 (70,),
    qtrack, qtime (Q,)).  Even tracks start within half a degree of the antimeridian, every fourth of them stored unwrapped
    (longitudes past 180).  Queries: every knot of every track, the knots of tracks 0 .. 7 once more, three times inside
    the steps of every track that has any, one time before and one after every track, a NaN time and two indices outside
    [0, B); shuffled, so neither tracks nor times arrive in order."""
    if "fleet" in _CACHE:
        return _CACHE["fleet"]
    rng = np.random.default_rng(FLEET_SEED)
    S, N, B = FLEET_S, FLEET_N, FLEET_B
    st = np.zeros((S, N + 1, 4, B))
    astride = np.arange(B) % 2 == 0
    lon0 = np.where(astride, 180.0 + rng.uniform(-0.5, 0.5, B), rng.uniform(-170.0, 170.0, B))
    lat0 = rng.uniform(-60.0, 60.0, B)
    drift = rng.normal(0.0, 0.05, (2, B))
    steps = drift[None, None] + rng.normal(0.0, 0.02, (S, N, 2, B))
    st[:, 0, 0], st[:, 0, 1] = lon0, lat0
    st[:, 1:, :2] = np.stack([lon0, lat0])[None, None] + np.cumsum(steps, axis=1)
    wrapped = np.arange(B) % 4 != 0
    st[:, :, 0, wrapped] = wrap180(st[:, :, 0, wrapped])
    st[:, :, 2] = rng.uniform(0.0, 30.0, (S, N + 1, B))
    st[:, :, 3] = rng.uniform(-720.0, 720.0, (S, N + 1, B))  # headings as a filter leaves them: not reduced
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    dt = rng.uniform(0.2, 1.5, (N, B))
    dt[rng.uniform(size=(N, B)) < 0.05] = 0.0
    t0 = np.round(rng.uniform(-50.0, 50.0, B), 2)
    for t, kind in FLEET_BAD.items():
        assert nsteps[t] >= 1
        if kind == "nan dt":
            dt[0, t] = np.nan
        elif kind == "negative dt":
            dt[nsteps[t] - 1, t] = -0.25
        else:
            t0[t] = np.nan
    s, t, row, c = FLEET_BROKEN
    assert nsteps[t] > row and dt[row, t] > 0.0 and dt[row - 1, t] > 0.0
    st[s, row, c, t] = np.nan
    T = knot_times(nsteps, np.nan_to_num(dt))
    qs = []
    for t in range(B):
        ns, clock = int(nsteps[t]), (0.0 if np.isnan(t0[t]) else t0[t])
        knots = [clock + T[k, t] for k in range(ns + 1)]
        qs += [(t, v) for v in knots]
        if t < 8:
            qs += [(t, v) for v in knots]
        if ns > 0:
            for _ in range(3):
                k = int(rng.integers(ns))
                qs.append((t, knots[k] + rng.uniform(0.05, 0.95) * (knots[k + 1] - knots[k])))
        if t == FLEET_BROKEN[1]:
            qs.append((t, knots[FLEET_BROKEN[2]] + 0.5 * dt[FLEET_BROKEN[2], t]))
        qs += [(t, knots[0] - rng.uniform(0.1, 5.0)), (t, knots[-1] + rng.uniform(0.1, 5.0))]
    qs += [(1, np.nan), (-1, 0.0), (B, 0.0)]
    order = rng.permutation(len(qs))
    _CACHE["fleet"] = dict(states=st, nsteps=nsteps, dt=dt, t0=t0, qtrack=np.array([qs[i][0] for i in order], dtype=np.int32),
                           qtime=np.array([qs[i][1] for i in order], dtype=np.float64))
    return _CACHE["fleet"]


def fleet_anchor():
    """(2, Q): sample 0's own position at each query (0 where it has none), rounded to 1e-3 degrees."""
    if "anchor" not in _CACHE:
        w = fleet()
        r = positions(w["states"][:1], w["nsteps"], w["dt"], w["qtrack"], w["qtime"], w["t0"])
        _CACHE["anchor"] = np.round(np.nan_to_num(np.stack([r["lon"][0], r["lat"][0]])), 3)
    return _CACHE["anchor"]


def fleet_reference():
    """The restatement on the fleet with moments about ``fleet_anchor()`` from zero, computed once; read-only."""
    if "ref" not in _CACHE:
        w = fleet()
        ref = positions(w["states"], w["nsteps"], w["dt"], w["qtrack"], w["qtime"], w["t0"], anchor=fleet_anchor())
        for v in ref.values():
            v.setflags(write=False)
        _CACHE["ref"] = ref
    return _CACHE["ref"]
