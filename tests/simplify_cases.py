"""Simplification of tracks within a tolerance (include/ste.h: ste_simplify_f64): the definition restated in NumPy, operation
for operation, so that the device is compared BIT FOR BIT, and the fleets of tests/test_simplify.py.

    clock        T_0 = 0, T_{k+1} = T_k + dt_k in order (np.cumsum adds in order); bad when a dt below ns is not finite or < 0
    longitude    X_0 = lon_0, X_{k+1} = X_k + wrap180(lon_{k+1} - lon_k) in order; broken when |delta| < 90 is false or a latitude
                 of rows 0 .. ns is not finite
    deviation    xk = (X_k - X_i) * c, yk = Y_k - Y_i, xj, yj alike; clock: den = T_j - T_i, u = den > 0 ? (T_k - T_i) / den : 0;
                 shape: den = xj * xj + yj * yj, u = den > 0 ? clamp01((xk * xj + yk * yj) / den) : 0;
                 ex = xk - u * xj, ey = yk - u * yj, d2 = ex * ex + ey * ey
    rule         the first row of the largest d2 of a range (a NaN never wins) is kept when d2 > tol * tol, else the range is
                 closed and worst_sq takes the d2 when that is larger
NumPy evaluates every one of these element by element in IEEE doubles, without contraction."""
import numpy as np
from track_sampling_cases import wrap180

BAD_TIME, BAD_LIMIT, BROKEN, TRUNCATED = 1, 2, 4, 8
KM_PER_DEG = 6378.137 * np.pi / 180.0
SENTINEL = -12345.5   # what the tests fill double outputs with: untouched entries keep it
SENTINEL_I = -7       # int32 outputs
SENTINEL_B = 9        # keep flags


def deviations(X, Y, T, c, i, j, shape):
    """d2 of rows i + 1 .. j - 1 from the chord (i, j)."""
    k = np.arange(i + 1, j)
    with np.errstate(all="ignore"):
        xk, yk = (X[k] - X[i]) * c, Y[k] - Y[i]
        xj, yj = (X[j] - X[i]) * c, Y[j] - Y[i]
        if shape:
            den = xj * xj + yj * yj
            q = (xk * xj + yk * yj) / den if den > 0.0 else np.zeros_like(xk)
            u = np.where(q < 0.0, 0.0, np.where(q > 1.0, 1.0, q)) if den > 0.0 else q
        else:
            den = T[j] - T[i]
            u = (T[k] - T[i]) / den if den > 0.0 else np.zeros_like(xk)
        ex, ey = xk - u * xj, yk - u * yj
        return ex * ex + ey * ey


def winner(d2):
    """(best, offset of the winner in d2): the smallest k with d2 > best scanning upwards, best starting at -1."""
    d = np.where(np.isnan(d2), -np.inf, d2)
    m = int(np.argmax(d))  # the first of equal rows
    return (float(d[m]), m) if d[m] > -1.0 else (-1.0, -1)


def staged(lon, lat, dts, shape):
    """(X, Y, T, status bits of the clock and the rows) of rows 0 .. ns."""
    status = 0
    with np.errstate(all="ignore"):
        T = np.cumsum(np.concatenate([[0.0], dts]))
        if not shape and (~np.isfinite(dts) | (dts < 0.0)).any():
            status |= BAD_TIME
        delta = wrap180(lon[1:] - lon[:-1])
        X = np.cumsum(np.concatenate([lon[:1], delta]))
        if (~(np.abs(delta) < 90.0)).any() or (~np.isfinite(lat)).any():
            status |= BROKEN
    return X, lat, T, status


def simplify_track(lon, lat, dts, c, tol, shape, order="lifo", rng=None):
    """One track of ns + 1 rows -> (keep (ns + 1,) uint8, worst_sq, status, depth): ``order`` takes the pending ranges last in
    first out ("lifo", both parts pushed: ``depth`` is the deepest level of that recursion), first in first out ("fifo") or at
    random ("random", with ``rng``)."""
    ns = len(lon) - 1
    X, Y, T, status = staged(lon, lat, dts, shape)
    if not (np.isfinite(c) and c >= 0.0 and np.isfinite(tol) and tol >= 0.0):
        status |= BAD_LIMIT
    if status:
        return np.ones(ns + 1, dtype=np.uint8), np.nan, status, 0
    keep = np.zeros(ns + 1, dtype=np.uint8)
    keep[0] = keep[ns] = 1
    tol2, worst, depth = tol * tol, 0.0, 0
    pending = [(0, ns, 1)] if ns > 1 else []
    while pending:
        at = {"lifo": -1, "fifo": 0}.get(order)
        i, j, level = pending.pop(int(rng.integers(len(pending))) if at is None else at)
        depth = max(depth, level)
        best, m = winner(deviations(X, Y, T, c, i, j, shape))
        if best > tol2:
            k = i + 1 + m
            keep[k] = 1
            pending += [(a, b, level + 1) for a, b in ((i, k), (k, j)) if b > a + 1]
        elif best > worst:
            worst = best
    return keep, worst, status, depth


def simplify(states, nsteps, dt, tol, scale, shape, cap=None):
    """The call restated: states (S, N+1, 4, B), dt (N, B) or None, tol and scale scalars or (B,) -> dict of keep, nkeep,
    worst_sq, status and, with ``cap``, rows, out_states and out_dt, untouched entries holding the sentinels."""
    S, rows, _, B = states.shape
    tol, scale = np.broadcast_to(np.asarray(tol, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(scale, dtype=np.float64), (B,))
    out = {"keep": np.full((S, rows, B), SENTINEL_B, dtype=np.uint8), "nkeep": np.zeros((S, B), dtype=np.int32),
           "worst_sq": np.zeros((S, B)), "status": np.zeros((S, B), dtype=np.int32)}
    if cap is not None:
        out.update(rows=np.full((S, cap, B), SENTINEL_I, dtype=np.int32), out_states=np.full((S, cap, 4, B), SENTINEL),
                   out_dt=np.full((S, cap - 1, B), SENTINEL))
    for s in range(S):
        for t in range(B):
            ns = int(nsteps[t])
            dts = dt[:ns, t] if dt is not None else np.zeros(ns)
            keep, worst, status, _ = simplify_track(states[s, :ns + 1, 0, t], states[s, :ns + 1, 1, t], dts, scale[t], tol[t], shape)
            r = np.flatnonzero(keep)
            out["keep"][s, :ns + 1, t] = keep
            out["nkeep"][s, t], out["worst_sq"][s, t] = len(r), worst
            if cap is not None:
                if len(r) > cap:
                    status |= TRUNCATED
                w = r[:cap]
                out["rows"][s, :len(w), t] = w
                out["out_states"][s, :len(w), :, t] = states[s, w, :, t]
                for m in range(min(len(r) - 1, cap - 1)):
                    acc = dt[r[m], t]
                    for q in range(r[m] + 1, r[m + 1]):
                        acc = acc + dt[q, t]
                    out["out_dt"][s, m, t] = acc
            out["status"][s, t] = status
    return out


def dropped_rows_within_tolerance(lon, lat, dts, c, tol, shape, keep):
    """The guarantee, recomputed by the formula: the largest d2 of a dropped row against its two surviving neighbours (0.0
    without a dropped row), and whether each is <= tol * tol."""
    X, Y, T, _ = staged(lon, lat, dts, shape)
    r = np.flatnonzero(keep)
    worst = 0.0
    for i, j in zip(r[:-1], r[1:]):
        if j > i + 1:
            d2 = deviations(X, Y, T, c, i, j, shape)
            assert (d2 <= tol * tol).all(), (i, j, d2.max(), tol * tol)
            worst = max(worst, float(d2.max()))
    return worst


# ---- the hand-made ships: on the equator, scale 1 ----------------------------------------------------------------------------
HAND_SHIPS = ("steady", "pace", "corner", "tie", "still", "antimeridian", "ns0", "ns1", "nan_lat", "neg_dt", "nan_tol")
HAND_TOL = np.array([0.1, 0.1, 0.5, 0.8, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, np.nan])
HAND_KEEP = {"steady": ([0, 6], [0, 6]), "pace": ([0, 3, 6], [0, 6]), "corner": ([0, 3, 6], [0, 3, 6]), "tie": ([0, 1, 4], [0, 1, 4]),
             "still": ([0, 6], [0, 6]), "antimeridian": ([0, 6], [0, 6]), "ns0": ([0], [0]), "ns1": ([0, 1], [0, 1])}  # clock, shape
HAND_STATUS = {"nan_lat": BROKEN, "neg_dt": BAD_TIME, "nan_tol": BAD_LIMIT}  # clock mode; shape has no bad clock


def hand_batch():
    """dict(states (1, 7, 4, 11), nsteps, dt (6, 11), tol (11,) degrees)."""
    B, N = len(HAND_SHIPS), 6
    st = np.zeros((1, N + 1, 4, B))
    dt = np.ones((N, B))
    ns = np.full(B, N, dtype=np.int32)
    k = np.arange(N + 1.0)
    col = {name: t for t, name in enumerate(HAND_SHIPS)}
    for name in ("steady", "pace", "ns0", "ns1", "nan_lat", "neg_dt", "nan_tol"):
        st[0, :, 0, col[name]] = k
    dt[:, col["pace"]] = [1, 1, 1, 3, 3, 3]
    st[0, :, 0, col["corner"]] = [0, 1, 2, 3, 3, 3, 3]
    st[0, :, 1, col["corner"]] = [0, 0, 0, 0, 1, 2, 3]
    st[0, :5, 0, col["tie"]], st[0, :5, 1, col["tie"]] = [0, 1, 2, 3, 4], [0, 1, 0, 1, 0]
    st[0, 5:, :2, col["tie"]] = 77.0  # past nsteps: never read
    ns[col["tie"]] = 4
    st[0, :, 0, col["still"]], st[0, :, 1, col["still"]] = 12.5, -3.25
    st[0, :, 0, col["antimeridian"]] = wrap180(179.5 + k)
    ns[col["ns0"]], ns[col["ns1"]] = 0, 1
    st[0, 2, 1, col["nan_lat"]] = np.nan
    st[0, 4, 1, col["nan_lat"]] = 0.5  # a row the identity keeps and the rule would, too
    dt[2, col["neg_dt"]] = -1.0
    st[0, 3, 1, col["neg_dt"]] = 1.0
    st[0, 3, 1, col["nan_tol"]] = 1.0
    st[0, :, 2, :], st[0, :, 3, :] = 10.0 + k[:, None], 90.0 - k[:, None]  # speed and heading: carried along by the compaction
    return dict(states=st, nsteps=ns, dt=dt, tol=HAND_TOL.copy())


def check_hand_answers(got, what, shape):
    """The known answers, on outputs of the restatement or of the device (keep, nkeep, worst_sq, status)."""
    h = hand_batch()
    for t, name in enumerate(HAND_SHIPS):
        ns = int(h["nsteps"][t])
        kept = np.flatnonzero(got["keep"][0, :ns + 1, t]).tolist()
        status = HAND_STATUS.get(name, 0)
        if shape and name == "neg_dt":
            status = 0
        assert got["status"][0, t] == status, (what, name, got["status"][0, t])
        if status:
            assert kept == list(range(ns + 1)) and got["nkeep"][0, t] == ns + 1 and np.isnan(got["worst_sq"][0, t]), (what, name)
        elif name in HAND_KEEP:
            assert kept == HAND_KEEP[name][int(shape)] and got["nkeep"][0, t] == len(kept), (what, name, kept)
            # a closed range of a steady leg leaves the rounding of (k / n) * n; the tie's range (1, 4) leaves 4/9 (shape: 0.4)
            limit = ((0.4 if shape else 4.0 / 9.0) + 1e-12) if name == "tie" else 1e-20
            assert 0.0 <= got["worst_sq"][0, t] <= limit, (what, name, got["worst_sq"][0, t])
        assert (got["keep"][0, ns + 1:, t] == SENTINEL_B).all(), (what, name, "rows past nsteps")


# ---- the walk fleet: S = 3, Nmax = 199, piecewise-steady courses with small noise ----------------------------------------------
WALK_S, WALK_N, WALK_SEED = 3, 199, 21
WALK_NSTEPS = (0, 1, 2, 62, 63, 64, 65, 127, 128, 129, 199, 3, 31, 33, 100, 150, 191, 192, 193, 198, 199, 199, 96, 199)
WALK_B = len(WALK_NSTEPS)
WALK_WINDOW = (3, 19)
WALK_TOL_KM = (0.0, 1.0, 10.0)
WALK_ANTIMERIDIAN = (10, 14, 20, 23)  # ships that start just west of 180 degrees and sail east
_CACHE = {}


def walk():
    """dict(states (3, 200, 4, 24), nsteps, dt (199, 24), factor (24,), scale (24,)): legs of 8 .. 40 steps at a steady course and
    speed (15 .. 35 km/h, steps of 0.05 .. 0.3 h that change with the leg, so the pace changes as well as the course), noise of
    0.3 km per row and sample; ``factor`` scales a tolerance per track (0.5 .. 2) and ``scale`` is cos of the start latitude."""
    if "walk" in _CACHE:
        return _CACHE["walk"]
    rng = np.random.default_rng(WALK_SEED)
    S, N, B = WALK_S, WALK_N, WALK_B
    st = np.zeros((S, N + 1, 4, B))
    dt = np.zeros((N, B))
    lat0 = rng.uniform(-60.0, 60.0, B)
    lon0 = rng.uniform(-170.0, 170.0, B)
    lon0[list(WALK_ANTIMERIDIAN)] = 179.9
    for t in range(B):
        x, y, k = np.zeros(N + 1), np.zeros(N + 1), 0
        head = rng.uniform(30.0, 150.0) if t in WALK_ANTIMERIDIAN else rng.uniform(0.0, 360.0)
        spd = np.zeros(N + 1)
        hd = np.zeros(N + 1)
        while k < N:
            n = min(int(rng.integers(8, 41)), N - k)
            v, h = rng.uniform(15.0, 35.0), rng.uniform(0.05, 0.3)
            dt[k:k + n, t] = h
            step = v * h / KM_PER_DEG
            x[k + 1:k + n + 1] = x[k] + step * np.sin(np.radians(head)) * np.arange(1, n + 1) / np.cos(np.radians(lat0[t]))
            y[k + 1:k + n + 1] = y[k] + step * np.cos(np.radians(head)) * np.arange(1, n + 1)
            spd[k:k + n + 1], hd[k:k + n + 1] = v, head % 360.0
            k += n
            head += rng.uniform(-70.0, 70.0) if t in WALK_ANTIMERIDIAN else rng.uniform(-120.0, 120.0)
        noise = rng.normal(0.0, 0.3 / KM_PER_DEG, (S, 2, N + 1))
        st[:, :, 0, t] = wrap180(lon0[t] + x[None] + noise[:, 0])
        st[:, :, 1, t] = lat0[t] + y[None] + noise[:, 1]
        st[:, :, 2, t], st[:, :, 3, t] = spd[None], hd[None]
    w = dict(states=st, nsteps=np.array(WALK_NSTEPS, dtype=np.int32), dt=dt, factor=rng.uniform(0.5, 2.0, B),
             scale=np.cos(np.radians(lat0)))
    _CACHE["walk"] = w
    return w


def walk_tolerance(tol_km):
    """Degrees per track of the walk fleet for a tolerance in km."""
    return walk()["factor"] * (tol_km / KM_PER_DEG)


def walk_reference(tol_km, shape, cap=WALK_N + 1):
    key = ("ref", tol_km, shape, cap)
    if key not in _CACHE:
        w = walk()
        _CACHE[key] = simplify(w["states"], w["nsteps"], w["dt"], walk_tolerance(tol_km), w["scale"], shape, cap)
    return _CACHE[key]


# ---- the unbalanced ship: every split takes about one row off an end ------------------------------------------------------------
UNBALANCED_ROWS = 160


def unbalanced(n=UNBALANCED_ROWS - 1):
    """dict(states (1, n + 1, 4, 1), nsteps, dt): x_k = k, y_k = (-1)^k (n - k) / n, steps of one hour, tolerance 0."""
    k = np.arange(n + 1.0)
    st = np.zeros((1, n + 1, 4, 1))
    st[0, :, 0, 0], st[0, :, 1, 0] = k, np.where(k % 2 == 0, 1.0, -1.0) * (n - k) / n
    return dict(states=st, nsteps=np.array([n], dtype=np.int32), dt=np.ones((n, 1)))


def long_track(rows, seed=5):
    """One track of ``rows`` rows for the workspace path: a slow zigzag with noise, steps of 0.1 h."""
    rng = np.random.default_rng(seed)
    k = np.arange(rows, dtype=np.float64)
    st = np.zeros((1, rows, 4, 1))
    st[0, :, 0, 0] = wrap180(178.0 + 0.002 * k + rng.normal(0.0, 2e-4, rows))
    st[0, :, 1, 0] = 10.0 + 0.05 * np.abs(((k / 150.0) % 2.0) - 1.0) + rng.normal(0.0, 2e-4, rows)
    return dict(states=st, nsteps=np.array([rows - 1], dtype=np.int32), dt=np.full((rows - 1, 1), 0.1))
