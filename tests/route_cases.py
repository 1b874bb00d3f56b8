"""NumPy restatement of the route quantities (include/ste.h: ste_route_metrics_f64; DESIGN.md, "Routes"), a brute force over
every monotone coupling that checks it, and the batches its tests share.

For pair (i, j) of sample s, with the points a = 0 .. ns_i of track i and b = 0 .. ns_j of track j (row b, or row ns_j - b with
the reverse flag):
    point            u = (cos(phi) cos(lambda), cos(phi) sin(lambda), sin(phi)), lambda = lon * kDeg2Rad, phi = lat * kDeg2Rad
    cell             q(a, b) = (d.x * d.x + d.y * d.y) + d.z * d.z, d = u_i(a) - u_j(b); not finite counts as +inf
    cost             (2 * 6378.137) * asin(min(0.5 * sqrt(q), 1))
    admissible       band == 0 or |a - b| <= band
    predecessor      of (a-1, b-1), (a-1, b), (a, b-1), among the admissible ones that exist, the first; a later one only when
                     its table value is strictly smaller
    F, at            F(0, 0) = q(0, 0) at (0, 0); m = F(predecessor); q >= m: F = q, at = (a, b); else F = m, at = at(predecessor)
    D, L             D(0, 0) = cost, L = 1; D = cost + D(predecessor), L = 1 + L(predecessor)
    outputs          at (ns_i, ns_j): frechet = the leg of path_metrics between the two rows of `at`, dtw = D, dtw_len = L

The recurrence is evaluated along anti-diagonals for every (sample, pair) at once: the cells of a diagonal depend on the two
diagonals before it alone, which are all that is kept.  A cell that does not exist or is not admissible holds +inf.
"""
import itertools

import numpy as np
import path_metrics_cases as pmc

K_DEG2RAD = 0.017453292519943295
TWO_R = 2.0 * 6378.137
BAD_INDEX, NO_PATH, NOT_FINITE = 1, 2, 4
DTW_ATOL_PER_CELL = 1e-9  # km: 200 x the 5.4e-12 km per cell of the cost's form against 50 digits (the issue's measurement)
NEAR_TIE_EPS = 1e-13
_CACHE = {}


def unit_vectors(lon, lat):
    lam, phi = np.asarray(lon) * K_DEG2RAD, np.asarray(lat) * K_DEG2RAD
    c = np.cos(phi)
    return np.stack([c * np.cos(lam), c * np.sin(lam), np.sin(phi)], axis=-1)


def cell_q(ui, uj, axis=-1):
    """The squared chord between unit vectors whose components lie along ``axis``."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (np.take(ui, c, axis=axis) - np.take(uj, c, axis=axis) for c in range(3))
        q = (dx * dx + dy * dy) + dz * dz
    return np.where(np.isfinite(q), q, np.inf)


def cell_cost(q):
    with np.errstate(invalid="ignore"):
        h = 0.5 * np.sqrt(q)
    return TWO_R * np.arcsin(np.where(h > 1.0, 1.0, h))


def route_tables(UI, UJ, ni, nj, band=0, perturb=None, chunk=160):
    """``UI`` (I, A, 3) and ``UJ`` (I, M, 3): unit vectors of the points of the two curves of I items (track j already in point
    order), ``ni`` and ``nj`` (I,): the last point of each.  ``perturb``: a seed; every q and every cost is then scaled by a
    factor 1 +- NEAR_TIE_EPS of its own.  Returns F, at_a, at_b, D, L at (ni, nj), (I,) each.  ``chunk`` items at a time."""
    I = UI.shape[0]
    ni, nj = np.asarray(ni, dtype=np.int64), np.asarray(nj, dtype=np.int64)
    rng = None if perturb is None else np.random.default_rng(perturb)
    parts = [_route_tables(UI[lo:lo + chunk], UJ[lo:lo + chunk], ni[lo:lo + chunk], nj[lo:lo + chunk], band, rng)
             for lo in range(0, I, chunk)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(5))


def _route_tables(UI, UJ, ni, nj, band, rng):
    I, A, _ = UI.shape
    M = UJ.shape[1]
    K = int((ni + nj).max()) + 1
    a = np.arange(A, dtype=np.int64)[None, :]
    inf = np.inf
    # every cell's q and cost, then skewed: diagonal k holds the cells (a, k - a)
    q = cell_q(np.moveaxis(UI, 2, 0)[:, :, :, None], np.moveaxis(UJ, 2, 0)[:, :, None, :], axis=0)
    cost = cell_cost(q)
    if rng is not None:
        q = q * (1.0 + NEAR_TIE_EPS * (2.0 * rng.integers(0, 2, size=q.shape, dtype=np.int8) - 1.0))
        cost = cost * (1.0 + NEAR_TIE_EPS * (2.0 * rng.integers(0, 2, size=q.shape, dtype=np.int8) - 1.0))
    bk = np.clip(np.arange(K, dtype=np.int64)[:, None] - a, 0, M - 1)  # (K, A)
    qs, cs = q[:, a, bk], cost[:, a, bk]  # (I, K, A)
    # diagonal k - 1 and k - 2 by row, shifted by one: column a + 1 holds row a, column 0 the row above the table
    p1 = dict(F=np.full((I, A + 1), inf), A=np.full((I, A + 1), -1), B=np.full((I, A + 1), -1), D=np.full((I, A + 1), inf),
              L=np.zeros((I, A + 1), dtype=np.int64))
    p2 = {k: v.copy() for k, v in p1.items()}
    out = dict(F=np.full((I,), inf), A=np.full((I,), -1), B=np.full((I,), -1), D=np.full((I,), inf), L=np.zeros((I,), dtype=np.int64))
    item = np.arange(I)
    for k in range(K):
        # rows lo .. hi - 1 have a cell on this diagonal; a row outside holds values that no cell of the table reads any more
        lo, hi = max(0, k - (M - 1)), min(A - 1, k) + 1
        ak = a[:, lo:hi]
        b = k - ak
        ok = (b <= nj[:, None]) & (ak <= ni[:, None])
        if band > 0:
            ok &= np.abs(ak - b) <= band
        q, cost = qs[:, k, lo:hi], cs[:, k, lo:hi]
        origin = k == 0
        up, left = slice(lo, hi), slice(lo + 1, hi + 1)  # row a - 1 and row a in the shifted arrays
        cur = {}
        # Frechet: diag, up, left; a later one only when strictly smaller
        mF, mA, mB = p2["F"][:, up], p2["A"][:, up], p2["B"][:, up]
        for sl in (up, left):
            sel = p1["F"][:, sl] < mF
            mF, mA, mB = np.where(sel, p1["F"][:, sl], mF), np.where(sel, p1["A"][:, sl], mA), np.where(sel, p1["B"][:, sl], mB)
        here = (q >= mF) | origin
        cur["F"] = np.where(ok, np.where(here, q, mF), inf)
        cur["A"], cur["B"] = np.where(here, ak, mA), np.where(here, b, mB)
        mD, mL = p2["D"][:, up], p2["L"][:, up]
        for sl in (up, left):
            sel = p1["D"][:, sl] < mD
            mD, mL = np.where(sel, p1["D"][:, sl], mD), np.where(sel, p1["L"][:, sl], mL)
        cur["D"] = np.where(ok, cost if origin else cost + mD, inf)
        cur["L"] = np.ones_like(mL) if origin else 1 + mL
        last = ni + nj == k
        if last.any():
            for name in out:
                out[name][last] = cur[name][item[last], ni[last] - lo]
        p2, p1 = p1, p2  # the older diagonal's arrays take the new one
        for name, v in cur.items():
            p1[name][:, left] = v
    return out["F"], out["A"], out["B"], out["D"], out["L"]


def route_metrics(states, nsteps, pairs, band=0, reverse=False, model="sphere", perturb=None, leg=True):
    """``states`` (S, N+1, 4, B) in the device layout, ``nsteps`` (B,), ``pairs`` (P, 2) -> dict(frechet (S, P) km, frechet_at
    (S, P, 2) int32, dtw (S, P) km, dtw_len (S, P) int32, status (S, P) int32, F (S, P): the squared chord behind frechet)."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    pairs = np.asarray(pairs, dtype=np.int64)
    P = len(pairs)
    nsteps = np.clip(np.asarray(nsteps, dtype=np.int64), 0, rows - 1)
    status = np.zeros((P,), dtype=np.int32)
    bad = ((pairs < 0) | (pairs >= B)).any(axis=1)
    status[bad] = BAD_INDEX
    pi, pj = np.where(bad, 0, pairs[:, 0]), np.where(bad, 0, pairs[:, 1])
    ni, nj = nsteps[pi], nsteps[pj]
    if band > 0:
        status[~bad & (np.abs(ni - nj) > band)] = NO_PATH
    out = {"frechet": np.full((S, P), np.nan), "frechet_at": np.full((S, P, 2), -1, dtype=np.int32), "dtw": np.full((S, P), np.nan),
           "dtw_len": np.zeros((S, P), dtype=np.int32), "status": np.tile(status, (S, 1)), "F": np.full((S, P), np.nan)}
    run = np.flatnonzero(status == 0)
    if not run.size:
        return out
    A, M = int(ni[run].max()) + 1, int(nj[run].max()) + 1
    UI, UJ = [], []
    for s in range(S):
        U = unit_vectors(states[s, :, 0, :], states[s, :, 1, :])  # (rows, B, 3)
        UI.append(U[:A, pi[run]].transpose(1, 0, 2))
        rj = np.arange(M)[None, :]
        rj = np.clip(nj[run][:, None] - rj if reverse else rj, 0, rows - 1)  # (I, M): the row of point b
        UJ.append(np.broadcast_to(U[rj, pj[run][:, None]], (len(run), M, 3)))
    # every (sample, pair) at once
    F, atA, atB, D, L = (v.reshape(S, len(run)) for v in route_tables(np.concatenate(UI), np.concatenate(UJ), np.tile(ni[run], S),
                                                                     np.tile(nj[run], S), band, perturb))
    for s in range(S):
        for n, p in enumerate(run):
            out["F"][s, p] = F[s, n]
            if not F[s, n] < np.inf:
                out["status"][s, p] |= NOT_FINITE
                continue
            ra, rb = int(atA[s, n]), int(nj[p] - atB[s, n] if reverse else atB[s, n])
            out["frechet_at"][s, p] = (ra, rb)
            out["dtw"][s, p], out["dtw_len"][s, p] = D[s, n], L[s, n]
            if leg:
                out["frechet"][s, p] = pmc.leg_km(model, states[s, ra, 0, pi[p]], states[s, ra, 1, pi[p]],
                                                  states[s, rb, 0, pj[p]], states[s, rb, 1, pj[p]])
    return out


def near_ties(states, nsteps, pairs, band=0, reverse=False, ref=None):
    """(at_tie, len_tie), (S, P) bool each: the restatement rerun twice with every q and cost scaled by seeded factors
    1 +- 1e-13 changes frechet_at, or dtw_len."""
    if ref is None:
        ref = route_metrics(states, nsteps, pairs, band, reverse, leg=False)
    at_tie = np.zeros(ref["dtw_len"].shape, dtype=bool)
    len_tie = at_tie.copy()
    for seed in (101, 202):
        again = route_metrics(states, nsteps, pairs, band, reverse, perturb=seed, leg=False)
        at_tie |= (again["frechet_at"] != ref["frechet_at"]).any(axis=-1)
        len_tie |= again["dtw_len"] != ref["dtw_len"]
    return at_tie, len_tie


# ---- brute force: every monotone coupling, no dynamic programme ---------------------------------------------------------------
def couplings(n, m, band=0):
    """Every path from (0, 0) to (n - 1, m - 1) in steps (1, 1), (1, 0), (0, 1) through admissible cells, as lists of cells."""
    ok = lambda a, b: band == 0 or abs(a - b) <= band  # noqa: E731
    paths = []

    def walk(path):
        a, b = path[-1]
        if (a, b) == (n - 1, m - 1):
            paths.append(list(path))
            return
        for da, db in ((1, 1), (1, 0), (0, 1)):
            if a + da < n and b + db < m and ok(a + da, b + db):
                path.append((a + da, b + db))
                walk(path)
                path.pop()

    walk([(0, 0)])
    return paths


def brute_force(ci, cj, band=0):
    """Curves (n, 2) and (m, 2) -> dict(F, at (None on a tie), D, L (None on a tie)) from the couplings one by one."""
    ui, uj = unit_vectors(ci[:, 0], ci[:, 1]), unit_vectors(cj[:, 0], cj[:, 1])
    q = cell_q(ui[:, None, :], uj[None, :, :])
    cost = cell_cost(q)
    best_f, best_d, lens = np.inf, np.inf, []
    for path in couplings(len(ci), len(cj), band):
        f = max(q[c] for c in path)
        d = cost[path[0]]
        for c in path[1:]:
            d = cost[c] + d
        best_f = min(best_f, f)
        if d < best_d:
            best_d, lens = d, [len(path)]
        elif d == best_d:
            lens.append(len(path))
    where = np.argwhere(q == best_f)
    return {"F": best_f, "at": tuple(int(v) for v in where[0]) if len(where) == 1 else None, "D": best_d,
            "L": lens[0] if len(lens) == 1 else None}


# ---- hand-made curves ------------------------------------------------------------------------------------------------------------
HAND_ROWS = 20


def _line(lons, lat):
    lons = np.asarray(lons, dtype=np.float64)
    return np.stack([lons, np.full(lons.shape, float(lat))], axis=1)


def hand_batch():
    """Nine tracks of unequal length, rows past nsteps NaN: 0 a bent track of 7 points, 1 its copy, 2 its reverse, 3 six points
    on the equator a degree apart, 4 the same a degree north, 5 a single point, 6 track 3 with a NaN latitude in row 2, 7 eleven
    points on the equator, 8 the same route a tenth of a degree north with a detour: on to 7 degrees, back to 3, on to 10."""
    if "hand" in _CACHE:
        return _CACHE["hand"]
    bent = np.array([(10.0, 50.0), (10.5, 50.25), (11.0, 50.25), (11.75, 50.0), (12.0, 49.5), (12.0, 49.0), (12.5, 48.75)])
    nanrow = _line(np.arange(6.0), 0.0)
    nanrow[2, 1] = np.nan
    detour = list(range(8)) + [6, 5, 4, 3] + list(range(4, 11))
    tracks = [bent, bent.copy(), bent[::-1].copy(), _line(np.arange(6.0), 0.0), _line(np.arange(6.0), 1.0), np.array([(2.25, 0.5)]),
              nanrow, _line(np.arange(11.0), 0.0), _line(detour, 0.125)]
    B = len(tracks)
    states = np.full((1, HAND_ROWS, 4, B), np.nan)
    nsteps = np.zeros((B,), dtype=np.int32)
    for t, c in enumerate(tracks):
        assert len(c) <= HAND_ROWS
        states[0, :len(c), :2, t] = c
        nsteps[t] = len(c) - 1
    pairs = np.array([(0, 1), (0, 0), (0, 2), (3, 4), (5, 3), (3, 5), (7, 8), (8, 7), (3, 6), (6, 6), (-1, 0), (0, B), (4, 3)],
                     dtype=np.int32)
    _CACHE["hand"] = dict(states=states, nsteps=nsteps, pairs=pairs, tracks=tracks, dt=np.zeros((HAND_ROWS - 1, B)))
    return _CACHE["hand"]


def hausdorff_km(ca, cb):
    """Directed discrete Hausdorff distance on the sphere: the largest distance from a point of ca to its nearest point of cb."""
    return max(min(pmc.leg_km("sphere", *p, *r) for r in cb) for p in ca)


def check_hand_answers(plain, rev, band2, what, model="sphere"):
    """``plain``: the hand batch unreversed without a band; ``rev``: with the reverse flag; ``band2``: unreversed, band 2."""
    h = hand_batch()
    pairs, tr = h["pairs"].tolist(), h["tracks"]
    col = {tuple(p): k for k, p in enumerate(pairs)}

    def row(res, p):
        k = col[p]
        return (float(res["frechet"][0, k]), tuple(int(v) for v in res["frechet_at"][0, k]), float(res["dtw"][0, k]),
                int(res["dtw_len"][0, k]), int(res["status"][0, k]))

    def dead(res, p, bit):
        f, at, d, n, st = row(res, p)
        assert np.isnan(f) and np.isnan(d) and at == (-1, -1) and n == 0 and st == bit, (what, p, f, at, d, n, st)

    # identical tracks, a track against itself, and a track against its reverse with the flag
    for res, p in ((plain, (0, 1)), (plain, (0, 0)), (rev, (0, 2))):
        f, at, d, n, st = row(res, p)
        assert f == 0.0 and d == 0.0 and n == 7 and st == 0, (what, p, f, d, n, st)
    assert row(plain, (0, 2))[0] > 100.0 and row(rev, (0, 1))[0] > 100.0  # the reverse flag does something
    # two parallels a degree apart: every point's nearest is across, one degree of meridian
    for p in ((3, 4), (4, 3)):
        f, at, d, n, st = row(plain, p)
        assert st == 0 and n == 6 and at[0] == at[1]
        if model == "sphere":
            assert abs(f - pmc.KM_PER_DEG_EQUATOR) <= 1e-12 * pmc.KM_PER_DEG_EQUATOR, (what, p, f)
            assert abs(d - 6.0 * pmc.KM_PER_DEG_EQUATOR) <= 1e-12 * d, (what, p, d)
    # a single point against six: the largest distance, the sum, six cells
    legs = [pmc.leg_km("sphere", *tr[5][0], *r) for r in tr[3]]
    for p in ((5, 3), (3, 5)):
        f, at, d, n, st = row(plain, p)
        assert st == 0 and n == 6 and at == ((0, 5) if p == (5, 3) else (5, 0)), (what, p, at)  # the far end, 2.75 degrees east
        assert abs(d - sum(legs)) <= 1e-12 * d, (what, p, d, sum(legs))
        if model == "sphere":
            assert abs(f - max(legs)) <= 1e-12 * f, (what, p, f, max(legs))
    # the detour: each point of either curve has one of the other a tenth of a degree away, yet the coupling has to wait
    hd = max(hausdorff_km(tr[7], tr[8]), hausdorff_km(tr[8], tr[7]))
    for p in ((7, 8), (8, 7)):
        f = row(plain, p)[0]
        assert hd < 15.0 and f > 200.0 and f > 10.0 * hd, (what, p, f, hd)
    # status: a NaN row, indices outside the batch, and lengths further apart than the band
    dead(plain, (3, 6), NOT_FINITE)
    dead(plain, (6, 6), NOT_FINITE)
    dead(plain, (-1, 0), BAD_INDEX)
    dead(plain, (0, len(tr)), BAD_INDEX)
    dead(band2, (5, 3), NO_PATH)
    dead(band2, (7, 8), NO_PATH)
    dead(band2, (-1, 0), BAD_INDEX)
    for p in ((0, 1), (3, 4)):  # the diagonal lies inside any band
        assert row(band2, p)[::2] == row(plain, p)[::2] and row(band2, p)[3] == row(plain, p)[3], (what, p)


# ---- the edge fleet: Nmax = 130, S = 3, four base routes, 48 ships, 160 pairs ------------------------------------------------
FLEET_N, FLEET_S, FLEET_BASES, FLEET_P, FLEET_SEED = 130, 3, 4, 160, 20
FLEET_NSTEPS = (0, 1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130)  # the edges of the strips of 64 rows
FLEET_B = FLEET_BASES * len(FLEET_NSTEPS)
FLEET_BAND = 70
FLEET_WINDOW = (5, 41)


def make_fleet(seed=FLEET_SEED):
    """Each base route is a 130-step random walk, N(0, 0.05) degrees per step plus a constant drift N(0, 0.03) degrees, started
    anywhere in +-170 lon and +-55 lat.  Every ship is its base route resampled at sorted uniform parameters with both ends
    pinned, plus N(0, 0.02) degrees of noise per sample; base r owns ships 12 r .. 12 r + 11, one per length in FLEET_NSTEPS.
    The pairs: 160 of the ordered pairs (i != j) within base routes, shuffled; a track against its own reverse is a table of
    exact ties, which the hand-made curves cover.  Rows past nsteps are NaN."""
    rng = np.random.default_rng(seed)
    N, S, B = FLEET_N, FLEET_S, FLEET_B
    states = np.full((S, N + 1, 4, B), np.nan)
    nsteps = np.zeros((B,), dtype=np.int32)
    allpairs = []
    for r in range(FLEET_BASES):
        start = np.array([rng.uniform(-170.0, 170.0), rng.uniform(-55.0, 55.0)])
        drift = rng.normal(0.0, 0.03, 2)
        base = start + np.concatenate([np.zeros((1, 2)), np.cumsum(drift + rng.normal(0.0, 0.05, (N, 2)), axis=0)])
        ships = []
        for n, ns in enumerate(FLEET_NSTEPS):
            t = r * len(FLEET_NSTEPS) + n
            ships.append(t)
            nsteps[t] = ns
            par = np.sort(rng.uniform(0.0, 1.0, ns + 1))
            par[0] = 0.0
            if ns > 0:
                par[-1] = 1.0
            pos = np.stack([np.interp(par * N, np.arange(N + 1.0), base[:, c]) for c in range(2)], axis=1)
            states[:, :ns + 1, :2, t] = pos[None] + rng.normal(0.0, 0.02, (S, ns + 1, 2))
            states[:, :ns + 1, 2:, t] = rng.normal(0.0, 1.0, (S, ns + 1, 2))  # speed and heading: not read
        allpairs += list(itertools.permutations(ships, 2))
    pairs = np.array(allpairs, dtype=np.int32)[rng.permutation(len(allpairs))[:FLEET_P]]
    return dict(states=states, nsteps=nsteps, pairs=pairs, dt=np.zeros((N, B)))


def fleet():
    if "fleet" not in _CACHE:
        _CACHE["fleet"] = make_fleet()
    return _CACHE["fleet"]


def fleet_reference(band, reverse, model="sphere"):
    """The restatement on the edge fleet with its near ties, computed once per (band, reverse, model)."""
    key = ("ref", band, reverse, model)
    if key not in _CACHE:
        w = fleet()
        base = ("ref", band, reverse, "sphere")
        if model != "sphere" and base in _CACHE:  # the model touches frechet alone
            ref = dict(_CACHE[base])
            at = ref["frechet_at"]
            ref["frechet"] = ref["frechet"].copy()
            for s, p in zip(*np.nonzero(ref["status"] == 0)):
                i, j = w["pairs"][p]
                ref["frechet"][s, p] = pmc.leg_km(model, *w["states"][s, at[s, p, 0], :2, i], *w["states"][s, at[s, p, 1], :2, j])
        else:
            ref = route_metrics(w["states"], w["nsteps"], w["pairs"], band, reverse, model)
            ref["at_tie"], ref["len_tie"] = near_ties(w["states"], w["nsteps"], w["pairs"], band, reverse, ref)
        _CACHE[key] = ref
    return _CACHE[key]


# ---- one long pair that leaves the LDS -----------------------------------------------------------------------------------------
def long_pair(lds_cols):
    """Two ships on one random walk: ns_i = lds_cols + 70 and ns_j = ns_i - 3 (S = 1)."""
    key = ("long", lds_cols)
    if key not in _CACHE:
        rng = np.random.default_rng(31)
        ni = lds_cols + 70
        nj = ni - 3
        base = np.array([20.0, -30.0]) + np.cumsum(np.array([0.01, 0.004]) + rng.normal(0.0, 0.01, (ni + 1, 2)), axis=0)
        states = np.full((1, ni + 1, 4, 2), np.nan)
        states[0, :, :2, 0] = base + rng.normal(0.0, 0.004, base.shape)
        par = np.linspace(0.0, ni, nj + 1)
        states[0, :nj + 1, :2, 1] = np.stack([np.interp(par, np.arange(ni + 1.0), base[:, c]) for c in range(2)], axis=1) + \
            rng.normal(0.0, 0.004, (nj + 1, 2))
        _CACHE[key] = dict(states=states, nsteps=np.array([ni, nj], dtype=np.int32), pairs=np.array([(0, 1)], dtype=np.int32),
                           dt=np.zeros((ni, 2)))
    return _CACHE[key]
