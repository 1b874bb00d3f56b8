"""NumPy restatement of the errors of tracks against truth positions (include/ste.h: ste_errors_f64, ste_track_errors_f64;
DESIGN.md, "Errors") and the small fleets its tests share.

For track t of sample s, with ns = nsteps[t], rows 0 .. ns of the state's (lon, lat), the truth's (lon_t, lat_t), the course
and the covariance's entries a = C00, b = C01, c = C11:
    truthed          both truth coordinates finite
    broken           a truthed row whose state is not finite, or whose leg is not: nbroken + 1, NaN in the row outputs
    e_k, h_k         path_metrics_cases.leg_km(truth -> state) and the heading of that leg: utils.heading's formula on the
                     sphere, geodesic.inverse's azimuth on WGS84 (0 and 0 for points closer than 1e-8 degrees)
    sums             n, sum_err += e, sum_sq += e * e, max_err / max_row (strict: the first row wins), cumerr = running sum_err
    along, cross     theta = (h - course) * DEG2RAD; e cos(theta), e sin(theta) where the course is finite
    nees             dx = wrap180(lon - lon_t), dy = lat - lat_t; det = a c - b b; q = (c dx dx - 2 b dx dy + a dy dy) / det;
                     scored when a, b, c, q are finite, a > 0 and det > 0; inside when q <= nees_limit
"""
import math

import numpy as np
import path_metrics_cases as pmc
from track_sampling_cases import wrap180

DEG2RAD = 0.017453292519943295
SENTINEL = -12345.0  # what the row outputs past nsteps hold: the call leaves them alone
SUMS = ("sum_err", "sum_sq", "max_err")
COUNTS = ("n", "max_row", "nbroken")
COURSE_SUMS = ("sum_along", "sum_along_sq", "sum_cross", "sum_cross_sq")
COURSE_OUTPUTS = COURSE_SUMS + ("ncoursed", "along", "cross")
NEES_OUTPUTS = ("sum_nees", "nscored", "ninside", "nees")
ROW_OUTPUTS = ("err", "cumerr", "along", "cross", "nees")
INT_OUTPUTS = ("n", "max_row", "nbroken", "ncoursed", "nscored", "ninside")
LIMIT95 = -2.0 * math.log(1.0 - 0.95)  # the chi-square quantile for 2 degrees of freedom: 5.99...
GAP_RTOL = 1e-6
K = pmc.KM_PER_DEG_EQUATOR
_CACHE = {}


def leg(model, lon1, lat1, lon2, lat2, head):
    """(e, h) of the leg from point 1 to point 2; h only where ``head`` (else 0.0).  Worked out once however many cases share it."""
    key = ("leg", model, float(lon1), float(lat1), float(lon2), float(lat2), bool(head))
    if key in _CACHE:
        return _CACHE[key]
    from track_estimators import geodesic, utils

    e, h = pmc.leg_km(model, lon1, lat1, lon2, lat2), 0.0
    if head and model == "sphere":
        h = float(utils.heading(lon1, lat1, lon2, lat2))
    elif head and not (abs(lat1 - lat2) < 1e-8 and abs(lon1 - lon2) < 1e-8):
        h = (geodesic.inverse(lat1, lon1, lat2, lon2)[1] + 360.0) % 360.0
    _CACHE[key] = (e, h)
    return e, h


def cov_entries(cov, k, t):
    """a, b, c = entries 00, 01, 11 of row k of track t of a (N+1, 16 or 10, B) covariance history."""
    return cov[k, 0, t], cov[k, 1, t], cov[k, 4 if cov.shape[1] == 10 else 5, t]


def track_errors(states, nsteps, truth, model="sphere", course=None, cov=None, nees_limit=LIMIT95):
    """``states`` (S, N+1, 4, B), ``nsteps`` (B,), ``truth`` (N+1, 2, B), ``course`` (N+1, B) or None, ``cov`` (N+1, 16 or 10, B)
    or None -> dict of every output of the call that exists for these inputs: per (sample, track) (S, B), per row (S, N+1, B)
    with SENTINEL past nsteps."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    out = {k: np.zeros((S, B)) for k in SUMS}
    out.update({k: np.zeros((S, B), dtype=np.int32) for k in COUNTS})
    out.update({k: np.full((S, rows, B), SENTINEL) for k in ("err", "cumerr")})
    if course is not None:
        out.update({k: np.zeros((S, B)) for k in COURSE_SUMS})
        out["ncoursed"] = np.zeros((S, B), dtype=np.int32)
        out.update({k: np.full((S, rows, B), SENTINEL) for k in ("along", "cross")})
    if cov is not None:
        assert S == 1
        out["sum_nees"] = np.zeros((S, B))
        out.update({k: np.zeros((S, B), dtype=np.int32) for k in ("nscored", "ninside")})
        out["nees"] = np.full((S, rows, B), SENTINEL)
    for s in range(S):
        for t in range(B):
            n = nbroken = ncoursed = nscored = ninside = 0
            sum_err = sum_sq = sum_al = sum_al2 = sum_cr = sum_cr2 = sum_q = 0.0
            max_err, max_row = -np.inf, -1
            for k in range(int(nsteps[t]) + 1):
                lon, lat = states[s, k, 0, t], states[s, k, 1, t]
                tlon, tlat = truth[k, 0, t], truth[k, 1, t]
                e = al = cr = q = np.nan
                if np.isfinite(tlon) and np.isfinite(tlat):
                    sound = np.isfinite(lon) and np.isfinite(lat)
                    if sound:
                        e, h = leg(model, tlon, tlat, lon, lat, course is not None)
                        sound = np.isfinite(e)
                    if not sound:
                        e = np.nan
                        nbroken += 1
                    else:
                        n += 1
                        sum_err = sum_err + e
                        sum_sq = sum_sq + e * e
                        if e > max_err:
                            max_err, max_row = e, k
                        if course is not None and np.isfinite(course[k, t]):
                            theta = (h - course[k, t]) * DEG2RAD
                            al, cr = e * np.cos(theta), e * np.sin(theta)
                            ncoursed += 1
                            sum_al, sum_al2 = sum_al + al, sum_al2 + al * al
                            sum_cr, sum_cr2 = sum_cr + cr, sum_cr2 + cr * cr
                        if cov is not None:
                            a, b, c = cov_entries(cov, k, t)
                            dx, dy = wrap180(lon - tlon), lat - tlat
                            with np.errstate(all="ignore"):
                                det = a * c - b * b
                                qk = (c * dx * dx - 2.0 * b * dx * dy + a * dy * dy) / det
                            if all(np.isfinite(x) for x in (a, b, c, qk)) and a > 0.0 and det > 0.0:
                                q = qk
                                nscored += 1
                                sum_q = sum_q + qk
                                ninside += int(qk <= nees_limit)
                out["err"][s, k, t], out["cumerr"][s, k, t] = e, sum_err
                if course is not None:
                    out["along"][s, k, t], out["cross"][s, k, t] = al, cr
                if cov is not None:
                    out["nees"][s, k, t] = q
            out["sum_err"][s, t], out["sum_sq"][s, t], out["max_err"][s, t] = sum_err, sum_sq, max_err if n else np.nan
            out["n"][s, t], out["max_row"][s, t], out["nbroken"][s, t] = n, max_row, nbroken
            if course is not None:
                out["sum_along"][s, t], out["sum_along_sq"][s, t] = sum_al, sum_al2
                out["sum_cross"][s, t], out["sum_cross_sq"][s, t], out["ncoursed"][s, t] = sum_cr, sum_cr2, ncoursed
            if cov is not None:
                out["sum_nees"][s, t], out["nscored"][s, t], out["ninside"][s, t] = sum_q, nscored, ninside
    return out


# ---- hand-made ships: Nmax = 3 --------------------------------------------------------------------------------------------
HAND_SHIPS = ("equator", "north0", "north90", "broken", "untruthed", "tie", "nosteps", "notruth", "antimeridian")
HAND_A, HAND_C = 0.04, 0.01  # the diagonal covariance of every row: q = dx^2 / 0.04 + dy^2 / 0.01


def hand_batch():
    """dict(states (1, 4, 4, 9), nsteps, truth (4, 2, 9), course (4, 9), cov (4, 16, 9)); ``check_hand_answers`` has the answers.
      equator       on the equator, the truth 0.5, 0.25, 0.125 and 0.0625 degrees west of the state, course 90: along = e
      north0        the state 0.25 degrees due north of the truth, course 0: along = e, cross = 0
      north90       the same under course 90: along = 0, cross = -e
      broken        equator with a NaN state in row 2
      untruthed     equator with no truth in row 1: cumerr carries
      tie           rows 0 and 2 are the same pair of points and the largest error: row 0 wins
      nosteps       equator with nsteps = 0: row 0 alone
      notruth       no truth at all: n = 0, NaN, -1
      antimeridian  the state at 179.9, the truth at -179.9: 0.2 degrees, heading west, dx = -0.2"""
    names = HAND_SHIPS
    B = len(names)
    st = np.zeros((1, 4, 4, B))
    truth = np.full((4, 2, B), np.nan)
    course = np.full((4, B), 90.0)
    off = np.array([0.5, 0.25, 0.125, 0.0625])
    for name in ("equator", "broken", "untruthed", "nosteps", "notruth"):
        t = names.index(name)
        st[0, :, 0, t] = 10.0 + np.arange(4.0)
        truth[:, 0, t], truth[:, 1, t] = st[0, :, 0, t] - off, 0.0
    for name, crs in (("north0", 0.0), ("north90", 90.0)):
        t = names.index(name)
        st[0, :, 0, t], st[0, :, 1, t] = 20.0, 30.0 + np.arange(4.0)
        truth[:, 0, t], truth[:, 1, t] = 20.0, st[0, :, 1, t] - 0.25
        course[:, t] = crs
    st[0, 2, 0, names.index("broken")] = np.nan
    truth[1, :, names.index("untruthed")] = np.nan
    truth[:, :, names.index("notruth")] = np.nan
    t = names.index("tie")
    st[0, :, 0, t] = [10.0, 11.0, 10.0, 13.0]
    truth[:, 0, t], truth[:, 1, t] = st[0, :, 0, t] - [0.5, 0.25, 0.5, 0.125], 0.0
    t = names.index("antimeridian")
    st[0, :, 0, t] = 179.9
    truth[:, 0, t], truth[:, 1, t] = -179.9, 0.0
    cov = np.zeros((4, 16, B))
    cov[:, 0], cov[:, 5], cov[:, 10], cov[:, 15] = HAND_A, HAND_C, 1.0, 1.0
    nsteps = np.full(B, 3, dtype=np.int32)
    nsteps[names.index("nosteps")] = 0
    return dict(states=st, nsteps=nsteps, truth=truth, course=course, cov=cov)


def check_hand_answers(out, model, what):
    """The answers worked out by hand.  On the sphere a displacement along the equator or a meridian is K km per degree; on
    WGS84 it is within the flattening (0.7 %) of that, and everything that is a count, a NaN, a row index or a NEES is the same."""
    i = {name: t for t, name in enumerate(HAND_SHIPS)}
    rt = 1e-12 if model == "sphere" else 7e-3
    near = lambda a, b: np.allclose(a, b, rtol=rt, atol=1e-9)  # noqa: E731
    off = K * np.array([0.5, 0.25, 0.125, 0.0625])
    t = i["equator"]
    assert near(out["err"][0, :, t], off) and near(out["cumerr"][0, :, t], np.cumsum(off)), what
    assert out["sum_err"][0, t] == out["cumerr"][0, 3, t] and near(out["sum_sq"][0, t], (off ** 2).sum()), what
    assert (out["n"][0, t], out["max_row"][0, t], out["nbroken"][0, t]) == (4, 0, 0) and out["max_err"][0, t] == out["err"][0, 0, t], what
    assert near(out["along"][0, :, t], off) and np.allclose(out["cross"][0, :, t], 0.0, atol=1e-9), what  # ahead on course 90
    qs = np.array([0.5, 0.25, 0.125, 0.0625]) ** 2 / HAND_A
    assert np.allclose(out["nees"][0, :, t], qs, rtol=1e-12) and out["nscored"][0, t] == 4, what
    assert out["ninside"][0, t] == int((qs <= LIMIT95).sum()) == 3 and np.isclose(out["sum_nees"][0, t], qs.sum(), rtol=1e-12), what
    for name, al, cr in (("north0", 1.0, 0.0), ("north90", 0.0, -1.0)):
        t = i[name]
        e = out["err"][0, :, t]
        assert near(e, K * 0.25) and out["n"][0, t] == 4 and out["ncoursed"][0, t] == 4, (what, name)
        assert np.allclose(out["along"][0, :, t], al * e, rtol=1e-12, atol=1e-9), (what, name)
        assert np.allclose(out["cross"][0, :, t], cr * e, rtol=1e-12, atol=1e-9), (what, name)
        assert np.allclose(out["nees"][0, :, t], 0.25 ** 2 / HAND_C, rtol=1e-12) and out["ninside"][0, t] == 0, (what, name)
    t = i["broken"]
    assert (out["n"][0, t], out["nbroken"][0, t], out["ncoursed"][0, t], out["nscored"][0, t]) == (3, 1, 3, 3), what
    for k in ("err", "along", "cross", "nees"):
        assert np.isnan(out[k][0, 2, t]) and not np.isnan(out[k][0, [0, 1, 3], t]).any(), (what, k)
    assert out["cumerr"][0, 2, t] == out["cumerr"][0, 1, t] and near(out["sum_err"][0, t], off[[0, 1, 3]].sum()), what
    t = i["untruthed"]
    assert (out["n"][0, t], out["nbroken"][0, t]) == (3, 0) and np.isnan(out["err"][0, 1, t]), what
    assert out["cumerr"][0, 1, t] == out["cumerr"][0, 0, t] and near(out["sum_err"][0, t], off[[0, 2, 3]].sum()), what
    t = i["tie"]
    assert out["err"][0, 0, t] == out["err"][0, 2, t] == out["max_err"][0, t] and out["max_row"][0, t] == 0, what
    t = i["nosteps"]
    assert (out["n"][0, t], out["max_row"][0, t]) == (1, 0) and near(out["sum_err"][0, t], off[0]), what
    assert out["cumerr"][0, 0, t] == out["sum_err"][0, t] and (out["err"][0, 1:, t] == SENTINEL).all(), what
    t = i["notruth"]
    assert (out["n"][0, t], out["max_row"][0, t], out["nbroken"][0, t], out["nscored"][0, t]) == (0, -1, 0, 0), what
    assert np.isnan(out["max_err"][0, t]) and out["sum_err"][0, t] == 0.0 and out["sum_sq"][0, t] == 0.0, what
    assert np.isnan(out["err"][0, :, t]).all() and (out["cumerr"][0, :, t] == 0.0).all(), what
    t = i["antimeridian"]
    assert near(out["err"][0, :, t], K * 0.2) and np.allclose(out["nees"][0, :, t], 0.2 ** 2 / HAND_A, rtol=1e-9), what
    assert near(out["along"][0, :, t], -K * 0.2) and np.allclose(out["cross"][0, :, t], 0.0, atol=1e-9), what  # west of it, course 90


# ---- the random fleet of the device comparison: S = 3, Nmax = 37, B = 70 (a full wave and a partial one) -----------------
FLEET_S, FLEET_N, FLEET_B, FLEET_SEED = 3, 37, 70, 11
FLEET_WIDE, FLEET_COLS = 150, (64, 134)  # the wider fleet of the window test and this fleet's columns in it


def fleet():
    """dict(states (3, 38, 4, 70), nsteps (every length 0 .. 37), truth (38, 2, 70), course (38, 70), cov16 (38, 16, 70), cov10).
    Three rows in five have truth: a base position displaced by 0.01 to 2.9 degrees in a random direction, while the samples'
    states lie within 0.004 degrees of the base in each coordinate, so every error is a displacement of 0.001 to 3 degrees;
    |lat| <= 66; tracks 0 .. 5 lie within a few degrees of the antimeridian, unwrapped.  One truthed row in six has no
    course.  The covariances are random symmetric positive definite 4 x 4 matrices with position entries of the order of the
    displacements squared, so that q lies on both sides of the limit."""
    if "fleet" in _CACHE:
        return _CACHE["fleet"]
    rng = np.random.default_rng(FLEET_SEED)
    S, N, B = FLEET_S, FLEET_N, FLEET_B
    lon0 = rng.uniform(-170.0, 170.0, B)
    lon0[:6] = 178.0 + rng.uniform(0.0, 1.0, 6)
    lat0 = rng.uniform(-55.0, 55.0, B)
    steps = rng.normal(0.0, 0.15, (N, 2, B))
    base = np.concatenate([np.stack([lon0, lat0])[None], np.stack([lon0, lat0])[None] + np.cumsum(steps, axis=0)])  # (N+1, 2, B)
    st = np.zeros((S, N + 1, 4, B))
    st[:, :, :2] = base[None] + rng.uniform(-0.004, 0.004, (S, N + 1, 2, B))
    st[:, :, 2:] = rng.normal(0.0, 1.0, (S, N + 1, 2, B))  # speed and heading: not read
    r, ang = np.exp(rng.uniform(np.log(0.01), np.log(2.9), (N + 1, B))), rng.uniform(0.0, 2.0 * np.pi, (N + 1, B))
    truth = base + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    truth[:, 0] = np.where(np.arange(B)[None] < 3, wrap180(truth[:, 0]), truth[:, 0])  # three of the six wrapped, three not
    truth = np.ascontiguousarray(np.where((rng.uniform(size=(N + 1, B)) < 0.4)[:, None], np.nan, truth))
    course = rng.uniform(0.0, 360.0, (N + 1, B))
    course[rng.uniform(size=(N + 1, B)) < 1.0 / 6.0] = np.nan
    A = rng.normal(0.0, 1.0, (N + 1, B, 4, 4))
    P = np.einsum("kbij,kblj->kbil", A, A) * (r[..., None, None] ** 2) * 0.06
    cov16 = np.ascontiguousarray(P.reshape(N + 1, B, 16).transpose(0, 2, 1))
    cov10 = np.ascontiguousarray(cov16[:, [0, 1, 2, 3, 5, 6, 7, 10, 11, 15]])
    nsteps = (np.arange(B) % (N + 1)).astype(np.int32)
    _CACHE["fleet"] = dict(states=st, nsteps=nsteps, truth=truth, course=course, cov16=cov16, cov10=cov10)
    return _CACHE["fleet"]


def fleet_reference(model, sample0_cov=False):
    """The restatement on the fleet, computed once: all samples with the course, or (``sample0_cov``) sample 0 with course and
    covariance."""
    key = ("ref", model, sample0_cov)
    if key not in _CACHE:
        f = fleet()
        if sample0_cov:
            _CACHE[key] = track_errors(f["states"][:1], f["nsteps"], f["truth"], model, f["course"], f["cov16"])
        else:
            _CACHE[key] = track_errors(f["states"], f["nsteps"], f["truth"], model, f["course"])
    return _CACHE[key]


def faulty_fleet():
    """Sample 0 of the fleet with injected faults, each in a row at or below its track's nsteps that has truth: NaN and inf in
    the states (broken rows), NaN and inf in the truth (rows without truth), NaN and inf in the course (rows without a course),
    NaN and inf in the covariance, a covariance with det < 0, det == 0, and a <= 0 (rows that are not scored).  Returns
    (dict like ``fleet`` with S = 1, the list of (kind, row, track))."""
    f = {k: v.copy() for k, v in fleet().items()}
    f["states"] = f["states"][:1].copy()
    have = np.isfinite(f["truth"][:, 0]) & np.isfinite(f["course"]) & (np.arange(FLEET_N + 1)[:, None] <= f["nsteps"][None])
    spots = np.argwhere(have)
    rng = np.random.default_rng(FLEET_SEED + 1)
    tracks = rng.choice(np.unique(spots[:, 1]), 13, replace=False)  # one fault to a track
    pick = [spots[spots[:, 1] == t][rng.integers((spots[:, 1] == t).sum())] for t in tracks]
    kinds = ("state_nan", "state_inf", "state_lat_nan", "truth_nan", "truth_inf", "course_nan", "course_inf", "cov_nan", "cov_inf",
             "cov_b_nan", "det_negative", "det_zero", "a_negative")
    done = []
    for kind, (k, t) in zip(kinds, pick):
        if kind == "state_nan":
            f["states"][0, k, 0, t] = np.nan
        elif kind == "state_inf":
            f["states"][0, k, 0, t] = np.inf
        elif kind == "state_lat_nan":
            f["states"][0, k, 1, t] = np.nan
        elif kind == "truth_nan":
            f["truth"][k, 1, t] = np.nan
        elif kind == "truth_inf":
            f["truth"][k, 0, t] = -np.inf
        elif kind == "course_nan":
            f["course"][k, t] = np.nan
        elif kind == "course_inf":
            f["course"][k, t] = np.inf
        elif kind == "cov_nan":
            f["cov16"][k, 0, t] = np.nan
        elif kind == "cov_inf":
            f["cov16"][k, 5, t] = np.inf
        elif kind == "cov_b_nan":
            f["cov16"][k, 1, t] = np.nan
        elif kind == "det_negative":
            f["cov16"][k, 1, t] = 2.0 * np.sqrt(f["cov16"][k, 0, t] * f["cov16"][k, 5, t])
        elif kind == "det_zero":
            f["cov16"][k, 0, t], f["cov16"][k, 1, t], f["cov16"][k, 5, t] = 4.0, 2.0, 1.0
        elif kind == "a_negative":
            f["cov16"][k, 0, t], f["cov16"][k, 5, t] = -f["cov16"][k, 0, t], -f["cov16"][k, 5, t]
        done.append((kind, int(k), int(t)))
    f["cov10"] = np.ascontiguousarray(f["cov16"][:, [0, 1, 2, 3, 5, 6, 7, 10, 11, 15]])
    return f, done
