"""NumPy restatement of the speeds of tracks (include/ste.h: ste_speed_f64, ste_speed_metrics_f64; DESIGN.md, "Speeds") and the
small fleets its tests share.

For track t of sample s, with ns = nsteps[t], rows 0 .. ns of (lon, lat) and the steps' dt:
    clock            T_0 = 0, T_{k+1} = T_k + dt_k in order; a dt_k, k < ns, that is not finite or is negative makes the clock bad
    step k           examined when dt_k > 0, else skipped; L_k = path_metrics_cases.leg_km(row k, row k+1), v_k = L_k / dt_k;
                     broken when v_k is not finite, else sound
    sums             dist and sound_time add L_k and dt_k over the sound steps
    maximum          the first sound step with the largest v_k: vmax and vmax_time = T_k
    bands            j = (number of edges <= v_k) - 1; dt_k goes to band j when 0 <= j < nbands
    runs             a sound step qualifies when v_k <= thr (>= with ``above``); consecutive qualifying steps form a run, closed by
                     anything else and by the end of the track; a run of length >= min_run_h counts (nruns, run_time, first_run),
                     the longest run of all (the first of equal ones) gives longest and longest_start
    bad              a bad clock, or with a threshold a bad one (not finite, negative): NaN for vmax, vmax_time, first_run,
                     longest_start and the speed rows below ns, zero for the rest
"""
import numpy as np
import path_metrics_cases as pmc

BAD_TIME, BAD_LIMIT = 0x1, 0x2
SENTINEL = -12345.0  # what the speed rows past nsteps hold: the call leaves them alone
FLOAT_OUTPUTS = ("dist", "sound_time", "vmax", "vmax_time", "cond_time", "run_time", "first_run", "longest", "longest_start")
INT_OUTPUTS = ("nruns", "nbroken")
RUN_OUTPUTS = ("cond_time", "run_time", "first_run", "longest", "longest_start", "nruns")
NAN_WHEN_BAD = ("vmax", "vmax_time", "first_run", "longest_start")
LEG_DERIVED = ("speed", "dist", "vmax")  # compared within pmc.DIST_RTOL / DIST_ATOL; everything else bit for bit
K = pmc.KM_PER_DEG_EQUATOR
_CACHE = {}


def _leg(model, lon1, lat1, lon2, lat2):
    """pmc.leg_km, NaN for a coordinate that is not finite; a leg is worked out once however many cases share it."""
    if not np.isfinite(lon1 + lat1 + lon2 + lat2):
        return np.nan
    key = ("leg", model, float(lon1), float(lat1), float(lon2), float(lat2))
    if key not in _CACHE:
        _CACHE[key] = pmc.leg_km(model, lon1, lat1, lon2, lat2)
    return _CACHE[key]


def speed_metrics(states, nsteps, dt, model="sphere", edges=None, threshold=None, above=False, min_run_h=0.0):
    """``states`` (S, N+1, 4, B), ``nsteps`` (B,), ``dt`` (N, B), ``edges`` (nbands+1,) or None, ``threshold`` None, a scalar or
    (B,) -> dict of every output of the call (speed (S, N, B) with SENTINEL past nsteps, band_time (S, nbands, B), the run
    outputs only with a threshold), plus ``run_lengths``: the length of every run that was closed, for the conditions test."""
    states = np.asarray(states, dtype=np.float64)
    S, rows, _, B = states.shape
    N = rows - 1
    edges = None if edges is None else np.asarray(edges, dtype=np.float64)
    nb = 0 if edges is None else len(edges) - 1
    runs = threshold is not None
    thr_all = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (B,)) if runs else None
    out = {k: np.zeros((S, B)) for k in FLOAT_OUTPUTS}
    out.update({k: np.zeros((S, B), dtype=np.int32) for k in INT_OUTPUTS})
    out["speed"] = np.full((S, N, B), SENTINEL)
    out["band_time"] = np.zeros((S, nb, B))
    out["track_status"] = np.zeros((B,), dtype=np.int32)
    lengths = []
    for t in range(B):
        ns = int(nsteps[t])
        d = dt[:ns, t]
        status = 0 if all(np.isfinite(x) and x >= 0.0 for x in d) else BAD_TIME
        thr = thr_all[t] if runs else 0.0
        if runs and not (np.isfinite(thr) and thr >= 0.0):
            status |= BAD_LIMIT
        out["track_status"][t] = status
        for s in range(S):
            if status:
                for k in NAN_WHEN_BAD:
                    out[k][s, t] = np.nan
                out["speed"][s, :ns, t] = np.nan
                continue
            lon, lat = states[s, :, 0, t], states[s, :, 1, t]
            T = dist = sound = cond = run_time = longest = 0.0
            vmax, vmax_time, first, lstart = -np.inf, np.nan, np.nan, np.nan
            nruns = nbroken = 0
            run = None  # an open run: [length, start]

            def close():
                nonlocal run, nruns, run_time, first, longest, lstart
                length, start = run
                lengths.append(length)
                if length >= min_run_h:
                    if nruns == 0:
                        first = start
                    nruns += 1
                    run_time = run_time + length
                if length > longest:
                    longest, lstart = length, start
                run = None

            for k in range(ns):
                dk = d[k]
                v, qual = np.nan, False
                if dk > 0.0:
                    L = _leg(model, lon[k], lat[k], lon[k + 1], lat[k + 1])
                    with np.errstate(over="ignore"):
                        v = L / dk
                    if np.isfinite(v):
                        dist = dist + L
                        sound = sound + dk
                        if v > vmax:
                            vmax, vmax_time = v, T
                        if nb:
                            j = int((edges <= v).sum()) - 1
                            if 0 <= j < nb:
                                out["band_time"][s, j, t] += dk
                        qual = runs and (v >= thr if above else v <= thr)
                    else:
                        nbroken += 1
                        v = np.nan
                out["speed"][s, k, t] = v
                if qual:
                    cond = cond + dk
                    if run is None:
                        run = [dk, T]
                    else:
                        run[0] = run[0] + dk
                elif run is not None:
                    close()
                T = T + dk
            if run is not None:
                close()
            vals = dict(dist=dist, sound_time=sound, vmax=vmax if vmax >= 0.0 else np.nan, vmax_time=vmax_time, cond_time=cond,
                        run_time=run_time, first_run=first, longest=longest, longest_start=lstart, nruns=nruns, nbroken=nbroken)
            for k, x in vals.items():
                out[k][s, t] = x
    if not runs:
        for k in RUN_OUTPUTS:
            del out[k]
    out["run_lengths"] = np.asarray(lengths)
    return out


# ---- the hand-made ships: one-degree legs along the equator (K km each, for either leg function), six steps ------------------
HAND_SHIPS = ("paces", "never moves", "faults", "negative dt", "no limit", "no steps", "two steps")
HAND_EDGES = np.array([0.0, 0.3 * K, 0.75 * K, 1.5 * K, 3.0 * K])
HAND_MIN_RUN_H = 1.0


def hand_batch():
    """dict(states (1, 7, 4, 7), nsteps, dt (6, 7), threshold (7,)): HAND_SHIPS in this order.
    paces        dt 1 1 2 4 4 0.5: speeds K K K/2 K/4 K/4 2K; threshold 0.6 K
    never moves  one position, dt 1 .. 6; threshold 0
    faults       dt 1 0 2 1 1 4 and a NaN latitude in row 4: step 1 skipped, steps 3 and 4 broken, speeds K, K/2, K/4;
                 threshold 2 K
    negative dt  dt 1 -1 1 1 1 1: a bad clock
    no limit     the paces with a NaN threshold: a bad limit where runs are asked for, the paces where they are not
    no steps     nsteps 0
    two steps    nsteps 2 of six: a NaN dt and rows of NaN past them are not read; dt 2 4, threshold 0.6 K
    No two sound steps of a ship that decide its maximum have the same nominal speed: only exact zeros tie."""
    N, B = 6, len(HAND_SHIPS)
    tracks = [pmc.equator_track(N, lon0=10.0 * b) for b in range(B)]
    tracks[1][:] = tracks[1][0]
    tracks[4][:] = tracks[0]
    tracks[2][4, 1] = np.nan
    tracks[6][3:] = np.nan
    dt = np.ones((N, B))
    dt[:, 0] = dt[:, 4] = (1.0, 1.0, 2.0, 4.0, 4.0, 0.5)
    dt[:, 1] = np.arange(1.0, N + 1.0)
    dt[:, 2] = (1.0, 0.0, 2.0, 1.0, 1.0, 4.0)
    dt[1, 3] = -1.0
    dt[:, 6] = (2.0, 4.0, np.nan, -3.0, 1.0, 1.0)
    nsteps = np.array([N, N, N, N, N, 0, 2], dtype=np.int32)
    thr = np.array([0.6 * K, 0.0, 2.0 * K, K, np.nan, K, 0.6 * K])
    return dict(states=pmc.states_of(tracks), nsteps=nsteps, dt=dt, threshold=thr)


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = np.isnan(want) | (np.abs(got - want) <= pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(want))
    assert ok.all(), (what, got, want)


def _same(got, want, what):
    got = np.asarray(got)
    want = np.asarray(want).astype(got.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), (what, got, want)


def check_hand_answers(res, what, above):
    """What the seven ships give for HAND_EDGES, their thresholds and HAND_MIN_RUN_H, known by inspection: times, counts and
    status exactly, leg-derived values within the leg's tolerance.  ``res``: the outputs for sample 0, run outputs included."""
    nan = np.nan
    r = {k: (v[0] if k != "track_status" else v) for k, v in res.items() if k != "run_lengths"}
    _same(r["track_status"], [0, 0, 0, BAD_TIME, BAD_LIMIT, 0, 0], (what, "track_status"))
    _same(r["nbroken"], [0, 0, 2, 0, 0, 0, 0], (what, "nbroken"))
    _same(r["sound_time"], [12.5, 21.0, 7.0, 0.0, 0.0, 0.0, 6.0], (what, "sound_time"))
    _close(r["dist"], [6 * K, 0.0, 3 * K, 0.0, 0.0, 0.0, 2 * K], (what, "dist"))
    _close(r["vmax"], [2 * K, 0.0, K, nan, nan, nan, K / 2], (what, "vmax"))
    _same(r["vmax_time"], [12.0, 0.0, 0.0, nan, nan, nan, 0.0], (what, "vmax_time"))  # the first step wins a tie
    assert r["vmax"][1] == 0.0 and r["dist"][1] == 0.0
    speed = np.full((6, 7), SENTINEL)
    speed[:, 0] = (K, K, K / 2, K / 4, K / 4, 2 * K)
    speed[:, 1] = 0.0
    speed[:, 2] = (K, nan, K / 2, nan, nan, K / 4)
    speed[:, 3] = speed[:, 4] = nan
    speed[:2, 6] = (K / 2, K / 4)
    _close(r["speed"], speed, (what, "speed"))
    bands = np.zeros((4, 7))
    bands[:, 0] = (8.0, 2.0, 2.0, 0.5)
    bands[0, 1] = 21.0  # v == edges[0] == 0 is in band 0
    bands[:3, 2] = (4.0, 2.0, 1.0)
    bands[:2, 6] = (4.0, 2.0)
    _same(r["band_time"], bands, (what, "band_time"))
    if above:  # paces: steps 0, 1 (2 h from 0) and step 5 (0.5 h from 12, below min_run_h); never moves: 0 >= 0; faults: none
        _same(r["cond_time"], [2.5, 21.0, 0.0, 0.0, 0.0, 0.0, 0.0], (what, "cond_time"))
        _same(r["run_time"], [2.0, 21.0, 0.0, 0.0, 0.0, 0.0, 0.0], (what, "run_time"))
        _same(r["nruns"], [1, 1, 0, 0, 0, 0, 0], (what, "nruns"))
        _same(r["first_run"], [0.0, 0.0, nan, nan, nan, nan, nan], (what, "first_run"))
        _same(r["longest"], [2.0, 21.0, 0.0, 0.0, 0.0, 0.0, 0.0], (what, "longest"))
        _same(r["longest_start"], [0.0, 0.0, nan, nan, nan, nan, nan], (what, "longest_start"))
    else:  # paces: steps 2, 3, 4 (10 h from 2); never moves: the whole track; faults: runs of 1, 2 and 4 hours from 0, 1 and 5
        _same(r["cond_time"], [10.0, 21.0, 7.0, 0.0, 0.0, 0.0, 6.0], (what, "cond_time"))
        _same(r["run_time"], [10.0, 21.0, 7.0, 0.0, 0.0, 0.0, 6.0], (what, "run_time"))
        _same(r["nruns"], [1, 1, 3, 0, 0, 0, 1], (what, "nruns"))
        _same(r["first_run"], [2.0, 0.0, 0.0, nan, nan, nan, 0.0], (what, "first_run"))
        _same(r["longest"], [10.0, 21.0, 4.0, 0.0, 0.0, 0.0, 6.0], (what, "longest"))
        _same(r["longest_start"], [2.0, 0.0, 5.0, nan, nan, nan, 0.0], (what, "longest_start"))


# ---- the random-walk fleet of path_metrics_cases with band edges and thresholds in the gaps of its own speeds ----------------
WALK_MIN_RUN_H = 1.0
WALK_BANDS = (0, 1, 5, 32)
GAP_RTOL = 1e-6  # no speed may lie this close (relative) to an edge or to its track's threshold


def _widest_gap(u, lo, hi):
    """The midpoint of the widest relative gap between neighbours of the sorted array ``u`` with indices in [lo, hi)."""
    lo, hi = max(lo, 0), min(hi, len(u) - 1)
    i = lo + int(np.argmax((u[lo + 1:hi + 1] - u[lo:hi]) / u[lo + 1:hi + 1]))
    return 0.5 * (u[i] + u[i + 1])


def walk_speeds(model):
    """The restatement on the walk fleet without bands or a threshold: the speeds the edges and thresholds are placed between."""
    key = ("speeds", model)
    if key not in _CACHE:
        w = pmc.walk()
        _CACHE[key] = speed_metrics(w["states"], w["nsteps"], w["dt"], model)
    return _CACHE[key]


def walk_edges(model, nbands):
    """nbands + 1 edges at the 5 % .. 95 % quantiles of the fleet's speeds, each moved to the middle of the widest gap among the
    twenty speeds on either side: some speeds lie below the first edge and some above the last."""
    if nbands == 0:
        return None
    v = walk_speeds(model)["speed"]
    u = np.unique(v[v != SENTINEL])
    at = np.round(np.linspace(0.05, 0.95, nbands + 1) * (len(u) - 1)).astype(int)
    return np.array([_widest_gap(u, i - 20, i + 20) for i in at])


def walk_thresholds(model):
    """One threshold per track: the middle of the widest gap in the middle half of that track's speeds over all samples (1 km/h
    for the tracks without a step)."""
    v = walk_speeds(model)["speed"]
    B = v.shape[2]
    thr = np.ones((B,))
    for t in range(B):
        u = np.unique(v[:, :, t][v[:, :, t] != SENTINEL])
        if len(u) > 1:
            thr[t] = _widest_gap(u, len(u) // 4, max(3 * len(u) // 4, len(u) // 4 + 1))
    return thr


def walk_reference(model, nbands, above):
    """The restatement on the walk fleet, computed once per (model, nbands, above)."""
    key = ("ref", model, nbands, above)
    if key not in _CACHE:
        w = pmc.walk()
        _CACHE[key] = speed_metrics(w["states"], w["nsteps"], w["dt"], model, walk_edges(model, nbands), walk_thresholds(model), above,
                                    WALK_MIN_RUN_H)
    return _CACHE[key]


def faulty_walk():
    """A copy of the walk fleet with faults: zero dt in the middle of four tracks, NaN coordinates in five rows (one of them row 0,
    one the last row read), one negative dt (track 17, step 3 of its 8) and one NaN threshold (track 26).  -> (fleet, threshold
    factors): the thresholds of a model are walk_thresholds(model) times the factors."""
    if "faulty" not in _CACHE:
        w = {k: np.array(v, copy=True) for k, v in pmc.walk().items()}
        ns = w["nsteps"]
        assert ns[17] == 8 and ns[26] == 8 and ns[35] == 8
        for t, k in ((8, 2), (16, 0), (44, 5), (35, 7)):
            assert k < ns[t]
            w["dt"][k, t] = 0.0
        for s, t, row, c in ((0, 7, 3, 0), (2, 25, 0, 1), (4, 34, 7, 1), (1, 53, 8, 0), (3, 62, 4, 1)):
            assert row <= ns[t]
            w["states"][s, row, c, t] = np.nan
        w["dt"][3, 17] = -0.5
        factor = np.ones((pmc.WALK_B,))
        factor[26] = np.nan
        _CACHE["faulty"] = (w, factor)
    return _CACHE["faulty"]
