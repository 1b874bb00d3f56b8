"""Pairs of tracks on the device against each other (include/ste.h: ste_encounter_f64, ste_encounter_metrics_f64; DESIGN.md,
"Encounters"): declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers, the
conditions of the meeting fleet that the device comparison rests on, and the candidate pairs (CPU); on the GPU the hand-made
tracks for both leg functions, the meeting fleet against the restatement, independence of the surroundings bit for bit,
reversed pairs, the Python front ends on a real run, and the refusals on the device build."""
import ctypes as C
import os
import re

import encounter_cases as enc
import numpy as np
import path_metrics_cases as pmc
import pytest
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "npairs", "pairs", "t0", "radius_km", "flags", "reserved", "min_dist", "min_time",
          "time_within", "first_within", "nwithin", "overlap", "nbroken", "status"]
OUTPUTS = FIELDS[9:]
PER_SAMPLE = enc.FLOAT_OUTPUTS + enc.INT_OUTPUTS


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_encounter_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_encounter_f64\* en, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_encounter_f64 {"): hdr.index("} ste_encounter_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteEncounterF64._fields_] == FIELDS
    # the layout of the C struct by hand: two 32-bit integers share a word, every pointer, double and int64 takes one
    offsets = {"nstates": 0, "model": 4, "states": 8, "npairs": 16, "pairs": 24, "t0": 32, "radius_km": 40, "flags": 48,
               "reserved": 52}
    offsets.update({name: 56 + 8 * k for k, name in enumerate(OUTPUTS)})
    assert {f: getattr(binding.SteEncounterF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteEncounterF64) == 120
    assert "ste_encounter_metrics_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_encounter_metrics_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the encounter arguments travel beside the batch
    assert re.search(r"#define STE_ENCOUNTER_MAX_PAIRS \(1 << 26\)", hdr) and binding.STE_ENCOUNTER_MAX_PAIRS == 1 << 26
    assert float(re.search(r"#define STE_ENCOUNTER_MAX_RADIUS_KM ([\d.]+)", hdr).group(1)) == binding.STE_ENCOUNTER_MAX_RADIUS_KM == 1000.0
    assert int(re.search(r"#define STE_ENC_BAD_INDEX 0x(\d+)", hdr).group(1), 16) == binding.STE_ENC_BAD_INDEX == enc.BAD_INDEX == 1
    assert int(re.search(r"#define STE_ENC_BAD_TIME +0x(\d+)", hdr).group(1), 16) == binding.STE_ENC_BAD_TIME == enc.BAD_TIME == 2
    comment = hdr[hdr.index("ENCOUNTERS:"): hdr.index("#define STE_ENCOUNTER_MAX_PAIRS")]
    for word in ("Clock.", "Walk.", "Bad clock.", "Bad index.", "Soundness.", "Positions in a piece.", "Relative motion.",
                 "Closest approach.", "Within R", "Overlap.", "Accuracy.", "PIECE", "BROKEN", "RUN", "wrap180", "clamp01",
                 "1.6e-3", "re-wrapped", "first piece wins a tie"):
        assert word in comment, word


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The pointers below are not memory: nothing may be launched, with a GPU or without one."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.dt, s.nsteps = 0x1000, 0x2000
        return s

    def good_enc():
        e = binding.SteEncounterF64()
        e.nstates, e.model, e.states, e.npairs, e.pairs, e.t0 = 3, binding.STE_PREP_WGS84, 0x3000, 5, 0x4000, 0x5000
        e.radius_km, e.flags, e.reserved = 30.0, 0, 0
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x6000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_enc()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc = lib.ste_encounter_metrics_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_encounter_metrics_f64" in msg, (fields, rc, msg)

    for s, e, reason in ((None, good_enc(), "batch pointer is NULL"), (good_batch(), None, "encounter arguments (en) are NULL")):
        assert lib.ste_encounter_metrics_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_encounter_metrics_f64" in msg
    refused("en->states is required", states=None)
    refused("en->pairs is required", pairs=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1, (1 << 26) + 1, 1 << 40):
        refused("between 1 and STE_ENCOUNTER_MAX_PAIRS", npairs=n)
    for m in (-1, 2, 7):
        refused("STE_PREP_SPHERE or STE_PREP_WGS84 when min_dist is asked for", model=m)
    for r in (float("nan"), float("inf"), -float("inf"), -1e-300, -5.0, 1000.0000000000001, 1e9):
        refused("radius_km must be finite and between 0 and STE_ENCOUNTER_MAX_RADIUS_KM", radius_km=r)
    for f in (1, 0x80000000):
        refused("en->flags must be 0", flags=f)
        refused("en->reserved must be 0", reserved=f)
    refused("batch's dt is required", dt=None)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_hand_answers():
    """Sixteen hand-made ships, R = 30 km (encounter_cases.HAND_PAIRS names the pairs): a meeting mid-step on the equator
    (distance 0 at 2.5 h, R / 111.3 h within), parallel courses 0.1 degrees apart on different dt grids and t0 (time_within
    equals overlap bit for bit), a zigzag past a stationary ship with a pause beside it and one away from it (two runs, dd ==
    0 on either side of R), a pair astride the antimeridian with one ship stored wrapped, clocks that never overlap, a NaN
    latitude that breaks two pieces and splits the run, i == j, nsteps 0 and 1, a NaN and a negative dt met by the walk (and
    a NaN dt the walk never meets), a NaN t0, and indices outside [0, B)."""
    h = enc.hand_batch()
    for model in ("sphere", "wgs84"):
        r = enc.encounter_metrics(h["states"], h["nsteps"], h["dt"], h["pairs"], enc.HAND_R, h["t0"], model)
        if model == "sphere":
            enc.check_hand_answers(r, "restatement, sphere")
        else:  # the same but for the ellipsoid's equator and meridian scales
            s = enc.encounter_metrics(h["states"], h["nsteps"], h["dt"], h["pairs"], enc.HAND_R, h["t0"], "sphere")
            for k in PER_SAMPLE[1:] + ("status",):
                assert np.array_equal(_u64(r[k].astype(np.float64)), _u64(s[k].astype(np.float64))), k
            both = np.isfinite(s["min_dist"])
            assert np.array_equal(both, np.isfinite(r["min_dist"]))
            assert np.allclose(r["min_dist"][both], s["min_dist"][both], rtol=7e-3, atol=0.0)
    # R = 0: only coincident ships are within
    r0 = enc.encounter_metrics(h["states"], h["nsteps"], h["dt"], h["pairs"], 0.0, h["t0"])
    names = h["names"]
    assert r0["nwithin"][0].tolist() == [1 if n in ("same ship", "one step") else 0 for n in names]
    assert r0["time_within"][0, names.index("same ship")] == r0["overlap"][0, names.index("same ship")]


def test_conditions_of_the_meeting_fleet():
    """The restatement alone on all five samples of the meeting fleet: what the device comparison assumes of it.  At most 2 %
    of the (sample, pair) values are near ties (runner-up q <= best q (1 + 1e-9): min_time may come from either piece) and at
    most 1 % graze R (|sqrt(best q) - R| < 1e-9 R: a rounding decides nwithin); at least 15 pairs come within R and at least 20
    have no sound piece in sample 0; every kind of row is there."""
    w, ref = enc.fleet(), enc.fleet_reference()
    S, P = enc.FLEET_S, enc.FLEET_P
    assert w["states"].shape == (S, enc.FLEET_N + 1, 4, enc.FLEET_B) and w["pairs"].shape == (P, 2) and P == 2 * 64 + 2
    assert set(w["nsteps"][8:].tolist()) == set(range(9)) and (w["nsteps"][:8] == enc.FLEET_N).all()
    assert (np.abs(w["states"][:, :, 0, :4]) <= 180.0).all() and (w["states"][:, :, 0, 4:8] > 180.0).any()
    tie, graze = enc.near_tie(ref), enc.grazing(ref, enc.FLEET_R)
    found = np.isfinite(ref["min_dist"])
    within, none = int((ref["nwithin"][0] > 0).sum()), int((~found[0]).sum())
    d = ref["min_dist"][found]
    print(f"meeting fleet: {int(found[0].sum())} pairs of sample 0 with sound pieces, {none} without, {within} within R; "
          f"min_dist {d.min():.3g} .. {d.max():.3g} km; near ties {int(tie.sum())} and grazing {int(graze.sum())} of {S * P}; "
          f"runs: {np.bincount(ref['nwithin'].ravel()).tolist()}; pieces per pair up to {int(ref['npieces'].max())}")
    assert tie.mean() <= 0.02 and graze.mean() <= 0.01
    assert within >= 15 and none >= 20
    assert not ref["status"].any() and not ref["nbroken"].any()
    assert (ref["nwithin"] > 1).any(), "no pair leaves R and comes back"
    planar = np.sqrt(ref["best_q"][found])
    far = d > 1.0
    assert np.abs(planar[far] / d[far] - 1.0).max() < 1.6e-3  # the accuracy note of the header
    assert ref["min_dist"][0, P - 6] == 0.0 or np.isnan(ref["min_dist"][0, P - 6])  # the (i, i) pair


def test_candidate_pairs_hold_every_encounter():
    """batch.candidate_pairs (the tensor core of encounter_candidates) on the CPU, on sample 0 of the meeting fleet as the
    smoothed track: sorted by (i, j), i < j, no duplicates, no track without steps, no pair between the two groups, and every
    pair (of all B (B - 1) / 2) that the restatement brings within R is there.  Blocks of 16 rows give the same list."""
    import torch
    from track_estimators import batch

    w = enc.fleet()
    B = enc.FLEET_B
    mean = torch.from_numpy(w["states"][0].copy())
    args = (mean, torch.from_numpy(w["nsteps"]), torch.from_numpy(w["dt"]), enc.FLEET_R)
    cand = batch.candidate_pairs(*args, t0=torch.from_numpy(w["t0"]))
    assert cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[1] == 2
    c = cand.numpy().astype(np.int64)
    key = c[:, 0] * B + c[:, 1]
    assert (c[:, 0] < c[:, 1]).all() and (np.diff(key) > 0).all() and c.min() >= 0 and c.max() < B
    assert (w["nsteps"][c] > 0).all() and ((c[:, 0] < 8) == (c[:, 1] < 8)).all()
    assert torch.equal(cand, batch.candidate_pairs(*args, t0=torch.from_numpy(w["t0"]), chunk=16))
    every = np.array([(i, j) for i in range(B) for j in range(i + 1, B)], dtype=np.int32)
    ref = enc.encounter_metrics(w["states"][:1], w["nsteps"], w["dt"], every, enc.FLEET_R, w["t0"])
    met = every[ref["nwithin"][0] > 0].astype(np.int64)
    assert len(met) >= 100 and np.isin(met[:, 0] * B + met[:, 1], key).all()
    assert len(c) < len(every)  # and it does prune
    # a NaN row, a NaN t0 and disjoint clocks pair with nothing
    st = w["states"][0].copy()
    st[1, 1, 20] = np.nan
    t0 = w["t0"].copy()
    t0[30], t0[40] = np.nan, 1000.0
    pruned = batch.candidate_pairs(torch.from_numpy(st), *args[1:], t0=torch.from_numpy(t0)).numpy()
    assert not np.isin(pruned, (20, 30, 40)).any() and len(pruned) > 0


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _abi_call(db, states, pairs, radius_km, t0, model="sphere", want=OUTPUTS, batch_struct=None):
    """ste_encounter_metrics_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor; ``want``: the outputs asked for
    (the others are NULL); -> dict of NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    S, P = int(states.shape[0]), len(pairs)
    pr = _dev(db, np.asarray(pairs, dtype=np.int32))
    clock = None if t0 is None else _dev(db, np.asarray(t0, dtype=np.float64))
    out = {}
    en = binding.SteEncounterF64()
    en.nstates, en.model, en.states = S, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model], states.data_ptr()
    en.npairs, en.pairs, en.t0, en.radius_km = P, pr.data_ptr(), None if clock is None else clock.data_ptr(), radius_km
    for k in want:
        dtype = torch.int32 if k in ("nwithin", "nbroken", "status") else torch.float64
        out[k] = torch.empty((P,) if k == "status" else (S, P), dtype=dtype, device=db.device)
        setattr(en, k, out[k].data_ptr())
    s = db.struct if batch_struct is None else batch_struct
    binding.check(db.lib.ste_encounter_metrics_f64(C.byref(s), C.byref(en), db._stream(None)), "ste_encounter_metrics_f64")
    torch.cuda.synchronize()
    return _host(out)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_hand_made_tracks_on_the_device(model):
    """The sixteen hand-made ships through the C ABI: the known answers (sphere), and the restatement for either model."""
    from track_estimators import batch

    h = enc.hand_batch()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    got = _abi_call(db, _dev(db, h["states"]), h["pairs"], enc.HAND_R, h["t0"], model)
    if model == "sphere":
        enc.check_hand_answers(got, "device, sphere")
    ref = enc.encounter_metrics(h["states"], h["nsteps"], h["dt"], h["pairs"], enc.HAND_R, h["t0"], model)
    # the planted NaN (dt, t0) and the indices outside [0, B) belong to pairs that have no time to compare
    span = enc.clock_span(h["nsteps"], np.nan_to_num(h["dt"]), np.nan_to_num(h["t0"]), np.clip(h["pairs"], 0, enc.HAND_B - 1))
    _compare(got, ref, span, enc.HAND_R, f"hand-made tracks, {model}")


def _compare(got, ref, span, radius_km, what):
    """The device against the restatement: integers and status equal (nwithin outside the grazing set), overlap bit for bit,
    NaN patterns identical, min_dist within pmc.DIST_RTOL / DIST_ATOL, the times within pmc.TIME_RTOL of the pair's clock span
    (min_time outside the near-tie set).  Returns the largest deviations as fractions of their tolerances."""
    graze = enc.grazing(ref, radius_km)
    tie = enc.near_tie(ref)
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], ref["status"]), (what, "status")
    assert got["nbroken"].dtype == np.int32 and np.array_equal(got["nbroken"], ref["nbroken"]), (what, "nbroken")
    assert got["nwithin"].dtype == np.int32 and np.array_equal(got["nwithin"][~graze], ref["nwithin"][~graze]), (what, "nwithin")
    assert np.array_equal(_u64(got["overlap"]), _u64(ref["overlap"])), (what, "overlap")
    worst = {}
    for k in ("min_dist", "min_time", "time_within", "first_within"):
        assert got[k].dtype == np.float64
        skip = graze if k in ("time_within", "first_within") else (tie if k == "min_time" else np.zeros_like(graze))
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k])[~skip], nan[~skip]), (what, k, "NaN pattern")
        use = ~nan & ~skip
        err = np.abs(got[k] - ref[k])
        tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref[k]) if k == "min_dist" else np.broadcast_to(pmc.TIME_RTOL * span, err.shape)
        frac = err[use] / tol[use]
        worst[k] = float(frac.max()) if frac.size else 0.0
        at = np.unravel_index(np.argmax(np.where(use, err / tol, 0.0)), err.shape)
        print(f"{what}: {k} deviates by at most {worst[k]:.3g} of its tolerance ({int(use.sum())} values); worst at {tuple(int(v) for v in at)}: "
              f"{got[k][at]!r} against {ref[k][at]!r}")
        assert worst[k] <= 1.0, (what, k, worst[k], np.argwhere(use & (err > tol))[:5].tolist())
        if k == "min_dist":
            worst["min_dist_km"] = float(err[use].max()) if frac.size else 0.0
    return worst


def _fleet_batch():
    from track_estimators import batch

    w = enc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_meeting_fleet_against_the_restatement(model):
    """S = 5, Nmax = 8, B = 70, P = 130 (two waves plus two lanes), R = 30 km: integers and status equal, overlap bit for bit,
    NaN patterns identical, min_dist within 1e-10 relative, times within 1e-12 of the pair's clock span; NaN in the rows past
    nsteps changes nothing.  Largest deviations measured on an MI355X, as fractions of their tolerances: min_dist 4.0e-6
    (sphere), min_time 3.8e-5, time_within 3.8e-5, first_within 0 (on the CPU a one-ulp change of cos moves min_dist by up to
    4e-4 of its tolerance).  On WGS84 min_dist deviates by 3.0e-2 of its tolerance, 1.4e-12 km on 0.463 km: the device's and
    the host's evaluation of Karney's inverse agree to 1.4 nm there, each being held to 20 nm of the true geodesic; every other
    output has the sphere's bits."""
    w, db, full = _fleet_batch()
    ref = enc.fleet_reference(model)
    got = _host(db.encounter_metrics(full, w["pairs"], enc.FLEET_R, t0=w["t0"], model=model))
    assert set(got) == set(OUTPUTS) and got["min_dist"].shape == (enc.FLEET_S, enc.FLEET_P) and got["status"].shape == (enc.FLEET_P,)
    worst = _compare(got, ref, enc.clock_span(w["nsteps"], w["dt"], w["t0"], w["pairs"]), enc.FLEET_R, f"meeting fleet, {model}")
    # Beyond the tolerances: both sides evaluate one definition, so what is left is the libm's cos (and, for min_dist, its
    # haversine): a deviation above 1e-2 of a tolerance wants an explanation.  The WGS84 leg is the exception: the device's
    # solver and track_estimators.geodesic are two evaluations of Karney's inverse, each held to 20 nm of the true geodesic
    # ("Geodesy against the definition"), so there the two may differ by 4e-11 km whatever the distance.
    km = worst.pop("min_dist_km")
    if model == "wgs84":
        assert km <= 4e-11, km
        del worst["min_dist"]
    assert max(worst.values()) <= 1e-2, ("a deviation above 1e-2 of its tolerance wants an explanation", worst)
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.encounter_metrics(_dev(db, poisoned), w["pairs"], enc.FLEET_R, t0=w["t0"], model=model))
    for k in OUTPUTS:
        assert np.array_equal(_u64(got[k].astype(np.float64)), _u64(again[k].astype(np.float64))), (k, "rows past nsteps were read")


def _same_bits(a, b, what, cols_a=slice(None), cols_b=slice(None), keys=OUTPUTS):
    for k in keys:
        x, y = a[k][..., cols_a], b[k][..., cols_b]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(_u64(x.astype(np.float64)), _u64(y.astype(np.float64))), (what, k)


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit: the pair list reversed and shuffled; S = 1 slices against S = 5; a subset of the outputs (each alone, and
    the three that need no within-R arithmetic); the window [3, 70) with re-based indices, in place on the fleet's rows and as
    a contiguous copy; t0 NULL against zeros; one pair alone."""
    w, db, full = _fleet_batch()
    pairs, t0, R = w["pairs"], w["t0"], enc.FLEET_R
    whole = _host(db.encounter_metrics(full, pairs, R, t0=t0))
    P = enc.FLEET_P
    for name, perm in (("reversed", np.arange(P)[::-1]), ("shuffled", np.random.default_rng(3).permutation(P))):
        got = _host(db.encounter_metrics(full, pairs[perm], R, t0=t0))
        _same_bits(got, whole, name, cols_b=perm)
    for s in range(enc.FLEET_S):
        one = _host(db.encounter_metrics(full[s], pairs, R, t0=t0))
        _same_bits({k: v for k, v in one.items() if k != "status"}, {k: v[s:s + 1] for k, v in whole.items() if k != "status"},
                   f"sample {s} alone", keys=PER_SAMPLE)
        assert np.array_equal(one["status"], whole["status"])
    for want in [(k,) for k in OUTPUTS] + [("min_time", "overlap", "nbroken"), ("min_dist", "nwithin")]:
        got = _abi_call(db, full, pairs, R, t0, want=want)
        _same_bits(got, whole, f"outputs {want}", keys=want)
    lo, hi = enc.FLEET_WINDOW
    inside = ((pairs >= lo) & (pairs < hi)).all(axis=1)
    assert inside.sum() > 100
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == enc.FLEET_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _host(win.encounter_metrics(view, pairs[inside] - lo, R, t0=t0[lo:hi]))
        _same_bits(got, whole, f"window, copied={copied}", cols_b=inside)
    wgs = _host(db.encounter_metrics(full, pairs, R, t0=t0, model="wgs84"))
    _same_bits(wgs, whole, "the model touches min_dist alone", keys=[k for k in OUTPUTS if k != "min_dist"])
    zeros = _abi_call(db, full, pairs, R, np.zeros(enc.FLEET_B))
    null = _abi_call(db, full, pairs, R, None)
    _same_bits(null, zeros, "t0 NULL against zeros")
    _same_bits(_host(db.encounter_metrics(full, pairs, R)), zeros, "t0=None through the front end")
    assert not np.array_equal(_u64(zeros["overlap"]), _u64(whole["overlap"]))
    k = int(np.argmax(whole["nwithin"][0] > 0))
    alone = _host(db.encounter_metrics(full, pairs[k:k + 1], R, t0=t0))
    _same_bits(alone, whole, "one pair alone", cols_b=slice(k, k + 1))
    with pytest.raises(ValueError, match=r"pairs must have shape \(P, 2\)"):
        db.encounter_metrics(full, pairs.T, R)
    with pytest.raises(ValueError, match="integer array or tensor"):
        db.encounter_metrics(full, pairs.astype(np.float64), R)
    with pytest.raises(ValueError, match="radius_km must be finite"):
        db.encounter_metrics(full, pairs, 1000.5)
    with pytest.raises(ValueError, match="t0 must be None, a scalar or have shape"):
        db.encounter_metrics(full, pairs, R, t0=np.zeros(3))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.encounter_metrics(full[:, :, :3], pairs, R)


@pytest.mark.gpu
def test_reversed_pairs():
    """(j, i) against (i, j), on the sphere: integers, overlap and status equal; times and min_dist within the tolerances of
    the comparison with the restatement.  The relative position changes sign and the roles of the two ships swap in sums of
    two terms, so the values need not be bit-equal; on an MI355X all four came out bit-equal (printed)."""
    w, db, full = _fleet_batch()
    pairs, t0 = w["pairs"], w["t0"]
    inside = (pairs >= 0).all(axis=1)
    fwd = _host(db.encounter_metrics(full, pairs, enc.FLEET_R, t0=t0))
    rev = _host(db.encounter_metrics(full, pairs[:, ::-1].copy(), enc.FLEET_R, t0=t0))
    span = enc.clock_span(w["nsteps"], w["dt"], t0, pairs)
    ref = enc.fleet_reference()
    skip = enc.grazing(ref, enc.FLEET_R) | enc.near_tie(ref)
    for k in ("nbroken", "status"):
        assert np.array_equal(fwd[k], rev[k]), k
    assert np.array_equal(fwd["nwithin"][~skip], rev["nwithin"][~skip])
    assert np.array_equal(_u64(fwd["overlap"]), _u64(rev["overlap"]))
    equal = {}
    for k in ("min_dist", "min_time", "time_within", "first_within"):
        nan = np.isnan(fwd[k])
        assert np.array_equal(nan[~skip], np.isnan(rev[k])[~skip]), k
        use = ~nan & ~skip
        err = np.abs(fwd[k] - rev[k])
        tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(fwd[k]) if k == "min_dist" else np.broadcast_to(pmc.TIME_RTOL * span, err.shape)
        assert (err[use] <= tol[use]).all(), (k, float((err[use] / tol[use]).max()))
        equal[k] = bool(np.array_equal(_u64(fwd[k]), _u64(rev[k])))
    print("reversed pairs bit-equal:", equal)
    # the reversed copies inside the list itself
    for r, o in enc.REVERSED:
        assert tuple(pairs[r]) == tuple(pairs[o][::-1]) and inside[r]
        assert fwd["nbroken"][:, r].tolist() == fwd["nbroken"][:, o].tolist()
        assert np.array_equal(_u64(fwd["overlap"][:, r]), _u64(fwd["overlap"][:, o]))


def _real_batch():
    """Four synthetic tracks of 20 steps through the filter and the smoother: track 1 is a copy of track 0, track 2 is track 0
    moved 60 degrees east, track 3 is another ship."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(4, nobs=11, seed0=100)
    arrays = {f.name: getattr(sb, f.name).copy() for f in dataclasses.fields(sb)}
    for a in arrays.values():
        a[1] = a[0]
        a[2] = a[0]
    arrays["lon"][2] += 60.0
    arrays["z"][2, 0] += 60.0
    hb = batch.pack_uniform(synthetic.SyntheticBatch(**arrays), 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 20, 13], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    return hb, db


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    """encounter_metrics on sm_mean and on the sampler's output of a real run against the restatement; encounter_statistics
    with one chunk equals sample_smoothed + encounter_metrics; two copies of one track meet with probability 1 and ships 60
    degrees apart with probability 0; other chunks draw other samples after the first chunk; encounter_candidates keeps the
    copies and drops the far ship."""
    from track_estimators import batch

    hb, db = _real_batch()
    pairs = np.array([(0, 1), (0, 2), (0, 3), (3, 1), (2, 2)], dtype=np.int32)
    R, nsamples = 500.0, 6
    t0 = np.array([0.0, 0.25, 0.0, 1.5])
    span = enc.clock_span(hb.nsteps, hb.dt, t0, pairs)
    sm = db.sm_mean.cpu().numpy()[None]
    got = _host(db.encounter_metrics(db.sm_mean, pairs, R, t0=t0))
    _compare(got, enc.encounter_metrics(sm, hb.nsteps, hb.dt, pairs, R, t0), span, R, "smoothed tracks")
    samples = db.sample_smoothed(nsamples, seed=4)
    direct = _host(db.encounter_metrics(samples, db.torch.from_numpy(pairs.astype(np.int64)).to(db.device), R, t0=t0))
    _compare(direct, enc.encounter_metrics(samples.cpu().numpy(), hb.nsteps, hb.dt, pairs, R, t0), span, R, "sampled tracks")
    one = batch.encounter_statistics(db, pairs, R, nsamples, seed=4, chunk=16, t0=t0)  # one chunk: sample_smoothed's draws
    for k in ("min_dist", "min_time", "time_within", "first_within", "nwithin"):
        assert one[k].shape == (nsamples, len(pairs)) and np.array_equal(_u64(one[k].astype(np.float64)), _u64(direct[k].astype(np.float64))), k
    for k in ("min_dist", "min_time", "time_within", "overlap"):
        assert np.array_equal(_u64(one[k + "_smoothed"]), _u64(got[k][0])), k
    assert np.array_equal(one["status"], got["status"]) and not one["status"].any() and not one["sample_status"].any()
    assert one["sample_status"].shape == (hb.B,)
    assert one["encounter_prob"].tolist() == [1.0, 0.0, float((direct["nwithin"][:, 2] > 0).mean()), float((direct["nwithin"][:, 3] > 0).mean()), 1.0]
    assert (one["min_dist"][:, 1] > 3000.0).all() and (one["min_dist"][:, 4] == 0.0).all() and (one["min_dist"][:, 0] < 200.0).all()
    close = dict(rtol=1e-13, atol=1e-13)  # the NaN-aware reductions may add in another order
    assert np.allclose(one["min_dist_mean"], direct["min_dist"].mean(axis=0), **close)
    assert np.allclose(one["min_dist_std"], direct["min_dist"].std(axis=0, ddof=1), **close)
    q = np.asarray((0.05, 0.5, 0.95))
    assert np.allclose(one["min_dist_quantiles"], np.quantile(direct["min_dist"], q, axis=0), **close)
    assert np.allclose(one["time_within_mean"], direct["time_within"].mean(axis=0), **close)
    assert one["time_within_quantiles"].shape == one["min_time_quantiles"].shape == (3, len(pairs))
    assert np.isnan(one["first_within_quantiles"][:, 1]).all() and np.isfinite(one["first_within_quantiles"][:, 0]).all()
    two = batch.encounter_statistics(db, pairs, R, nsamples, seed=4, chunk=2, t0=t0)  # chunks of 2: other draws after the first
    assert set(two) == set(one) and all(two[k].shape == one[k].shape and two[k].dtype == one[k].dtype for k in two)
    assert np.array_equal(_u64(two["min_dist"][:2]), _u64(one["min_dist"][:2]))
    assert not np.array_equal(_u64(two["min_dist"][2:, 0]), _u64(one["min_dist"][2:, 0]))
    assert two["encounter_prob"][[0, 1, 4]].tolist() == [1.0, 0.0, 1.0]
    a = batch.encounter_statistics(hb, pairs, R, 3, seed=9, chunk=3, t0=t0)
    b = batch.encounter_statistics(db, pairs, R, 3, seed=9, chunk=3, t0=t0)
    assert all(np.array_equal(_u64(a[k].astype(np.float64)), _u64(b[k].astype(np.float64))) for k in b)
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.encounter_statistics(db, pairs, R, 0)
    cand = batch.encounter_candidates(db, R, margin_km=100.0, t0=t0)
    assert cand.dtype == db.torch.int32 and cand.device == db.device
    c = [tuple(p) for p in cand.cpu().numpy().tolist()]
    assert (0, 1) in c and all(2 not in p for p in c) and c == sorted(c)
    apart = batch.encounter_candidates(db, R, margin_km=100.0, t0=[0.0, 100.0, 0.0, 0.0]).cpu().numpy().tolist()
    assert all(1 not in p and 2 not in p for p in apart)  # ship 1's clock is now disjoint from every other


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
