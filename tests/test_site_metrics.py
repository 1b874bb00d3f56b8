"""Tracks on the device against fixed sites (include/ste.h: ste_site_f64, ste_site_metrics_f64; DESIGN.md, "Sites"): declaration
and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers and against the encounter
restatement with one stationary ship per site, bit for bit, and the conditions of the port fleet that the device comparison
rests on (CPU); on the GPU the hand-made ships for both leg functions, the port fleet against the restatement, independence of
the surroundings bit for bit, the encounter kernel on the same data, the Python front ends on a real run, and the refusals on
the device build."""
import ctypes as C
import os
import re

import encounter_cases as enc
import numpy as np
import path_metrics_cases as pmc
import pytest
import site_cases as sc
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "nsites", "sites", "radius_km", "t0", "flags", "reserved", "min_dist", "min_time",
          "time_within", "first_within", "longest", "nwithin", "sound_time", "nbroken", "track_status", "site_status"]
OUTPUTS = FIELDS[9:]
PER_SITE = sc.FLOAT_OUTPUTS + sc.INT_OUTPUTS  # (S, M, B)
INT32 = ("nwithin", "nbroken", "track_status", "site_status")
SHARED = ("min_dist", "min_time", "time_within", "first_within", "nwithin")  # what an encounter call gives as well


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bits(a):
    return _u64(np.asarray(a).astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_site_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_site_f64\* si, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    assert re.search(r"^int ste_site_tile\(void\);", hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_site_f64 {"): hdr.index("} ste_site_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteSiteF64._fields_] == FIELDS
    # the layout of the C struct by hand: nstates and model share a word, nsites has one to itself (four bytes of padding before
    # the pointer that follows), flags and reserved share one, every pointer takes one
    offsets = {"nstates": 0, "model": 4, "states": 8, "nsites": 16, "sites": 24, "radius_km": 32, "t0": 40, "flags": 48,
               "reserved": 52}
    offsets.update({name: 56 + 8 * k for k, name in enumerate(OUTPUTS)})
    assert {f: getattr(binding.SteSiteF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteSiteF64) == 136 and re.search(r"} ste_site_f64;\s*/\* 136 bytes \*/", hdr)
    assert "ste_site_metrics_f64" in binding.SYMBOLS and "ste_site_tile" in binding.SYMBOLS
    lib = binding.load()
    assert hasattr(lib, "ste_site_metrics_f64") and 1 <= lib.ste_site_tile() <= 64
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert "(ste_site_metrics_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the site arguments travel beside the batch
    assert int(re.search(r"#define STE_SITES_MAX (\d+)", hdr).group(1)) == binding.STE_SITES_MAX == 65536
    assert int(re.search(r"#define STE_SITE_BAD_TIME 0x(\d+)", hdr).group(1), 16) == binding.STE_SITE_BAD_TIME == sc.BAD_TIME == 1
    assert int(re.search(r"#define STE_SITE_BAD_SITE 0x(\d+)", hdr).group(1), 16) == binding.STE_SITE_BAD_SITE == sc.BAD_SITE == 1
    assert sc.MAX_RADIUS_KM == binding.STE_ENCOUNTER_MAX_RADIUS_KM
    comment = hdr[hdr.index("SITES:"): hdr.index("#define STE_SITES_MAX")]
    for word in ("Clock.", "Bad clock.", "Pieces.", "Soundness.", "Bad site.", "Relative motion", "Closest approach.", "Within R",
                 "Accuracy.", "PIECE", "BROKEN", "RUN", "wrap180", "clamp01", "re-wrapped", "first piece wins a tie",
                 "without contraction", "longest", "skipped piece", "Refused with STE_EINVAL"):
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

    def good_site():
        e = binding.SteSiteF64()
        e.nstates, e.model, e.states, e.nsites, e.sites, e.radius_km, e.t0 = 3, binding.STE_PREP_WGS84, 0x3000, 5, 0x4000, 0x4800, 0x5000
        e.flags, e.reserved = 0, 0
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x6000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_site()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc = lib.ste_site_metrics_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_site_metrics_f64" in msg, (fields, rc, msg)

    for s, e, reason in ((None, good_site(), "batch pointer is NULL"), (good_batch(), None, "site arguments (si) are NULL")):
        assert lib.ste_site_metrics_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_site_metrics_f64" in msg
    refused("si->states is required", states=None)
    refused("si->sites is required", sites=None)
    refused("si->radius_km is required", radius_km=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1, 65537, 1 << 30):
        refused("between 1 and STE_SITES_MAX", nsites=n)
    for m in (-1, 2, 7):
        refused("STE_PREP_SPHERE or STE_PREP_WGS84 when min_dist is asked for", model=m)
    for f in (1, 0x80000000):
        refused("si->flags must be 0", flags=f)
        refused("si->reserved must be 0", reserved=f)
    refused("batch's dt is required", dt=None)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
    refused("2^31 - 1 blocks", B=2 ** 31 - 1, nsites=65536)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_hand_answers():
    """Twelve hand-made ships against fifteen sites, every coordinate a dyadic number (site_cases.HAND_SHIPS and HAND_SITES name
    them): a ship over a site in the middle of a step (0 km at the known time, 2 R / speed hours within) and past one at a known
    distance; a radius of a site's own; a zigzag with a pause inside R and one outside (two runs, longest the longer one,
    time_within their sum); a stationary ship inside and outside R (dd == 0); a ship stored wrapped against a site across the
    antimeridian; one point given as 180 and as -180 (the same bits, but for the min_dist of ships a hemisphere away: the leg
    function sees the longitude as given); a NaN latitude that splits a run; nsteps 0 and 1; a negative and a NaN dt inside nsteps, a NaN dt past them, a NaN
    t0; a step of zero length in the middle of a stay; and sites with a NaN coordinate or a radius that is NaN, negative or
    above the limit."""
    h = sc.hand_batch()
    res = {}
    for model in ("sphere", "wgs84"):
        res[model] = sc.site_metrics(h["states"], h["nsteps"], h["dt"], h["sites"], h["radius"], h["t0"], model)
        sc.check_hand_answers(res[model], f"restatement, {model}", model)
    r, s = res["wgs84"], res["sphere"]  # the model touches min_dist alone, and that by the ellipsoid's scales
    for k in PER_SITE[1:] + sc.TRACK_OUTPUTS + ("track_status", "site_status"):
        assert np.array_equal(_bits(r[k]), _bits(s[k])), k
    both = np.isfinite(s["min_dist"])
    assert np.array_equal(both, np.isfinite(r["min_dist"]))
    assert np.allclose(r["min_dist"][both], s["min_dist"][both], rtol=7e-3, atol=1e-9)  # atol: a ship on a site, 0 or a rounding


def _fleet_as_encounters():
    """The encounter restatement on the port fleet with its sites as stationary ships, one call per radius, as site-shaped
    arrays (S, M, B), overlap and nbroken included."""
    if "oracle" not in sc._CACHE:
        w = sc.fleet()
        e = sc.as_encounters(w["states"], w["nsteps"], w["dt"], w["t0"], w["sites"])
        S, M, B = sc.FLEET_S, sc.FLEET_M, sc.FLEET_B
        out = {}
        for R in sc.FLEET_RADII:
            sel = np.flatnonzero(w["radius"][e["pairs"][:, 1] - B] == R)
            r = enc.encounter_metrics(e["states"], e["nsteps"], e["dt"], e["pairs"][sel], R, e["t0"])
            for k in SHARED + ("overlap", "nbroken"):
                full = out.setdefault(k, np.zeros((S, B * M), dtype=r[k].dtype))
                full[:, sel] = r[k]
            assert not r["status"].any()
        sc._CACHE["oracle"] = {k: v.reshape(S, B, M).transpose(0, 2, 1) for k, v in out.items()}
    return sc._CACHE["oracle"]


def test_restatement_against_the_encounter_restatement():
    """The independent oracle.  Every dt and t0 of the port fleet is a multiple of 2^-6 h, so every knot is exact; one
    stationary ship per site is appended (nsteps = 1, t0 = the smallest t0 - 1, dt = the largest span + 2) and
    encounter_cases.encounter_metrics is given the full list of (track, site) pairs.  Bit for bit: min_dist, min_time,
    time_within, first_within, nwithin; overlap against sound_time and nbroken, for every site of every track."""
    ref, orc = sc.fleet_reference(), _fleet_as_encounters()
    w = sc.fleet()
    assert np.array_equal(w["dt"] * 64.0, np.round(w["dt"] * 64.0)) and np.array_equal(w["t0"] * 64.0, np.round(w["t0"] * 64.0))
    for k in SHARED:
        assert orc[k].shape == ref[k].shape and np.array_equal(_bits(orc[k]), _bits(ref[k])), k
    M = sc.FLEET_M
    assert np.array_equal(_bits(orc["overlap"]), _bits(np.repeat(ref["sound_time"][:, None], M, axis=1)))
    assert np.array_equal(orc["nbroken"], np.repeat(ref["nbroken"][:, None], M, axis=1))


def test_conditions_of_the_port_fleet():
    """The restatement alone on all five samples of the port fleet: what the device comparison assumes of it.  No value grazes
    (|sqrt(best q) - R| < 1e-9 R, or an end of a sound piece that close to the circle: a rounding of cos would decide nwithin or
    where a run ends) and none is a near tie (runner-up q <= best q (1 + 1e-9): min_time could come from either piece), so no
    case is excluded from any comparison.  In sample 0, 567 of the 4810 (site, track) pairs come within R, 6 of them twice or more,
    and 4243 never; every kind of row is there."""
    w, ref = sc.fleet(), sc.fleet_reference()
    S, M, B = sc.FLEET_S, sc.FLEET_M, sc.FLEET_B
    assert w["states"].shape == (S, sc.FLEET_N + 1, 4, B) and w["sites"].shape == (M, 2) and B == 2 * 64 + 2 and M == 37
    assert set(w["nsteps"][16:].tolist()) == set(range(9)) and (w["nsteps"][:16] == sc.FLEET_N).all()
    assert (np.abs(w["states"][:, :, 0, :8]) <= 180.0).all() and (w["states"][:, :, 0, 8:16] > 180.0).any()
    assert (w["sites"][:10, 0] > 179.0).all() and (w["sites"][:10, 0] > 180.0).any() and (w["sites"][:10, 0] < 180.0).any()
    assert sorted(set(w["radius"].tolist())) == list(sc.FLEET_RADII)
    for b, ns in enumerate(w["nsteps"]):  # garbage past nsteps
        assert ns == sc.FLEET_N or np.abs(w["states"][:, ns + 1:, :2, b]).max() > 90.0 or ns + 1 > sc.FLEET_N
    tie, graze = sc.near_tie(ref), sc.grazing(ref, w["radius"])
    nw = ref["nwithin"]
    within, twice, never = int((nw[0] > 0).sum()), int((nw[0] > 1).sum()), int((nw[0] == 0).sum())
    found = np.isfinite(ref["min_dist"])
    d = ref["min_dist"][found]
    print(f"port fleet: {within} (site, track) pairs of sample 0 within R, {twice} with two runs or more, {never} never; "
          f"{int((~found[0]).sum())} without a sound piece; min_dist {d.min():.3g} .. {d.max():.3g} km; near ties {int(tie.sum())} "
          f"and grazing {int(graze.sum())} of {S * M * B}; runs: {np.bincount(nw.ravel()).tolist()}; "
          f"least knot margin {ref['knot_margin'].min():.3g}")
    assert int(tie.sum()) == 0 and int(graze.sum()) == 0
    assert (within, twice, never) == (567, 6, 4243)
    assert not ref["track_status"].any() and not ref["site_status"].any() and not ref["nbroken"].any()
    assert (~found[0]).sum() == M * int((w["nsteps"] == 0).sum())
    assert (ref["longest"] <= ref["time_within"]).all() and (ref["longest"][nw > 1] < ref["time_within"][nw > 1]).all()
    assert np.array_equal(_bits(ref["longest"][nw == 1]), _bits(ref["time_within"][nw == 1]))


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _abi_call(db, states, sites, radius, t0, model="sphere", want=OUTPUTS):
    """ste_site_metrics_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor; ``want``: the outputs asked for (the
    others are NULL); -> dict of NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    S, B, M = int(states.shape[0]), int(states.shape[3]), len(sites)
    xy = _dev(db, np.asarray(sites, dtype=np.float64).T)
    rad = _dev(db, np.broadcast_to(np.asarray(radius, dtype=np.float64), (M,)))
    clock = None if t0 is None else _dev(db, np.asarray(t0, dtype=np.float64))
    shape = {"sound_time": (S, B), "nbroken": (S, B), "track_status": (B,), "site_status": (M,)}
    out = {}
    si = binding.SteSiteF64()
    si.nstates, si.model, si.states = S, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model], states.data_ptr()
    si.nsites, si.sites, si.radius_km, si.t0 = M, xy.data_ptr(), rad.data_ptr(), None if clock is None else clock.data_ptr()
    for k in want:
        out[k] = torch.empty(shape.get(k, (S, M, B)), dtype=torch.int32 if k in INT32 else torch.float64, device=db.device)
        setattr(si, k, out[k].data_ptr())
    binding.check(db.lib.ste_site_metrics_f64(C.byref(db.struct), C.byref(si), db._stream(None)), "ste_site_metrics_f64")
    torch.cuda.synchronize()
    return _host(out)


def _compare(got, ref, span, what, shared_only=False):
    """The device against a reference: integers and status equal, sound_time bit for bit, NaN patterns identical, min_dist within
    pmc.DIST_RTOL / DIST_ATOL, the times within pmc.TIME_RTOL of the track's clock span (``span``, (B,)).  Nothing is left out.
    Returns the largest deviations as fractions of their tolerances."""
    names = SHARED if shared_only else PER_SITE
    if not shared_only:
        for k in ("track_status", "site_status", "nbroken"):
            assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k)
        assert np.array_equal(_u64(got["sound_time"]), _u64(ref["sound_time"])), (what, "sound_time")
    assert got["nwithin"].dtype == np.int32 and np.array_equal(got["nwithin"], ref["nwithin"]), (what, "nwithin")
    worst = {}
    for k in names:
        if k == "nwithin":
            continue
        assert got[k].dtype == np.float64
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k]), nan), (what, k, "NaN pattern")
        err = np.abs(got[k] - ref[k])
        tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref[k]) if k == "min_dist" else np.broadcast_to(pmc.TIME_RTOL * span, err.shape)
        frac = (err / tol)[~nan]
        worst[k] = float(frac.max()) if frac.size else 0.0
        at = np.unravel_index(np.argmax(np.where(~nan, err / np.where(tol > 0, tol, 1.0), 0.0)), err.shape)
        print(f"{what}: {k} deviates by at most {worst[k]:.3g} of its tolerance ({int((~nan).sum())} values); worst at "
              f"{tuple(int(v) for v in at)}: {got[k][at]!r} against {ref[k][at]!r}")
        assert worst[k] <= 1.0, (what, k, worst[k], np.argwhere(~nan & (err > tol))[:5].tolist())
        if k == "min_dist":
            worst["min_dist_km"] = float(err[~nan].max()) if frac.size else 0.0
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_hand_made_ships_on_the_device(model):
    """The twelve hand-made ships and fifteen sites through the C ABI: the known answers, and the restatement."""
    from track_estimators import batch

    h = sc.hand_batch()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    got = _abi_call(db, _dev(db, h["states"]), h["sites"], h["radius"], h["t0"], model)
    sc.check_hand_answers(got, f"device, {model}", model)
    ref = sc.site_metrics(h["states"], h["nsteps"], h["dt"], h["sites"], h["radius"], h["t0"], model)
    # the planted NaN and negative dt belong to tracks that have no time to compare: their span only has to be a number
    span = sc.clock_span(h["nsteps"], np.abs(np.nan_to_num(h["dt"])), None) + 1.0
    _compare(got, ref, span, f"hand-made ships, {model}")


def _fleet_batch():
    from track_estimators import batch

    w = sc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_port_fleet_against_the_restatement(model):
    """S = 5, Nmax = 8, B = 130 (two waves plus two lanes), M = 37: integers and status equal, sound_time bit for bit, NaN patterns
    identical, min_dist within 1e-10 relative, times within 1e-12 of the track's clock span, nothing left out; NaN in the rows
    past nsteps changes nothing.  Largest deviations measured on an MI355X, as fractions of their tolerances: min_dist 1.6e-5
    (sphere), min_time 8.6e-4, time_within and longest 2.2e-3, first_within 4.3e-4.  On WGS84 min_dist deviates by 0.18 of its
    tolerance, 1.1e-12 km on 0.051 km; the leg is held to 4e-11 km as in the encounter tests: the device's solver and
    track_estimators.geodesic are two evaluations of Karney's inverse, each held to 20 nm of the true geodesic."""
    w, db, full = _fleet_batch()
    ref = sc.fleet_reference(model)
    got = _host(db.site_metrics(full, w["sites"], w["radius"], t0=w["t0"], model=model))
    S, M, B = sc.FLEET_S, sc.FLEET_M, sc.FLEET_B
    assert set(got) == set(OUTPUTS) and got["min_dist"].shape == (S, M, B) and got["sound_time"].shape == (S, B)
    assert got["track_status"].shape == (B,) and got["site_status"].shape == (M,)
    worst = _compare(got, ref, sc.clock_span(w["nsteps"], w["dt"], w["t0"]) + 1e-300, f"port fleet, {model}")
    km = worst.pop("min_dist_km")
    if model == "wgs84":
        assert km <= 4e-11, km
        del worst["min_dist"]
    assert max(worst.values()) <= 1e-2, ("a deviation above 1e-2 of its tolerance wants an explanation", worst)
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.site_metrics(_dev(db, poisoned), w["sites"], w["radius"], t0=w["t0"], model=model))
    for k in OUTPUTS:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, "rows past nsteps were read")


def _same_bits(a, b, what, keys=OUTPUTS, site_a=slice(None), site_b=slice(None), track_b=slice(None), sample_b=slice(None)):
    """``a`` against ``b`` restricted to the given sites (of either), tracks and samples (of ``b``)."""
    for k in keys:
        x, y = a[k], b[k]
        if k in PER_SITE:
            x, y = x[:, site_a], y[sample_b][:, site_b][..., track_b]
        elif k in sc.TRACK_OUTPUTS:
            y = y[sample_b][..., track_b]
        elif k == "track_status":
            y = y[track_b]
        else:
            x, y = x[site_a], y[site_b]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit: the site list reversed and shuffled; M = 1; M one below, at and one above one and two multiples of the kernel's
    site tile; S = 1 slices against S = 5; each output alone and two subsets; the window [3, 70) in place on the fleet's rows and
    as a contiguous copy; t0 NULL against zeros; one site alone against its column; the model changes min_dist alone."""
    from track_estimators._hip import binding

    w, db, full = _fleet_batch()
    sites, radius, t0 = w["sites"], w["radius"], w["t0"]
    M = sc.FLEET_M
    whole = _host(db.site_metrics(full, sites, radius, t0=t0))
    for name, perm in (("reversed", np.arange(M)[::-1]), ("shuffled", np.random.default_rng(3).permutation(M))):
        got = _host(db.site_metrics(full, sites[perm], radius[perm], t0=t0))
        _same_bits(got, whole, name, site_b=perm)
    tile = binding.load().ste_site_tile()
    sizes = sorted({1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1} - {0})
    assert sizes[-1] <= M
    for m in sizes:
        got = _host(db.site_metrics(full, sites[:m], radius[:m], t0=t0))
        _same_bits(got, whole, f"the first {m} sites (tile {tile})", site_b=slice(0, m))
    for s in range(sc.FLEET_S):
        one = _host(db.site_metrics(full[s], sites, radius, t0=t0))
        _same_bits(one, whole, f"sample {s} alone", sample_b=slice(s, s + 1))
    for want in [(k,) for k in OUTPUTS] + [("min_time", "sound_time", "nbroken", "track_status"), ("min_dist", "longest", "site_status")]:
        got = _abi_call(db, full, sites, radius, t0, want=want)
        _same_bits(got, whole, f"outputs {want}", keys=want)
    lo, hi = sc.FLEET_WINDOW
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == sc.FLEET_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _host(win.site_metrics(view, sites, radius, t0=t0[lo:hi]))
        assert got["min_dist"].shape == (sc.FLEET_S, M, hi - lo)
        _same_bits(got, whole, f"window, copied={copied}", track_b=slice(lo, hi))
    wgs = _host(db.site_metrics(full, sites, radius, t0=t0, model="wgs84"))
    _same_bits(wgs, whole, "the model touches min_dist alone", keys=[k for k in OUTPUTS if k != "min_dist"])
    assert not np.array_equal(_bits(wgs["min_dist"]), _bits(whole["min_dist"]))
    zeros = _abi_call(db, full, sites, radius, np.zeros(sc.FLEET_B))
    null = _abi_call(db, full, sites, radius, None)
    _same_bits(null, zeros, "t0 NULL against zeros")
    _same_bits(_host(db.site_metrics(full, sites, radius)), zeros, "t0=None through the front end")
    assert not np.array_equal(_u64(zeros["min_time"]), _u64(whole["min_time"]))
    k = int(np.argmax((whole["nwithin"][0] > 1).any(axis=1)))
    alone = _host(db.site_metrics(full, sites[k:k + 1], float(radius[k]), t0=t0))
    _same_bits(alone, whole, "one site alone", site_b=slice(k, k + 1))
    with pytest.raises(ValueError, match=r"sites must have shape \(M, 2\)"):
        db.site_metrics(full, sites.T, radius)
    with pytest.raises(ValueError, match="radius_km must be a scalar or have shape"):
        db.site_metrics(full, sites, radius[:3])
    with pytest.raises(ValueError, match="t0 must be None, a scalar or have shape"):
        db.site_metrics(full, sites, radius, t0=np.zeros(3))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.site_metrics(full[:, :, :3], sites, radius)
    with pytest.raises(ValueError, match="model must be one of"):
        db.site_metrics(full, sites, radius, model="flat")


@pytest.mark.gpu
def test_against_the_encounter_kernel_on_the_device():
    """The port fleet with one stationary ship per site appended, through ste_encounter_metrics_f64 (one call per radius) and
    through ste_site_metrics_f64: the shared outputs agree within the tolerances of the comparison with the restatement, overlap
    against sound_time and nbroken exactly.  Whether they agree bit for bit is printed ("Sites"): nothing promises
    it, the two kernels call cos in different surroundings."""
    from track_estimators import batch

    w, db, full = _fleet_batch()
    S, M, B = sc.FLEET_S, sc.FLEET_M, sc.FLEET_B
    got = _host(db.site_metrics(full, w["sites"], w["radius"], t0=w["t0"]))
    e = sc.as_encounters(w["states"], w["nsteps"], w["dt"], w["t0"], w["sites"])
    edb = batch.DeviceBatch(pmc.bare_batch(e["nsteps"], e["dt"]), histories=False)
    est = _dev(edb, e["states"])
    orc = {}
    for R in sc.FLEET_RADII:
        sel = np.flatnonzero(w["radius"][e["pairs"][:, 1] - B] == R)
        r = _host(edb.encounter_metrics(est, e["pairs"][sel], R, t0=e["t0"]))
        assert not r["status"].any()
        for k in SHARED + ("overlap", "nbroken"):
            orc.setdefault(k, np.zeros((S, B * M), dtype=r[k].dtype))[:, sel] = r[k]
    orc = {k: v.reshape(S, B, M).transpose(0, 2, 1) for k, v in orc.items()}
    _compare({k: got[k] for k in SHARED}, orc, sc.clock_span(w["nsteps"], w["dt"], w["t0"]) + 1e-300, "site kernel against encounter kernel",
             shared_only=True)
    assert np.array_equal(_bits(orc["overlap"]), _bits(np.repeat(got["sound_time"][:, None], M, axis=1)))
    assert np.array_equal(orc["nbroken"], np.repeat(got["nbroken"][:, None], M, axis=1))
    print("site kernel against encounter kernel, bit-equal:", {k: bool(np.array_equal(_bits(got[k]), _bits(orc[k]))) for k in SHARED})


def _real_batch():
    """Four synthetic tracks of 20 steps through the filter and the smoother; track 1 is a copy of track 0 and track 3 is short."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(4, nobs=11, seed0=100)
    arrays = {f.name: getattr(sb, f.name).copy() for f in dataclasses.fields(sb)}
    for a in arrays.values():
        a[1] = a[0]
    hb = batch.pack_uniform(synthetic.SyntheticBatch(**arrays), 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 20, 13], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    return hb, db


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    """site_metrics on sm_mean and on the sampler's output of a real run against the restatement; nearest_site against NumPy;
    site_statistics with zero draws gives the smoothed track's values for every sample and probabilities of 0 or 1; for given
    draws chunk = 3 and chunk = 16 agree bit for bit; with the generator and one chunk it is sample_smoothed + site_metrics; the
    quantile path is refused above max_bytes and agrees with NumPy below it."""
    from track_estimators import batch

    hb, db = _real_batch()
    torch = db.torch
    sm = db.sm_mean.cpu().numpy()[None]
    # a site on row 7 of track 0 (and of its copy), one on the last row of track 2, one 60 degrees away, and a bad one
    sites = np.array([sm[0, 7, :2, 0], sm[0, 20, :2, 2], sm[0, 0, :2, 0] + (60.0, 0.0), (np.nan, 0.0)])
    radius = np.array([40.0, 25.0, 500.0, 40.0])
    t0 = np.array([0.0, 0.25, 0.0, 1.5])
    span = sc.clock_span(hb.nsteps, hb.dt, t0)
    got = _host(db.site_metrics(db.sm_mean, sites, radius, t0=t0))
    ref = sc.site_metrics(sm, hb.nsteps, hb.dt, sites, radius, t0)
    assert not sc.grazing(ref, radius).any()
    _compare(got, ref, span, "smoothed tracks")
    assert got["site_status"].tolist() == [0, 0, 0, sc.BAD_SITE] and got["nwithin"][0, 0, 0] >= 1 and got["nwithin"][0, 2].sum() == 0
    nsamples = 7
    samples = db.sample_smoothed(nsamples, seed=4)
    dev = db.site_metrics(samples, torch.from_numpy(sites).to(db.device), torch.from_numpy(radius), t0=t0)
    direct = _host(dev)
    sref = sc.site_metrics(samples.cpu().numpy(), hb.nsteps, hb.dt, sites, radius, t0)
    assert not sc.grazing(sref, radius).any()
    _compare(direct, sref, span, "sampled tracks")
    # nearest_site against NumPy, with a track that has no distance at all (every site's NaN)
    md = dev["min_dist"].clone()
    md[2, :, 1] = float("nan")
    idx, dist = (v.cpu().numpy() for v in batch.nearest_site(md))
    h = md.cpu().numpy()
    filled = np.where(np.isnan(h), np.inf, h)
    want = np.where(np.isnan(h).all(axis=1), -1, filled.argmin(axis=1))
    assert idx.shape == (nsamples, hb.B) and np.array_equal(idx, want) and idx[2, 1] == -1 and (idx[:, 0] != 3).all()
    assert np.array_equal(_u64(dist), _u64(np.where(want < 0, np.nan, filled.min(axis=1))))
    # zero draws: every sample is the smoothed track
    kw = dict(t0=t0, min_stay_h=0.5)
    zero = batch.site_statistics(db, sites, radius, nsamples, chunk=3, draws=lambda buf, first: buf.zero_(), **kw)
    zsm = _host(db.site_metrics(db.sample_smoothed(1, draws=torch.zeros((1, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, device=db.device)),
                                sites, radius, t0=t0))
    for k in PER_SITE:
        assert np.array_equal(_bits(zero[k + "_smoothed"]), _bits(got[k][0])), k
    _compare({**zsm, "track_status": got["track_status"]}, {k: v[:1] if k in PER_SITE + sc.TRACK_OUTPUTS else v for k, v in got.items()}, span,
             "a sample of zero draws against the smoothed track")
    assert set(np.unique(zero["visit_prob"]).tolist()) <= {0.0, 1.0} and set(np.unique(zero["call_prob"]).tolist()) <= {0.0, 1.0}
    assert np.array_equal(zero["visit_prob"], (zsm["nwithin"][0] > 0).astype(np.float64))
    assert np.array_equal(zero["call_prob"], ((zsm["nwithin"][0] > 0) & (zsm["longest"][0] >= 0.5)).astype(np.float64))
    assert zero["visit_prob"][0, 0] == 1.0 and zero["visit_prob"][2].sum() == 0.0 and zero["visit_prob"][3].sum() == 0.0
    assert np.allclose(zero["time_within_mean"], zsm["time_within"][0], rtol=1e-14, atol=0.0)
    assert np.array_equal(zero["min_dist_count"], np.where(np.isnan(zsm["min_dist"][0]), 0, nsamples))
    # given draws, sample by sample: the chunk changes nothing, bit for bit
    noise = torch.randn((nsamples, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(db.device)
    fill = lambda buf, first: buf.copy_(noise[first:first + buf.shape[0]])  # noqa: E731
    a = batch.site_statistics(db, sites, radius, nsamples, chunk=3, draws=fill, **kw)
    b = batch.site_statistics(db, sites, radius, nsamples, chunk=16, draws=fill, **kw)
    assert set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    each = _host(db.site_metrics(db.sample_smoothed(nsamples, draws=noise.clone()), sites, radius, t0=t0))
    assert np.array_equal(a["visit_prob"], (each["nwithin"] > 0).mean(axis=0))
    assert 0.0 < a["time_within_mean"][0, 0] and np.allclose(a["time_within_mean"], each["time_within"].mean(axis=0), rtol=1e-13, atol=1e-15)
    # the generator and one chunk: sample_smoothed's draws
    one = batch.site_statistics(db, sites, radius, nsamples, seed=4, chunk=16, quantiles=(0.25, 0.5), **kw)
    assert np.array_equal(one["visit_prob"], (direct["nwithin"] > 0).mean(axis=0))
    assert np.array_equal(one["call_prob"], ((direct["nwithin"] > 0) & (direct["longest"] >= 0.5)).mean(axis=0))
    assert np.allclose(one["longest_mean"], direct["longest"].mean(axis=0), rtol=1e-13, atol=1e-15)
    good = one["min_dist_count"] > 0
    mean = np.array([[np.mean(c[~np.isnan(c)]) if (~np.isnan(c)).any() else np.nan for c in row.T] for row in direct["min_dist"].transpose(1, 0, 2)])
    assert np.allclose(one["min_dist_mean"][good], mean[good], rtol=1e-13) and np.isnan(one["min_dist_mean"][3]).all()
    assert one["time_within_quantiles"].shape == (2, 4, hb.B)
    assert np.allclose(one["time_within_quantiles"], np.quantile(direct["time_within"], (0.25, 0.5), axis=0), rtol=1e-13, atol=1e-15)
    assert not one["sample_status"].any() and one["site_status"].tolist() == [0, 0, 0, 1] and not one["track_status"].any()
    assert "min_dist_quantiles" not in a
    with pytest.raises(ValueError, match=rf"{nsamples} x 4 x {hb.B} doubles per quantity, {8 * nsamples * 4 * hb.B} bytes, above max_bytes = 100"):
        batch.site_statistics(db, sites, radius, nsamples, quantiles=(0.5,), max_bytes=100)
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.site_statistics(db, sites, radius, 0)
    viahb = batch.site_statistics(hb, sites, radius, 3, seed=9, chunk=3, **kw)
    viadb = batch.site_statistics(db, sites, radius, 3, seed=9, chunk=3, **kw)
    assert all(np.array_equal(_bits(viahb[k]), _bits(viadb[k])) for k in viadb)


@pytest.mark.gpu
def test_site_visits_of_the_drop_in_filter():
    """UnscentedKalmanFilter.site_visits on the committed ship 01203823 with two sites: for that ship, what the batch calls give
    (DeviceBatch.site_metrics on its smoothed track, nearest_site, site_statistics with the filter's seed and one chunk)."""
    from conftest import GOLDEN, load_cases
    from track_estimators import batch
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter
    from track_estimators.ship_track import ShipTrack

    assert os.path.exists(os.path.join(GOLDEN, "ship_01203823.csv"))
    c = load_cases("ukf_ship_01203823.npz")[0]
    st = ShipTrack()
    st.lon, st.lat, st.dts = c["z"][0].copy(), c["z"][1].copy(), c["dts"].copy()
    st.sog, st.cog, st.sog_rate, st.cog_rate, st.z = c["sog"].copy(), c["cog"].copy(), c["sog_rate"].copy(), c["cog_rate"].copy(), c["z"].copy()
    ukf = UnscentedKalmanFilter(H=c["H"], Q=c["Q"], R=c["R"], P=c["P0"], x0=st.z[:, 0].reshape(-1, 1).copy(),
                                non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.site_visits([(0.0, 0.0)], 10.0)
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    sm = db.sm_mean.cpu().numpy()
    sites = np.array([sm[hb.Nmax // 2, :2, 0] + (0.05, 0.0), sm[0, :2, 0] + (3.0, 1.0)])
    radius = (25.0, 10.0)
    want = _host(db.site_metrics(db.sm_mean, sites, radius, model="wgs84"))
    got = ukf.site_visits(sites, radius, model="wgs84")
    assert set(got) == set(PER_SITE) | {"nearest"} and got["nearest"] == 0
    for k in PER_SITE:
        assert got[k].shape == (2,) and np.array_equal(_bits(got[k]), _bits(want[k][0, :, 0])), k
    assert got["nwithin"][0] >= 1 and got["nwithin"][1] == 0 and got["min_dist"][0] < 25.0
    n = 5
    stats = batch.site_statistics(hb, sites, radius, n, seed=3, chunk=n, min_stay_h=0.25, model="wgs84")
    vis = ukf.site_visits(sites, radius, nsamples=n, min_stay_h=0.25, model="wgs84", random_state=3)
    for k in ("visit_prob", "call_prob", "min_dist_mean", "time_within_mean", "longest_mean") + tuple(p + "_smoothed" for p in PER_SITE):
        assert vis[k].shape == (2,) and np.array_equal(_bits(vis[k]), _bits(stats[k][:, 0])), k
    assert vis["visit_prob"][1] == 0.0 and 0.0 <= vis["call_prob"][0] <= vis["visit_prob"][0] <= 1.0
    with pytest.raises(ValueError, match="nsamples must be >= 0"):
        ukf.site_visits(sites, radius, nsamples=-1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
