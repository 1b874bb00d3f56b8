"""Speed made good, speed bands and stops of tracks on the device (include/ste.h: ste_speed_f64, ste_speed_metrics_f64; DESIGN.md,
"Speeds"): declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers and against
the path restatement, and the conditions of the random-walk fleet that the device comparison rests on (CPU); on the GPU the
hand-made ships for both leg functions, the walk fleet against the restatement with and without injected faults, independence
of the surroundings bit for bit, the distance of path_metrics bit for bit, the Python front ends on a real run, and the refusals
on the device build."""
import ctypes as C
import os
import re

import numpy as np
import path_metrics_cases as pmc
import pytest
import speed_cases as spc
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "flags", "nbands", "band_edges", "threshold", "threshold_all", "min_run_h", "speed", "dist",
          "sound_time", "vmax", "vmax_time", "band_time", "cond_time", "run_time", "first_run", "longest", "longest_start", "nruns",
          "nbroken", "track_status"]
OUTPUTS = FIELDS[9:]
INT32 = ("nruns", "nbroken", "track_status")
MODELS = ("sphere", "wgs84")


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bits(a):
    return _u64(np.asarray(a).astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators import batch
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_speed_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_speed_f64\* sp, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_speed_f64 {"): hdr.index("} ste_speed_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteSpeedF64._fields_] == FIELDS
    # the layout of the C struct by hand: nstates and model share a word, flags and nbands share one, every pointer and double
    # takes one
    offsets = {"nstates": 0, "model": 4, "states": 8, "flags": 16, "nbands": 20, "band_edges": 24, "threshold": 32,
               "threshold_all": 40, "min_run_h": 48}
    offsets.update({name: 56 + 8 * k for k, name in enumerate(OUTPUTS)})
    assert {f: getattr(binding.SteSpeedF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteSpeedF64) == 168 and re.search(r"} ste_speed_f64;\s*/\* 168 bytes \*/", hdr)
    assert "ste_speed_metrics_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_speed_metrics_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert "(ste_speed_metrics_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the speed arguments travel beside the batch
    assert int(re.search(r"#define STE_SPEED_MAX_BANDS (\d+)", hdr).group(1)) == binding.STE_SPEED_MAX_BANDS == 32
    assert int(re.search(r"#define STE_SPEED_ABOVE 0x(\d+)u", hdr).group(1), 16) == binding.STE_SPEED_ABOVE == 1
    assert int(re.search(r"#define STE_SPEED_BAD_TIME 0x(\d+)", hdr).group(1), 16) == binding.STE_SPEED_BAD_TIME == spc.BAD_TIME == 1
    assert int(re.search(r"#define STE_SPEED_BAD_LIMIT 0x(\d+)", hdr).group(1), 16) == binding.STE_SPEED_BAD_LIMIT == spc.BAD_LIMIT == 2
    assert batch.KNOT_KMH == 1.852
    comment = hdr[hdr.index("SPEEDS:"): hdr.index("#define STE_SPEED_MAX_BANDS")]
    for word in ("Clock.", "Bad clock, bad limit.", "Step.", "Sums.", "Maximum.", "Bands.", "Runs.", "SKIPPED", "BROKEN", "SOUND",
                 "QUALIFIES", "RUN", "first step wins", "without contraction", "longest", "No tolerance", "Refused with STE_EINVAL"):
        assert word in comment, word


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The device pointers below are not memory: nothing may be launched, with a GPU or without one.  The
    band edges are the one host array the call reads."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    runs = spc.RUN_OUTPUTS

    def edges(*values):
        return (C.c_double * len(values))(*values)

    good_edges = edges(0.0, 5.0, 10.0, 40.0)

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.dt, s.nsteps = 0x1000, 0x2000
        return s

    def good_speed():
        e = binding.SteSpeedF64()
        e.nstates, e.model, e.states, e.flags = 3, binding.STE_PREP_WGS84, 0x3000, binding.STE_SPEED_ABOVE
        e.nbands, e.band_edges = 3, C.cast(good_edges, C.c_void_p)
        e.threshold, e.threshold_all, e.min_run_h = 0x4000, float("nan"), 0.5
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x6000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_speed()
        keep = []
        for name, value in fields.items():
            if name == "band_edges" and value is not None:
                keep.append(value)
                value = C.cast(value, C.c_void_p)
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc = lib.ste_speed_metrics_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_speed_metrics_f64" in msg, (fields, rc, msg)

    for s, e, reason in ((None, good_speed(), "batch pointer is NULL"), (good_batch(), None, "speed arguments (sp) are NULL")):
        assert lib.ste_speed_metrics_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_speed_metrics_f64" in msg
    refused("sp->states is required", states=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for m in (-1, 2, 7):
        refused("STE_PREP_SPHERE or STE_PREP_WGS84", model=m)
    for f in (2, 3, 0x80000000):
        refused("sp->flags must be 0 or STE_SPEED_ABOVE", flags=f)
    for n in (-1, 33, 1 << 30):
        refused("between 0 and STE_SPEED_MAX_BANDS", nbands=n)
    refused("band_edges is required with nbands > 0", band_edges=None)
    refused("band_edges must be NULL with nbands == 0", nbands=0, band_time=None)
    refused("band_time needs bands", nbands=0, band_edges=None)
    for bad in ((0.0, 5.0, float("nan"), 40.0), (0.0, 5.0, 10.0, float("inf")), (-1.0, 5.0, 10.0, 40.0), (0.0, 5.0, 5.0, 40.0),
                (0.0, 10.0, 5.0, 40.0), (-0.5, -0.25, 10.0, 40.0)):
        refused("finite, >= 0 and strictly ascending", band_edges=edges(*bad))
    for h in (-1.0, float("nan"), float("inf")):
        refused("min_run_h must be finite and >= 0", min_run_h=h)
    for v in (float("nan"), float("inf"), -2.0):
        refused("needs sp->threshold, or a threshold_all", threshold=None, threshold_all=v)
        for k in runs:  # one run output is enough
            refused("needs sp->threshold, or a threshold_all", threshold=None, threshold_all=v, **{o: None for o in runs if o != k})
    refused("batch's dt is required", dt=None)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def _hand_restatement(model, above, runs=True):
    h = spc.hand_batch()
    return spc.speed_metrics(h["states"], h["nsteps"], h["dt"], model, spc.HAND_EDGES, h["threshold"] if runs else None, above,
                             spc.HAND_MIN_RUN_H)


def test_restatement_against_hand_answers():
    """Seven hand-made ships on one-degree legs along the equator (speed_cases.HAND_SHIPS names them): chosen dt give speeds of
    K, K/2, K/4 and 2 K km/h in known bands and runs; a ship that never moves has vmax == 0 at time 0 (the first step wins) and,
    with threshold 0, one run of the whole track under either flag; a zero dt and a NaN row split runs; a negative dt and a NaN
    threshold null the track; nsteps 0 and 2.  Without a threshold there is no bad limit: that ship is the paces again."""
    for model in MODELS:
        for above in (False, True):
            spc.check_hand_answers(_hand_restatement(model, above), f"restatement, {model}, above={above}", above)
        free = _hand_restatement(model, False, runs=False)
        assert not set(spc.RUN_OUTPUTS) & set(free) and free["track_status"].tolist() == [0, 0, 0, spc.BAD_TIME, 0, 0, 0]
        for k in ("dist", "sound_time", "vmax", "vmax_time"):
            assert free[k][0, 4] == free[k][0, 0] and free[k][0, 0] > 0.0, k
        assert np.array_equal(free["band_time"][0, :, 4], free["band_time"][0, :, 0])


@pytest.mark.parametrize("model", MODELS)
def test_restatement_distance_is_that_of_the_path_restatement(model):
    """Every step of the walk fleet is examined and sound, so dist is path_metrics_cases.path_metrics' distance bit for bit."""
    ref = spc.walk_speeds(model)
    assert not ref["nbroken"].any() and not ref["track_status"].any()
    assert np.array_equal(_u64(ref["dist"]), _u64(pmc.walk_reference(model, None)["distance"]))
    w = pmc.walk()
    total = np.array([sum(w["dt"][:ns, t], 0.0) for t, ns in enumerate(w["nsteps"])])
    assert np.array_equal(_u64(ref["sound_time"]), _u64(np.broadcast_to(total, ref["sound_time"].shape)))


@pytest.mark.parametrize("model", MODELS)
def test_conditions_of_the_walk_fleet(model):
    """What the device comparison assumes of the walk fleet (S = 5, Nmax = 8, B = 130, every nsteps from 0 to 8) with its band
    edges and per-track thresholds: no speed within 1e-6 relative of an edge or of its track's threshold (a rounding of the leg
    would decide a band or a run), each track's two largest speeds more than 1e-6 relative apart (vmax_time could come from
    either), and min_run_h equal to no run length.  No case is left out of any comparison."""
    w = pmc.walk()
    assert w["states"].shape == (5, 9, 4, 130) and set(w["nsteps"].tolist()) == set(range(9))
    v = spc.walk_speeds(model)["speed"]
    live = v != spc.SENTINEL
    assert np.isfinite(v[live]).all() and (v[live] > 0.0).all() and live.sum() == 5 * int(w["nsteps"].sum())
    for nb in spc.WALK_BANDS[1:]:
        e = spc.walk_edges(model, nb)
        assert e.shape == (nb + 1,) and (np.diff(e) > 0.0).all() and e[0] > 0.0
        gap = np.abs(v[live][:, None] - e[None]) / e[None]
        assert gap.min() > spc.GAP_RTOL, (nb, gap.min())
        assert (v[live] < e[0]).any() and (v[live] >= e[-1]).any()
    thr = spc.walk_thresholds(model)
    gap = np.abs(v - thr[None, None]) / thr[None, None]
    assert gap[live].min() > spc.GAP_RTOL, gap[live].min()
    top = np.sort(np.where(live, v, -np.inf), axis=1)[:, -2:]  # (S, 2, B): runner-up and best
    two = np.isfinite(top[:, 0])
    assert (top[:, 1][two] - top[:, 0][two] > spc.GAP_RTOL * top[:, 1][two]).all()
    for above in (False, True):
        ref = spc.walk_reference(model, 5, above)
        assert (ref["run_lengths"] != spc.WALK_MIN_RUN_H).all()
        counting = ref["run_lengths"] >= spc.WALK_MIN_RUN_H
        print(f"walk fleet, {model}, above={above}: {len(counting)} runs, {int(counting.sum())} of min_run_h or longer; nruns "
              f"{np.bincount(ref['nruns'].ravel()).tolist()}; least gaps: threshold {gap[live].min():.3g}")
        assert counting.any() and not counting.all() and (ref["nruns"] > 1).any()
        assert (ref["band_time"].sum(axis=1) <= ref["sound_time"] * (1.0 + 1e-14)).all() and (ref["band_time"] > 0.0).any(axis=(0, 2)).all()


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _abi_call(db, states, model="sphere", edges=None, threshold=None, above=False, min_run_h=0.0, want=OUTPUTS):
    """ste_speed_metrics_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor; ``threshold``: None, a scalar
    (threshold_all) or (B,); ``want``: the outputs asked for (the others are NULL), speed pre-filled with SENTINEL; -> dict of
    NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    S, N, B = int(states.shape[0]), int(states.shape[1]) - 1, int(states.shape[3])
    nb = 0 if edges is None else len(edges) - 1
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    shape = {"speed": (S, N, B), "band_time": (S, nb, B), "track_status": (B,)}
    sp = binding.SteSpeedF64()
    sp.nstates, sp.model, sp.states = S, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model], states.data_ptr()
    sp.flags, sp.nbands, sp.band_edges = (binding.STE_SPEED_ABOVE if above else 0), nb, None if e is None else e.ctypes.data
    sp.threshold, sp.threshold_all, sp.min_run_h = None, float("nan"), min_run_h
    limit = None
    if threshold is not None and np.ndim(threshold) == 0:
        sp.threshold_all = float(threshold)
    elif threshold is not None:
        limit = _dev(db, np.asarray(threshold, dtype=np.float64))
        sp.threshold = limit.data_ptr()
    out = {}
    for k in want:
        out[k] = torch.full(shape.get(k, (S, B)), spc.SENTINEL, dtype=torch.float64, device=db.device) if k not in INT32 else \
            torch.full(shape.get(k, (S, B)), -7, dtype=torch.int32, device=db.device)
        setattr(sp, k, out[k].data_ptr())
    binding.check(db.lib.ste_speed_metrics_f64(C.byref(db.struct), C.byref(sp), db._stream(None)), "ste_speed_metrics_f64")
    torch.cuda.synchronize()
    return _host(out)


def _compare(got, ref, what):
    """The device against the restatement: integers, status, sums of dt and times bit for bit; speed, dist and vmax (the values
    derived from a leg) with identical NaN patterns and untouched rows and within pmc.DIST_RTOL / DIST_ATOL, the project's
    tolerance for the same leg functions (the division by dt adds one rounding).  Every figure is printed before it is judged."""
    for k, g in got.items():
        r = ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        if k not in spc.LEG_DERIVED:
            assert np.array_equal(_bits(g), _bits(r)), (what, k, np.argwhere(_bits(g) != _bits(r))[:5].tolist())
            continue
        nan, left = np.isnan(r), r == spc.SENTINEL
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(g == spc.SENTINEL, left), (what, k, "NaN pattern or untouched rows")
        err = np.abs(g - r)
        frac = (err / (pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(r)))[~nan & ~left]
        worst = float(frac.max()) if frac.size else 0.0
        print(f"{what}: {k} deviates by at most {worst:.3g} of its tolerance ({frac.size} values)")
        assert worst <= 1.0, (what, k, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_hand_made_ships_on_the_device(model):
    """The seven hand-made ships through the C ABI, default and above: the known answers, and the restatement; without a run
    output the ship with the NaN threshold is the paces again."""
    from track_estimators import batch

    h = spc.hand_batch()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    states = _dev(db, h["states"])
    for above in (False, True):
        got = _abi_call(db, states, model, spc.HAND_EDGES, h["threshold"], above, spc.HAND_MIN_RUN_H)
        spc.check_hand_answers(got, f"device, {model}, above={above}", above)
        _compare(got, _hand_restatement(model, above), f"hand-made ships, {model}, above={above}")
    free = [k for k in OUTPUTS if k not in spc.RUN_OUTPUTS]
    got = _abi_call(db, states, model, spc.HAND_EDGES, None, False, spc.HAND_MIN_RUN_H, want=free)
    _compare(got, _hand_restatement(model, False, runs=False), f"hand-made ships without runs, {model}")


def _walk_batch(w=None):
    from track_estimators import batch

    w = pmc.walk() if w is None else w
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("above", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_walk_fleet_against_the_restatement(model, above):
    """S = 5, Nmax = 8, B = 130 (two waves plus two lanes) with 0, 1, 5 and 32 bands: nruns, nbroken, track_status, band_time,
    cond_time, run_time, first_run, longest, longest_start, vmax_time and sound_time bit for bit, speed, dist and vmax within the
    leg's tolerance, nothing left out; through the front end, which gives NaN past nsteps where the call leaves rows alone.
    Largest deviations measured on an MI355X, as fractions of the tolerance: speed 5.3e-6, dist 3.4e-6 and vmax 4.5e-6 on the
    sphere; speed 0.024, dist and vmax 0.0014 on WGS84 (two evaluations of Karney's inverse)."""
    w, db, full = _walk_batch()
    thr = spc.walk_thresholds(model)
    for nb in spc.WALK_BANDS:
        ref = dict(spc.walk_reference(model, nb, above))
        del ref["run_lengths"]
        edges = spc.walk_edges(model, nb)
        got = _abi_call(db, full, model, edges, thr, above, spc.WALK_MIN_RUN_H, want=[k for k in OUTPUTS if nb or k != "band_time"])
        if nb == 0:
            del ref["band_time"]
        assert set(got) == set(ref)
        _compare(got, ref, f"walk fleet, {model}, above={above}, {nb} bands")
        front = _host(db.speed_metrics(full, bands=edges, threshold=thr, above=above, min_run_h=spc.WALK_MIN_RUN_H, model=model,
                                       per_step=True))
        assert set(front) == set(got)
        assert np.isnan(front["speed"][got["speed"] == spc.SENTINEL]).all()
        front["speed"] = np.where(got["speed"] == spc.SENTINEL, spc.SENTINEL, front["speed"])
        for k in got:
            assert np.array_equal(_bits(front[k]), _bits(got[k])), (k, "front end against the C ABI")


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_walk_fleet_with_injected_faults(model):
    """A copy of the fleet with zero dt, NaN coordinates, one negative dt and one NaN threshold: the status bits, the NaN pattern
    and the closing of runs are the restatement's, and the speed rows past nsteps keep the sentinel they were filled with."""
    w, factor = spc.faulty_walk()
    _, db, full = _walk_batch(w)
    thr, edges = spc.walk_thresholds(model) * factor, spc.walk_edges(model, 5)
    for above in (False, True):
        ref = spc.speed_metrics(w["states"], w["nsteps"], w["dt"], model, edges, thr, above, spc.WALK_MIN_RUN_H)
        del ref["run_lengths"]
        assert ref["track_status"][17] == spc.BAD_TIME and ref["track_status"][26] == spc.BAD_LIMIT and ref["track_status"].sum() == 3
        assert ref["nbroken"].sum() == 7 and np.isnan(ref["speed"]).sum() == 7 + 4 * 5 + 2 * 8 * 5  # broken, skipped, bad tracks
        got = _abi_call(db, full, model, edges, thr, above, spc.WALK_MIN_RUN_H)
        _compare(got, ref, f"faulty walk fleet, {model}, above={above}")
        for t, ns in enumerate(w["nsteps"]):
            assert (got["speed"][:, ns:, t] == spc.SENTINEL).all() and (got["speed"][:, :ns, t] != spc.SENTINEL).all(), t
        clean = spc.walk_reference(model, 5, above)
        assert (got["nruns"] != clean["nruns"]).any()  # the faults did split or remove runs


def _same_bits(a, b, what, keys, track_b=slice(None), sample_b=slice(None)):
    """``a`` against ``b`` restricted to the given tracks and samples (of ``b``)."""
    for k in keys:
        x, y = a[k], b[k]
        y = y[track_b] if k == "track_status" else y[sample_b][..., track_b]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit: S = 1 slices against S = 5; the window pmc.WALK_WINDOW in place on the fleet's rows (track_stride) and as a
    contiguous copy; each output alone and two subsets against all outputs; a scalar threshold against the same value per track;
    fewer bands change band_time alone; the model changes the clock's outputs not at all."""
    w, db, full = _walk_batch()
    thr, edges = spc.walk_thresholds("sphere"), spc.walk_edges("sphere", 5)
    kw = dict(bands=edges, threshold=thr, min_run_h=spc.WALK_MIN_RUN_H, per_step=True)
    whole = _host(db.speed_metrics(full, **kw))
    assert set(whole) == set(OUTPUTS)
    for s in range(pmc.WALK_S):
        one = _host(db.speed_metrics(full[s], **kw))
        _same_bits(one, whole, f"sample {s} alone", OUTPUTS, sample_b=slice(s, s + 1))
    lo, hi = pmc.WALK_WINDOW
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == pmc.WALK_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _host(win.speed_metrics(view, **{**kw, "threshold": thr[lo:hi]}))
        assert got["dist"].shape == (pmc.WALK_S, hi - lo) and got["speed"].shape == (pmc.WALK_S, pmc.WALK_N, hi - lo)
        _same_bits(got, whole, f"window, copied={copied}", OUTPUTS, track_b=slice(lo, hi))
    base = _abi_call(db, full, "sphere", edges, thr, False, spc.WALK_MIN_RUN_H)
    for want in [(k,) for k in OUTPUTS] + [("vmax", "vmax_time"), ("dist", "band_time", "nbroken"), ("speed", "nruns", "longest")]:
        got = _abi_call(db, full, "sphere", edges if "band_time" in want else None, thr, False, spc.WALK_MIN_RUN_H, want=want)
        _same_bits(got, base, f"outputs {want}", want)
    flat = _host(db.speed_metrics(full, threshold=float(thr[5]), min_run_h=spc.WALK_MIN_RUN_H))
    each = _host(db.speed_metrics(full, threshold=np.full(pmc.WALK_B, thr[5]), min_run_h=spc.WALK_MIN_RUN_H))
    _same_bits(flat, each, "a scalar threshold against one per track", list(flat))
    _same_bits({k: v[..., 5:6] if k != "track_status" else v[5:6] for k, v in flat.items()}, whole, "track 5 under its own threshold",
               [k for k in flat], track_b=slice(5, 6))
    fewer = _host(db.speed_metrics(full, **{**kw, "bands": edges[1:4]}))
    _same_bits(fewer, whole, "fewer bands", [k for k in OUTPUTS if k != "band_time"])
    assert np.array_equal(_bits(fewer["band_time"]), _bits(whole["band_time"][:, 1:3]))
    wgs = _host(db.speed_metrics(full, **{**kw, "model": "wgs84"}))
    _same_bits(wgs, whole, "the model leaves the clock alone", ("sound_time", "nbroken", "track_status"))
    assert not np.array_equal(_bits(wgs["dist"]), _bits(whole["dist"]))
    with pytest.raises(ValueError, match="threshold must be None, a scalar or have shape"):
        db.speed_metrics(full, threshold=np.zeros(3))
    with pytest.raises(ValueError, match="bands must be None or 2 .. 33 band edges"):
        db.speed_metrics(full, bands=np.arange(40.0))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.speed_metrics(full[:, :, :3])
    with pytest.raises(ValueError, match="model must be one of"):
        db.speed_metrics(full, model="flat")


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_distance_is_that_of_path_metrics(model):
    """Every step of the clean fleet is examined and sound: dist has the bits of DeviceBatch.path_metrics' distance, whichever
    other outputs are asked for."""
    w, db, full = _walk_batch()
    path = _host(db.path_metrics(full, model=model))["distance"]
    lean = _host(db.speed_metrics(full, model=model))
    rich = _host(db.speed_metrics(full, bands=spc.walk_edges(model, 32), threshold=spc.walk_thresholds(model), model=model, per_step=True))
    assert not lean["nbroken"].any() and not lean["track_status"].any()
    for got in (lean, rich):
        assert np.array_equal(_u64(got["dist"]), _u64(path))


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
    """speed_metrics on sm_mean of a real run is consistent with path_metrics and with the restatement; speed_statistics with one
    chunk is sample_smoothed followed by speed_metrics; probabilities lie in [0, 1]; for given draws chunk 4 and chunk 16 agree
    bit for bit on every output (the sums take their terms in sample order)."""
    from track_estimators import batch

    hb, db = _real_batch()
    torch = db.torch
    sm = db.sm_mean.cpu().numpy()[None]
    free = _host(db.speed_metrics(db.sm_mean, per_step=True))
    path = _host(db.path_metrics(db.sm_mean))
    assert np.array_equal(_u64(free["dist"]), _u64(path["distance"])) and not free["nbroken"].any() and not free["track_status"].any()
    total = np.array([sum(hb.dt[:ns, t], 0.0) for t, ns in enumerate(hb.nsteps)])
    assert np.array_equal(_u64(free["sound_time"][0]), _u64(total))
    assert np.array_equal(_u64(free["vmax"]), _u64(np.nanmax(free["speed"], axis=1)))
    assert np.isnan(free["speed"][0, 13:, 3]).all() and not np.isnan(free["speed"][0, :13, 3]).any()
    v = np.sort(free["speed"][0][~np.isnan(free["speed"][0])])
    edges = np.array([0.0, 0.5 * (v[3] + v[4]), 0.5 * (v[len(v) // 2] + v[len(v) // 2 + 1]), 2.0 * v[-1]])
    thr = float(edges[2])
    kw = dict(bands=edges, threshold=thr, min_run_h=0.5)
    got = _host(db.speed_metrics(db.sm_mean, per_step=True, **kw))
    ref = spc.speed_metrics(sm, hb.nsteps, hb.dt, "sphere", edges, thr, False, 0.5)
    ref["speed"] = np.where(ref["speed"] == spc.SENTINEL, np.nan, ref["speed"])
    del ref["run_lengths"]
    _compare(got, ref, "smoothed tracks")
    assert np.allclose(got["band_time"][0].sum(axis=0), got["sound_time"][0], rtol=1e-14)  # the edges span every speed
    for k in got:
        if k != "track_status":
            assert np.array_equal(_bits(got[k][..., 1]), _bits(got[k][..., 0])), (k, "a copy of a track")
    nsamples = 7
    samples = db.sample_smoothed(nsamples, seed=4)
    direct = _host(db.speed_metrics(samples, **kw))
    limit = np.array([float(np.median(direct["vmax"][:, t])) for t in range(hb.B)]) + 1e-9
    one = batch.speed_statistics(db, nsamples, seed=4, chunk=16, limit_kmh=limit, quantiles=(0.25, 0.5), **kw)
    assert np.array_equal(_u64(one["vmax"]), _u64(direct["vmax"]))
    assert np.array_equal(_u64(one["mean_speed"]), _u64(direct["dist"] / direct["sound_time"]))
    assert np.array_equal(one["exceed_prob"], (direct["vmax"] > limit).mean(axis=0)) and 0.0 < one["exceed_prob"][0] < 1.0
    assert np.array_equal(one["run_prob"], (direct["nruns"] >= 1).mean(axis=0))
    for k in ("exceed_prob", "run_prob"):
        assert ((one[k] >= 0.0) & (one[k] <= 1.0)).all(), k
    for k in ("band_time", "cond_time", "run_time"):
        assert np.allclose(one[k + "_mean"], direct[k].mean(axis=0), rtol=1e-13, atol=1e-15), k
    assert np.allclose(one["vmax_mean"], direct["vmax"].mean(axis=0), rtol=1e-13)
    assert np.allclose(one["vmax_std"], direct["vmax"].std(axis=0, ddof=1), rtol=1e-10)
    assert one["mean_speed_quantiles"].shape == (2, hb.B)
    assert np.allclose(one["vmax_quantiles"], np.quantile(direct["vmax"], (0.25, 0.5), axis=0), rtol=1e-13)
    for k in got:
        if k not in ("track_status", "speed"):
            assert np.array_equal(_bits(one[k + "_smoothed"]), _bits(got[k][0])), k
    assert np.array_equal(_u64(one["mean_speed_smoothed"]), _u64(got["dist"][0] / got["sound_time"][0]))
    assert not one["status"].any() and not one["track_status"].any()
    scalar = batch.speed_statistics(db, nsamples, seed=4, chunk=16, limit_kmh=float(limit[0]), **kw)
    assert scalar["exceed_prob"][0] == one["exceed_prob"][0]
    bare = batch.speed_statistics(db, 3, seed=4)
    assert not {"exceed_prob", "run_prob", "band_time_mean", "cond_time_mean", "run_time_mean"} & set(bare)
    # given draws, sample by sample: the chunk changes nothing, bit for bit
    noise = torch.randn((nsamples, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(db.device)
    fill = lambda buf, first: buf.copy_(noise[first:first + buf.shape[0]])  # noqa: E731
    a = batch.speed_statistics(db, nsamples, chunk=4, draws=fill, limit_kmh=limit, **kw)
    b = batch.speed_statistics(db, nsamples, chunk=16, draws=fill, limit_kmh=limit, **kw)
    assert set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    each = _host(db.speed_metrics(db.sample_smoothed(nsamples, draws=noise.clone()), **kw))
    assert np.array_equal(_u64(a["vmax"]), _u64(each["vmax"])) and np.array_equal(a["run_prob"], (each["nruns"] >= 1).mean(axis=0))
    with pytest.raises(ValueError, match="limit_kmh must be None, a scalar or have shape"):
        batch.speed_statistics(db, nsamples, limit_kmh=np.zeros(3))
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.speed_statistics(db, 0)
    viahb = batch.speed_statistics(hb, 3, seed=9, chunk=3, **kw)
    viadb = batch.speed_statistics(db, 3, seed=9, chunk=3, **kw)
    assert all(np.array_equal(_bits(viahb[k]), _bits(viadb[k])) for k in viadb)


@pytest.mark.gpu
def test_speed_profile_of_the_drop_in_filter():
    """UnscentedKalmanFilter.speed_profile on the committed ship 01203823: for that ship, what the batch calls give
    (DeviceBatch.speed_metrics on its smoothed track, speed_statistics with the filter's seed and one chunk)."""
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
        ukf.speed_profile()
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    plain = ukf.speed_profile(model="wgs84")
    assert plain["speed"].shape == (hb.Nmax,) and plain["vmax"] == np.nanmax(plain["speed"]) and "nruns" not in plain
    edges = np.array([0.0, 0.5 * plain["vmax"], 2.0 * plain["vmax"]])
    kw = dict(bands=edges, threshold=0.5 * plain["vmax"], above=True, min_run_h=0.25, model="wgs84")
    want = _host(db.speed_metrics(db.sm_mean, per_step=True, **kw))
    got = ukf.speed_profile(limit_kmh=0.9 * plain["vmax"], **kw)
    assert set(got) == (set(OUTPUTS) - {"track_status"}) | {"mean_speed", "exceeds"} and got["exceeds"] is True
    for k in want:
        if k != "track_status":
            assert got[k].shape == want[k].shape[1:-1] and np.array_equal(_bits(got[k]), _bits(want[k][0, ..., 0])), k
    assert got["band_time"].shape == (2,) and got["cond_time"] > 0.0 and got["mean_speed"] == got["dist"] / got["sound_time"]
    n = 5
    stats = batch.speed_statistics(hb, n, seed=3, chunk=n, limit_kmh=1.1 * plain["vmax"], **kw)
    prof = ukf.speed_profile(nsamples=n, limit_kmh=1.1 * plain["vmax"], random_state=3, **kw)
    assert set(prof) == set(stats) - {"status", "track_status", "mean_speed", "vmax"}
    for k in prof:
        assert prof[k].shape == stats[k].shape[:-1] and np.array_equal(_bits(prof[k]), _bits(stats[k][..., 0])), k
    assert 0.0 <= prof["exceed_prob"] <= 1.0 and 0.0 <= prof["run_prob"] <= 1.0
    with pytest.raises(ValueError, match="nsamples must be >= 0"):
        ukf.speed_profile(nsamples=-1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
