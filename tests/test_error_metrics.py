"""Errors of tracks on the device against truth positions (include/ste.h: ste_errors_f64, ste_track_errors_f64; DESIGN.md,
"Errors"): declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers, the host
front ends (observation_rows, hold_out, truth_course, performance_metrics) against small hand arrays, and the conditions of the
random fleet that the device comparison rests on (CPU); on the GPU the hand-made ships for both leg functions, the fleet against
the restatement with and without injected faults, independence of the surroundings bit for bit, sum_err == cumerr[nsteps], the
Python front ends on a real run of the committed ship, and the refusals on the device build."""
import ctypes as C
import dataclasses
import os
import re

import error_cases as erc
import numpy as np
import path_metrics_cases as pmc
import pytest
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "truth", "course", "cov", "cov_rows", "reserved", "nees_limit", "sum_err", "sum_sq", "max_err",
          "sum_along", "sum_along_sq", "sum_cross", "sum_cross_sq", "sum_nees", "n", "max_row", "nbroken", "ncoursed", "nscored",
          "ninside", "err", "cumerr", "along", "cross", "nees"]
OUTPUTS = FIELDS[9:]
MODELS = ("sphere", "wgs84")


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
    proto = r"int ste_track_errors_f64\(const ste_ukf_batch_f64\* b, const ste_errors_f64\* er, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_errors_f64 {"): hdr.index("} ste_errors_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteErrorsF64._fields_] == FIELDS
    # the layout of the C struct by hand: nstates and model share a word, the four input pointers take one each, cov_rows and
    # reserved share one, nees_limit and every output pointer take one
    offsets = {"nstates": 0, "model": 4, "states": 8, "truth": 16, "course": 24, "cov": 32, "cov_rows": 40, "reserved": 44,
               "nees_limit": 48}
    offsets.update({name: 56 + 8 * k for k, name in enumerate(OUTPUTS)})
    assert {f: getattr(binding.SteErrorsF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteErrorsF64) == 208 and re.search(r"} ste_errors_f64;\s*/\* 208 bytes \*/", hdr)
    assert "ste_track_errors_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_track_errors_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert "(ste_track_errors_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the error arguments travel beside the batch
    assert int(re.search(r"#define STE_ERRORS_COV_FULL (\d+)", hdr).group(1)) == binding.STE_ERRORS_COV_FULL == 16
    assert int(re.search(r"#define STE_ERRORS_COV_PACKED (\d+)", hdr).group(1)) == binding.STE_ERRORS_COV_PACKED == 10
    comment = hdr[hdr.index("ERRORS:"): hdr.index("#define STE_ERRORS_COV_FULL")]
    for word in ("Rows.", "Error.", "Sums", "Along and cross", "NEES", "Row outputs.", "TRUTHED", "BROKEN", "SOUND", "COURSED", "SCORED",
                 "first row wins", "without contraction", "FROM the truth", "TO the state", "wrap180", "det = a * c - b * b",
                 "2.0 * b * dx * dy", "cumerr row nsteps[t] bit for bit", "positive to starboard", "ahead of the truth", "No tolerance",
                 "no dt", "Refused with STE_EINVAL"):
        assert word in comment, word


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The device pointers below are not memory: nothing may be launched, with a GPU or without one."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.nsteps = 0x2000  # no dt: the call reads none
        return s

    def good_errors():
        e = binding.SteErrorsF64()
        e.nstates, e.model, e.states, e.truth, e.course, e.cov = 1, binding.STE_PREP_WGS84, 0x3000, 0x4000, 0x5000, 0x6000
        e.cov_rows, e.reserved, e.nees_limit = 10, 0, 5.99
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x10000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_errors()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc = lib.ste_track_errors_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_track_errors_f64" in msg, (fields, rc, msg)

    for s, e, reason in ((None, good_errors(), "batch pointer is NULL"), (good_batch(), None, "error arguments (er) are NULL")):
        assert lib.ste_track_errors_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_track_errors_f64" in msg
    refused("er->states is required", states=None)
    refused("er->truth is required", truth=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    no_nees = {k: None for k in erc.NEES_OUTPUTS}
    refused("limited to 65535", nstates=65536, cov=None, **no_nees)
    for m in (-1, 2, 7):
        refused("STE_PREP_SPHERE or STE_PREP_WGS84", model=m)
    for r in (0, 4, 15, 17, -10):
        refused("cov_rows must be 16", cov_rows=r)
    for n in (2, 3, 65535):
        refused("er->cov needs nstates == 1", nstates=n)
    for v in (float("nan"), float("inf"), 0.0, -1.0):
        refused("nees_limit must be finite and > 0", nees_limit=v)
    for k in erc.COURSE_OUTPUTS:  # one along / cross output is enough
        refused("needs er->course", course=None, **{o: None for o in erc.COURSE_OUTPUTS if o != k})
    for k in erc.NEES_OUTPUTS:  # one NEES output is enough
        refused("needs er->cov", cov=None, **{o: None for o in erc.NEES_OUTPUTS if o != k})
    for r in (1, -1):
        refused("er->reserved must be 0", reserved=r)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def _hand_restatement(model):
    h = erc.hand_batch()
    return erc.track_errors(h["states"], h["nsteps"], h["truth"], model, h["course"], h["cov"])


@pytest.mark.parametrize("model", MODELS)
def test_restatement_against_hand_answers(model):
    """Nine hand-made ships (error_cases.hand_batch names them): truth displaced by known degrees along the equator and along
    a meridian, so e = KM_PER_DEG_EQUATOR x degrees on the sphere; a state due north of the truth under courses 0 and 90; a
    diagonal covariance, q = dx^2 / a + dy^2 / c; a broken row; a row without truth that carries cumerr; a tie for the maximum;
    a track of no steps; a track with no truth; 179.9 against -179.9."""
    erc.check_hand_answers(_hand_restatement(model), model, f"restatement, {model}")


def _small_batch():
    """Three tracks of four steps with hand-made update columns: track 0 updates at every step (columns 1 .. 4), track 1 at
    steps 1 and 3 (columns 1 and 2), track 2 never; column 9 of step 2 of track 2 lies past Tmax = 5."""
    from track_estimators import batch

    N, B, T = 4, 3, 5
    z = np.zeros((T, 4, B))
    z[:, 0], z[:, 1] = 100.0 * np.arange(B)[None] + np.arange(T)[:, None], -(10.0 * np.arange(B)[None] + np.arange(T)[:, None])
    upd = np.full((N, B), -1, dtype=np.int32)
    upd[:, 0] = [1, 2, 3, 4]
    upd[[1, 3], 1] = [1, 2]
    upd[2, 2] = 9
    zero = np.zeros((N, B))
    return batch.HostBatch(B=B, Nmax=N, Tmax=T, H=np.eye(4), Q=np.eye(4), R=np.eye(4), nsteps=np.full(B, N, dtype=np.int32),
                           x0=np.zeros((4, B)), P0=np.eye(4).reshape(16), dt=zero + 1.0, sog_rate=zero, cog_rate=zero.copy(),
                           sog_rate_rts=None, cog_rate_rts=None, upd_idx=upd, z=z)


def test_observation_rows_and_hold_out():
    from track_estimators import batch

    hb = _small_batch()
    rows = batch.observation_rows(hb)
    assert rows.shape == (5, 2, 3)
    assert np.array_equal(rows[:, 0, 0], [0.0, 1.0, 2.0, 3.0, 4.0]) and np.array_equal(rows[:, 1, 0], [-0.0, -1.0, -2.0, -3.0, -4.0])
    assert np.array_equal(rows[:, 0, 1], [100.0, np.nan, 101.0, np.nan, 102.0], equal_nan=True)
    assert np.array_equal(rows[:, 1, 1], [-10.0, np.nan, -11.0, np.nan, -12.0], equal_nan=True)
    assert rows[0, 0, 2] == 200.0 and np.isnan(rows[1:, :, 2]).all()  # the column past Tmax is no observation
    bare = batch.observation_rows(dataclasses.replace(hb, initial_update=False))
    assert np.isnan(bare[0]).all() and np.array_equal(bare[1:], rows[1:], equal_nan=True)
    other = np.full((4, 3), -1)
    other[0, 2] = 4
    assert batch.observation_rows(hb, other)[1, 0, 2] == 204.0 and np.isnan(batch.observation_rows(hb, other)[2:]).all()
    with pytest.raises(ValueError, match="upd_idx must have shape"):
        batch.observation_rows(hb, np.zeros((3, 3), dtype=np.int32))
    fires = (hb.upd_idx >= 0) & (hb.upd_idx < hb.Tmax)
    for every, offset in ((2, 0), (2, 1), (3, 1), (1, 0)):
        thin, truth = batch.hold_out(hb, every, offset)
        assert thin is not hb and thin.upd_idx is not hb.upd_idx and thin.upd_idx.dtype == hb.upd_idx.dtype
        kept = (thin.upd_idx >= 0) & (thin.upd_idx < hb.Tmax)
        withheld = np.isfinite(truth[1:, 0])
        # the withheld and the kept updates partition the original ones, and the kept ones keep their columns
        assert np.array_equal(kept | withheld, fires) and not (kept & withheld).any()
        assert np.array_equal(thin.upd_idx[~withheld], hb.upd_idx[~withheld]) and (thin.upd_idx[withheld] == -1).all()
        both = np.broadcast_to(withheld[:, None], truth[1:].shape)
        assert np.array_equal(truth[1:][both], rows[1:][both]) and np.isnan(truth[1:][~both]).all()
        assert np.isnan(truth[0]).all() and thin.initial_update  # the initial update stays and is no truth
        for t in range(hb.B):  # ordinals in step order
            steps = np.flatnonzero(fires[:, t])
            assert np.array_equal(np.flatnonzero(withheld[:, t]), steps[offset::every]), (every, offset, t)
        assert thin.z is hb.z and thin.sog_rate is hb.sog_rate  # what it does not withhold
    thin, truth = batch.hold_out(hb, 1)
    assert (thin.upd_idx[fires] == -1).all() and np.array_equal(np.isfinite(truth[1:, 0]), fires)  # every = 1 withholds all
    assert "sog_rate" in batch.hold_out.__doc__ and "cog_rate" in batch.hold_out.__doc__ and "packs the batch again" in batch.hold_out.__doc__
    for every, offset in ((0, 0), (2, 2), (2, -1)):
        with pytest.raises(ValueError, match="every must be >= 1 and 0 <= offset < every"):
            batch.hold_out(hb, every, offset)


def test_truth_course_without_a_device():
    """What truth_course answers without ste_track_prep_f64: a track with fewer than two rows of truth has no course, and a
    truth array of another shape is refused.  The hand arrays with courses are in the GPU part: the course IS the prepared COG."""
    from track_estimators import batch

    truth = np.full((5, 2, 3), np.nan)
    truth[2, :, 1] = [10.0, 20.0]  # one row of truth
    truth[3, 0, 2], truth[4, 1, 2] = 1.0, 2.0  # two half rows: no row of truth
    got = batch.truth_course(truth)
    assert got.shape == (5, 3) and np.isnan(got).all()
    with pytest.raises(ValueError, match="truth must have shape"):
        batch.truth_course(np.zeros((5, 3)))
    with pytest.raises(ValueError, match="model must be one of"):
        batch.truth_course(truth, model="flat")


def test_performance_metrics():
    import track_estimators
    from track_estimators import performance_metrics as perf

    assert "performance_metrics" in track_estimators.__all__ and perf.__all__ == ["rmse", "cum_abs_diff", "abs_diff"]
    x, ref = np.array([1.0, -2.0, 4.0, 0.5]), np.array([0.0, 2.0, 4.0, -1.5])
    assert np.array_equal(perf.abs_diff(x, ref), [1.0, 4.0, 0.0, 2.0])
    assert np.array_equal(perf.cum_abs_diff(x, ref), [1.0, 5.0, 5.0, 7.0])
    assert perf.rmse(x, ref) == np.sqrt((1.0 + 16.0 + 0.0 + 4.0) / 4.0) and isinstance(perf.rmse(x, ref), float)
    assert np.array_equal(perf.abs_diff([[1.0, 2.0], [3.0, 5.0]], [1.0, 1.0]), [[0.0, 1.0], [2.0, 4.0]])  # broadcast to one shape
    assert perf.rmse([3.0, 3.0], 0.0) == 3.0 and np.array_equal(perf.cum_abs_diff([[1.0, 2.0], [3.0, 5.0]], 0.0), [1.0, 3.0, 6.0, 11.0])
    for f in (perf.abs_diff, perf.cum_abs_diff, perf.rmse):
        with pytest.raises(ValueError, match="must broadcast to one shape"):
            f(np.zeros(3), np.zeros(4))


@pytest.mark.parametrize("model", MODELS)
def test_conditions_of_the_fleet(model):
    """What the device comparison assumes of the fleet (S = 3, Nmax = 37, B = 70, every nsteps from 0 to 37); all of it holds by
    construction and is asserted here, so no case is left out of any comparison: every truthed row's truth is the state's
    position displaced by 0.001 to 3 degrees at |lat| <= 70, so every error is above 0.03 km and its heading is well
    conditioned; no two errors of a track tie for the maximum within 1e-6 relative; no q lies within 1e-6 relative of the
    limit."""
    f = erc.fleet()
    st, truth = f["states"], f["truth"]
    assert st.shape == (3, 38, 4, 70) and set(f["nsteps"].tolist()) == set(range(38))
    have = np.isfinite(truth[:, 0]) & np.isfinite(truth[:, 1])
    live = have & (np.arange(38)[:, None] <= f["nsteps"][None])
    d = np.hypot(erc.wrap180(st[:, :, 0] - truth[None, :, 0]), st[:, :, 1] - truth[None, :, 1])
    assert (d[:, live] >= 0.001).all() and (d[:, live] <= 3.0).all(), (d[:, live].min(), d[:, live].max())
    assert (np.abs(st[:, :, 1]) <= 70.0).all() and (np.abs(truth[:, 1][have]) <= 70.0).all()
    assert 0.5 < have.mean() < 0.7 and (np.isnan(f["course"]) & live).sum() > 20 and np.isfinite(f["course"][live]).sum() > 500
    ref = erc.fleet_reference(model)
    e = ref["err"]
    sound = ~np.isnan(e) & (e != erc.SENTINEL)
    assert (sound == np.broadcast_to(live[None], e.shape)).all() and not ref["nbroken"].any() and (e[sound] > 0.03).all()
    top = np.sort(np.where(sound, e, -np.inf), axis=1)[:, -2:]  # (S, 2, B): runner-up and best
    two = np.isfinite(top[:, 0])
    assert two.sum() > 150 and (top[:, 1][two] - top[:, 0][two] > erc.GAP_RTOL * top[:, 1][two]).all()
    q = erc.fleet_reference(model, sample0_cov=True)
    scored = ~np.isnan(q["nees"]) & (q["nees"] != erc.SENTINEL)
    gap = np.abs(q["nees"][scored] - erc.LIMIT95) / erc.LIMIT95
    print(f"fleet, {model}: {int(sound.sum())} sound rows, least error {e[sound].min():.3g} km, {int(scored.sum())} scored rows, "
          f"{int(q['ninside'].sum())} inside, least gap of q to the limit {gap.min():.3g}")
    assert gap.min() > erc.GAP_RTOL and (q["nscored"] == q["n"]).all()
    assert 0.2 < q["ninside"].sum() / q["nscored"].sum() < 0.8  # q on both sides of the limit
    assert np.array_equal(f["cov10"], f["cov16"][:, [0, 1, 2, 3, 5, 6, 7, 10, 11, 15]])


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bare(nsteps, N):
    from track_estimators import batch

    return batch.DeviceBatch(pmc.bare_batch(nsteps, np.ones((N, len(nsteps)))), histories=False)


def _abi_call(db, states, truth, model="sphere", course=None, cov=None, want=OUTPUTS, limit=erc.LIMIT95):
    """ste_track_errors_f64 through ctypes on contiguous device tensors ((S, N+1, 4, B), (N+1, 2, B), (N+1, B), (N+1, 16 or 10, B));
    ``want``: the outputs asked for (the others are NULL), pre-filled with SENTINEL / -7; -> dict of NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    S, N, B = int(states.shape[0]), int(states.shape[1]) - 1, int(states.shape[3])
    er = binding.SteErrorsF64()
    er.nstates, er.model, er.states = S, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model], states.data_ptr()
    er.truth = truth.data_ptr()
    er.course = None if course is None else course.data_ptr()
    if cov is not None:
        er.cov, er.cov_rows, er.nees_limit = cov.data_ptr(), int(cov.shape[1]), limit
    out = {}
    for k in want:
        shape = (S, N + 1, B) if k in erc.ROW_OUTPUTS else (S, B)
        out[k] = torch.full(shape, -7, dtype=torch.int32, device=db.device) if k in erc.INT_OUTPUTS else \
            torch.full(shape, erc.SENTINEL, dtype=torch.float64, device=db.device)
        setattr(er, k, out[k].data_ptr())
    binding.check(db.lib.ste_track_errors_f64(C.byref(db.struct), C.byref(er), db._stream(None)), "ste_track_errors_f64")
    torch.cuda.synchronize()
    return _host(out)


def _compare(got, ref, what):
    """The device against the restatement.  Bit for bit: the counts, max_row, the NaN patterns and the untouched rows.  Within
    pmc.DIST_RTOL / DIST_ATOL, the project's tolerance for the same leg functions: err, max_err, and cumerr and sum_err (sums of
    non-negative legs keep the relative error).  sum_sq: d(e^2) = 2 e de with de <= ATOL + RTOL e, summed over n rows, is at most
    2 (ATOL n max_err + RTOL sum_sq): the tolerance scaled by max_err.  along and cross: |delta| <= ATOL + RTOL e of the row, scaled
    by the error and not by the component (the heading agrees to 1e-10 degrees where tests/test_track_prep.py::compare allows
    atol 1e-10 and rtol 1e-11 for cog, and 1e-10 degrees turn a vector of length e by 1.7e-12 e); their sums n ATOL + RTOL sum_err,
    their sums of squares as sum_sq.  nees and sum_nees (positive terms): rtol 1e-10, the project's tolerance for such a quotient.
    Every figure is printed before it is judged."""
    n, sum_err, sum_sq, max_err = ref["n"], ref["sum_err"], ref["sum_sq"], np.nan_to_num(ref["max_err"])
    square = 2.0 * (pmc.DIST_ATOL * n * max_err + pmc.DIST_RTOL * sum_sq)
    for k, g in got.items():
        r = ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        if k in erc.INT_OUTPUTS:
            assert np.array_equal(g, r), (what, k, np.argwhere(g != r)[:5].tolist())
            continue
        nan, left = np.isnan(r), r == erc.SENTINEL
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(g == erc.SENTINEL, left), (what, k, "NaN pattern or untouched rows")
        if k in ("err", "cumerr", "sum_err", "max_err"):
            tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(r)
        elif k in ("along", "cross"):
            tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref["err"])
        elif k in ("sum_along", "sum_cross"):
            tol = pmc.DIST_ATOL * np.maximum(n, 1) + pmc.DIST_RTOL * sum_err
        elif k in ("sum_sq", "sum_along_sq", "sum_cross_sq"):
            tol = np.maximum(square, 1e-300)
        else:
            assert k in ("nees", "sum_nees"), k
            tol = 1e-10 * np.abs(r)
        ok = ~nan & ~left
        frac = (np.abs(g - r)[ok] / np.broadcast_to(np.maximum(tol, 1e-300), r.shape)[ok])
        worst = float(frac.max()) if frac.size else 0.0
        print(f"{what}: {k} deviates by at most {worst:.3g} of its tolerance ({frac.size} values)")
        assert worst <= 1.0, (what, k, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_hand_made_ships_on_the_device(model):
    """The nine hand-made ships through the C ABI: the known answers, and the restatement."""
    h = erc.hand_batch()
    db = _bare(h["nsteps"], 3)
    got = _abi_call(db, _dev(db, h["states"]), _dev(db, h["truth"]), model, _dev(db, h["course"]), _dev(db, h["cov"]))
    erc.check_hand_answers(got, model, f"device, {model}")
    _compare(got, _hand_restatement(model), f"hand-made ships, {model}")


def _fleet_batch(f=None):
    f = erc.fleet() if f is None else f
    db = _bare(f["nsteps"], erc.FLEET_N)
    return f, db, {k: _dev(db, v) for k, v in f.items() if k != "nsteps"}


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_fleet_against_the_restatement(model):
    """S = 3, Nmax = 37, B = 70 (a full wave and a partial one), nsteps 0 .. 37: the three samples with the course, sample 0 with
    course and covariance; nothing left out; and the front end, which gives NaN past nsteps where the call leaves rows alone,
    against the C ABI bit for bit.  Largest deviations measured on an MI355X, as fractions of the tolerance: err 4.3e-6, along
    0.0024 and cross 0.0033 on the sphere; err 0.017, along 0.011 and cross 0.015 on WGS84; nees has the restatement's bits."""
    f, db, d = _fleet_batch()
    want = [k for k in OUTPUTS if k not in erc.NEES_OUTPUTS]
    got = _abi_call(db, d["states"], d["truth"], model, d["course"], None, want=want)
    ref = erc.fleet_reference(model)
    assert set(got) == set(ref)
    _compare(got, ref, f"fleet, {model}")
    one = _abi_call(db, d["states"][:1].contiguous(), d["truth"], model, d["course"], d["cov16"])
    ref1 = erc.fleet_reference(model, sample0_cov=True)
    assert set(one) == set(ref1) == set(OUTPUTS)
    _compare(one, ref1, f"fleet, sample 0 with its covariance, {model}")
    front = _host(db.track_errors(d["states"][0], f["truth"], course=f["course"], cov=d["cov16"], model=model, rows=True, cumulative=True))
    for k in OUTPUTS:
        x = front[k]
        if k in erc.ROW_OUTPUTS:
            assert np.isnan(x[one[k] == erc.SENTINEL]).all(), k
            x = np.where(one[k] == erc.SENTINEL, erc.SENTINEL, x)
        assert np.array_equal(_bits(x), _bits(one[k])), (k, "front end against the C ABI")
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, v in (("rmse", np.sqrt(one["sum_sq"] / one["n"])), ("mean_err", one["sum_err"] / one["n"]),
                     ("mean_along", one["sum_along"] / one["ncoursed"]), ("rms_cross", np.sqrt(one["sum_cross_sq"] / one["ncoursed"])),
                     ("mean_nees", one["sum_nees"] / one["nscored"]), ("coverage", one["ninside"] / one["nscored"])):
            assert np.array_equal(_bits(front[k]), _bits(v)), k
    assert set(front) == set(OUTPUTS) | {"rmse", "mean_err", "mean_along", "rms_cross", "mean_nees", "coverage"}
    assert np.isnan(front["coverage"][0, one["nscored"][0] == 0]).all() and np.isnan(front["rmse"][0, one["n"][0] == 0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_fleet_with_injected_faults(model):
    """NaN and inf in the states, the truth, the course and the covariance, and covariances with det < 0, det == 0 and a <= 0:
    flags and counts bit for bit, both covariance layouts."""
    f, done = erc.faulty_fleet()
    _, db, d = _fleet_batch(f)
    ref = erc.track_errors(f["states"], f["nsteps"], f["truth"], model, f["course"], f["cov16"])
    clean = erc.fleet_reference(model, sample0_cov=True)
    kinds = {kind: (k, t) for kind, k, t in done}
    assert len(kinds) == 13
    for kind, (k, t) in kinds.items():
        broken, truthless = kind.startswith("state"), kind.startswith("truth")
        assert np.isnan(ref["err"][0, k, t]) == (broken or truthless), kind
        assert ref["nbroken"][0, t] == int(broken) and ref["n"][0, t] == clean["n"][0, t] - int(broken or truthless), kind
        assert np.isnan(ref["along"][0, k, t]) == (broken or truthless or kind.startswith("course")), kind
        assert np.isnan(ref["nees"][0, k, t]) == (not kind.startswith("course")), kind
    assert ref["nbroken"].sum() == 3 and ref["n"].sum() == clean["n"].sum() - 5
    assert ref["ncoursed"].sum() == clean["ncoursed"].sum() - 7 and ref["nscored"].sum() == clean["nscored"].sum() - 11
    for cov in ("cov16", "cov10"):
        got = _abi_call(db, d["states"], d["truth"], model, d["course"], d[cov])
        _compare(got, ref, f"faulty fleet, {model}, {cov}")


def _same_bits(a, b, what, keys, track_b=slice(None), sample_b=slice(None)):
    """``a`` against ``b`` restricted to the given tracks and samples (of ``b``)."""
    for k in keys:
        x, y = a[k], b[k][sample_b][..., track_b]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_same_bits_whatever_the_surroundings(model):
    """Bit for bit: S = 1 slices against S = 3; the fleet as columns 64 .. 133 of a fleet 150 tracks wide, read in place
    (track_stride) and as a contiguous copy; either covariance layout; each output alone against all together."""
    f, db, d = _fleet_batch()
    kw = dict(course=d["course"], model=model, rows=True, cumulative=True)
    whole = _host(db.track_errors(d["states"], d["truth"], **kw))
    keys = [k for k in OUTPUTS if k not in erc.NEES_OUTPUTS]
    assert set(keys) <= set(whole)
    for s in range(erc.FLEET_S):
        one = _host(db.track_errors(d["states"][s], d["truth"], **kw))
        _same_bits(one, whole, f"sample {s} alone", keys, sample_b=slice(s, s + 1))
    scored = _host(db.track_errors(d["states"][0], d["truth"], cov=d["cov16"], **kw))
    _same_bits(scored, whole, "sample 0 with its covariance", keys, sample_b=slice(0, 1))
    packed = _host(db.track_errors(d["states"][0], d["truth"], cov=d["cov10"], **kw))
    _same_bits(packed, scored, "packed covariance against full", list(scored))
    # the fleet inside a wider one: other tracks (of other lengths) around it
    lo, hi = erc.FLEET_COLS
    W, N = erc.FLEET_WIDE, erc.FLEET_N
    rng = np.random.default_rng(5)
    nsteps = rng.integers(0, N + 1, W).astype(np.int32)
    nsteps[lo:hi] = f["nsteps"]
    wide_db = _bare(nsteps, N)
    wide = {}
    for k, v in f.items():
        if k != "nsteps":
            a = rng.uniform(-60.0, 60.0, v.shape[:-1] + (W,))
            a[..., lo:hi] = v
            wide[k] = _dev(wide_db, a)
    win = wide_db.window(lo, hi)
    assert int(win.struct.track_stride) == W and win.ntracks == erc.FLEET_B
    view = {k: v[..., lo:hi] for k, v in wide.items()}
    for copied in (False, True):
        st = view["states"].contiguous() if copied else view["states"]
        got = _host(win.track_errors(st, view["truth"], course=view["course"], model=model, rows=True, cumulative=True))
        _same_bits(got, whole, f"window, copied={copied}", keys)
        got = _host(win.track_errors(st[0], f["truth"], course=f["course"], cov=view["cov10"], model=model, rows=True, cumulative=True))
        _same_bits(got, scored, f"window with covariance, copied={copied}", list(scored))
    # any subset of the outputs: each alone, and three mixed ones, against all together
    s0 = d["states"][:1].contiguous()
    base = _abi_call(db, s0, d["truth"], model, d["course"], d["cov16"])
    for want in [(k,) for k in OUTPUTS] + [("sum_err", "cumerr"), ("n", "along", "ninside"), ("max_row", "sum_cross_sq", "nees")]:
        got = _abi_call(db, s0, d["truth"], model, d["course"] if set(want) & set(erc.COURSE_OUTPUTS) else None,
                        d["cov16"] if set(want) & set(erc.NEES_OUTPUTS) else None, want=want)
        _same_bits(got, base, f"outputs {want}", want)
    with pytest.raises(ValueError, match="cov goes with one track per ship"):
        db.track_errors(d["states"], d["truth"], cov=d["cov16"])
    with pytest.raises(ValueError, match="truth must be float64 of shape"):
        db.track_errors(d["states"], f["truth"][:, :1])
    with pytest.raises(ValueError, match="course must be float64 of shape"):
        db.track_errors(d["states"], d["truth"], course=f["course"][:-1])
    with pytest.raises(ValueError, match="cov must be float64 of shape"):
        db.track_errors(d["states"][0], d["truth"], cov=f["cov16"][:, :12])
    with pytest.raises(ValueError, match="coverage must lie strictly between 0 and 1"):
        db.track_errors(d["states"][0], d["truth"], cov=d["cov16"], coverage=1.0)
    with pytest.raises(ValueError, match="this batch holds no such covariance"):
        db.track_errors(d["states"][0], d["truth"], cov="sm")
    with pytest.raises(ValueError, match="model must be one of"):
        db.track_errors(d["states"], d["truth"], model="flat")


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_sum_err_is_the_last_cumerr_and_zero_against_itself(model):
    """sum_err == cumerr[nsteps] bit for bit; with truth = the states every sum is exactly 0 and n counts the rows."""
    f, db, d = _fleet_batch()
    got = _abi_call(db, d["states"], d["truth"], model, d["course"], None, want=[k for k in OUTPUTS if k not in erc.NEES_OUTPUTS])
    last = got["cumerr"][:, f["nsteps"], np.arange(erc.FLEET_B)]
    assert np.array_equal(_u64(got["sum_err"]), _u64(last)) and (got["sum_err"][got["n"] > 0] > 0.0).all()
    own = d["states"][0, :, :2].contiguous()
    zero = _abi_call(db, d["states"][:1].contiguous(), own, model, d["course"], d["cov16"])
    assert np.array_equal(zero["n"][0], f["nsteps"] + 1) and not zero["nbroken"].any() and (zero["max_row"] == 0).all()
    for k in erc.SUMS + erc.COURSE_SUMS + ("sum_nees",):
        assert np.array_equal(_u64(zero[k]), _u64(np.zeros_like(zero[k]))), k
    assert np.array_equal(zero["nscored"][0], f["nsteps"] + 1) and np.array_equal(zero["ninside"], zero["nscored"])
    live = zero["err"] != erc.SENTINEL
    assert (zero["err"][live] == 0.0).all() and (zero["cumerr"][live] == 0.0).all() and (zero["nees"][live] == 0.0).all()


@pytest.mark.gpu
def test_truth_course_is_the_prepared_cog():
    """truth_course against hand arrays: along the equator eastwards 90, up a meridian 0, the last truthed row takes its
    predecessor's, rows without truth and tracks with fewer than two truthed rows NaN; and it is prepare_observations' cog of
    the compacted rows, bit for bit."""
    from track_estimators import batch

    truth = np.full((6, 2, 4), np.nan)
    truth[[0, 2, 5], 0, 0], truth[[0, 2, 5], 1, 0] = [10.0, 11.0, 13.0], 0.0  # eastwards along the equator
    truth[[1, 2, 3, 4], 0, 1], truth[[1, 2, 3, 4], 1, 1] = 20.0, [30.0, 31.0, 32.0, 31.5]  # north, north, then south
    truth[3, :, 2] = [5.0, 5.0]  # one row: no course
    for model in MODELS:
        got = batch.truth_course(truth, model=model)
        assert got.shape == (6, 4)
        assert np.allclose(got[[0, 2, 5], 0], 90.0, atol=1e-9) and np.isnan(got[[1, 3, 4], 0]).all()
        assert np.allclose(got[[1, 2], 1], 0.0, atol=1e-9) and np.allclose(got[[3, 4], 1], 180.0, atol=1e-9) and np.isnan(got[[0, 5], 1]).all()
        assert np.isnan(got[:, 2:]).all()
        prep = batch.prepare_observations([truth[[0, 2, 5], 0, 0]], [truth[[0, 2, 5], 1, 0]], [np.ones(2)], model=model)[0]["cog"]
        assert np.array_equal(_u64(got[[0, 2, 5], 0]), _u64(prep))


def _golden_filter():
    """The committed ship 01203823 through the drop-in filter: (ukf, its packed batch)."""
    from conftest import GOLDEN, load_cases
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
    return ukf, c, st


@pytest.mark.gpu
def test_front_ends_on_a_real_run():
    """The committed ship through the filter and the smoother.  track_errors(sm_mean, observation_rows(hb), cov="sm") is the
    restatement on the downloaded arrays; hold_out -> run -> track_errors gives an rmse against the withheld reports that is
    larger than the rmse against the used ones; error_statistics with chunk 2 equals chunk 8 for given draws bit for bit, and its
    mean of rmse is the direct mean over sample_smoothed + track_errors (rtol 1e-13 for means, 1e-10 for std, as in
    tests/test_speed_metrics.py)."""
    from track_estimators import batch

    ukf, c, st = _golden_filter()
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    torch = db.torch
    truth = batch.observation_rows(hb)
    course = batch.truth_course(truth)
    assert np.isfinite(truth[:, 0, 0]).sum() >= 6 and np.array_equal(np.isfinite(course), np.isfinite(truth[:, 0]))
    got = _host(db.track_errors(db.sm_mean, truth, course=course, cov="sm", rows=True, cumulative=True))
    sm, cov = db.sm_mean.cpu().numpy()[None], db.sm_cov.cpu().numpy()
    assert cov.shape[1] == 10
    ref = erc.track_errors(sm, hb.nsteps, truth, "sphere", course, cov)
    for k in erc.ROW_OUTPUTS:
        ref[k] = np.where(ref[k] == erc.SENTINEL, np.nan, ref[k])
    _compare({k: got[k] for k in OUTPUTS}, ref, "the smoothed ship against its own reports")
    assert got["n"][0, 0] == np.isfinite(truth[:, 0, 0]).sum() and got["nscored"][0, 0] == got["n"][0, 0]
    assert 0.0 <= got["coverage"][0, 0] <= 1.0 and got["rmse"][0, 0] > 0.0
    # withheld reports are further from the track than used ones
    thin, held = batch.hold_out(hb, 3, 1)
    tdb = batch.DeviceBatch(thin)
    tdb.run()
    assert not tdb.status_host().any()
    against_held = _host(tdb.track_errors(tdb.sm_mean, held, cov="sm"))
    against_used = _host(tdb.track_errors(tdb.sm_mean, batch.observation_rows(thin), cov="sm"))
    assert against_held["n"][0, 0] + against_used["n"][0, 0] == got["n"][0, 0] and against_held["n"][0, 0] >= 2
    print(f"rmse against the withheld reports {against_held['rmse'][0, 0]:.4g} km ({against_held['n'][0, 0]} rows, coverage "
          f"{against_held['coverage'][0, 0]:.3g}), against the used ones {against_used['rmse'][0, 0]:.4g} km "
          f"({against_used['n'][0, 0]} rows, coverage {against_used['coverage'][0, 0]:.3g})")
    assert against_held["rmse"][0, 0] > against_used["rmse"][0, 0]
    # posterior samples
    nsamples = 7
    noise = torch.randn((nsamples, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(db.device)
    fill = lambda buf, first: buf.copy_(noise[first:first + buf.shape[0]])  # noqa: E731
    kw = dict(course=course, within_km=float(got["rmse"][0, 0]) * 2.0, quantiles=(0.25, 0.5), rows=True)
    a = batch.error_statistics(db, truth, nsamples, chunk=2, draws=fill, **kw)
    b = batch.error_statistics(db, truth, nsamples, chunk=8, draws=fill, **kw)
    assert set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    direct = _host(db.track_errors(db.sample_smoothed(nsamples, draws=noise.clone()), truth, rows=True))
    assert np.array_equal(_u64(a["rmse"]), _u64(direct["rmse"]))
    assert np.allclose(a["rmse_mean"], direct["rmse"].mean(axis=0), rtol=1e-13)
    assert np.allclose(a["rmse_std"], direct["rmse"].std(axis=0, ddof=1), rtol=1e-10)
    assert np.allclose(a["rmse_quantiles"], np.quantile(direct["rmse"], (0.25, 0.5), axis=0), rtol=1e-13)
    assert np.array_equal(a["within_prob"], (direct["rmse"] <= kw["within_km"]).mean(axis=0)) and 0.0 <= a["within_prob"][0] <= 1.0
    has = np.isfinite(truth[:, 0])
    assert np.allclose(a["err_rows_mean"][has], direct["err"].mean(axis=0)[has], rtol=1e-13) and np.isnan(a["err_rows_mean"][~has]).all()
    for k in ("rmse", "mean_err", "mean_along", "rms_cross", "mean_nees", "coverage"):
        assert np.array_equal(_bits(a[k + "_smoothed"]), _bits(got[k][0])), k
    assert np.array_equal(a["n"], got["n"][0]) and not a["status"].any()
    seeded = batch.error_statistics(db, truth, nsamples, seed=4, chunk=16)
    again = _host(db.track_errors(db.sample_smoothed(nsamples, seed=4), truth))
    assert np.array_equal(_u64(seeded["rmse"]), _u64(again["rmse"]))
    assert not {"within_prob", "rmse_quantiles", "err_rows_mean", "mean_along_smoothed"} & set(seeded)
    viahb = batch.error_statistics(hb, truth, 3, seed=9, chunk=3)
    viadb = batch.error_statistics(db, truth, 3, seed=9, chunk=3)
    assert all(np.array_equal(_bits(viahb[k]), _bits(viadb[k])) for k in viadb)
    with pytest.raises(ValueError, match="within_km must be None, a scalar or have shape"):
        batch.error_statistics(db, truth, nsamples, within_km=np.zeros(3))
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.error_statistics(db, truth, 0)


@pytest.mark.gpu
def test_track_error_of_the_drop_in_filter():
    """UnscentedKalmanFilter.track_error on the committed ship: for that ship, what the batch calls give."""
    from track_estimators import batch

    ukf, c, st = _golden_filter()
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.track_error()
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    truth = batch.observation_rows(hb)
    course = batch.truth_course(truth, model="wgs84")
    want = _host(db.track_errors(db.sm_mean, truth, course=course, cov="sm", model="wgs84", rows=True, cumulative=True))
    own = ukf.track_error(course=course[:, 0], model="wgs84")  # truth=None: the ship track's own observations
    given = ukf.track_error(truth=truth[:, :, 0], course=course[:, 0], model="wgs84")
    assert set(own) == set(given) == set(want)
    for k in want:
        assert own[k].shape == want[k].shape[1:-1] and np.array_equal(_bits(own[k]), _bits(want[k][0, ..., 0])), k
        assert np.array_equal(_bits(given[k]), _bits(own[k])), k
    assert own["err"].shape == (hb.Nmax + 1,) and own["rmse"] > 0.0 and "mean_along" not in ukf.track_error()
    n = 5
    stats = batch.error_statistics(hb, truth, n, seed=3, chunk=n, course=course, within_km=10.0)
    prof = ukf.track_error(n_samples=n, course=course[:, 0], within_km=10.0, random_state=3)
    assert set(prof) == set(stats) - {"status"}
    for k in prof:
        assert prof[k].shape == stats[k].shape[:-1] and np.array_equal(_bits(prof[k]), _bits(stats[k][..., 0])), k
    assert prof["rmse"].shape == (n,) and 0.0 <= prof["within_prob"] <= 1.0
    with pytest.raises(ValueError, match="n_samples must be >= 0"):
        ukf.track_error(n_samples=-1)
    with pytest.raises(ValueError, match="truth must be None or have shape"):
        ukf.track_error(truth=np.zeros((3, 2)))


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
