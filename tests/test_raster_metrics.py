"""The values of a gridded field along device tracks (include/ste.h: ste_raster_f64, ste_raster_metrics_f64; DESIGN.md,
"Rasters"): declaration and layout of the C ABI, the refusals of the call and of the front end, the Python restatement against
the grid's restatement (the two walks are dual: one adds to every cell, the other reads it) and against hand answers, and its
identity (CPU); on the GPU the restatement bit for bit on the hand-made tracks and on the ragged fleet, the duality with the
grid kernel as integer equalities, independence of the surroundings, a map fed back on the device, the posterior statistics
and the drop-in class.  Ticks are integers and every floating-point sum is ordered: every GPU comparison is an equality."""
import ctypes as C
import os
import re

import grid_metrics_cases as gmc
import numpy as np
import path_metrics_cases as pmc
import pytest
import raster_cases as rc
from conftest import ROOT

FIELDS = ["nstates", "flags", "states", "nx", "ny", "lon0", "lat0", "dlon", "dlat", "lon_ref", "values", "threshold", "min_ticks",
          "total", "outside", "nbroken", "valid", "nodata", "wsum", "vmin", "vmax", "tmin", "tmax", "hit_ticks", "hit_first",
          "nhit", "nhit_long", "hit_longest", "row_value"]
OUTPUTS = rc.INT64 + rc.INT32 + rc.FLOAT
T20, T19 = 1 << 20, 1 << 19


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_raster_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_raster_f64\* r, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_raster_f64 {"): hdr.index("} ste_raster_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for names in re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+(?:\s*,\s*\w+)*)\s*;", body):
        fields += [n.strip() for n in names.split(",")]
    assert fields == [f[0] for f in binding.SteRasterF64._fields_] == FIELDS
    # the layout of the C struct by hand: two 32-bit integers share a word, every pointer, double and int64 takes one
    offsets = {"nstates": 0, "flags": 4, "states": 8, "nx": 16, "ny": 20}
    offsets.update({f: 24 + 8 * i for i, f in enumerate(FIELDS[5:])})
    assert offsets["values"] == 64 and offsets["min_ticks"] == 80 and offsets["total"] == 88 and offsets["row_value"] == 208
    assert {f: getattr(binding.SteRasterF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteRasterF64) == 216 and "216 bytes" in hdr[hdr.index("} ste_raster_f64;"):][:60]
    assert "ste_raster_metrics_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_raster_metrics_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert "(ste_raster_metrics_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264 and C.sizeof(binding.SteGridF64) == 104  # unchanged
    assert int(re.search(r"#define STE_RASTER_BELOW 0x(\d+)u", hdr).group(1), 16) == binding.STE_RASTER_BELOW == 2
    assert int(re.search(r"#define STE_RASTER_NO_THRESHOLD 0x(\d+)u", hdr).group(1), 16) == binding.STE_RASTER_NO_THRESHOLD == 4
    assert binding.STE_GRID_PERIODIC_LON == 1  # the third flag of ste_raster_f64.flags
    comment = hdr[hdr.index("RASTERS:"): hdr.index("#define STE_RASTER_BELOW")]
    for word in ("Raster.", "Track.", "Runs.", "Threshold.", "NO DATA", "START", "VALID", "HIT", "EXCURSION", "word for word",
                 "valid + nodata + outside = total", "not contracted", "if (!(vmin <= v))", "row_value[s][k][t]", "ties to x"):
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

    def good_raster():
        g = binding.SteRasterF64()
        g.nstates, g.flags, g.states, g.nx, g.ny = 3, 0, 0x3000, 32, 24
        g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref = 172.0, -3.0, 0.5, 0.25, 180.0
        g.values, g.threshold, g.min_ticks = 0x4000, 1.0, 0
        for i, name in enumerate(FIELDS[13:]):
            setattr(g, name, 0x10000 + 0x1000 * i)
        return g

    def refused(reason, **fields):
        s, g = good_batch(), good_raster()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(g, name) else g, name, value)
        rc_ = lib.ste_raster_metrics_f64(ref(s), ref(g), None)
        msg = lib.ste_last_error().decode()
        assert rc_ == -1 and reason in msg and "ste_raster_metrics_f64" in msg, (fields, rc_, msg)

    for s, g, reason in ((None, good_raster(), "batch pointer is NULL"), (good_batch(), None, "raster arguments (r) are NULL")):
        assert lib.ste_raster_metrics_f64(ref(s), ref(g), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_raster_metrics_f64" in msg
    # the grid call's
    refused("r->states is required", states=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1):
        refused("nx and r->ny must be >= 1", nx=n)
        refused("nx and r->ny must be >= 1", ny=n)
    refused("STE_GRID_MAX_CELLS", nx=8193, ny=8192, dlon=0.001)
    refused("STE_GRID_MAX_CELLS", nx=1 << 30, ny=1 << 30, dlon=1e-6)  # the product does not fit 32 bits
    for bad in (float("nan"), float("inf"), -float("inf")):
        for name in ("lon0", "lat0", "lon_ref"):
            refused("must be finite", **{name: bad})
        for name in ("dlon", "dlat"):
            refused("finite and >= 1e-6", **{name: bad})
    for bad in (0.0, -0.5, 9e-7):
        for name in ("dlon", "dlat"):
            refused("finite and >= 1e-6", **{name: bad})
    per = dict(flags=binding.STE_GRID_PERIODIC_LON, lon0=-180.0, lon_ref=0.0)
    refused("nx * dlon == 360 exactly", nx=359, dlon=1.0, **per)
    refused("nx * dlon == 360 exactly", nx=360, dlon=1.0000000000000002, **per)
    refused("nx * dlon == 360 exactly", **dict(per, lon0=172.0, lon_ref=180.0))  # the good grid is 16 degrees wide
    refused("within lon_ref +- 360", nx=360, dlon=1.0, **dict(per, lon_ref=181.0))
    refused("within lon_ref +- 90", nx=360, dlon=1.0, lon0=-180.0, lon_ref=0.0)  # the globe without the flag
    refused("within lon_ref +- 90", nx=361)
    refused("within lon_ref +- 90", lon_ref=90.0)
    refused("within lon_ref +- 90", lon_ref=270.0)
    refused("batch's dt is required", dt=None)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
    # its own
    refused("r->values is required", values=None)
    for f in (0x8, 0x10, 0x80000000, 0xF):
        refused("unknown bits", flags=f)
    refused("threshold is NaN", threshold=float("nan"))
    refused("threshold is NaN", threshold=float("nan"), flags=binding.STE_RASTER_BELOW)
    refused("min_ticks must be >= 0", min_ticks=-1)
    for name in rc.HIT:
        only = {k: None for k in rc.HIT if k != name}
        refused("the hit outputs", flags=binding.STE_RASTER_NO_THRESHOLD, **only)
    refused("no output asked for", **{k: None for k in FIELDS[13:]})
    no_hits = {k: None for k in rc.HIT}
    refused("no output asked for", flags=binding.STE_RASTER_NO_THRESHOLD, **{k: None for k in FIELDS[13:]})
    # what is not refused: without a threshold, a NaN threshold and a negative min_ticks are not looked at.  (Such a call
    # would launch, so it is made only where the refusals above have been seen to come first: with a refusal of its own.)
    refused("r->values is required", flags=binding.STE_RASTER_NO_THRESHOLD, threshold=float("nan"), min_ticks=-5, values=None,
            **no_hits)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_front_end_refusals():
    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    g = batch.track_grid(0.0, -0.5, 1.0, 1.0, 10, 1)
    with pytest.raises(ValueError, match="grid must be a TrackGrid"):
        batch.track_raster((0.0, -0.5, 1.0, 1.0, 10, 1), np.zeros((1, 10)))
    for bad in (np.zeros((10, 1)), np.zeros(10), np.zeros((1, 10, 1)), torch.zeros((2, 10))):
        with pytest.raises(ValueError, match=r"shape \(ny, nx\) = \(1, 10\)"):
            batch.track_raster(g, bad)
    for bad in (np.zeros((1, 10), dtype=np.complex128), np.full((1, 10), "land"), np.full((1, 10), None),
                torch.zeros((1, 10), dtype=torch.complex64)):
        with pytest.raises(ValueError, match="must be real numbers"):
            batch.track_raster(g, bad)
    assert batch._raster_threshold(None, False, 0.0) == (binding.STE_RASTER_NO_THRESHOLD, 0.0, 0)
    assert batch._raster_threshold(None, True, 2.0) == (binding.STE_RASTER_NO_THRESHOLD, 0.0, 0)
    assert batch._raster_threshold(3, False, 0.25) == (0, 3.0, 1 << 18)
    assert batch._raster_threshold(-np.inf, True, 1.0) == (binding.STE_RASTER_BELOW, -np.inf, 1 << 20)
    with pytest.raises(ValueError, match="threshold must not be NaN"):
        batch._raster_threshold(np.nan, False, 0.0)
    for bad in (-1e-9, np.nan, np.inf):
        with pytest.raises(ValueError, match="min_hours must be finite and >= 0"):
            batch._raster_threshold(1.0, False, bad)
    with pytest.raises(ValueError, match="raster must be a TrackRaster"):
        batch.raster_statistics(None, np.zeros((1, 10)), 4)


FLEET_GRIDS = {"global 5": gmc.FLEET_GRIDS["global 5"], "half-degree north": gmc.FLEET_GRIDS["half-degree north"],
               "fine": rc.FINE_GRID}


@pytest.mark.parametrize("name", list(FLEET_GRIDS))
def test_restatement_against_the_grids_restatement(name):
    """The runs made of the pieces of raster_cases give the per-track ticks and entries of grid_metrics_cases exactly, and its
    outside, total and nbroken: on the mapping fleet (S = 5, Nmax = 8, B = 130, garbage rows planted) for three grids.  And
    valid + nodata + outside = total for every track."""
    from track_estimators import batch

    w = gmc.fleet()
    g = batch.track_grid(*FLEET_GRIDS[name])
    if name == "fine":
        assert g.lon_ref == 179.64 and not g.periodic
    grid = gmc.grid_tuple(g)
    values = rc.raster_values(g.ny, g.nx)
    ref = gmc.grid_metrics(w["states"], w["nsteps"], w["dt"], grid, tracks=True)
    got = rc.raster_metrics(w["states"], w["nsteps"], w["dt"], grid, values, rc.THRESHOLD, False, rc.MIN_TICKS, tracks=True)
    nruns = 0
    for s in range(gmc.FLEET_S):
        for t in range(gmc.FLEET_B):
            ticks, entries = {}, {}
            for c, q, _ in got["per_track"][s][t]:
                assert q > 0
                if c is not None:
                    ticks[c] = ticks.get(c, 0) + q
                    entries[c] = entries.get(c, 0) + 1
            assert (ticks, entries) == ref["per_track"][s][t], (name, s, t)
            starts = [r[2] for r in got["per_track"][s][t]]
            assert starts == sorted(starts) and (not starts or starts[0] == 0)
            nruns += len(starts)
    for k in ("outside", "total", "nbroken"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (name, k)
    assert np.array_equal(got["valid"] + got["nodata"] + got["outside"], got["total"]), name
    assert nruns > (20 if name == "fine" else 1) * gmc.FLEET_S * gmc.FLEET_B


def _hand(name, values, **kw):
    """The restatement on a hand-made track of the grid tests with ``values`` in columns 0 .. 9 (a periodic grid's other
    columns hold no data): (case, TrackGrid, values (ny, nx), result as Python scalars)."""
    from track_estimators import batch

    case = gmc.hand_cases()[name]
    g = batch.track_grid(*case[0])
    full = np.full((g.ny, g.nx), np.nan)
    full[0, :10] = values
    r = rc.raster_metrics(case[1], case[2], case[3], gmc.grid_tuple(g), full, **kw)
    return case, g, full, {k: v[0, 0].item() for k, v in r.items() if k != "row_value"}


@pytest.mark.parametrize("where", ["", "/antimeridian", "/periodic"])
def test_restatement_against_hand_answers(where):
    """`one`: ten 1-degree cells, half an hour in cell 0, an hour each in cells 1 .. 9, half an hour off the grid (in column 10
    of the periodic grid, which holds no data)."""
    name = "one" + where
    off = "nodata" if where == "/periodic" else "outside"
    ramp = np.arange(10.0)
    r = _hand(name, ramp)[3]
    assert r["wsum"] == 45.0 * T20 and r["valid"] == T19 + 9 * T20 and r[off] == T19 and r["total"] == 10 * T20
    assert r["outside" if off == "nodata" else "nodata"] == 0 and r["nbroken"] == 0
    assert (r["vmin"], r["tmin"], r["vmax"], r["tmax"]) == (0.0, 0, 9.0, T19 + 8 * T20)
    assert (r["hit_ticks"], r["hit_first"], r["nhit"], r["nhit_long"], r["hit_longest"]) == (0, -1, 0, 0, 0)
    r = _hand(name, ramp, threshold=5.0)[3]
    assert (r["hit_ticks"], r["hit_first"], r["nhit"], r["nhit_long"], r["hit_longest"]) == (5 * T20, T19 + 4 * T20, 1, 1, 5 * T20)
    r = _hand(name, ramp, threshold=5.0, below=True)[3]  # cells 0 .. 5
    assert (r["hit_ticks"], r["hit_first"], r["nhit"], r["hit_longest"]) == (T19 + 5 * T20, 0, 1, T19 + 5 * T20)
    mask = np.array([1.0, 0.0] * 5)
    r = _hand(name, mask, threshold=1.0, min_ticks=T20)[3]
    assert (r["nhit"], r["hit_ticks"], r["hit_longest"], r["nhit_long"], r["hit_first"]) == (5, T19 + 4 * T20, T20, 4, 0)
    assert r["wsum"] == float(T19 + 4 * T20) and (r["vmin"], r["tmin"], r["vmax"], r["tmax"]) == (0.0, T19, 1.0, 0)
    mask[3] = np.nan
    r = _hand(name, mask, threshold=1.0, min_ticks=T20)[3]
    assert r["nodata"] == T20 + (T19 if off == "nodata" else 0) and r["valid"] == T19 + 8 * T20
    assert (r["nhit"], r["hit_ticks"], r["hit_longest"], r["nhit_long"]) == (5, T19 + 4 * T20, T20, 4)
    ones = np.ones(10)
    r = _hand(name, ones, threshold=1.0, min_ticks=3 * T20)[3]
    assert (r["nhit"], r["nhit_long"], r["hit_longest"]) == (1, 1, T19 + 9 * T20)
    ones[3] = np.nan  # the excursion that spanned cell 3 is cut: cells 0 .. 2 and 4 .. 9
    r = _hand(name, ones, threshold=1.0, min_ticks=3 * T20)[3]
    assert (r["nhit"], r["nhit_long"], r["hit_longest"], r["hit_ticks"]) == (2, 1, 6 * T20, T19 + 8 * T20)
    assert r["nodata"] == T20 + (T19 if off == "nodata" else 0) and (r["tmin"], r["tmax"]) == (0, 0)


def test_coverage_of_the_fleet_raster():
    """The raster the parity test uses on "half-degree north" takes the fleet through every branch: time with data, without
    data and off the grid, tracks with several excursions, and excursions shorter than min_ticks."""
    _, _, ref = rc.fleet_reference("half-degree north")
    total = int(ref["total"].sum())
    share = {k: int(ref[k].sum()) / total for k in ("valid", "nodata", "outside")}
    several, short = int((ref["nhit"] >= 2).sum()), int((ref["nhit"] > ref["nhit_long"]).sum())
    print(f"half-degree north: valid {share['valid']:.3f}, nodata {share['nodata']:.3f}, outside {share['outside']:.3f} of the "
          f"ticks; {several} of {ref['nhit'].size} tracks with two or more excursions, {short} with a short one")
    assert all(v >= 0.05 for v in share.values()), share
    assert ref["nhit"].size == 650 and several >= 100 and short >= 100, (several, short)


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def _same(got, ref, what, keys):
    """Equal as bit patterns (NaN included), with the dtypes of the call."""
    for k in keys:
        want = np.float64 if k in rc.FLOAT + ("row_value",) else np.int32 if k in rc.INT32 else np.int64
        assert got[k].dtype == want and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
        if not np.array_equal(_bits(got[k]), _bits(np.asarray(ref[k], dtype=want))):
            bad = np.argwhere(_bits(got[k]) != _bits(np.asarray(ref[k], dtype=want)))
            raise AssertionError((what, k, len(bad), bad[:5].tolist(), got[k][tuple(bad[0])], ref[k][tuple(bad[0])]))


def _companions(got, what):
    """The front end's own columns, from the device's integers."""
    tph = float(rc.TICKS_PER_HOUR)
    assert np.array_equal(got["valid"] + got["nodata"] + got["outside"], got["total"]), what
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(_bits(got["mean"]), _bits(np.where(got["valid"] > 0, got["wsum"] / got["valid"], np.nan))), what
    for k, name in (("valid", "valid_hours"), ("tmin", "tmin_hours"), ("tmax", "tmax_hours"), ("hit_ticks", "hit_hours"),
                    ("hit_first", "hit_first_hours"), ("hit_longest", "hit_longest_hours")):
        if k in got:
            assert np.array_equal(_bits(got[name]), _bits(np.where(got[k] < 0, np.nan, got[k] / tph))), (what, name)


@pytest.mark.gpu
def test_hand_made_tracks_on_the_device():
    from track_estimators import batch

    ramp, mask = np.arange(10.0), np.array([1.0, 0.0, 1.0, np.nan, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0])
    for name in gmc.hand_cases():
        for values, kw in ((ramp, dict(threshold=5.0)), (ramp, dict(threshold=5.0, below=True, min_ticks=6 * T20)),
                           (mask, dict(threshold=1.0, min_ticks=T20)), (ramp, dict())):
            case, g, full, want = _hand(name, values, **kw)
            ref = rc.raster_metrics(case[1], case[2], case[3], gmc.grid_tuple(g), full, **kw)
            db = batch.DeviceBatch(pmc.bare_batch(case[2], case[3]), histories=False)
            args = dict(threshold=kw.get("threshold"), below=kw.get("below", False),
                        min_hours=kw.get("min_ticks", 0) / rc.TICKS_PER_HOUR)
            got = _host(db.raster_metrics(_dev(db, case[1]), batch.track_raster(g, full, device=db.device), rows=True, **args))
            keys = OUTPUTS if kw else tuple(k for k in OUTPUTS if k not in rc.HIT)
            assert kw or not set(rc.HIT) & set(got)
            _same(got, ref, (name, kw), keys + ("row_value",))
            _companions(got, (name, kw))
            if name.startswith("one") and values is ramp:
                assert got["wsum"].tolist() == [[45.0 * T20]] and got["tmax"].tolist() == [[T19 + 8 * T20]]
                assert np.array_equal(got["row_value"][0, :10, 0], ramp) and np.isnan(got["row_value"][0, 10, 0])


def _fleet_batch():
    from track_estimators import batch

    w = gmc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


FLEET_KW = dict(threshold=rc.THRESHOLD, min_hours=rc.MIN_HOURS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rc.FLEET_RASTERS))
def test_fleet_against_the_restatement(name):
    """S = 5, Nmax = 8, B = 130 (two waves plus two lanes), ragged (every length 0 .. 8), garbage rows planted: every output
    equals the restatement bit for bit, row_value too, and NaN in the rows past nsteps changes nothing."""
    from track_estimators import batch

    w, db, full = _fleet_batch()
    g, values, ref = rc.fleet_reference(name)
    raster = batch.track_raster(g, values, device=db.device)
    got = _host(db.raster_metrics(full, raster, rows=True, **FLEET_KW))
    _same(got, ref, name, OUTPUTS + ("row_value",))
    _companions(got, name)
    none = w["nsteps"] == 0
    assert not got["total"][:, none].any() and (got["tmin"][:, none] == -1).all() and np.isnan(got["vmin"][:, none]).all()
    assert (got["hit_first"][:, none] == -1).all() and not got["wsum"][:, none].any()
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.raster_metrics(_dev(db, poisoned), raster, rows=True, **FLEET_KW))
    _same(again, got, (name, "rows past nsteps were read"), OUTPUTS + ("row_value",))


@pytest.mark.gpu
def test_duality_with_the_grid_kernel():
    """What the grid kernel adds to the cells, this kernel reads along the tracks: with integer values the sum over all tracks
    of wsum is the sum over the cells of value x ticks, exactly (every product and partial sum an integer below 2^53); and
    outside, total and nbroken are the grid call's."""
    from track_estimators import batch

    w, db, full = _fleet_batch()
    for name in ("half-degree north", "global 5", "fine"):
        g = batch.track_grid(*rc.FLEET_RASTERS[name])
        values = rc.raster_values(g.ny, g.nx, nodata=False)
        grid = db.grid_metrics(full, g)
        got = db.raster_metrics(full, batch.track_raster(g, values, device=db.device))
        ticks = grid["ticks"].cpu().numpy()
        cells = sum(int(v) * int(q) for v, q in zip(values.ravel(), ticks.ravel()))
        wsum = got["wsum"].cpu().numpy()
        assert np.array_equal(wsum, np.rint(wsum)) and np.abs(wsum).max() < 2.0 ** 53
        assert sum(int(v) for v in wsum.ravel()) == cells and ticks.any(), name
        absolute = sum(abs(int(v)) * int(q) for v, q in zip(values.ravel(), ticks.ravel()))
        assert absolute < 2 ** 53
        for k in ("outside", "total", "nbroken"):
            assert got[k].dtype == grid[k].dtype and db.torch.equal(got[k], grid[k]), (name, k)
        assert not got["nodata"].any() and db.torch.equal(got["valid"], got["total"] - got["outside"])
        assert int(got["valid"].sum().item()) == int(ticks.sum())


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """A window [3, 70) (in place, and as a contiguous copy) plus the rest against the whole call; S = 1 slices against S = 5;
    with and without row_value; with and without the threshold outputs."""
    from track_estimators import batch

    w, db, full = _fleet_batch()
    g, values, ref = rc.fleet_reference("half-degree north")
    raster = batch.track_raster(g, values, device=db.device)
    whole = _host(db.raster_metrics(full, raster, rows=True, **FLEET_KW))
    keys = OUTPUTS + ("row_value",)
    _same(whole, ref, "whole fleet", keys)
    lo, hi = gmc.FLEET_WINDOW
    for copied in (False, True):
        cols = {}
        for a, z in ((lo, hi), (0, lo), (hi, gmc.FLEET_B)):
            win = db.window(a, z)
            assert int(win.struct.track_stride) == gmc.FLEET_B
            view = full[..., a:z].contiguous() if copied else full[..., a:z]
            cols[a] = _host(win.raster_metrics(view, raster, rows=True, **FLEET_KW))
        joined = {k: np.concatenate([cols[0][k], cols[lo][k], cols[hi][k]], axis=-1) for k in keys}
        _same(joined, whole, ("windows", copied), keys)
    for s in range(gmc.FLEET_S):
        one = _host(db.raster_metrics(full[s:s + 1], raster, rows=True, **FLEET_KW))
        _same(one, {k: whole[k][s:s + 1] for k in keys}, ("S = 1", s), keys)
    _same(_host(db.raster_metrics(full[2], raster, **FLEET_KW)), {k: whole[k][2:3] for k in OUTPUTS}, "a 3-d tensor", OUTPUTS)
    plain = _host(db.raster_metrics(full, raster, **FLEET_KW))
    assert "row_value" not in plain
    _same(plain, whole, "without row_value", OUTPUTS)
    rest = tuple(k for k in OUTPUTS if k not in rc.HIT)
    for rows in (False, True):
        bare = _host(db.raster_metrics(full, raster, rows=rows))
        assert not set(rc.HIT) & set(bare) and "hit_hours" not in bare
        _same(bare, whole, ("without the threshold outputs", rows), rest + (("row_value",) if rows else ()))
    below = _host(db.raster_metrics(full, raster, threshold=rc.THRESHOLD, below=True, min_hours=rc.MIN_HOURS))
    w_ = gmc.fleet()
    _same(below, rc.raster_metrics(w_["states"], w_["nsteps"], w_["dt"], gmc.grid_tuple(g), values, rc.THRESHOLD, True,
                                   rc.MIN_TICKS), "below", OUTPUTS)
    with pytest.raises(ValueError, match="raster must be a TrackRaster"):
        db.raster_metrics(full, values)
    with pytest.raises(ValueError, match="threshold must not be NaN"):
        db.raster_metrics(full, raster, threshold=float("nan"))
    with pytest.raises(ValueError, match="min_hours must be finite and >= 0"):
        db.raster_metrics(full, raster, threshold=1.0, min_hours=-1.0)
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.raster_metrics(full[:, :, :3], raster)


@pytest.mark.gpu
def test_a_map_fed_back_on_the_device():
    """The ship-hours map of grid_metrics goes back in as a raster without leaving the device: the same storage, no NaN, and
    every track's valid ticks are its own ticks on the grid."""
    from track_estimators import batch

    w, db, full = _fleet_batch()
    g = batch.track_grid(*gmc.FLEET_GRIDS["half-degree north"])
    grid = db.grid_metrics(full, g)
    raster = batch.track_raster(g, grid["hours"])
    assert raster.values.data_ptr() == grid["hours"].data_ptr() and raster.grid is g
    again = batch.track_raster(g, grid["ticks"])  # int64: converted, a tensor of its own on the same device
    assert again.values.dtype == db.torch.float64 and again.values.device == db.device
    got = db.raster_metrics(full, raster, threshold=1.0)
    assert db.torch.equal(got["valid"], grid["total"] - grid["outside"]) and not got["nodata"].any()
    assert db.torch.equal(got["outside"], grid["outside"]) and bool((got["vmin"][got["valid"] > 0] > 0.0).all())
    # a track's own time in a cell is in the map, so its mean along the track is at least its shortest run there, and the
    # fleet's sum of wsum is the sum over cells of hours x ticks (in floating point: no equality)
    ws, tk = float(got["wsum"].sum().item()), grid["ticks"].to(db.torch.float64)
    assert abs(ws - float((grid["hours"] * tk).sum().item())) <= 1e-12 * ws


def _sampled_batch():
    """The small batch of the grid tests' statistics: six synthetic tracks of 20 steps, ragged, run() done; a raster of
    0.05-degree cells about the middle row of track 0."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(synthetic.make_batch(6, nobs=11, seed0=100), 2, H, Q, R, P0)
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 13, 7, 1, 0], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    lon, lat = (float(v) for v in db.sm_mean[10, :2, 0].cpu().numpy())
    g = batch.track_grid(np.floor(lon * 20.0) / 20.0 - 0.8, np.floor(lat * 20.0) / 20.0 - 0.8, 0.05, 0.05, 32, 32)
    return hb, db, batch.track_raster(g, rc.raster_values(32, 32), device=db.device)


@pytest.mark.gpu
def test_raster_statistics():
    from track_estimators import batch

    hb, db, raster = _sampled_batch()
    nsamples = 3
    kw = dict(threshold=rc.THRESHOLD, min_hours=0.05)
    a = batch.raster_statistics(db, raster, nsamples, seed=4, chunk=3, **kw)
    b = batch.raster_statistics(db, raster, nsamples, seed=4, chunk=16, **kw)
    assert set(a) == set(b) and a["mean"].shape == a["hit_hours"].shape == a["nbroken"].shape == (nsamples, hb.B)
    assert a["mean_quantiles"].shape == a["hit_hours_quantiles"].shape == (3, hb.B) and a["p_hit"].shape == (hb.B,)
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)  # one seed, chunk >= nsamples both: the same draws
    # two chunks of 3: the first chunk's draws are those, the second drew on; what does not depend on the draws is equal
    c = batch.raster_statistics(db, raster, 6, seed=4, chunk=3, **kw)
    assert c["mean"].shape == (6, hb.B) and np.array_equal(_bits(c["mean"][:3]), _bits(a["mean"]))
    assert np.array_equal(c["hit_hours"][:3], a["hit_hours"]) and not np.array_equal(c["hit_hours"][3:], a["hit_hours"])
    assert all(np.array_equal(_bits(a[k]), _bits(c[k])) for k in a if k.endswith("_smoothed") or k == "status")
    # chunk >= nsamples: the draws of sample_smoothed(nsamples, seed), so per-sample calls on them give the same columns
    samples = db.sample_smoothed(nsamples, seed=4)
    per = [_host(db.raster_metrics(samples[s], raster, **kw)) for s in range(nsamples)]
    nhit = np.concatenate([p["nhit"] for p in per])
    assert np.array_equal(b["p_hit"], (nhit > 0).mean(axis=0)) and 0.0 < b["p_hit"].max() <= 1.0
    assert np.array_equal(b["p_hit_long"], (np.concatenate([p["nhit_long"] for p in per]) > 0).mean(axis=0))
    assert np.array_equal(b["hit_hours"], np.concatenate([p["hit_hours"] for p in per]))
    assert np.array_equal(_bits(b["mean"]), _bits(np.concatenate([p["mean"] for p in per])))
    assert np.array_equal(b["hit_hours_mean"], b["hit_hours"].mean(axis=0)) and not b["status"].any()
    sm = _host(db.raster_metrics(db.sm_mean, raster, **kw))
    assert all(np.array_equal(_bits(b[k + "_smoothed"]), _bits(v[0])) for k, v in sm.items())
    # the restatement on the smoothed track
    g = raster.grid
    ref = rc.raster_metrics(db.sm_mean.cpu().numpy()[None], hb.nsteps, hb.dt, gmc.grid_tuple(g), raster.values.cpu().numpy(),
                            rc.THRESHOLD, False, int(np.rint(0.05 * rc.TICKS_PER_HOUR)))
    _same(sm, ref, "smoothed", OUTPUTS)
    assert ref["valid"].any() and ref["outside"].any()
    d = batch.raster_statistics(hb, raster, 3, seed=9, chunk=3)  # a HostBatch is uploaded and run first; no threshold
    assert "p_hit" not in d and d["mean"].shape == (3, hb.B) and np.isnan(d["mean"][:, 5]).all()
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.raster_statistics(db, raster, 0)


@pytest.mark.gpu
def test_dropin_raster_along_track():
    import types

    import track_sampling_cases as tsc
    from track_estimators import batch, synthetic
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter

    sb = tsc.synthetic_batch()
    H, Q, R, P0 = synthetic.example_matrices()
    trk = types.SimpleNamespace(z=sb.z[0], dts=sb.dts[0], sog=sb.sog[0], cog=sb.cog[0], sog_rate=sb.sog_rate[0].copy(),
                                cog_rate=sb.cog_rate[0].copy())
    ukf = UnscentedKalmanFilter(H=H, Q=Q, R=R, P=P0, x0=sb.z[0][:, 0], non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.raster_along_track(None)
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    with pytest.raises(ValueError, match="raster must be a TrackRaster"):
        ukf.raster_along_track(np.zeros((4, 4)))
    samples = ukf.sample_smoothed(4, random_state=1)  # (4, N+1, 4)
    lon, lat = samples[0, tsc.NMAX // 2, 0], samples[0, tsc.NMAX // 2, 1]
    g = batch.track_grid(np.floor(lon * 10.0) / 10.0 - 1.6, np.floor(lat * 10.0) / 10.0 - 1.6, 0.1, 0.1, 32, 32)
    values = rc.raster_values(32, 32)
    raster = batch.track_raster(g, values)
    kw = dict(threshold=rc.THRESHOLD, min_hours=0.05)
    r0 = ukf.raster_along_track(raster, **kw)
    assert "posterior" not in r0 and r0["row_value"].shape == (tsc.NMAX + 1,) and r0["wsum"].shape == ()
    assert int(r0["total"]) == int(np.rint(dt * rc.TICKS_PER_HOUR).sum()) and int(r0["valid"]) > 0
    r4 = ukf.raster_along_track(raster, n_samples=4, random_state=1, **kw)
    assert all(np.array_equal(_bits(r0[k]), _bits(r4[k])) for k in r0)
    ref = rc.raster_metrics(samples[..., None], [tsc.NMAX], dt[:, None], gmc.grid_tuple(g), values, rc.THRESHOLD, False,
                            int(np.rint(0.05 * rc.TICKS_PER_HOUR)))
    post = r4["posterior"]
    assert np.array_equal(post["hit_hours"], ref["hit_ticks"][:, 0] / rc.TICKS_PER_HOUR)
    assert post["p_hit"] == (ref["nhit"][:, 0] > 0).mean() and post["mean"].shape == (4,)
    with pytest.raises(ValueError, match="n_samples must be >= 0"):
        ukf.raster_along_track(raster, n_samples=-1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
