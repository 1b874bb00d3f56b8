"""Tracks on the device on a regular lon / lat grid (include/ste.h: ste_grid_f64, ste_grid_metrics_f64; DESIGN.md, "Grids"):
declaration and layout of the C ABI, the Python restatement against hand answers and against sampling, its conservation
identity with garbage rows, and the refusals of the front end and of the call (CPU); on the GPU the hand-made tracks, the edges
of the lane mapping on a ragged fleet, independence of the surroundings, the shapes at the ends, the sampler's output through
the Python front ends, and the refusals on the device build.  Time is integer ticks: every GPU comparison is an equality."""
import ctypes as C
import os
import re

import grid_metrics_cases as gmc
import numpy as np
import path_metrics_cases as pmc
import pytest
import region_metrics_cases as rmc
from conftest import ROOT

FIELDS = ["nstates", "flags", "states", "nx", "ny", "lon0", "lat0", "dlon", "dlat", "lon_ref", "ticks", "entries", "outside",
          "total", "nbroken"]
INT_OUTPUTS = ("ticks", "entries", "outside", "total", "nbroken")


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_grid_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_grid_f64\* g, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_grid_f64 {"): hdr.index("} ste_grid_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for names in re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+(?:\s*,\s*\w+)*)\s*;", body):
        fields += [n.strip() for n in names.split(",")]
    assert fields == [f[0] for f in binding.SteGridF64._fields_] == FIELDS
    # the layout of the C struct by hand: two 32-bit integers share a word, every pointer and every double takes one
    offsets = {"nstates": 0, "flags": 4, "states": 8, "nx": 16, "ny": 20, "lon0": 24, "lat0": 32, "dlon": 40, "dlat": 48,
               "lon_ref": 56, "ticks": 64, "entries": 72, "outside": 80, "total": 88, "nbroken": 96}
    assert {f: getattr(binding.SteGridF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteGridF64) == 104
    assert "ste_grid_metrics_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_grid_metrics_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the grid arguments travel beside the batch
    assert int(re.search(r"#define STE_GRID_TICKS_PER_HOUR (\d+)", hdr).group(1)) == binding.STE_GRID_TICKS_PER_HOUR == 1 << 20
    assert re.search(r"#define STE_GRID_MAX_CELLS \(1 << 26\)", hdr) and binding.STE_GRID_MAX_CELLS == 1 << 26
    assert int(re.search(r"#define STE_GRID_PERIODIC_LON 0x(\d+)u", hdr).group(1), 16) == binding.STE_GRID_PERIODIC_LON == 1
    assert gmc.TICKS_PER_HOUR == binding.STE_GRID_TICKS_PER_HOUR
    comment = hdr[hdr.index("GRIDS:"): hdr.index("#define STE_GRID_TICKS_PER_HOUR")]
    for word in ("Ticks.", "Grid.", "Unwrapping.", "Pieces.", "Runs.", "SOUND", "BROKEN", "OUTSIDE", "wrap180", "ties to x"):
        assert word in comment, word


def _check_hand_case(name, case, r):
    args, st, nsteps, dt, want, outside, col10 = case
    assert r["ticks"][0, :10].tolist() == want, (name, r["ticks"][0, :12])
    assert r["entries"][0, :10].tolist() == [1] * 10, (name, r["entries"][0, :12])
    assert r["outside"].tolist() == [[outside]] and not r["nbroken"].any(), (name, r["outside"])
    assert r["total"].tolist() == [[10 << 20]], name
    if col10 is not None:  # periodic: what was outside is in column 10, and nowhere else
        assert r["ticks"][0, 10] == col10 and r["entries"][0, 10] == 1 and not r["ticks"][0, 11:].any(), name
    assert int(r["ticks"].sum()) + outside == 10 << 20, name


def test_restatement_against_hand_answers():
    """The equator at one degree an hour over a row of ten one-degree cells from lon 0.  From 0.5 in ten steps of an hour: cell
    0 gets 2^19 ticks, cells 1 .. 9 get 2^20 each, 2^19 are outside, every cell is entered once.  From 0.25 in four steps of
    2.5 hours: cell 0 gets 786 432, the rest 2^20, 262 144 are outside.  The same with track and grid moved to 175 .. 185 and
    stored wrapped, and through a periodic 360 x 1 grid (where the last piece lies in column 10)."""
    from track_estimators import batch

    cases = gmc.hand_cases()
    assert cases["one"][4] == [1 << 19] + [1 << 20] * 9 and cases["one"][5] == 1 << 19
    assert cases["two"][4] == [786432] + [1 << 20] * 9 and cases["two"][5] == 262144
    for name, case in cases.items():
        g = batch.track_grid(*case[0])
        assert g.periodic == name.endswith("/periodic")
        _check_hand_case(name, case, gmc.grid_metrics(case[1], case[2], case[3], gmc.grid_tuple(g)))


def _sampled_track(lon, lat, dt, ns, grid, nsub=1000):
    """Hours per cell of one track from ``nsub`` mid-point samples of every sound step, classified by floor alone."""
    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = grid
    u = (np.arange(nsub) + 0.5) / nsub
    hours = {}
    for k in range(ns):
        ax = lon_ref + gmc.wrap180(lon[k] - lon_ref)
        delta = gmc.wrap180(lon[k + 1] - lon[k])
        ix = np.floor((ax + u * delta - lon0) / dlon).astype(np.int64)
        iy = np.floor((lat[k] + u * (lat[k + 1] - lat[k]) - lat0) / dlat).astype(np.int64)
        if periodic:
            ix = ix % nx
        on = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
        if not on.any():
            continue
        cells, counts = np.unique(np.stack([iy[on], ix[on]]), axis=1, return_counts=True)
        for (cy, cx), n in zip(cells.T, counts):
            hours[(int(cy), int(cx))] = hours.get((int(cy), int(cx)), 0.0) + dt[k] * n / nsub
    return hours


def test_restatement_against_sampling():
    """Three grids (half-degree cells across the antimeridian, the global 5-degree grid, one cell of 20 x 10 degrees) against
    1000 mid-point samples of every step of 300 random ragged tracks, classified by floor alone.  A cell of a track may differ
    by max(dt) * 2 * entries[cell] / 1000 + 1e-9 h: each end of a run misplaces at most one sampling interval."""
    from track_estimators import batch

    w = gmc.random_tracks()
    st, nsteps, dt = w["states"], w["nsteps"], w["dt"]
    B = st.shape[3]
    for name, args in gmc.SAMPLING_GRIDS.items():
        grid = gmc.grid_tuple(batch.track_grid(*args))
        assert grid[6] == (name == "global 5") and (name != "half-degree" or grid[7] == 180.0)
        r = gmc.grid_metrics(st, nsteps, dt, grid, tracks=True)
        assert not r["nbroken"].any()
        worst, many = 0.0, 0
        for t in range(B):
            ns = int(nsteps[t])
            tk, en = r["per_track"][0][t]
            hours = _sampled_track(st[0, :, 0, t], st[0, :, 1, t], dt[:, t], ns, grid)
            many += len(tk) > 1
            for c in set(tk) | set(hours):
                err = abs(tk.get(c, 0) / gmc.TICKS_PER_HOUR - hours.get(c, 0.0))
                tol = dt[:ns, t].max() * 2.0 * en.get(c, 0) / 1000.0 + 1e-9
                assert err <= tol, (name, t, c, err, tol)
                worst = max(worst, err / tol)
        share = r["outside"].sum() / r["total"].sum()
        print(f"restatement against 1000-point sampling, {name}: worst error {worst:.3g} of its bound, {many} of {B} tracks in "
              f"more than one cell, {share:.3f} of the ticks outside")
        if name == "half-degree":  # a fair sample
            assert many >= B // 2 and 0.05 <= share <= 0.50, (many, share)


def test_conservation_and_additivity_on_the_restatement():
    """The grid's ticks of a track + its outside ticks = its total ticks = the rounded dt of its sound steps, as integers, for
    every track of the mapping fleet on every grid, the garbage rows included: latitude 1e300 (two sound steps that run off
    the grid), NaN longitude and inf latitude (two broken steps each), dt = -1 and NaN (one each).  No other track moves."""
    from track_estimators import batch

    w, clean = gmc.fleet(), rmc.fleet()
    planted = {gmc.HUGE_LAT_TRACK: 0, gmc.NAN_LON_TRACK: 2, gmc.INF_LAT_TRACK: 2, gmc.NEG_DT_TRACK: 1, gmc.NAN_DT_TRACK: 1,
               rmc.NAN_TRACK: 2, rmc.JUMP_TRACK: 1}
    dtq = np.rint(w["dt"] * gmc.TICKS_PER_HOUR)
    for name, args in gmc.FLEET_GRIDS.items():
        grid = gmc.grid_tuple(batch.track_grid(*args))
        r = gmc.grid_metrics(w["states"], w["nsteps"], w["dt"], grid, tracks=True)
        c = gmc.grid_metrics(clean["states"], clean["nsteps"], clean["dt"], grid, tracks=True)
        assert gmc.conserved(r)
        for s in range(gmc.FLEET_S):
            for t in range(gmc.FLEET_B):
                tk, en = r["per_track"][s][t]
                assert sum(tk.values()) + int(r["outside"][s, t]) == int(r["total"][s, t]), (name, s, t)
                assert r["nbroken"][s, t] == planted.get(t, 0), (name, s, t)
                if t not in planted:
                    assert int(r["total"][s, t]) == int(dtq[: w["nsteps"][t], t].sum())
                    assert (tk, en) == c["per_track"][s][t] and r["outside"][s, t] == c["outside"][s, t]
        b = gmc.HUGE_LAT_TRACK  # steps 2 and 3 run off the grid: they are sound, and all of step 2 but its start is outside
        assert (r["total"][:, b] == int(dtq[:, b].sum())).all() and (r["outside"][:, b] >= int(dtq[3, b])).all()
        for b, steps in ((gmc.NAN_LON_TRACK, (3, 4)), (gmc.INF_LAT_TRACK, (1, 2)), (gmc.NEG_DT_TRACK, (5,)), (gmc.NAN_DT_TRACK, (1,))):
            assert (r["total"][:, b] == int(np.delete(dtq[:, b], steps).sum())).all(), (name, b)
        # additivity: a window and the rest, and the samples one by one, sum to the whole
        lo, hi = gmc.FLEET_WINDOW
        parts = [gmc.grid_metrics(w["states"][..., a:z], w["nsteps"][a:z], w["dt"][:, a:z], grid)
                 for a, z in ((0, lo), (lo, hi), (hi, gmc.FLEET_B))]
        parts2 = [gmc.grid_metrics(w["states"][s:s + 1], w["nsteps"], w["dt"], grid) for s in range(gmc.FLEET_S)]
        for k in ("ticks", "entries"):
            assert np.array_equal(sum(p[k] for p in parts), r[k]) and np.array_equal(sum(p[k] for p in parts2), r[k]), (name, k)


def test_front_end_refusals():
    from track_estimators import batch

    ok = (0.0, -10.0, 0.5, 0.5, 40, 40)
    g = batch.track_grid(*ok)
    assert (g.nx, g.ny, g.periodic, g.lon_ref) == (40, 40, False, 10.0)
    assert np.array_equal(g.lon_edges, np.arange(41) * 0.5) and np.array_equal(g.lat_edges, -10.0 + np.arange(41) * 0.5)
    p = batch.track_grid(-180.0, -90.0, 1.0, 1.0, 360, 180)
    assert p.periodic and p.lon_ref == 0.0 and p.lon_edges[-1] == 180.0
    assert batch.track_grid(10.0, 0.0, 0.25, 1.0, 720, 2).lon_ref == 100.0  # 180 degrees wide: the most without wrapping

    def refused(match, **kw):
        a = dict(zip(("lon0", "lat0", "dlon", "dlat", "nx", "ny"), ok))
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            batch.track_grid(**a)

    for bad in (0, -1, 2.5):
        refused("integers >= 1", nx=bad)
        refused("integers >= 1", ny=bad)
    refused("at most 67108864 cells", nx=8193, ny=8192)
    assert batch.track_grid(0.0, 0.0, 0.01, 0.01, 8192, 8192).nx == 8192
    for bad in (np.nan, np.inf, -np.inf):
        refused("lon0 and lat0 must be finite", lon0=bad)
        refused("lon0 and lat0 must be finite", lat0=bad)
        refused("finite and >= 1e-6", dlon=bad)
        refused("finite and >= 1e-6", dlat=bad)
    for bad in (0.0, -0.5, 9e-7):
        refused("finite and >= 1e-6", dlon=bad)
        refused("finite and >= 1e-6", dlat=bad)
    refused("at most 180 degrees wide", nx=361)
    refused("at most 180 degrees wide", dlon=1.0, nx=359)
    refused("at most 180 degrees wide", dlon=1.0, nx=361)


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

    def good_grid():
        g = binding.SteGridF64()
        g.nstates, g.flags, g.states, g.nx, g.ny = 3, 0, 0x3000, 32, 24
        g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref = 172.0, -3.0, 0.5, 0.25, 180.0
        g.ticks, g.entries, g.outside, g.total, g.nbroken = 0x5000, 0x6000, 0x7000, 0x8000, 0x9000
        return g

    def refused(reason, **fields):
        s, g = good_batch(), good_grid()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(g, name) else g, name, value)
        rc = lib.ste_grid_metrics_f64(ref(s), ref(g), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_grid_metrics_f64" in msg, (fields, rc, msg)

    for s, g, reason in ((None, good_grid(), "batch pointer is NULL"), (good_batch(), None, "grid arguments (g) are NULL")):
        assert lib.ste_grid_metrics_f64(ref(s), ref(g), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_grid_metrics_f64" in msg
    refused("g->states is required", states=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for f in (0x2, 0x3, 0x80000000):
        refused("unknown bits", flags=f)
    for n in (0, -1):
        refused("nx and g->ny must be >= 1", nx=n)
        refused("nx and g->ny must be >= 1", ny=n)
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
    refused("within lon_ref +- 90", nx=361)                                     # 180.5 degrees wide
    refused("within lon_ref +- 90", lon_ref=90.0)                               # 16 degrees wide, but east of lon_ref + 90
    refused("within lon_ref +- 90", lon_ref=270.0)
    refused("batch's dt is required", dt=None)
    nothing = dict(ticks=None, entries=None, outside=None, total=None, nbroken=None)
    refused("no output asked for", **nothing)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _equal(got, ref, what, keys=INT_OUTPUTS):
    """Integer outputs equal to the restatement's, with their dtypes; hours = ticks / 2^20; the identity on the device's own
    outputs."""
    for k in keys:
        assert got[k].dtype == (np.int32 if k == "nbroken" else np.int64), (what, k, got[k].dtype)
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError((what, k, len(bad), bad[:5].tolist(), got[k][tuple(bad[0])], ref[k][tuple(bad[0])]))
    assert np.array_equal(got["hours"], got["ticks"] / gmc.TICKS_PER_HOUR), what
    if "total" in keys:
        assert gmc.conserved(got), what


@pytest.mark.gpu
def test_hand_made_tracks_on_the_device():
    from track_estimators import batch

    for name, case in gmc.hand_cases().items():
        args, st, nsteps, dt = case[:4]
        db = batch.DeviceBatch(pmc.bare_batch(nsteps, dt), histories=False)
        g = batch.track_grid(*args)
        got = _host(db.grid_metrics(_dev(db, st), g, entries=True))
        _check_hand_case(name, case, got)
        _equal(got, gmc.grid_metrics(st, nsteps, dt, gmc.grid_tuple(g)), f"hand-made tracks, {name}")


def _fleet_batch():
    from track_estimators import batch

    w = gmc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gmc.FLEET_GRIDS))
def test_edges_of_the_mapping(name):
    """S = 5, Nmax = 8, B = 130 (two waves plus two lanes), ragged (nsteps 0 .. Nmax), about (179.6, 10), garbage rows planted:
    ticks, entries, outside, total and nbroken equal the restatement, the identity holds on the device's own outputs, and NaN
    in the rows past nsteps changes nothing."""
    from track_estimators import batch

    w, db, full = _fleet_batch()
    g = batch.track_grid(*gmc.FLEET_GRIDS[name])
    ref = gmc.fleet_reference(name)
    got = _host(db.grid_metrics(full, g, entries=True))
    _equal(got, ref, f"mapping fleet, {name}")
    for b, n in ((gmc.HUGE_LAT_TRACK, 0), (gmc.NAN_LON_TRACK, 2), (gmc.INF_LAT_TRACK, 2), (gmc.NEG_DT_TRACK, 1), (gmc.NAN_DT_TRACK, 1)):
        assert (got["nbroken"][:, b] == n).all(), b
    assert not got["total"][:, w["nsteps"] == 0].any() and not got["outside"][:, w["nsteps"] == 0].any()
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.grid_metrics(_dev(db, poisoned), g, entries=True))
    for k in INT_OUTPUTS:
        assert np.array_equal(got[k], again[k]), (k, "rows past nsteps were read")


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """A window [3, 70) (in place, and as a contiguous copy) plus the rest, accumulated into one grid, equals the whole call;
    S = 1 slices accumulated equal S = 5; calling twice doubles the grid; ticks alone, through the C ABI, are the same ticks."""
    from track_estimators import batch
    from track_estimators._hip import binding

    w, db, full = _fleet_batch()
    g = batch.track_grid(*gmc.FLEET_GRIDS["half-degree north"])
    whole = _host(db.grid_metrics(full, g, entries=True))
    _equal(whole, gmc.fleet_reference("half-degree north"), "whole fleet")
    lo, hi = gmc.FLEET_WINDOW
    for copied in (False, True):
        acc, cols = None, {}
        for a, z in ((lo, hi), (0, lo), (hi, gmc.FLEET_B)):
            win = db.window(a, z)
            assert int(win.struct.track_stride) == gmc.FLEET_B
            view = full[..., a:z].contiguous() if copied else full[..., a:z]
            acc = win.grid_metrics(view, g, entries=True, out=acc)
            cols[a] = _host({k: acc[k] for k in ("outside", "total", "nbroken")})
        got = _host(acc)
        for k in ("ticks", "entries"):
            assert np.array_equal(got[k], whole[k]), (k, "windows accumulated", copied)
        for k in ("outside", "total", "nbroken"):
            assert np.array_equal(np.concatenate([cols[0][k], cols[lo][k], cols[hi][k]], axis=1), whole[k]), (k, copied)
    acc = None
    for s in range(gmc.FLEET_S):
        acc = db.grid_metrics(full[s:s + 1], g, entries=True, out=acc)
        for k in ("outside", "total", "nbroken"):
            assert np.array_equal(acc[k].cpu().numpy(), whole[k][s:s + 1]), (k, s)
    for k in ("ticks", "entries"):
        assert np.array_equal(acc[k].cpu().numpy(), whole[k]), (k, "S = 1 slices accumulated")
    twice = db.grid_metrics(full, g, entries=True, out=db.grid_metrics(full, g, entries=True))
    for k in ("ticks", "entries"):
        assert np.array_equal(twice[k].cpu().numpy(), 2 * whole[k]), (k, "twice")
    assert np.array_equal(twice["hours"].cpu().numpy(), 2 * whole["hours"])
    plain = _host(db.grid_metrics(full, g))
    assert set(plain) == {"ticks", "hours", "outside", "total", "nbroken"} and np.array_equal(plain["ticks"], whole["ticks"])
    # ticks alone, through the C ABI
    torch = db.torch
    alone = torch.zeros((g.ny, g.nx), dtype=torch.int64, device=db.device)
    a = binding.SteGridF64()
    a.nstates, a.flags, a.states, a.nx, a.ny = gmc.FLEET_S, 0, full.data_ptr(), g.nx, g.ny
    a.lon0, a.lat0, a.dlon, a.dlat, a.lon_ref = g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref
    a.ticks = alone.data_ptr()
    binding.check(db.lib.ste_grid_metrics_f64(C.byref(db.struct), C.byref(a), db._stream(None)), "ste_grid_metrics_f64")
    assert np.array_equal(alone.cpu().numpy(), whole["ticks"]), "ticks alone"
    with pytest.raises(ValueError, match=r"out\['ticks'\] must be a contiguous int64 tensor"):
        db.grid_metrics(full, batch.track_grid(*gmc.FLEET_GRIDS["global 5"]), out=twice)
    with pytest.raises(ValueError, match="grid must be a TrackGrid"):
        db.grid_metrics(full, gmc.FLEET_GRIDS["global 5"])
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.grid_metrics(full[:, :, :3], g)


END_GRIDS = {"one cell across the fleet": (178.0, 9.0, 4.0, 2.0, 1, 1),         # nx = ny = 1, much of the fleet outside
             "one cell that holds the fleet": (150.0, -20.0, 60.0, 60.0, 1, 1),  # every lane flushes to one address
             "global 1": (-180.0, -90.0, 1.0, 1.0, 360, 180),                    # the periodic 360 x 180 grid
             # either side of the size up to which a block sums the grid in a copy of its own (256 cells)
             "256 cells": (176.0, 6.0, 0.5, 0.5, 16, 16), "272 cells": (176.0, 6.0, 0.5, 0.5, 17, 16)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(END_GRIDS))
def test_shapes_at_the_ends(name):
    from track_estimators import batch

    w, db, full = _fleet_batch()
    g = batch.track_grid(*END_GRIDS[name])
    ref = gmc.fleet_reference(name, END_GRIDS[name])
    got = _host(db.grid_metrics(full, g, entries=True))
    _equal(got, ref, f"mapping fleet, {name}")
    if name == "one cell that holds the fleet":
        # only the 120-degree jump's first rows (at 59.6 E) and the latitude of 1e300 are off the grid
        away = {rmc.JUMP_TRACK, gmc.HUGE_LAT_TRACK}
        assert all(not got["outside"][:, b].any() for b in range(gmc.FLEET_B) if b not in away)
        assert got["ticks"][0, 0] == got["total"].sum() - got["outside"].sum() > 0
        assert got["entries"][0, 0] >= gmc.FLEET_S * (w["nsteps"] > 0).sum()
    if name == "global 1":
        assert g.periodic and (got["outside"][:, [b for b in range(gmc.FLEET_B) if b != gmc.HUGE_LAT_TRACK]] == 0).all()


def _fine_fleet():
    """S = 2, Nmax = 6, B = 70 about a grid of 64 x 64 cells of 0.001 degrees across the antimeridian: steps of N(0, 0.02)
    degrees from starts in and about the grid's 0.064 degrees, so that a step crosses tens of lines of either kind."""
    rng = np.random.default_rng(23)
    S, N, B = 2, 6, 70
    st = np.zeros((S, N + 1, 4, B))
    start = np.stack([179.968 + rng.uniform(-0.01, 0.074, B), 9.968 + rng.uniform(-0.01, 0.074, B)])
    st[:, 0, :2] = start
    st[:, 1:, :2] = start[None, None] + np.cumsum(rng.normal(0.0, 0.02, (S, N, 2, B)), axis=1)
    st[:, :, 0] = gmc.wrap180(st[:, :, 0])
    return st, (np.arange(B) % (N + 1)).astype(np.int32), rng.uniform(0.2, 1.5, (N, B))


@pytest.mark.gpu
def test_a_grid_every_step_crosses_many_lines_of():
    """The walker's longest loops: 0.001-degree cells, 64 x 64 of them, and steps of some 0.02 degrees."""
    from track_estimators import batch

    st, nsteps, dt = _fine_fleet()
    g = batch.track_grid(179.968, 9.968, 0.001, 0.001, 64, 64)
    ref = gmc.grid_metrics(st, nsteps, dt, gmc.grid_tuple(g))
    live = int((nsteps > 0).sum()) * st.shape[0]
    assert ref["entries"].sum() > 20 * live and (ref["ticks"] > 0).mean() > 0.5  # tens of cells per track; most cells visited
    db = batch.DeviceBatch(pmc.bare_batch(nsteps, dt), histories=False)
    _equal(_host(db.grid_metrics(_dev(db, st), g, entries=True)), ref, "fine grid")


def _sampled_batch():
    """Six synthetic tracks of 20 steps, ragged, forward pass and smoother done; a grid of 0.05-degree cells about the middle
    row of track 0 (much of the fleet is off it), and the global 5-degree grid."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(synthetic.make_batch(6, nobs=11, seed0=100), 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 13, 7, 1, 0], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    lon, lat = (float(v) for v in db.sm_mean[10, :2, 0].cpu().numpy())
    local = batch.track_grid(np.floor(lon * 20.0) / 20.0 - 0.8, np.floor(lat * 20.0) / 20.0 - 0.8, 0.05, 0.05, 32, 32)
    return hb, db, {"local": local, "global 5": batch.track_grid(*gmc.SAMPLING_GRIDS["global 5"])}


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    from track_estimators import batch

    hb, db, grids = _sampled_batch()
    ns, nsamples = hb.nsteps, 6
    samples = db.sample_smoothed(nsamples, seed=4).cpu().numpy()
    dtq = np.rint(hb.dt * gmc.TICKS_PER_HOUR).astype(np.int64)
    sound = sum(int(dtq[: ns[b], b].sum()) for b in range(hb.B))
    for name, g in grids.items():
        ref = gmc.grid_metrics(samples, ns, hb.dt, gmc.grid_tuple(g))
        assert not ref["nbroken"].any() and ref["ticks"].any()
        one = batch.grid_statistics(db, g, nsamples, seed=4, chunk=16, entries=True)  # one chunk: sample_smoothed's draws
        assert one["ticks"].dtype == np.int64 and np.array_equal(one["ticks"], ref["ticks"]), name
        assert np.array_equal(one["entries_mean"], ref["entries"] / nsamples)
        assert np.array_equal(one["hours_mean"], ref["ticks"] / (gmc.TICKS_PER_HOUR * nsamples))
        assert np.array_equal(one["outside_hours"], ref["outside"] / gmc.TICKS_PER_HOUR) and not one["nbroken"].any()
        assert np.array_equal(one["total_ticks"], ref["total"]) and not one["status"].any()
        sm = gmc.grid_metrics(db.sm_mean.cpu().numpy()[None], ns, hb.dt, gmc.grid_tuple(g))
        assert np.array_equal(one["hours_smoothed"], sm["ticks"] / gmc.TICKS_PER_HOUR)
        two = batch.grid_statistics(db, g, nsamples, seed=4, chunk=2)                  # chunks of 2: other draws
        assert set(two) == set(one) - {"entries_mean"}
        assert all(two[k].shape == one[k].shape and two[k].dtype == one[k].dtype for k in two)
        assert np.array_equal(two["outside_hours"][:2], one["outside_hours"][:2])  # the first chunk's draws are the same
        assert not np.array_equal(two["ticks"], one["ticks"])                      # the later chunks drew afresh
        for r in (one, two):  # the tracks' total sound time, exactly in ticks
            outside = np.rint(r["outside_hours"] * gmc.TICKS_PER_HOUR).astype(np.int64)
            assert np.array_equal(outside / gmc.TICKS_PER_HOUR, r["outside_hours"])
            assert int(r["ticks"].sum()) + int(outside.sum()) == int(r["total_ticks"].sum()) == nsamples * sound, name
            hours = r["hours_mean"].sum() * nsamples + r["outside_hours"].sum()
            assert abs(hours - nsamples * sound / gmc.TICKS_PER_HOUR) <= 1e-12 * hours
        if name == "local":
            assert 0 < one["outside_hours"].sum() and (one["ticks"] > 0).sum() > 10
    # a HostBatch is uploaded and run first; a list of windows sums into one grid
    g = grids["local"]
    a = batch.grid_statistics(hb, g, 3, seed=9, chunk=3)
    b = batch.grid_statistics(db, g, 3, seed=9, chunk=3)
    assert all(np.array_equal(a[k], b[k]) for k in b) and "entries_mean" not in a
    c = batch.grid_statistics([db.window(0, 4), db.window(4, 6)], g, 3, seed=9, chunk=3)
    assert c["outside_hours"].shape == (3, 6) and c["status"].shape == (6,)
    assert int(c["ticks"].sum()) + int(np.rint(c["outside_hours"] * gmc.TICKS_PER_HOUR).sum()) == int(c["total_ticks"].sum()) == 3 * sound
    assert np.array_equal(c["hours_smoothed"], b["hours_smoothed"])
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.grid_statistics(db, g, 0)
    with pytest.raises(ValueError, match="grid must be a TrackGrid"):
        batch.grid_statistics(db, (0.0, 0.0, 1.0, 1.0, 4, 4), 2)


@pytest.mark.gpu
def test_dropin_time_on_grid():
    """UnscentedKalmanFilter.time_on_grid(): the smoothed track's map for n_samples = 0, the mean map of sample_smoothed's tracks
    for n_samples = 4, both equal to the restatement on the track run() packed."""
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
    grid = batch.track_grid(*gmc.SAMPLING_GRIDS["global 5"])
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.time_on_grid(grid)
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    samples = ukf.sample_smoothed(4, random_state=1)  # (4, N+1, 4)
    lon, lat = samples[0, tsc.NMAX // 2, 0], samples[0, tsc.NMAX // 2, 1]
    grid = batch.track_grid(np.floor(lon * 10.0) / 10.0 - 1.6, np.floor(lat * 10.0) / 10.0 - 1.6, 0.1, 0.1, 32, 32)
    total = int(np.rint(dt * gmc.TICKS_PER_HOUR).sum())
    h0 = ukf.time_on_grid(grid)
    st = batch.grid_statistics(ukf._sample_hb, grid, 4, seed=1, chunk=4)
    assert h0.shape == (32, 32) and h0.dtype == np.float64 and np.array_equal(h0, st["hours_smoothed"])
    assert 0.0 < h0.sum() <= total / gmc.TICKS_PER_HOUR and (h0 > 0.0).sum() > 1
    h4 = ukf.time_on_grid(grid, 4, random_state=1)
    ref = gmc.grid_metrics(samples[..., None], [tsc.NMAX], dt[:, None], gmc.grid_tuple(grid))
    assert h4.shape == (32, 32) and np.array_equal(h4, ref["ticks"] / (gmc.TICKS_PER_HOUR * 4))
    assert np.array_equal(h4, st["hours_mean"]) and int(ref["total"].sum()) == 4 * total
    with pytest.raises(ValueError, match="grid must be a TrackGrid"):
        ukf.time_on_grid((0.0, 0.0, 1.0, 1.0, 4, 4))
    with pytest.raises(ValueError, match="n_samples must be >= 0"):
        ukf.time_on_grid(grid, -1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
