"""Tracks on the device against a polygon (include/ste.h: ste_region_f64, ste_region_metrics_f64; DESIGN.md, "Regions"):
declaration and layout of the C ABI, the NumPy restatement against hand answers and against sampling, and the front end's
refusals (CPU); on the GPU the hand-made tracks, the edges of the lane mapping on a ragged fleet about a concave star across the
antimeridian, independence of the surroundings bit for bit, V = 3 and V = 1024, the bounding-box skip, the sampler's output
through the Python front ends, and the refusals of the call."""
import ctypes as C
import os
import re

import numpy as np
import path_metrics_cases as pmc
import pytest
import region_metrics_cases as rmc
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "nvert", "reserved", "vert", "lon_ref", "time_inside", "first_entry", "nenter", "nbroken",
          "dist_inside", "inside"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint8)


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_region_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_region_f64\* rg, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_region_f64 {"): hdr.index("} ste_region_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|uint8_t|int64_t|double|size_t|void)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteRegionF64._fields_] == FIELDS
    # the layout of the C struct by hand: two int32 share a word, every pointer and the double take one
    offsets = {"nstates": 0, "model": 4, "states": 8, "nvert": 16, "reserved": 20, "vert": 24, "lon_ref": 32, "time_inside": 40,
               "first_entry": 48, "nenter": 56, "nbroken": 64, "dist_inside": 72, "inside": 80}
    assert {f: getattr(binding.SteRegionF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteRegionF64) == 88
    assert "ste_region_metrics_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_region_metrics_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert int(re.search(r"#define STE_REGION_MAX_VERT (\d+)", hdr).group(1)) == binding.STE_REGION_MAX_VERT == 1024
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the region arguments travel beside the batch
    comment = hdr[hdr.index("REGIONS:"): hdr.index("typedef struct ste_region_f64 {")]
    for word in ("Polygon.", "Unwrapping.", "Row inside.", "Step fraction", "Outputs", "BROKEN", "ENTERING", "wrap180"):
        assert word in comment, word


def test_restatement_against_hand_answers():
    """The equator at one degree an hour against the square [2.5, 6.5] x [-1, 1]: inside for 4 h from 2.5 h on, entered once,
    4 degrees of the equator sailed inside.  The same answers with the ring clockwise and closed, and with square and track
    moved across the antimeridian and stored wrapped.  A track cut before the square is never inside; one that starts in it
    entered at time 0."""
    from track_estimators import batch

    first = None
    for name, (ring, shift, wrapped) in rmc.hand_polygons().items():
        poly = batch.region_polygon(ring)
        assert poly.vert.shape == (2, 4) and abs(poly.lon_ref - (4.5 + shift)) < 1e-12, name
        px, py = poly.vert
        assert np.sum(px * np.roll(py, -1) - np.roll(px, -1) * py) > 0.0, name  # counter-clockwise
        st, nsteps, dt = rmc.hand_tracks(shift, wrapped)
        for model in ("sphere", "wgs84"):
            r = rmc.region_metrics(st, nsteps, dt, poly.vert, poly.lon_ref, model)
            assert r["time_inside"][0].tolist() == rmc.HAND_TIME, (name, r["time_inside"])
            assert np.array_equal(r["first_entry"][0], rmc.HAND_FIRST, equal_nan=True), (name, r["first_entry"])
            assert r["nenter"][0].tolist() == rmc.HAND_NENTER and not r["nbroken"].any(), name
            assert np.allclose(r["dist_inside"][0], np.array(rmc.HAND_TIME) * pmc.KM_PER_DEG_EQUATOR, rtol=1e-9, atol=0.0), name
            assert r["inside"][0, :, 0].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
            assert r["inside"][0, :, 1].tolist() == [0] * 11 and r["inside"][0, :, 2].tolist() == [1, 1] + [0] * 9
        first = r if first is None else first
        assert all(np.array_equal(first[k], r[k], equal_nan=True) for k in ("time_inside", "first_entry", "nenter", "inside"))


def test_restatement_against_sampling():
    """A convex hexagon, where a point is inside when it is left of every edge (a rule that shares nothing with the ray test or
    the crossing sum): time_inside of a small random fleet against the mean of that rule over 1000 points of every step.  A
    crossing misplaces at most one sampling interval, dt / 1000, so a track may differ by max(dt) * crossings / 1000."""
    from track_estimators import batch

    rng = np.random.default_rng(3)
    S, N, B = 2, 6, 40
    poly = batch.region_polygon(rmc.star((10.0, 20.0), (1.5,), 6, wrapped=False))
    st = np.zeros((S, N + 1, 4, B))
    start = np.stack([10.0 + rng.uniform(-2.5, 2.5, B), 20.0 + rng.uniform(-2.5, 2.5, B)])
    st[:, 0, :2] = start
    st[:, 1:, :2] = start[None, None] + np.cumsum(rng.normal(0.0, 0.6, (S, N, 2, B)), axis=1)
    nsteps, dt = np.full(B, N), rng.uniform(0.2, 1.5, (N, B))
    r = rmc.region_metrics(st, nsteps, dt, poly.vert, poly.lon_ref)
    px, py = poly.vert
    ex, ey = np.roll(px, -1) - px, np.roll(py, -1) - py
    frac = (np.arange(1000) + 0.5) / 1000.0
    worst, crossed = 0.0, 0
    for s in range(S):
        for t in range(B):
            total = 0.0
            for k in range(N):
                x = st[s, k, 0, t] + frac * (st[s, k + 1, 0, t] - st[s, k, 0, t])
                y = st[s, k, 1, t] + frac * (st[s, k + 1, 1, t] - st[s, k, 1, t])
                left = ex[:, None] * (y[None] - py[:, None]) - ey[:, None] * (x[None] - px[:, None]) > 0.0
                total = total + dt[k, t] * left.all(axis=0).mean()
            ncr = int(r["ncrossings"][s, t])
            tol = dt[:, t].max() * ncr / 1000.0
            err = abs(r["time_inside"][s, t] - total)
            assert err <= tol + 1e-12 * dt[:, t].sum(), (s, t, err, tol, ncr)
            worst, crossed = max(worst, err / tol if ncr else 0.0), crossed + (ncr > 0)
    print(f"restatement against 1000-point sampling: worst error {worst:.3g} of its bound, {crossed} of {S * B} tracks cross")
    assert crossed >= S * B // 4 and (r["time_inside"] > 0.0).mean() > 0.25 and (r["time_inside"] == 0.0).any()


def test_front_end_refusals():
    from track_estimators import batch

    sq = rmc.SQUARE
    with pytest.raises(ValueError, match="between 3 and 1024"):
        batch.region_polygon(sq[:2])
    with pytest.raises(ValueError, match="between 3 and 1024"):
        batch.region_polygon(np.concatenate([sq[:2], sq[:1]]))  # two vertices and the closing one
    with pytest.raises(ValueError, match="between 3 and 1024"):
        batch.region_polygon(rmc.star((0.0, 0.0), (1.0,), 1025))
    assert batch.region_polygon(rmc.star((0.0, 0.0), (1.0,), 1024)).vert.shape == (2, 1024)
    assert batch.region_polygon(np.concatenate([rmc.star((0.0, 0.0), (1.0,), 1024), rmc.star((0.0, 0.0), (1.0,), 1)])).vert.shape == (2, 1024)
    for bad in (np.nan, np.inf):
        ring = sq.copy()
        ring[2, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            batch.region_polygon(ring)
    with pytest.raises(ValueError, match="degrees of longitude"):
        batch.region_polygon([[-91.0, 0.0], [91.0, 0.0], [0.0, 10.0]])
    assert batch.region_polygon([[-89.0, 0.0], [89.0, 0.0], [0.0, 10.0]]).lon_ref == 0.0
    with pytest.raises(ValueError, match=r"\(V, 2\)"):
        batch.region_polygon(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="zero area"):
        batch.region_polygon([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])


def test_fleet_is_a_fair_sample():
    """The mapping fleet on the restatement alone: enough tracks enter, re-enter, start inside and stay outside for the GPU tests
    to mean something; the NaN-latitude track and the 120-degree jump follow the rule for broken steps."""
    r, w = rmc.fleet_reference("star", rmc.star12(), "sphere"), rmc.fleet()
    ne = r["nenter"]
    shares = ((ne > 0).mean(), (ne >= 2).mean(), r["inside"][:, 0].mean(), (ne == 0).mean())
    print("fleet: enter %.3f, enter twice or more %.3f, start inside %.3f, never enter %.3f" % shares)
    assert shares[0] >= 0.20 and shares[1] >= 0.05 and shares[2] >= 0.05 and shares[3] >= 0.40
    assert {0, 1, rmc.FLEET_N} <= set(w["nsteps"].tolist())
    # a NaN latitude in row 4 breaks the two steps that touch it; row 5 is inside while row 4 is not: entered at T_5
    b = rmc.NAN_TRACK
    T = np.concatenate([[0.0], np.cumsum(w["dt"][:, b])])
    assert (r["nbroken"][:, b] == 2).all() and (ne[:, b] == 1).all() and (r["first_entry"][:, b] == T[5]).all()
    assert np.allclose(r["time_inside"][:, b], w["dt"][5:, b].sum(), rtol=1e-14)
    # the jump of 120 degrees is step 3: row 4 is inside while row 3 is not: entered at T_4, and steps 4 .. 7 are inside
    b = rmc.JUMP_TRACK
    T = np.concatenate([[0.0], np.cumsum(w["dt"][:, b])])
    assert (r["nbroken"][:, b] == 1).all() and (ne[:, b] == 1).all() and (r["first_entry"][:, b] == T[4]).all()
    assert np.allclose(r["time_inside"][:, b], w["dt"][4:, b].sum(), rtol=1e-14)
    assert r["nbroken"].sum() == 3 * rmc.FLEET_S


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, what):
    """nenter, nbroken, inside and the NaN pattern of first_entry exactly; times at TIME_RTOL of the track's total time;
    dist_inside at DIST_ATOL + DIST_RTOL x the track's total distance.  Prints the worst figures before it asserts."""
    for k in ("nenter", "nbroken", "inside"):
        if k in got:
            assert np.array_equal(got[k], ref[k]), (what, k)
    worst, bitwise = {}, {}
    if "first_entry" in got:
        assert np.array_equal(np.isnan(got["first_entry"]), np.isnan(ref["first_entry"])), what
        assert np.array_equal(np.isnan(ref["first_entry"]), ref["nenter"] == 0)
    for k in ("time_inside", "first_entry"):
        if k not in got:
            continue
        tol = pmc.TIME_RTOL * np.broadcast_to(ref["total_time"], got[k].shape)
        err, ok = np.abs(got[k] - ref[k]), ~np.isnan(ref[k])
        assert (err[ok & (tol == 0.0)] == 0.0).all(), (what, k)
        live = ok & (tol > 0.0)
        worst[k] = float((err[live] / tol[live]).max()) if live.any() else 0.0
        bitwise[k] = bool(np.array_equal(_bits(got[k]), _bits(ref[k])))
    if "dist_inside" in got:
        tol = pmc.DIST_ATOL + pmc.DIST_RTOL * ref["total_dist"]
        worst["dist_inside"] = float((np.abs(got["dist_inside"] - ref["dist_inside"]) / tol).max())
    print(f"{what}: worst error as a fraction of its tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + "; bit for bit: " + ", ".join(f"{k} {v}" for k, v in bitwise.items()))
    for k, v in worst.items():
        assert v <= 1.0, (what, k, v)


@pytest.mark.gpu
def test_hand_made_tracks_on_the_device():
    """The CPU anchors through the kernel, S = 1, B = 3, both models: the square counter-clockwise, clockwise and closed, and
    across the antimeridian with the tracks stored wrapped."""
    from track_estimators import batch

    for name, (ring, shift, wrapped) in rmc.hand_polygons().items():
        st, nsteps, dt = rmc.hand_tracks(shift, wrapped)
        db = batch.DeviceBatch(pmc.bare_batch(nsteps, dt), histories=False)
        poly = batch.region_polygon(ring)
        for model in ("sphere", "wgs84"):
            got = _host(db.region_metrics(_dev(db, st), ring, model=model, distance=True, mask=True))
            _compare(got, rmc.region_metrics(st, nsteps, dt, poly.vert, poly.lon_ref, model), f"hand-made tracks, {name}, {model}")
            assert np.abs(got["time_inside"][0] - rmc.HAND_TIME).max() <= pmc.TIME_RTOL * rmc.HAND_N, (name, got["time_inside"])
            assert abs(got["first_entry"][0, 0] - 2.5) <= pmc.TIME_RTOL * rmc.HAND_N and got["first_entry"][0, 2] == 0.0
            assert np.isnan(got["first_entry"][0, 1]) and got["nenter"][0].tolist() == rmc.HAND_NENTER and not got["nbroken"].any()
            assert np.allclose(got["dist_inside"][0], np.array(rmc.HAND_TIME) * pmc.KM_PER_DEG_EQUATOR, rtol=pmc.DIST_RTOL,
                               atol=pmc.DIST_ATOL), (name, model)


def _fleet_batch():
    from track_estimators import batch

    w = rmc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_edges_of_the_mapping(model):
    """S = 5, Nmax = 8, B = 130, ragged, about the concave star across the antimeridian: parity with the restatement; NaN in the
    rows past nsteps changes no output bit; mask rows past nsteps keep their zeros; the NaN-latitude and the jump track report
    their broken steps and the end-of-step entry.
    Measured on an MI355X: time_inside and first_entry equal bit for bit; dist_inside at 2.3e-6 of its tolerance (rtol 1e-10 of
    the track's distance, atol 1e-12 km) on the sphere and 3.7e-4 on WGS84."""
    w, db, full = _fleet_batch()
    ref = rmc.fleet_reference("star", rmc.star12(), model)
    got = _host(db.region_metrics(full, rmc.star12(), model=model, distance=True, mask=True))
    _compare(got, ref, f"mapping fleet, star, {model}")
    assert (got["nbroken"][:, rmc.NAN_TRACK] == 2).all() and (got["nbroken"][:, rmc.JUMP_TRACK] == 1).all()
    for b, row in ((rmc.NAN_TRACK, 5), (rmc.JUMP_TRACK, 4)):
        assert (got["nenter"][:, b] == 1).all() and (got["inside"][:, row - 1, b] == 0).all() and (got["inside"][:, row, b] == 1).all()
        assert np.array_equal(_bits(got["first_entry"][:, b]), _bits(ref["first_entry"][:, b]))
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.region_metrics(_dev(db, poisoned), rmc.star12(), model=model, distance=True, mask=True))
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, "rows past nsteps were read")
    for b, ns in enumerate(w["nsteps"]):
        assert not got["inside"][:, ns + 1:, b].any(), (b, "mask rows past nsteps were written")


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """The window [3, 70) of the fleet (read in place, and as a contiguous copy) against those columns of the whole-fleet call;
    S = 1 slices against the S = 5 call; a call for time_inside alone against one for every output; and the ring rotated by one
    vertex: equal counts and masks, times within tolerance (the order of the crossing sum changes)."""
    from track_estimators import batch
    from track_estimators._hip import binding

    w, db, full = _fleet_batch()
    ring = rmc.star12()
    kw = dict(model="wgs84", distance=True, mask=True)
    whole = _host(db.region_metrics(full, ring, **kw))
    lo, hi = rmc.FLEET_WINDOW
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == rmc.FLEET_B
    in_place = _host(win.region_metrics(full[..., lo:hi], ring, **kw))
    copied = _host(win.region_metrics(full[..., lo:hi].contiguous(), ring, **kw))
    slices = [_host(db.region_metrics(full[s:s + 1], ring, **kw)) for s in range(rmc.FLEET_S)]
    plain = _host(db.region_metrics(full, ring))
    assert set(plain) == {"time_inside", "first_entry", "nenter", "nbroken"} and set(whole) == set(plain) | {"dist_inside", "inside"}
    for k, v in whole.items():
        cols = _bits(v[..., lo:hi])
        assert np.array_equal(cols, _bits(in_place[k])), (k, "window")
        assert np.array_equal(cols, _bits(copied[k])), (k, "window copy")
        for s in range(rmc.FLEET_S):
            assert np.array_equal(_bits(v[s:s + 1]), _bits(slices[s][k])), (k, s, "S = 5 / S = 1")
        if k in plain:
            assert np.array_equal(_bits(v), _bits(plain[k])), (k, "with / without distance and mask")
    # time_inside alone, through the C ABI
    torch = db.torch
    poly = batch.region_polygon(ring)
    vert = _dev(db, poly.vert)
    alone = torch.empty((rmc.FLEET_S, rmc.FLEET_B), dtype=torch.float64, device=db.device)
    rg = binding.SteRegionF64()
    rg.nstates, rg.states, rg.nvert, rg.vert, rg.lon_ref = rmc.FLEET_S, full.data_ptr(), 12, vert.data_ptr(), poly.lon_ref
    rg.time_inside = alone.data_ptr()
    binding.check(db.lib.ste_region_metrics_f64(C.byref(db.struct), C.byref(rg), db._stream(None)), "ste_region_metrics_f64")
    assert np.array_equal(_bits(alone.cpu().numpy()), _bits(whole["time_inside"])), "time_inside alone"
    # the ring rotated by one position
    rolled = batch.RegionPolygon(vert=np.ascontiguousarray(np.roll(poly.vert, 1, axis=1)), lon_ref=poly.lon_ref)
    got = _host(db.region_metrics(full, rolled, **kw))
    _compare(got, rmc.fleet_reference("star", ring, "wgs84"), "mapping fleet, star rotated by one vertex against the star")
    _compare(got, rmc.fleet_reference("rolled", rolled, "wgs84"), "mapping fleet, star rotated by one vertex")


@pytest.mark.gpu
@pytest.mark.parametrize("nvert", [3, 1024])
def test_fewest_and_most_vertices(nvert):
    """V = 3 (a triangle) and V = STE_REGION_MAX_VERT (a 1024-gon), both inscribed in the star's circumscribed circle."""
    w, db, full = _fleet_batch()
    ring = rmc.star((rmc.CENTRE[0], rmc.CENTRE[1]), (1.2,), nvert)
    ref = rmc.fleet_reference(f"circle{nvert}", ring, "sphere")
    assert (ref["nenter"] > 0).mean() > 0.1
    got = _host(db.region_metrics(full, ring, distance=True, mask=True))
    _compare(got, ref, f"mapping fleet, {nvert} vertices")


@pytest.mark.gpu
def test_region_far_away():
    """The star moved 60 degrees east: no step's box meets the polygon's, the edge loop never runs, and every output is 0 / NaN /
    0 with an all-zero mask -- as the restatement has it; the 120-degree jump is still a broken step."""
    w, db, full = _fleet_batch()
    ring = rmc.star12(east=60.0)
    got = _host(db.region_metrics(full, ring, distance=True, mask=True))
    _compare(got, rmc.fleet_reference("far", ring, "sphere"), "mapping fleet, star 60 degrees east")
    assert not got["time_inside"].any() and not got["dist_inside"].any() and not got["nenter"].any() and not got["inside"].any()
    assert np.isnan(got["first_entry"]).all()
    assert got["nbroken"].sum() == 3 * rmc.FLEET_S


def _sampled_batch():
    """Six synthetic tracks of 20 steps, ragged, forward pass and smoother done; and a box whose west edge runs through the
    middle row of track 0, so that when its posterior samples enter, and whether, differs from sample to sample."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(synthetic.make_batch(6, nobs=11, seed0=100), 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 13, 7, 1, 0], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    lon, lat = (float(v) for v in db.sm_mean[10, :2, 0].cpu().numpy())
    ring = np.array([[lon, lat - 30.0], [lon + 90.0, lat - 30.0], [lon + 90.0, lat + 30.0], [lon, lat + 30.0]])
    return hb, db, ring


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    from track_estimators import batch

    hb, db, ring = _sampled_batch()
    poly = batch.region_polygon(ring)
    ns, N = hb.nsteps, hb.Nmax
    # the sampler's output and the smoothed track against the restatement
    samples = db.sample_smoothed(10, seed=4)
    direct = _host(db.region_metrics(samples, ring, distance=True, mask=True))
    _compare(direct, rmc.region_metrics(samples.cpu().numpy(), ns, hb.dt, poly.vert, poly.lon_ref, "sphere"), "sampled tracks")
    sm = _host(db.region_metrics(db.sm_mean, ring, mask=True))
    _compare(sm, rmc.region_metrics(db.sm_mean.cpu().numpy()[None], ns, hb.dt, poly.vert, poly.lon_ref), "smoothed tracks")
    # one chunk: the draws of sample_smoothed(10, seed), bit for bit
    one = batch.region_statistics(db, ring, 10, seed=4, chunk=16, distance=True)
    for k in ("time_inside", "first_entry", "nenter", "dist_inside"):
        assert np.array_equal(_bits(one[k]), _bits(direct[k])), k
    live = np.arange(N + 1)[:, None] <= ns[None, :]
    assert np.array_equal(one["occupancy"][live], direct["inside"].mean(axis=0)[live]) and np.isnan(one["occupancy"][~live]).all()
    assert np.array_equal(_bits(one["time_inside_smoothed"]), _bits(sm["time_inside"][0]))
    assert one["inside_smoothed"].dtype == bool and np.array_equal(one["inside_smoothed"], sm["inside"][0].astype(bool))
    # chunks of 4, 4, 2: other draws, the same shapes
    q = (0.1, 0.5, 0.9)
    st = batch.region_statistics(db, ring, 10, seed=4, chunk=4, distance=True, quantiles=q)
    ref = batch.region_statistics(db, ring, 10, seed=4, chunk=16, distance=True, quantiles=q)
    assert set(st) == set(ref) and all(st[k].shape == ref[k].shape and st[k].dtype == ref[k].dtype for k in ref)
    assert st["time_inside"].shape == st["first_entry"].shape == st["nenter"].shape == st["dist_inside"].shape == (10, 6)
    assert st["time_inside_quantiles"].shape == st["first_entry_quantiles"].shape == (3, 6)
    assert st["occupancy"].shape == st["inside_smoothed"].shape == (N + 1, 6)
    assert st["entry_prob"].shape == st["time_inside_mean"].shape == st["time_inside_std"].shape == st["status"].shape == (6,)
    assert np.array_equal(_bits(st["time_inside"][:4]), _bits(ref["time_inside"][:4]))  # the first chunk's draws are the same
    assert not np.array_equal(st["time_inside"][4:, 0], ref["time_inside"][4:, 0])       # the later chunks drew afresh
    for r in (st, ref):
        assert ((r["entry_prob"] >= 0.0) & (r["entry_prob"] <= 1.0)).all() and not r["status"].any()
        assert np.array_equal(r["entry_prob"], (r["nenter"] > 0).mean(axis=0))
        live = np.arange(N + 1)[:, None] <= ns[None, :]
        assert np.array_equal(np.isnan(r["occupancy"]), ~live)
        assert ((r["occupancy"][live] >= 0.0) & (r["occupancy"][live] <= 1.0)).all()
        some = r["entry_prob"] > 0.0
        assert np.isfinite(r["first_entry_quantiles"][:, some]).all() and np.isnan(r["first_entry_quantiles"][:, ~some]).all()
        assert (np.diff(r["time_inside_quantiles"], axis=0) >= 0.0).all()
        assert (r["time_inside"] <= hb.dt.sum(axis=0)[None] * (1.0 + 1e-12)).all()
    # the west edge runs through the middle of track 0: its samples are inside for different times
    assert ref["time_inside_std"][0] > 0.0 and 0.0 < ref["time_inside_smoothed"][0] < hb.dt[:, 0].sum()
    # a HostBatch is uploaded and run first: same values as the resident batch
    a = batch.region_statistics(hb, ring, 4, seed=9, chunk=4)
    b = batch.region_statistics(db, ring, 4, seed=9, chunk=4)
    assert np.array_equal(_bits(a["time_inside"]), _bits(b["time_inside"])) and "dist_inside" not in a
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.region_metrics(db.sm_mean[:, :, :5], ring)
    with pytest.raises(ValueError, match="model must be"):
        db.region_metrics(db.sm_mean, ring, model="flat")
    with pytest.raises(ValueError, match="between 3 and 1024"):
        db.region_metrics(db.sm_mean, ring[:2])


@pytest.mark.gpu
def test_dropin_time_in_region():
    """UnscentedKalmanFilter.time_in_region(): the smoothed track's time is region_statistics' time_inside_smoothed for the track
    run() packed; with samples, the times of sample_smoothed's tracks."""
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
        ukf.time_in_region(rmc.SQUARE)
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    samples = ukf.sample_smoothed(5, random_state=1)  # (5, N+1, 4)
    lon, lat = samples[0, tsc.NMAX // 2, 0], samples[0, tsc.NMAX // 2, 1]
    ring = np.array([[lon, lat - 30.0], [lon + 90.0, lat - 30.0], [lon + 90.0, lat + 30.0], [lon, lat + 30.0]])
    t = ukf.time_in_region(ring)
    st = batch.region_statistics(ukf._sample_hb, ring, 5, seed=1, chunk=5)
    assert isinstance(t, float) and t == st["time_inside_smoothed"][0] and 0.0 <= t <= dt.sum()
    ts = ukf.time_in_region(ring, 5, random_state=1)
    assert ts.shape == (5,) and np.array_equal(_bits(ts), _bits(st["time_inside"][:, 0]))
    # ... and they are the times of sample_smoothed's tracks, by the restatement
    poly = batch.region_polygon(ring)
    ref = rmc.region_metrics(samples[..., None], [tsc.NMAX], dt[:, None], poly.vert, poly.lon_ref)
    assert np.abs(ts - ref["time_inside"][:, 0]).max() <= pmc.TIME_RTOL * dt.sum()
    assert 0.0 < ts[0] < dt.sum()  # the west edge runs through the middle row of sample 0


@pytest.mark.gpu
def test_refusals_before_any_launch():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2), and the pointers below are not memory, so a launch that happened would fault."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.dt, s.nsteps = 0x1000, 0x2000
        return s

    def good_region():
        rg = binding.SteRegionF64()
        rg.nstates, rg.model, rg.states, rg.nvert, rg.vert, rg.lon_ref = 3, binding.STE_PREP_SPHERE, 0x3000, 12, 0x4000, 10.0
        rg.time_inside, rg.first_entry, rg.nenter, rg.nbroken, rg.dist_inside, rg.inside = 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xA000
        return rg

    def refused(reason, **fields):
        s, rg = good_batch(), good_region()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(rg, name) else rg, name, value)
        rc = lib.ste_region_metrics_f64(ref(s), ref(rg), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_region_metrics_f64" in msg, (fields, rc, msg)

    for s, rg, reason in ((None, good_region(), "batch pointer is NULL"), (good_batch(), None, "region arguments (rg) are NULL")):
        assert lib.ste_region_metrics_f64(ref(s), ref(rg), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_region_metrics_f64" in msg
    refused("rg->states is required", states=None)
    refused("rg->vert is required", vert=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for v in (2, 0, -1, 1025):
        refused("nvert must be between 3 and", nvert=v)
    refused("rg->reserved must be 0", reserved=1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused("lon_ref must be finite", lon_ref=bad)
    for m in (-1, 2, 7):
        refused("rg->model must be", model=m)
    refused("need the batch's dt", dt=None)
    refused("need the batch's dt", dt=None, time_inside=None)  # first_entry alone needs it too
    refused("need the batch's dt", dt=None, first_entry=None)
    nothing = dict(time_inside=None, first_entry=None, nenter=None, nbroken=None, dist_inside=None, inside=None)
    refused("no output asked for", **nothing)
    refused("no output asked for", model=7, dt=None, **nothing)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
