"""Distance sailed and line-crossing times of tracks on the device (include/ste.h: ste_path_f64, ste_path_metrics_f64;
DESIGN.md, "Path quantities"): declaration and refusals of the C ABI and the NumPy restatement on hand-made tracks (CPU); on
the GPU the same hand-made tracks, the edges of the lane mapping on a ragged random-walk fleet, independence of the
surroundings (sample count, windows, the other outputs) bit for bit, the sampler's output, and the Python front ends."""
import ctypes as C
import os
import re

import numpy as np
import path_metrics_cases as pmc
import pytest
import track_sampling_cases as tsc
from conftest import ROOT


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_path_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_path_f64\* pm, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_path_f64 {"): hdr.index("} ste_path_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double|size_t|void)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.StePathF64._fields_] == [
        "nstates", "model", "states", "dist", "cumdist", "line_axis", "reserved", "line_value", "cross_time", "ncross"]
    assert C.sizeof(binding.StePathF64) == 64
    assert "ste_path_metrics_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_path_metrics_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the path arguments travel beside the batch
    # the definitions travel with the declaration
    comment = hdr[hdr.index("PATH QUANTITIES"): hdr.index("typedef struct ste_path_f64 {")]
    for word in ("Leg.", "Distance.", "Offset from the line", "Crossing.", "Crossing time.", "Non-finite values.", "wrap180"):
        assert word in comment, word


def test_refusals_before_any_launch():
    """Every refusal of the header returns STE_EINVAL (-1) with its reason and the call's name; a launch on a machine without a
    GPU would return STE_ELAUNCH (-2), so -1 shows the call stopped before launching (tests/test_track_sampling.py)."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.dt, s.nsteps = 0x1000, 0x2000
        return s

    def good_path():
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.cumdist = 3, binding.STE_PREP_SPHERE, 0x3000, 0x4000, 0x5000
        pm.line_axis, pm.line_value, pm.cross_time, pm.ncross = 1, 0x6000, 0x7000, 0x8000
        return pm

    def refused(reason, batch=None, path=None, **fields):
        s, pm = good_batch() if batch is None else batch, good_path() if path is None else path
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(pm, name) else pm, name, value)
        rc = lib.ste_path_metrics_f64(ref(s), ref(pm), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_path_metrics_f64" in msg, (fields, rc, msg)

    for s, pm, reason in ((None, good_path(), "batch pointer is NULL"), (good_batch(), None, "path arguments (pm) are NULL")):
        assert lib.ste_path_metrics_f64(ref(s), ref(pm), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_path_metrics_f64" in msg
    refused("pm->states is required", states=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for m in (-1, 2, 7):
        refused("pm->model must be", model=m)
    for ax in (-2, 2):
        refused("pm->line_axis must be", line_axis=ax)
    refused("pm->reserved must be 0", reserved=1)
    refused("a line needs pm->line_value", line_value=None)
    for ax in (0, 1):
        refused("a line needs the batch's dt", line_axis=ax, dt=None)
    refused("need a line", line_axis=-1, line_value=None, ncross=None)  # cross_time without a line
    refused("need a line", line_axis=-1, line_value=None, cross_time=None)  # ncross without a line
    refused("no output asked for", dist=None, cumdist=None, cross_time=None, ncross=None)
    refused("no output asked for", dist=None, cumdist=None, cross_time=None, ncross=None, line_axis=-1)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)


def test_restatement_on_hand_made_tracks():
    """n legs of one degree on the equator are n * 6378.137 * pi / 180 km on either model (the WGS84 equator is a geodesic of
    that radius); with dt = 1 the meridian 2.5 is crossed at 2.5 h; 179 -> 181 and 179 -> -179 are the same leg, cross the
    meridian 180 once and the meridian 0 never."""
    n = 6
    st = pmc.states_of([pmc.equator_track(n)])
    dt = np.ones((n, 1))
    for model in ("sphere", "wgs84"):
        r = pmc.path_metrics(st, [n], dt, model, "lon", 2.5)
        assert np.isclose(r["distance"][0, 0], n * pmc.KM_PER_DEG_EQUATOR, rtol=1e-12, atol=0.0), model
        assert np.allclose(r["cumulative"][0, :, 0], np.arange(n + 1) * pmc.KM_PER_DEG_EQUATOR, rtol=1e-12, atol=0.0), model
        assert np.isclose(r["cross_time"][0, 0], 2.5, rtol=1e-12, atol=0.0) and r["ncross"][0, 0] == 1
    # a shorter track of the same rows: rows past nsteps are not looked at
    r = pmc.path_metrics(st, [2], dt, "sphere", "lon", 2.5)
    assert np.isclose(r["distance"][0, 0], 2 * pmc.KM_PER_DEG_EQUATOR, rtol=1e-12) and np.isnan(r["cross_time"][0, 0])
    assert r["ncross"][0, 0] == 0 and np.isnan(r["cumulative"][0, 3:, 0]).all()
    r = pmc.path_metrics(st, [0], dt, "sphere", "lat", 0.0)
    assert r["distance"][0, 0] == 0.0 and np.isnan(r["cross_time"][0, 0]) and r["ncross"][0, 0] == 0
    # the antimeridian, unwrapped and wrapped
    st = pmc.states_of([[[179.0, 10.0], [181.0, 10.0]], [[179.0, 10.0], [-179.0, 10.0]]])
    dt = np.ones((1, 2))
    for model in ("sphere", "wgs84"):
        r = pmc.path_metrics(st, [1, 1], dt, model, "lon", 180.0)
        assert np.isclose(r["distance"][0, 0], r["distance"][0, 1], rtol=1e-12, atol=0.0) and r["distance"][0, 0] > 200.0
        assert (r["ncross"] == 1).all() and np.allclose(r["cross_time"], 0.5, rtol=1e-12, atol=0.0)
        r = pmc.path_metrics(st, [1, 1], dt, model, "lon", 0.0)
        assert (r["ncross"] == 0).all() and np.isnan(r["cross_time"]).all()
    # a parallel touched from below and left again counts once per sign change; a NaN row poisons the distance, not the count
    st = pmc.states_of([[[0.0, -1.0], [0.0, 1.0], [0.0, -1.0], [0.0, np.nan], [0.0, 1.0]]])
    r = pmc.path_metrics(st, [4], np.full((4, 1), 2.0), "sphere", "lat", 0.0)
    assert r["ncross"][0, 0] == 2 and r["cross_time"][0, 0] == 1.0 and np.isnan(r["distance"][0, 0])


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, nsteps, what):
    """distance and cumulative at DIST_RTOL / DIST_ATOL, crossing times at TIME_RTOL of the track's total time; ncross and the
    NaN pattern exactly.  Prints the worst figures before it asserts."""
    d_err = np.abs(got["distance"] - ref["distance"]) / (pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref["distance"]))
    worst = {"distance": float(d_err.max())}
    if "cumulative" in got:
        live = np.arange(ref["cumulative"].shape[1])[None, :, None] <= np.asarray(nsteps)[None, None, :]
        c_err = np.abs(got["cumulative"] - ref["cumulative"]) / (pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref["cumulative"]))
        assert not np.isnan(got["cumulative"][np.broadcast_to(live, c_err.shape)]).any(), what
        worst["cumulative"] = float(c_err[np.broadcast_to(live, c_err.shape)].max())
    if "cross_time" in got:
        assert np.array_equal(got["ncross"], ref["ncross"]), what
        assert np.array_equal(np.isnan(got["cross_time"]), np.isnan(ref["cross_time"])), what
        assert np.array_equal(np.isnan(ref["cross_time"]), ref["ncross"] == 0)
        hit = ~np.isnan(ref["cross_time"])
        t_err = np.abs(got["cross_time"] - ref["cross_time"]) / (pmc.TIME_RTOL * np.broadcast_to(ref["total_time"], hit.shape))
        worst["cross_time"] = float(t_err[hit].max()) if hit.any() else 0.0
    print(f"{what}: worst error as a fraction of its tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (what, k, v)


@pytest.mark.gpu
def test_hand_made_tracks_on_the_device():
    """The CPU anchors through the kernel, both models: the equator, the meridian 2.5 crossed at 2.5 h, the antimeridian
    unwrapped and wrapped, nsteps 0, and a NaN row."""
    from track_estimators import batch

    n = 6
    eq = pmc.equator_track(n)
    anti_a = np.concatenate([[[179.0, 10.0], [181.0, 10.0]], np.full((n - 1, 2), np.nan)])
    anti_b = np.concatenate([[[179.0, 10.0], [-179.0, 10.0]], np.full((n - 1, 2), np.nan)])
    zig = np.concatenate([[[0.0, -1.0], [0.0, 1.0], [0.0, -1.0], [0.0, np.nan], [0.0, 1.0]], np.full((n - 4, 2), np.nan)])
    st = pmc.states_of([eq, eq, eq, anti_a, anti_b, anti_a, anti_b, zig])
    nsteps = np.array([n, 2, 0, 1, 1, 1, 1, 4], dtype=np.int32)
    dt = np.ones((n, 8))
    lon_line = np.array([2.5, 2.5, 2.5, 180.0, 180.0, 0.0, 0.0, 0.0])
    db = batch.DeviceBatch(pmc.bare_batch(nsteps, dt), histories=False)
    for model in ("sphere", "wgs84"):
        got = _host(db.path_metrics(_dev(db, st), model=model, cumulative=True, line_axis="lon", line_value=lon_line))
        ref = pmc.path_metrics(st, nsteps, dt, model, "lon", lon_line)
        what = f"hand-made tracks, {model}"
        assert np.array_equal(np.isnan(got["distance"]), np.isnan(ref["distance"])), what
        ok = ~np.isnan(ref["distance"][0])
        _compare({k: v[..., ok] for k, v in got.items()}, {k: v[..., ok] for k, v in ref.items()}, nsteps[ok], what)
        d, ct, nc = got["distance"][0], got["cross_time"][0], got["ncross"][0]
        assert np.isclose(d[0], n * pmc.KM_PER_DEG_EQUATOR, rtol=pmc.DIST_RTOL, atol=pmc.DIST_ATOL)
        assert np.isclose(d[1], 2 * pmc.KM_PER_DEG_EQUATOR, rtol=pmc.DIST_RTOL, atol=pmc.DIST_ATOL) and d[2] == 0.0
        assert abs(ct[0] - 2.5) <= pmc.TIME_RTOL * n and nc[0] == 1 and np.isnan(ct[1:3]).all() and not nc[1:3].any()
        assert np.isclose(d[3], d[4], rtol=pmc.DIST_RTOL, atol=pmc.DIST_ATOL) and d[3] > 200.0
        assert list(nc[3:7]) == [1, 1, 0, 0] and np.allclose(ct[3:5], 0.5, rtol=pmc.TIME_RTOL, atol=0.0) and np.isnan(ct[5:7]).all()
        assert np.isnan(d[7]) and nc[7] == 0  # the meridian 0 along lon = 0: offsets are 0, nothing is negative
        lat = _host(db.path_metrics(_dev(db, st), model=model, line_axis="lat", line_value=0.0))
        assert lat["ncross"][0, 7] == 2 and lat["cross_time"][0, 7] == 0.5 and np.isnan(lat["distance"][0, 7])


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_edges_of_the_mapping(model):
    """S = 5, Nmax = 8, B = 130, ragged: parity with the restatement with a line on each axis; NaN in the rows past nsteps
    changes no output bit; cumulative rows past nsteps keep their fill; distance is cumulative row nsteps bit for bit.
    Measured on an MI355X, as a fraction of the tolerances (rtol 1e-10, atol 1e-12 km): distance 3.4e-6, cumulative 4.4e-6 on the
    sphere; 1.4e-3 and 5.3e-3 on WGS84; crossing times equal bit for bit."""
    from track_estimators import batch

    w = pmc.walk()
    nsteps = w["nsteps"]
    assert {0, 1, pmc.WALK_N} <= set(nsteps.tolist())
    db = batch.DeviceBatch(pmc.bare_batch(nsteps, w["dt"]), histories=False)
    poisoned = w["states"].copy()
    for b, ns in enumerate(nsteps):
        poisoned[:, ns + 1:, :, b] = np.nan
    for axis in ("lon", "lat"):
        ref = pmc.walk_reference(model, axis)
        crossing = ~np.isnan(ref["cross_time"])
        assert crossing.any() and (~crossing.any(axis=0) & (nsteps > 0)).any(), "the lines must split the fleet"
        kw = dict(model=model, cumulative=True, line_axis=axis, line_value=w[axis + "_line"])
        got = _host(db.path_metrics(_dev(db, w["states"]), **kw))
        _compare(got, ref, nsteps, f"random walk, {model}, line on {axis}")
        again = _host(db.path_metrics(_dev(db, poisoned), **kw))
        for k in got:
            assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), (axis, k, "rows past nsteps were read")
        for b, ns in enumerate(nsteps):
            assert np.isnan(got["cumulative"][:, ns + 1:, b]).all(), (b, "cumulative rows past nsteps were written")
            assert np.array_equal(_u64(got["distance"][:, b]), _u64(got["cumulative"][:, ns, b])), b
            assert (got["cumulative"][:, 0, b] == 0.0).all()


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Sample s of an S = 5 call equals an S = 1 call on that slice; the window [3, 70) of the B = 130 fleet (track_stride 130,
    read in place, and as a contiguous copy) equals columns 3 .. 69 of the whole-fleet call; distance-only outputs equal those
    of a call that also asks for a line."""
    from track_estimators import batch

    w = pmc.walk()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    full = _dev(db, w["states"])
    lo, hi = pmc.WALK_WINDOW
    for model in ("sphere", "wgs84"):
        kw = dict(model=model, cumulative=True, line_axis="lon", line_value=w["lon_line"])
        whole = _host(db.path_metrics(full, **kw))
        one = _host(db.path_metrics(full[2:3], **kw))
        plain = _host(db.path_metrics(full, model=model, cumulative=True))
        win = db.window(lo, hi)
        assert int(win.struct.track_stride) == pmc.WALK_B
        kw["line_value"] = w["lon_line"][lo:hi]
        in_place = _host(win.path_metrics(full[..., lo:hi], **kw))
        copied = _host(win.path_metrics(full[..., lo:hi].contiguous(), **kw))
        for k, v in whole.items():
            bits = v.view(np.uint8 if v.dtype == np.int32 else np.uint64)
            same = lambda other: np.array_equal(bits, other.view(bits.dtype))  # noqa: E731
            assert np.array_equal(bits[2:3], one[k].view(bits.dtype)), (model, k, "S = 5 / S = 1")
            cols = np.ascontiguousarray(v[..., lo:hi])
            assert np.array_equal(cols.view(bits.dtype), np.ascontiguousarray(in_place[k]).view(bits.dtype)), (model, k, "window")
            assert np.array_equal(cols.view(bits.dtype), np.ascontiguousarray(copied[k]).view(bits.dtype)), (model, k, "window copy")
            if k in plain:
                assert same(plain[k]), (model, k, "with / without a line")
        assert set(plain) == {"distance", "cumulative"}


def _sampled_batch():
    """The eight tracks of the sampler's tests plus a ragged copy, forward pass and smoother done."""
    from track_estimators import batch

    ragged = [0, 1, 2, 5, 7, 9, 11, 12]
    hb = tsc.host_batch(np.arange(16) % 8, [tsc.NMAX] * 8 + ragged)
    db = batch.DeviceBatch(hb)
    db.run()
    return hb, db


@pytest.mark.gpu
def test_through_the_sampler():
    """S = 3 recorded draws on the eight tracks plus their ragged copy: path_metrics(sample_smoothed(...)) against the
    restatement on the downloaded samples, path_metrics(sm_mean) against the restatement on download("means_smoothed"), and
    zero draws give the smoothed track's distance bit for bit."""
    hb, db = _sampled_batch()
    torch = db.torch
    draws = np.random.default_rng(5).standard_normal((3, tsc.NMAX + 1, 4, 16))
    samples = db.sample_smoothed(3, draws=_dev(db, draws))
    assert not db.sample_status.cpu().numpy().any()
    sm = db.download(("means_smoothed",))["means_smoothed"]  # (B, N+1, 4)
    sm_states = np.ascontiguousarray(sm.transpose(1, 2, 0))[None]
    ns = hb.nsteps
    mid = sm[np.arange(16), ns // 2]  # a line through every smoothed track's middle row
    for model in ("sphere", "wgs84"):
        for axis, c in (("lon", 0), ("lat", 1)):
            kw = dict(model=model, cumulative=True, line_axis=axis, line_value=mid[:, c])
            got = _host(db.path_metrics(samples, **kw))
            ref = pmc.path_metrics(samples.cpu().numpy(), ns, hb.dt, model, axis, mid[:, c])
            _compare(got, ref, ns, f"sampled tracks, {model}, line on {axis}")
            got = _host(db.path_metrics(db.sm_mean, **kw))
            ref = pmc.path_metrics(sm_states, ns, hb.dt, model, axis, mid[:, c])
            _compare(got, ref, ns, f"smoothed tracks, {model}, line on {axis}")
        zero = db.sample_smoothed(2, draws=torch.zeros((2, tsc.NMAX + 1, 4, 16), dtype=torch.float64, device=db.device))
        d0 = _host(db.path_metrics(zero, model=model))["distance"]
        dsm = _host(db.path_metrics(db.sm_mean, model=model))["distance"]
        assert np.array_equal(_u64(d0[0]), _u64(dsm[0])) and np.array_equal(_u64(d0[1]), _u64(dsm[0])), model
        assert (dsm[0][ns == 0] == 0.0).all() and (dsm[0][ns > 0] > 0.0).all()


@pytest.mark.gpu
def test_front_ends():
    from track_estimators import batch

    hb, db = _sampled_batch()
    torch = db.torch
    sm = db.download(("means_smoothed", "covs_smoothed"))
    ns = hb.nsteps
    mid_lat = sm["means_smoothed"][np.arange(16), ns // 2, 1]
    # one chunk: the draws of sample_smoothed(8, seed)
    st = batch.path_statistics(db, 8, seed=4, chunk=8, line_axis="lat", line_value=mid_lat)
    direct = _host(db.path_metrics(db.sample_smoothed(8, seed=4), line_axis="lat", line_value=mid_lat))
    assert np.array_equal(_u64(st["distance"]), _u64(direct["distance"]))
    assert np.array_equal(_u64(st["cross_time"]), _u64(direct["cross_time"]))
    assert np.array_equal(_u64(st["distance_smoothed"]), _u64(_host(db.path_metrics(db.sm_mean))["distance"][0]))
    assert st["status"].shape == (16,) and not st["status"].any()
    # chunks of 3, 3, 2
    q = (0.1, 0.5, 0.9)
    for model in ("sphere", "wgs84"):
        st = batch.path_statistics(db, 8, seed=4, chunk=3, model=model, line_axis="lat", line_value=mid_lat, quantiles=q)
        assert st["distance"].shape == (8, 16) and st["cross_time"].shape == (8, 16) and st["distance_smoothed"].shape == (16,)
        assert st["distance_mean"].shape == st["distance_std"].shape == st["cross_prob"].shape == st["status"].shape == (16,)
        assert st["distance_quantiles"].shape == st["cross_time_quantiles"].shape == (3, 16)
        for k in ("distance", "distance_smoothed", "distance_mean", "distance_std", "distance_quantiles", "cross_prob"):
            assert np.isfinite(st[k]).all(), (model, k)
        assert (np.diff(st["distance_quantiles"], axis=0) >= 0.0).all()
        assert ((st["cross_prob"] >= 0.0) & (st["cross_prob"] <= 1.0)).all()
        assert np.array_equal(st["cross_prob"], (~np.isnan(st["cross_time"])).mean(axis=0))
        some = st["cross_prob"] > 0.0
        assert some.any() and not st["cross_prob"][ns == 0].any()
        assert np.isfinite(st["cross_time_quantiles"][:, some]).all() and np.isnan(st["cross_time_quantiles"][:, ~some]).all()
        assert (np.diff(st["cross_time_quantiles"][:, some], axis=0) >= 0.0).all()
        assert not np.array_equal(st["distance"][0], st["distance"][3])  # the second chunk drew afresh
    # a parallel farther north than 20 smoothed standard deviations beyond every smoothed row: no sample gets there
    live = np.arange(tsc.NMAX + 1)[None] <= ns[:, None]  # rows past nsteps are padding
    lat, sd = sm["means_smoothed"][..., 1], np.sqrt(np.where(live, sm["covs_smoothed"][..., 1, 1], 0.0))
    far = float(np.max((lat + 20.0 * sd)[live])) + 1e-3
    st = batch.path_statistics(db, 8, seed=4, chunk=3, line_axis="lat", line_value=far)
    assert (st["cross_prob"] == 0.0).all() and np.isnan(st["cross_time"]).all() and np.isnan(st["cross_time_quantiles"]).all()
    # a HostBatch is uploaded and run first: same values as the resident batch
    a = batch.path_statistics(hb, 4, seed=9, chunk=4)
    b = batch.path_statistics(db, 4, seed=9, chunk=4)
    assert np.array_equal(_u64(a["distance"]), _u64(b["distance"])) and "cross_time" not in a
    # the argument checks
    N1 = tsc.NMAX + 1
    f64 = dict(dtype=torch.float64, device=db.device)
    with pytest.raises(ValueError, match=rf"shape \(S, {N1}, 4, 16\) or \({N1}, 4, 16\)"):
        db.path_metrics(torch.zeros((2, N1, 4, 15), **f64))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.path_metrics(torch.zeros((N1, 16), **f64))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.path_metrics(torch.zeros((N1, 4, 16), dtype=torch.float32, device=db.device))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.path_metrics(torch.zeros((N1, 4, 16), dtype=torch.float64))
    with pytest.raises(ValueError, match="model must be"):
        db.path_metrics(db.sm_mean, model="flat")
    with pytest.raises(ValueError, match="line_axis must be"):
        db.path_metrics(db.sm_mean, line_axis="x", line_value=0.0)
    with pytest.raises(ValueError, match="go together"):
        db.path_metrics(db.sm_mean, line_axis="lat")
    with pytest.raises(ValueError, match=r"line_value must be a scalar or have shape \(16,\)"):
        db.path_metrics(db.sm_mean, line_axis="lat", line_value=np.zeros(3))


@pytest.mark.gpu
def test_dropin_distance_sailed():
    """UnscentedKalmanFilter.distance_sailed(): the smoothed track's distance is path_statistics' distance_smoothed for the
    track run() packed; with samples, the distances of sample_smoothed's tracks."""
    import types

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
        ukf.distance_sailed()
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    for model in ("sphere", "wgs84"):
        d = ukf.distance_sailed(model=model)
        st = batch.path_statistics(ukf._sample_hb, 5, seed=1, chunk=5, model=model)
        assert isinstance(d, float) and d > 0.0 and d == st["distance_smoothed"][0]
        ds = ukf.distance_sailed(5, random_state=1, model=model)
        assert ds.shape == (5,) and np.array_equal(_u64(ds), _u64(st["distance"][:, 0]))
    # ... and they are the distances of sample_smoothed's tracks, by the restatement
    samples = ukf.sample_smoothed(5, random_state=1)  # (5, N+1, 4)
    ref = pmc.path_metrics(samples[..., None], [tsc.NMAX])["distance"][:, 0]
    assert np.allclose(ukf.distance_sailed(5, random_state=1), ref, rtol=pmc.DIST_RTOL, atol=pmc.DIST_ATOL)
