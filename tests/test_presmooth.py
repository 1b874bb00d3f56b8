"""SOG / COG smoothed on the device before the rates and the measurements are formed (ste_track_prep_smooth_f64).

Yardsticks: arrays made by RUNNING the reference (tests/golden/cli_smooth.npz: its CLI's ``"smooth": 5`` on ship 01203823;
tests/golden/savgol_example.npz: its Savitzky-Golay example, windows 20 / 4, orders 4 / 2), with the tolerances of
tests/test_track_prep.py, and the NumPy restatement of the filter form (tests/presmooth_cases.py) applied to the device's own
raw series, with the standard bound of a dot product of w terms, |err| <= 2 w 2^-53 sum_k |c_k y_k|, which holds for any
summation order, with or without FMA.  The tables themselves are pinned to scipy / np.convolve without a GPU in
tests/test_presmooth_tables.py, where the STE_EINVAL cases of the ABI are as well (they need no device).

Circular mode: the device filters differences from the row's own value, y_i + sum c_k d_k.  Against the plain filter of the
unwrapped course, sum c_k u_k = u_i + sum c_k (u_k - u_i) + (sum c_k - 1) u_i, that differs by the rounding of the
differences and the products (inside the dot-product bound taken on the larger u_k), by (sum c_k - 1) u_i <= 4 ulp(1) |u_i|
(tests/test_presmooth_tables.py) and by the roundings of y_i + sum and of mod 360, a few ulp of 360: the issue's
2 w 2^-53 sum |c_k u_k| + 8 * 2^-52 * 360.  For the box filter that identity needs the whole window inside the track (at the
ends the reference's zero padding shortens the sum, and sum c_k < 1), so it is asserted on those rows; Savitzky-Golay edge
rows sum to 1 and every row is asserted.
"""
import ctypes as C
import os

import numpy as np
import pytest
from conftest import GOLDEN

import presmooth_cases as pc
from track_estimators import batch
from track_estimators._hip import binding
from track_estimators.ship_track import ShipTrack
from track_estimators.utils import generate_dts, haversine_formula, heading, smooth

pytestmark = pytest.mark.gpu
SPHERE = dict(calc_distance_func=haversine_formula, calc_heading_func=heading)
FILTERS = {"box4": lambda: batch.box_filter(4), "box5": lambda: batch.box_filter(5),
           "savgol63": lambda: batch.savgol_filter_table(6, 3), "savgol73": lambda: batch.savgol_filter_table(7, 3)}


def device_call(tracks, model="sphere", fs=None, fc=None, circular=False, smoothed=True):
    """The C ABI on padded arrays, outputs pre-filled with NaN so that every element the call must write shows: a dict of
    [T][B] arrays (z: [T][4][B]) and nobs."""
    import torch

    lib = binding.require_gpu()
    B, nobs = len(tracks), np.array([len(t[0]) for t in tracks], dtype=np.int32)
    T = int(nobs.max())
    lon, lat, gap = np.zeros((T, B)), np.zeros((T, B)), np.ones((max(T - 1, 1), B))
    for b, (lo, la, dts) in enumerate(tracks):
        lon[: nobs[b], b], lat[: nobs[b], b], gap[: nobs[b] - 1, b] = lo, la, dts
    dev = torch.device("cuda:0")
    up = [torch.from_numpy(a).to(dev) for a in (nobs, lon, lat, gap)]
    nan = dict(dtype=torch.float64, device=dev)
    outs, z, raw = torch.full((4, T, B), np.nan, **nan), torch.full((T, 4, B), np.nan, **nan), torch.full((2, T, B), np.nan, **nan)
    s = binding.StePrepBatchF64()
    s.B, s.Tmax, s.model = B, T, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model]
    s.nobs, s.lon, s.lat, s.gap = (t.data_ptr() for t in up)
    s.sog, s.cog, s.sog_rate, s.cog_rate = (outs[i].data_ptr() for i in range(4))
    s.z = z.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if smoothed:
        keep = []
        firs = [None if f is None else C.byref(batch._fir_struct(f, c, dev, keep)) for f, c in ((fs, False), (fc, circular))]
        binding.check(lib.ste_track_prep_smooth_f64(C.byref(s), firs[0], firs[1], raw[0].data_ptr(), raw[1].data_ptr(), stream),
                      "ste_track_prep_smooth_f64")
    else:
        binding.check(lib.ste_track_prep_f64(C.byref(s), stream), "ste_track_prep_f64")
    torch.cuda.synchronize()
    h, r = outs.cpu().numpy(), raw.cpu().numpy()
    return dict(sog=h[0], cog=h[1], sog_rate=h[2], cog_rate=h[3], z=z.cpu().numpy(), raw_sog=r[0], raw_cog=r[1], nobs=nobs)


def against_golden(res, g):
    np.testing.assert_allclose(res["raw_sog"], g["raw_sog"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["raw_cog"], g["raw_cog"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["sog"], g["sog"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["cog"], g["cog"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res["sog_rate"], g["sog_rate"], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(res["cog_rate"], g["cog_rate"], rtol=1e-8, atol=1e-9)
    assert res["z"].shape == g["z"].shape
    np.testing.assert_allclose(res["z"], g["z"], rtol=1e-10, atol=1e-10)
    assert res["status"] == 0


def test_box5_vs_reference_cli_smooth():
    g = np.load(os.path.join(GOLDEN, "cli_smooth.npz"))
    st = ShipTrack(**SPHERE)
    st.read_csv(os.path.join(GOLDEN, "ship_01203823.csv"), ship_id="01203823", id_col="primary.id", lat_col="lat", lon_col="lon")
    f = batch.box_filter(int(g["box"]))
    res = batch.prepare_observations([st.lon], [st.lat], [st.dts], model="sphere", smooth_sog=f, smooth_cog=f)
    against_golden(res[0], g)


def test_savgol_vs_reference_example():
    g = np.load(os.path.join(GOLDEN, "savgol_example.npz"))
    res = batch.prepare_observations([g["lon"]], [g["lat"]], [g["dts"]], model="sphere", smooth_sog=batch.savgol_filter_table(20, 4),
                                     smooth_cog=batch.savgol_filter_table(4, 2))
    against_golden(res[0], g)


def ragged_tracks(w, B=70, seed=3):
    rng = np.random.default_rng(seed)
    lengths = rng.choice([w, w + 1, w + 2, 2 * w + 3, 90], B)
    lengths[:5] = [w, w + 1, w + 2, 2 * w + 3, 90]  # every length at least once, and in the first wave
    if B >= 69:
        lengths[64:69] = [90, w, 2 * w + 3, w + 1, w + 2]  # and in the second, partly empty one
    out = []
    for T in lengths:
        lon = rng.uniform(-170, 170) + np.cumsum(rng.normal(0, 0.3, T))
        lat = rng.uniform(-60, 60) + np.cumsum(rng.normal(0, 0.2, T))
        out.append((lon, lat, rng.choice([0.5, 1.0, 6.0, 23.0, 24.0, 25.0], T - 1)))
    return out


@pytest.mark.parametrize("name", list(FILTERS))
def test_ragged_batch_vs_restatement(name):
    f = FILTERS[name]()
    w = f.window
    tracks = ragged_tracks(w)
    r = device_call(tracks, fs=f, fc=f)
    plain = device_call(tracks, smoothed=False)
    for key in ("sog", "cog", "sog_rate", "cog_rate", "raw_sog", "raw_cog", "z"):
        assert np.all(np.isfinite(r[key])), key  # every element written (the outputs started as NaN)
    np.testing.assert_array_equal(r["raw_sog"], plain["sog"])  # the raw series are the existing call's, bit for bit
    np.testing.assert_array_equal(r["raw_cog"], plain["cog"])
    np.testing.assert_array_equal(r["z"][:, 2], r["sog"])
    np.testing.assert_array_equal(r["z"][:, 3], r["cog"])
    np.testing.assert_array_equal(r["z"][:, :2], plain["z"][:, :2])
    worst = 0.0
    for b, (_, _, dts) in enumerate(tracks):
        n = r["nobs"][b]
        for key in ("sog", "cog", "sog_rate", "cog_rate", "raw_sog", "raw_cog"):
            assert np.array_equal(r[key][n:, b], np.zeros(r[key].shape[0] - n)), (key, b)
        assert not r["z"][n:, :, b].any()
        for key in ("sog", "cog"):
            raw = r["raw_" + key][:n, b]
            want, bound = pc.apply(f, raw), 2 * w * 2.0 ** -53 * pc.abs_sum(f, raw) + 1e-300
            err = np.abs(r[key][:n, b] - want)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (key, b, n, float(np.max(err / bound)))
            np.testing.assert_allclose(r[key + "_rate"][:n, b], pc.rates(want, dts), rtol=1e-8, atol=1e-9, err_msg=f"{key} {b}")
    print(f"{name}: worst error / bound = {worst:.3f}")


def test_filter_of_one_series_only_leaves_the_other_bit_equal():
    tracks = ragged_tracks(7, B=20, seed=8)
    args = ([t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks])
    plain = batch.prepare_observations(*args, model="sphere")
    f = batch.savgol_filter_table(7, 3)
    only_sog = batch.prepare_observations(*args, model="sphere", smooth_sog=f)
    only_cog = batch.prepare_observations(*args, model="sphere", smooth_cog=f)
    for p, s, c in zip(plain, only_sog, only_cog):
        assert "raw_sog" not in p and "raw_cog" not in p
        for r in (s, c):
            np.testing.assert_array_equal(r["raw_sog"], p["sog"])
            np.testing.assert_array_equal(r["raw_cog"], p["cog"])
        np.testing.assert_array_equal(s["cog"], p["cog"])
        np.testing.assert_array_equal(s["cog_rate"], p["cog_rate"])
        np.testing.assert_array_equal(s["z"][3], p["z"][3])
        np.testing.assert_array_equal(c["sog"], p["sog"])
        np.testing.assert_array_equal(c["sog_rate"], p["sog_rate"])
        np.testing.assert_array_equal(c["z"][2], p["z"][2])
        assert not np.array_equal(s["sog"], p["sog"]) and not np.array_equal(c["cog"], p["cog"])
        np.testing.assert_array_equal(s["z"][2], s["sog"])
        np.testing.assert_array_equal(c["z"][3], c["cog"])


def same_masks(a, b, what):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what)
    np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b), err_msg=what)
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b), err_msg=what)


def test_non_finite_values_reach_exactly_the_rows_that_read_them():
    # the zero-gap track of test_prep_duplicate_timestamps_and_coincident_points_device_vs_host_class, lengthened to 12 rows
    lon = np.array([10.0, 10.2, 10.2, 10.5, 10.6, 10.9, 11.0, 11.2, 11.3, 11.5, 11.6, 11.8])
    lat = np.array([50.0, 50.1, 50.1, 50.3, 50.3, 50.2, 50.2, 50.1, 50.0, 50.0, 49.9, 49.8])
    dts = np.array([1.0, 0.0, 2.0, 1.0, 0.0, 1.0, 1.0, 2.0, 1.0, 1.0, 0.5])  # rows 1 -> 2: no move, NaN; rows 4 -> 5: a move, inf
    box3, sg = batch.box_filter(3), batch.savgol_filter_table(5, 2)
    with np.errstate(all="ignore"):
        for f, ref in ((box3, lambda y: np.convolve(y, np.ones(3) / 3, "same")), (sg, lambda y: pc.apply(sg, y))):
            r = batch.prepare_observations([lon], [lat], [dts], model="sphere", smooth_sog=f, smooth_cog=f)[0]
            assert np.isnan(r["raw_sog"]).any() and np.isinf(r["raw_sog"]).any() and np.isfinite(r["raw_sog"]).sum() >= 8
            for key in ("sog", "cog"):
                want = ref(r["raw_" + key])
                same_masks(r[key], want, key)
                ok = np.isfinite(want)
                np.testing.assert_allclose(r[key][ok], want[ok], rtol=1e-10, atol=1e-10, err_msg=key)
                same_masks(r[key + "_rate"], pc.rates(want, dts), key + "_rate")
            assert np.isfinite(r["sog"]).any() and not np.isfinite(r["sog"]).all()
            np.testing.assert_array_equal(r["z"][2], r["sog"])


def turning_tracks():
    """Three tracks whose course turns steadily through north, 2 to 5 degrees per row over 40 rows."""
    out = []
    for start, turn, lon0, lat0 in ((300.0, 3.0, -20.0, 40.0), (60.0, -2.0, 100.0, -10.0), (250.0, 5.0, 5.0, 55.0)):
        course = np.radians(start + turn * np.arange(39))
        lat = lat0 + np.concatenate([[0.0], np.cumsum(0.05 * np.cos(course))])
        lon = lon0 + np.concatenate([[0.0], np.cumsum(0.05 * np.sin(course) / np.cos(np.radians(lat0)))])
        out.append((lon, lat, np.ones(39)))
    return out


def circ_err(a, b):
    return np.abs((a - b + 180.0) % 360.0 - 180.0)


@pytest.mark.parametrize("name", ["box5", "savgol73"])
def test_circular_course_filter(name):
    f = FILTERS[name]()
    w = f.window
    tracks = turning_tracks()
    circ = device_call(tracks, fc=f, circular=True)
    plain = device_call(tracks, fc=f)
    np.testing.assert_array_equal(circ["raw_cog"], plain["raw_cog"])
    np.testing.assert_array_equal(circ["sog"], plain["sog"])  # the option touches the course alone
    for b in range(len(tracks)):
        raw, got = circ["raw_cog"][:, b], circ["cog"][:, b]
        n = len(raw)
        assert raw.min() < 20.0 and raw.max() > 340.0  # the track does pass north
        assert np.all((got >= 0.0) & (got < 360.0))
        u = raw - 360.0 * np.concatenate([[0.0], np.cumsum(np.rint(np.diff(raw) / 360.0))])  # unwrapped, one rounding per row
        assert np.max(np.abs(np.diff(u))) < 10.0
        rows = slice(0, n) if f.nedge else slice(f.left, n - (w - 1 - f.left))  # module docstring
        want = np.mod(pc.apply(f, u), 360.0)
        bound = 2 * w * 2.0 ** -53 * pc.abs_sum(f, u) + 8 * 2.0 ** -52 * 360.0
        err = circ_err(got, want)
        assert np.all(err[rows] <= bound[rows]), (b, float(np.max(err[rows] / bound[rows])))
        # the restatement's circular variant, every row: the same sum of wrapped differences, so the dot-product bound on
        # them and the roundings of y_i + sum and of mod 360
        want_c = pc.apply_circular(f, raw)
        bound_c = 2 * w * 2.0 ** -53 * pc.abs_sum_circular(f, raw) + 8 * 2.0 ** -52 * 360.0
        assert np.all(circ_err(got, want_c) <= bound_c), (b, float(np.max(circ_err(got, want_c) / bound_c)))
        # and the option does something: averaged as plain numbers, a window across the seam lands far from the course
        assert np.max(circ_err(plain["cog"][w: n - w, b], got[w: n - w])) > 100.0
        np.testing.assert_array_equal(circ["cog_rate"][1:, b], np.diff(got))  # gaps of 1 h: built on the filtered course


def test_front_end_short_track_raises_and_ship_tracks_match():
    tracks = ragged_tracks(5, B=6, seed=4)
    args = ([t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks])
    with pytest.raises(ValueError, match="track 2"):
        batch.prepare_observations(args[0][:2] + [args[0][2][:4]], args[1][:2] + [args[1][2][:4]], args[2][:2] + [args[2][2][:3]],
                                   model="sphere", smooth_cog=batch.box_filter(5))
    fs, fc = batch.savgol_filter_table(5, 2), batch.box_filter(4)
    res = batch.prepare_observations(*args, model="sphere", smooth_sog=fs, smooth_cog=fc, cog_circular=True)
    sts = []
    for lon, lat, dts in tracks:
        st = ShipTrack(**SPHERE)
        st.lon, st.lat, st.dts = lon, lat, dts
        sts.append(st)
    assert batch.prepare_ship_tracks(sts, smooth_sog=fs, smooth_cog=fc, cog_circular=True) is sts
    for st, r in zip(sts, res):
        for key in ("sog", "cog", "sog_rate", "cog_rate", "z"):
            np.testing.assert_array_equal(getattr(st, key), r[key], err_msg=key)


def test_defaults_are_the_existing_call_bit_for_bit():
    tracks = ragged_tracks(5, B=9, seed=6)
    args = ([t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks])
    for model in ("sphere", "wgs84"):
        direct = device_call(tracks, model=model, smoothed=False)
        for res in (batch.prepare_observations(*args, model=model),
                    batch.prepare_observations(*args, model=model, smooth_sog=None, smooth_cog=None, cog_circular=False)):
            for b, r in enumerate(res):
                assert sorted(r) == ["cog", "cog_rate", "sog", "sog_rate", "status", "z"]
                n = len(tracks[b][0])
                for key in ("sog", "cog", "sog_rate", "cog_rate"):
                    np.testing.assert_array_equal(r[key], direct[key][:n, b], err_msg=key)
                np.testing.assert_array_equal(r["z"], direct["z"][:n, :, b].T)


def test_device_smoothed_preparation_feeds_filter_end_to_end():
    # the twelve steady ships of test_prep_wgs84_unpinned_feeds_filter_end_to_end, SOG / COG box-smoothed by 5: on the
    # device in one launch against utils.smooth per ship on the host, both through pack_tracks and run_batch
    H, Q, R = np.diag([1.0, 1, 0, 0]), np.diag([1e-4, 1e-4, 1e-6, 1e-6]), np.diag([0.25, 0.25, 0, 0])
    P0 = np.eye(4)
    rng = np.random.default_rng(5)
    host, dev = [], []
    for _ in range(12):
        T = int(rng.integers(20, 60))
        dts = rng.choice([1.0, 2.0, 6.0], T - 1)
        course = np.radians(rng.uniform(0, 360) + np.cumsum(rng.normal(0, 2.0, T - 1)))
        lat = rng.uniform(-50, 50) + np.concatenate([[0], np.cumsum(0.18 * dts * np.cos(course))])
        lon = rng.uniform(-150, 150) + np.concatenate([[0], np.cumsum(0.18 * dts * np.sin(course))])
        lon, lat = lon + rng.normal(0, 0.01, T), lat + rng.normal(0, 0.01, T)
        for sts in (host, dev):
            st = ShipTrack()
            st.lon, st.lat, st.dts = lon, lat, dts
            sts.append(st)
    for st in host:
        st.calculate_cog()
        st.calculate_sog()
        st.sog, st.cog = smooth(st.sog, 5), smooth(st.cog, 5)
        st.get_measurements(include_sog=True, include_cog=True)
        st.calculate_cog_rate()
        st.calculate_sog_rate()
    batch.prepare_ship_tracks(dev, smooth_sog=batch.box_filter(5), smooth_cog=batch.box_filter(5))
    outs = []
    for sts in (host, dev):
        hb = batch.pack_tracks(sts, [generate_dts(st.dts, 2) for st in sts], [st.z[:, 0] for st in sts], H, Q, R, P0)
        outs.append(batch.run_batch(hb))
    assert not outs[0]["status"].any() and not outs[1]["status"].any()
    for b in range(len(host)):
        n = outs[0]["nsteps"][b] + 1
        a, c = outs[0]["means_smoothed"][b, :n], outs[1]["means_smoothed"][b, :n]
        assert np.max(np.abs(a - c) / np.maximum(np.abs(a), 1e-12)) < 1e-6


def test_cli_device_prep_equals_host_preparation(tmp_path, monkeypatch):
    """``"device_prep": true`` with ``"smooth": 5`` on two ships in one batched run: the files the CLI writes agree with the
    run that prepares each ship on the host (utils.smooth), smoothed predictions to 1e-6 relative."""
    import gzip
    import json
    import shutil

    from track_estimators.cli.main_cli import track_estimator

    base = {"dim": 4, "H": [1, 1, 0, 0], "R": [0.001, 0.001, 0, 0], "Q": [1e-2, 1e-2, 1e-4, 1e-4], "P": [1.0, 1.0, 1.0, 1.0],
            "dt": -1, "nsteps": 2, "smooth": 5}
    with gzip.open(os.path.join(GOLDEN, "data", "historical_ship_data.csv.gz"), "rb") as src, open(tmp_path / "hist.csv", "wb") as dst:
        shutil.copyfileobj(src, dst)
    for name, extra in (("host", {}), ("device", {"device_prep": True})):
        os.makedirs(tmp_path / name)
        monkeypatch.chdir(tmp_path / name)
        with open("input.json", "w") as f:
            json.dump(dict(base, **extra), f)
        track_estimator(["-t", "../hist.csv", "-s", "01203823,01205638", "-ic", "primary.id", "-lat", "lat", "-lon", "lon", "-rts",
                         "--no-noise"])
    for sid in ("01203823", "01205638"):
        for kind in ("predictions", "predictions_smoothed", "variances_smoothed"):
            a = np.loadtxt(tmp_path / "host" / f"output_{sid}_{kind}.txt")
            c = np.loadtxt(tmp_path / "device" / f"output_{sid}_{kind}.txt")
            assert a.shape == c.shape and np.all(np.isfinite(a))
            assert np.max(np.abs(a - c) / np.maximum(np.abs(a), 1e-12)) < 1e-6, (sid, kind)
