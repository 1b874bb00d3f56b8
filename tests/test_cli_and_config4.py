"""CLI surface (reference cli/main_cli.py), the robustification helpers, and BASELINE configs[3] (modern ships)."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest
from conftest import GOLDEN


def test_input_settings_parsing():
    from track_estimators.cli.main_cli import _get_input_matrix, get_input_settings

    s = {"dim": 4, "H": [1, 1, 0, 0], "R": [0.001, 0.001, 0, 0], "Q": [1e-2, 1e-2, 1e-4, 1e-4], "P": [1.0, 1, 1, 1],
         "dt": -1, "nsteps": 2}
    dim, dt, nsteps, H, Q, R, P, smooth = get_input_settings(s)
    assert (dim, dt, nsteps, smooth) == (4, -1, 2, None)
    assert np.array_equal(H, np.diag([1, 1, 0, 0])) and np.array_equal(Q, np.diag([1e-2, 1e-2, 1e-4, 1e-4]))
    assert get_input_settings({**s, "smooth": 5})[-1] == 5
    full = np.arange(16.0).reshape(4, 4).tolist()
    assert np.array_equal(_get_input_matrix({"H": full}, "H", 4), np.arange(16.0).reshape(4, 4))
    for missing in ("dim", "dt", "nsteps", "H", "Q", "R", "P"):
        with pytest.raises(KeyError):
            get_input_settings({k: v for k, v in s.items() if k != missing})
    with pytest.raises(AssertionError):
        _get_input_matrix({"H": [1, 1, 0]}, "H", 4)


def test_parser_flags_match_reference_surface():
    from track_estimators.cli.argument_parser import create_parser

    a = create_parser().parse_args(["-t", "f.csv", "-s", "01203823", "-ic", "primary.id", "-lat", "lat", "-lon", "lon",
                                    "-rts", "-rev", "-o", "out", "-i", "in.json"])
    assert (a.track_file, a.ship_id, a.id_col, a.lat_id, a.lon_id) == ("f.csv", "01203823", "primary.id", "lat", "lon")
    assert a.apply_rts_smoother and a.reverse and a.output_prefix == "out" and a.input_file == "in.json"
    d = create_parser().parse_args(["-t", "f", "-s", "1", "-ic", "i", "-lat", "a", "-lon", "o"])
    assert d.input_file == "input.json" and d.output_prefix == "output" and not d.apply_rts_smoother and not d.reverse


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path, monkeypatch):
    """The reference's CLI example (examples/cli_example/run.sh + input.json) through this package's entry point.
    Row 0 of the predictions and the dts file are noise-free known answers of the reference's committed outputs."""
    from track_estimators.cli.main_cli import track_estimator

    monkeypatch.chdir(tmp_path)
    with open("input.json", "w") as f:
        json.dump({"dim": 4, "H": [1, 1, 0, 0], "R": [0.001, 0.001, 0, 0], "Q": [1e-2, 1e-2, 1e-4, 1e-4],
                   "P": [1.0, 1.0, 1.0, 1.0], "dt": -1, "nsteps": 2}, f)
    csv = os.path.join(GOLDEN, "ship_01203823.csv")
    track_estimator(["-i", "input.json", "-o", "output", "-t", csv, "-s", "01203823", "-ic", "primary.id", "-lat", "lat",
                     "-lon", "lon", "-rts", "--no-noise"])
    pred = np.loadtxt("output_01203823_predictions.txt")
    var = np.loadtxt("output_01203823_variances.txt")
    dts = np.loadtxt("output_01203823_dts.txt")
    orig = np.loadtxt("original_01203823_track.txt")
    sm = np.loadtxt("output_01203823_predictions_smoothed.txt")
    vsm = np.loadtxt("output_01203823_variances_smoothed.txt")
    assert pred.shape == (103, 4) and var.shape == (103, 4) and sm.shape == (103, 4) and vsm.shape == (103, 4)
    assert dts.shape == (102,) and orig.shape == (52, 2)
    np.testing.assert_allclose(pred[0], [-30.5, -0.5, 14.578418614021368, 198.52495095065817], rtol=1e-11)
    assert set(np.unique(dts)) <= {11.5, 12.0, 12.5}
    assert np.array_equal(var[0], [1.0, 1.0, 1.0, 1.0]) and np.all(np.isfinite(sm))
    # same answer as the class API on the same inputs
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter
    from track_estimators.ship_track import ShipTrack
    from track_estimators.utils import generate_dts

    st = ShipTrack()
    st.read_csv(csv, ship_id="01203823", id_col="primary.id")
    z = st.get_measurements(include_sog=True, include_cog=True)
    st.calculate_cog_rate()
    st.calculate_sog_rate()
    ukf = UnscentedKalmanFilter(H=np.diag([1, 1, 0, 0]), Q=np.diag([1e-2, 1e-2, 1e-4, 1e-4]), R=np.diag([0.001, 0.001, 0, 0]),
                                P=np.eye(4), x0=z[:, 0].reshape(-1, 1).copy(), non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    dt = generate_dts(st.dts, 2)
    m, _ = ukf.run(len(dt), dt, st)
    np.testing.assert_allclose(pred, m, rtol=1e-12, atol=1e-12)
    # batch mode: two ids in one launch write the same files per id
    os.makedirs("b", exist_ok=True)
    monkeypatch.chdir(tmp_path / "b")
    shutil.copy(tmp_path / "input.json", "input.json")
    hist = os.path.join(GOLDEN, "data", "historical_ship_data.csv.gz")
    with gzip.open(hist, "rb") as src, open("hist.csv", "wb") as dst:
        shutil.copyfileobj(src, dst)
    track_estimator(["-t", "hist.csv", "-s", "01203823,01205638", "-ic", "primary.id", "-lat", "lat", "-lon", "lon", "-rts",
                     "--no-noise"])
    pb = np.loadtxt("output_01203823_predictions.txt")
    np.testing.assert_allclose(pb, pred, rtol=1e-12, atol=1e-12)
    assert os.path.exists("output_01205638_predictions_smoothed.txt")


@pytest.mark.gpu
def test_cli_with_presmoothing(tmp_path, monkeypatch, caplog):
    """input.json key `smooth` (reference cli/main_cli.py:99-104, :209-212): SOG / COG are moving-averaged before the
    measurements and rates are formed.  The host arithmetic of that step is pinned to the reference in
    tests/test_host_logic.py::test_cli_presmoothing_vs_reference; here the CLI plumbing: the log line, a different prior
    speed / course in row 0 than without smoothing, and equality with the class API fed the same smoothed track."""
    from track_estimators.cli.main_cli import track_estimator
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter
    from track_estimators.ship_track import ShipTrack
    from track_estimators.utils import generate_dts, smooth

    import logging

    caplog.set_level(logging.INFO)
    monkeypatch.chdir(tmp_path)
    base = {"dim": 4, "H": [1, 1, 0, 0], "R": [0.001, 0.001, 0, 0], "Q": [1e-2, 1e-2, 1e-4, 1e-4], "P": [1.0, 1.0, 1.0, 1.0],
            "dt": -1, "nsteps": 2}
    csv = os.path.join(GOLDEN, "ship_01203823.csv")
    with open("input.json", "w") as f:
        json.dump(dict(base, smooth=5), f)
    track_estimator(["-i", "input.json", "-o", "sm5", "-t", csv, "-s", "01203823", "-ic", "primary.id", "-lat", "lat", "-lon", "lon",
                     "-rts", "--no-noise"])
    assert "Smoothing SOG and COG by 5." in caplog.text
    pred = np.loadtxt("sm5_01203823_predictions.txt")
    smo = np.loadtxt("sm5_01203823_predictions_smoothed.txt")
    assert pred.shape == (103, 4) and smo.shape == (103, 4) and np.all(np.isfinite(smo))
    assert abs(pred[0, 2] - 14.578418614021368) > 1e-3  # the prior's speed is the smoothed one
    st = ShipTrack()
    st.read_csv(csv, ship_id="01203823", id_col="primary.id")
    st.calculate_cog()
    st.calculate_sog()
    st.sog, st.cog = smooth(st.sog, 5), smooth(st.cog, 5)
    z = st.get_measurements(include_sog=True, include_cog=True)
    st.calculate_cog_rate()
    st.calculate_sog_rate()
    H, R, Q, P = (np.diag(base[k]).astype(float) for k in ("H", "R", "Q", "P"))
    ukf = UnscentedKalmanFilter(H=H, Q=Q, R=R, P=P, x0=z[:, 0].reshape(-1, 1).copy(), non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    dt = generate_dts(st.dts, 2)
    m, _ = ukf.run(len(dt), dt, st)
    np.testing.assert_allclose(pred, m, rtol=1e-12, atol=1e-12)
    caplog.clear()
    with open("input.json", "w") as f:
        json.dump(dict(base, smooth=1), f)  # -1, 0, 1 and a missing key all mean "no smoothing"
    track_estimator(["-i", "input.json", "-o", "sm1", "-t", csv, "-s", "01203823", "-ic", "primary.id", "-lat", "lat", "-lon", "lon",
                     "--no-noise"])
    assert "Smoothing" not in caplog.text
    np.testing.assert_allclose(np.loadtxt("sm1_01203823_predictions.txt")[0], [-30.5, -0.5, 14.578418614021368, 198.52495095065817],
                               rtol=1e-11)


@pytest.mark.gpu
def test_robust_helpers_and_flag():
    """criterion_index / update_lambda_factor methods vs the reference's known answers; the opt-in robust update of the
    batched path vs the oracle's restatement of check_robustness (noise-free)."""
    from oracle import ukf_oracle as orc
    from track_estimators import batch, synthetic
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter

    k = np.load(os.path.join(GOLDEN, "kats.npz"))
    for i in range(8):
        u = UnscentedKalmanFilter(H=k["H"], Q=k["Q"], R=k["R"], P=k["rb_P"][i], x0=k["rb_x"][i])
        c = u.criterion_index(k["rb_z"][i].reshape(-1, 1), k["rb_P"][i], k["R"])
        assert np.isclose(c, k["rb_ci"][i], rtol=1e-10)
        lam = u.update_lambda_factor(1.0, c, 50.0, k["rb_z"][i].reshape(-1, 1), k["rb_P"][i], k["R"])
        assert np.isclose(lam, k["rb_lambda"][i], rtol=1e-10)
        assert np.array_equal(u.scale_measurement_uncertainty(k["R"], 3.0), k["R"] * 3.0)
    # robust flag: a track with one gross outlier; emulate with the oracle step by step
    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(3, nobs=9, gap_h=1.0, seed0=31)
    sb.z[1, 0, 4] += 25.0  # 25 degrees of longitude off
    hb = batch.pack_uniform(sb, 1, H, Q, R, P0)
    hb.robust = True
    out = batch.run_batch(hb, smooth=False)
    plain = batch.run_batch(batch.pack_uniform(sb, 1, H, Q, R, P0), smooth=False)
    # oracle emulation for track 1
    W = orc.weight_matrix(4)
    x, P = sb.z[1][:, 0].reshape(-1, 1).copy(), P0.copy()

    def upd(x, P, z):
        Rr = orc.check_robustness(x, H, z, P, R)
        return orc.update_track(x, P, H, Rr, z)

    x, P = upd(x, P, sb.z[1][:, 0])
    for kk in range(8):
        x, P = orc.predict_track(x, P, Q, W, sb.dts[1][kk], sb.sog_rate[1][kk], sb.cog_rate[1][kk])
        x, P = upd(x, P, sb.z[1][:, kk + 1])
        np.testing.assert_allclose(out["means"][1, kk + 1], x[:, 0], rtol=1e-7, atol=1e-9)
    assert abs(out["means"][1, 4, 0] - plain["means"][1, 4, 0]) > 1.0  # the outlier was down-weighted
    np.testing.assert_allclose(out["means"][0], plain["means"][0], rtol=1e-9)  # clean tracks are untouched


def _modern_batch(robust):
    from track_estimators import batch
    from track_estimators.ship_track import ShipTrack
    from track_estimators.utils import generate_dts, haversine_formula, heading

    g = np.load(os.path.join(GOLDEN, "modern_ships.npz"))
    csv = os.path.join(GOLDEN, "data", "modern_ship_data.csv.gz")
    H = np.diag([1.0, 1, 0, 0]); R = np.diag([0.25, 0.25, 0, 0]); Q = np.diag([1e-4, 1e-4, 1e-6, 1e-6]); P = np.eye(4)
    tracks, dts, x0s = [], [], []
    ids = [str(s) for s in g["ids"]]
    with np.errstate(all="ignore"):
        for sid in ids:
            st = ShipTrack(calc_distance_func=haversine_formula, calc_heading_func=heading)
            st.read_csv(csv, ship_id=sid, id_col="id", lat_col="lat", lon_col="lon")
            z = st.get_measurements(include_sog=True, include_cog=True)
            st.calculate_cog_rate()
            st.calculate_sog_rate()
            assert len(st.lon) == int(g[f"{sid}_T"]) and int((st.dts == 0).sum()) == int(g[f"{sid}_zero_dt"])
            np.testing.assert_allclose([np.nansum(np.where(np.isfinite(z), z, 0.0)), st.dts.sum()], g[f"{sid}_zsum"],
                                       rtol=1e-12)
            tracks.append(st)
            dts.append(generate_dts(st.dts, 2))
            x0s.append(z[:, 0])
    hb = batch.pack_tracks(tracks, dts, x0s, H, Q, R, P)
    hb.robust = robust
    return g, ids, batch.run_batch(hb)


def _check_against(out, b, sid, g, max_row):
    rows = g[f"{sid}_rows"]
    keep = rows <= min(max_row, rows.max())
    assert keep.sum() >= 140
    for key in ("means", "means_smoothed"):
        ref = g[f"{sid}_{key}"][keep]
        err = np.max(np.abs(out[key][b, rows[keep]] - ref) / np.maximum(np.abs(ref), 1e-3))
        assert err < 1e-6, (sid, key, err)
    for key in ("covs", "covs_smoothed"):
        ref = g[f"{sid}_{key}"][keep]
        err = np.max(np.abs(out[key][b, rows[keep]] - ref) / np.max(np.abs(ref), axis=(-1, -2), keepdims=True))
        assert err < 1e-5, (sid, key, err)


@pytest.mark.gpu
def test_config4_modern_ships_batch():
    """All seven ids of data/modern_ships in one ragged batch (13 274 .. 19 236 steps).  Two ships run clean and must
    match the reference; five contain duplicate timestamps (dt = 0): the reference dies with LinAlgError inside pinv,
    the batch flags them with STE_STATUS_NAN and carries on (like the batch example's try/except/continue)."""
    g, ids, out = _modern_batch(robust=False)
    # AMOUK05 sits in port for months; from about step 7 200 the filter itself runs away on that data (latitude passes
    # 92 degrees, speeds of -190..160 km/h) and the trajectory becomes chaotic: two CPU restatements of the reference
    # that differ only in the square-root algorithm end up 220 degrees of longitude apart.  Parity is therefore checked on
    # the stable prefix of that ship and on the whole of WCE5063 (17 084 steps).  A stationary ship has speeds of ~1e-13
    # (pure rounding), so the relative measure gets an absolute floor of 1e-3 here.
    stable_rows = {"AMOUK05": 7000}
    for b, sid in enumerate(ids):
        if int(g[f"{sid}_ok"]):
            assert not (out["status"][b] & 0x1)
            _check_against(out, b, sid, g, stable_rows.get(sid, 1 << 30))
        else:
            assert out["status"][b] & 0x11, sid  # non-finite state and/or update index past the last observation


@pytest.mark.gpu
def test_config4_modern_ships_robust_on():
    """BASELINE configs[3] as written -- Mahalanobis outlier rejection ON: the same ragged batch with STE_FLAG_ROBUST,
    against the reference run with its check_robustness call site enabled (tests/golden/modern_ships_robust.npz; the two
    ships the reference can filter at all; 1 861 and 38 419 updates get their R rescaled).  The five ships with
    duplicate timestamps are flagged as before."""
    g, ids, out = _modern_batch(robust=True)
    gr = np.load(os.path.join(GOLDEN, "modern_ships_robust.npz"))
    assert int(gr["WCE5063_rescalings"]) > 1000
    stable_rows = {"AMOUK05": 7000}
    for b, sid in enumerate(ids):
        if sid in [str(s) for s in gr["ids"]]:
            assert not (out["status"][b] & 0x1)
            _check_against(out, b, sid, gr, stable_rows.get(sid, 1 << 30))
            plain = g[f"{sid}_means"]
            assert np.abs(gr[f"{sid}_means"] - plain).max() > 1e-3  # the robust reference run differs from the plain one
        else:
            assert out["status"][b] & 0x11, sid


@pytest.mark.gpu
def test_config4_modern_ships_deduplicated_robust_on():
    """The five ids of data/modern_ships whose hour-resolution timestamps repeat (zero gaps: the reference dies with
    LinAlgError, this package flags them) with ``ShipTrack.read_csv(drop_duplicate_times=True)`` -- an opt-in extra of this
    package -- and outlier rejection on, against the REFERENCE run on files from which those rows were deleted
    (tests/golden/modern_ships_dedup.npz, made by make_golden.modern_dedup_cases).  configs[3]'s full-length parity no
    longer rests on WCE5063 alone."""
    from track_estimators import batch
    from track_estimators.ship_track import ShipTrack
    from track_estimators.utils import generate_dts, haversine_formula, heading

    g = np.load(os.path.join(GOLDEN, "modern_ships_dedup.npz"))
    csv = os.path.join(GOLDEN, "data", "modern_ship_data.csv.gz")
    H = np.diag([1.0, 1, 0, 0]); R = np.diag([0.25, 0.25, 0, 0]); Q = np.diag([1e-4, 1e-4, 1e-6, 1e-6]); P = np.eye(4)
    ids = [str(s) for s in g["ids"]]
    tracks, dts, x0s = [], [], []
    for sid in ids:
        st = ShipTrack(calc_distance_func=haversine_formula, calc_heading_func=heading)
        st.read_csv(csv, ship_id=sid, id_col="id", lat_col="lat", lon_col="lon", drop_duplicate_times=True)
        assert len(st.lon) == int(g[f"{sid}_T"]) and not (st.dts == 0).any() and int(g[f"{sid}_dropped"]) > 0
        z = st.get_measurements(include_sog=True, include_cog=True)
        st.calculate_cog_rate()
        st.calculate_sog_rate()
        tracks.append(st)
        dts.append(generate_dts(st.dts, 2))
        x0s.append(z[:, 0])
    hb = batch.pack_tracks(tracks, dts, x0s, H, Q, R, P)
    hb.robust = True
    out = batch.run_fleet(hb)
    # The fixture says, row by row, how far ONE change inside the reference's own arithmetic (eigen instead of Schur square
    # root: the same matrix function to 1e-15) moves each history of that ship.  Where that is < 1e-8 -- every sampled row
    # of three ships, 94 % and 58 % of the other two -- the north-star tolerances are asserted; the remaining rows sit in
    # episodes where rounding decides (a ship at rest, the rejection threshold crossed or not) and move by 1e-5 .. 1e-4 for
    # ANY implementation that does not reproduce LAPACK's rounding: held to 1e-3 there.
    strict_rows = 0
    for b, sid in enumerate(ids):
        assert int(g[f"{sid}_ok"]) and not (out["status"][b] & 0x1), sid
        rows = g[f"{sid}_rows"]
        for key, tol in (("means", 1e-6), ("means_smoothed", 1e-6), ("covs", 1e-5), ("covs_smoothed", 1e-5)):
            ref, got = g[f"{sid}_{key}"], out[key][b, rows]
            if key.startswith("means"):
                d = np.abs(got - ref)
                d[:, 3] = np.abs((got[:, 3] - ref[:, 3] + 180.0) % 360.0 - 180.0)  # 359.9999 against 0.0001 is 2e-4 degrees
                err = np.max(d / np.maximum(np.abs(ref), 1e-3), axis=1)
            else:
                err = np.max(np.abs(got - ref), axis=(-1, -2)) / np.max(np.abs(ref), axis=(-1, -2))
            stable = g[f"{sid}_sens_{key}"] <= 1e-8
            assert stable.mean() > 0.5, (sid, key)
            assert err[stable].max() < tol, (sid, key, float(err[stable].max()))
            assert err.max() < 1e-3, (sid, key, float(err.max()))
            strict_rows += int(stable.sum()) if key == "means_smoothed" else 0
    assert strict_rows > 1300  # of 1 545 sampled rows over the five ships

    # EVERY row of the five ships: tests/golden/modern_ships_dedup_full.npz holds the whole histories of the
    # same reference runs -- means in fp64, covariances as fp32 upper triangles (6e-8 of an entry: the 1e-5 bound gets 1e-7 of
    # slack for it) -- and the row-by-row sensitivity.  Rows the reference's own arithmetic holds to 1e-8 under a change of
    # its square-root algorithm meet the north-star tolerances; the rest (counted below) are held to 1e-3.
    gf = np.load(os.path.join(GOLDEN, "modern_ships_dedup_full.npz"))
    iu = np.triu_indices(4)
    total = strict = 0
    loose = {}
    for b, sid in enumerate(ids):
        n1 = int(out["nsteps"][b]) + 1
        assert gf[f"{sid}_means"].shape[0] == n1, sid
        for key, tol in (("means", 1e-6), ("means_smoothed", 1e-6), ("covs", 1e-5 + 1e-7), ("covs_smoothed", 1e-5 + 1e-7)):
            got = out[key][b, :n1]
            if key.startswith("means"):
                ref = gf[f"{sid}_{key}"]
                d = np.abs(got - ref)
                d[:, 3] = np.abs((got[:, 3] - ref[:, 3] + 180.0) % 360.0 - 180.0)
                err = np.max(d / np.maximum(np.abs(ref), 1e-3), axis=1)
            else:
                ref = gf[f"{sid}_{key}_tri_f32"].astype(np.float64)
                err = np.max(np.abs(got[:, iu[0], iu[1]] - ref), axis=1) / np.max(np.abs(ref), axis=1)
            stable = gf[f"{sid}_sens_{key}"] <= 1e-8
            assert err[stable].max() < tol, (sid, key, float(err[stable].max()), int(np.argmax(np.where(stable, err, 0))))
            assert err.max() < 1e-3, (sid, key, float(err.max()))
            total += n1
            strict += int(stable.sum())
            loose[(sid, key)] = int((~stable).sum())
    # 71 743 rows x 4 histories; the sensitive ones sit in two ships (WDA7827: at rest for weeks; KAOU)
    assert total == 4 * sum(int(out["nsteps"][b]) + 1 for b in range(len(ids))) and strict > 0.93 * total, (strict, total, loose)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_two_rank_control_flow():
    """bench.py launched as two ranks by torch.distributed.run (as the driver does for N>1), both on this box's one GPU
    with the gloo backend standing in for RCCL: checks rank handling, track sharding, the overlapped all-gather of the
    smoothed positions, the max-over-ranks timing and the single JSON line."""
    import subprocess
    import sys

    from conftest import ROOT

    env = dict(os.environ, STE_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--tracks", "256", "--cpu-tracks", "0", "--full"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["unit"] == "track-steps/s"
    assert out["config"]["tracks_per_gpu"] == 256 and "all-gather" in out["config"]["parallelism"]
    assert out["value"] > 0 and out["status_flagged_tracks"] == 0
    ag = out["all_gather_alone"]  # the step's exchange timed on its own
    assert ag["ms"] > 0 and ag["bytes_sent_per_rank"] == 501 * 2 * 256 * 8 and ag["bytes_received_per_rank"] == ag["bytes_sent_per_rank"]
    assert "rccl" in ag and ag["rccl"] is None  # RCCL's algorithm / protocol lines: only the nccl backend logs them
    fo = out["filter_only"]  # the timed loop without the exchange, slowest rank and every rank
    assert len(fo["per_rank_ms_per_step"]) == 2 and abs(max(fo["per_rank_ms_per_step"]) - fo["ms_per_step"]) < 1e-9
    assert out["config"]["gather_every"] == 1
    # one exchange per fleet of K batches instead of one per batch
    cmd2 = cmd[:cmd.index("29533")] + ["29534"] + cmd[cmd.index("29533") + 1:] + ["--gather-every", "2"]
    res = subprocess.run(cmd2, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    out2 = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][0])
    assert out2["config"]["gather_every"] == 2 and "once per 2 steps" in out2["config"]["parallelism"] and out2["value"] > 0
    # the exchange behind SCHEDULED forward launches (bench.py --sequence N; not the default with more than one rank): the
    # all-gather hook of every step goes behind that step's smoother on its gated smoother stream
    cmd3 = cmd[:cmd.index("29533")] + ["29535"] + cmd[cmd.index("29533") + 1:] + ["--sequence", "2"]
    res = subprocess.run(cmd3, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    out3 = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][0])
    assert out3["config"]["steps_per_scheduled_forward_launch"] == [2] and out3["status_flagged_tracks"] == 0 and out3["value"] > 0
    assert out["config"]["steps_per_scheduled_forward_launch"] == 0  # auto: per-step launches when ranks exchange


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_one_rank_over_rccl():
    """The N > 1 code path of bench.py with the REAL backend (nccl = RCCL), one rank, as a fresh child process
    (`--force-dist`): process group on the device, 32 compute units reserved for the collective's kernels, the all-gather
    of the smoother's own sm_pos output overlapped with the following steps, `all_gather_alone` and `filter_only` in the
    line.  (More than one RCCL rank cannot share this box's one GPU: the two-rank tests use gloo.)"""
    import subprocess
    import sys

    from conftest import ROOT

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "STE_BENCH_BACKEND")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29537", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--force-dist", "--tracks", "640", "--steps", "3", "--warmup", "1",
           "--cpu-tracks", "0", "--full"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and "RCCL all-gather" in out["config"]["parallelism"] and out["value"] > 0
    assert "32 left to the collective's kernels" in out["config"]["pipeline"]
    ag, fo = out["all_gather_alone"], out["filter_only"]
    assert ag["ms"] > 0 and ag["bytes_sent_per_rank"] == 501 * 2 * 640 * 8
    assert fo["value"] > 0 and fo["ms_per_step"] > 0 and out["status_flagged_tracks"] == 0
    assert len(fo["per_rank_ms_per_step"]) == 1
    # RCCL's own log of the exchange, read back after the untimed leg (one rank: the calls are logged, an algorithm may not be)
    assert isinstance(ag["rccl"], dict) and "error" not in ag["rccl"], ag["rccl"]
    assert ag["rccl"]["allgather_calls_logged"] >= 1 or ag["rccl"]["tuning_lines"], ag["rccl"]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_line_carries_the_contract():
    """One small N = 1 run of bench.py: exactly one JSON line with every field the driver's contract names -- the metric
    of BASELINE.json, whole-job value, the roofline object of the dominant kernel with its traffic, the CPU baseline of the
    same run with core count and kind -- and the parity block of the cross-check inside tolerance."""
    import subprocess
    import sys

    from conftest import ROOT

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "2", "--tracks", "640",
           "--cpu-tracks", "64", "--cpu-ref-tracks", "2", "--cpu-pool-tracks", "0", "--no-gp", "--fleet-tracks", "1500",
           "--fleet-chunk", "500", "--full"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"].startswith("UKF+URTSS track-steps/sec") and out["unit"] == "track-steps/s"
    assert (out["n_gpus"], out["steps"], out["warmup"]) == (1, 30, 2) and out["higher_is_better"] is True
    assert out["scaling"] == "weak" and out["vs_baseline"] is None and out["dtype"] == "f64" and out["data"] == "synthetic"
    assert "workload" in out["config"] and "model" not in out["config"]
    assert abs(out["value"] - 640 * 500 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    r = out["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["traffic"] > 0
    # achieved = 512 algorithmic bytes per track-step x the track-steps/s of the timed region
    assert abs(r["achieved"] - 512 * out["value"] / 1e9) < 1e-6 * r["achieved"] and r["algorithmic_bytes_per_track_step"] == 512
    pl = r["per_launch"]  # one launch of the dominant kernel over its own HIP-event duration
    assert pl["kernel"] == "ukf_forward" and pl["launch_ms"] > 0 and pl["launches_in_flight"] >= 1
    # bench.py --sequence auto: the clock chooses, untimed, between one launch per step and scheduled launches (30 steps of 10
    # tiles do not fill the chip: ONE scheduled launch), and the line says which it took and what either cost
    auto = out["config"]["sequence_auto"]
    assert auto["steps"] == 30 and auto["per_step_launches_ms"] > 0 and auto["scheduled_launches_ms"] > 0
    # three untimed runs of either form, the slowest decides; the scheduled form ran on a pipeline of its own (2 forward streams)
    assert len(auto["per_step_launches_ms_all"]) == 3 and max(auto["per_step_launches_ms_all"]) == auto["per_step_launches_ms"]
    assert len(auto["scheduled_launches_ms_all"]) == 3 and max(auto["scheduled_launches_ms_all"]) == auto["scheduled_launches_ms"]
    if auto["chosen"] == "scheduled":
        assert auto["scheduled_launches_ms"] <= auto["per_step_launches_ms"]
        assert pl["steps_per_launch"] == 30 and out["config"]["steps_per_scheduled_forward_launch"] == [30]
        assert [d["steps"] for d in out["kernels_ms"]["scheduled_launches"]] == [30] and auto["streams"].startswith("2 forward")
    else:
        assert auto["chosen"] == "per_step" and auto["scheduled_launches_ms"] > auto["per_step_launches_ms"]
        assert pl["steps_per_launch"] == 1 and out["config"]["steps_per_scheduled_forward_launch"] == 0
    assert abs(pl["achieved"] - 192 * 640 * 500 * pl["steps_per_launch"] / (pl["launch_ms"] * 1e-3) / 1e9) < 1e-6 * pl["achieved"]
    fl = out["extra"]["fleet_100k"]  # the product entry point for a fleet, on a small one here
    assert fl["bit_identical_to_one_launch"] is True and fl["track_steps"] == 1500 * 500 and fl["value"] > 0
    assert fl["gpu_vs_oracle"]["means_smoothed_max_rel_err"] < 1e-6 and fl["flagged_tracks"] == 0
    c = out["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c and c["unit"] == "track-steps/s"
    par = c["gpu_vs_oracle"]
    assert par["tracks"] == 64
    for name in ("means", "means_smoothed"):
        assert par[name]["max_rel_err"] < 1e-6, name
    for name in ("covs", "covs_smoothed"):
        assert par[name]["max_rel_err_per_matrix"] < 1e-5, name
    # the reference's own call sequence (the oracle's bit-exact per-track form) timed beside the vectorised port
    rc = c["reference_call_sequence"]
    assert rc["cores"] == 1 and rc["unit"] == "track-steps/s" and 0 < rc["value"] < c["value"] and "sample" in rc
    assert rc["gpu_vs_this"]["tracks"] == 2 and rc["gpu_vs_this"]["means_smoothed_max_rel_err"] < 1e-6
    assert rc["gpu_vs_this"]["covs_smoothed_max_rel_err_per_matrix"] < 1e-5
    assert out["steady_state"] is None or out["steady_state"]["ms_per_step"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_gpus_flag_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no external launcher (the form the driver's N = 1 command has): bench.py must start
    the two ranks itself -- as a child job, before it touches the GPU -- relay rank 0's one JSON line and exit 0."""
    import subprocess
    import sys

    from conftest import ROOT

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["STE_BENCH_BACKEND"] = "gloo"  # two ranks share this box's one GPU
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--tracks", "256",
           "--cpu-tracks", "0"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["total_tracks"] == 512 and out["value"] > 0


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain N = 1 run (no --full): the headline line without the figures that take runs of their own, and
    --dump-outputs writes the histories of the last timed step for the fixed track sample -- checked against the oracle."""
    import subprocess
    import sys

    import bench
    from conftest import ROOT
    from track_estimators import batch, synthetic

    from oracle import ukf_oracle as orc

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--tracks", "640",
           "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert (out["steps"], out["warmup"], out["dtype"], out["higher_is_better"]) == (3, 1, "f64", True)
    assert abs(out["value"] - 640 * 500 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert out["serial"] is None and not {"cpu_baseline", "pcie_inclusive", "extra"} & set(out)
    idx = bench.dump_sample(640)
    files = {f[:-len(".npy")]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(files) == ["covs", "covs_smoothed", "means", "means_smoothed", "status"]
    assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["means"].shape == (len(idx), 501, 4) and files["covs_smoothed"].shape == (len(idx), 501, 4, 4)
    assert files["status"].shape == (640,) and not files["status"].any()
    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(640, nobs=126, gap_h=1.0, seed0=0)  # bench.py's batch: seed = global track index
    hb = batch.pack_uniform(sb, 4, H, Q, R, P0)
    fires = hb.upd_idx.T[idx] >= 0
    zidx = np.where(fires, hb.upd_idx.T[idx], 0)
    ridx = np.cumsum(fires, axis=1) - fires
    rr = np.broadcast_to(batch.rts_rate_index(hb.Nmax + 1, 125, 126), (len(idx), hb.Nmax))
    m, P = orc.forward_batch(hb.x0.T[idx], P0, H, Q, R, hb.dt.T[idx], fires, zidx, ridx, sb.z[idx], sb.sog_rate[idx],
                             sb.cog_rate[idx])
    sm, sP = orc.backward_batch(m, P, Q, hb.dt.T[idx], rr, sb.sog_rate[idx], sb.cog_rate[idx])
    par = bench.compare_histories(files, {"means": m, "covs": P, "means_smoothed": sm, "covs_smoothed": sP})
    for name in ("means", "means_smoothed"):
        assert par[name]["max_rel_err"] < 1e-6, (name, par[name])
    for name in ("covs", "covs_smoothed"):
        assert par[name]["max_rel_err_per_matrix"] < 1e-5, (name, par[name])


def test_bench_dump_sample_is_fixed_and_bounded():
    """The --dump-outputs sample: the same tracks in every run, every track of a small batch, and within 64 MB at the
    default 10 000-track batch (four histories of 501 rows, 4 + 16 + 4 + 16 doubles per row, plus the status words)."""
    import bench

    a, b = bench.dump_sample(10_000), bench.dump_sample(10_000)
    assert np.array_equal(a, b) and len(np.unique(a)) == bench.DUMP_TRACKS and np.all(np.diff(a) > 0)
    assert a[0] >= 0 and a[-1] < 10_000
    assert np.array_equal(bench.dump_sample(100), np.arange(100))
    assert bench.DUMP_TRACKS * 501 * 40 * 8 + 10_000 * 8 <= 64 << 20


def test_bench_self_launch_command(monkeypatch):
    """CPU side of the same: the child command is the driver's own launch line around this script and its arguments."""
    import subprocess
    import sys

    import bench

    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env

        class R:
            returncode = 7

        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    assert bench.self_launch(4) == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_cli_optional_keys_parse_and_validate():
    from track_estimators.cli.main_cli import get_optional_settings

    assert get_optional_settings({}) == (False, 50.0, "wgs84", False)  # absent = the reference's behaviour
    assert get_optional_settings({"robust": True, "chi_alpha": 30, "geodesy": "sphere", "drop_duplicate_times": True}) == (
        True, 30.0, "sphere", True)
    for bad in ({"robust": "yes"}, {"chi_alpha": 0}, {"geodesy": "flat"}, {"drop_duplicate_times": 1}):
        with pytest.raises(ValueError):
            get_optional_settings(bad)


@pytest.mark.gpu
def test_cli_config4_robust_through_the_entry_point(tmp_path, monkeypatch):
    """BASELINE configs[3] through the reference's own entry point: `track_estimator` on a modern_ships id with
    `"robust": true` in input.json (plus `"geodesy": "sphere"`, the distance / heading pair the fixture's reference run
    used -- geographiclib is on neither box) must write the predictions and smoothed predictions of the reference run with
    its check_robustness call site enabled (tests/golden/modern_ships_robust.npz)."""
    from track_estimators.cli.main_cli import track_estimator

    gr = np.load(os.path.join(GOLDEN, "modern_ships_robust.npz"))
    monkeypatch.chdir(tmp_path)
    with gzip.open(os.path.join(GOLDEN, "data", "modern_ship_data.csv.gz"), "rb") as src, open("modern.csv", "wb") as dst:
        shutil.copyfileobj(src, dst)
    with open("input.json", "w") as f:
        json.dump({"dim": 4, "H": [1, 1, 0, 0], "R": [0.25, 0.25, 0, 0], "Q": [1e-4, 1e-4, 1e-6, 1e-6], "P": [1.0, 1.0, 1.0, 1.0],
                   "dt": -1, "nsteps": 2, "robust": True, "chi_alpha": 50.0, "geodesy": "sphere"}, f)
    with np.errstate(all="ignore"):
        track_estimator(["-t", "modern.csv", "-s", "WCE5063", "-ic", "id", "-lat", "lat", "-lon", "lon", "-rts", "--no-noise"])
    rows = gr["WCE5063_rows"]
    for fname, key in (("output_WCE5063_predictions.txt", "WCE5063_means"),
                       ("output_WCE5063_predictions_smoothed.txt", "WCE5063_means_smoothed")):
        got = np.loadtxt(fname)[rows]
        ref = gr[key]
        assert float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3))) < 1e-6, fname
    var = np.loadtxt("output_WCE5063_variances_smoothed.txt")[rows]
    refv = np.diagonal(gr["WCE5063_covs_smoothed"], axis1=1, axis2=2)
    assert float(np.max(np.abs(var - refv) / np.max(np.abs(gr["WCE5063_covs_smoothed"]), axis=(-1, -2))[:, None])) < 1e-5
    # without the key the same command is the plain filter: a different answer on this ship (38 419 rescaled updates)
    with open("input.json") as f:
        cfg = json.load(f)
    cfg.pop("robust")
    os.makedirs("plain", exist_ok=True)
    with open("plain/input.json", "w") as f:
        json.dump(cfg, f)
    monkeypatch.chdir(tmp_path / "plain")
    with np.errstate(all="ignore"):
        track_estimator(["-t", "../modern.csv", "-s", "WCE5063", "-ic", "id", "-lat", "lat", "-lon", "lon", "--no-noise"])
    plain = np.loadtxt("output_WCE5063_predictions.txt")[rows]
    assert np.abs(plain - gr["WCE5063_means"]).max() > 1e-3
