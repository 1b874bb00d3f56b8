"""The ``device_prep`` key of the CLI's input.json, with the device stubbed: ``batch.prepare_ship_tracks`` and
``batch.run_fleet`` are replaced, so these run without a GPU and check the plumbing alone."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest
from conftest import GOLDEN

BASE = {"dim": 4, "H": [1, 1, 0, 0], "R": [0.001, 0.001, 0, 0], "Q": [1e-2, 1e-2, 1e-4, 1e-4], "P": [1.0, 1.0, 1.0, 1.0],
        "dt": -1, "nsteps": 2}
ARGS = ["-t", "hist.csv", "-ic", "primary.id", "-lat", "lat", "-lon", "lon", "--no-noise"]


@pytest.fixture
def stubbed(tmp_path, monkeypatch):
    from track_estimators import batch
    from track_estimators.utils import smooth

    monkeypatch.chdir(tmp_path)
    with gzip.open(os.path.join(GOLDEN, "data", "historical_ship_data.csv.gz"), "rb") as src, open("hist.csv", "wb") as dst:
        shutil.copyfileobj(src, dst)
    calls = {"prep": [], "fleet": 0}

    def fake_prepare(ship_tracks, smooth_sog=None, smooth_cog=None, cog_circular=False, device="cuda:0"):
        calls["prep"].append((len(ship_tracks), smooth_sog, smooth_cog, cog_circular))
        for st in ship_tracks:  # the host's arithmetic stands in for the launch
            st.calculate_cog()
            st.calculate_sog()
            if smooth_sog is not None:
                st.sog = smooth(st.sog, smooth_sog.window)
            if smooth_cog is not None:
                st.cog = smooth(st.cog, smooth_cog.window)
            st.get_measurements(include_sog=True, include_cog=True)
            st.calculate_cog_rate()
            st.calculate_sog_rate()
        return ship_tracks

    def fake_fleet(hb, smooth=True, **kw):
        calls["fleet"] += 1
        calls["hb"] = hb
        n1 = hb.Nmax + 1
        return {"status": np.zeros(hb.B, dtype=np.int32), "nsteps": hb.nsteps, "means": np.zeros((hb.B, n1, 4)),
                "covs": np.zeros((hb.B, n1, 4, 4)), "means_smoothed": np.zeros((hb.B, n1, 4)),
                "covs_smoothed": np.zeros((hb.B, n1, 4, 4))}

    monkeypatch.setattr(batch, "prepare_ship_tracks", fake_prepare)
    monkeypatch.setattr(batch, "run_fleet", fake_fleet)
    return calls


def _write_input(**extra):
    with open("input.json", "w") as f:
        json.dump(dict(BASE, **extra), f)


def test_device_prep_prepares_all_ships_in_one_call_with_box_filters(stubbed):
    from track_estimators import batch
    from track_estimators.cli.main_cli import track_estimator

    _write_input(device_prep=True, smooth=5, geodesy="sphere")
    track_estimator(ARGS + ["-s", "01203823,01205638"])
    assert len(stubbed["prep"]) == 1 and stubbed["fleet"] == 1
    ntracks, fs, fc, circular = stubbed["prep"][0]
    assert ntracks == 2 and circular is False
    for f in (fs, fc):
        want = batch.box_filter(5)
        assert (f.window, f.left, f.nedge) == (want.window, want.left, want.nedge) and np.array_equal(f.taps, want.taps)
    assert stubbed["hb"].B == 2 and os.path.exists("output_01205638_predictions.txt")
    # the prior of ship 01203823 is the smoothed row 0 of the reference's CLI run (tests/golden/cli_smooth.npz, sphere pair)
    z0 = np.load(os.path.join(GOLDEN, "cli_smooth.npz"))["z"][:, 0]
    assert any(np.allclose(stubbed["hb"].x0[:, b], z0, rtol=1e-12, atol=0) for b in range(2))


@pytest.mark.parametrize("smooth", [None, -1, 0, 1])
def test_device_prep_without_smoothing_passes_no_filter(stubbed, smooth):
    from track_estimators.cli.main_cli import track_estimator

    _write_input(device_prep=True, **({} if smooth is None else {"smooth": smooth}))
    track_estimator(ARGS + ["-s", "01203823,01205638"])
    assert stubbed["prep"] == [(2, None, None, False)]


def test_device_prep_must_be_a_boolean(stubbed):
    from track_estimators.cli.main_cli import get_device_prep, track_estimator

    assert get_device_prep({}) is False and get_device_prep({"device_prep": True}) is True
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="device_prep"):
            get_device_prep({"device_prep": bad})
    _write_input(device_prep="yes")
    with pytest.raises(ValueError, match="device_prep"):
        track_estimator(ARGS + ["-s", "01203823,01205638"])
    assert stubbed["prep"] == [] and stubbed["fleet"] == 0


def test_without_the_key_nothing_new_is_called(stubbed):
    from track_estimators.cli.main_cli import track_estimator

    _write_input(smooth=5)
    track_estimator(ARGS + ["-s", "01203823,01205638"])
    assert stubbed["prep"] == [] and stubbed["fleet"] == 1
    _write_input(smooth=5, device_prep=False)
    track_estimator(ARGS + ["-s", "01203823,01205638"])
    assert stubbed["prep"] == [] and stubbed["fleet"] == 2
