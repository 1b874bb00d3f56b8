"""The forward step's outputs, bit for bit, against the build of the commit recorded in tests/golden/forward_step_bits.npz.

Work on the step's instruction stream (the range guards of the branch-free transcendentals, the shape of the Jacobi sweep
loop) must move no bit of the four histories, the smoother's work rows or the status words -- for ordinary lanes, for lanes
that leave through the fallback fan and for lanes that are non-finite from the start.  The batch and the digests are those of
tests/golden/make_forward_step_bits.py (which also says why the file holds digests of the bit patterns, not the 8 MB of
arrays): 130 tracks x 130 steps, crafted tracks among synthetic ones, lanes=1 and lanes=4.

Where the crafted tracks sit in the lane-per-track mapping (waves 0-63, 64-127, 128-129):
  * the track just UNDER the pi/4 limit of a pair delta is in the first wave, whose other lanes are ordinary: if its verdict
    turned to "out of range" the whole wave would go through the fallback fan, whose last bits differ from the fast path's
    (known dependence on wave neighbours), and the wave's digests would leave the recording;
  * the track just OVER the limit is the only crafted lane of the third wave: that wave takes the fallback in the recording
    because of this lane's verdict alone, so a verdict turned to "in range" shows in the bits of both its tracks;
  * the polar track, the two with steps of tens of degrees, the NaN prior and the infinite state share the second wave.
With lanes=4 these 130 tracks run one per wave (KParams::qpw), so every verdict shows in its own track.
"""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_forward_step_bits", os.path.join(GOLDEN, "make_forward_step_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rec():
    return _recorder()


@pytest.fixture(scope="module")
def hb(rec):
    return rec.build_batch()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "forward_step_bits.npz"))


def test_fixture_is_recorded_from_a_named_commit_and_fits(golden):
    assert len(str(golden["commit"])) == 40
    assert os.path.getsize(os.path.join(GOLDEN, "forward_step_bits.npz")) < 1 << 20


def test_fixture_holds_lanes_in_range_and_lanes_out_of_range(rec, hb):
    """On the host, the guarded quantities of the crafted tracks at the first fan (T = sqrt(fan_scale P0) there): the two
    pi/4 tracks sit on either side of sincos_delta_n's limit, the fast tracks step by more than asin(1/2) = 30 degrees
    (geodetic_finish_n's |xs| <= 1/2), the polar track fails the arctangent's |a| <= 0.4375 b for its longitude pair."""
    from track_estimators import batch

    scale = batch.sigma_constants(4)[0]
    d = np.sqrt(scale * hb.P0[15, [10, 129]]) * 0.017453292519943295
    assert d[0] < 0.78539816339744828 < d[1]
    assert abs(d[0] / 0.78539816339744828 - 1) < 2e-6 and abs(d[1] / 0.78539816339744828 - 1) < 2e-6
    step = hb.x0[2, [90, 91]] * hb.dt[0, [90, 91]] / 6378.137  # arc of the centre point's step, radians
    assert (np.sin(step) > 0.5).all() and (step < np.pi / 2).all()
    # polar track: the +T[0][0] point's longitude differs from the centre's by sqrt(3) degrees and the track starts 11 m from the pole, which the step
    # of 5 km carries it across: b = cos(lat') cos(dlon) and a = cos(lat') sin(dlon) are of one size
    assert 90.0 - hb.x0[1, 70] < 1.1e-4 and set(rec.FALLBACK) == {70, 90, 91, 129}
    assert not any(t < 64 for t in rec.CRAFTED if t != 10)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_forward_step_bits_match_the_recorded_build(rec, hb, golden, lanes):
    out = rec.run(hb, lanes)
    assert np.array_equal(out["status"], golden[f"l{lanes}_status"]), (out["status"], golden[f"l{lanes}_status"])
    for name in rec.ARRAYS:
        rows, tracks, sha = rec.digests(out[name])
        g_rows, g_tracks = golden[f"l{lanes}_{name}_rows"], golden[f"l{lanes}_{name}_tracks"]
        assert np.array_equal(tracks, g_tracks), f"{name}: tracks {np.nonzero(tracks != g_tracks)[0].tolist()} differ"
        assert np.array_equal(rows, g_rows), f"{name}: first differing row {int(np.nonzero(rows != g_rows)[0][0])}"
        assert sha == str(golden[f"l{lanes}_{name}_sha256"]), name
    # the crafted tracks are what they were meant to be: the two non-finite ones end non-finite, the others finite
    fin = np.isfinite(out["fwd_mean"][-1]).all(axis=0)
    assert not fin[100] and not fin[110]
    assert fin[[10, 70, 90, 91, 129]].all()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4])
def test_waves_without_a_lane_out_of_range_do_not_take_the_fallback(rec, hb, golden, lanes):
    """A second run without the crafted tracks -- no wave of it takes the fallback fan -- track by track against the recorded
    digests: an ordinary track whose wave holds no lane out of range has the recorded bits.  lanes=1: tracks 0-63 (the
    first wave, which in the recording also holds the track just under pi/4); lanes=4: every ordinary track.  Nothing is
    asserted about the ordinary tracks of the other two lanes=1 waves: they went through the fallback in the recording, and
    whether its bits equal the fast path's is not this test's business (today they do not; the count is printed)."""
    keep = np.array([t for t in range(rec.NTRACKS) if t not in rec.CRAFTED])
    assert len(keep) == rec.NTRACKS - 7
    out = rec.run(rec.take_tracks(hb, keep), lanes)
    assert not out["status"].any() and not golden[f"l{lanes}_status"][keep].any()
    alone = np.ones(len(keep), dtype=bool) if lanes == 4 else keep < 64
    for name in rec.ARRAYS:
        tracks = rec.digests(out[name])[1]
        g = golden[f"l{lanes}_{name}_tracks"][keep]
        assert np.array_equal(tracks[alone], g[alone]), f"{name}: kept tracks {np.nonzero((tracks != g) & alone)[0].tolist()} differ"
        print(f"lanes={lanes} {name}: {int((tracks != g).sum())} ordinary tracks carry other bits than without the crafted tracks")
