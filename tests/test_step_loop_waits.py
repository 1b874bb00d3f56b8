"""The step loops of the lane-per-track forward pass and of the one-kernel smoother after their loads and stores were
reordered ("Store drain"): no bit of the histories, the work rows, the status words or the first-bad words
moved.

Against tests/golden/step_loop_bits_parent.npz, which the commit before that change wrote on the GPU (the batches, the launch
forms and the digests are in tests/step_loop_cases.py, which also says why each case is there), and within this build between
the forms the project documents as bit-identical: whole pass = two time slices = scheduled launch (include/ste.h: step_begin /
step_end, ste_ukf_forward_sched_f64), one-kernel = two-kernel smoother (csrc/ste_smooth.hip).
"""
import os

import numpy as np
import pytest

import step_loop_cases as slc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_loop_bits_parent.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def whole():
    """Case -> outputs of the whole pass (DeviceBatch.run, one-kernel smoother), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = slc.run_whole(slc.build_case(name))
        return cache[name]

    return get


def _same_bits(a, b, what):
    for k in slc.ARRAYS + ("status",):
        x, y = a[k], b[k]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f"{what}: {k} differs at {np.argwhere(x != y)[:4].tolist()}"


def test_fixture_is_recorded_from_a_named_commit_and_fits(golden):
    assert len(str(golden["commit"])) == 40
    assert os.path.getsize(GOLDEN) < 400 << 10
    assert int(golden["ntracks"]) == slc.NTRACKS and int(golden["nsteps"]) == slc.NSTEPS


def test_cases_are_what_they_are_meant_to_be():
    """On the host: the lengths hold 0, 1, 2, 3 and both sides of the 64-step restart in the first wave, the second wave has
    one lane, two slices cut at step 64, and the update patterns are all / none / one in four."""
    from track_estimators import batch

    n = slc.ragged_lengths()
    assert len(n) == 65 and set((0, 1, 2, 3, 63, 64, 65)) <= set(n[:64].tolist()) and n[64] == 65
    assert batch.DeviceBatch.slice_bounds(slc.NSTEPS, 2) == [(0, 64), (64, 65)]
    frac = {name: float((slc.build_case(name).upd_idx >= 0).mean()) for name in ("every", "none", "quarter")}
    assert frac["every"] == 1.0 and frac["none"] == 0.0 and abs(frac["quarter"] - 0.25) < 0.01
    hb = slc.build_case("none_noinit")
    assert not hb.initial_update and slc.build_case("none").initial_update
    assert slc.build_case("noise").noise_rts is not None and slc.build_case("shift").sog_rate_rts is not None
    assert slc.build_case("track_noise").Q_tracks is not None and slc.build_case("track_noise").R_tracks is not None
    bad = slc.build_case("bad_prior")
    assert n[9] > 3 and n[20] > 3 and n[30] > 3 and np.isnan(bad.P0[5, 20]) and np.isinf(bad.x0[2, 30]) and bad.P0[5, 9] < 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", slc.CASES)
def test_bits_match_the_build_before_the_reordering(golden, whole, name):
    out = whole(name)
    assert np.array_equal(out["status"], golden[f"{name}_status"])
    assert np.array_equal(out["rts_work"][-1].view(np.uint64), golden[f"{name}_first_bad"].view(np.uint64))
    for arr in slc.ARRAYS:
        rows, tracks, sha = slc.digests(out[arr])
        g_rows, g_tracks = golden[f"{name}_{arr}_rows"], golden[f"{name}_{arr}_tracks"]
        assert np.array_equal(tracks, g_tracks), f"{arr}: tracks {np.nonzero(tracks != g_tracks)[0].tolist()} differ"
        assert np.array_equal(rows, g_rows), f"{arr}: first differing row {int(np.nonzero(rows != g_rows)[0][0])}"
        assert sha == str(golden[f"{name}_{arr}_sha256"]), arr
    if name == "bad_prior":  # the clamped tracks took the gain's cold branch from step 0 on, the non-finite ones end non-finite
        fb = out["rts_work"][-1]
        assert fb[9] == 0.0 and fb[64] == 0.0 and fb[0] == 1e300
        assert not np.isfinite(out["sm_mean"][0][:, [20, 30]]).any(axis=0).any() and np.isfinite(out["sm_mean"][0][:, [9, 64]]).all()
    # a live case: every track with steps has smoothed rows that are not the buffer's fill
    n = slc.ragged_lengths()
    assert (out["sm_mean"][0][:, n > 0] != slc.SENTINEL).all() and (out["sm_mean"][1][:, n == 0] == slc.SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", slc.CASES)
def test_two_time_slices_are_the_whole_pass(whole, name):
    _same_bits(whole(name), slc.run_sliced(slc.build_case(name), 2), f"{name}, 2 slices")


@pytest.mark.gpu
def test_scheduled_launch_is_the_whole_pass(whole):
    """Forward pass and smoother as scheduled launches (ukf_forward_sched, urtss_recur_sched), every case but the one with
    per-track noise, which scheduled launches do not take."""
    from track_estimators import batch

    with batch.SmootherPipeline(ntracks=slc.NTRACKS, sequence_only=True) as pipe:
        for name in slc.CASES:
            if name == "track_noise":
                continue
            _same_bits(whole(name), slc.run_scheduled(slc.build_case(name), pipe), f"{name}, scheduled")


@pytest.mark.gpu
@pytest.mark.parametrize("name", slc.CASES)
def test_two_kernel_smoother_is_the_one_kernel_smoother(whole, name):
    """urtss_gains_all + the quad and the lane recurrence against urtss_recur_l1 / _tn: histories and status (the work rows
    hold gains afterwards).  Bit for bit, except that a NaN equals a NaN whatever its payload: on the NaN and infinite tracks
    of `bad_prior` the lane recurrence propagates other payloads into sm_cov than the one-kernel smoother, in the build the
    fixture was recorded from as well (tests/test_fleet.py compares the two forms the same way)."""
    def bits(a):
        return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64)) if a.dtype == np.float64 else a

    one = whole(name)
    for tuning in (slc.TWO_KERNEL, slc.TWO_KERNEL | slc.LANE_RECURRENCE):
        two = slc.run_whole(slc.build_case(name), tuning)
        for k in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "status"):
            x, y = bits(one[k]), bits(two[k])
            assert np.array_equal(x, y), f"{name}, tuning {tuning:#x}: {k} differs at {np.argwhere(x != y)[:4].tolist()}"
