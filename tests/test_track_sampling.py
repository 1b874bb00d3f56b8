"""Posterior ship tracks sampled from the unscented smoother on the device (include/ste.h: ste_ukf_sample_f64 and the three
ste_urtss_sample_*_f64 entry points; DESIGN.md, "Posterior tracks"): declarations and refusals of the C ABI, the NumPy
restatement of the recursion against the pinned oracle, and on the GPU the two anchors -- zero draws reproduce the smoother
bit for bit, the ensemble covariance is the smoother's -- plus parity with the restatement on recorded draws, independence
of the surroundings (state of the work rows, sample count, windows, per-track noise) and the Python surface."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import track_sampling_cases as tsc
from conftest import ROOT
from test_hip_parity import MEAN_TOL
from test_ukf_loglik import _batch

STAT_S, STAT_SEED = 4096, 20241  # test 8 / test 4: sample count and the seed of the host draws
VAR_BOUND = 5.0 * np.sqrt(2.0 / (STAT_S - 1))


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for proto in (r"int ste_urtss_sample_prepare_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_noise_f64\* nz, "
                  r"const ste_ukf_sample_f64\* sm, void\* stream\);",
                  r"int ste_urtss_sample_draw_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_sample_f64\* sm, void\* stream\);",
                  r"int ste_urtss_sample_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_noise_f64\* nz, "
                  r"const ste_ukf_sample_f64\* sm, void\* stream\);"):
        assert re.search("^" + proto, hdr, flags=re.M), proto
    body = hdr[hdr.index("typedef struct ste_ukf_sample_f64 {"): hdr.index("} ste_ukf_sample_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double|size_t|void)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteUkfSampleF64._fields_] == ["nsamples", "flags", "samples", "coef", "status"]
    assert C.sizeof(binding.SteUkfSampleF64) == 32
    for name in ("ste_urtss_sample_prepare_f64", "ste_urtss_sample_draw_f64", "ste_urtss_sample_f64"):
        assert name in binding.SYMBOLS
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the sampler's arguments travel beside the batch
    # the ordering against a two-kernel smoother on another stream is the caller's, and the header says so
    assert "the caller orders prepare" in hdr[hdr.index("Posterior TRACKS"): hdr.index("typedef struct ste_ukf_sample_f64 {")]


def test_refusals_before_any_launch():
    """Every refusal of the header returns STE_EINVAL (-1) with its reason; a launch on a machine without a GPU would return
    STE_ELAUNCH (-2), so -1 shows the call stopped before launching (the pattern of tests/test_ukf_track_noise.py)."""
    from track_estimators._hip import binding

    lib, keep = binding.load(), []
    nz = binding.SteUkfNoiseF64(0x4000, None, 0, 0)
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    calls = {
        "ste_urtss_sample_prepare_f64": lambda s, m: lib.ste_urtss_sample_prepare_f64(ref(s), ref(nz), ref(m), None),
        "ste_urtss_sample_draw_f64": lambda s, m: lib.ste_urtss_sample_draw_f64(ref(s), ref(m), None),
        "ste_urtss_sample_f64": lambda s, m: lib.ste_urtss_sample_f64(ref(s), None, ref(m), None),
    }

    def good_batch():
        s = _batch(binding, keep)
        s.sm_mean = s.sm_cov = 0x6000
        s.rts_work = 0x3000
        return s

    def good_sample():
        return binding.SteUkfSampleF64(3, 0, 0x7000, 0x8000, 0x9000)

    for name, call in calls.items():
        def err(s, m):
            return call(s, m), lib.ste_last_error().decode()

        rc, msg = err(None, good_sample())
        assert rc == -1 and "batch pointer is NULL" in msg, name
        rc, msg = err(good_batch(), None)
        assert rc == -1 and "sampler arguments (sm) are NULL" in msg and name in msg
        for field in ("samples", "coef"):
            m = good_sample()
            setattr(m, field, None)
            rc, msg = err(good_batch(), m)
            assert rc == -1 and "sm->samples and sm->coef are required" in msg and name in msg, field
        for n in (0, -2):
            m = good_sample()
            m.nsamples = n
            rc, msg = err(good_batch(), m)
            assert rc == -1 and "nsamples must be >= 1" in msg and name in msg
        m = good_sample()
        m.flags = 0x1
        rc, msg = err(good_batch(), m)
        assert rc == -1 and "sm->flags must be 0" in msg and name in msg
        for field in ("rts_work", "fwd_mean", "fwd_cov"):
            s = good_batch()
            setattr(s, field, None)
            rc, msg = err(s, good_sample())
            assert rc == -1 and "completed forward pass with rts_work" in msg and name in msg, field
        for b, e in ((64, 0), (0, 128), (64, 256), (32, 128)):
            s = good_batch()
            s.step_begin, s.step_end = b, e
            rc, msg = err(s, good_sample())
            assert rc == -1 and "time slices" in msg and name in msg, (b, e)
        # whatever ste_urtss_backward_f64 refuses
        s = good_batch()
        s.n = 3
        rc, msg = err(s, good_sample())
        assert rc == -1 and "state dimension" in msg
        s = good_batch()
        s.track_stride = 4
        rc, msg = err(s, good_sample())
        assert rc == -1 and "track_stride" in msg
        s = good_batch()
        s.status = None
        rc, msg = err(s, good_sample())
        assert rc == -1 and "status" in msg
        s = good_batch()
        s.sm_mean = None
        rc, msg = err(s, good_sample())
        assert rc == -1 and "sm_mean and sm_cov are required" in msg
        assert lib.ste_urtss_backward_f64(C.byref(s), None) == -1  # ... and the smoother refuses it too
        # lane-mapping flags are ignored: with both set the smoother's own check (they exclude each other) is what is left
        s = good_batch()
        s.flags = binding.STE_FLAG_LANES_4
        s.n = 3
        rc, msg = err(s, good_sample())
        assert rc == -1 and "state dimension" in msg and "LANES" not in msg


def test_restatement_against_the_pinned_oracle():
    """Zero draws: the recursion is backward_track's mean recursion, difference exactly 0.  The propagated covariance
    C_k + K Cov(x_{k+1}) K^T is its smoothed covariance (1e-13 relative; measured 7e-16), and every conditional covariance
    C_k is positive definite with margin (smallest eigenvalue ratio > 1e-7; measured 4e-6)."""
    worst_cov, worst_eig, worst_seam = 0.0, np.inf, np.inf
    for case in tsc.oracle_cases():
        zero = tsc.sample_track(case.means, case.covs, case.steps, np.zeros((1, tsc.NMAX + 1, 4)))[0]
        assert np.array_equal(zero, case.sm_means)
        pc = tsc.propagated_cov(case.covs, case.steps)
        worst_cov = max(worst_cov, float(np.max(np.abs(pc - case.sm_covs) / np.max(np.abs(case.sm_covs), axis=(-1, -2), keepdims=True))))
        for q in case.steps:
            w = np.linalg.eigvalsh(0.5 * (q["C"] + q["C"].T))
            worst_eig = min(worst_eig, float(w[0] / w[-1]))
        h = case.sm_means[:, 3]
        worst_seam = min(worst_seam, float(np.min(np.minimum(h, 360.0 - h))))
    print(f"propagated covariance vs backward_track: {worst_cov:.2e} relative; min eigenvalue ratio of C_k: {worst_eig:.2e}; "
          f"closest heading to the 0/360 seam: {worst_seam:.1f} deg")
    assert worst_cov < 1e-13
    assert worst_eig > 1e-7
    assert worst_seam > 10.0  # what lets the statistics below treat heading like any other component


def _stat_draws():
    """Host draws of the statistics tests, (S, Nmax+1, 4, 8): the device layout of ste_ukf_sample_f64.samples."""
    return np.random.default_rng(STAT_SEED).standard_normal((STAT_S, tsc.NMAX + 1, 4, 8))


def _assert_statistics(samples_by_track, what):
    worst_m = worst_v = 0.0
    for b, case in enumerate(tsc.oracle_cases()):
        m, v = tsc.sample_statistics(samples_by_track(b), case.sm_means, case.sm_covs)
        worst_m, worst_v = max(worst_m, m), max(worst_v, v)
    print(f"{what}: worst |mean_S - sm_mean| = {worst_m:.3f} of its 5-sigma bound, worst |var_S / sm_var - 1| = "
          f"{worst_v * VAR_BOUND:.4f} (bound {VAR_BOUND:.3f})")
    assert worst_m <= 1.0 and worst_v <= 1.0


def test_statistics_of_the_restatement():
    """The 832 comparisons of test_statistics (GPU) on the restatement with the same host draws: the reference itself stays
    inside the 5-sigma bounds for the chosen seed."""
    xi = _stat_draws()
    cases = tsc.oracle_cases()
    _assert_statistics(lambda b: tsc.sample_track(cases[b].means, cases[b].covs, cases[b].steps,
                                                  np.ascontiguousarray(xi[..., b])), "restatement")


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _sample(db, draws, how="both", noise="own"):
    """Run the sampler on a DeviceBatch through the C ABI with host draws (S, N+1, 4, B); returns (samples, status)."""
    from track_estimators._hip import binding

    torch = db.torch
    t = torch.from_numpy(np.ascontiguousarray(draws)).to(db.device)
    sm, status, keep = db._sample_struct(t, t.shape[0])
    nz = None if db.noise is None else C.byref(db.noise)
    st = db._stream(None)
    if how == "both":
        binding.check(db.lib.ste_urtss_sample_f64(C.byref(db.struct), nz, C.byref(sm), st), "ste_urtss_sample_f64")
    else:
        binding.check(db.lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), nz, C.byref(sm), st), "prepare")
        binding.check(db.lib.ste_urtss_sample_draw_f64(C.byref(db.struct), C.byref(sm), st), "draw")
        first = t.cpu().numpy().copy()
        t.copy_(torch.from_numpy(np.ascontiguousarray(draws)))
        binding.check(db.lib.ste_urtss_sample_draw_f64(C.byref(db.struct), C.byref(sm), st), "draw")
        assert np.array_equal(_u64(first), _u64(t.cpu().numpy())), "draw twice from one prepare"
    torch.cuda.synchronize()
    return t.cpu().numpy(), status.cpu().numpy()


def _snapshot(db):
    return {n: getattr(db, n).cpu().numpy().copy() for n in ("status", "fwd_mean", "fwd_cov", "rts_work")}


@pytest.mark.gpu
def test_zero_draws_reproduce_the_smoother():
    """S = 2, B = 70, ragged: with all draws zero every sample is sm_mean on rows 0 .. ns, as values, whatever the work rows hold
    -- after forward() alone (against a later backward()), after the two-kernel smoother, after the one-kernel smoother --
    and rows past ns are untouched."""
    from track_estimators import batch

    hb = tsc.host_batch(tsc.B70_TRACKS, tsc.B70_NSTEPS)
    mark = -777.0
    draws = np.zeros((2, tsc.NMAX + 1, 4, 70))
    for b, ns in enumerate(hb.nsteps):
        draws[:, ns + 1:, :, b] = mark
    for state, tuning in (("forward", 0x200), ("two-kernel", 0x200), ("two-kernel-lane", 0x200 | 0x800), ("one-kernel", 0x400)):
        db = batch.DeviceBatch(hb, tuning=tuning)
        db.forward()
        if state != "forward":
            db.backward()
        got, status = _sample(db, draws)
        if state == "forward":
            db.backward()
        db.torch.cuda.synchronize()
        sm = db.sm_mean.cpu().numpy()
        assert not status.any() and not db.status.cpu().numpy().any(), state
        for b, ns in enumerate(hb.nsteps):
            for s in range(2):
                assert np.array_equal(got[s, : ns + 1, :, b], sm[: ns + 1, :, b]), (state, b, s)
                assert np.all(got[s, ns + 1:, :, b] == mark), (state, b, s)


@pytest.mark.gpu
@pytest.mark.parametrize("track_q", [False, True], ids=["shared-Q", "per-track-Q"])
def test_zero_draws_reproduce_a_smoother_with_rates_of_its_own(track_q):
    """The same with smoother rates that differ from the forward pass's (sog_rate_rts / cog_rate_rts: the kShift instantiations
    of urtss_sample_coef, which the eight tracks' packing -- two sub-steps, shared rates -- never takes), with the shared Q and
    with a Q per track: S = 2, B = 70, ragged, all draws zero.  Every sample is sm_mean on rows 0 .. ns, as values, from work
    rows that hold D (after forward() alone, against the one-kernel smoother) and from rows that hold gains (after the
    two-kernel smoother)."""
    from track_estimators import batch, synthetic

    Qs = None
    if track_q:
        _, Q, _, _ = synthetic.example_matrices()
        Q2 = Q * 2.0
        Q2[0, 2] = Q2[2, 0] = 1e-6
        Q2[1, 3] = Q2[3, 1] = -2e-6
        Qs = np.stack([Q, Q2, Q * 0.5, Q2] * 2)[tsc.B70_TRACKS]
    hb = tsc.host_batch(tsc.B70_TRACKS, tsc.B70_NSTEPS, Qs=Qs, lanes=1)
    hb = dataclasses.replace(hb, sog_rate_rts=hb.sog_rate * 1.25 + 0.01, cog_rate_rts=hb.cog_rate * 0.75 - 0.02)
    draws = np.zeros((2, tsc.NMAX + 1, 4, 70))
    for state, tuning in (("forward", 0x400), ("two-kernel", 0x200)):
        db = batch.DeviceBatch(hb, tuning=tuning)
        assert db.struct.sog_rate_rts and db.struct.cog_rate_rts and (db.noise is not None) == track_q
        db.forward()
        if state != "forward":
            db.backward()
        got, status = _sample(db, draws)
        if state == "forward":
            db.backward()
        db.torch.cuda.synchronize()
        sm = db.sm_mean.cpu().numpy()
        assert not status.any() and not db.status.cpu().numpy().any(), state
        for b, ns in enumerate(hb.nsteps):
            for s in range(2):
                assert np.array_equal(got[s, : ns + 1, :, b], sm[: ns + 1, :, b]), (state, b, s)


@pytest.mark.gpu
def test_recorded_draws_against_the_restatement():
    """S = 3 with host draws, the eight tracks plus a ragged copy of them: every component within MEAN_TOL of the restatement,
    relative to max(|ref|, smoothed standard deviation), heading through wrap180; sampler status 0; the batch's status,
    histories and work rows are bit-identical before and after (the sampler only reads them).
    Measured on an MI355X: 1.54e-12, after forward() and after the two-kernel smoother alike."""
    from track_estimators import batch

    cases = tsc.oracle_cases()
    ragged = [0, 1, 2, 5, 7, 9, 11, 12]
    hb = tsc.host_batch(np.arange(16) % 8, [tsc.NMAX] * 8 + ragged)
    draws = np.random.default_rng(5).standard_normal((3, tsc.NMAX + 1, 4, 16))
    for state in ("forward", "smoothed"):
        db = batch.DeviceBatch(hb)
        db.forward()
        if state == "smoothed":
            db.backward()
        db.torch.cuda.synchronize()
        before = _snapshot(db)
        got, status = _sample(db, draws)
        after = _snapshot(db)
        for name in before:
            assert np.array_equal(before[name].view(np.uint8), after[name].view(np.uint8)), (state, name)
        assert not status.any(), state
        worst = 0.0
        for b, ns in enumerate(hb.nsteps):
            means, covs, steps, _, sm_cov = tsc.truncated(cases[b % 8], int(ns))
            ref = tsc.sample_track(means, covs, steps, np.ascontiguousarray(draws[:, : ns + 1, :, b]))
            d = got[:, : ns + 1, :, b] - ref
            d[..., 3] = tsc.wrap180(d[..., 3])
            scale = np.maximum(np.abs(ref), np.sqrt(np.einsum("kcc->kc", sm_cov))[None])
            worst = max(worst, float(np.max(np.abs(d) / scale)))
        print(f"samples vs restatement ({state}): {worst:.2e}")
        assert worst < MEAN_TOL, state


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Samples from D-form rows equal samples from gain-form rows; S = 5 and S = 1 agree on the third sample, and S = 5 with 1,
    2 and 4 samples per lane agree (a sample count that is no multiple of the samples per lane); windows [0, 64) and [64, 70)
    equal the whole-batch call; draw twice from one prepare gives the same bits."""
    from track_estimators import batch

    hb = tsc.host_batch(tsc.B70_TRACKS, tsc.B70_NSTEPS)
    draws = np.random.default_rng(11).standard_normal((5, tsc.NMAX + 1, 4, 70))
    db = batch.DeviceBatch(hb, tuning=0x200)
    db.forward()
    from_d, st_d = _sample(db, draws)
    one, _ = _sample(db, draws[2:3])
    twice, _ = _sample(db, draws, how="prepare+draw+draw")
    parts = np.empty_like(draws)
    for lo, hi in ((0, 64), (64, 70)):
        w = db.window(lo, hi)
        out = w.sample_smoothed(5, draws=db.torch.from_numpy(np.ascontiguousarray(draws[..., lo:hi])).to(db.device))
        parts[..., lo:hi] = out.cpu().numpy()
    # the library picks 1, 2 or 4 samples per lane by launch size: same bits whichever, S = 5 being a multiple of none but 1
    lanes = db.lib.ste_dbg_sample_lanes
    lanes.restype, lanes.argtypes = C.c_int, [C.c_int]
    forced = {}
    try:
        for spl in (1, 2, 4):
            lanes(spl)
            forced[spl] = _sample(db, draws)[0]
    finally:
        lanes(0)
    db.backward()  # two-kernel form: the work rows hold gains from here on
    db.torch.cuda.synchronize()
    assert (db.rts_work[-1].cpu().numpy() < 0).all()
    from_k, st_k = _sample(db, draws)
    assert not st_d.any() and not st_k.any()
    assert not np.array_equal(from_d[0], from_d[1])
    for b, ns in enumerate(hb.nsteps):
        rows = (slice(None), slice(0, ns + 1), slice(None), b)
        assert np.array_equal(_u64(from_d[rows]), _u64(from_k[rows])), ("D / gain form", b)
        assert np.array_equal(_u64(from_d[rows][2]), _u64(one[rows][0])), ("S = 5 / S = 1", b)
        assert np.array_equal(_u64(from_d[rows]), _u64(twice[rows])), ("prepare + draw", b)
        assert np.array_equal(_u64(from_d[rows]), _u64(parts[rows])), ("windows", b)
        for spl in (1, 2, 4):
            assert np.array_equal(_u64(from_d[rows]), _u64(forced[spl][rows])), ("samples per lane", spl, b)
            assert np.array_equal(_u64(forced[spl][:, ns + 1:, :, b]), _u64(draws[:, ns + 1:, :, b])), ("rows past ns", spl, b)
        assert np.array_equal(_u64(from_d[:, ns + 1:, :, b]), _u64(draws[:, ns + 1:, :, b])), ("rows past ns", b)


@pytest.mark.gpu
def test_per_track_noise_equals_the_shared_batch_of_that_track():
    from track_estimators import batch, synthetic

    _, Q, _, _ = synthetic.example_matrices()
    Q2 = Q * 2.0
    Q2[0, 2] = Q2[2, 0] = 1e-6
    Q2[1, 3] = Q2[3, 1] = -2e-6
    Qs = np.stack([Q, Q2, Q * 0.5, Q2] * 2)
    draws = np.random.default_rng(12).standard_normal((3, tsc.NMAX + 1, 4, 8))
    nsteps = [12, 11, 12, 7, 12, 12, 3, 12]
    per, st = _sample(_forward(batch.DeviceBatch(tsc.host_batch(np.arange(8), nsteps, Qs=Qs, lanes=1))), draws)
    assert not st.any()
    shared = {}
    for b in (1, 2, 6):
        key = Qs[b].tobytes()
        if key not in shared:
            hb = dataclasses.replace(tsc.host_batch(np.arange(8), nsteps, lanes=1), Q=np.ascontiguousarray(Qs[b]))
            shared[key] = _sample(_forward(batch.DeviceBatch(hb)), draws)[0]
        ns = nsteps[b]
        assert np.array_equal(_u64(per[:, : ns + 1, :, b]), _u64(shared[key][:, : ns + 1, :, b])), b
    assert not np.array_equal(shared[Qs[1].tobytes()][..., 0], shared[Qs[2].tobytes()][..., 0])


def _forward(db):
    db.forward()
    return db


@pytest.mark.gpu
def test_statistics():
    """S = 4096 on the eight tracks with host draws: per track, row and component |mean_S - sm_mean| <= 5 sqrt(sm_var / S) and
    |var_S / sm_var - 1| <= 5 sqrt(2 / (S - 1)) = 0.110 (heading differences through wrap180): the 5-sigma bounds of the two
    estimators under the ensemble-covariance property.  832 comparisons; with the fixed seed the false-alarm question is
    settled by test_statistics_of_the_restatement."""
    from track_estimators import batch

    db = _forward(batch.DeviceBatch(tsc.host_batch(np.arange(8))))
    got, status = _sample(db, _stat_draws())
    assert not status.any()
    _assert_statistics(lambda b: got[..., b], "device")


@pytest.mark.gpu
def test_python_surface():
    from track_estimators import batch

    hb = tsc.host_batch(np.arange(8), [12, 11, 12, 7, 12, 12, 3, 12])
    db = _forward(batch.DeviceBatch(hb))
    a, b, c = db.sample_smoothed(4, seed=3), db.sample_smoothed(4, seed=3), db.sample_smoothed(4, seed=4)
    assert tuple(a.shape) == (4, tsc.NMAX + 1, 4, 8) and a.is_cuda
    assert db.torch.equal(a, b) and not db.torch.equal(a, c)
    assert not db.sample_status.cpu().numpy().any()
    # batch.sample_tracks: track-major like download, from a DeviceBatch and from a HostBatch
    s1, st1 = batch.sample_tracks(db, 4, seed=3)
    s2, st2 = batch.sample_tracks(hb, 4, seed=3)
    assert s1.shape == (4, 8, tsc.NMAX + 1, 4) and st1.shape == (8,) and not st1.any() and not st2.any()
    assert np.array_equal(s1, a.permute(0, 3, 1, 2).cpu().numpy()) and np.array_equal(s1, s2)
    db.backward()
    sm = db.download(("means_smoothed",))["means_smoothed"]
    zero = db.sample_smoothed(1, draws=db.torch.zeros((1, tsc.NMAX + 1, 4, 8), dtype=db.torch.float64, device=db.device))
    for t, ns in enumerate(hb.nsteps):
        assert np.array_equal(zero.permute(0, 3, 1, 2).cpu().numpy()[0, t, : ns + 1], sm[t, : ns + 1]), t
    with pytest.raises(ValueError, match="fuse_gains=False"):
        _forward(batch.DeviceBatch(hb, fuse_gains=False)).sample_smoothed(2)
    with pytest.raises(ValueError, match="histories=False"):
        batch.DeviceBatch(hb, histories=False).sample_smoothed(2)
    with pytest.raises(ValueError, match="draws must be"):
        db.sample_smoothed(2, draws=db.torch.zeros((3, 2), dtype=db.torch.float64, device=db.device))


@pytest.mark.gpu
def test_dropin_sample_smoothed():
    """UnscentedKalmanFilter.sample_smoothed: (n, N+1, 4) whose mean over n = 256 lies within the 5-sigma bound of
    run_rts_smoother's means (variances from its covariances)."""
    import types

    from track_estimators import synthetic
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter

    sb = tsc.synthetic_batch()
    H, Q, R, P0 = synthetic.example_matrices()
    trk = types.SimpleNamespace(z=sb.z[0], dts=sb.dts[0], sog=sb.sog[0], cog=sb.cog[0], sog_rate=sb.sog_rate[0].copy(),
                                cog_rate=sb.cog_rate[0].copy())
    ukf = UnscentedKalmanFilter(H=H, Q=Q, R=R, P=P0, x0=sb.z[0][:, 0], non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.sample_smoothed(2)
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    n = 256
    samples = ukf.sample_smoothed(n, random_state=1)
    assert samples.shape == (n, tsc.NMAX + 1, 4)
    sm, sP = ukf.run_rts_smoother(trk)
    d = samples - sm[None]
    d[..., 3] = tsc.wrap180(d[..., 3])
    ratio = np.abs(d.mean(axis=0)) / (5.0 * np.sqrt(np.einsum("kcc->kc", sP) / n))
    print(f"drop-in: worst |mean_n - smoothed mean| = {ratio.max():.3f} of its 5-sigma bound")
    assert ratio.max() <= 1.0
    assert np.array_equal(ukf.sample_smoothed(3, random_state=1), ukf.sample_smoothed(3, random_state=1))
