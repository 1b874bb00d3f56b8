"""Per-track process and measurement noise (include/ste.h: ste_ukf_noise_f64 and the three *_noise_f64 entry points;
DESIGN.md section 5, "Per-track noise"): declarations and refusals of the C ABI, packing of (B, 4, 4) stacks, the step from
``best_noise(per_track=True)`` to a batch that uses the answer, and on the GPU the bit-identity with shared launches the
header promises, parity with the per-track oracle, independence of the other tracks' matrices, windows and fleets."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
from conftest import ROOT
from test_hip_parity import COV_TOL, MEAN_TOL, cov_err, mean_err
from test_ukf_loglik import (FLEET_SUBSTEPS, GENERAL_R, LIK_RTOL, _batch, _check_track, _synthetic_hb, fleet_candidates,
                             fleet_restatement, restate_track)


# The mixed fleet of the issue: the 16-track fleet of the R-grid tests with extra lon / lat noise on the odd-numbered tracks
# (0.2 deg std in all, against the generator's 0.05), so that two populations of sources share one batch.
ORACLE_ARGMAX = [4, 8, 4, 8, 3, 8, 4, 8, 4, 8, 4, 8, 4, 7, 4, 8]  # per-track argmax of the oracle over fleet_candidates()
ORACLE_BEST_SHARED = (7, 354.046)  # best shared candidate and its fleet log-likelihood
ORACLE_SUM_OF_MAXIMA = 605.866


def mixed_fleet():
    from track_estimators import synthetic

    sb = synthetic.make_batch(16, nobs=26, gap_h=1.0, seed0=100)
    z = np.array(sb.z, dtype=np.float64)
    extra = np.random.default_rng(7).normal(0, np.sqrt(0.2 ** 2 - 0.05 ** 2), z[1::2, 0:2, :].shape)
    z[1::2, 0:2, :] += extra
    return dataclasses.replace(sb, z=z)


def _tri(M):
    return np.asarray(M)[np.triu_indices(4)]


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for proto in (r"int ste_ukf_forward_noise_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_noise_f64\* nz, "
                  r"const ste_ukf_loglik_f64\* l, void\* stream\);",
                  r"int ste_urtss_backward_noise_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_noise_f64\* nz, void\* stream\);",
                  r"int ste_ukf_urtss_noise_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_noise_f64\* nz, void\* stream\);"):
        assert re.search("^" + proto, hdr, flags=re.M), proto
    body = hdr[hdr.index("typedef struct ste_ukf_noise_f64 {"): hdr.index("} ste_ukf_noise_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double|size_t|void)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteUkfNoiseF64._fields_] == ["Q", "R", "flags", "reserved"]
    assert C.sizeof(binding.SteUkfNoiseF64) == 24
    assert re.search(r"#define STE_NOISE_R_BLOCK2 0x1u", hdr) and binding.STE_NOISE_R_BLOCK2 == 1
    for name in ("ste_ukf_forward_noise_f64", "ste_urtss_backward_noise_f64", "ste_ukf_urtss_noise_f64"):
        assert name in binding.SYMBOLS
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the per-track matrices travel beside the batch


def test_refusals_before_any_launch():
    """Every refusal of the header returns STE_EINVAL (-1) with its reason; a launch on a machine without a GPU would return
    STE_ELAUNCH (-2), so -1 shows the call stopped before launching (the pattern of tests/test_ukf_loglik.py)."""
    from track_estimators._hip import binding

    lib, keep = binding.load(), []
    nz = binding.SteUkfNoiseF64(0x4000, 0x5000, binding.STE_NOISE_R_BLOCK2, 0)
    lk = binding.SteUkfLoglikF64(0x2000, 0x2000, 0x2000, None)
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    calls = {
        "ste_ukf_forward_noise_f64": lambda s, n, l=None: lib.ste_ukf_forward_noise_f64(ref(s), ref(n), ref(l), None),
        "ste_urtss_backward_noise_f64": lambda s, n, l=None: lib.ste_urtss_backward_noise_f64(ref(s), ref(n), None),
        "ste_ukf_urtss_noise_f64": lambda s, n, l=None: lib.ste_ukf_urtss_noise_f64(ref(s), ref(n), None),
    }

    def smoothed(s):
        s.sm_mean = s.sm_cov = 0x6000
        return s

    for name, call in calls.items():
        def err(s, n, l=None):
            return call(s, n, l), lib.ste_last_error().decode()

        rc, msg = err(None, nz)
        assert rc == -1 and "batch pointer is NULL" in msg, name
        rc, msg = err(smoothed(_batch(binding, keep)), None)
        assert rc == -1 and "per-track noise (nz) is NULL" in msg and name in msg
        rc, msg = err(smoothed(_batch(binding, keep)), binding.SteUkfNoiseF64(None, None, 0, 0))
        assert rc == -1 and "both NULL" in msg and "plain call" in msg and name in msg
        s = smoothed(_batch(binding, keep))
        s.flags = binding.STE_FLAG_LANES_4
        rc, msg = err(s, nz)
        assert rc == -1 and "STE_FLAG_LANES_4" in msg and "quad forward kernel" in msg
        rc, msg = err(smoothed(_batch(binding, keep)), binding.SteUkfNoiseF64(0x4000, None, 0x2, 0))
        assert rc == -1 and "unknown bits in nz->flags" in msg
        # whatever the plain call refuses
        s = smoothed(_batch(binding, keep))
        s.n = 3
        rc, msg = err(s, nz)
        assert rc == -1 and "state dimension" in msg
        s = smoothed(_batch(binding, keep))
        s.track_stride = 4
        rc, msg = err(s, nz)
        assert rc == -1 and "track_stride" in msg
        s = smoothed(_batch(binding, keep))
        s.status = None
        rc, msg = err(s, nz)
        assert rc == -1 and "status" in msg
    # the smoother's outputs
    for name in ("ste_urtss_backward_noise_f64", "ste_ukf_urtss_noise_f64"):
        rc = calls[name](_batch(binding, keep), nz)
        assert rc == -1 and "sm_mean and sm_cov are required" in lib.ste_last_error().decode()
    # time slices: misaligned ones are refused as in the plain call; with the likelihood every slice is
    fwd = calls["ste_ukf_forward_noise_f64"]
    s = _batch(binding, keep)
    s.step_begin, s.step_end = 32, 128
    assert fwd(s, nz) == -1 and "multiples of STE_SLICE_ALIGN" in lib.ste_last_error().decode()
    for b, e in ((64, 0), (0, 128), (64, 256)):
        s = _batch(binding, keep)
        s.step_begin, s.step_end = b, e
        assert fwd(s, nz, lk) == -1 and "time slices" in lib.ste_last_error().decode(), (b, e)
    s = smoothed(_batch(binding, keep))
    s.step_begin, s.step_end = 64, 128
    assert calls["ste_ukf_urtss_noise_f64"](s, nz) == -1 and "whole passes" in lib.ste_last_error().decode()
    # the likelihood's own checks
    assert fwd(_batch(binding, keep), nz, binding.SteUkfLoglikF64(None, 0x2000, 0x2000, 0x2000)) == -1
    assert "l->loglik is required" in lib.ste_last_error().decode()
    for name in ("fwd_mean", "fwd_cov"):
        s = _batch(binding, keep)
        setattr(s, name, None)
        assert fwd(s, nz, lk) == -1 and "both (histories) or neither" in lib.ste_last_error().decode(), name
    s = _batch(binding, keep)
    s.fwd_mean = s.fwd_cov = None
    s.rts_work = 0x3000
    assert fwd(s, nz, lk) == -1 and "rts_work needs the histories" in lib.ste_last_error().decode()
    s = _batch(binding, keep)
    s.fwd_mean = None  # without the likelihood the histories are required
    assert fwd(s, nz) == -1 and "fwd_mean, fwd_cov and status are required" in lib.ste_last_error().decode()


def _ragged_tracks(n=7):
    """n small synthetic tracks with different numbers of observations, as pack_tracks takes them."""
    import types

    from track_estimators import synthetic

    tracks, dts, x0s = [], [], []
    for b in range(n):
        sb = synthetic.make_batch(1, nobs=5 + (b * 3) % 7, gap_h=1.0, seed0=50 + b)
        tracks.append(types.SimpleNamespace(z=sb.z[0], dts=sb.dts[0], sog_rate=sb.sog_rate[0], cog_rate=sb.cog_rate[0]))
        dts.append(np.repeat(sb.dts[0] / 2, 2))
        x0s.append(sb.z[0][:, 0])
    return tracks, dts, x0s


def test_packing_of_stacks():
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    tracks, dts, x0s = _ragged_tracks()
    B = len(tracks)
    Qs = np.stack([Q * (1.0 + b) for b in range(B)])
    Rs = np.stack([R * (2.0 + b) for b in range(B)])
    Rs[:, 0, 1] = Rs[:, 1, 0] = 0.01 * np.arange(B)
    plain = batch.pack_tracks(tracks, dts, x0s, H, Q, R, P0)
    assert plain.Q_tracks is None and plain.R_tracks is None and not plain.track_noise
    hb = batch.pack_tracks(tracks, dts, x0s, H, Qs, list(Rs), P0)  # a stack and a sequence of matrices
    assert hb.order is not None and sorted(hb.order.tolist()) == list(range(B)) and hb.order.tolist() != list(range(B))
    assert hb.Q_tracks.shape == hb.R_tracks.shape == (10, B) and hb.Q_tracks.dtype == np.float64 and hb.track_noise
    assert hb.Q_tracks.flags.c_contiguous and hb.R_tracks.flags.c_contiguous
    for s in range(B):  # the triangle in slot s is that of the caller's track order[s]
        assert np.array_equal(hb.Q_tracks[:, s], _tri(Qs[hb.order[s]]))
        assert np.array_equal(hb.R_tracks[:, s], _tri(Rs[hb.order[s]]))
    assert hb.Q.shape == hb.R.shape == (4, 4)
    # without bucketing: slot order is the caller's
    hb2 = batch.pack_tracks(tracks, dts, x0s, H, Qs, R, P0, bucket_by_length=False)
    assert hb2.order is None and hb2.R_tracks is None and np.array_equal(hb2.R, R)
    assert np.array_equal(hb2.Q_tracks, np.stack([_tri(q) for q in Qs], axis=1))
    # one matrix each: field by field what it is without this feature
    again = batch.pack_tracks(tracks, dts, x0s, H, Q.copy(), R.copy(), P0)
    for f in dataclasses.fields(batch.HostBatch):
        a, b = getattr(plain, f.name), getattr(again, f.name)
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) or a is None else a == b, f.name
    assert [f.name for f in dataclasses.fields(batch.HostBatch)][-2:] == ["Q_tracks", "R_tracks"]
    # refusals: an asymmetric matrix in the stack (the message names it), wrong length, wrong shape
    bad = Qs.copy()
    bad[3, 0, 1] = 0.5
    with pytest.raises(ValueError, match=r"Q\[3\] must be symmetric"):
        batch.pack_tracks(tracks, dts, x0s, H, bad, R, P0)
    with pytest.raises(ValueError, match=r"R must be one 4x4 matrix or a stack"):
        batch.pack_tracks(tracks, dts, x0s, H, Q, Rs[:-1], P0)
    with pytest.raises(ValueError, match=r"Q must be one 4x4 matrix or a stack"):
        batch.pack_tracks(tracks, dts, x0s, H, np.zeros((B, 3, 3)), R, P0)
    with pytest.raises(ValueError, match="Q must be 4x4"):
        batch.pack_tracks(tracks, dts, x0s, H, np.eye(3), R, P0)
    # pack_uniform
    sb = synthetic.make_batch(5, nobs=6, seed0=3)
    hu = batch.pack_uniform(sb, 2, H, Qs[:5], Rs[:5], P0)
    assert np.array_equal(hu.Q_tracks, np.stack([_tri(q) for q in Qs[:5]], axis=1))
    assert np.array_equal(hu.R_tracks, np.stack([_tri(r) for r in Rs[:5]], axis=1))
    pu, pa = batch.pack_uniform(sb, 2, H, Q, R, P0), batch.pack_uniform(sb, 2, H, Q, R, P0)
    assert pu.Q_tracks is None and pu.R_tracks is None and np.array_equal(pu.Q, pa.Q)
    with pytest.raises(ValueError, match=r"R\[1\] must be symmetric"):
        bad = Rs[:5].copy()
        bad[1, 2, 3] = 1.0
        batch.pack_uniform(sb, 2, H, Q, bad, P0)
    with pytest.raises(ValueError, match="stack of one per track"):
        batch.pack_uniform(sb, 2, H, Qs[:4], R, P0)


def test_with_track_noise_and_apply_noise_choice():
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(6, nobs=6, seed0=3)
    hb = batch.pack_uniform(sb, 2, H, Q, R, P0)
    cands = [(Q, np.diag([0.01, 0.01, 0.0, 0.0])), (Q * 2.0, np.diag([0.04, 0.04, 0.0, 0.0])), (Q * 3.0, GENERAL_R)]
    choice = batch.NoiseChoice(index=np.array([0, 1, -1, 1, 0, 0]), loglik=np.zeros(6), excluded=1)
    out = batch.apply_noise_choice(hb, cands, choice)
    assert out is not hb and out.z is hb.z and hb.Q_tracks is None  # a copy, arrays shared, hb untouched
    want = [cands[0], cands[1], (hb.Q, hb.R), cands[1], cands[0], cands[0]]  # -1 keeps the shared pair
    for b, (q, r) in enumerate(want):
        assert np.array_equal(out.Q_tracks[:, b], _tri(q)) and np.array_equal(out.R_tracks[:, b], _tri(r)), b
    # R_BLOCK2: every R of that stack is confined to the leading block (the shipped R of track 2 too); one general R in a
    # stack takes the promise away
    assert batch.r_tracks_block2(out.R_tracks)
    blk = batch.apply_noise_choice(hb, cands, batch.NoiseChoice(index=np.array([0, 1, 0, 1, 0, 0]), loglik=None, excluded=0))
    assert batch.r_tracks_block2(blk.R_tracks)
    one = batch.apply_noise_choice(hb, cands, batch.NoiseChoice(index=np.array([0, 1, 0, 2, 0, 0]), loglik=None, excluded=0))
    assert not batch.r_tracks_block2(one.R_tracks)
    with pytest.raises(ValueError, match="one candidate index per track"):
        batch.apply_noise_choice(hb, cands, batch.NoiseChoice(index=1, loglik=None, excluded=0))
    with pytest.raises(ValueError, match="out of range"):
        batch.apply_noise_choice(hb, cands, batch.NoiseChoice(index=np.array([0, 1, 0, 3, 0, 0]), loglik=None, excluded=0))
    # a batch that already carries stacks: -1 keeps the track's own pair, not the shared one
    again = batch.apply_noise_choice(out, cands, batch.NoiseChoice(index=np.array([-1, -1, 2, 0, -1, 1]), loglik=None, excluded=0))
    want = [cands[0], cands[1], cands[2], cands[0], cands[0], cands[1]]
    for b, (q, r) in enumerate(want):
        assert np.array_equal(again.Q_tracks[:, b], _tri(q)) and np.array_equal(again.R_tracks[:, b], _tri(r)), b
    tq, tr = batch.track_matrices(out)
    assert tq.shape == tr.shape == (6, 4, 4) and np.array_equal(tq[1], cands[1][0]) and np.array_equal(tr[2], hb.R)
    assert np.array_equal(tq, np.swapaxes(tq, 1, 2))
    sq, sr = batch.track_matrices(hb)
    assert np.array_equal(sq[5], hb.Q) and np.array_equal(sr[0], hb.R)
    gq, gr = batch.track_matrices(one)
    assert np.array_equal(gr[3], GENERAL_R) and np.array_equal(gq[3], cands[2][0])
    # with_track_noise: slot order, one of the two may stay shared, shapes are checked
    Qs = np.stack([Q * (1 + b) for b in range(6)])
    w = batch.with_track_noise(hb, Q=Qs)
    assert w.R_tracks is None and np.array_equal(w.Q_tracks, np.stack([_tri(q) for q in Qs], axis=1))
    w2 = batch.with_track_noise(w, R=np.stack([R] * 6))
    assert np.array_equal(w2.Q_tracks, w.Q_tracks) and w2.R_tracks.shape == (10, 6)
    with pytest.raises(ValueError, match="stack of one 4x4 matrix per track"):
        batch.with_track_noise(hb, Q=Q)
    with pytest.raises(ValueError, match=r"R\[2\] must be symmetric"):
        bad = np.stack([R] * 6)
        bad[2, 0, 3] = 1.0
        batch.with_track_noise(hb, R=bad)


def _oracle_grid(sb):
    from track_estimators import synthetic

    H, _, _, P0 = synthetic.example_matrices()
    return np.array([[t["loglik"] for t in fleet_restatement(sb, FLEET_SUBSTEPS, H, Qc, Rc, P0)]
                     for Qc, Rc in fleet_candidates()])


def test_oracle_separates_the_two_populations_of_the_mixed_fleet():
    """The yardstick of the end-to-end GPU test: on the mixed fleet the oracle's per-track argmax over the nine-point R grid
    separates the clean and the noisy tracks, and choosing per track is worth about 250 nats over the best shared choice."""
    ll = _oracle_grid(mixed_fleet())
    assert np.all(np.isfinite(ll))
    assert np.argmax(ll, axis=0).tolist() == ORACLE_ARGMAX
    sums = ll.sum(axis=1)
    assert int(np.argmax(sums)) == ORACLE_BEST_SHARED[0]
    assert abs(sums.max() - ORACLE_BEST_SHARED[1]) < 1e-3
    assert abs(ll.max(axis=0).sum() - ORACLE_SUM_OF_MAXIMA) < 1e-3
    srt = np.sort(ll, axis=0)
    assert abs((srt[-1] - srt[-2]).min() - 0.0995) < 1e-3  # smallest gap between a track's best and second-best candidate


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _candidates(route):
    """Three exactly symmetric (Q, R) pairs that all take ``route``."""
    from track_estimators import synthetic

    _, Q, _, _ = synthetic.example_matrices()
    Q2 = Q * 2.0
    Q2[0, 1] = Q2[1, 0] = 2e-5
    Q2[0, 2] = Q2[2, 0] = 1e-6
    Q2[1, 3] = Q2[3, 1] = -2e-6
    Q3 = Q * 0.5
    Q3[2, 3] = Q3[3, 2] = 1e-7
    if route == "general":
        R2 = GENERAL_R * 2.0
        R3 = GENERAL_R.copy()
        R3[0, 1] = R3[1, 0] = -0.0006
        R3[2, 3] = R3[3, 2] = 0.01
        Rs = [GENERAL_R, R2, R3]
    else:
        R2 = np.diag([0.01, 0.02, 0.0, 0.0])
        R2[0, 1] = R2[1, 0] = 0.003
        Rs = [np.diag([0.0025, 0.0025, 0.0, 0.0]), R2, np.diag([0.04, 0.04, 0.0, 0.0])]
    cands = list(zip([Q, Q2, Q3], Rs))
    for q, r in cands:
        assert np.array_equal(q, q.T) and np.array_equal(r, r.T)
    return cands


def _ragged_hb(ntracks=192, seed0=3, nobs=26, robust=False):
    hb = _synthetic_hb(ntracks, seed0, nobs=nobs, robust=robust)
    nsteps = (hb.Nmax - (np.arange(ntracks) * 7) % 40).astype(np.int32)
    return dataclasses.replace(hb, nsteps=nsteps, lanes=1)


def _stacks(cands, assign):
    return np.stack([cands[k][0] for k in assign]), np.stack([cands[k][1] for k in assign])


def _run_all(hb, lik=True, **kw):
    """Forward pass with the likelihood, then the smoother; every output as NumPy arrays, track index last."""
    from track_estimators import batch

    db = batch.DeviceBatch(hb, **kw)
    for t in (db.fwd_mean, db.fwd_cov, db.sm_mean, db.sm_cov, db.rts_work):
        if t is not None:
            t.zero_()
    out = {}
    if lik:
        res = db.log_likelihood(nis=True)
        out.update(loglik=res.loglik, dof=res.dof, nupd=res.nupd, nis=res.nis.T)
    else:
        db.forward()
    out["status_fwd"] = db.status.cpu().numpy().copy()
    db.backward()
    db.torch.cuda.synchronize()
    for name in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "status"):
        out[name] = getattr(db, name).cpu().numpy()
    return out


_F64 = ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "loglik", "nis")
_I32 = ("status", "status_fwd", "dof", "nupd")


def _assert_tracks_equal(per, shared, assign, nsteps=None, names=_F64 + _I32):
    """Track b of ``per`` equals track b of ``shared[assign[b]]`` bit for bit (rows past a track's end are not compared:
    nothing writes them)."""
    B = len(assign)
    for name in names:
        if name not in per:
            continue
        for b in range(B):
            a, r = per[name][..., b], shared[assign[b]][name][..., b]
            if nsteps is not None and a.ndim >= 1 and name not in ("loglik",):
                a, r = a[: nsteps[b] + 1], r[: nsteps[b] + 1]
            if name in _F64:
                assert np.array_equal(_u64(a), _u64(r)), (name, b, assign[b])
            else:
                assert np.array_equal(a, r), (name, b, assign[b])


def _assert_candidates_differ(shared, nsteps):
    """Two tracks with different candidates do differ: the comparison above cannot pass vacuously."""
    n = int(nsteps[0])
    for name in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov"):
        assert not np.array_equal(shared[0][name][: n + 1, ..., 0], shared[1][name][: n + 1, ..., 0]), name
        assert not np.array_equal(shared[1][name][: n + 1, ..., 0], shared[2][name][: n + 1, ..., 0]), name
    if "loglik" in shared[0]:
        assert shared[0]["loglik"][0] != shared[1]["loglik"][0] != shared[2]["loglik"][0]


SMOOTHERS = {"standalone": dict(fuse_gains=False), "one-kernel": dict(tuning=0x400), "two-kernel-quad": dict(tuning=0x200),
             "two-kernel-lane": dict(tuning=0x200 | 0x800)}


@pytest.mark.gpu
@pytest.mark.parametrize("smoother", list(SMOOTHERS))
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "full"])
@pytest.mark.parametrize("route", ["closed", "robust", "general"])
def test_bit_identical_to_shared_launches(route, packed, smoother):
    """192 ragged tracks (three tiles), track b with candidate b % 3: histories, smoothed histories, status and the
    likelihood's outputs of every track are those of the shared run of its candidate, bit for bit."""
    from track_estimators import batch

    cands = _candidates(route)
    hb = _ragged_hb(robust=route == "robust")
    assign = np.arange(hb.B) % 3
    kw = dict(packed_cov=packed, **SMOOTHERS[smoother])
    shared = [_run_all(dataclasses.replace(hb, Q=q, R=r), **kw) for q, r in cands]
    hbt = batch.with_track_noise(hb, *_stacks(cands, assign))
    assert batch.r_tracks_block2(hbt.R_tracks) == (route != "general")
    per = _run_all(hbt, **kw)
    _assert_tracks_equal(per, shared, assign, hb.nsteps)
    _assert_candidates_differ(shared, hb.nsteps)
    assert np.all(np.isfinite(per["loglik"]))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["closed", "general"])
def test_bit_identical_with_non_finite_observations(route):
    """A NaN speed or course in one observation makes a track's state, and every later S, non-finite.  Such a track takes
    the route its shared launch takes (no 2 x 2 shortcut for a non-finite S on the general route), so its status bits and
    likelihood counts are the shared launch's too."""
    from track_estimators import batch
    from track_estimators._hip import binding

    cands = _candidates(route)
    hb = _ragged_hb()
    z = hb.z.copy()
    poisoned = {5: (10, 2), 6: (10, 3), 7: (3, 2), 70: (14, 3), 71: (9, 2), 72: (1, 3), 190: (12, 2)}  # track: (observation column, component), every column inside the shortest track
    for b, (col, comp) in poisoned.items():
        z[col, comp, b] = np.nan
    hb = dataclasses.replace(hb, z=z)
    assign = np.arange(hb.B) % 3
    for kw in (dict(tuning=0x400), dict(fuse_gains=False)):
        shared = [_run_all(dataclasses.replace(hb, Q=q, R=r), **kw) for q, r in cands]
        per = _run_all(batch.with_track_noise(hb, *_stacks(cands, assign)), **kw)
        _assert_tracks_equal(per, shared, assign, hb.nsteps)
        for b in range(hb.B):
            assert bool(per["status_fwd"][b] & binding.STE_STATUS_NAN) == (b in poisoned), b
            assert np.isnan(per["loglik"][b]) == (b in poisoned), b


@pytest.mark.gpu
def test_bit_identical_with_recorded_noise():
    from track_estimators import batch, synthetic

    cands = _candidates("closed")
    hb = _ragged_hb()
    B, N = hb.B, hb.Nmax
    _, Q, R, _ = synthetic.example_matrices()
    npred, nupd, nrts = np.zeros((N, 4, B)), np.zeros((N + 1, 4, B)), np.zeros((N, 4, B))
    np.random.seed(11)
    for b in range(B):
        dts = np.full(N // 4, 1.0)
        d = batch.draw_reference_noise(Q * 1e-2, np.diag([1e-4, 1e-4, 1e-2, 1e-2]), np.asarray(hb.dt[:, b]), dts)
        npred[:, :, b], nupd[:, :, b], nrts[:, :, b] = d["noise_pred"], d["noise_upd"], d["noise_rts"]
    hb = dataclasses.replace(hb, noise_pred=npred, noise_upd=nupd, noise_rts=nrts)
    assign = np.arange(B) % 3
    for kw in (dict(tuning=0x400), dict(fuse_gains=False)):
        shared = [_run_all(dataclasses.replace(hb, Q=q, R=r), **kw) for q, r in cands]
        per = _run_all(batch.with_track_noise(hb, *_stacks(cands, assign)), **kw)
        _assert_tracks_equal(per, shared, assign, hb.nsteps)
        _assert_candidates_differ(shared, hb.nsteps)


@pytest.mark.gpu
def test_bit_identical_with_smoother_rates_of_their_own():
    from track_estimators import batch

    cands = _candidates("closed")
    hb = _ragged_hb()
    hb = dataclasses.replace(hb, sog_rate_rts=hb.sog_rate * 1.25 + 0.01, cog_rate_rts=hb.cog_rate * 0.75 - 0.02)
    assign = np.arange(hb.B) % 3
    for kw in (dict(tuning=0x400), dict(tuning=0x200), dict(fuse_gains=False)):
        shared = [_run_all(dataclasses.replace(hb, Q=q, R=r), **kw) for q, r in cands]
        per = _run_all(batch.with_track_noise(hb, *_stacks(cands, assign)), **kw)
        _assert_tracks_equal(per, shared, assign, hb.nsteps)
        _assert_candidates_differ(shared, hb.nsteps)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["Q", "R"])
def test_bit_identical_with_one_of_the_two_stacked(which):
    """Q stacked with R shared, and R stacked with Q shared: the NULL member falls back on the batch's shared matrix."""
    from track_estimators import batch

    cands = _candidates("closed")
    hb = _ragged_hb()
    assign = np.arange(hb.B) % 3
    Qs, Rs = _stacks(cands, assign)
    q0, r0 = cands[1]
    if which == "Q":
        shared = [_run_all(dataclasses.replace(hb, Q=q, R=r0), tuning=0x400) for q, _ in cands]
        hbt = batch.with_track_noise(dataclasses.replace(hb, R=r0), Q=Qs)
        assert hbt.R_tracks is None
    else:
        shared = [_run_all(dataclasses.replace(hb, Q=q0, R=r), tuning=0x400) for _, r in cands]
        hbt = batch.with_track_noise(dataclasses.replace(hb, Q=q0), R=Rs)
        assert hbt.Q_tracks is None
    per = _run_all(hbt, tuning=0x400)
    _assert_tracks_equal(per, shared, assign, hb.nsteps)
    assert not np.array_equal(shared[0]["sm_mean"][..., 0], shared[2]["sm_mean"][..., 0])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["closed", "general"])
def test_likelihood_without_histories_bit_identical(route):
    from track_estimators import batch

    cands = _candidates(route)
    hb = _ragged_hb()
    assign = np.arange(hb.B) % 3
    grid = batch.log_likelihood_grid(hb, cands, nis=True)  # the shared likelihood-only launches
    hbt = batch.with_track_noise(hb, *_stacks(cands, assign))
    res = batch.DeviceBatch(hbt, histories=False).log_likelihood(nis=True)
    for b in range(hb.B):
        k, n = assign[b], hb.nsteps[b]
        assert _u64(res.loglik[b: b + 1])[0] == _u64(grid.loglik[k, b: b + 1])[0], b
        assert np.array_equal(_u64(res.nis[b, : n + 1]), _u64(grid.nis[k, b, : n + 1])), b
        assert res.dof[b] == grid.dof[k, b] and res.nupd[b] == grid.nupd[k, b] and res.status[b] == grid.status[k, b]
    assert grid.loglik[0, 0] != grid.loglik[1, 0]


@pytest.mark.gpu
def test_forward_in_three_time_slices_bit_identical():
    from track_estimators import batch

    cands = _candidates("closed")
    hb = _ragged_hb(nobs=36)  # 140 steps: slices [0, 64), [64, 128), [128, 140)
    assert len(batch.DeviceBatch.slice_bounds(hb.Nmax, 3)) == 3
    assign = np.arange(hb.B) % 3
    hbt = batch.with_track_noise(hb, *_stacks(cands, assign))
    outs = []
    for slices in (1, 3):
        db = batch.DeviceBatch(hbt, tuning=0x400)
        for t in (db.fwd_mean, db.fwd_cov, db.rts_work):
            t.zero_()
        db.forward(slices=slices)
        db.backward()
        outs.append({n: getattr(db, n).cpu().numpy() for n in ("fwd_mean", "fwd_cov", "rts_work", "sm_mean", "sm_cov", "status")})
    for name in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov"):
        for b in range(hb.B):
            n = hb.nsteps[b]
            assert np.array_equal(_u64(outs[0][name][: n + 1, :, b]), _u64(outs[1][name][: n + 1, :, b])), (name, b)
    assert np.array_equal(outs[0]["status"], outs[1]["status"])
    shared = [_run_all(dataclasses.replace(hb, Q=q, R=r), lik=False, tuning=0x400) for q, r in cands]
    _assert_tracks_equal(outs[1], shared, assign, hb.nsteps, names=("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "status"))


@pytest.mark.gpu
def test_oracle_parity_on_the_mixed_fleet():
    """Per-track (Q, R) on the mixed fleet -- R from the oracle's argmax list, Q scaled by 1 + 0.25 (b % 3) -- against the
    per-track oracle: filtered and smoothed histories at test_hip_parity's tolerances, the likelihood at LIK_RTOL."""
    from oracle import ukf_oracle as orc
    from track_estimators import batch, synthetic

    H, Q, _, P0 = synthetic.example_matrices()
    sb = mixed_fleet()
    cands = fleet_candidates()
    B = sb.z.shape[0]
    Qs = np.stack([Q * (1.0 + 0.25 * (b % 3)) for b in range(B)])
    Rs = np.stack([cands[k][1] for k in ORACLE_ARGMAX])
    hb = batch.pack_uniform(sb, FLEET_SUBSTEPS, H, Qs, Rs, P0)
    db = batch.DeviceBatch(dataclasses.replace(hb, lanes=1))
    res = db.log_likelihood(nis=True)
    db.backward()
    d = db.download()
    assert not db.status_host().any()
    N = hb.Nmax
    worst = [0.0] * 5
    for b in range(B):
        dt = np.repeat(sb.dts[b] / FLEET_SUBSTEPS, FLEET_SUBSTEPS)
        m, P = orc.forward_track(sb.z[b][:, 0], P0, H, Qs[b], Rs[b], dt, sb.dts[b], sb.z[b], sb.sog_rate[b], sb.cog_rate[b])
        sm, sP = orc.backward_track(m, P, Qs[b], dt, len(sb.dts[b]), sb.sog_rate[b], sb.cog_rate[b])
        errs = (mean_err(d["means"][b], m), cov_err(d["covs"][b], P), mean_err(d["means_smoothed"][b], sm),
                cov_err(d["covs_smoothed"][b], sP))
        print(f"[track-noise] oracle parity track {b}: mean {errs[0]:.2e} cov {errs[1]:.2e} sm mean {errs[2]:.2e} sm cov {errs[3]:.2e}")
        assert errs[0] < MEAN_TOL and errs[2] < MEAN_TOL and errs[1] < COV_TOL and errs[3] < COV_TOL, (b, errs)
        ref = restate_track(sb.z[b][:, 0], P0, H, Qs[b], Rs[b], dt, sb.dts[b], sb.z[b], sb.sog_rate[b], sb.cog_rate[b])
        lerr = _check_track(res, b, ref, N, d["means"])
        worst = [max(w, e) for w, e in zip(worst, errs + (lerr[0],))]
    print(f"[track-noise] oracle parity worst: mean {worst[0]:.2e} cov {worst[1]:.2e} sm mean {worst[2]:.2e} sm cov {worst[3]:.2e} "
          f"loglik {worst[4]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["closed", "general"])
def test_one_track_alone_equals_slot_517_of_1000(route):
    """(general: the route on which the pseudo-inverse's 2 x 2 shortcut is decided per lane; the neighbours of slot 517 carry
    the other two general matrices.)"""
    from track_estimators import batch

    j = 517
    cands = _candidates(route)
    big = dataclasses.replace(_synthetic_hb(1000, 7), lanes=1)
    one = dataclasses.replace(_synthetic_hb(1, 7 + j), lanes=1)
    assign = (np.arange(1000) * 5 + 1) % 3
    big = batch.with_track_noise(big, *_stacks(cands, assign))
    one = batch.with_track_noise(one, *_stacks(cands, assign[j: j + 1]))
    for kw in (dict(tuning=0x400), dict(tuning=0x200), dict(fuse_gains=False)):
        a, b = _run_all(big, **kw), _run_all(one, **kw)
        for name in _F64:
            assert np.array_equal(_u64(a[name][..., j]), _u64(b[name][..., 0])), (name, kw)
        for name in _I32:
            assert a[name][j] == b[name][0], (name, kw)


@pytest.mark.gpu
def test_window_of_a_resident_batch_equals_a_batch_of_its_own():
    from track_estimators import batch

    cands = _candidates("closed")
    assign = (np.arange(256) * 7 + 2) % 3
    fleet_hb = batch.with_track_noise(dataclasses.replace(_synthetic_hb(256, 40), lanes=1), *_stacks(cands, assign))
    own_hb = batch.with_track_noise(dataclasses.replace(_synthetic_hb(128, 40 + 64), lanes=1), *_stacks(cands, assign[64:192]))
    fleet, own = batch.DeviceBatch(fleet_hb), batch.DeviceBatch(own_hb)
    for t in (fleet.fwd_mean, fleet.sm_mean, fleet.fwd_cov, fleet.sm_cov):
        t.fill_(-7.0)
    w = fleet.window(64, 192)
    lw, lo = w.log_likelihood(nis=True), own.log_likelihood(nis=True)
    w.backward()
    own.backward()
    for f in ("loglik", "nis"):
        assert np.array_equal(_u64(getattr(lw, f)), _u64(getattr(lo, f))), f
    for f in ("dof", "nupd", "status"):
        assert np.array_equal(getattr(lw, f), getattr(lo, f)), f
    for name in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "status"):
        full = getattr(fleet, name).cpu().numpy()
        assert np.array_equal(full[..., 64:192].view(np.uint8) if name == "status" else _u64(full[..., 64:192]),
                              getattr(own, name).cpu().numpy().view(np.uint8) if name == "status"
                              else _u64(getattr(own, name).cpu().numpy())), name
    # the window touched its own columns only
    assert np.all(fleet.fwd_mean.cpu().numpy()[..., :64] == -7.0) and np.all(fleet.sm_mean.cpu().numpy()[..., 192:] == -7.0)
    # run(): forward + smoother in one call on the window
    w.run()
    own.run()
    for name in ("fwd_mean", "sm_mean", "sm_cov"):
        assert np.array_equal(_u64(getattr(fleet, name).cpu().numpy()[..., 64:192]), _u64(getattr(own, name).cpu().numpy())), name


@pytest.mark.gpu
def test_run_fleet_equals_run_batch():
    from track_estimators import batch

    cands = _candidates("closed")
    hb = _ragged_hb()
    assign = (np.arange(hb.B) * 5 + 1) % 3
    hbt = batch.with_track_noise(hb, *_stacks(cands, assign))
    assert len(batch.fleet_windows(hbt.B, 64)) == 3
    ref = batch.run_batch(hbt)
    names = ("means", "covs", "means_smoothed", "covs_smoothed")

    def same(out):
        for name in names:
            for b in range(hbt.B):
                n = hbt.nsteps[b]
                assert np.array_equal(_u64(out[name][b, : n + 1]), _u64(ref[name][b, : n + 1])), (name, b)
        assert np.array_equal(out["status"], ref["status"])

    same(batch.run_fleet(hbt, chunk=64))  # from the host: the triangles come up window by window
    db = batch.DeviceBatch(hbt)
    for t in (db.fwd_mean, db.fwd_cov, db.sm_mean, db.sm_cov):
        t.zero_()
    same(batch.run_fleet(db, chunk=64, outputs=names))  # resident, scheduled=None: per-window launches for this fleet
    with pytest.raises(ValueError, match="per-track noise"):
        batch.run_fleet(db, chunk=64, scheduled=True)
    with batch.SmootherPipeline(db.device, ntracks=64, sequence_only=True) as pipe:
        with pytest.raises(ValueError, match="per-track noise"):
            pipe.submit_sequence([db.window(lo, hi) for lo, hi in batch.fleet_windows(hbt.B, 64)])
    # the shared runs agree with what the fleet computed (the comparison above is not between two wrong answers)
    shared = [batch.run_batch(dataclasses.replace(hb, Q=q, R=r)) for q, r in cands]
    for b in range(hbt.B):
        n = hbt.nsteps[b]
        assert np.array_equal(_u64(ref["means_smoothed"][b, : n + 1]), _u64(shared[assign[b]]["means_smoothed"][b, : n + 1])), b
    with pytest.raises(ValueError, match="lanes=4"):
        batch.DeviceBatch(dataclasses.replace(hbt, lanes=4))
    # a quad pipeline and a batch that names no mapping: refused in Python, before the library has to
    auto = batch.DeviceBatch(dataclasses.replace(hbt, lanes=0))
    with batch.SmootherPipeline(db.device, ntracks=hbt.B, forward_lanes=4, forward_streams=1, smoother_streams=1) as pipe:
        with pytest.raises(ValueError, match="forward_lanes=4"):
            pipe.submit(auto)


@pytest.mark.gpu
def test_end_to_end_grid_choice_apply():
    """mixed fleet -> log_likelihood_grid -> best_noise(per_track=True) -> apply_noise_choice -> log_likelihood / run_batch."""
    from track_estimators import batch, synthetic

    H, _, _, P0 = synthetic.example_matrices()
    sb = mixed_fleet()
    cands = fleet_candidates()
    hb = batch.pack_uniform(sb, FLEET_SUBSTEPS, H, cands[0][0], cands[0][1], P0)
    grid = batch.log_likelihood_grid(hb, cands)
    choice = batch.best_noise(grid, per_track=True)
    assert choice.excluded == 0
    # the smallest gap between a track's best and second-best candidate is the oracle's 0.0995 nats on the device too: the
    # values that compete for a track's argmax are a few tens of nats, LIK_RTOL of which is four orders below that gap, so
    # rounding cannot flip the choice (the grid's largest |loglik|, ~2 600 nats, belongs to candidates far from any maximum)
    srt = np.sort(grid.loglik, axis=0)
    assert abs(float((srt[-1] - srt[-2]).min()) - 0.0995) < 1e-3
    assert float(np.abs(srt[-2:]).max()) * LIK_RTOL < 0.0995e-2
    assert choice.index.tolist() == ORACLE_ARGMAX
    hbt = batch.apply_noise_choice(hb, cands, choice)
    res = batch.DeviceBatch(hbt).log_likelihood()
    for b in range(hb.B):
        assert _u64(res.loglik[b: b + 1])[0] == _u64(grid.loglik[choice.index[b], b: b + 1])[0], b
    fleet = batch.best_noise(grid)
    assert fleet.index == ORACLE_BEST_SHARED[0]
    print(f"[track-noise] end to end: per-track sum {res.loglik.sum():.6f} (oracle {ORACLE_SUM_OF_MAXIMA}), best shared "
          f"{fleet.loglik[fleet.index]:.6f} (oracle {ORACLE_BEST_SHARED[1]})")
    assert res.loglik.sum() > fleet.loglik[fleet.index]
    # Against the oracle within LIK_RTOL, on the project's scale for it (tests/test_ukf_loglik.py): relative to sum |l_u| of
    # the values compared.  The oracle's sums are restated here, so nothing hangs on the three decimals they are quoted
    # to; that the restated sums are the quoted 605.866 / 354.046 is asserted beside it.
    refs = {k: fleet_restatement(sb, FLEET_SUBSTEPS, H, cands[k][0], cands[k][1], P0) for k in sorted(set(ORACLE_ARGMAX))}
    assert ORACLE_BEST_SHARED[0] in refs
    chosen = [refs[k][b] for b, k in enumerate(ORACLE_ARGMAX)]
    for what, dev, ref, quoted in (("per-track", float(res.loglik.sum()), chosen, ORACLE_SUM_OF_MAXIMA),
                                   ("best shared", float(fleet.loglik[fleet.index]), refs[ORACLE_BEST_SHARED[0]], ORACLE_BEST_SHARED[1])):
        want, scale = sum(t["loglik"] for t in ref), sum(t["abs"] for t in ref)
        print(f"[track-noise] end to end {what}: device {dev:.9f} oracle {want:.9f} sum |l_u| {scale:.3f} "
              f"rel err {abs(dev - want) / scale:.2e}")
        assert abs(want - quoted) < 1e-3
        assert abs(dev - want) < LIK_RTOL * scale, (what, dev, want, scale)
    out = batch.run_batch(hbt)
    assert not out["status"].any() and np.all(np.isfinite(out["means_smoothed"]))
    one = batch.run_batch(dataclasses.replace(hb, Q=cands[4][0], R=cands[4][1], lanes=1))  # track 0 chose candidate 4
    assert ORACLE_ARGMAX[0] == 4 and np.array_equal(_u64(out["means_smoothed"][0]), _u64(one["means_smoothed"][0]))
