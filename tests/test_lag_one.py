"""The smoother's lag-one cross-covariance and the exact covariance of a position at a query time (include/ste.h:
ste_urtss_lag_one_f64, ste_track_position_cov_f64; DESIGN.md, "Lag-one covariance"): the NumPy restatements against the pinned
oracle and against 4 096 restated posterior samples, the ellipse finishing against position_ellipse, and on the GPU the two
kernels against the restatements (lag1 to the history parity bound, the query kernel bit for bit), the closed form against
position_statistics' ensemble, and the Python surface."""
import ctypes as C
import dataclasses
import hashlib

import lag_one_cases as loc
import numpy as np
import path_metrics_cases as pmc
import position_cases as pc
import pytest
import track_sampling_cases as tsc
from test_hip_parity import COV_TOL


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    va, vb = (_u64(a), _u64(b)) if a.dtype == np.float64 else (a, b)
    if a.dtype == np.float64:  # a NaN is a NaN: the payload of an output NaN is not part of the definition
        nan = np.isnan(a) & np.isnan(b)
        va, vb = np.where(nan, 0, va), np.where(nan, 0, vb)
    assert np.array_equal(va, vb), (what, np.flatnonzero((va != vb).reshape(-1))[:8])


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_lag_one_is_the_cross_covariance_of_the_recursion():
    """Test 1.  The linear map A from all draws to all row deviations of the sampler's recursion (wraps aside): the (k, k+1)
    block of A A^T is the cross-covariance of rows k and k + 1 of the sampled tracks, and it equals L_k = K_k P^s_{k+1} to 1e-12
    of the block's largest entry (measured 1.3e-15); the diagonal blocks are the oracle's sm_cov likewise."""
    worst = worst_diag = 0.0
    for case in tsc.oracle_cases():
        L = loc.lag_one(case)
        assert L.shape == (tsc.NMAX, 4, 4)
        A = loc.draws_to_deviations(case.covs, case.steps)
        G = np.dot(A, A.T)
        for k in range(tsc.NMAX):
            blk = G[4 * k:4 * k + 4, 4 * k + 4:4 * k + 8]
            worst = max(worst, float(np.max(np.abs(blk - L[k])) / np.max(np.abs(L[k]))))
            dia = G[4 * k:4 * k + 4, 4 * k:4 * k + 4]
            worst_diag = max(worst_diag, float(np.max(np.abs(dia - case.sm_covs[k])) / np.max(np.abs(case.sm_covs[k]))))
    print(f"(k, k+1) block of A A^T vs K_k P^s_(k+1): {worst:.2e} of the largest entry; diagonal blocks vs sm_cov: {worst_diag:.2e}")
    assert worst <= 1e-12 and worst_diag <= 1e-12


def test_position_cov_restatement():
    """Test 2.  u = 0 returns row k's entries bit for bit (through blend and through the query restatement at a knot); the
    lon / lat block of P(u) has non-negative eigenvalues on every step of the eight tracks at u = 0.25, 0.5, 0.875; and the
    joint covariance [[P_k, L], [L^T, P_{k+1}]] is positive definite."""
    worst_eig, worst_joint = np.inf, np.inf
    for case in tsc.oracle_cases():
        L = loc.lag_one(case)
        for k in range(tsc.NMAX):
            A, B = case.sm_covs[k], case.sm_covs[k + 1]
            _same_bits(loc.blend(0.0, A, B, L[k]), np.ascontiguousarray(A), "u = 0")
            for u in loc.US:
                P = loc.blend(u, A, B, L[k])
                w = np.linalg.eigvalsh(P[:2, :2], UPLO="U")  # the upper triangle: what the kernel reads and writes
                worst_eig = min(worst_eig, float(w[0] / w[1]))
                assert w[0] >= 0.0, (k, u, w)
            J = np.block([[A, L[k]], [L[k].T, B]])
            worst_joint = min(worst_joint, float(np.linalg.eigvalsh(0.5 * (J + J.T))[0] / np.max(np.diag(J))))
    print(f"smallest eigenvalue ratio of the lon / lat block of P(u): {worst_eig:.2e}; smallest eigenvalue of the joint covariance: "
          f"{worst_joint:.2e} of its largest diagonal entry")
    assert worst_joint > 0.0
    # the query restatement: a knot hit copies the row, an interior query is blend() of the two rows and the lag-one block
    cov, lag1 = loc.random_covariances(5, 3, seed=1)
    nsteps, dt = np.array([4, 2, 0], dtype=np.int32), np.ones((4, 3))
    r = loc.position_cov(cov, lag1, nsteps, dt, [0, 0, 1, 2, 2, 3], [2.0, 2.25, 1.5, 0.0, 0.5, 0.0], full=True)
    assert r["status"].tolist() == [0, 0, 0, 0, pc.OUTSIDE, pc.BAD_INDEX] and r["step"].tolist() == [2, 2, 1, 0, -1, -1]
    _same_bits(r["pcov"][:, 0], np.array([cov[2, a, b, 0] for a, b in loc.PACKED]), "knot hit")
    _same_bits(r["pcov"][:, 1], np.array([loc.blend(0.25, cov[2, :, :, 0], cov[3, :, :, 0], lag1[2, :, :, 0])[a, b] for a, b in loc.PACKED]),
               "interior")
    assert np.isnan(r["pcov"][:, 4:]).all() and np.isfinite(r["pcov"][:, :4]).all()
    short = loc.position_cov(cov, lag1, nsteps, dt, [0, 0, 1, 2, 2, 3], [2.0, 2.25, 1.5, 0.0, 0.5, 0.0])
    _same_bits(short["pcov"], r["pcov"][[0, 1, 4]], "position form against the full one")


def test_analytic_covariance_against_the_restated_ensemble():
    """Test 3.  4 096 restated samples per track (the host draws of the statistics tests), interpolated at u = 0.25, 0.5, 0.875
    of every step: the analytic P(u) holds |var_S / var - 1| <= 5 sqrt(2 / (S - 1)) = 0.1105 on all four components and the
    lon / lat covariance within 5 sqrt((var_x var_y + cov^2) / (S - 1)); the mean offset stays within 5 standard errors.  The
    formula WITHOUT the cross term fails the variance bound on every one of the 96 steps at u = 0.5 -- which is what makes the
    GPU statistics test able to see L.  Measured with these draws: 0.056 over the four components (0.055 lon / lat), covariance
    0.77 of its bound, mean 2.5 standard errors; without the cross term var_S / var - 1 = 0.77 .. 1.09 (the formula gives
    0.48 - 0.57 of the ensemble's variance)."""
    S = loc.STAT_S
    worst_all = worst_pos = worst_cov = worst_mean = 0.0
    off = []
    for case, d in zip(tsc.oracle_cases(), loc.stat_samples()):
        L = loc.lag_one(case)
        for k in range(tsc.NMAX):
            for u in loc.US:
                P = loc.blend(u, case.sm_covs[k], case.sm_covs[k + 1], L[k])
                x = (1.0 - u) * d[:, k] + u * d[:, k + 1]  # (S, 4)
                var_s = x.var(axis=0, ddof=1)
                cxy_s = float(np.cov(x[:, 0], x[:, 1], ddof=1)[0, 1])
                var = np.diag(P)
                worst_all = max(worst_all, float(np.max(np.abs(var_s / var - 1.0))))
                r, cfrac = loc.ensemble_check(var[:2], P[0, 1], var_s[:2], cxy_s, S)
                worst_pos, worst_cov = max(worst_pos, r), max(worst_cov, cfrac)
                worst_mean = max(worst_mean, float(np.max(np.abs(x.mean(axis=0)) / np.sqrt(var / S))))
                if u == 0.5:
                    P0 = loc.blend_without_cross(u, case.sm_covs[k], case.sm_covs[k + 1])
                    off.append(np.abs(var_s[:2] / np.diag(P0)[:2] - 1.0))
    off = np.array(off)
    print(f"analytic P(u) vs {S} restated samples: worst |var_S / var - 1| = {worst_all:.4f} over four components, {worst_pos:.4f} "
          f"lon / lat (bound {loc.VAR_BOUND:.4f}); covariance {worst_cov:.3f} of its 5-sigma bound; mean {worst_mean:.2f} standard "
          f"errors; without the cross term at u = 0.5: {off.min():.3f} .. {off.max():.3f} off on {len(off)} steps")
    assert worst_all <= loc.VAR_BOUND and worst_cov <= 1.0 and worst_mean <= 5.0
    assert off.shape == (8 * tsc.NMAX, 2) and (off > loc.VAR_BOUND).all()


def test_covariance_ellipse_against_position_ellipse():
    """Test 4.  Two samples at anchor +- (dx, dy) have the moments (0, 0, 2 dx dx, 2 dx dy, 2 dy dy) and, with ddof = 1, the
    covariance (2 dx dx, 2 dx dy, 2 dy dy) exactly: position_ellipse on the moments and covariance_ellipse on the covariance give
    the same half-axes and orientation to 1e-14 relative (the minor axis, which is 0 here, to 1e-14 of the major)."""
    from track_estimators import batch

    rng = np.random.default_rng(4)
    Q = 64
    dx, dy, lat = rng.normal(0.0, 0.05, Q), rng.normal(0.0, 0.03, Q), rng.uniform(-75.0, 75.0, Q)
    moments = np.stack([np.zeros(Q), np.zeros(Q), 2.0 * dx * dx, 2.0 * dx * dy, 2.0 * dy * dy])
    a = batch.position_ellipse(np.full(Q, 2, dtype=np.int32), moments, lat, prob=0.9)
    b = batch.covariance_ellipse(2.0 * dx * dx, 2.0 * dx * dy, 2.0 * dy * dy, lat, prob=0.9)
    assert set(b) == {"cov_km", "semi_major_km", "semi_minor_km", "orientation_deg"}
    assert np.max(np.abs(b["semi_major_km"] / a["semi_major_km"] - 1.0)) <= 1e-14
    assert np.max(np.abs(b["semi_minor_km"] - a["semi_minor_km"]) / a["semi_major_km"]) <= 1e-14
    assert np.max(np.abs(b["orientation_deg"] - a["orientation_deg"]) / 180.0) <= 1e-14
    assert np.max(np.abs(b["cov_km"] - a["cov_km"]) / np.max(np.abs(a["cov_km"]), axis=(1, 2), keepdims=True)) <= 1e-14
    # a full-rank case with a known answer: variances 4 and 1 km^2 along east and north at the equator
    k = batch.KM_PER_DEG
    e = batch.covariance_ellipse([4.0 / k / k], [0.0], [1.0 / k / k], [0.0], prob=1.0 - np.exp(-0.5))  # scale 1
    assert e["semi_major_km"][0] == pytest.approx(2.0, rel=1e-14) and e["semi_minor_km"][0] == pytest.approx(1.0, rel=1e-14)
    assert e["orientation_deg"][0] == pytest.approx(90.0, abs=1e-12)
    assert np.isnan(batch.covariance_ellipse([np.nan], [0.0], [1.0], [0.0])["semi_major_km"][0])
    with pytest.raises(ValueError, match="prob must lie strictly between 0 and 1"):
        batch.covariance_ellipse([1.0], [0.0], [1.0], [0.0], prob=1.0)
    with pytest.raises(ValueError, match=r"wanted as \(Q,\) arrays"):
        batch.covariance_ellipse([1.0, 2.0], [0.0], [1.0], [0.0])


def test_refusals_before_any_launch():
    """Every refusal of the two headers returns STE_EINVAL (-1) with its reason; a launch on a machine without a GPU would
    return STE_ELAUNCH (-2), so -1 shows the call stopped before launching."""
    from test_ukf_loglik import _batch
    from track_estimators._hip import binding

    lib, keep = binding.load(), []
    name = "ste_urtss_lag_one_f64"

    def good_batch():
        s = _batch(binding, keep)
        s.sm_mean = s.sm_cov = 0x6000
        s.rts_work = 0x3000
        return s

    def lag(s, g):
        rc = lib.ste_urtss_lag_one_f64(None if s is None else C.byref(s), None, None if g is None else C.byref(g), None)
        return rc, lib.ste_last_error().decode()

    good = lambda: binding.SteLagOneF64(0x7000, 0x8000, 0, 0)  # noqa: E731
    rc, msg = lag(None, good())
    assert rc == -1 and "batch pointer is NULL" in msg
    rc, msg = lag(good_batch(), None)
    assert rc == -1 and "lag-one arguments (lg) are NULL" in msg and name in msg
    g = good()
    g.lag1 = None
    rc, msg = lag(good_batch(), g)
    assert rc == -1 and "lg->lag1 is required" in msg and name in msg
    g = good()
    g.flags = 0x2
    rc, msg = lag(good_batch(), g)
    assert rc == -1 and "unknown bits" in msg and name in msg
    g = good()
    g.reserved = 1
    rc, msg = lag(good_batch(), g)
    assert rc == -1 and "reserved must be 0" in msg
    for field in ("rts_work", "fwd_mean", "fwd_cov"):
        s = good_batch()
        setattr(s, field, None)
        rc, msg = lag(s, good())
        assert rc == -1 and "completed forward pass with rts_work" in msg and name in msg, field
    for b, e in ((64, 0), (0, 128), (64, 256)):
        s = good_batch()
        s.step_begin, s.step_end = b, e
        rc, msg = lag(s, good())
        assert rc == -1 and "time slices" in msg and name in msg, (b, e)
    s = good_batch()
    s.sm_cov = None
    rc, msg = lag(s, good())
    assert rc == -1 and "sm_mean and sm_cov are required" in msg
    s = good_batch()
    s.track_stride = 4
    rc, msg = lag(s, good())
    assert rc == -1 and "track_stride" in msg

    name = "ste_track_position_cov_f64"

    def pcov(s, p):
        rc = lib.ste_track_position_cov_f64(None if s is None else C.byref(s), None if p is None else C.byref(p), None)
        return rc, lib.ste_last_error().decode()

    def good_pc(**kw):
        p = binding.StePositionCovF64()
        p.nqueries = 5
        for f in ("qtrack", "qtime", "knots", "cov", "lag1", "pcov"):
            setattr(p, f, 0x9000)
        for f, v in kw.items():
            setattr(p, f, v)
        return p

    rc, msg = pcov(None, good_pc())
    assert rc == -1 and "batch pointer is NULL" in msg and name in msg
    rc, msg = pcov(good_batch(), None)
    assert rc == -1 and "(pc) are NULL" in msg
    for field in ("qtrack", "qtime", "knots"):
        rc, msg = pcov(good_batch(), good_pc(**{field: None}))
        assert rc == -1 and f"pc->{field} is required" in msg and name in msg, field
    for n in (0, (1 << 26) + 1):
        rc, msg = pcov(good_batch(), good_pc(nqueries=n))
        assert rc == -1 and "nqueries" in msg
    rc, msg = pcov(good_batch(), good_pc(flags=0x4))
    assert rc == -1 and "unknown bits" in msg
    rc, msg = pcov(good_batch(), good_pc(reserved=3))
    assert rc == -1 and "reserved must be 0" in msg
    rc, msg = pcov(good_batch(), good_pc(flags=binding.STE_PCOV_FULL | binding.STE_PCOV_LAG1_POSITION))
    assert rc == -1 and "needs the 16-entry lag1" in msg
    rc, msg = pcov(good_batch(), good_pc(pcov=None))
    assert rc == -1 and "no output asked for" in msg
    rc, msg = pcov(good_batch(), good_pc(cov=None))
    assert rc == -1 and "pc->cov is required" in msg
    rc, msg = pcov(good_batch(), good_pc(lag1=None))
    assert rc == -1 and "pc->lag1 is required" in msg
    s = good_batch()
    s.track_stride = 4
    rc, msg = pcov(s, good_pc())
    assert rc == -1 and "track_stride" in msg
    s = good_batch()
    s.B = 0
    rc, msg = pcov(s, good_pc())
    assert rc == -1 and "B must be > 0" in msg


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
SENTINEL = -777.0


def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _lag_abi(db, position=False, into=None):
    """ste_urtss_lag_one_f64 through ctypes into a sentinel-filled [N][rows][ld] tensor (``into``: a fleet-wide one, written
    at this window's columns); -> (lag1 as NumPy (N, rows, ld), status (B,))."""
    from track_estimators._hip import binding

    torch = db.torch
    N, ld = int(db.struct.Nmax), int(db.struct.track_stride or db.struct.B)
    rows = 4 if position else 16
    t = torch.full((N, rows, ld), SENTINEL, dtype=torch.float64, device=db.device) if into is None else into
    status = torch.full((db.ntracks,), 0x7FFF, dtype=torch.int32, device=db.device)  # the call clears it
    lg = binding.SteLagOneF64(t.data_ptr() + 8 * db.lo, status.data_ptr(), binding.STE_LAG1_POSITION if position else 0, 0)
    nz = None if db.noise is None else C.byref(db.noise)
    binding.check(db.lib.ste_urtss_lag_one_f64(C.byref(db.struct), nz, C.byref(lg), db._stream(None)), "ste_urtss_lag_one_f64")
    torch.cuda.synchronize()
    return t.cpu().numpy(), status.cpu().numpy()


def _digest(db):
    h = hashlib.sha256()
    for n in ("status", "fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "rts_work"):
        h.update(getattr(db, n).cpu().numpy().tobytes())
    return h.hexdigest()


def _lag_reference(cases, track_index, nsteps):
    """(Nmax, 16, B) from the restatement, NaN where a track has no such step."""
    ref = np.full((tsc.NMAX, 16, len(track_index)), np.nan)
    for b, (i, ns) in enumerate(zip(track_index, nsteps)):
        _, _, steps, _, sm_cov = tsc.truncated(cases[i], int(ns))
        if ns:
            ref[:ns, :, b] = loc.lag_one(steps, sm_cov).reshape(ns, 16)
    return ref


def _check_lag(got, pos, ref, what):
    live = ~np.isnan(ref)
    err = float(np.max(np.abs(got[live] - ref[live])) / max(float(np.max(np.abs(ref[live]))), 1.0))
    print(f"lag1 vs restatement ({what}): {err:.2e} of max(max|ref|, 1)")
    assert err <= COV_TOL, what
    assert (got[~live] == SENTINEL).all(), (what, "rows past nsteps")
    _same_bits(pos[:, [0, 1, 2, 3]], got[:, [0, 1, 4, 5]], (what, "position form"))


RAGGED = [0, 1, 2, 5, 7, 9, 11, 12]


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "full"])
@pytest.mark.parametrize("smoother", [0x400, 0x200], ids=["one-kernel", "two-kernel"])
def test_lag_one_against_the_restatement(packed, smoother):
    """Test 5.  The eight tracks plus a ragged copy (nsteps 0 and 1 among them), full and packed covariances, work rows in D form
    (one-kernel smoother) and rewritten into gains (two-kernel smoother): max |dev - ref| <= COV_TOL max(max |ref|, 1), both
    output forms, the position form bit-equal to its four entries of the full one, rows >= nsteps untouched, status cleared and
    0, the batch's arrays unchanged.  Also printed, not asserted: whether K P^s formed on the host from the sampler's coefficient
    buffer gives the same bits.  Measured on an MI355X: 1.6e-13 in all four cases, and the host product has the kernel's bits."""
    from track_estimators import batch
    from track_estimators._hip import binding

    cases = tsc.oracle_cases()
    idx, nsteps = np.arange(16) % 8, [tsc.NMAX] * 8 + RAGGED
    hb = tsc.host_batch(idx, nsteps)
    db = batch.DeviceBatch(hb, tuning=smoother, packed_cov=packed)
    db.run()
    db.torch.cuda.synchronize()
    assert ((db.rts_work[-1].cpu().numpy() < 0).all()) == (smoother == 0x200)
    before = _digest(db)
    got, status = _lag_abi(db)
    pos, status_p = _lag_abi(db, position=True)
    assert _digest(db) == before
    assert not status.any() and not status_p.any()
    _check_lag(got, pos, _lag_reference(cases, idx, nsteps), f"packed={packed}, tuning={smoother:#x}")
    # K P^s on the host from the sampler's coefficients (K at rows 0 .. 15 of coef), with the kernel's operation order
    coef = db.torch.empty((tsc.NMAX + 1, binding.STE_SAMPLE_COEF_ROWS, 16), dtype=db.torch.float64, device=db.device)
    sm = binding.SteUkfSampleF64(1, 0, coef.data_ptr(), coef.data_ptr(), None)
    binding.check(db.lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), None, C.byref(sm), db._stream(None)), "prepare")
    db.torch.cuda.synchronize()
    K = coef.cpu().numpy()[:-1, :16].reshape(tsc.NMAX, 4, 4, 16)
    sP = db.download(("covs_smoothed",))["covs_smoothed"].reshape(16, tsc.NMAX + 1, 4, 4).transpose(1, 2, 3, 0)  # (N+1, 4, 4, B)
    live = np.broadcast_to((np.arange(tsc.NMAX)[:, None] < np.asarray(nsteps)[None, :])[:, None, :], (tsc.NMAX, 16, 16))
    K, P1 = np.where(live.reshape(tsc.NMAX, 4, 4, 16), K, 0.0), sP[1:]  # coefficient rows past nsteps are not the call's
    host = K[:, :, 0, None] * P1[:, None, 0]
    for i in range(1, 4):
        host = _fma(K[:, :, i, None], P1[:, None, i], host)
    same = np.array_equal(_u64(host.reshape(tsc.NMAX, 16, 16)[live]), _u64(got[live]))
    print(f"K P^s on the host from the sampler's coefficient buffer gives the kernel's bits: {same}")


def _fma(a, b, c):
    """Element-wise fused multiply-add in NumPy: exact product and sum in long double would not be a single rounding, so go
    through Python's math.fma where it exists and else through fractions (slow, small arrays)."""
    import math

    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape)
    if hasattr(math, "fma"):
        f = math.fma
    else:
        from fractions import Fraction

        def f(x, y, z):
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                return x * y + z
            return float(Fraction(x) * Fraction(y) + Fraction(z))
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1), b.reshape(-1), c.reshape(-1))):
        flat[i] = f(float(x), float(y), float(z))
    return out


@pytest.mark.gpu
def test_lag_one_with_a_q_per_track():
    """Test 5, per-track noise: a Q stack (four different matrices over the eight tracks, ragged) against the restatement of
    the oracle run with each track's own Q."""
    from track_estimators import batch, synthetic

    _, Q, _, _ = synthetic.example_matrices()
    Q2 = Q * 2.0
    Q2[0, 2] = Q2[2, 0] = 1e-6
    Q2[1, 3] = Q2[3, 1] = -2e-6
    Qs = np.stack([Q, Q2, Q * 0.5, Q2] * 2)
    nsteps = [12, 11, 12, 7, 12, 12, 3, 12]
    db = batch.DeviceBatch(tsc.host_batch(np.arange(8), nsteps, Qs=Qs, lanes=1))
    assert db.noise is not None
    db.run()
    got, status = _lag_abi(db)
    pos, _ = _lag_abi(db, position=True)
    assert not status.any()
    _check_lag(got, pos, _lag_reference(tsc.oracle_cases(Qs), np.arange(8), nsteps), "per-track Q")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [65, 129])
def test_lag_one_batch_sizes_and_windows(B):
    """Test 5, B = 65 and 129 (one and two full waves plus a lane, ragged, every length 0 .. Nmax): against the restatement;
    and for B = 129 the window [3, 70) in place (track_stride 129) equals a batch of its own of those tracks bit for bit,
    writes nothing outside its columns, and leaves the fleet's arrays alone."""
    from track_estimators import batch

    idx = np.arange(B) % 8
    nsteps = (tsc.NMAX - (np.arange(B) * 5) % (tsc.NMAX + 1)).astype(np.int32)
    db = batch.DeviceBatch(tsc.host_batch(idx, nsteps))
    db.run()
    got, status = _lag_abi(db)
    pos, _ = _lag_abi(db, position=True)
    assert not status.any()
    _check_lag(got, pos, _lag_reference(tsc.oracle_cases(), idx, nsteps), f"B = {B}")
    if B != 129:
        return
    lo, hi = 3, 70
    win = db.window(lo, hi)
    before = _digest(db)
    fleet_wide = db.torch.full((tsc.NMAX, 16, B), SENTINEL, dtype=db.torch.float64, device=db.device)
    inplace, st = _lag_abi(win, into=fleet_wide)
    assert _digest(db) == before and st.shape == (hi - lo,) and not st.any()
    assert (inplace[..., :lo] == SENTINEL).all() and (inplace[..., hi:] == SENTINEL).all()
    own = batch.DeviceBatch(tsc.host_batch(idx[lo:hi], nsteps[lo:hi]))
    own.run()
    alone, _ = _lag_abi(own)
    _same_bits(inplace[..., lo:hi], alone, "window [3, 70) of 129 in place against a batch of its own")
    _same_bits(inplace[..., lo:hi], got[..., lo:hi], "window against the whole batch")
    # the front end: a tensor of the window's tracks, rows past nsteps zero
    lag, lst = win.lag_one_covariance()
    assert tuple(lag.shape) == (tsc.NMAX, 16, hi - lo) and not lst.cpu().numpy().any()
    live = np.arange(tsc.NMAX)[:, None, None] < nsteps[None, None, lo:hi]
    _same_bits(np.where(live, lag.cpu().numpy(), SENTINEL), alone, "lag_one_covariance() of a window")
    assert (lag.cpu().numpy()[~np.broadcast_to(live, lag.shape)] == 0.0).all()


# ---- the query kernel ---------------------------------------------------------------------------------------------
PCOV_OUT = ("pcov", "step", "frac", "status")
_DT = {"step": "int32", "status": "int32"}


def _pcov_abi(db, knots, cov, lag1, qtrack, qtime, t0, full=False, lag_position=False, want=PCOV_OUT, batch_struct=None):
    """ste_track_position_cov_f64 through ctypes: cov, lag1 and knots device tensors in rows of the struct's track_stride with
    the pointers at the window's first track; ``want``: the outputs asked for (the others are NULL) -> dict of NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    s = db.struct if batch_struct is None else batch_struct
    Q = len(qtrack)
    keep = [_dev(db, np.asarray(qtrack, dtype=np.int32)), _dev(db, np.asarray(qtime, dtype=np.float64))]
    p = binding.StePositionCovF64()
    p.flags = (binding.STE_PCOV_FULL if full else 0) | (binding.STE_PCOV_LAG1_POSITION if lag_position else 0)
    p.nqueries, p.qtrack, p.qtime = Q, keep[0].data_ptr(), keep[1].data_ptr()
    if t0 is not None:
        keep.append(_dev(db, np.asarray(t0, dtype=np.float64)))
        p.t0 = keep[-1].data_ptr()
    off = 8 * db.lo
    p.knots, p.cov, p.lag1 = knots.data_ptr() + off, cov.data_ptr() + off, lag1.data_ptr() + off
    out = {}
    for k in want:
        shape = ((10 if full else 3), Q) if k == "pcov" else (Q,)
        out[k] = torch.full(shape, -5, dtype=getattr(torch, _DT.get(k, "float64")), device=db.device)
        setattr(p, k, out[k].data_ptr())
    binding.check(db.lib.ste_track_position_cov_f64(C.byref(s), C.byref(p), db._stream(None)), "ste_track_position_cov_f64")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_outputs(a, b, what, cols_b=slice(None), keys=PCOV_OUT):
    for k in keys:
        _same_bits(a[k], b[k][..., cols_b], (what, k))


@pytest.mark.gpu
def test_position_cov_against_the_restatement():
    """Test 6.  The fleet of position_cases (B = 70, Nmax = 9, Q = 754: antimeridian, zero-hour steps, bad times and indices,
    outside) and its 35 named queries on the eight hand-made tracks, with seeded random symmetric cov and random lag1 (the
    kernel reads no states): pcov, step, frac and status equal the restatement bit for bit, NaN patterns included, in both
    output forms and from both lag1 forms; step, frac and status are those of positions_at on the same list.  The same bits
    for the list reversed and shuffled, Q = 64 and 65, the window [3, 70), t0 NULL against zeros, each output alone, full
    against position output on the three shared entries, packed against full cov, and through the front end."""
    from track_estimators import batch
    from track_estimators._hip import binding

    # the hand-made tracks: 35 named queries
    h = pc.hand_batch()
    hdb = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False, packed_cov=False)
    cov, lag1 = loc.random_covariances(pc.HAND_N + 1, pc.HAND_B, seed=21)
    states = _dev(hdb, h["states"])
    pos = hdb.positions_at(states, h["qtrack"], h["qtime"], t0=h["t0"], sort=False)
    dcov, dlag = _dev(hdb, cov.reshape(pc.HAND_N + 1, 16, pc.HAND_B)), _dev(hdb, lag1.reshape(pc.HAND_N, 16, pc.HAND_B))
    assert len(h["qtrack"]) == 35
    for full in (False, True):
        got = _pcov_abi(hdb, pos["knots"], dcov, dlag, h["qtrack"], h["qtime"], h["t0"], full=full)
        _same_outputs(got, loc.position_cov(cov, lag1, h["nsteps"], h["dt"], h["qtrack"], h["qtime"], h["t0"], full=full), f"hand, full={full}")
        for k in ("step", "frac", "status"):
            _same_bits(got[k], pos[k].cpu().numpy(), ("hand, against positions_at", k))

    # the fleet
    w = pc.fleet()
    N, B = pc.FLEET_N, pc.FLEET_B
    qtrack, qtime, t0 = w["qtrack"], w["qtime"], w["t0"]
    Q = len(qtrack)
    assert (B, N, Q) == (70, 9, 754)
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False, packed_cov=False)
    cov, lag1 = loc.random_covariances(N + 1, B, seed=22)
    for b, ns in enumerate(w["nsteps"]):  # rows past nsteps are not read: NaN there changes nothing
        cov[ns + 1:, :, :, b] = np.nan
        lag1[ns:, :, :, b] = np.nan
    ref = {f: loc.position_cov(cov, lag1, w["nsteps"], w["dt"], qtrack, qtime, t0, full=f) for f in (False, True)}
    assert np.isnan(ref[True]["pcov"]).all(axis=0).sum() == (ref[True]["step"] < 0).sum() > 100
    assert not np.isnan(ref[True]["pcov"][:, ref[True]["step"] >= 0]).any()
    pos = db.positions_at(_dev(db, w["states"]), qtrack, qtime, t0=t0, sort=False)
    knots = pos["knots"]
    dcov, dlag = _dev(db, cov.reshape(N + 1, 16, B)), _dev(db, lag1.reshape(N, 16, B))
    dlag4 = _dev(db, lag1.reshape(N, 16, B)[:, [0, 1, 4, 5]])
    whole = {f: _pcov_abi(db, knots, dcov, dlag, qtrack, qtime, t0, full=f) for f in (False, True)}
    for f in (False, True):
        _same_outputs(whole[f], ref[f], f"fleet, full={f}")
    for k in ("step", "frac", "status"):
        _same_bits(whole[False][k], pos[k].cpu().numpy(), ("fleet, against positions_at", k))
    _same_bits(whole[True]["pcov"][[0, 1, 4]], whole[False]["pcov"], "full against position output")
    _same_outputs(_pcov_abi(db, knots, dcov, dlag4, qtrack, qtime, t0, lag_position=True), whole[False], "4-entry lag1")
    base = whole[False]
    for name, perm in (("reversed", np.arange(Q)[::-1]), ("shuffled", np.random.default_rng(3).permutation(Q))):
        _same_outputs(_pcov_abi(db, knots, dcov, dlag, qtrack[perm], qtime[perm], t0), base, name, cols_b=perm)
        _same_outputs(_pcov_abi(db, knots, dcov, dlag, qtrack[perm], qtime[perm], t0, full=True), whole[True], name + ", full", cols_b=perm)
    for n in (64, 65):
        _same_outputs(_pcov_abi(db, knots, dcov, dlag, qtrack[:n], qtime[:n], t0), base, f"Q = {n}", cols_b=slice(0, n))
    for k in PCOV_OUT:
        _same_outputs(_pcov_abi(db, knots, dcov, dlag, qtrack, qtime, t0, want=(k,)), base, f"{k} alone", keys=(k,))
    zeros = _pcov_abi(db, knots, dcov, dlag, qtrack, qtime, np.zeros(B))
    _same_outputs(_pcov_abi(db, knots, dcov, dlag, qtrack, qtime, None), zeros, "t0 NULL against zeros")
    assert not np.array_equal(zeros["status"], base["status"])
    # packed cov: the same bits from upper triangles
    packed_struct = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
    packed_struct.flags |= binding.STE_FLAG_PACKED_COV
    dpk = _dev(db, loc.packed_rows(cov))
    for f in (False, True):
        _same_outputs(_pcov_abi(db, knots, dpk, dlag, qtrack, qtime, t0, full=f, batch_struct=packed_struct), whole[f], f"packed cov, full={f}")
    # the window [3, 70) in place (rows of 70 tracks, pointers at column 3)
    lo, hi = pc.FLEET_WINDOW
    inside = (qtrack >= lo) & (qtrack < hi)
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == B and inside.sum() > 600
    kn_full = db.torch.full((N + 1, B), np.nan, dtype=db.torch.float64, device=db.device)
    kn_full[:, :] = knots
    for f in (False, True):
        got = _pcov_abi(win, kn_full, dcov, dlag, qtrack[inside] - lo, qtime[inside], t0[lo:hi], full=f)
        _same_outputs(got, whole[f], f"window, full={f}", cols_b=inside)


@pytest.mark.gpu
def test_statistics_against_the_samples():
    """Test 7.  The eight tracks with the 4 096 host draws of the statistics tests, queried at u = 0.25, 0.5, 0.875 of every
    step and at every knot (392 queries): cov_km of position_statistics' ensemble (the moments continued over four calls of
    1 024 samples) against cov_km of position_covariance: |var_S / var - 1| <= 5 sqrt(2 / (S - 1)) on both diagonals and the
    covariance within 5 sqrt((var_e var_n + cov^2) / (S - 1)) -- bounds the formula without L misses by a factor of four at
    mid-step (test_analytic_covariance_against_the_restated_ensemble).  At the knots position_covariance is the lon / lat
    block of sm_cov in km, exactly.  Measured on an MI355X: 0.055 (inside the steps 0.048) and 0.77 of the covariance bound."""
    from track_estimators import batch

    hb = tsc.host_batch(np.arange(8))
    db = batch.DeviceBatch(hb)
    db.run()
    N, S = tsc.NMAX, loc.STAT_S
    T = pc.knot_times(hb.nsteps, hb.dt)  # (N+1, 8)
    qtrack, qtime = [], []
    for t in range(8):
        for k in range(N):
            qtrack += [t] * 4
            qtime += [T[k, t]] + [T[k, t] + u * (T[k + 1, t] - T[k, t]) for u in loc.US]
        qtrack.append(t)
        qtime.append(T[N, t])
    qtrack, qtime = np.array(qtrack, dtype=np.int32), np.array(qtime)
    exact = batch.position_covariance(db, qtrack, qtime)
    assert not exact["status"].any() and not exact["lag_status"].any() and exact["lag_status"].shape == (8,)
    knot = exact["frac"] == 0.0
    assert knot.sum() == 8 * (N + 1) and (exact["frac"][~knot] > 0.0).all()
    anchor = db.torch.stack([_dev(db, exact["lon"]), _dev(db, exact["lat"])])
    draws = np.random.default_rng(loc.STAT_SEED).standard_normal((S, N + 1, 4, 8))
    acc, chunk, knots = None, 1024, None
    for i in range(0, S, chunk):
        samples = db.sample_smoothed(chunk, draws=_dev(db, draws[i:i + chunk]))
        r = db.positions_at(samples, qtrack, qtime, anchor=anchor, accumulate=acc, knots=knots)
        acc, knots = (r["count"], r["moments"]), r["knots"]
    assert not db.sample_status.cpu().numpy().any() and (acc[0].cpu().numpy() == S).all()
    e = batch.position_ellipse(acc[0].cpu().numpy(), acc[1].cpu().numpy(), exact["lat"])
    cs, ca = e["cov_km"], exact["cov_km"]
    ratio = max(np.abs(cs[:, 0, 0] / ca[:, 0, 0] - 1.0).max(), np.abs(cs[:, 1, 1] / ca[:, 1, 1] - 1.0).max())
    cbound = 5.0 * np.sqrt((ca[:, 0, 0] * ca[:, 1, 1] + ca[:, 0, 1] ** 2) / (S - 1))
    cfrac = (np.abs(cs[:, 0, 1] - ca[:, 0, 1]) / cbound).max()
    inner = np.abs(cs[~knot, 0, 0] / ca[~knot, 0, 0] - 1.0).max()
    print(f"position_covariance vs {S} samples at {len(qtrack)} queries: worst |var_S / var - 1| = {ratio:.4f} (inside the steps "
          f"{inner:.4f}; bound {loc.VAR_BOUND:.4f}), worst covariance deviation {cfrac:.3f} of its 5-sigma bound")
    assert ratio <= loc.VAR_BOUND and cfrac <= 1.0
    assert (exact["semi_major_km"] >= exact["semi_minor_km"]).all() and (exact["semi_minor_km"] > 0.0).all()
    # at the knots: the lon / lat block of sm_cov in km, exactly
    sP = db.download(("covs_smoothed",))["covs_smoothed"].reshape(8, N + 1, 4, 4)
    rows = sP[qtrack[knot], exact["step"][knot]]
    ke, kn = batch.KM_PER_DEG * np.cos(np.radians(exact["lat"][knot])), batch.KM_PER_DEG
    _same_bits(ca[knot, 0, 0], rows[:, 0, 0] * ke * ke, "knots, east")
    _same_bits(ca[knot, 0, 1], rows[:, 0, 1] * ke * kn, "knots, cross")
    _same_bits(ca[knot, 1, 1], rows[:, 1, 1] * kn * kn, "knots, north")


@pytest.mark.gpu
def test_front_ends():
    """Test 8.  position_covariance on a HostBatch equals the call on the DeviceBatch after run(); lag_one= and knots= passed
    back in give the same bits, in both lag1 forms, sorted or not; UnscentedKalmanFilter.position_at(covariance=True) agrees
    with it for one track and without the keyword returns what it returned before; a batch without work rows raises."""
    import types

    from track_estimators import batch, synthetic
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter

    nsteps = [12, 11, 12, 7, 12, 12, 3, 12]
    hb = tsc.host_batch(np.arange(8), nsteps)
    db = batch.DeviceBatch(hb)
    db.run()
    rng = np.random.default_rng(5)
    T = pc.knot_times(hb.nsteps, hb.dt)
    t0 = np.round(rng.uniform(-5.0, 5.0, 8), 1)
    qtrack = np.concatenate([np.repeat(np.arange(8), 6), [0, 3, 6, 8]]).astype(np.int32)
    span = np.array([T[hb.nsteps[t], t] for t in range(8)])
    qtime = np.concatenate([t0[qtrack[:48]] + rng.uniform(0.0, 1.0, 48) * span[qtrack[:48]], [t0[0], t0[3] + span[3], t0[6] + span[6] + 1.0, 0.0]])
    a = batch.position_covariance(hb, qtrack, qtime, t0=t0)
    b = batch.position_covariance(db, qtrack, qtime, t0=t0)
    assert set(a) == {"lon", "lat", "speed", "heading", "step", "frac", "status", "cov_km", "semi_major_km", "semi_minor_km",
                      "orientation_deg", "lag_status"}
    for k in a:
        _same_bits(a[k], b[k], k)
    assert b["status"][-4:].tolist() == [0, 0, pc.OUTSIDE, pc.BAD_INDEX] and b["cov_km"].shape == (52, 2, 2)
    assert np.isnan(b["cov_km"][-2:]).all() and np.isfinite(b["cov_km"][:-2]).all() and b["lag_status"].shape == (8,)
    smoothed = batch.position_statistics(db, qtrack, qtime, 2, t0=t0)
    for k in ("lon", "lat", "speed", "heading", "step", "frac", "status"):
        _same_bits(b[k], smoothed[k], ("against position_statistics", k))
    first = db.position_covariance_at(qtrack, qtime, t0=t0)
    assert set(first) == {"pcov", "step", "frac", "status", "knots", "lag_one", "lag_status"}
    assert tuple(first["pcov"].shape) == (3, 52) and tuple(first["lag_one"].shape) == (tsc.NMAX, 4, 8)
    again = db.position_covariance_at(qtrack, qtime, t0=t0, lag_one=first["lag_one"], knots=first["knots"], sort=False)
    assert "lag_status" not in again
    full = db.position_covariance_at(qtrack, qtime, t0=t0, full=True)
    assert tuple(full["pcov"].shape) == (10, 52) and tuple(full["lag_one"].shape) == (tsc.NMAX, 16, 8)
    from16 = db.position_covariance_at(qtrack, qtime, t0=t0, lag_one=full["lag_one"])
    for other, what in ((again, "passed back in"), (from16, "16-entry lag_one")):
        for k in ("pcov", "step", "frac", "status"):
            _same_bits(other[k].cpu().numpy(), first[k].cpu().numpy(), (what, k))
    _same_bits(full["pcov"].cpu().numpy()[[0, 1, 4]], first["pcov"].cpu().numpy(), "full=True")
    with pytest.raises(ValueError, match="full=True needs the 16-entry"):
        db.position_covariance_at(qtrack, qtime, lag_one=first["lag_one"], full=True)
    with pytest.raises(ValueError, match="lag_one must be"):
        db.position_covariance_at(qtrack, qtime, lag_one=first["knots"])
    with pytest.raises(ValueError, match="fuse_gains=False"):
        nogains = batch.DeviceBatch(hb, fuse_gains=False)
        nogains.run()
        nogains.lag_one_covariance()
    with pytest.raises(ValueError, match="fuse_gains=False"):
        batch.position_covariance(nogains, qtrack, qtime)
    with pytest.raises(ValueError, match="prob must lie strictly between 0 and 1"):
        batch.position_covariance(db, qtrack, qtime, prob=1.5)

    # the drop-in filter, one track
    sb = tsc.synthetic_batch()
    H, Q, R, P0 = synthetic.example_matrices()
    trk = types.SimpleNamespace(z=sb.z[0], dts=sb.dts[0], sog=sb.sog[0], cog=sb.cog[0], sog_rate=sb.sog_rate[0].copy(),
                                cog_rate=sb.cog_rate[0].copy())
    ukf = UnscentedKalmanFilter(H=H, Q=Q, R=R, P=P0, x0=sb.z[0][:, 0], non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    one = ukf._sample_hb
    Tk = pc.knot_times(one.nsteps, one.dt)[:, 0]
    times = np.concatenate([Tk[:3], [0.5 * (Tk[1] + Tk[2]), 0.25 * Tk[1], Tk[-1] + 1.0]])
    plain = ukf.position_at(times)
    odb = batch.DeviceBatch(one)
    odb.run()
    want = odb.positions_at(odb.sm_mean, np.zeros(6, dtype=np.int32), times, velocity=True)
    _same_bits(plain, np.stack([want[k][0].cpu().numpy() for k in ("lon", "lat", "speed", "heading")], axis=1), "position_at as before")
    r = ukf.position_at(times, covariance=True)
    assert set(r) == {"position", "cov_km", "semi_major_km", "semi_minor_km", "orientation_deg"}
    _same_bits(r["position"], plain, "position")
    ref = batch.position_covariance(one, np.zeros(6, dtype=np.int32), times)
    for k in ("cov_km", "semi_major_km", "semi_minor_km", "orientation_deg"):
        _same_bits(r[k], ref[k], ("drop-in", k))
    assert np.isnan(r["cov_km"][-1]).all() and (r["semi_major_km"][:-1] >= r["semi_minor_km"][:-1]).all()
    with pytest.raises(ValueError, match="leave n_samples at 0"):
        ukf.position_at(times, n_samples=4, covariance=True)
