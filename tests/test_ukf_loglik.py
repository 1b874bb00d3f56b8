"""Innovation log-likelihood of the forward pass (include/ste.h: ste_ukf_forward_loglik_f64; DESIGN.md, "Innovation
log-likelihood"): the C ABI's declarations and refusals, a NumPy restatement of l_u checked against scipy, where the
likelihood of a synthetic fleet peaks over an R grid, and on the GPU the device values against the restatement and the
bit-identities the header promises."""
import ctypes as C
import dataclasses
import os
import re
import types

import numpy as np
import pytest
from conftest import ROOT, load_cases

GOLDEN = os.path.join(ROOT, "tests", "golden")
PINV_RCOND = 1e-15  # ste_math.h kPinvRcond = np.linalg.pinv's default


# ----------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------
def lik_terms(S, y):
    """(nis, sum of log of the kept eigenvalues, rank) of one update: the eigenvalues np.linalg.pinv keeps
    (|lambda| > 1e-15 max |lambda|), nis = y^T pinv(S) y."""
    S = np.asarray(S, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    w = np.linalg.eigvalsh(0.5 * (S + S.T))
    keep = np.abs(w) > PINV_RCOND * np.abs(w).max()
    with np.errstate(invalid="ignore"):
        logdet = float(np.sum(np.log(w[keep])))
    nis = float(y @ np.linalg.pinv(S) @ y)
    return nis, logdet, int(keep.sum())


def lik_u(S, y):
    nis, logdet, r = lik_terms(S, y)
    return -0.5 * (nis + logdet + r * np.log(2.0 * np.pi)), nis, r


def restate_track(x0, P0, H, Q, R, dt, dts, z, sog_rate, cog_rate, noise_pred=None, noise_upd=None, robust=False,
                  chi_alpha=50.0, initial_update=True):
    """The oracle's forward_track with every update scored: predict_track, then S and y from the state the update starts
    from, then update_track (robust: with check_robustness's R, on the un-noised observation).  Returns loglik, the sum
    of |l_u|, dof, nupd, nis per history row (NaN without an update) and the filtered means."""
    from oracle import ukf_oracle as orc

    H, R = np.asarray(H, dtype=np.float64), np.asarray(R, dtype=np.float64)
    N = len(dt)
    W = orc.weight_matrix(4)
    x = np.asarray(x0, dtype=np.float64).reshape(-1, 1)
    P = np.asarray(P0, dtype=np.float64)
    out = dict(loglik=0.0, abs=0.0, dof=0, nupd=0, nis=np.full(N + 1, np.nan), means=[x[:, 0]])

    def update(x, P, zc, nz, row):
        Ru = orc.check_robustness(x, H, zc, P, R, chi_alpha=chi_alpha) if robust else R
        zn = zc.reshape(-1, 1) + (0.0 if nz is None else np.asarray(nz).reshape(-1, 1))
        S = H @ P @ H.T + Ru
        y = zn - H @ x
        y[3, 0] = (y[3, 0] + 180.0) % 360.0 - 180.0
        lu, nis, r = lik_u(S, y)
        out["loglik"] += lu
        out["abs"] += abs(lu)
        out["dof"] += r
        out["nupd"] += 1
        out["nis"][row] = nis
        return orc.update_track(x, P, H, Ru, zc.copy(), nz)

    if initial_update:
        x, P = update(x, P, z[:, 0], None if noise_upd is None else noise_upd[0], 0)
    ui, time, cums = 0, 0, np.cumsum(dts)
    for k, d in enumerate(dt):
        x, P = orc.predict_track(x, P, Q, W, d, sog_rate[ui], cog_rate[ui], None if noise_pred is None else noise_pred[k])
        time += d
        if time in cums:
            ui += 1
            x, P = update(x, P, z[:, ui], None if noise_upd is None else noise_upd[k + 1], k + 1)
        out["means"].append(x[:, 0])
    out["means"] = np.asarray(out["means"])
    return out


def fleet_restatement(sb, substeps, H, Q, R, P0):
    """restate_track over every track of a synthetic batch (pack_uniform's schedule: dt = dts / substeps)."""
    res = []
    for b in range(sb.z.shape[0]):
        dt = np.repeat(sb.dts[b] / substeps, substeps)
        res.append(restate_track(sb.z[b][:, 0], P0, H, Q, R, dt, sb.dts[b], sb.z[b], sb.sog_rate[b], sb.cog_rate[b]))
    return res


# The fleet of the R-grid tests: 16 synthetic tracks of 26 fixes an hour apart, 4 filter steps per gap, filtered with the
# examples' H, Q and P0 while R's lon / lat variance runs over a factor-2 grid around the generator's observation noise
# (synthetic.make_batch: 0.05 deg std, 0.0025 deg^2).
FLEET = dict(ntracks=16, nobs=26, gap_h=1.0, seed0=100)
FLEET_SUBSTEPS = 4
R_FACTORS = (1 / 16, 1 / 8, 1 / 4, 1 / 2, 1, 2, 4, 8, 16)
R_GRID = [0.0025 * f for f in R_FACTORS]


def fleet_candidates():
    from track_estimators import synthetic

    _, Q, _, _ = synthetic.example_matrices()
    return [(Q, np.diag([r, r, 0.0, 0.0])) for r in R_GRID]


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_entry_point_and_struct_mirror_matches():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    assert re.search(r"^int ste_ukf_forward_loglik_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_loglik_f64\* l, "
                     r"void\* stream\);", hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_ukf_loglik_f64 {"): hdr.index("} ste_ukf_loglik_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double|size_t|void)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteUkfLoglikF64._fields_] == ["loglik", "dof", "nupd", "nis"]
    assert C.sizeof(binding.SteUkfLoglikF64) == 32
    assert "ste_ukf_forward_loglik_f64" in binding.SYMBOLS
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340


def _batch(binding, keep):
    """A batch struct that passes every NULL check; its pointers are never dereferenced (argument errors come first)."""
    s = binding.SteUkfBatchF64()
    s.B, s.Nmax, s.Tmax, s.n = 8, 256, 4, 4
    s.w0, s.wi, s.fan_scale = -1.0 / 3.0, 1.0 / 6.0, 3.0
    m = np.eye(4)
    keep.append(m)
    s.H = s.Q = s.R = m.ctypes.data
    for name in ("x0", "P0", "dt", "sog_rate", "cog_rate", "upd_idx", "z", "fwd_mean", "fwd_cov", "status"):
        setattr(s, name, 0x1000)
    return s


def test_refusals_before_any_launch():
    """Every refusal of the header returns STE_EINVAL (-1) with its reason.  No GPU is needed: a launch on a machine without
    one would return STE_ELAUNCH (-2), so -1 shows the call stopped before launching."""
    from track_estimators._hip import binding

    lib, keep = binding.load(), []
    l = binding.SteUkfLoglikF64(0x2000, 0x2000, 0x2000, None)

    def call(s, lk):
        rc = lib.ste_ukf_forward_loglik_f64(None if s is None else C.byref(s), None if lk is None else C.byref(lk), None)
        return rc, lib.ste_last_error().decode()

    rc, msg = call(None, l)
    assert rc == -1 and "batch pointer is NULL" in msg
    s = _batch(binding, keep)
    s.flags = binding.STE_FLAG_LANES_4
    rc, msg = call(s, l)
    assert rc == -1 and "STE_FLAG_LANES_4" in msg and "lane-per-track" in msg
    for b, e in ((64, 0), (0, 128), (64, 256)):
        s = _batch(binding, keep)
        s.step_begin, s.step_end = b, e
        rc, msg = call(s, l)
        assert rc == -1 and "time slices" in msg, (b, e, msg)
    for b, e in ((0, 0), (0, 256)):  # a whole pass may name its end
        s = _batch(binding, keep)
        s.step_begin, s.step_end, s.B = b, e, 0  # (B = 0 so that the call still stops before a launch)
        rc, msg = call(s, l)
        assert rc == -1 and "B must be > 0" in msg
    rc, msg = call(_batch(binding, keep), None)
    assert rc == -1 and "likelihood outputs (l) are NULL" in msg
    rc, msg = call(_batch(binding, keep), binding.SteUkfLoglikF64(None, 0x2000, 0x2000, 0x2000))
    assert rc == -1 and "l->loglik is required" in msg
    for name in ("fwd_mean", "fwd_cov"):
        s = _batch(binding, keep)
        setattr(s, name, None)
        rc, msg = call(s, l)
        assert rc == -1 and "both (histories) or neither" in msg, name
    s = _batch(binding, keep)
    s.fwd_mean = s.fwd_cov = None
    s.rts_work = 0x3000
    rc, msg = call(s, l)
    assert rc == -1 and "rts_work needs the histories" in msg
    # the usual batch checks, with and without histories
    for hist in (True, False):
        s = _batch(binding, keep)
        if not hist:
            s.fwd_mean = s.fwd_cov = None
        s.n = 3
        rc, msg = call(s, l)
        assert rc == -1 and "state dimension" in msg
        s = _batch(binding, keep)
        if not hist:
            s.fwd_mean = s.fwd_cov = None
        s.status = None
        rc, msg = call(s, l)
        assert rc == -1 and "status" in msg
        s = _batch(binding, keep)
        if not hist:
            s.fwd_mean = s.fwd_cov = None
        s.track_stride = 4
        rc, msg = call(s, l)
        assert rc == -1 and "track_stride" in msg


@pytest.mark.parametrize("rank", [2, 4])
def test_restated_lu_is_the_gaussian_density_on_the_range_of_S(rank):
    """l_u = -1/2 (y^T S^+ y + sum log lambda_i + r log 2 pi) is scipy's log density of N(0, S) (allow_singular) at y_p, the
    projection of y onto the range of S: scipy returns -inf for a y with components outside the support, and the shipped
    H = diag(1, 1, 0, 0) always leaves y[2], y[3] there."""
    from scipy.stats import multivariate_normal

    rng = np.random.default_rng(5 + rank)
    for _ in range(20):
        A = rng.normal(size=(4, 4))
        P = A @ A.T + 0.1 * np.eye(4)
        if rank == 2:
            H = np.diag([1.0, 1.0, 0.0, 0.0])
            R = np.diag([0.0025, 0.0025, 0.0, 0.0])
            R[0, 1] = R[1, 0] = 0.0007
        else:
            H = np.eye(4)
            H[0, 2] = 0.3
            B2 = rng.normal(size=(4, 4))
            R = 0.01 * (B2 @ B2.T) + 1e-3 * np.eye(4)
        S = H @ P @ H.T + R
        y = rng.normal(size=4) * 2.0
        lu, nis, r = lik_u(S, y)
        assert r == rank
        w, V = np.linalg.eigh(S)
        Vk = V[:, np.abs(w) > PINV_RCOND * np.abs(w).max()]
        yp = Vk @ (Vk.T @ y)
        ref = multivariate_normal(np.zeros(4), S, allow_singular=True).logpdf(yp)
        assert abs(lu - ref) <= 1e-10 * max(1.0, abs(ref)), (lu, ref)
        if rank == 2:
            assert multivariate_normal(np.zeros(4), S, allow_singular=True).logpdf(y) == -np.inf
    # a kept eigenvalue <= 0 makes l_u NaN
    assert np.isnan(lik_u(np.diag([1.0, -0.5, 0.0, 0.0]), np.ones(4))[0])


def test_restatement_reproduces_the_oracle_forward_pass():
    """The restatement filters exactly as the oracle's forward_track does (it calls the same predict_track / update_track),
    so its S and y are those of the reference's own pass."""
    from oracle import ukf_oracle as orc

    c = load_cases("ukf_synthetic.npz")[1]
    nz = c["mode"] != "zero"
    kw = dict(noise_pred=c["noise_pred"], noise_upd=c["noise_upd"]) if nz else {}
    r = restate_track(c["x0"], c["P0"], c["H"], c["Q"], c["R"], c["dt"], c["dts"], c["z"], c["sog_rate"], c["cog_rate"], **kw)
    m, _ = orc.forward_track(c["x0"], c["P0"], c["H"], c["Q"], c["R"], c["dt"], c["dts"], c["z"], c["sog_rate"],
                             c["cog_rate"], **kw)
    assert np.array_equal(r["means"], m)
    assert r["nupd"] == 1 + int(c["fires"].sum()) and r["dof"] == 2 * r["nupd"]
    assert np.isfinite(r["loglik"])


def test_oracle_fleet_likelihood_peaks_at_the_generators_noise():
    """Over R = r diag(1, 1, 0, 0) with r on a factor-2 grid from 0.0025 / 16 to 0.0025 * 16, the fleet-summed innovation
    log-likelihood of the oracle peaks at r = 0.0025 = 0.05^2, the variance of the lon / lat noise synthetic.make_batch
    adds.  Why it lands there and not beside it: the filter is handed the generator's own speed and course rates, so the
    process model's error is the difference between the generator's one-hour legs at constant speed and course and the
    filter's four quarter-hour steps with continuously applied rates -- plus Q's 1e-4 deg^2 per step, about 4e-4 deg^2
    per gap in H P- H^T.  Both are small beside 0.0025 but not negligible, so the peak is broad and, on a factor-2 grid,
    still at the generator's value; the shipped R (0.25, 100x) scores far below it."""
    from track_estimators import synthetic

    H, Q, R0, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(**FLEET)
    tot = np.array([sum(t["loglik"] for t in fleet_restatement(sb, FLEET_SUBSTEPS, H, Qc, Rc, P0))
                    for Qc, Rc in fleet_candidates()])
    assert np.all(np.isfinite(tot))
    assert R_GRID[int(np.argmax(tot))] == 0.0025, dict(zip(R_GRID, tot))
    # unimodal on the grid: rises to the peak, falls after it
    k = int(np.argmax(tot))
    assert np.all(np.diff(tot[: k + 1]) > 0) and np.all(np.diff(tot[k:]) < 0)
    shipped = sum(t["loglik"] for t in fleet_restatement(sb, FLEET_SUBSTEPS, H, Q, R0, P0))
    assert shipped < tot[-1] < tot[k]


def test_best_noise_leaves_out_unusable_tracks():
    from track_estimators import batch
    from track_estimators._hip import binding

    ll = np.array([[-10.0, -5.0, np.nan, -1.0],
                   [-9.0, -6.0, -1.0, -100.0],
                   [-12.0, -7.0, -2.0, -3.0]])
    status = np.zeros_like(ll, dtype=np.int32)
    status[2, 3] = binding.STE_STATUS_NAN
    g = batch.LogLikelihood(loglik=ll, dof=np.zeros_like(status), nupd=np.zeros_like(status), status=status)
    fleet = batch.best_noise(g)
    # tracks 2 (NaN under candidate 0) and 3 (STE_STATUS_NAN under candidate 2) leave every sum
    assert fleet.excluded == 2
    assert np.allclose(fleet.loglik, [-15.0, -15.0, -19.0])
    assert fleet.index == 0  # the first of equal sums
    per = batch.best_noise(g, per_track=True)
    assert per.excluded == 0
    assert per.index.tolist() == [1, 0, 1, 0]
    assert per.loglik.tolist() == [-9.0, -5.0, -1.0, -1.0]
    g.loglik = np.full((2, 1), np.inf)
    g.status = np.zeros((2, 1), dtype=np.int32)
    per = batch.best_noise(g, per_track=True)
    assert per.index.tolist() == [-1] and per.excluded == 1
    # every track left out: no candidate wins the fleet either
    fleet = batch.best_noise(g)
    assert fleet.index == -1 and fleet.excluded == 1 and np.all(np.isnan(fleet.loglik))


def test_grid_refuses_bad_candidates_before_touching_the_device():
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(synthetic.make_batch(2, nobs=5), 1, H, Q, R, P0)
    bad = np.diag([1.0, 1.0, 0.0, 0.0])
    bad[0, 1] = 0.5
    with pytest.raises(ValueError, match="R must be symmetric"):
        batch.log_likelihood_grid(hb, [(Q, R), (Q, bad)])
    with pytest.raises(ValueError, match="Q must be 4x4"):
        batch.log_likelihood_grid(hb, [(np.eye(3), R)])
    with pytest.raises(ValueError, match="no candidates"):
        batch.log_likelihood_grid(hb, [])


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
# Tolerance of the device's loglik against the restatement, relative to sum |l_u| over the track.  The argument: l_u is a
# smooth function of the state the update starts from; to first order it moves by (S^+ y) . dy for a change dy of the
# innovation and by 1/2 tr(S^+ dS (S^+ y y^T - I)) for a change dS, i.e. by the state's own relative change times terms of
# the size of nis + r -- the size of |l_u| itself.  The device histories agree with the restatement's to the parity bound of
# tests/test_hip_parity.py (1e-6 relative, MEAN_TOL), and each test below measures that agreement on the case it scores
# (_hist_err) and asserts it, so the same 1e-6 bounds the likelihood's relative error.  Measured on an MI355X: histories to
# 2e-11, loglik to 2.4e-13 of sum |l_u|, nis to 4.5e-13 ("Innovation log-likelihood").
LIK_RTOL = 1e-6
HIST_RTOL = 1e-6


def _track(c):
    return types.SimpleNamespace(z=c["z"], dts=c["dts"], sog_rate=c["sog_rate"], cog_rate=c["cog_rate"])


def _hist_err(dev_means, ref_means):
    return float(np.max(np.abs(dev_means - ref_means) / np.maximum(np.abs(ref_means), 1e-12)))


def _check_track(res, b, ref, N, means=None, nis=True):
    """Device result of track b against one restated track; returns (relative loglik error, nis error)."""
    assert int(res.nupd[b]) == ref["nupd"] and int(res.dof[b]) == ref["dof"]
    if means is not None:
        assert _hist_err(means[b, : N + 1], ref["means"]) < HIST_RTOL
    if np.isnan(ref["loglik"]):
        assert np.isnan(res.loglik[b])
        return 0.0, 0.0
    err = abs(float(res.loglik[b]) - ref["loglik"]) / ref["abs"]
    assert err < LIK_RTOL, (b, res.loglik[b], ref["loglik"], err)
    nerr = 0.0
    if nis:
        dn, rn = res.nis[b, : N + 1], ref["nis"]
        assert np.array_equal(np.isnan(dn), np.isnan(rn))
        f = ~np.isnan(rn)
        nerr = float(np.max(np.abs(dn[f] - rn[f]) / np.maximum(np.abs(rn[f]), 1.0))) if f.any() else 0.0
        assert nerr < LIK_RTOL
    return err, nerr


def _golden_cases():
    out = []
    for name, n in (("ukf_synthetic.npz", 10), ("ukf_edge.npz", 3), ("ukf_ship_01203823.npz", 2)):
        out += [(name, i) for i in range(n)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", _golden_cases())
def test_golden_cases_match_the_restatement(name, i):
    """ukf_synthetic (zero and replayed noise), ukf_edge (dense H and R: the general update route) and the real ship, each
    as a batch of one: loglik, dof, nupd and every NIS row against the restatement of the reference's own pass."""
    from track_estimators import batch

    c = load_cases(name)[i]
    nz = None if c["mode"] == "zero" else dict(noise_pred=c["noise_pred"], noise_upd=c["noise_upd"], noise_rts=c["noise_rts"])
    hb = batch.pack_tracks([_track(c)], [c["dt"]], [c["x0"]], c["H"], c["Q"], c["R"], c["P0"],
                           noise=None if nz is None else [nz])
    db = batch.DeviceBatch(hb)
    res = db.log_likelihood(nis=True)
    means, _ = db.filtered()
    kw = {} if nz is None else dict(noise_pred=c["noise_pred"], noise_upd=c["noise_upd"])
    ref = restate_track(c["x0"], c["P0"], c["H"], c["Q"], c["R"], c["dt"], c["dts"], c["z"], c["sog_rate"],
                        c["cog_rate"], **kw)
    err = _check_track(res, 0, ref, len(c["dt"]), means)
    print(f"[loglik] {name}[{i}] mode={c['mode']} loglik={res.loglik[0]:.6f} rel err {err[0]:.2e} nis err {err[1]:.2e} "
          f"hist err {_hist_err(means[0, : len(c['dt']) + 1], ref['means']):.2e}")


@pytest.mark.gpu
def test_robust_runs_match_the_restatement():
    """The robust runs of tests/golden/robust.npz (R rescaled per update by check_robustness; closed-form route) and the
    same runs through the general route (an R with a tiny off-block entry the closed form does not take)."""
    from track_estimators import batch

    g = np.load(os.path.join(GOLDEN, "robust.npz"))
    for general in (False, True):
        R = np.array(g["R"], dtype=np.float64)
        if general:
            R[2, 2] = 1e-300  # not zero: leaves the closed form's structure; S keeps rank 2 (1e-300 < 1e-15 max|lambda|)
        for ci in range(int(g["nruns"])):
            z, dts, dt = g[f"run{ci}_z"], g[f"run{ci}_dts"], g[f"run{ci}_dt"]
            tr = types.SimpleNamespace(z=z, dts=dts, sog_rate=g[f"run{ci}_sog_rate"], cog_rate=g[f"run{ci}_cog_rate"])
            hb = batch.pack_tracks([tr], [dt], [z[:, 0]], g["H"], g["Q"], R, g["P0"])
            hb.robust = True
            db = batch.DeviceBatch(hb)
            res = db.log_likelihood(nis=True)
            means, _ = db.filtered()
            ref = restate_track(z[:, 0], g["P0"], g["H"], g["Q"], R, dt, dts, z, tr.sog_rate, tr.cog_rate, robust=True)
            err = _check_track(res, 0, ref, len(dt), means)
            print(f"[loglik] robust run {ci} general={general} rel err {err[0]:.2e} nis err {err[1]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("initial_update", [True, False], ids=["initial-update", "no-initial-update"])
def test_ragged_batch_matches_the_restatement(initial_update):
    """All zero-noise synthetic golden cases in one ragged, length-bucketed batch (several waves, different N and T), with
    and without the initial update; NIS rows past a track's end keep what was there."""
    from track_estimators import batch
    from track_estimators._hip import binding

    cs = [c for c in load_cases("ukf_synthetic.npz") if c["mode"] == "zero"]
    reps = 20
    tracks = [_track(c) for c in cs] * reps
    hb = batch.pack_tracks(tracks, [c["dt"] for c in cs] * reps, [c["x0"] for c in cs] * reps, cs[0]["H"], cs[0]["Q"],
                           cs[0]["R"], cs[0]["P0"])
    hb.initial_update = initial_update
    assert len(set(hb.nsteps.tolist())) > 1
    refs = [restate_track(c["x0"], c["P0"], c["H"], c["Q"], c["R"], c["dt"], c["dts"], c["z"], c["sog_rate"],
                          c["cog_rate"], initial_update=initial_update) for c in cs]
    db = batch.DeviceBatch(hb)
    res = db.log_likelihood(nis=True)
    means, _ = db.filtered()
    worst = 0.0
    for b in range(hb.B):
        caller = int(hb.order[b]) if hb.order is not None else b
        ref = refs[caller % len(cs)]
        worst = max(worst, _check_track(res, b, ref, int(hb.nsteps[b]), means)[0])
    print(f"[loglik] ragged initial_update={initial_update}: worst rel err {worst:.2e}")

    # rows past nsteps are not written: the raw call on a sentinel-filled NIS buffer
    torch = db.torch
    sentinel = 12345.0
    nis = torch.full((hb.Nmax + 1, hb.B), sentinel, dtype=torch.float64, device=db.device)
    ll = torch.empty(hb.B, dtype=torch.float64, device=db.device)
    s = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
    lk = binding.SteUkfLoglikF64(ll.data_ptr(), None, None, nis.data_ptr())
    binding.check(db.lib.ste_ukf_forward_loglik_f64(C.byref(s), C.byref(lk), None), "ste_ukf_forward_loglik_f64")
    nis = nis.cpu().numpy()
    for b in range(hb.B):
        n = int(hb.nsteps[b])
        assert np.all(nis[n + 1:, b] == sentinel)
        assert not np.any(nis[: n + 1, b] == sentinel)
        assert np.array_equal(nis[: n + 1, b], res.nis[b, : n + 1], equal_nan=True)
        fired = np.concatenate([[initial_update], hb.upd_idx[:n, b] >= 0])
        assert np.array_equal(np.isnan(nis[: n + 1, b]), ~fired)
    assert np.array_equal(ll.cpu().numpy(), res.loglik)


def _bits_equal(a, b):
    """Two device tensors hold the same bytes (NaN-safe)."""
    return a.shape == b.shape and bool(np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)))


def _synthetic_hb(ntracks, seed0, R=None, nobs=26, substeps=4, robust=False):
    from track_estimators import batch, synthetic

    H, Q, R0, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(synthetic.make_batch(ntracks, nobs=nobs, seed0=seed0), substeps, H, Q, R0 if R is None else R, P0)
    hb.robust = robust
    return hb


GENERAL_R = np.array([[0.0025, 0.0004, 0.0, 0.0], [0.0004, 0.0025, 0.0, 0.0], [0.0, 0.0, 0.01, 0.0], [0.0, 0.0, 0.0, 0.5]])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["closed", "robust", "general"])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "full"])
def test_histories_bit_identical_to_the_lane_forward_pass(route, packed):
    """With histories, everything the call writes -- histories, rts_work, status -- is ste_ukf_forward_f64's with
    STE_FLAG_LANES_1, bit for bit (the batch doing the likelihood was built for the quad mapping), and the smoother after
    each gives the same bits; the likelihood-only pass gives the same likelihood bits as the pass with histories."""
    from track_estimators import batch

    R = GENERAL_R if route == "general" else np.diag([0.0025, 0.0025, 0.0, 0.0]) if route == "robust" else None
    hb = _synthetic_hb(200, 3, R=R, robust=route == "robust")
    a = batch.DeviceBatch(dataclasses.replace(hb, lanes=1), packed_cov=packed)
    b = batch.DeviceBatch(dataclasses.replace(hb, lanes=4), packed_cov=packed)
    for db in (a, b):
        for t in (db.fwd_mean, db.fwd_cov, db.sm_mean, db.sm_cov, db.rts_work):
            t.zero_()
        db.status.fill_(-1)
    a.forward()
    res = b.log_likelihood(nis=True)
    for name in ("fwd_mean", "fwd_cov", "rts_work", "status"):
        assert _bits_equal(getattr(a, name), getattr(b, name)), name
    a.backward()
    b.backward()
    for name in ("sm_mean", "sm_cov", "status"):
        assert _bits_equal(getattr(a, name), getattr(b, name)), name
    assert np.all(np.isfinite(res.loglik)) and np.all(res.nupd == 26)
    # the likelihood alone: same bits
    only = batch.log_likelihood_grid(hb, [(hb.Q, hb.R)], nis=True)
    assert np.array_equal(only.loglik[0].view(np.uint64), res.loglik.view(np.uint64))
    assert np.array_equal(only.nis[0].view(np.uint64), res.nis.view(np.uint64))
    assert np.array_equal(only.dof[0], res.dof) and np.array_equal(only.nupd[0], res.nupd)
    assert np.array_equal(only.status[0], res.status)


@pytest.mark.gpu
def test_window_of_a_resident_fleet_equals_a_batch_of_its_own():
    from track_estimators import batch

    fleet = batch.DeviceBatch(_synthetic_hb(200, 40))
    w = fleet.window(64, 150).log_likelihood(nis=True)
    own = batch.DeviceBatch(_synthetic_hb(86, 40 + 64)).log_likelihood(nis=True)
    for f in ("loglik", "nis"):
        assert np.array_equal(getattr(w, f).view(np.uint64), getattr(own, f).view(np.uint64)), f
    for f in ("dof", "nupd", "status"):
        assert np.array_equal(getattr(w, f), getattr(own, f)), f
    # the window wrote its columns of the fleet's histories
    fm = fleet.fwd_mean[..., 64:150].cpu().numpy()
    ref = batch.DeviceBatch(dataclasses.replace(_synthetic_hb(86, 40 + 64), lanes=1))  # the mapping the likelihood uses
    ref.forward()
    assert np.array_equal(fm.view(np.uint64), ref.fwd_mean.cpu().numpy().view(np.uint64))


def _grid_candidates():
    from track_estimators import synthetic

    _, Q, R, _ = synthetic.example_matrices()
    return [(Q, R), (Q * 4.0, np.diag([0.0025, 0.0025, 0.0, 0.0])), (Q, GENERAL_R)]


@pytest.mark.gpu
def test_grid_rows_equal_separate_calls():
    from track_estimators import batch

    hb = _synthetic_hb(150, 21)
    grid = batch.log_likelihood_grid(hb, _grid_candidates(), nis=True)
    assert grid.loglik.shape == (3, 150) and grid.nis.shape == (3, 150, hb.Nmax + 1)
    for k, (Q, R) in enumerate(_grid_candidates()):
        one = batch.DeviceBatch(dataclasses.replace(hb, Q=np.array(Q), R=np.array(R))).log_likelihood(nis=True)
        assert np.array_equal(grid.loglik[k].view(np.uint64), one.loglik.view(np.uint64)), k
        assert np.array_equal(grid.nis[k].view(np.uint64), one.nis.view(np.uint64)), k
        for f in ("dof", "nupd", "status"):
            assert np.array_equal(getattr(grid, f)[k], getattr(one, f)), (k, f)
    assert not np.array_equal(grid.loglik[0], grid.loglik[1])


@pytest.mark.gpu
def test_one_track_alone_equals_the_same_track_in_a_batch_of_1000():
    from track_estimators import batch

    j = 517
    big = batch.log_likelihood_grid(_synthetic_hb(1000, 7), _grid_candidates(), nis=True)
    one = batch.log_likelihood_grid(_synthetic_hb(1, 7 + j), _grid_candidates(), nis=True)
    assert np.array_equal(big.loglik[:, j].view(np.uint64), one.loglik[:, 0].view(np.uint64))
    assert np.array_equal(big.nis[:, j].view(np.uint64), one.nis[:, 0].view(np.uint64))
    assert np.array_equal(big.status[:, j], one.status[:, 0])


@pytest.mark.gpu
def test_device_grid_best_noise_equals_the_oracle_argmax():
    """The fleet of test_oracle_fleet_likelihood_peaks_at_the_generators_noise on the device: per-track loglik against the
    restatement, and best_noise picks the oracle's argmax (0.0025)."""
    from track_estimators import batch, synthetic

    H, _, _, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(**FLEET)
    cands = fleet_candidates()
    hb = batch.pack_uniform(sb, FLEET_SUBSTEPS, H, cands[0][0], cands[0][1], P0)
    grid = batch.log_likelihood_grid(hb, cands)
    tot = []
    worst = 0.0
    for k, (Q, R) in enumerate(cands):
        refs = fleet_restatement(sb, FLEET_SUBSTEPS, H, Q, R, P0)
        tot.append(sum(r["loglik"] for r in refs))
        for b, r in enumerate(refs):
            assert int(grid.nupd[k, b]) == r["nupd"] and int(grid.dof[k, b]) == r["dof"]
            err = abs(grid.loglik[k, b] - r["loglik"]) / r["abs"]
            worst = max(worst, err)
            assert err < LIK_RTOL
    choice = batch.best_noise(grid)
    assert choice.excluded == 0
    assert choice.index == int(np.argmax(tot)) and R_GRID[choice.index] == 0.0025
    per = batch.best_noise(grid, per_track=True)
    assert per.index.shape == (hb.B,) and per.excluded == 0
    print(f"[loglik] fleet grid: worst rel err {worst:.2e}; fleet sums {np.round(choice.loglik, 3).tolist()}")


@pytest.mark.gpu
def test_log_likelihood_on_a_stream_of_its_own():
    """DeviceBatch.log_likelihood(stream=...) on a fresh stream: the pass is ordered after the current stream's work and its
    results are read back only once it is done -- same bits as on the current stream, histories included."""
    import torch
    from track_estimators import batch

    hb = _synthetic_hb(300, 55)
    ref_db = batch.DeviceBatch(hb)
    ref = ref_db.log_likelihood(nis=True)
    for rep in range(3):
        db = batch.DeviceBatch(hb)
        side = torch.cuda.Stream(db.device)
        res = db.log_likelihood(stream=side, nis=True)
        for f in ("loglik", "nis"):
            assert np.array_equal(getattr(res, f).view(np.uint64), getattr(ref, f).view(np.uint64)), (rep, f)
        for f in ("dof", "nupd", "status"):
            assert np.array_equal(getattr(res, f), getattr(ref, f)), (rep, f)
        torch.cuda.current_stream(db.device).wait_stream(side)
        assert _bits_equal(db.fwd_mean, ref_db.fwd_mean) and _bits_equal(db.fwd_cov, ref_db.fwd_cov)


@pytest.mark.gpu
def test_batch_without_histories_refuses_history_calls():
    from track_estimators import batch

    db = batch.DeviceBatch(_synthetic_hb(70, 9), histories=False)
    for call in (db.forward, db.backward, db.run, db.filtered):
        with pytest.raises(ValueError, match="histories=False"):
            call()
    res = db.log_likelihood()  # the likelihood alone
    own = batch.DeviceBatch(_synthetic_hb(70, 9)).log_likelihood()
    assert np.array_equal(res.loglik.view(np.uint64), own.loglik.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["closed", "general"])
def test_non_finite_observation_makes_loglik_nan(route):
    """A NaN speed or course in one observation column poisons the update's state (0 * NaN in the gain's unused columns on
    the closed form, a real gain column on the general route): the track's loglik is NaN and STE_STATUS_NAN is set.
    Poisoned in the last column, the restatement sees the same NaN and every earlier count; poisoned mid-track, every later
    S is NaN, whose eigenvalues the pseudo-inverse does not keep, so those updates add to nupd and not to dof (ste.h)."""
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R0, P0 = synthetic.example_matrices()
    R = GENERAL_R if route == "general" else R0
    full_rank = 4 if route == "general" else 2
    sb = synthetic.make_batch(6, nobs=26, seed0=300)
    T = sb.z.shape[2]
    poison = {1: (T - 1, 2), 2: (T - 1, 3), 3: (10, 2), 4: (10, 3)}  # track: (observation column, component)
    for b, (col, comp) in poison.items():
        sb.z[b, comp, col] = np.nan
    hb = batch.pack_uniform(sb, 4, H, Q, R, P0)
    res = batch.DeviceBatch(hb).log_likelihood(nis=True)
    nupd = T  # the initial update and one per later column
    assert np.all(res.nupd == nupd)
    for b in range(6):
        if b not in poison:
            assert np.isfinite(res.loglik[b]) and res.dof[b] == full_rank * nupd and not (res.status[b] & 1)
            continue
        col, _ = poison[b]
        assert np.isnan(res.loglik[b]) and (res.status[b] & binding.STE_STATUS_NAN), b
        assert res.dof[b] == full_rank * (col + 1), (b, res.dof[b])  # updates 0 .. col keep a finite S
        if col == T - 1:
            dt = np.repeat(sb.dts[b] / 4, 4)
            ref = restate_track(sb.z[b][:, 0], P0, H, Q, R, dt, sb.dts[b], sb.z[b], sb.sog_rate[b], sb.cog_rate[b])
            assert np.isnan(ref["loglik"]) and ref["nupd"] == nupd and ref["dof"] == res.dof[b]
            assert np.isnan(res.nis[b, -1]) and np.isfinite(res.nis[b, :-1][~np.isnan(ref["nis"][:-1])]).all()
