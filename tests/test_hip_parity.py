"""
Parity of the HIP path (through the C ABI) with the golden vectors of the reference and with the oracle.
Needs a real MI355X: run with ``pytest -m gpu``.

Tolerances (BASELINE.json north_star / SURVEY.md §8d): state means <= 1e-6 relative element-wise
(|d| / max(|ref|, 1e-12)); covariances max|dP| <= 1e-5 * max|P| per matrix.
"""
import types

import numpy as np
import pytest
from conftest import load_cases

pytestmark = pytest.mark.gpu

MEAN_TOL = 1e-6
COV_TOL = 1e-5

@pytest.fixture(params=[1, 4, 0], ids=["lane-per-track", "quad-per-track", "auto"], autouse=True)
def lanes_per_track(request):
    """Every parity test runs with both forward-kernel lane mappings (include/ste.h: STE_FLAG_LANES_1 / _4, a per-call
    flag; ``batch.default_lanes`` is what batches that do not name a mapping get)."""
    from track_estimators import batch

    prev = batch.default_lanes
    batch.default_lanes = request.param
    yield request.param
    batch.default_lanes = prev


@pytest.fixture(params=[0, 0x400], ids=["smoother-by-size", "one-kernel-smoother"], autouse=True)
def smoother_form(request):
    """The goldens are small batches, which smooth in the two-kernel form by default (all gains at once, then the lean
    recurrence: include/ste.h ``tuning``); every parity test also runs with the one-kernel smoother the bench batch uses."""
    from track_estimators import batch

    prev = batch.default_tuning
    batch.default_tuning = request.param
    yield request.param
    batch.default_tuning = prev


def test_the_fixtures_reach_the_batch(lanes_per_track, smoother_form):
    """What the two fixtures set is what a batch that names neither is built with: the lane flags and the tuning word of
    its struct differ between the fixtures' parameters, so no parity test runs one variant under several names."""
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R, P0 = synthetic.example_matrices()
    db = batch.DeviceBatch(batch.pack_uniform(synthetic.make_batch(2, nobs=3, gap_h=1.0, seed0=1), 1, H, Q, R, P0))
    lane_flags = {1: binding.STE_FLAG_LANES_1, 4: binding.STE_FLAG_LANES_4, 0: 0}
    assert len(set(lane_flags.values())) == 3
    assert db.struct.flags & (binding.STE_FLAG_LANES_1 | binding.STE_FLAG_LANES_4) == lane_flags[lanes_per_track]
    assert db.struct.tuning == smoother_form


CASES = [("ukf_synthetic.npz", i) for i in range(10)] + [("ukf_edge.npz", i) for i in range(3)] + [
    ("ukf_ship_01203823.npz", i) for i in range(2)
]


def mean_err(a, ref):
    return float(np.max(np.abs(a - ref) / np.maximum(np.abs(ref), 1e-12)))


def cov_err(a, ref):
    scale = np.max(np.abs(ref), axis=(-1, -2), keepdims=True)
    return float(np.max(np.abs(a - ref) / scale))


def _track(c):
    return types.SimpleNamespace(z=c["z"], dts=c["dts"], sog_rate=c["sog_rate"], cog_rate=c["cog_rate"])


def _noise(c):
    if c["mode"] == "zero":
        return None
    return dict(noise_pred=c["noise_pred"], noise_upd=c["noise_upd"], noise_rts=c["noise_rts"])


@pytest.mark.parametrize("fuse", [True, False], ids=["work-rows", "standalone-smoother"])
@pytest.mark.parametrize("i", range(5))
def test_golden_ill_conditioned_smoother_gains(i, fuse):
    """Reference runs whose smoother inverts a P_b of condition number 1e2 ... 3e13 (tests/golden/ukf_illcond.npz: tiny
    process noise, a prior that knows speed and heading far better than position, long steps; cond(P_b) of the reference's
    own pass is in the fixture).  The factorisation route (pivots >= 1e-7 of the largest diagonal entry) and the
    eigenvalue route with NumPy's cutoff must both stay inside the parity bound through cond ~ 1e10; at 3e13 the
    reference's own answer moves by 2e-6 when its arithmetic is merely reordered (the vectorised oracle,
    test_oracle_golden), so that case is held to 1e-4 / 1e-5."""
    from track_estimators import batch

    c = load_cases("ukf_illcond.npz")[i]
    hb = batch.pack_tracks([_track(c)], [c["dt"]], [c["x0"]], c["H"], c["Q"], c["R"], c["P0"])
    out = batch.run_batch(hb, fuse_gains=fuse)
    N = len(c["dt"])
    mtol = MEAN_TOL if c["cond_pb"].max() < 1e11 else 1e-4
    assert mean_err(out["means"][0, : N + 1], c["means"]) < MEAN_TOL
    assert cov_err(out["covs"][0, : N + 1], c["covs"]) < COV_TOL
    assert mean_err(out["means_smoothed"][0, : N + 1], c["means_smoothed"]) < mtol, c["cond_pb"].max()
    assert cov_err(out["covs_smoothed"][0, : N + 1], c["covs_smoothed"]) < COV_TOL
    assert not (out["status"][0] & 0x1)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused-gains", "standalone-smoother"])
@pytest.mark.parametrize("name,i", CASES)
def test_golden_single_track(name, i, fuse):
    """Each reference-generated case as a batch of one, zero and replayed noise; with the smoother gains produced by
    the forward pass (rts_work) and with the stand-alone smoother kernel that recomputes them."""
    from track_estimators import batch

    c = load_cases(name)[i]
    nz = _noise(c)
    hb = batch.pack_tracks([_track(c)], [c["dt"]], [c["x0"]], c["H"], c["Q"], c["R"], c["P0"],
                           noise=None if nz is None else [nz])
    out = batch.run_batch(hb, fuse_gains=fuse)
    N = len(c["dt"])
    assert mean_err(out["means"][0, : N + 1], c["means"]) < MEAN_TOL
    assert cov_err(out["covs"][0, : N + 1], c["covs"]) < COV_TOL
    assert mean_err(out["means_smoothed"][0, : N + 1], c["means_smoothed"]) < MEAN_TOL
    assert cov_err(out["covs_smoothed"][0, : N + 1], c["covs_smoothed"]) < COV_TOL
    expect_clamped = name == "ukf_edge.npz" and i == 2  # indefinite prior
    assert bool(out["status"][0] & 0x2) == expect_clamped
    assert not (out["status"][0] & 0x5)


def test_golden_ragged_batch():
    """All zero-noise golden cases with the example matrices in ONE ragged batch (different N and T per track),
    replicated so that several waves and partially filled waves are exercised."""
    from track_estimators import batch

    cs = [c for c in load_cases("ukf_synthetic.npz") if c["mode"] == "zero"]
    reps = 30
    tracks = [_track(c) for c in cs] * reps
    hb = batch.pack_tracks(tracks, [c["dt"] for c in cs] * reps, [c["x0"] for c in cs] * reps, cs[0]["H"], cs[0]["Q"],
                           cs[0]["R"], cs[0]["P0"])
    assert hb.B == len(cs) * reps and len(set(hb.nsteps.tolist())) > 1
    out = batch.run_batch(hb)
    for b in range(hb.B):
        c = cs[b % len(cs)]
        N = len(c["dt"])
        assert mean_err(out["means"][b, : N + 1], c["means"]) < MEAN_TOL
        assert cov_err(out["covs"][b, : N + 1], c["covs"]) < COV_TOL
        assert mean_err(out["means_smoothed"][b, : N + 1], c["means_smoothed"]) < MEAN_TOL
        assert cov_err(out["covs_smoothed"][b, : N + 1], c["covs_smoothed"]) < COV_TOL
    # identical tracks in different batch positions give identical bits (no cross-track coupling)
    for b in range(len(cs), hb.B):
        N = out["nsteps"][b]
        assert np.array_equal(out["means_smoothed"][b, : N + 1], out["means_smoothed"][b % len(cs), : N + 1])


@pytest.mark.parametrize("B,nobs,s", [(1, 11, 2), (64, 26, 4), (65, 26, 4), (1000, 51, 2)])
def test_synthetic_vs_oracle(B, nobs, s):
    """Seeded synthetic batches vs the vectorised oracle, at sizes the oracle finishes in seconds."""
    from oracle import ukf_oracle as orc
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(B, nobs=nobs, gap_h=1.0, seed0=1234)
    hb = batch.pack_uniform(sb, s, H, Q, R, P0)
    out = batch.run_batch(hb)
    fires = hb.upd_idx.T >= 0
    zidx = np.where(fires, hb.upd_idx.T, 0)
    ridx = np.cumsum(fires, axis=1) - fires
    m, P = orc.forward_batch(hb.x0.T, P0, H, Q, R, hb.dt.T, fires, zidx, ridx, sb.z, sb.sog_rate, sb.cog_rate)
    rr = np.broadcast_to(batch.rts_rate_index(hb.Nmax + 1, nobs - 1, nobs), (B, hb.Nmax))
    sm, sP = orc.backward_batch(m, P, Q, hb.dt.T, rr, sb.sog_rate, sb.cog_rate)
    assert not out["status"].any()
    assert mean_err(out["means"], m) < MEAN_TOL
    assert cov_err(out["covs"], P) < COV_TOL
    assert mean_err(out["means_smoothed"], sm) < MEAN_TOL
    assert cov_err(out["covs_smoothed"], sP) < COV_TOL


def test_fused_and_standalone_smoother_agree():
    """The two smoother formulations are the same arithmetic in a different place: they agree far inside the parity
    tolerance on a batch that fills several waves."""
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(300, nobs=41, gap_h=1.0, seed0=77)
    hb = batch.pack_uniform(sb, 4, H, Q, R, P0)
    a = batch.run_batch(hb, fuse_gains=True)
    b = batch.run_batch(hb, fuse_gains=False)
    assert np.array_equal(a["means"], b["means"]) and np.array_equal(a["covs"], b["covs"])
    assert mean_err(a["means_smoothed"], b["means_smoothed"]) < 1e-9
    assert cov_err(a["covs_smoothed"], b["covs_smoothed"]) < 1e-9


def test_single_function_kernels():
    """geodetic_dynamics and compute_sigma_points through the C ABI vs the reference's known answers."""
    import ctypes as C
    import os

    import torch
    from conftest import GOLDEN
    from track_estimators._hip import binding

    lib = binding.require_gpu()
    k = np.load(os.path.join(GOLDEN, "kats.npz"))
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x = up(k["gd_x"].T)
    dt, sr, cr = up(k["gd_dt"]), up(k["gd_sr"]), up(k["gd_cr"])
    out = torch.empty_like(x)
    binding.check(lib.ste_geodetic_dynamics_f64(64, x.data_ptr(), dt.data_ptr(), sr.data_ptr(), cr.data_ptr(),
                                                out.data_ptr(), None), "geodetic")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy().T, k["gd_y"], rtol=1e-13, atol=1e-12)

    n = len(k["sp_x"])
    xs = up(k["sp_x"].T)
    Ps = up(k["sp_P"].reshape(n, 16).T)
    sig = torch.empty((9, 4, n), dtype=torch.float64, device=dev)
    for scale, key in ((4.0 / (1 - (1 - 4 / 3.0)), "sp_sig_weighted"), (4.0, "sp_sig_unweighted")):
        binding.check(lib.ste_sigma_points_f64(n, xs.data_ptr(), Ps.data_ptr(), C.c_double(scale), sig.data_ptr(), None),
                      "sigma_points")
        torch.cuda.synchronize()
        got = sig.cpu().numpy().transpose(2, 1, 0)  # (n, 4, 9) like the reference's (n_state, n_sigma)
        np.testing.assert_allclose(got, k[key], rtol=0, atol=1e-11)


def test_full_size_batch_properties():
    """BASELINE.json configs[1] at full size (10 000 tracks x 500 steps) through size-independent properties:
    no status flags, identical tracks in different batch slots give identical bits, the two lane mappings agree, and 1 024
    tracks match the oracle in all four histories (filtered and smoothed, means and covariances) for both mappings
    (was 256; bench.py's own cross-check of 3 072 tracks is not a test)."""
    from oracle import ukf_oracle as orc
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    nuniq, B = 2500, 10_000
    sbu = synthetic.make_batch(nuniq, nobs=126, gap_h=1.0, seed0=10_000)
    idx = np.concatenate([np.arange(nuniq), np.random.default_rng(0).permutation(np.arange(nuniq).repeat(3))])
    sb = synthetic.SyntheticBatch(**{f.name: getattr(sbu, f.name)[idx] for f in __import__("dataclasses").fields(sbu)})
    hb = batch.pack_uniform(sb, 4, H, Q, R, P0)
    assert hb.B == B and hb.Nmax == 500
    res, full, nchk = {}, {}, 1024
    for lanes in (1, 4):
        hb.lanes = lanes
        db = batch.DeviceBatch(hb)
        db.run()
        db.torch.cuda.synchronize()
        assert not db.status_host().any()
        res[lanes] = db.sm_mean.cpu().numpy()  # [N+1][4][B]
        full[lanes] = db.download(("means", "covs", "means_smoothed", "covs_smoothed"), db.torch.arange(nchk, device=db.device))
        first = np.full(nuniq, -1)
        for slot, src in enumerate(idx):
            if first[src] < 0:
                first[src] = slot
        dup = np.arange(B)[first[idx] != np.arange(B)]
        assert np.array_equal(res[lanes][:, :, dup], res[lanes][:, :, first[idx[dup]]])
        del db
    a, b = res[1], res[4]
    assert np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-12)) < 1e-7
    n = nchk
    fires = hb.upd_idx.T[:n] >= 0
    zidx = np.where(fires, hb.upd_idx.T[:n], 0)
    ridx = np.cumsum(fires, axis=1) - fires
    m, P = orc.forward_batch(hb.x0.T[:n], P0, H, Q, R, hb.dt.T[:n], fires, zidx, ridx, sb.z[:n], sb.sog_rate[:n], sb.cog_rate[:n])
    rr = np.broadcast_to(batch.rts_rate_index(501, 125, 126), (n, 500))
    sm, sP = orc.backward_batch(m, P, Q, hb.dt.T[:n], rr, sb.sog_rate[:n], sb.cog_rate[:n])
    got = res[4][:, :, :n].transpose(2, 0, 1)
    assert mean_err(got, sm) < MEAN_TOL
    for lanes in (1, 4):  # all four histories at full size (was smoothed means of 48 tracks)
        f = full[lanes]
        assert mean_err(f["means"], m) < MEAN_TOL and mean_err(f["means_smoothed"], sm) < MEAN_TOL, lanes
        assert cov_err(f["covs"], P) < COV_TOL and cov_err(f["covs_smoothed"], sP) < COV_TOL, lanes


def test_degenerate_shapes():
    """Tracks with zero steps, a single observation, and batches that do not fill a wave or a quad group."""
    import types

    from oracle import ukf_oracle as orc
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(3, nobs=5, gap_h=1.0, seed0=91)
    tr = [types.SimpleNamespace(z=sb.z[i], dts=sb.dts[i], sog_rate=sb.sog_rate[i], cog_rate=sb.cog_rate[i]) for i in range(3)]
    dts = [np.repeat(sb.dts[0] / 2, 2), np.zeros(0), np.repeat(sb.dts[2] / 2, 2)[:3]]  # 8 steps, 0 steps, 3 steps
    hb = batch.pack_tracks(tr, dts, [sb.z[i][:, 0] for i in range(3)], H, Q, R, P0)
    out = batch.run_batch(hb)
    assert out["nsteps"].tolist() == [8, 0, 3] and not out["status"].any()
    # zero steps: history row 0 is the prior, and the smoother leaves it alone
    assert np.array_equal(out["means"][1, 0], sb.z[1][:, 0]) and np.array_equal(out["means_smoothed"][1, 0], sb.z[1][:, 0])
    assert np.array_equal(out["covs"][1, 0], P0)
    for b in (0, 2):
        m, P = orc.forward_track(sb.z[b][:, 0], P0, H, Q, R, dts[b], sb.dts[b], sb.z[b], sb.sog_rate[b], sb.cog_rate[b])
        n1 = len(dts[b]) + 1
        assert mean_err(out["means"][b, :n1], m) < MEAN_TOL and cov_err(out["covs"][b, :n1], P) < COV_TOL
    # a single observation: only the initial update can happen
    one = types.SimpleNamespace(z=sb.z[0][:, :1], dts=np.zeros(0), sog_rate=sb.sog_rate[0][:1], cog_rate=sb.cog_rate[0][:1])
    hb1 = batch.pack_tracks([one], [np.zeros(0)], [sb.z[0][:, 0]], H, Q, R, P0)
    o1 = batch.run_batch(hb1)
    assert o1["means"].shape == (1, 1, 4) and not o1["status"].any()
