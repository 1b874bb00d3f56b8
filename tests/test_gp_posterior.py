"""Posterior covariance on the device (ste_gp_predict_cov_f64), sample_y and normalize_y on the GP path, against
scikit-learn itself (the reference delegates every GP number to it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

gpu = pytest.mark.gpu

JITTER = 1e-10
KINDS = ["rbf", 0.5, 1.5, 2.5]  # RBF and the three Materns
# one short and one long length scale (hours), as in test_gp_matern.py
THETAS = {"short": np.log([1.5, 3.0, 0.02]), "long": np.log([2.0, 80.0, 0.05])}
SIZES = [2, 63, 64, 65, 129]  # n and m on both sides of the 64-tile boundaries


def _kind(k):
    from track_estimators._hip import binding

    return {"rbf": binding.STE_GP_KERNEL_RBF, 0.5: binding.STE_GP_KERNEL_MATERN12, 1.5: binding.STE_GP_KERNEL_MATERN32,
            2.5: binding.STE_GP_KERNEL_MATERN52}[k]


def _sk_kernel(k, theta=None):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel

    base = RBF(1.0) if k == "rbf" else Matern(length_scale=1.0, nu=k)
    kern = ConstantKernel(1.0) * base + WhiteKernel(0.5)
    return kern if theta is None else kern.clone_with_theta(np.asarray(theta, dtype=np.float64))


def _track(rng, n, nout=2):
    """x: cumulative sums of random gaps in hours; y: nout random-walk columns."""
    x = np.insert(np.cumsum(rng.choice([0.25, 0.5, 1.0, 2.0, 6.0], n - 1) * rng.uniform(0.5, 1.5, n - 1)), 0, 0.0)
    y = np.cumsum(rng.normal(0.0, 0.1, (n, nout)), axis=0)
    return x, y


def _queries(rng, x, m):
    return np.sort(rng.uniform(-5.0, x[-1] + 5.0, m))


def _ship_track(rng, n):
    """A track with lon / lat far from 0, where a zero-mean prior on the raw targets is a poor model."""
    from track_estimators.ship_track import ShipTrack

    x, y = _track(rng, n)
    st = ShipTrack()
    st.dts, st.lon, st.lat = np.diff(x), y[:, 0] - 30.0, y[:, 1] + 45.0
    return st


def _raw_predictions(batch, thetas, xq):
    """Both device predict calls on the same K^-1 and alpha, with the buffers as the library leaves them:
    (mean_cov [B][nout][mmax], cov [B][mmax][mmax], mean [B][nout][mmax], var [B][mmax], m)."""
    import torch
    from track_estimators._hip import binding

    batch.objective(thetas, eval_gradient=False, keep_kinv=True)
    m = np.array([len(q) for q in xq], dtype=np.int32)
    mmax = int(m.max())
    xs = np.zeros((batch.B, mmax))
    for b, q in enumerate(xq):
        xs[b, : len(q)] = q
    dev = dict(dtype=torch.float64, device=batch.device)
    t_m, t_xs = torch.from_numpy(m).to(batch.device), torch.from_numpy(xs).to(batch.device)
    ks = torch.empty((batch.B, 64 * ((mmax + 63) // 64), batch.ld), **dev)
    w = torch.empty_like(ks)
    mean_c = torch.zeros((batch.B, batch.nout, mmax), **dev)
    cov = torch.full((batch.B, mmax, mmax), float("nan"), **dev)  # every element must be written
    mean_p = torch.zeros((batch.B, batch.nout, mmax), **dev)
    var = torch.zeros((batch.B, mmax), **dev)
    s = batch._stream()
    binding.check(batch.lib.ste_gp_predict_cov_f64(C.byref(batch.struct), mmax, t_m.data_ptr(), t_xs.data_ptr(),
                                                   ks.data_ptr(), w.data_ptr(), mean_c.data_ptr(), cov.data_ptr(), s),
                  "ste_gp_predict_cov_f64")
    binding.check(batch.lib.ste_gp_predict_f64(C.byref(batch.struct), mmax, t_m.data_ptr(), t_xs.data_ptr(), ks.data_ptr(),
                                               mean_p.data_ptr(), var.data_ptr(), s), "ste_gp_predict_f64")
    return mean_c.cpu().numpy(), cov.cpu().numpy(), mean_p.cpu().numpy(), var.cpu().numpy(), m


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_predict_cov():
    from track_estimators._hip import binding

    with open(os.path.join(ROOT, "include", "ste.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert re.search(r"\bint ste_gp_predict_cov_f64\(", hdr)
    restype, argtypes = binding.SYMBOLS["ste_gp_predict_cov_f64"]
    assert restype is C.c_int and len(argtypes) == 9
    assert binding.load().ste_version() == 340


def _fake_batch(kernel=0):
    from track_estimators._hip import binding

    s = binding.SteGpBatchF64()
    s.B, s.nmax, s.nout, s.jitter = 1, 64, 2, JITTER
    for name in ("n", "x", "y", "theta", "K", "U", "Dinv", "Kinv", "alpha", "lml", "tr", "status"):
        setattr(s, name, 0x1000)  # never dereferenced: argument errors come first
    s.kernel = kernel
    return s


def test_predict_cov_refuses_bad_arguments_before_any_launch():
    from track_estimators._hip import binding

    lib = binding.load()
    p = 0x1000
    s = _fake_batch()
    for mmax in (0, -3):
        assert lib.ste_gp_predict_cov_f64(C.byref(s), mmax, p, p, p, p, p, p, None) == -1
        assert b"mmax" in lib.ste_gp_last_error()
    for i, what in enumerate([b"m", b"xs", b"Kstar", b"W", b"mean", b"cov"]):
        args = [p] * 6
        args[i] = None
        assert lib.ste_gp_predict_cov_f64(C.byref(s), 64, *args, None) == -1
        assert what in lib.ste_gp_last_error()
    s.Kinv = None
    assert lib.ste_gp_predict_cov_f64(C.byref(s), 64, p, p, p, p, p, p, None) == -1
    assert b"Kinv" in lib.ste_gp_last_error()
    for kind in (7, -1):
        s = _fake_batch(kind)
        assert lib.ste_gp_predict_cov_f64(C.byref(s), 64, p, p, p, p, p, p, None) == -1
        assert b"kernel" in lib.ste_gp_last_error()
    assert lib.ste_gp_predict_cov_f64(None, 64, p, p, p, p, p, p, None) == -1


def test_predict_refuses_std_and_cov_together():
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor

    gpr = DeviceGaussianProcessRegressor(_sk_kernel("rbf"))
    with pytest.raises(RuntimeError, match="At most one"):
        gpr.predict(np.zeros((3, 1)), return_std=True, return_cov=True)


def test_normalization_matches_sklearn_including_a_constant_column():
    from sklearn.gaussian_process import GaussianProcessRegressor
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor, _normalization

    rng = np.random.default_rng(3)
    x, y = _track(rng, 40, nout=3)
    y = y + np.array([-30.0, 45.0, 0.0])
    y[:, 2] = 7.25  # constant: scikit-learn's _handle_zeros_in_scale makes its std 1
    ref = GaussianProcessRegressor(_sk_kernel("rbf"), optimizer=None, normalize_y=True).fit(x[:, None], y)
    mean, std = _normalization(y)
    assert np.array_equal(mean, ref._y_train_mean) and np.array_equal(std, ref._y_train_std)
    assert std[2] == 1.0
    assert np.array_equal((y - mean) / std, ref.y_train_)
    # the constructor takes normalize_y now (it raised NotImplementedError)
    assert DeviceGaussianProcessRegressor(_sk_kernel("rbf"), normalize_y=True).normalize_y


# ---- GPU -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nout", [1, 2])
@pytest.mark.parametrize("kind", KINDS, ids=["rbf", "matern12", "matern32", "matern52"])
def test_cov_vs_sklearn_across_tile_boundaries(kind, nout):
    """Every (n, m) pair of SIZES in one batch.  cond(K) <= ~ n c / s ~ 1e4 here, so K^-1 carries ~1e-12 relative error
    and the covariance entries land far inside atol = 1e-7 (c + s), the tolerance the std tests imply (std atol 1e-6).
    Observed on the MI355X: at most 6.0e-13 (c + s) (Matern 3/2, long length scale), 1.6e-14 to 6.0e-13 over the cases."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(21)
    pairs = [(n, m) for n in SIZES for m in SIZES]
    data = [_track(rng, n, nout) for n, _ in pairs]
    xq = [_queries(rng, x, m) for (x, _), (_, m) in zip(data, pairs)]
    batch = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(kind))
    worst = {}
    for label, th in THETAS.items():
        out = batch.predict(np.tile(th, (len(data), 1)), xq, return_cov=True)
        c, s = np.exp(th[0]), np.exp(th[2])
        err = 0.0
        for (x, y), q, (mean, cov) in zip(data, xq, out):
            ref = GaussianProcessRegressor(_sk_kernel(kind, th), optimizer=None).fit(x[:, None], y)
            want_mean, want_cov = ref.predict(q[:, None], return_cov=True)
            want_mean = want_mean.reshape(len(q), nout)
            if want_cov.ndim == 3:
                want_cov = want_cov[..., 0]
            assert mean.shape == (len(q), nout) and cov.shape == (len(q), len(q))
            np.testing.assert_allclose(mean, want_mean, rtol=1e-8, atol=1e-7)
            np.testing.assert_allclose(cov, want_cov, rtol=0, atol=1e-7 * (c + s))
            err = max(err, float(np.abs(cov - want_cov).max()) / (c + s))
        worst[label] = err
    print(f"max |cov - sklearn| / (c + s), {kind}, nout {nout}: {worst}")


@gpu
@pytest.mark.parametrize("nout", [1, 2])
def test_regressor_predict_cov_shapes_and_values_vs_sklearn(nout):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor

    rng = np.random.default_rng(22)
    x, y = _track(rng, 90, nout)
    if nout == 1:
        y = y[:, 0]
    q = _queries(rng, x, 70)[:, None]
    kernel = _sk_kernel(1.5, THETAS["short"])
    dev = DeviceGaussianProcessRegressor(kernel, optimizer=None).fit(x[:, None], y)
    ref = GaussianProcessRegressor(kernel, optimizer=None).fit(x[:, None], y)
    mean, cov = dev.predict(q, return_cov=True)
    want_mean, want_cov = ref.predict(q, return_cov=True)
    assert mean.shape == want_mean.shape and cov.shape == want_cov.shape
    np.testing.assert_allclose(mean, want_mean, rtol=1e-8, atol=1e-7)
    np.testing.assert_allclose(cov, want_cov, rtol=0, atol=1e-7 * np.exp(THETAS["short"][[0, 2]]).sum())
    # return_std is unchanged by the new path
    assert np.array_equal(dev.predict(q, return_std=True)[0], mean)


@gpu
@pytest.mark.parametrize("kind", KINDS, ids=["rbf", "matern12", "matern32", "matern52"])
def test_cov_is_symmetric_zero_padded_and_agrees_with_predict(kind):
    """Mixed n and m in one batch: the cov call's mean is ste_gp_predict_f64's bit for bit, its diagonal is that call's
    variance to 1e-10 (c + s), both triangles are the same bits, and every element outside [0, m)^2 is 0."""
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(23)
    ns, ms = [129, 2, 65, 64, 200, 63], [65, 129, 2, 63, 64, 1]
    data = [_track(rng, n) for n in ns]
    xq = [_queries(rng, x, m) for (x, _), m in zip(data, ms)]
    batch = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(kind))
    thetas = np.stack([THETAS["short"], THETAS["long"]] * 3)
    mean_c, cov, mean_p, var, m = _raw_predictions(batch, thetas, xq)
    for b in range(batch.B):
        c, s = np.exp(thetas[b, 0]), np.exp(thetas[b, 2])
        mb = m[b]
        assert np.array_equal(cov[b], cov[b].T), b
        assert (cov[b, mb:, :] == 0).all() and (cov[b, :, mb:] == 0).all(), b
        assert np.array_equal(mean_c[b, :, :mb], mean_p[b, :, :mb]), b
        assert np.abs(np.diag(cov[b])[:mb] - var[b, :mb]).max() <= 1e-10 * (c + s), b


@gpu
@pytest.mark.parametrize("B, order", [(128, 2), (5, 1)], ids=["column-ordered-inverse", "row-ordered-inverse"])
def test_cov_does_not_depend_on_the_other_tracks(B, order):
    """One batch with mixed n and m gives the covariances of one-track batches with the same inverse_order, bit for bit."""
    from track_estimators._hip import binding
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(24)
    data = [_track(rng, int(rng.integers(2, 200))) for _ in range(B)]
    xq = [_queries(rng, x, int(rng.integers(1, 150))) for x, _ in data]
    thetas = np.tile(np.log([1.5, 10.0, 0.03]), (B, 1)) + rng.normal(0, 0.2, (B, 3))
    big = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=binding.STE_GP_KERNEL_MATERN52)
    assert big.inverse_order == order
    out = big.predict(thetas, xq, return_cov=True)
    for b in sorted({0, 1, B // 2, B - 1}):
        one = GpDeviceBatch([data[b][0]], [data[b][1]], inverse_order=order, kernel=binding.STE_GP_KERNEL_MATERN52)
        mean1, cov1 = one.predict(thetas[b:b + 1], [xq[b]], return_cov=True)[0]
        assert np.array_equal(out[b][1], cov1), b
        assert np.array_equal(out[b][0], mean1), b


@gpu
@pytest.mark.parametrize("nout", [1, 2])
def test_sample_y_is_multivariate_normal_on_the_device_posterior(nout):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor

    rng = np.random.default_rng(25)
    x, y = _track(rng, 60, nout)
    if nout == 1:
        y = y[:, 0]
    q = np.array([-2.0, 3.3, 10.1, x[-1] * 0.5, x[-1] + 1.0, x[-1] + 4.0])[:, None]
    kernel = _sk_kernel("rbf", THETAS["short"])
    dev = DeviceGaussianProcessRegressor(kernel, optimizer=None).fit(x[:, None], y)
    ref = GaussianProcessRegressor(kernel, optimizer=None).fit(x[:, None], y)
    for n_samples in (1, 3):
        assert dev.sample_y(q, n_samples).shape == ref.sample_y(q, n_samples).shape
    # scikit-learn's procedure on the device's mean and covariance, bit for bit
    got = dev.sample_y(q, 5, random_state=7)
    mean, cov = dev.predict(q, return_cov=True)
    r = np.random.RandomState(7)
    if nout == 1:
        want = r.multivariate_normal(mean, cov, 5).T
    else:
        want = np.hstack([r.multivariate_normal(mean[:, t], cov[..., t], 5).T[:, np.newaxis] for t in range(nout)])
    assert np.array_equal(got, want)
    # and statistically: the draws have the predicted mean and covariance
    N = 40000
    draws = dev.sample_y(q, N, random_state=np.random.RandomState(8))
    draws = draws.reshape(len(q), -1, N)
    mean, cov = mean.reshape(len(q), -1), cov.reshape(len(q), len(q), -1)
    for t in range(draws.shape[1]):
        d, C_ = draws[:, t, :], cov[..., t]
        sd = np.sqrt(np.diag(C_))
        assert (np.abs(d.mean(axis=1) - mean[:, t]) <= 5 * sd / np.sqrt(N) + 1e-12).all()
        emp = np.cov(d)
        bound = 6 * np.sqrt((np.outer(np.diag(C_), np.diag(C_)) + C_**2) / N)
        assert (np.abs(emp - C_) <= bound + 1e-12).all()


@gpu
@pytest.mark.timeout(600)
def test_normalize_y_fit_vs_sklearn_and_fit_batch_matches_single_fits():
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    from track_estimators.gaussian_processes.gaussian_process import GPRegression

    kernel = 1.0 * Matern(nu=1.5) + WhiteKernel(0.5)
    rng = np.random.default_rng(26)
    tracks = [_ship_track(rng, n) for n in (200, 170, 230)]
    kwargs = {"normalize_y": True, "n_restarts_optimizer": 2, "random_state": 0}
    gp = GPRegression(kernel=kernel)
    model = gp.fit(tracks[0], dict(kwargs))
    X, y = GPRegression._training_data(tracks[0])
    ref = GaussianProcessRegressor(kernel, **kwargs).fit(X, y)
    assert np.isclose(model.log_marginal_likelihood_value_, ref.log_marginal_likelihood_value_, rtol=1e-6)
    np.testing.assert_allclose(model.kernel_.theta, ref.kernel_.theta, rtol=1e-3, atol=1e-3)
    # predictions at the device's optimum, against scikit-learn's at the same theta
    at = GaussianProcessRegressor(model.kernel_, optimizer=None, normalize_y=True).fit(X, y)
    q = np.linspace(-3.0, X[-1, 0] + 3.0, 150)
    c_s = np.exp(model.kernel_.theta[[0, 2]]).sum() * at._y_train_std.max() ** 2
    pred, std = gp.predict(q)
    want_mean, want_std = at.predict(q[:, None], return_std=True)
    assert pred.shape == want_mean.shape == std.shape == want_std.shape == (150, 2)
    np.testing.assert_allclose(pred, want_mean, rtol=1e-8, atol=1e-7)
    np.testing.assert_allclose(std, want_std, rtol=1e-5, atol=1e-6)
    mean, cov = model.predict(q[:, None], return_cov=True)
    want_mean, want_cov = at.predict(q[:, None], return_cov=True)
    assert cov.shape == want_cov.shape == (150, 150, 2)
    np.testing.assert_allclose(mean, want_mean, rtol=1e-8, atol=1e-7)
    np.testing.assert_allclose(cov, want_cov, rtol=0, atol=1e-7 * c_s)
    # the lock-step batch fit sees each track's own normalisation: the same objective bits as the single fits
    batch = GPRegression(kernel=kernel)
    thetas, lml = batch.fit_batch(tracks, gpr_kwargs=dict(kwargs))
    q_b = [np.linspace(0.0, 50.0, 40 + 7 * b) for b in range(len(tracks))]
    for b, st in enumerate(tracks):
        one = GPRegression(kernel=kernel)
        m = one.fit(st, dict(kwargs))
        # (kernel_.theta is log(exp(theta)) through the kernel's parameters, which is not always theta's last bit: the
        #  raw optimum is compared through the same round trip)
        assert np.array_equal(kernel.clone_with_theta(thetas[b]).theta, m.kernel_.theta), b
        assert lml[b] == m.log_marginal_likelihood_value_, b
        (mb, sb), (mc, cb) = batch.predict_batch([q_b[b]] * 3)[b], batch.predict_batch(q_b, return_cov=True)[b]
        m1, s1 = one.predict(q_b[b])
        np.testing.assert_allclose(mb, m1, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(sb, s1, rtol=1e-12, atol=1e-14)
        mc1, cc1 = m.predict(q_b[b][:, None], return_cov=True)
        np.testing.assert_allclose(mc, mc1, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(cb, cc1, rtol=0, atol=1e-13 * max(1.0, np.abs(cc1).max()))
