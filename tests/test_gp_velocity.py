"""Posterior of the time derivative on the GP path (ste_gp_predict_deriv_f64, ste_gp_predict_deriv_cov_f64): the velocity of
a track, its SOG / COG, against a dense NumPy closed form and against central differences of scikit-learn's own predictions
(which know nothing of the derivative formulas)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

gpu = pytest.mark.gpu

JITTER = 1e-10
DKINDS = ["rbf", 1.5, 2.5]  # the kernels with a derivative (Matern 1/2 has none)
KIND_IDS = ["rbf", "matern32", "matern52"]
# the two THETAS of test_gp_posterior.py: one short and one long length scale (hours)
THETAS = {"short": np.log([1.5, 3.0, 0.02]), "long": np.log([2.0, 80.0, 0.05])}
SIZES = [2, 63, 64, 65, 129]  # n and m on both sides of the 64-tile boundaries
Q = {"rbf": 1.0, 1.5: 3.0, 2.5: 5.0 / 3.0}  # q = -kappa''(0)


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
    """x: cumulative sums of random gaps in hours; y: nout random-walk columns (as test_gp_posterior.py)."""
    x = np.insert(np.cumsum(rng.choice([0.25, 0.5, 1.0, 2.0, 6.0], n - 1) * rng.uniform(0.5, 1.5, n - 1)), 0, 0.0)
    y = np.cumsum(rng.normal(0.0, 0.1, (n, nout)), axis=0)
    return x, y


def _queries(rng, x, m):
    return np.sort(rng.uniform(-5.0, x[-1] + 5.0, m))


def _v0(theta, kind):
    """c q / l^2: the prior variance of the derivative, the scale of dvar and dcov."""
    c, l = np.exp(theta[0]), np.exp(theta[1])
    return c * Q[kind] / l**2


# ---- the closed form, written out densely -----------------------------------------------------------------------------
def _kappa(kind, d):
    """(kappa(d), kappa'(d), -kappa''(d)) of the unit-amplitude kernel function at d = (t - x) / l."""
    if kind == "rbf":
        e = np.exp(-0.5 * d * d)
        return e, -d * e, (1.0 - d * d) * e
    if kind == 1.5:
        a = np.sqrt(3.0) * np.abs(d)
        e = np.exp(-a)
        return (1.0 + a) * e, -3.0 * d * e, 3.0 * (1.0 - a) * e
    if kind == 2.5:
        a = np.sqrt(5.0) * np.abs(d)
        e = np.exp(-a)
        return (1.0 + a + a * a / 3.0) * e, -(5.0 / 3.0) * d * (1.0 + a) * e, (5.0 / 3.0) * (1.0 + a - 5.0 * d * d) * e
    raise ValueError(kind)


def _closed_form(kind, theta, x, y, t):
    """dmean (m, nout), dvar (m,), dcov (m, m) from include/ste.h's formulas with np.linalg.solve."""
    c, l, s = np.exp(theta)
    y = np.asarray(y, dtype=np.float64).reshape(len(x), -1)
    K = c * _kappa(kind, (x[:, None] - x[None, :]) / l)[0] + (s + JITTER) * np.eye(len(x))
    Kd = (c / l) * _kappa(kind, (t[:, None] - x[None, :]) / l)[1]  # K'*[j][i]
    dmean = Kd @ np.linalg.solve(K, y)
    red = Kd @ np.linalg.solve(K, Kd.T)
    dcov = (c / l**2) * _kappa(kind, (t[:, None] - t[None, :]) / l)[2] - red
    dvar = c * Q[kind] / l**2 - np.diag(red)
    return dmean, dvar, dcov


def _sklearn_differences(kind, theta, x, y, t):
    """dmean (m, nout) and dcov (m, m) from scikit-learn's GaussianProcessRegressor.predict alone: central differences of
    the mean at h = 1e-4 l, and the 4-point stencil of the latent covariance (the WhiteKernel's s removed where two
    shifted query points coincide)."""
    from sklearn.gaussian_process import GaussianProcessRegressor

    h = 1e-4 * np.exp(theta[1])
    s = np.exp(theta[2])
    ref = GaussianProcessRegressor(_sk_kernel(kind, theta), optimizer=None).fit(x[:, None], y)
    m = len(t)
    z = np.concatenate([t + h, t - h])
    mean, cov = ref.predict(z[:, None], return_cov=True)
    mean = np.asarray(mean).reshape(2 * m, -1)
    if cov.ndim == 3:
        cov = cov[..., 0]
    cov = cov - s * (z[:, None] == z[None, :])
    dmean = (mean[:m] - mean[m:]) / (2 * h)
    pp, pm, mp, mm = cov[:m, :m], cov[:m, m:], cov[m:, :m], cov[m:, m:]
    dcov = (pp - pm - mp + mm) / (4 * h * h)
    return dmean, dcov


# ---- raw device calls -------------------------------------------------------------------------------------------------
def _raw(batch, thetas, xq):
    """Both derivative calls and ste_gp_predict_f64 before and after them, on the same K^-1, alpha and workspaces:
    dict of NumPy arrays with the buffers as the library leaves them (dmean / dvar / dcov prefilled with NaN)."""
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
    nan = float("nan")
    dmean_p = torch.full((batch.B, batch.nout, mmax), nan, **dev)
    dvar = torch.full((batch.B, mmax), nan, **dev)
    dmean_c = torch.full((batch.B, batch.nout, mmax), nan, **dev)
    dcov = torch.full((batch.B, mmax, mmax), nan, **dev)  # every element must be written
    mean0, var0 = torch.zeros((batch.B, batch.nout, mmax), **dev), torch.zeros((batch.B, mmax), **dev)
    mean1, var1 = torch.zeros_like(mean0), torch.zeros_like(var0)
    lib, s, struct = batch.lib, batch._stream(), C.byref(batch.struct)
    binding.check(lib.ste_gp_predict_f64(struct, mmax, t_m.data_ptr(), t_xs.data_ptr(), ks.data_ptr(), mean0.data_ptr(),
                                         var0.data_ptr(), s), "ste_gp_predict_f64")
    binding.check(lib.ste_gp_predict_deriv_f64(struct, mmax, t_m.data_ptr(), t_xs.data_ptr(), ks.data_ptr(),
                                               dmean_p.data_ptr(), dvar.data_ptr(), s), "ste_gp_predict_deriv_f64")
    binding.check(lib.ste_gp_predict_deriv_cov_f64(struct, mmax, t_m.data_ptr(), t_xs.data_ptr(), ks.data_ptr(),
                                                   w.data_ptr(), dmean_c.data_ptr(), dcov.data_ptr(), s),
                  "ste_gp_predict_deriv_cov_f64")
    binding.check(lib.ste_gp_predict_f64(struct, mmax, t_m.data_ptr(), t_xs.data_ptr(), ks.data_ptr(), mean1.data_ptr(),
                                         var1.data_ptr(), s), "ste_gp_predict_f64")
    out = dict(dmean_p=dmean_p, dvar=dvar, dmean_c=dmean_c, dcov=dcov, mean0=mean0, var0=var0, mean1=mean1, var1=var1)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["m"] = m
    return out


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_derivative_calls():
    from track_estimators._hip import binding

    with open(os.path.join(ROOT, "include", "ste.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    # the signatures mirror the position calls': 8 and 9 arguments
    for name, position in (("ste_gp_predict_deriv_f64", "ste_gp_predict_f64"),
                           ("ste_gp_predict_deriv_cov_f64", "ste_gp_predict_cov_f64")):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        restype, argtypes = binding.SYMBOLS[name]
        assert restype is C.c_int and argtypes == binding.SYMBOLS[position][1], name
        assert len(argtypes) == (8 if position == "ste_gp_predict_f64" else 9), name
        assert hasattr(binding.load(), name), name
    assert binding.load().ste_version() == 340


def _fake_batch(kernel=None):
    from track_estimators._hip import binding

    s = binding.SteGpBatchF64()
    s.B, s.nmax, s.nout, s.jitter = 1, 64, 2, JITTER
    for name in ("n", "x", "y", "theta", "K", "U", "Dinv", "Kinv", "alpha", "lml", "tr", "status"):
        setattr(s, name, 0x1000)  # never dereferenced: argument errors come first
    s.kernel = binding.STE_GP_KERNEL_RBF if kernel is None else kernel
    return s


def _call(lib, which, s, mmax, ptrs):
    """ptrs: m, xs, Kstar, [W,] dmean, dvar|dcov"""
    if which == "deriv":
        return lib.ste_gp_predict_deriv_f64(s, mmax, *ptrs, None)
    return lib.ste_gp_predict_deriv_cov_f64(s, mmax, *ptrs, None)


@pytest.mark.parametrize("which", ["deriv", "deriv_cov"])
def test_derivative_calls_refuse_bad_arguments_before_any_launch(which):
    from track_estimators._hip import binding

    lib = binding.load()
    p = 0x1000
    names = [b"m", b"xs", b"Kstar", b"dmean", b"dvar"] if which == "deriv" else [b"m", b"xs", b"Kstar", b"W", b"dmean", b"dcov"]
    s = _fake_batch()
    for mmax in (0, -3):
        assert _call(lib, which, C.byref(s), mmax, [p] * len(names)) == -1
        assert b"mmax" in lib.ste_gp_last_error()
    for i, what in enumerate(names):
        args = [p] * len(names)
        args[i] = None
        assert _call(lib, which, C.byref(s), 64, args) == -1, what
        assert what in lib.ste_gp_last_error(), what
    s.Kinv = None
    assert _call(lib, which, C.byref(s), 64, [p] * len(names)) == -1
    assert b"Kinv" in lib.ste_gp_last_error()
    s = _fake_batch(binding.STE_GP_KERNEL_MATERN12)
    assert _call(lib, which, C.byref(s), 64, [p] * len(names)) == -1
    assert b"differentiable" in lib.ste_gp_last_error()
    for kind in (7, -1):
        s = _fake_batch(kind)
        assert _call(lib, which, C.byref(s), 64, [p] * len(names)) == -1
        assert b"kernel" in lib.ste_gp_last_error()
    assert _call(lib, which, None, 64, [p] * len(names)) == -1


def test_velocity_to_sog_cog_hand_computed():
    from track_estimators.constants import EARTH_RADIUS
    from track_estimators.gaussian_processes.gaussian_process import velocity_to_sog_cog

    deg = EARTH_RADIUS * np.pi / 180.0  # km per degree of latitude: 111.32
    sog, cog = velocity_to_sog_cog(10.0, 0.0, 1.0)  # 1 deg/h due north
    assert np.isclose(sog, 111.32, atol=5e-3) and np.isclose(sog, deg, rtol=1e-15) and cog == 0.0
    sog, cog = velocity_to_sog_cog(0.0, 0.5, 0.0)  # due east at the equator
    assert np.isclose(sog, 0.5 * deg, rtol=1e-15) and np.isclose(cog, 90.0, rtol=0, atol=1e-12)
    sog, cog = velocity_to_sog_cog(0.0, -0.5, 0.0)  # due west
    assert np.isclose(sog, 0.5 * deg, rtol=1e-15) and np.isclose(cog, 270.0, rtol=0, atol=1e-12)
    sog, _ = velocity_to_sog_cog(60.0, 1.0, 0.0)  # dlon counts cos(60) = 1/2 at latitude 60
    assert np.isclose(sog, 0.5 * deg, rtol=1e-14)
    sog, cog = velocity_to_sog_cog(60.0, 2.0, -1.0)  # (v_e, v_n) = deg * (1, -1): south-east
    assert np.isclose(sog, np.sqrt(2.0) * deg, rtol=1e-14) and np.isclose(cog, 135.0, rtol=0, atol=1e-9)
    # vectorised, every course in [0, 360), the convention of utils.heading
    rng = np.random.default_rng(1)
    lat, dlon, dlat = rng.uniform(-80, 80, 1000), rng.normal(0, 0.3, 1000), rng.normal(0, 0.3, 1000)
    dlat[:3], dlon[:3] = -1e-300, [-0.0, 0.0, -1e-300]
    sog, cog = velocity_to_sog_cog(lat, dlon, dlat)
    assert sog.shape == cog.shape == (1000,)
    assert ((cog >= 0.0) & (cog < 360.0)).all()
    from track_estimators.utils import heading

    lon2, lat2 = dlon * 1e-6, lat + dlat * 1e-6  # a tiny step along the velocity
    np.testing.assert_allclose(np.cos(np.radians(cog[3:] - heading(0.0, lat, lon2, lat2)[3:])), 1.0, atol=1e-8)


def test_closed_form_agrees_with_sklearn_central_differences():
    """The NumPy restatement the GPU tests compare against, checked against scikit-learn's predictions alone."""
    rng = np.random.default_rng(30)
    for kind in DKINDS:
        for label, th in THETAS.items():
            x, y = _track(rng, 40)
            t = _queries(rng, x, 30)
            dmean, dvar, dcov = _closed_form(kind, th, x, y, t)
            fd_mean, fd_cov = _sklearn_differences(kind, th, x, y, t)
            v0 = _v0(th, kind)
            np.testing.assert_allclose(dmean, fd_mean, rtol=1e-5, atol=1e-6 * np.abs(dmean).max())
            np.testing.assert_allclose(dcov, fd_cov, rtol=0, atol=1e-3 * v0)
            np.testing.assert_allclose(dvar, np.diag(fd_cov), rtol=0, atol=1e-3 * v0)


def test_regressor_refuses_matern12_before_any_device_work():
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor

    gpr = DeviceGaussianProcessRegressor(ConstantKernel(1.0) * Matern(nu=0.5) + WhiteKernel(0.1))
    with pytest.raises(ValueError, match="differentiable"):
        gpr.predict_derivative(np.zeros((3, 1)))
    gpr = DeviceGaussianProcessRegressor(ConstantKernel(1.0) * RBF(1.0) + WhiteKernel(0.1))
    with pytest.raises(RuntimeError, match="At most one"):
        gpr.predict_derivative(np.zeros((3, 1)), return_std=True, return_cov=True)


# ---- GPU --------------------------------------------------------------------------------------------------------------
def _pairs_batch(rng, kind, nout=2):
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    pairs = [(n, m) for n in SIZES for m in SIZES]
    data = [_track(rng, n, nout) for n, _ in pairs]
    xq = [_queries(rng, x, m) for (x, _), (_, m) in zip(data, pairs)]
    return data, xq, GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(kind))


@gpu
@pytest.mark.parametrize("kind", DKINDS, ids=KIND_IDS)
def test_derivative_vs_closed_form_across_tile_boundaries(kind):
    """Every (n, m) pair of SIZES in one batch, both THETAS, both calls."""
    rng = np.random.default_rng(31)
    data, xq, batch = _pairs_batch(rng, kind)
    worst = {}
    for label, th in THETAS.items():
        v0, l = _v0(th, kind), np.exp(th[1])
        std_out = batch.predict_derivative(np.tile(th, (batch.B, 1)), xq)
        cov_out = batch.predict_derivative(np.tile(th, (batch.B, 1)), xq, return_cov=True)
        err = 0.0
        for (x, y), q, (dm, dstd), (dm_c, dcov) in zip(data, xq, std_out, cov_out):
            want_mean, want_var, want_cov = _closed_form(kind, th, x, y, q)
            assert dm.shape == dstd.shape == (len(q), 2) and dcov.shape == (len(q), len(q))
            np.testing.assert_allclose(dm, want_mean, rtol=1e-8, atol=1e-7 * np.abs(y).max() / l)
            assert np.array_equal(dm, dm_c)
            np.testing.assert_allclose(dstd[:, 0] ** 2, np.maximum(want_var, 0.0), rtol=0, atol=1e-7 * v0)
            np.testing.assert_allclose(dcov, want_cov, rtol=0, atol=1e-7 * v0)
            err = max(err, float(np.abs(dcov - want_cov).max()) / v0)
        worst[label] = err
    print(f"max |dcov - closed form| / (c q / l^2), {kind}: {worst}")


@gpu
@pytest.mark.parametrize("kind", DKINDS, ids=KIND_IDS)
def test_derivative_vs_sklearn_central_differences(kind):
    """No formula of the derivative on this side: scikit-learn's predict, differenced."""
    rng = np.random.default_rng(32)
    data, xq, batch = _pairs_batch(rng, kind)
    for label, th in THETAS.items():
        v0 = _v0(th, kind)
        std_out = batch.predict_derivative(np.tile(th, (batch.B, 1)), xq)
        cov_out = batch.predict_derivative(np.tile(th, (batch.B, 1)), xq, return_cov=True)
        for (x, y), q, (dm, dstd), (_, dcov) in zip(data, xq, std_out, cov_out):
            fd_mean, fd_cov = _sklearn_differences(kind, th, x, y, q)
            np.testing.assert_allclose(dm, fd_mean, rtol=1e-5, atol=1e-6 * max(np.abs(fd_mean).max(), 1e-300))
            np.testing.assert_allclose(dcov, fd_cov, rtol=0, atol=1e-3 * v0)
            np.testing.assert_allclose(dstd[:, 0] ** 2, np.maximum(np.diag(fd_cov), 0.0), rtol=0, atol=1e-3 * v0)


@gpu
@pytest.mark.parametrize("kind", DKINDS, ids=KIND_IDS)
def test_derivative_contracts(kind):
    """Mixed n and m in one batch: dcov symmetric bit for bit and 0 outside [0, m)^2; rows >= m of dmean and dvar not
    written; both calls' dmean the same bits; ste_gp_predict_f64 the same bits before and after the derivative calls."""
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(33)
    ns, ms = [129, 2, 65, 64, 200, 63], [65, 129, 2, 63, 64, 1]
    data = [_track(rng, n) for n in ns]
    xq = [_queries(rng, x, m) for (x, _), m in zip(data, ms)]
    batch = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(kind))
    thetas = np.stack([THETAS["short"], THETAS["long"]] * 3)
    r = _raw(batch, thetas, xq)
    m = r["m"]
    for b in range(batch.B):
        mb = m[b]
        v0 = _v0(thetas[b], kind)
        assert np.array_equal(r["dcov"][b], r["dcov"][b].T), b
        assert (r["dcov"][b, mb:, :] == 0).all() and (r["dcov"][b, :, mb:] == 0).all(), b
        assert np.isfinite(r["dcov"][b, :mb, :mb]).all(), b
        assert np.isnan(r["dmean_p"][b, :, mb:]).all() and np.isnan(r["dvar"][b, mb:]).all(), b
        assert np.isnan(r["dmean_c"][b, :, mb:]).all(), b
        assert np.isfinite(r["dmean_p"][b, :, :mb]).all() and np.isfinite(r["dvar"][b, :mb]).all(), b
        assert np.array_equal(r["dmean_p"][b, :, :mb], r["dmean_c"][b, :, :mb]), b
        assert np.abs(np.diag(r["dcov"][b])[:mb] - r["dvar"][b, :mb]).max() <= 1e-10 * v0, b
    assert np.array_equal(r["mean0"], r["mean1"]) and np.array_equal(r["var0"], r["var1"])


@gpu
@pytest.mark.parametrize("kind", DKINDS, ids=KIND_IDS)
def test_derivative_does_not_depend_on_the_other_tracks(kind):
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(34)
    data = [_track(rng, n) for n in (150, 7, 90)]
    xq = [_queries(rng, x, m) for (x, _), m in zip(data, (70, 130, 3))]
    thetas = np.stack([THETAS["short"], THETAS["long"], np.log([1.2, 9.0, 0.03])])
    big = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(kind))
    std3 = big.predict_derivative(thetas, xq)
    cov3 = big.predict_derivative(thetas, xq, return_cov=True)
    for b in range(3):
        one = GpDeviceBatch([data[b][0]], [data[b][1]], inverse_order=big.inverse_order, kernel=_kind(kind))
        (dm1, ds1), (dmc1, dc1) = one.predict_derivative(thetas[b:b + 1], [xq[b]])[0], \
            one.predict_derivative(thetas[b:b + 1], [xq[b]], return_cov=True)[0]
        assert np.array_equal(std3[b][0], dm1) and np.array_equal(std3[b][1], ds1), b
        assert np.array_equal(cov3[b][0], dmc1) and np.array_equal(cov3[b][1], dc1), b


def _ship_track(rng, n):
    from track_estimators.ship_track import ShipTrack

    x, y = _track(rng, n)
    st = ShipTrack()
    st.dts, st.lon, st.lat = np.diff(x), y[:, 0] - 30.0, y[:, 1] + 45.0
    return st


@gpu
@pytest.mark.parametrize("nout", [1, 2])
def test_regressor_normalize_y_scales_the_normalised_derivative(nout):
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor, _normalization

    rng = np.random.default_rng(35)
    x, y = _track(rng, 90, nout)
    y = y * 3.0 + np.array([-30.0, 45.0])[:nout]
    if nout == 1:
        y = y[:, 0]
    kernel = 1.0 * Matern(length_scale=4.0, nu=2.5) + WhiteKernel(0.01)
    q = _queries(rng, x, 70)
    dev = DeviceGaussianProcessRegressor(kernel, optimizer=None, normalize_y=True).fit(x[:, None], y)
    _, sd = _normalization(np.asarray(y).reshape(len(x), -1))
    th = dev.kernel_.theta
    yn = (np.asarray(y).reshape(len(x), -1) - np.mean(np.asarray(y).reshape(len(x), -1), axis=0)) / sd
    want_mean, want_var, want_cov = _closed_form(2.5, th, x, yn, q)
    dm, dstd = dev.predict_derivative(q[:, None], return_std=True)
    dm_c, dcov = dev.predict_derivative(q[:, None], return_cov=True)
    shape = (len(q),) if nout == 1 else (len(q), nout)
    assert dm.shape == dstd.shape == shape and dcov.shape == (len(q), len(q)) + shape[1:]
    assert np.array_equal(dev.predict_derivative(q[:, None]), dm) and np.array_equal(dm, dm_c)
    v0 = _v0(th, 2.5)
    np.testing.assert_allclose(dm.reshape(len(q), -1), want_mean * sd, rtol=1e-8, atol=1e-7 * np.abs(yn).max() * sd.max())
    np.testing.assert_allclose(dstd.reshape(len(q), -1), np.sqrt(np.maximum(want_var, 0))[:, None] * sd, rtol=1e-6,
                               atol=1e-6 * np.sqrt(v0) * sd.max())
    np.testing.assert_allclose(dcov.reshape(len(q), len(q), -1), want_cov[:, :, None] * sd**2, rtol=0,
                               atol=1e-7 * v0 * sd.max() ** 2)
    # the regressor's own predict, differenced: no mean offset in the derivative
    h = 1e-4 * np.exp(th[1])
    fd = (dev.predict((q + h)[:, None]) - dev.predict((q - h)[:, None])) / (2 * h)
    np.testing.assert_allclose(dm, fd, rtol=1e-5, atol=1e-6 * np.abs(fd).max())


@gpu
def test_regressor_refuses_matern12_after_a_fit():
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    from track_estimators.gaussian_processes.device import GpDeviceBatch
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor

    rng = np.random.default_rng(36)
    x, y = _track(rng, 30)
    dev = DeviceGaussianProcessRegressor(1.0 * Matern(nu=0.5) + WhiteKernel(0.1), optimizer=None).fit(x[:, None], y)
    with pytest.raises(ValueError, match="differentiable"):
        dev.predict_derivative(x[:, None], return_std=True)
    batch = GpDeviceBatch([x], [y], kernel=_kind(0.5))
    with pytest.raises(ValueError, match="differentiable"):
        batch.predict_derivative(np.log([[1.0, 3.0, 0.1]]), [x])


@gpu
@pytest.mark.timeout(600)
def test_predict_velocity_batch_matches_single_fits():
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    from track_estimators.gaussian_processes.gaussian_process import GPRegression

    kernel = 1.0 * Matern(nu=1.5) + WhiteKernel(0.5)
    rng = np.random.default_rng(37)
    tracks = [_ship_track(rng, n) for n in (120, 90, 150)]
    kwargs = {"normalize_y": True, "n_restarts_optimizer": 1, "random_state": 0}
    batch = GPRegression(kernel=kernel)
    batch.fit_batch(tracks, gpr_kwargs=dict(kwargs))
    q_b = [np.linspace(0.0, 50.0, 40 + 7 * b) for b in range(len(tracks))]
    vel = batch.predict_velocity_batch(q_b)
    vel_c = batch.predict_velocity_batch(q_b, return_cov=True)
    for b, st in enumerate(tracks):
        one = GPRegression(kernel=kernel)
        model = one.fit(st, dict(kwargs))
        dm1, ds1 = one.predict_velocity(q_b[b])
        assert vel[b][0].shape == vel[b][1].shape == (len(q_b[b]), 2) and vel_c[b][1].shape == (len(q_b[b]),) * 2 + (2,)
        np.testing.assert_allclose(vel[b][0], dm1, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(vel[b][1], ds1, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(vel_c[b][0], dm1, rtol=1e-12, atol=1e-12)
        _, dc1 = model.predict_derivative(q_b[b][:, None], return_cov=True)
        np.testing.assert_allclose(vel_c[b][1], dc1, rtol=0, atol=1e-12 * max(1.0, np.abs(dc1).max()))


def _great_circle_track(u=20.0, course=60.0, hours=48.0, gap=0.5, sub=20, noise_deg=1e-4, seed=38):
    """Constant speed u (km/h) and course (deg) from (-30, 45), dead-reckoned by synthetic._advance in `sub` steps per gap;
    returns (ShipTrack with noisy observations, fine times, fine lon, fine lat)."""
    from track_estimators import synthetic
    from track_estimators.ship_track import ShipTrack

    nfine = int(round(hours / gap)) * sub
    dt = gap / sub
    lon, lat = np.empty(nfine + 1), np.empty(nfine + 1)
    lon[0], lat[0] = -30.0, 45.0
    for k in range(nfine):
        lon[k + 1], lat[k + 1] = synthetic._advance(lon[k], lat[k], u, course, dt)
    t = np.arange(nfine + 1) * dt
    rng = np.random.default_rng(seed)
    st = ShipTrack()
    st.dts = np.full(nfine // sub, gap)
    st.lon = lon[::sub] + rng.normal(0.0, noise_deg, nfine // sub + 1)
    st.lat = lat[::sub] + rng.normal(0.0, noise_deg, nfine // sub + 1)
    return st, t, lon, lat


@gpu
def test_end_to_end_velocity_and_sog_cog_of_a_great_circle_track():
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    from track_estimators.gaussian_processes.gaussian_process import GPRegression

    u, course = 20.0, 60.0
    st, t, lon, lat = _great_circle_track(u, course)
    gp = GPRegression(kernel=ConstantKernel(1.0) * RBF(20.0) + WhiteKernel(1e-6))
    gp.fit(st, {"optimizer": None, "normalize_y": True})
    dt = t[1] - t[0]
    k = np.arange(len(t))[(t >= 6.0) & (t <= t[-1] - 6.0)][::7]  # the interior
    true_v = np.column_stack([(lon[k + 1] - lon[k - 1]) / (2 * dt), (lat[k + 1] - lat[k - 1]) / (2 * dt)])
    dm, dstd = gp.predict_velocity(t[k])
    assert dm.shape == dstd.shape == (len(k), 2) and (dstd > 0).all()
    np.testing.assert_allclose(dm, true_v, rtol=0.01, atol=0)
    sog, cog = gp.predict_sog_cog(t[k])
    assert sog.shape == cog.shape == (len(k),)
    np.testing.assert_allclose(sog, u, rtol=0.01)
    assert np.abs(cog - course).max() <= 0.5
