"""Matern kernels (nu = 1/2, 3/2, 5/2) on the GP path: kernel description, C ABI, and the device kernels against
scikit-learn itself (the reference delegates every GP number to it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

gpu = pytest.mark.gpu

NUS = [0.5, 1.5, 2.5]
JITTER = 1e-10
# one short and one long length scale (hours), so that both ends of the kernel are exercised
THETAS = {"short": np.log([1.5, 3.0, 0.02]), "long": np.log([2.0, 80.0, 0.05])}
TILE_SIZES = [2, 16, 63, 64, 65, 128, 129, 192]


def _kind(nu):
    from track_estimators._hip import binding

    return {0.5: binding.STE_GP_KERNEL_MATERN12, 1.5: binding.STE_GP_KERNEL_MATERN32,
            2.5: binding.STE_GP_KERNEL_MATERN52}[nu]


def _sk_kernel(nu, theta=None):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    k = ConstantKernel(1.0) * Matern(length_scale=1.0, nu=nu) + WhiteKernel(0.5)
    return k if theta is None else k.clone_with_theta(np.asarray(theta, dtype=np.float64))


def _track(rng, n, nout=2):
    """x: cumulative sums of random gaps in hours; y: nout random-walk columns."""
    x = np.insert(np.cumsum(rng.choice([0.25, 0.5, 1.0, 2.0, 6.0], n - 1) * rng.uniform(0.5, 1.5, n - 1)), 0, 0.0)
    y = np.cumsum(rng.normal(0.0, 0.1, (n, nout)), axis=0)
    return x, y


def _sk_lml_grad(nu, theta, x, y):
    from sklearn.gaussian_process import GaussianProcessRegressor

    gpr = GaussianProcessRegressor(_sk_kernel(nu, theta), alpha=JITTER, optimizer=None).fit(x[:, None], y)
    return gpr.log_marginal_likelihood(theta, eval_gradient=True)


# ---- CPU: the kernel description -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", NUS)
def test_kernel_kind_and_spec_of_matern(nu):
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    from track_estimators.gaussian_processes import gaussian_process as gpm

    kernel = 2.0 * Matern(length_scale=7.0, nu=nu, length_scale_bounds=(1e-2, 1e4)) + WhiteKernel(0.3)
    assert gpm._kernel_kind(kernel) == _kind(nu)
    theta0, bounds = gpm._kernel_spec(kernel)
    np.testing.assert_array_equal(theta0, kernel.theta)
    np.testing.assert_array_equal(bounds, kernel.bounds)


def test_matern_nu_inf_is_rbf():
    from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel
    from track_estimators._hip import binding
    from track_estimators.gaussian_processes import gaussian_process as gpm

    assert gpm._kernel_kind(1.0 * Matern(nu=np.inf) + WhiteKernel()) == binding.STE_GP_KERNEL_RBF
    assert gpm._kernel_kind(1.0 * RBF() + WhiteKernel()) == binding.STE_GP_KERNEL_RBF


def _refused_kernels():
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, RationalQuadratic, WhiteKernel

    return {
        "nu=2.0": 1.0 * Matern(nu=2.0) + WhiteKernel(),
        "anisotropic": 1.0 * Matern(length_scale=[1.0, 2.0], nu=1.5) + WhiteKernel(),
        "fixed-constant": ConstantKernel(1.0, constant_value_bounds="fixed") * Matern(nu=1.5) + WhiteKernel(),
        "fixed-length-scale": 1.0 * Matern(nu=2.5, length_scale_bounds="fixed") + WhiteKernel(),
        "bare-matern": Matern(nu=1.5),
        "no-white-kernel": 1.0 * Matern(nu=1.5),
        "bare-rbf": RBF(),
        "rational-quadratic": 1.0 * RationalQuadratic() + WhiteKernel(),
    }


@pytest.mark.parametrize("name", list(_refused_kernels()))
def test_unsupported_kernels_are_refused(name):
    from track_estimators.gaussian_processes import gaussian_process as gpm

    kernel = _refused_kernels()[name]
    with pytest.raises(NotImplementedError, match="Matern"):
        gpm._kernel_kind(kernel)
    with pytest.raises(NotImplementedError):
        gpm._kernel_spec(kernel)


# ---- CPU: the C ABI ------------------------------------------------------------------------------------------------
def test_header_defines_the_kernel_kinds_of_the_binding():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for name in ("RBF", "MATERN12", "MATERN32", "MATERN52"):
        m = re.search(r"#define STE_GP_KERNEL_%s (\d+)" % name, hdr)
        assert m, name
        assert int(m.group(1)) == getattr(binding, "STE_GP_KERNEL_" + name)
    assert [f[0] for f in binding.SteGpBatchF64._fields_][-1] == "kernel"
    # appended: every earlier field keeps its offset
    assert binding.SteGpBatchF64.kernel.offset == binding.SteGpBatchF64.status.offset + 8


def test_unknown_kernel_kind_is_refused_before_any_launch():
    from track_estimators._hip import binding

    lib = binding.load()
    s = binding.SteGpBatchF64()
    s.B, s.nmax, s.nout, s.jitter = 1, 64, 2, JITTER
    for name in ("n", "x", "y", "theta", "K", "U", "Dinv", "alpha", "lml", "tr", "status"):
        setattr(s, name, 0x1000)  # never dereferenced: argument errors come first
    s.kernel = 7
    assert lib.ste_gp_lml_f64(C.byref(s), None) == -1
    assert b"kernel" in lib.ste_gp_last_error()
    assert lib.ste_gp_rbf_kmatrix_f64(C.byref(s), None) == -1 and b"kernel" in lib.ste_gp_last_error()
    s.kernel = -1
    assert lib.ste_gp_lml_f64(C.byref(s), None) == -1 and b"kernel" in lib.ste_gp_last_error()


# ---- GPU -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nu", NUS)
def test_kmatrix_vs_sklearn(nu):
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(11)
    data = [_track(rng, n) for n in (70, 200, 311)]
    batch = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(nu))
    for th in THETAS.values():
        K = batch.kmatrix(np.tile(th, (len(data), 1)))
        for b, (x, _) in enumerate(data):
            n = len(x)
            Kref = _sk_kernel(nu, th)(x[:, None])
            Kref[np.diag_indices(n)] += JITTER
            np.testing.assert_allclose(np.tril(K[b, :n, :n]), np.tril(Kref), rtol=1e-13, atol=1e-13)


@gpu
@pytest.mark.parametrize("order", [1, 2], ids=["row-ordered-inverse", "column-ordered-inverse"])
@pytest.mark.parametrize("nu", NUS)
def test_objective_builds_k_in_place_with_the_stand_alone_bits(nu, order):
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(12)
    data = [_track(rng, n) for n in (65, 129, 300)]
    batch = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], inverse_order=order, kernel=_kind(nu))
    for th in THETAS.values():
        thetas = np.tile(th, (len(data), 1))
        batch.kmatrix(thetas)
        L_alone, status = batch.cholesky()
        assert not status.any()
        _, _, status = batch.objective(thetas)
        assert not status.any()
        L_fused = np.tril(batch.t_K.cpu().numpy())
        for b, (x, _) in enumerate(data):
            n = len(x)
            assert np.array_equal(L_fused[b, :n, :n], L_alone[b, :n, :n])


@gpu
@pytest.mark.parametrize("nout", [1, 2])
@pytest.mark.parametrize("order", [1, 2], ids=["row-ordered-inverse", "column-ordered-inverse"])
@pytest.mark.parametrize("nu", NUS)
def test_lml_and_gradient_at_tile_boundaries_vs_sklearn(nu, order, nout):
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(13 + nout)
    data = [_track(rng, n, nout) for n in TILE_SIZES]
    batch = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], inverse_order=order, kernel=_kind(nu))
    for label, th in THETAS.items():
        lml, grad, status = batch.objective(np.tile(th, (len(data), 1)))
        assert not status.any()
        for b, (x, y) in enumerate(data):
            want_lml, want_grad = _sk_lml_grad(nu, th, x, y)
            msg = f"{label} n={len(x)}"
            assert np.isclose(lml[b], want_lml, rtol=1e-9, atol=1e-7), (msg, lml[b], want_lml)
            np.testing.assert_allclose(grad[b], want_grad, rtol=1e-6, atol=1e-5, err_msg=msg)


@gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("nu", NUS)
def test_lml_and_gradient_at_n2000_vs_sklearn(nu):
    """BASELINE configs[4]'s matrix size (32 tile columns), both inverse orders."""
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(2000)
    x, y = _track(rng, 2000)
    th = np.log([2.0, 20.0, 0.05])
    want_lml, want_grad = _sk_lml_grad(nu, th, x, y)
    for order in (1, 2):
        batch = GpDeviceBatch([x], [y], inverse_order=order, kernel=_kind(nu))
        lml, grad, status = batch.objective(th[None])
        assert not status.any()
        assert np.isclose(lml[0], want_lml, rtol=1e-9, atol=1e-7), (order, lml[0], want_lml)
        np.testing.assert_allclose(grad[0], want_grad, rtol=1e-6, atol=1e-5, err_msg=str(order))
        del batch


@gpu
@pytest.mark.parametrize("nu", NUS)
def test_large_batch_matches_per_track_row_order_and_subset_launch(nu):
    """>= 128 matrices take the column-ordered kernels; each track agrees with its own row-ordered evaluation, and a
    subset launch reproduces the full launch bit for bit and leaves the other matrices' outputs alone."""
    from track_estimators._hip import binding
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(14)
    B = 128
    data = [_track(rng, int(rng.integers(40, 200))) for _ in range(B)]
    xs, ys = [d[0] for d in data], [d[1] for d in data]
    theta = np.tile(np.log([1.5, 10.0, 0.03]), (B, 1)) + rng.normal(0, 0.2, (B, 3))
    big = GpDeviceBatch(xs, ys, kernel=_kind(nu))
    assert big.inverse_order == binding.STE_GP_INVERSE_COLS
    lml, grad, status = big.objective(theta)
    assert not status.any()
    for b in (0, 37, 127):
        one = GpDeviceBatch([xs[b]], [ys[b]], inverse_order=binding.STE_GP_INVERSE_ROWS, kernel=_kind(nu))
        l1, g1, s1 = one.objective(theta[b:b + 1])
        assert not s1.any()
        np.testing.assert_allclose(lml[b], l1[0], rtol=1e-11, atol=1e-9)
        np.testing.assert_allclose(grad[b], g1[0], rtol=1e-8, atol=1e-7)
    want_lml, want_grad = _sk_lml_grad(nu, theta[37], xs[37], ys[37])
    assert np.isclose(lml[37], want_lml, rtol=1e-9, atol=1e-7)
    np.testing.assert_allclose(grad[37], want_grad, rtol=1e-6, atol=1e-5)
    sub = np.sort(rng.choice(B, 19, replace=False))
    big.t_lml.fill_(-7.0)
    big.t_grad.fill_(-7.0)
    l2, g2, s2 = big.objective(theta, active=sub.tolist())
    assert not s2.any()
    assert np.array_equal(l2[sub], lml[sub]) and np.array_equal(g2[sub], grad[sub])
    others = np.setdiff1d(np.arange(B), sub)
    assert (l2[others] == -7.0).all() and (g2[others] == -7.0).all()


@gpu
@pytest.mark.parametrize("nu", NUS)
def test_replicated_batch_keeps_the_kernel_kind(nu):
    """The restarts of a fit run on a replicated batch: it must evaluate the same kernel, to the bit."""
    from track_estimators._hip import binding
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    rng = np.random.default_rng(15)
    data = [_track(rng, n) for n in (90, 150, 181)]
    theta = np.stack([THETAS["short"], THETAS["long"], np.log([1.0, 12.0, 0.04])])
    small = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=_kind(nu))
    big = small.replicated(4)
    assert big.kernel == _kind(nu)
    l0, g0, s0 = small.objective(theta)
    l1, g1, s1 = big.objective(np.tile(theta, (4, 1)))
    assert not s0.any() and not s1.any()
    for c in range(4):
        assert np.array_equal(l1[3 * c: 3 * c + 3], l0) and np.array_equal(g1[3 * c: 3 * c + 3], g0)
    rbf = GpDeviceBatch([d[0] for d in data], [d[1] for d in data], kernel=binding.STE_GP_KERNEL_RBF)
    assert not np.array_equal(rbf.objective(theta)[0], l0)  # the kind matters


@gpu
@pytest.mark.parametrize("nu", NUS)
def test_predict_vs_sklearn(nu):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from track_estimators.gaussian_processes.gaussian_process import DeviceGaussianProcessRegressor

    rng = np.random.default_rng(16)
    x, y = _track(rng, 150)
    xq = np.sort(rng.uniform(-5.0, x[-1] + 5.0, 97))
    for th in THETAS.values():
        kernel = _sk_kernel(nu, th)
        dev = DeviceGaussianProcessRegressor(kernel, optimizer=None).fit(x[:, None], y)
        ref = GaussianProcessRegressor(kernel, optimizer=None).fit(x[:, None], y)
        mean, std = dev.predict(xq[:, None], return_std=True)
        want_mean, want_std = ref.predict(xq[:, None], return_std=True)
        np.testing.assert_allclose(mean, want_mean, rtol=1e-8, atol=1e-7)
        np.testing.assert_allclose(std, want_std, rtol=1e-5, atol=1e-6)


def _ship_track(rng, n):
    from track_estimators.ship_track import ShipTrack

    x, y = _track(rng, n)
    st = ShipTrack()
    st.dts, st.lon, st.lat = np.diff(x), y[:, 0] - 30.0, y[:, 1] + 45.0
    return st


@gpu
@pytest.mark.timeout(600)
def test_gpregression_matern_fit_vs_sklearn_and_fit_batch_matches_single_fits():
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import Matern, WhiteKernel
    from track_estimators.gaussian_processes.gaussian_process import GPRegression

    kernel = 1.0 * Matern(nu=1.5) + WhiteKernel(0.5)
    rng = np.random.default_rng(17)
    tracks = [_ship_track(rng, n) for n in (200, 170, 230)]
    kwargs = {"n_restarts_optimizer": 2, "random_state": 0}
    gp = GPRegression(kernel=kernel)
    model = gp.fit(tracks[0], dict(kwargs))
    X, y = GPRegression._training_data(tracks[0])
    ref = GaussianProcessRegressor(kernel, **kwargs).fit(X, y)
    assert np.isclose(model.log_marginal_likelihood_value_, ref.log_marginal_likelihood_value_, rtol=1e-6)
    np.testing.assert_allclose(model.kernel_.theta, ref.kernel_.theta, rtol=1e-3, atol=1e-3)
    pred, std = gp.predict(X[:, 0])
    assert pred.shape == y.shape and std.shape == y.shape
    # the lock-step batch fit: the same objective bits as the single fits, hence the same optimiser paths
    thetas, lml = GPRegression(kernel=kernel).fit_batch(tracks, gpr_kwargs=dict(kwargs))
    for b, st in enumerate(tracks):
        m = GPRegression(kernel=kernel).fit(st, dict(kwargs))
        assert np.array_equal(thetas[b], m.kernel_.theta), b
        assert lml[b] == m.log_marginal_likelihood_value_, b
