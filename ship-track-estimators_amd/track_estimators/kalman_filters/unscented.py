"""
Unscented Kalman filter + unscented RTS smoother.  Mirrors reference
``track_estimators.kalman_filters.unscented.UnscentedKalmanFilter``
(/root/reference/src/track_estimators/kalman_filters/unscented.py:19-351): same constructor, methods, attributes and
error behaviour.  All filter arithmetic runs in the HIP kernels (csrc/) through the C ABI of include/ste.h; this
class only prepares inputs, draws the noise the reference draws, and reshapes outputs.  There is no CPU fallback.

Noise: the reference adds ``np.random.normal(scale=sqrt(diag(Q or R)), size=n)`` to the predicted mean, to every
consumed observation and to the smoother's back-prediction (unscented.py:198,232,320).  This class draws from the same
global NumPy generator with the same arguments in the same call order, so ``np.random.seed(s)`` yields the same stream
as it does for the reference.  Opt-in extra (not in the reference): set ``inject_noise = False`` (class or instance
attribute) to feed zeros instead.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import logging
import types
from typing import Callable, Optional

import numpy as np

from .. import batch as _batch
from ..ship_track import ShipTrack
from .kalman_filter import KalmanFilterBase
from .non_linear_process import geodetic_dynamics as _geodetic_dynamics


def _dev():
    import torch

    return torch, torch.device("cuda", torch.cuda.current_device())


def _up(torch, dev, a, shape):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))).to(dev)


class UnscentedKalmanFilter(KalmanFilterBase):
    inject_noise = True

    def __init__(self, H=None, Q=None, R=None, P=None, x0=None, non_linear_process: Optional[Callable] = None,
                 measurement_model: Optional[Callable] = None):
        super().__init__()
        if H is None:
            raise ValueError("Set proper system dynamics.")
        self.H = H
        self.n = H.shape[1]
        self.Q = np.eye(self.n) if Q is None else np.asarray(Q)
        self.R = np.eye(self.n) if R is None else np.asarray(R)
        self.P_orig = np.eye(self.n) if P is None else np.asarray(P)
        self.P = np.eye(self.n) if P is None else np.asarray(P)
        self.x = np.zeros((self.n, 1)) if x0 is None else np.asarray(x0).reshape(-1, 1)
        self.n_sigma_points = 2 * self.n + 1
        self.sigma_points = np.zeros((self.n, self.n_sigma_points))
        self.sigma_points_orig = None
        self.weights = np.zeros((self.n_sigma_points, self.n_sigma_points))
        self.non_linear_process = non_linear_process
        self.measurement_model = measurement_model

    # -- helpers -----------------------------------------------------------------------------------------------
    def _require_dim4(self, what):
        if self.n != 4:
            raise NotImplementedError(
                f"{what}: the HIP path implements the 4-state model [lon, lat, speed, heading] only (n={self.n}); "
                "the reference itself hard-codes the heading at index 3 (unscented.py:250). No CPU fallback.")

    def _require_geodetic(self, fn):
        assert fn is not None, "Non-linear process is not set."
        assert callable(fn), "Non-linear process model must be callable."
        if fn is not _geodetic_dynamics:
            raise NotImplementedError("the HIP path implements track_estimators.kalman_filters.non_linear_process."
                                      "geodetic_dynamics only; arbitrary Python process models have no device form")

    def _draw(self, cov):
        """One reference-style draw (same generator, arguments and shape as unscented.py:198-200)."""
        if self.inject_noise:
            return np.random.normal(scale=np.sqrt(np.diag(cov)), size=(self.n))
        return np.zeros(self.n)

    def _measure(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(-1, 1)
        if self.measurement_model is not None:
            assert callable(self.measurement_model), "Measurement model must be callable."
            z = self.measurement_model(z)
        return np.asarray(z, dtype=np.float64).reshape(-1)

    def _fan_constants(self):
        n = self.n
        w0 = self.weights[0, 0]
        return n / (1 - w0), w0, self.weights[1, 1]

    # -- sigma points / weights (unscented.py:76-142) -------------------------------------------------------------
    def compute_sigma_points(self, x: Optional[np.ndarray] = None, P: Optional[np.ndarray] = None) -> np.ndarray:
        """Sigma fan ``x, x +/- columns of sqrtm(n/(1-W0) P)`` as an (n, 2n+1) array, computed on the GPU."""
        from .._hip import binding

        if x is None:
            assert self.x is not None, "Set proper initial state estimate."
            x = self.x
        if P is None:
            assert self.P is not None, "Set proper initial state covariance matrix."
            P = self.P
        n = self.n
        lib = binding.require_gpu()
        torch, dev = _dev()
        xs, Ps = _up(torch, dev, x, (n, 1)), _up(torch, dev, P, (n * n, 1))
        out = torch.empty((2 * n + 1, n, 1), dtype=torch.float64, device=dev)
        scale = n / (1 - self.weights[0, 0])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if n == 4:
            binding.check(lib.ste_sigma_points_f64(1, xs.data_ptr(), Ps.data_ptr(), C.c_double(scale), out.data_ptr(),
                                                   stream), "ste_sigma_points_f64")
        else:
            binding.check(lib.ste_sigma_points_generic_f64(n, 1, xs.data_ptr(), Ps.data_ptr(), C.c_double(scale),
                                                           out.data_ptr(), stream), "ste_sigma_points_generic_f64")
        self.sigma_points[:, :] = out.cpu().numpy()[:, :, 0].T
        return self.sigma_points

    def compute_weights(self, weight0: Optional[float] = None) -> np.ndarray:
        """Diagonal (2n+1)x(2n+1) weight matrix: W0 = 1 - n/3 (or ``weight0``), Wi = (1 - W0)/(2n)."""
        if weight0 is None:
            weight0 = 1 - self.n / 3.0
        assert weight0 < 1.0 and weight0 > -1.0, "Weight0 value ({}) is outside [-1, 1] range.".format(weight0)
        weightn = (1 - weight0) / (2 * self.n)
        np.fill_diagonal(self.weights, weightn)
        self.weights[0, 0] = weight0
        logging.debug("Weights\n\n%s", self.weights)
        return self.weights

    # -- single-step API (unscented.py:144-265) -------------------------------------------------------------------
    def predict(self, non_linear_process: Optional[Callable] = None, **non_linear_process_kwargs) -> None:
        """One predict step (unscented.py:144-207).  kwargs: ``dt``, ``c`` (must be None), ``sog_rate``, ``cog_rate``."""
        from .._hip import binding

        if non_linear_process is None:
            assert self.non_linear_process is not None, "Non-linear process is not set."
            non_linear_process = self.non_linear_process
        self._require_geodetic(non_linear_process)
        self._require_dim4("predict")
        kw = dict(non_linear_process_kwargs)
        c = kw.pop("c", None)
        if c is not None and np.size(c):
            raise NotImplementedError("control vector c must be None on the HIP path (the reference passes None, "
                                      "kalman_filter.py:92)")
        dt = kw.pop("dt")
        sr, cr = kw.pop("sog_rate", 0.0), kw.pop("cog_rate", 0.0)
        if kw:
            raise TypeError(f"unexpected process-model arguments: {sorted(kw)}")
        self.x = np.asarray(self.x).reshape(-1, 1)
        self.compute_weights()
        fan_scale, w0, wi = self._fan_constants()
        noise = self._draw(self.Q)
        lib = binding.require_gpu()
        torch, dev = _dev()
        x, P = _up(torch, dev, self.x, (4, 1)), _up(torch, dev, self.P, (16, 1))
        d, a, b = (_up(torch, dev, v, (1,)) for v in (dt, sr, cr))
        nz = _up(torch, dev, noise, (4, 1))
        Q = _batch._as44(self.Q, "Q", True)
        _batch.require_symmetric(np.asarray(self.P, dtype=np.float64).reshape(4, 4), "P")
        xo, Po = torch.empty_like(x), torch.empty_like(P)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        binding.check(lib.ste_ukf_predict_f64(1, x.data_ptr(), P.data_ptr(), d.data_ptr(), a.data_ptr(), b.data_ptr(),
                                              nz.data_ptr(), Q.ctypes.data, fan_scale, w0, wi, xo.data_ptr(),
                                              Po.data_ptr(), None, stream), "ste_ukf_predict_f64")
        self.x = xo.cpu().numpy().reshape(4, 1)
        self.P = Po.cpu().numpy().reshape(4, 4)

    def update(self, z: np.ndarray) -> None:
        """One measurement update (unscented.py:209-265): pinv gain, heading wrap, Joseph-form covariance."""
        from .._hip import binding

        self._require_dim4("update")
        zz = self._measure(z)
        noise = self._draw(self.R)
        lib = binding.require_gpu()
        torch, dev = _dev()
        x, P = _up(torch, dev, self.x, (4, 1)), _up(torch, dev, self.P, (16, 1))
        zt, nz = _up(torch, dev, zz, (4, 1)), _up(torch, dev, noise, (4, 1))
        H, R = _batch._as44(self.H, "H"), _batch._as44(self.R, "R", True)
        _batch.require_symmetric(np.asarray(self.P, dtype=np.float64).reshape(4, 4), "P")
        xo, Po = torch.empty_like(x), torch.empty_like(P)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        binding.check(lib.ste_ukf_update_f64(1, x.data_ptr(), P.data_ptr(), zt.data_ptr(), nz.data_ptr(), H.ctypes.data,
                                             R.ctypes.data, xo.data_ptr(), Po.data_ptr(), None, stream),
                      "ste_ukf_update_f64")
        self.x = xo.cpu().numpy().reshape(4, 1)
        self.P = Po.cpu().numpy().reshape(4, 4)

    # -- whole-track API ------------------------------------------------------------------------------------------
    def _launch_forward(self, dt, ship_track):
        """Forward pass of ``run`` for this one track on the GPU (kalman_filter.py:61-117)."""
        self._require_geodetic(self.non_linear_process)
        self._require_dim4("run")
        self.compute_weights()
        N = len(dt)
        z = np.asarray(ship_track.z, dtype=np.float64)
        if self.measurement_model is not None:
            z = np.stack([self._measure(z[:, j]) for j in range(z.shape[1])], axis=1)
        upd_idx, _, t_end = _batch.update_schedule(dt, ship_track.dts, self.time)
        # noise in the reference's call order: initial update, then per step predict (+ update if it fires)
        npred = np.zeros((N, 4))
        nupd = np.zeros((N + 1, 4))
        nupd[0] = self._draw(self.R)
        for k in range(N):
            npred[k] = self._draw(self.Q)
            if upd_idx[k] >= 0:
                nupd[k + 1] = self._draw(self.R)
        trk = types.SimpleNamespace(z=z, dts=ship_track.dts, sog_rate=ship_track.sog_rate, cog_rate=ship_track.cog_rate)
        hb = _batch.pack_tracks([trk], [dt], [np.asarray(self.x, dtype=np.float64).reshape(-1)], self.H, self.Q, self.R,
                                np.asarray(self.P, dtype=np.float64), t0s=[self.time],
                                noise=[dict(noise_pred=npred, noise_upd=nupd, noise_rts=np.zeros((N, 4)))],
                                on_error="raise")
        self._sample_hb = hb  # what sample_smoothed re-runs: this track as run() packed it, recorded noise included
        out = _batch.run_batch(hb, smooth=False)
        self._status = int(out["status"][0])
        if self._status & 0x1:
            # the reference dies inside np.linalg.pinv once a NaN/inf reaches the covariance (e.g. dt = 0 -> sog = inf)
            raise np.linalg.LinAlgError("SVD did not converge")
        return out["means"][0], out["covs"][0], upd_idx, t_end

    def rts_step(self, fwd_means, fwd_vars, ship_track: ShipTrack, *args, **kwargs):
        """
        Unscented RTS smoother over a stored forward history (unscented.py:267-351).

        ``fwd_means`` (N+1, n, 1) or (N+1, n); ``fwd_vars`` (N+1, n, n).  Like the reference this expands
        ``ship_track.sog_rate`` / ``cog_rate`` in place with ``np.repeat`` (:287-292), so a second call on the same
        ShipTrack sees the already-expanded arrays.
        """
        self._require_geodetic(self.non_linear_process)
        self._require_dim4("rts_step")
        fwd_means = np.asarray(fwd_means, dtype=np.float64)
        nrows = fwd_means.shape[0]
        rep = int(nrows / len(ship_track.dts))
        ship_track.sog_rate = np.repeat(ship_track.sog_rate, rep)
        ship_track.cog_rate = np.repeat(ship_track.cog_rate, rep)
        N = nrows - 1
        dt = np.asarray(self.dt, dtype=np.float64)
        if N > len(dt) or N > len(ship_track.sog_rate):
            raise IndexError("index out of bounds: smoother needs dt and expanded rates for every stored step")
        self.compute_weights()
        nrts = np.zeros((N, 4))
        for k in range(N - 1, -1, -1):  # the reference draws while walking backwards (:297,320)
            nrts[k] = self._draw(self.Q)
        from .._hip import binding

        lib = binding.require_gpu()
        torch, dev = _dev()
        m = fwd_means.reshape(nrows, 4)
        _batch.require_symmetric(np.asarray(fwd_vars, dtype=np.float64).reshape(nrows, 4, 4), "fwd_vars")
        hb = _batch.HostBatch(
            B=1, Nmax=N, Tmax=1, H=_batch._as44(self.H, "H"), Q=_batch._as44(self.Q, "Q", True), R=_batch._as44(self.R, "R", True),
            nsteps=np.array([N], dtype=np.int32), x0=np.ascontiguousarray(m[0].reshape(4, 1)),
            P0=np.ascontiguousarray(np.asarray(fwd_vars[0], dtype=np.float64).reshape(16)),
            dt=np.ascontiguousarray(dt[:N].reshape(N, 1)),
            sog_rate=np.ascontiguousarray(np.asarray(ship_track.sog_rate[:N], dtype=np.float64).reshape(N, 1)),
            cog_rate=np.ascontiguousarray(np.asarray(ship_track.cog_rate[:N], dtype=np.float64).reshape(N, 1)),
            sog_rate_rts=None, cog_rate_rts=None, upd_idx=np.full((N, 1), -1, dtype=np.int32), z=np.zeros((1, 4, 1)),
            noise_pred=None, noise_upd=None, noise_rts=nrts.reshape(N, 4, 1))
        # the history comes from the caller, not from a forward launch on this batch: no precomputed gains
        db = _batch.DeviceBatch(hb, fuse_gains=False, packed_cov=False)  # the caller's full matrices go in as they are
        db.fwd_mean.copy_(_up(torch, dev, m, (nrows, 4, 1)))
        db.fwd_cov.copy_(_up(torch, dev, fwd_vars, (nrows, 16, 1)))
        db.backward()
        torch.cuda.synchronize(dev)
        sm, sP = db.smoothed()
        self._status_smoother = int(db.status_host()[0])
        if self._status_smoother & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return sm[0].reshape(nrows, 4, 1), sP[0]

    def sample_smoothed(self, n_samples: int, random_state: int = 0) -> np.ndarray:
        """``n_samples`` tracks drawn from the joint smoothing posterior of the track ``run`` filtered, (n_samples, N+1, 4):
        what ``run_rts_smoother`` gives as a mean and a covariance per row, as whole tracks whose rows are tied together by
        the smoother gains (``track_estimators.batch.sample_tracks``; no counterpart in the reference).  The track is packed
        as ``run`` packed it -- the noise ``run`` drew included, so the forward pass is the stored one -- and sampled on the
        device; the noise ``run_rts_smoother`` would inject into its back-predictions is not part of the posterior and is
        left out.  ``random_state`` seeds the device generator."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("sample_smoothed() samples the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("sample_smoothed() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        samples, status = _batch.sample_tracks(hb, int(n_samples), seed=int(random_state))
        self._status_sampler = int(status[0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return samples[:, 0]

    def fit_measurement_noise(self, structure: str = "scalar", max_iter: int = 20, rtol: float = 1e-3):
        """The measurement noise R that fits the track ``run`` filtered, by EM on the device
        (``track_estimators.batch.fit_measurement_noise``; no counterpart in the reference, where R is an argument).  The
        track is packed as ``run`` packed it but without the noise ``run`` drew: the fit is that of the deterministic filter.
        Returns ``(R (4, 4), loglik (iterations + 1,))``: the iterate with the highest log-likelihood and the trace, iterate 0
        being this filter's own R, which is left as it is."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("fit_measurement_noise() fits the track of the last run(): call run() first")
        hb = dataclasses.replace(hb, noise_pred=None, noise_upd=None, noise_rts=None)
        fit = _batch.fit_measurement_noise(hb, structure=structure, max_iter=max_iter, rtol=rtol)
        return fit.R[0], fit.loglik[:, 0]

    def distance_sailed(self, n_samples: int = 0, random_state: int = 0, model: str = "sphere"):
        """Distance in km along the track ``run`` filtered (``track_estimators.batch.path_statistics``; no counterpart in the
        reference, whose callers loop over ``utils.haversine_formula`` themselves).  ``n_samples == 0``: the distance of the
        smoothed track, a float.  Otherwise an ``(n_samples,)`` array: the distances of that many tracks drawn from the joint
        smoothing posterior, those of ``sample_smoothed(n_samples, random_state)``.  ``model``: "sphere" (haversine on the
        6378.137 km sphere) or "wgs84".  The track is packed as ``run`` packed it, as for ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("distance_sailed() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("distance_sailed() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        if n_samples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            return float(db.path_metrics(db.sm_mean, model=model)["distance"][0, 0].item())
        out = _batch.path_statistics(hb, n_samples, seed=int(random_state), chunk=n_samples, model=model)
        self._status_sampler = int(out["status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return out["distance"][:, 0]

    def time_in_region(self, polygon, n_samples: int = 0, random_state: int = 0):
        """Hours the track ``run`` filtered spends inside ``polygon``, a (V, 2) array of lon / lat degrees, planar as in
        GeoJSON (``track_estimators.batch.region_statistics``; no counterpart in the reference).  ``n_samples == 0``: the time
        of the smoothed track, a float.  Otherwise an ``(n_samples,)`` array: the times of that many tracks drawn from the
        joint smoothing posterior, those of ``sample_smoothed(n_samples, random_state)``.  The track is packed as ``run``
        packed it, as for ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("time_in_region() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("time_in_region() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        poly = _batch.region_polygon(polygon)
        if n_samples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            return float(db.region_metrics(db.sm_mean, poly)["time_inside"][0, 0].item())
        out = _batch.region_statistics(hb, poly, n_samples, seed=int(random_state), chunk=n_samples)
        self._status_sampler = int(out["status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return out["time_inside"][:, 0]

    def time_on_grid(self, grid, n_samples: int = 0, random_state: int = 0):
        """Hours the track ``run`` filtered spends in every cell of ``grid``, a ``track_estimators.batch.TrackGrid``
        (``track_estimators.batch.track_grid`` makes one; no counterpart in the reference): an (ny, nx) array.
        ``n_samples == 0``: the map of the smoothed track.  Otherwise the mean of the maps of that many tracks drawn from the
        joint smoothing posterior, those of ``sample_smoothed(n_samples, random_state)``.  The track is packed as ``run``
        packed it, as for ``time_in_region``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("time_on_grid() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("time_on_grid() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        if not isinstance(grid, _batch.TrackGrid):
            raise ValueError("grid must be a TrackGrid (track_estimators.batch.track_grid makes one)")
        if n_samples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            return db.grid_metrics(db.sm_mean, grid)["hours"].cpu().numpy()
        out = _batch.grid_statistics(hb, grid, n_samples, seed=int(random_state), chunk=n_samples)
        self._status_sampler = int(out["status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return out["hours_mean"]

    def raster_along_track(self, raster, threshold=None, below: bool = False, min_hours: float = 0.0, n_samples: int = 0,
                           random_state: int = 0):
        """The values of a gridded field -- a land mask, a depth, a density -- along the track ``run`` filtered
        (``DeviceBatch.raster_metrics`` and ``track_estimators.batch.raster_statistics``; no counterpart in the reference).
        ``raster``: a ``track_estimators.batch.TrackRaster`` (``track_estimators.batch.track_raster`` makes one);
        ``threshold``, ``below`` and ``min_hours`` as in ``raster_metrics``.  Returns a dict of the smoothed track's values,
        every output of ``raster_metrics`` as a scalar, and ``row_value`` (N+1,), the field at every row.  With ``n_samples``
        also ``posterior``, a dict of what ``raster_statistics`` gives over that many tracks drawn from the joint smoothing
        posterior, those of ``sample_smoothed(n_samples, random_state)``: ``mean`` (n_samples,), ``mean_quantiles``,
        ``nbroken`` and, with ``threshold``, ``hit_hours``, ``hit_hours_mean``, ``hit_hours_quantiles``, ``p_hit``,
        ``p_hit_long``.  The track is packed as ``run``
        packed it, as for ``time_on_grid``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("raster_along_track() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("raster_along_track() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        if not isinstance(raster, _batch.TrackRaster):
            raise ValueError("raster must be a TrackRaster (track_estimators.batch.track_raster makes one)")
        kw = dict(threshold=threshold, below=below, min_hours=min_hours)
        db = _batch.DeviceBatch(hb)
        db.run()
        if int(db.status_host()[0]) & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        got = db.raster_metrics(db.sm_mean, raster, rows=True, **kw)
        res = {k: v[0, ..., 0].cpu().numpy() for k, v in got.items()}
        if n_samples == 0:
            return res
        out = _batch.raster_statistics(db, raster, n_samples, seed=int(random_state), chunk=n_samples, **kw)
        self._status_sampler = int(out["status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        res["posterior"] = {k: v[..., 0] for k, v in out.items() if not k.endswith("_smoothed") and k != "status"}
        return res

    def position_at(self, times, n_samples: int = 0, random_state: int = 0, covariance: bool = False):
        """Where the track ``run`` filtered was at ``times``, hours from its first row
        (``track_estimators.batch.position_statistics``; no counterpart in the reference, whose callers search and interpolate
        the history themselves).  A position is linear in time inside a step, a time that is a step time returns that row, and
        a time before the first or after the last row gives NaN.  ``n_samples == 0``: the smoothed track there, a
        ``(len(times), 4)`` array of lon, lat, speed, heading.  Otherwise a dict: ``position``, that array, and per time
        ``count``, ``mean_east_km``, ``mean_north_km``, ``cov_km``, ``semi_major_km``, ``semi_minor_km``, ``orientation_deg``
        (the 95 % ellipse) from that many tracks drawn from the joint smoothing posterior, those of
        ``sample_smoothed(n_samples, random_state)``.  ``covariance=True`` (with ``n_samples == 0``): a dict with ``position`` and
        the EXACT ``cov_km``, ``semi_major_km``, ``semi_minor_km``, ``orientation_deg`` of the smoothing posterior there, in
        closed form from the smoothed covariances and the smoother's lag-one covariance, without samples
        (``track_estimators.batch.position_covariance``).  The track is packed as ``run`` packed it, as for ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("position_at() reads the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("position_at() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        times = np.atleast_1d(np.asarray(times, dtype=np.float64))
        if times.ndim != 1 or times.size < 1:
            raise ValueError(f"times must be a scalar or a one-dimensional array of hours, got shape {times.shape}")
        track = np.zeros(times.size, dtype=np.int32)
        if covariance:
            if n_samples != 0:
                raise ValueError("covariance=True gives the exact covariance and draws no samples: leave n_samples at 0")
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            out = _batch.position_covariance(db, track, times)
            self._status_lag_one = int(out["lag_status"][0])
            if self._status_lag_one & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            res = {"position": np.stack([out[k] for k in ("lon", "lat", "speed", "heading")], axis=1)}
            res.update({k: out[k] for k in ("cov_km", "semi_major_km", "semi_minor_km", "orientation_deg")})
            return res
        if n_samples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            got = db.positions_at(db.sm_mean, track, times, velocity=True)
            return np.stack([got[k][0].cpu().numpy() for k in ("lon", "lat", "speed", "heading")], axis=1)
        out = _batch.position_statistics(hb, track, times, n_samples, seed=int(random_state), chunk=n_samples)
        self._status_sampler = int(out["sample_status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        res = {"position": np.stack([out[k] for k in ("lon", "lat", "speed", "heading")], axis=1)}
        res.update({k: out[k] for k in ("count", "mean_east_km", "mean_north_km", "cov_km", "semi_major_km", "semi_minor_km",
                                        "orientation_deg")})
        return res

    def field_at(self, field, times, n_samples: int = 0, random_state: int = 0):
        """The value of a space-time gridded field where the track ``run`` filtered was at ``times``, hours from its first
        row (``DeviceBatch.field_at`` and ``track_estimators.batch.field_statistics``; no counterpart in the reference).
        ``field``: a ``track_estimators.batch.TrackField`` whose time axis runs on the same clock.  ``n_samples == 0``: a
        ``(len(times),)`` array, the field at the smoothed track, trilinear, NaN where the track or the field has nothing.
        Otherwise the dict of ``field_statistics`` from that many tracks drawn from the joint smoothing posterior, those of
        ``sample_smoothed(n_samples, random_state)``: ``anchor`` (that array), ``mean``, ``std``, ``min``, ``max``, ``n``,
        ``p_nodata``, ``p_off``, ``status``.  The track is packed as ``run`` packed it, as for ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("field_at() reads the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("field_at() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        times = np.atleast_1d(np.asarray(times, dtype=np.float64))
        if times.ndim != 1 or times.size < 1:
            raise ValueError(f"times must be a scalar or a one-dimensional array of hours, got shape {times.shape}")
        track = np.zeros(times.size, dtype=np.int32)
        if n_samples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            return db.field_at(db.sm_mean, field, track, times)["value"][0].cpu().numpy()
        out = _batch.field_statistics(hb, field, track, times, n_samples, seed=int(random_state), chunk=n_samples)
        self._status_sampler = int(out.pop("sample_status")[0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return out

    def site_visits(self, sites, radius_km, nsamples: int = 0, min_stay_h: float = 0.0, model: str = "sphere",
                    random_state: int = 0):
        """The track ``run`` filtered against fixed sites -- ports, anchorages, buoys -- (``DeviceBatch.site_metrics`` and
        ``track_estimators.batch.site_statistics``; no counterpart in the reference).  ``sites``: (M, 2) lon / lat in
        degrees; ``radius_km``: a scalar or one radius per site; times are hours from the first row.  ``nsamples == 0``: a
        dict of (M,) arrays of the smoothed track, ``min_dist`` (km), ``min_time``, ``time_within``, ``first_within``,
        ``longest``, ``nwithin``, and ``nearest``, the index of the closest site (-1 without one).  Otherwise those under
        ``*_smoothed`` names and per site ``visit_prob`` (the fraction of that many tracks drawn from the joint smoothing
        posterior that come within the radius), ``call_prob`` (that stay ``min_stay_h`` or longer at a stretch) and the means
        ``min_dist_mean``, ``time_within_mean``, ``longest_mean``.  The track is packed as ``run`` packed it, as for
        ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("site_visits() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("site_visits() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        nsamples = int(nsamples)
        if nsamples < 0:
            raise ValueError(f"nsamples must be >= 0, got {nsamples!r}")
        names = ("min_dist", "min_time", "time_within", "first_within", "longest", "nwithin")
        if nsamples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            got = db.site_metrics(db.sm_mean, sites, radius_km, model=model)
            res = {k: got[k][0, :, 0].cpu().numpy() for k in names}
            res["nearest"] = int(_batch.nearest_site(got["min_dist"])[0][0, 0].item())
            return res
        out = _batch.site_statistics(hb, sites, radius_km, nsamples, seed=int(random_state), chunk=nsamples,
                                     min_stay_h=min_stay_h, model=model)
        self._status_sampler = int(out["sample_status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        res = {k + "_smoothed": out[k + "_smoothed"][:, 0] for k in names}
        res.update({k: out[k][:, 0] for k in ("visit_prob", "call_prob", "min_dist_mean", "time_within_mean", "longest_mean")})
        return res

    def speed_profile(self, bands=None, threshold=None, above: bool = False, min_run_h: float = 0.0, limit_kmh=None,
                      nsamples: int = 0, model: str = "sphere", random_state: int = 0):
        """How fast the track ``run`` filtered went (``DeviceBatch.speed_metrics`` and
        ``track_estimators.batch.speed_statistics``; no counterpart in the reference).  Speeds are km/h
        (``track_estimators.batch.KNOT_KMH`` to the knot), times hours from the first row; ``bands``, ``threshold``, ``above``
        and ``min_run_h`` as in ``speed_metrics``.  ``nsamples == 0``: a dict of the smoothed track's values, ``dist``,
        ``sound_time``, ``mean_speed``, ``vmax``, ``vmax_time``, ``nbroken``, ``speed`` (one per step), with ``bands``
        ``band_time`` (nbands,), with ``threshold`` ``cond_time``, ``run_time``, ``nruns``, ``first_run``, ``longest``,
        ``longest_start``, and with ``limit_kmh`` ``exceeds``, whether ``vmax`` is above it.  Otherwise those (but ``speed`` and
        ``exceeds``) under ``*_smoothed`` names and, over that many tracks drawn from the joint smoothing posterior, the
        ``*_mean``, ``*_std`` and ``*_quantiles`` of ``mean_speed`` and ``vmax``, ``exceed_prob`` (with ``limit_kmh``),
        ``run_prob``, ``cond_time_mean``, ``run_time_mean`` (with ``threshold``) and ``band_time_mean`` (with ``bands``).  The
        track is packed as ``run`` packed it, as for ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("speed_profile() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("speed_profile() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        nsamples = int(nsamples)
        if nsamples < 0:
            raise ValueError(f"nsamples must be >= 0, got {nsamples!r}")
        kw = dict(bands=bands, threshold=threshold, above=above, min_run_h=min_run_h, model=model)
        if nsamples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            got = db.speed_metrics(db.sm_mean, per_step=True, **kw)
            res = {k: v[0, ..., 0].cpu().numpy() for k, v in got.items() if k != "track_status"}
            with np.errstate(invalid="ignore", divide="ignore"):
                res["mean_speed"] = res["dist"] / res["sound_time"]
            if limit_kmh is not None:
                res["exceeds"] = bool(res["vmax"] > float(limit_kmh))
            return res
        out = _batch.speed_statistics(hb, nsamples, seed=int(random_state), chunk=nsamples, limit_kmh=limit_kmh, **kw)
        self._status_sampler = int(out["status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return {k: v[..., 0] for k, v in out.items() if k not in ("status", "track_status", "mean_speed", "vmax")}

    def simplified_track(self, tolerance_km, which: str = "smoothed", shape: bool = False, lon_scale="track"):
        """The track ``run`` filtered, simplified within ``tolerance_km`` on the device
        (``track_estimators.batch.simplified_tracks``; no counterpart in the reference): a ``SimplifiedTrack``, a dict of
        the kept rows only, ``rows``, ``lon``, ``lat``, ``speed``, ``heading`` and ``time`` (hours from the first row), with
        ``worst_km`` and ``status``; its ``curves()`` gives the (n, 2) lon / lat arrays that ``curve_distance`` and
        ``track_lines`` take.  ``which``: "smoothed" or "filtered".  The default rule keeps ``positions_at`` within the
        tolerance at every row time; ``shape`` asks about the curve alone.  The track is packed as ``run`` packed it, as for
        ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("simplified_track() simplifies the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("simplified_track() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        return _batch.simplified_tracks(hb, tolerance_km, which=which, shape=shape, lon_scale=lon_scale)[0]

    def track_error(self, truth=None, n_samples: int = 0, course=None, coverage: float = 0.95, within_km=None,
                    quantiles=None, model: str = "sphere", random_state: int = 0):
        """How far the track ``run`` filtered is from truth positions (``DeviceBatch.track_errors`` and
        ``track_estimators.batch.error_statistics``; the reference's ``performance_metrics`` compares degrees row by row).
        ``truth``: (Nmax+1, 2) lon / lat at the track's own rows, NaN where there is none; None takes the ship track's own
        observations at the rows whose update used them (``track_estimators.batch.observation_rows``).  ``course``: None or
        (Nmax+1,) degrees (``track_estimators.batch.truth_course``).  ``n_samples == 0``: a dict of the smoothed track's
        values, every output of ``track_errors`` with ``cov="sm"``, per-row and cumulative ones included, scalars and
        (Nmax+1,) arrays.  Otherwise the outputs of ``error_statistics`` for that many tracks drawn from the joint smoothing
        posterior (``status`` apart), ``rmse`` as (n_samples,).  The track is packed as ``run`` packed it, as for
        ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("track_error() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("track_error() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError(f"n_samples must be >= 0, got {n_samples!r}")
        if truth is None:
            truth = _batch.observation_rows(hb)
        else:
            truth = np.asarray(truth, dtype=np.float64)
            if truth.shape != (hb.Nmax + 1, 2):
                raise ValueError(f"truth must be None or have shape ({hb.Nmax + 1}, 2), got {truth.shape}")
            truth = np.ascontiguousarray(truth[:, :, None])
        if course is not None:
            course = np.asarray(course, dtype=np.float64)
            if course.shape != (hb.Nmax + 1,):
                raise ValueError(f"course must be None or have shape ({hb.Nmax + 1},), got {course.shape}")
            course = np.ascontiguousarray(course[:, None])
        if n_samples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            got = db.track_errors(db.sm_mean, truth, course=course, cov="sm", coverage=coverage, model=model, rows=True,
                                  cumulative=True)
            return {k: v[0, ..., 0].cpu().numpy() for k, v in got.items()}
        out = _batch.error_statistics(hb, truth, n_samples, seed=int(random_state), chunk=n_samples, course=course, model=model,
                                      within_km=within_km, quantiles=quantiles)
        self._status_sampler = int(out["status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        return {k: v[..., 0] for k, v in out.items() if k != "status"}

    def line_approach(self, lines, nsamples: int = 0, within_km=None, model: str = "sphere", random_state: int = 0):
        """The track ``run`` filtered against polylines -- coasts, cables, routes, gates -- (``DeviceBatch.line_metrics``
        and ``track_estimators.batch.line_statistics``; no counterpart in the reference).  ``lines``: a list of (n, 2) lon /
        lat arrays in degrees, or what ``track_estimators.batch.track_lines`` made of one; times are hours from the first row.
        ``nsamples == 0``: a dict of (M,) arrays of the smoothed track, ``min_dist`` (km), ``min_time``, ``min_seg``,
        ``min_frac``, ``ncross``, ``net_cross``, ``first_cross``, ``last_cross``, and ``chainage``, the km along each line
        from its first vertex to the closest point.  Otherwise those (but ``chainage``) under ``*_smoothed`` names and per
        line ``cross_prob`` (the fraction of that many tracks drawn from the joint smoothing posterior that cross the
        line), ``net_prob`` (that end on its other side), ``first_cross_mean``, ``min_dist_mean`` and, with ``within_km``,
        ``approach_prob`` (that come that close).  The track is packed as ``run`` packed it, as for ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("line_approach() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("line_approach() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        nsamples = int(nsamples)
        if nsamples < 0:
            raise ValueError(f"nsamples must be >= 0, got {nsamples!r}")
        names = ("min_dist", "min_time", "min_seg", "min_frac", "ncross", "net_cross", "first_cross", "last_cross")
        tl = _batch.track_lines(lines)
        if nsamples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            got = db.line_metrics(db.sm_mean, tl, model=model)
            res = {k: got[k][0, :, 0].cpu().numpy() for k in names}
            res["chainage"] = _batch.line_chainage(tl, got["min_seg"], got["min_frac"], model=model)[0, :, 0].cpu().numpy()
            return res
        out = _batch.line_statistics(hb, tl, nsamples, seed=int(random_state), chunk=nsamples, within_km=within_km, model=model)
        self._status_sampler = int(out["sample_status"][0])
        if self._status_sampler & 0x1:
            raise np.linalg.LinAlgError("SVD did not converge")
        res = {k + "_smoothed": out[k + "_smoothed"][:, 0] for k in names}
        keys = ("cross_prob", "net_prob", "first_cross_mean", "min_dist_mean") + (("approach_prob",) if within_km is not None else ())
        res.update({k: out[k][:, 0] for k in keys})
        return res

    def route_distance(self, curve, nsamples: int = 0, dtw: bool = False, reverse: bool = False, model: str = "sphere",
                       random_state: int = 0):
        """The track ``run`` filtered against another curve -- its own observations, a planned route, a GP or Savitzky-Golay
        track of the same ship -- as curves without a clock (``track_estimators.batch.curve_distance``; the reference's
        ``performance_metrics.py`` compares two tracks row by row, which needs equal rows).  ``curve``: an (n, 2) array of
        lon / lat in degrees, of any length.  ``nsamples == 0``: the smoothed track against ``curve``, a dict of ``frechet``
        (km, a float: the discrete Frechet distance), ``frechet_at`` (the rows of the track and of ``curve`` whose distance
        it is), ``status`` and, with ``dtw``, ``dtw`` (km, the time-warping cost) and ``dtw_len`` (the cells on its path).
        Otherwise the same keys as arrays over that many tracks drawn from the joint smoothing posterior, those of
        ``sample_smoothed(nsamples, random_state)``.  ``reverse``: ``curve`` is read from its last point to its first.
        ``model``: the leg function of ``frechet``, "sphere" or "wgs84".  The track is packed as ``run`` packed it, as for
        ``sample_smoothed``."""
        hb = getattr(self, "_sample_hb", None)
        if hb is None:
            raise RuntimeError("route_distance() measures the track of the last run(): call run() first")
        if len(self.means) != hb.Nmax + 1:
            raise NotImplementedError("route_distance() covers a history filtered by ONE run() call; this filter has "
                                      f"{len(self.means)} stored rows and its last run() made {hb.Nmax + 1}")
        nsamples = int(nsamples)
        if nsamples < 0:
            raise ValueError(f"nsamples must be >= 0, got {nsamples!r}")
        curve = np.asarray(curve, dtype=np.float64)
        kw = dict(dtw=dtw, reverse=reverse, model=model)
        if nsamples == 0:
            db = _batch.DeviceBatch(hb)
            db.run()
            if int(db.status_host()[0]) & 0x1:
                raise np.linalg.LinAlgError("SVD did not converge")
            track = db.sm_mean[:, :2, 0].cpu().numpy()
            got = _batch.curve_distance([track], [curve], **kw)
            res = {"frechet": float(got["frechet"][0]), "frechet_at": tuple(int(v) for v in got["frechet_at"][0]),
                   "status": int(got["status"][0])}
            if dtw:
                res.update(dtw=float(got["dtw"][0]), dtw_len=int(got["dtw_len"][0]))
            return res
        samples = self.sample_smoothed(nsamples, random_state)
        return _batch.curve_distance([np.ascontiguousarray(t[:, :2]) for t in samples], [curve] * nsamples, **kw)

    # -- robustification helpers (unscented.py:353-511) -------------------------------------------------------------
    # The reference's call site is commented out (unscented.py:228), so ``run`` never invokes these; they are kept as
    # callable methods with the reference's signatures.  The batched path offers the same loop as an opt-in flag
    # (``HostBatch.robust``), evaluated inside the update kernel.
    def _robust_terms(self, z, P, R):
        """(gamma, denom) of unscented.py:420-426 and :468-478 for this filter's x and H, computed on the GPU."""
        from .._hip import binding

        self._require_dim4("robustification")
        lib = binding.require_gpu()
        torch, dev = _dev()
        x, Pm = _up(torch, dev, self.x, (4, 1)), _up(torch, dev, P, (16, 1))
        zt = _up(torch, dev, np.asarray(z, dtype=np.float64).reshape(-1), (4, 1))
        H, Rm = _batch._as44(self.H, "H"), _batch._as44(R, "R", True)
        _batch.require_symmetric(np.asarray(P, dtype=np.float64).reshape(4, 4), "P")
        g, d = torch.empty((1,), dtype=torch.float64, device=dev), torch.empty((1,), dtype=torch.float64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        binding.check(lib.ste_ukf_robust_terms_f64(1, x.data_ptr(), Pm.data_ptr(), zt.data_ptr(), H.ctypes.data,
                                                   Rm.ctypes.data, g.data_ptr(), d.data_ptr(), stream),
                      "ste_ukf_robust_terms_f64")
        return float(g.item()), float(d.item())

    def criterion_index(self, z: np.ndarray, P: np.ndarray, R: np.ndarray) -> float:
        """Mahalanobis judging index ``|y^T (H P H^T + R)^+ y|`` with ``y = z - x`` (unscented.py:389-428)."""
        return self._robust_terms(z, P, R)[0]

    def update_lambda_factor(self, lambda_factor: float, criterion_index: float, chi_alpha: float, z: np.ndarray,
                             P: np.ndarray, R: np.ndarray) -> float:
        """``lambda + (criterion - chi_alpha) / (y^T S^+ R S^+ y)`` (unscented.py:430-483)."""
        _, denom = self._robust_terms(z, P, R)
        return float(lambda_factor + (criterion_index - chi_alpha) / denom)

    def scale_measurement_uncertainty(self, R: np.ndarray, lambda_factor: float) -> np.ndarray:
        """``R * lambda`` (unscented.py:485-511)."""
        return R * lambda_factor

    def check_robustness(self, z: np.ndarray, P: np.ndarray, R: np.ndarray) -> np.ndarray:
        """The reference's rescaling loop (unscented.py:353-387), including its fresh noise draw per iteration and its
        prints; returns the scaled R."""
        lambda_factor = 1
        chi_alpha = 50
        z = np.asarray(z, dtype=np.float64).reshape(-1, 1)
        zn = z + self._draw(R).reshape(-1, 1)
        judging_index = self.criterion_index(zn, P, R)
        print(judging_index, lambda_factor)
        while judging_index > chi_alpha:
            zn = z + self._draw(R).reshape(-1, 1)
            lambda_factor = self.update_lambda_factor(lambda_factor, judging_index, chi_alpha, zn, P, R)
            R = self.scale_measurement_uncertainty(R, lambda_factor)
            judging_index = self.criterion_index(zn, P, R)
            print(judging_index, lambda_factor)
        return R
