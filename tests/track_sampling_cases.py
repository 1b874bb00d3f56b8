"""NumPy restatement of the posterior track sampler (include/ste.h: ste_urtss_sample_f64; DESIGN.md, "Posterior tracks")
and the small batches its tests share.  The per-step quantities are formed with the calls ``oracle.ukf_oracle.backward_track``
issues (same fan, same propagation, same ``np.dot`` products), so that with zero draws the recursion below reproduces its
smoothed means exactly.

For a track of ns steps, with m_k, P_k the filtered row k and x_b, P_b (about the filtered mean), D, K = D pinv(P_b) of step k:
    row ns:  x_ns = m_ns + T_ns xi_ns,                                     T_ns = symsqrt(P_ns)
    row k :  y = x_{k+1} - x_b, y[3] wrapped;  x_k = (m_k + K y) + T_k xi_k,   T_k = symsqrt(P_k - K P_b K^T)
    x_k[3] = x_k[3] mod 360, row ns included
"""
import dataclasses

import numpy as np

from oracle import ukf_oracle as orc

NOBS, SUBSTEPS, SEED0 = 7, 2, 100  # the eight tracks of the tests: 7 observations, 2 substeps -> Nmax = 12
NMAX = SUBSTEPS * (NOBS - 1)


def wrap180(a):
    return (a + 180.0) % 360.0 - 180.0


def step_rates(rate, nrows, dts_len):
    """The per-step rate array the smoother indexes (unscented.py:287-292), as backward_track expands it."""
    return np.repeat(rate, int(nrows / dts_len))


def step_quantities(means, covs, Q, dt, sr, cr):
    """x_b (4, 1), P_b, D, K and the conditional covariance C = P_k - K P_b K^T of steps 0 .. nrows - 2 of one track, formed
    as oracle.ukf_oracle.backward_track forms them (unscented.py:297-333)."""
    nrows, n = means.shape
    W = orc.weight_matrix(n)
    out = []
    for k in range(nrows - 1):
        xk = means[k].reshape(n, 1)
        sig0 = orc._sigma_points_track(xk, covs[k], n, W[0, 0])
        sig = orc._propagate_track(sig0, dt[k], sr[k], cr[k])
        xb = np.sum(np.dot(sig, W), axis=1, keepdims=True)
        xb += np.zeros((n, 1))
        S = sig - xk
        Pb = np.dot(np.dot(S, W), S.T) + Q
        S = sig - xb
        S0 = sig0 - xk
        D = np.dot(np.dot(S0, W), S.T)
        K = np.dot(D, np.linalg.pinv(Pb))
        C = covs[k] - np.dot(np.dot(K, Pb), K.T)
        out.append(dict(xb=xb, Pb=Pb, D=D, K=K, C=C))
    return out


def sample_track(means, covs, steps, xi):
    """The recursion for one track: ``xi`` (S, nrows, 4) standard normal draws -> samples (S, nrows, 4)."""
    S, nrows, n = xi.shape
    out = np.empty((S, nrows, n))
    T = orc.sym_sqrt(covs[nrows - 1])
    x = means[nrows - 1].reshape(n, 1) + np.dot(T, xi[:, nrows - 1].T)  # (4, S)
    x[3] = orc.floored_mod(x[3], 360.0)
    out[:, nrows - 1] = x.T
    for k in range(nrows - 2, -1, -1):
        q = steps[k]
        y = x - q["xb"]
        y[3] = (y[3] + 180.0) % 360.0 - 180.0
        mean = means[k].reshape(n, 1) + np.dot(q["K"], y)
        x = mean + np.dot(orc.sym_sqrt(q["C"]), xi[:, k].T)
        x[3] = orc.floored_mod(x[3], 360.0)
        out[:, k] = x.T
    return out


def propagated_cov(covs, steps):
    """Cov(x_k) = C_k + K Cov(x_{k+1}) K^T from Cov(x_ns) = P_ns: the ensemble covariance of the samples, row by row."""
    nrows = covs.shape[0]
    out = np.empty_like(covs)
    out[nrows - 1] = covs[nrows - 1]
    for k in range(nrows - 2, -1, -1):
        q = steps[k]
        out[k] = q["C"] + np.dot(np.dot(q["K"], out[k + 1]), q["K"].T)
    return out


@dataclasses.dataclass
class TrackCase:
    """One of the eight tracks through the pinned oracle: filtered and smoothed histories, per-step quantities."""

    means: np.ndarray
    covs: np.ndarray
    sm_means: np.ndarray
    sm_covs: np.ndarray
    dt: np.ndarray
    sr: np.ndarray
    cr: np.ndarray
    steps: list


_CACHE = {}


def synthetic_batch():
    from track_estimators import synthetic

    if "sb" not in _CACHE:
        _CACHE["sb"] = synthetic.make_batch(8, nobs=NOBS, seed0=SEED0)
    return _CACHE["sb"]


def oracle_cases(Qs=None):
    """The eight tracks (synthetic.make_batch(8, nobs=7, seed0=100), 2 substeps, the example matrices) through
    oracle.ukf_oracle.forward_track / backward_track, computed once.  ``Qs``: a (8, 4, 4) stack of per-track Q instead."""
    from track_estimators import synthetic

    key = "cases" if Qs is None else ("cases", np.asarray(Qs).tobytes())
    if key in _CACHE:
        return _CACHE[key]
    sb = synthetic_batch()
    H, Q, R, P0 = synthetic.example_matrices()
    cases = []
    for b in range(8):
        Qb = Q if Qs is None else np.asarray(Qs)[b]
        dt = np.repeat(sb.dts[b] / SUBSTEPS, SUBSTEPS)
        means, covs = orc.forward_track(sb.z[b][:, 0], P0, H, Qb, R, dt, sb.dts[b], sb.z[b], sb.sog_rate[b], sb.cog_rate[b])
        sm, sP = orc.backward_track(means, covs, Qb, dt, NOBS - 1, sb.sog_rate[b], sb.cog_rate[b])
        sr = step_rates(sb.sog_rate[b], NMAX + 1, NOBS - 1)
        cr = step_rates(sb.cog_rate[b], NMAX + 1, NOBS - 1)
        cases.append(TrackCase(means, covs, sm, sP, dt, sr, cr, step_quantities(means, covs, Qb, dt, sr, cr)))
    _CACHE[key] = cases
    return cases


def truncated(case: TrackCase, ns: int):
    """The same track cut after ``ns`` steps (a ragged batch's nsteps): the filter is causal, so the filtered rows are the
    full track's; the smoother starts from row ns.  Returns (means, covs, steps, smoothed means, smoothed covariances)."""
    means, covs, steps = case.means[: ns + 1], case.covs[: ns + 1], case.steps[:ns]
    sm = sample_track(means, covs, steps, np.zeros((1, ns + 1, 4)))[0]
    return means, covs, steps, sm, propagated_cov(covs, steps)


def host_batch(track_index, nsteps=None, Qs=None, lanes=None):
    """The HostBatch of tracks ``track_index`` (indices into the eight, repeats allowed) with ``nsteps`` per slot."""
    from track_estimators import batch, synthetic

    sb = synthetic_batch()
    idx = np.asarray(track_index)
    sel = dataclasses.replace(sb, **{f.name: getattr(sb, f.name)[idx] for f in dataclasses.fields(sb)})
    H, Q, R, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(sel, SUBSTEPS, H, Q if Qs is None else np.asarray(Qs), R, P0)
    assert hb.Nmax == NMAX
    if nsteps is not None:
        hb = dataclasses.replace(hb, nsteps=np.asarray(nsteps, dtype=np.int32))
    if lanes is not None:
        hb = dataclasses.replace(hb, lanes=lanes)
    return hb


# B = 70: one full wave plus six lanes, the eight tracks repeated, every length from 0 (the shortest the packers accept) to Nmax
B70_TRACKS = np.arange(70) % 8
B70_NSTEPS = (NMAX - (np.arange(70) * 5) % (NMAX + 1)).astype(np.int32)


def sample_statistics(samples, sm_mean, sm_cov):
    """Worst ratios of the two 5-sigma checks over rows and components for one track: samples (S, nrows, 4).
    |mean_S - sm_mean| / (5 sqrt(sm_var / S)) and |var_S / sm_var - 1| / (5 sqrt(2 / (S - 1))), heading through wrap180."""
    S = samples.shape[0]
    d = samples - sm_mean[None]
    d[..., 3] = wrap180(d[..., 3])
    var = np.einsum("kcc->kc", sm_cov)
    mean_ratio = np.abs(d.mean(axis=0)) / (5.0 * np.sqrt(var / S))
    var_ratio = np.abs(d.var(axis=0, ddof=1) / var - 1.0) / (5.0 * np.sqrt(2.0 / (S - 1)))
    return float(mean_ratio.max()), float(var_ratio.max())
