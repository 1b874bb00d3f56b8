"""The batch of 130 different (x, P, z, ...) elements that tests/test_single_step_batches.py pushes through the one-step
entry points, its 50-digit references, and the float64 oracle's error against them (the bar the device is held to).
Built once per process; tests/test_mp_reference.py checks the oracle side on the CPU.

The smaller counts (1, 63, 64, 65) are the first elements of the same batch, so one set of references serves all.
"""
import functools
import types

import numpy as np

from oracle import mp_reference as mpr
from oracle import ukf_oracle as orc

COUNT = 130
COUNTS = (1, 63, 64, 65, 130)
EPS = 2.0**-52


def _spd(r, n, cond_max=1e4):
    q, rr = np.linalg.qr(r.normal(size=(n, n)))
    w = 10.0 ** -r.uniform(0, np.log10(cond_max), n)
    w[0] = 1.0
    a = (q * w) @ q.T
    return 0.5 * (a + a.T)


@functools.lru_cache(None)
def batch():
    r = np.random.default_rng(4242)
    n = COUNT
    b = types.SimpleNamespace(count=n)
    b.x = np.stack([r.uniform(-170, 170, n), r.choice([-1.0, 1.0], n) * r.uniform(1, 60, n), r.uniform(5, 40, n), r.uniform(40, 320, n)], axis=1)
    b.P = np.array([_spd(r, 4) * 10.0 ** r.uniform(-4, -1) for _ in range(n)])  # cond <= 1e4, fan of up to ~0.5 degrees
    b.dt = r.uniform(0.05, 1.0, n)
    b.sr = r.uniform(-1, 1, n)
    b.cr = r.uniform(-5, 5, n)
    b.noise = r.uniform(-1e-3, 1e-3, (n, 4))
    b.Q = np.diag([1e-4, 1e-4, 1e-6, 1e-6]) + 1e-7 * np.array([[0, 1, 2, 3], [1, 0, 4, 5], [2, 4, 0, 6], [3, 5, 6, 0.0]])
    b.w0, b.wi = orc.sigma_weights(4)
    b.fan_scale = 4 / (1 - b.w0)
    b.H = {"block": np.diag([1.0, 1.0, 0.0, 0.0]), "dense": np.eye(4) + 0.1 * r.uniform(-1, 1, (4, 4))}
    Rb = np.zeros((4, 4))
    Rb[:2, :2] = [[0.25, 0.05], [0.05, 0.3]]
    b.R = {"block": Rb, "dense": _spd(r, 4, 1e2) * 0.3}
    inn = r.uniform(-0.05, 0.05, (n, 4))
    b.z = {k: b.x @ b.H[k].T + inn for k in ("block", "dense")}  # observations a small innovation away from H x
    # general dimension: n-vectors and n x n covariances for the generic sigma fan
    b.gen = {m: (r.uniform(-10, 10, (n, m)), np.array([_spd(r, m) * 10.0 ** r.uniform(-3, 0) for _ in range(n)])) for m in (1, 2, 4, 7, 16)}
    b.gen_scale = 3.0
    b.gen_exact_rows = {1: range(n), 2: range(n), 4: range(n), 7: (0, 1, 62, 63, 64, 65, 128, 129), 16: (0, 63, 64, 129)}
    for v in vars(b).values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            for arr in (a if isinstance(a, tuple) else [a]):
                if isinstance(arr, np.ndarray):
                    arr.setflags(write=False)
    return b


def mean_err(a, ref):
    """element-wise |d| / max(|ref|, 1e-12), the project's metric for state means (tests/test_hip_parity.py)"""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a) - ref) / np.maximum(np.abs(ref), 1e-12)))


def cov_err(a, ref):
    """max |dP| / max |P| per matrix, the project's metric for covariances"""
    ref = np.asarray(ref, dtype=np.float64)
    ax = tuple(range(1, ref.ndim))
    return float(np.max(np.max(np.abs(np.asarray(a) - ref), axis=ax) / np.max(np.abs(ref), axis=ax)))


def _f(v):
    return np.array([float(e) for e in v])


@functools.lru_cache(None)
def predict_reference(with_noise):
    b = batch()
    xs, Ps = [], []
    for i in range(b.count):
        x, P = mpr.ukf_predict(b.x[i], b.P[i], b.Q, b.dt[i], b.sr[i], b.cr[i], b.noise[i] if with_noise else None)
        xs.append(_f(x)), Ps.append(mpr.to_np(P))
    return np.array(xs), np.array(Ps)


@functools.lru_cache(None)
def update_reference(route):
    """(x, P, gamma, denom) of the update with z + noise (exact sum) and of the robust terms with z, per element."""
    b = batch()
    xs, Ps, ga, de = [], [], [], []
    for i in range(b.count):
        x, P = mpr.ukf_update(b.x[i], b.P[i], b.H[route], b.R[route], b.z[route][i], b.noise[i])
        g, d = mpr.robust_terms(b.x[i], b.P[i], b.H[route], b.R[route], b.z[route][i])
        xs.append(_f(x)), Ps.append(mpr.to_np(P)), ga.append(float(g)), de.append(float(d))
    return np.array(xs), np.array(Ps), np.array(ga), np.array(de)


@functools.lru_cache(None)
def geodetic_reference():
    b = batch()
    return np.array([_f(mpr.geodetic_step(b.x[i], b.dt[i], b.sr[i], b.cr[i])) for i in range(b.count)])


@functools.lru_cache(None)
def sigma_reference(m):
    """dict row -> (2m+1, m) exact sigma points of the general-dimension batch (every row for m <= 4, the rows around the
    wave boundaries for m = 7 and 16, where a 50-digit eigen-decomposition costs 20 to 150 ms)."""
    b = batch()
    x, P = b.gen[m]
    return {i: np.array([_f(p) for p in mpr.sigma_points(x[i], P[i], b.gen_scale)]) for i in b.gen_exact_rows[m]}


@functools.lru_cache(None)
def sigma4_reference():
    """(count, 9, 4) exact fans of (x, P) with the filter's own scale, for ste_sigma_points_f64"""
    b = batch()
    return np.array([[_f(p) for p in mpr.sigma_points(b.x[i], b.P[i], b.fan_scale)] for i in range(b.count)])


def oracle_sigma(x, P, scale):
    """The float64 oracle's fan, (2n+1, n): scipy.linalg.sqrtm as the reference calls it (unscented.py:95-105)."""
    n = len(x)
    return orc._sigma_points_track(np.asarray(x, dtype=np.float64).reshape(n, 1), P, n, 1 - n / scale).T


@functools.lru_cache(None)
def oracle_errors(route):
    """The float64 oracle (oracle/ukf_oracle.py: scipy.linalg.sqrtm, np.linalg.pinv) against the 50-digit restatement on
    the batch: the bar of tests/test_single_step_batches.py."""
    b = batch()
    W = orc.weight_matrix(4)
    e = {}
    for wn in (False, True):
        rx, rP = predict_reference(wn)
        got = [orc.predict_track(b.x[i].reshape(4, 1), b.P[i], b.Q, W, b.dt[i], b.sr[i], b.cr[i], b.noise[i] if wn else None)
               for i in range(b.count)]
        key = "predict+noise" if wn else "predict"
        e[key + " mean"] = mean_err(np.array([g[0][:, 0] for g in got]), rx)
        e[key + " cov"] = cov_err(np.array([g[1] for g in got]), rP)
    rx, rP, rg, rd = update_reference(route)
    H, R, z = b.H[route], b.R[route], b.z[route]
    got = [orc.update_track(b.x[i].reshape(4, 1), b.P[i], H, R, z[i], b.noise[i]) for i in range(b.count)]
    e["update mean"] = mean_err(np.array([g[0][:, 0] for g in got]), rx)
    e["update cov"] = cov_err(np.array([g[1] for g in got]), rP)
    e["gamma"] = mean_err([orc.criterion_index(b.x[i], H, z[i], b.P[i], R) for i in range(b.count)], rg)
    den = []
    for i in range(b.count):  # the denominator of update_lambda_factor: lambda' = 0 + (1 - 0) / den
        den.append(1.0 / orc.update_lambda_factor(b.x[i], H, 0.0, 1.0, 0.0, z[i], b.P[i], R))
    e["denom"] = mean_err(den, rd)
    e["geodetic"] = mean_err(orc.geodetic_dynamics(b.x, b.dt, b.sr, b.cr), geodetic_reference())
    e["sigma fan"] = cov_err(np.array([oracle_sigma(b.x[i], b.P[i], b.fan_scale) for i in range(b.count)]), sigma4_reference())
    for m in (1, 2, 4, 7, 16):
        ref = sigma_reference(m)
        x, P = b.gen[m]
        e["sigma n=%d" % m] = max(cov_err(oracle_sigma(x[i], P[i], b.gen_scale)[None], ref[i][None]) for i in ref)
    return e


def bound(oracle_error):
    return 4 * oracle_error + 8 * EPS
