"""NumPy restatement of the smoother's lag-one cross-covariance and of the covariance of a position at a query time
(include/ste.h: ste_urtss_lag_one_f64, ste_track_position_cov_f64; DESIGN.md, "Lag-one covariance"), and what their tests share.

    L_k  = Cov(x_k, x_{k+1} | all data) = K_k P^s_{k+1}                      k = 0 .. ns - 1
    P(u) = (1 - u)^2 P^s_k + u^2 P^s_{k+1} + (1 - u) u (L_k + L_k^T)          the state interpolated linearly at fraction u
per entry, with w1 = u and w0 = 1 - u:  P_rc = ((w0 w0) A_rc + (w1 w1) B_rc) + (w0 w1) (L_rc + L_cr), evaluated as written.
K_k is the gain of ``track_sampling_cases.step_quantities`` (the oracle's own calls) and P^s the oracle's smoothed covariance.
The query definition has no operation whose bits may differ between implementations, so the device is held to it bit for bit.
"""
import numpy as np
import position_cases as pc
import track_sampling_cases as tsc

US = (0.25, 0.5, 0.875)  # the fractions of the statistical tests
STAT_S, STAT_SEED = 4096, 20241  # as tests/test_track_sampling.py: sample count and seed of the host draws
VAR_BOUND = 5.0 * np.sqrt(2.0 / (STAT_S - 1))
PACKED = [(r, c) for r in range(4) for c in range(r, 4)]  # 00 01 02 03 11 12 13 22 23 33
POSITION = [(0, 0), (0, 1), (1, 1)]  # pcov without STE_PCOV_FULL
_CACHE = {}


def lag_one(case_or_steps, sm_covs=None):
    """L_k = np.dot(K_k, P^s_{k+1}) for every step of a TrackCase (or of (steps, smoothed covariances)): (ns, 4, 4)."""
    steps, sP = (case_or_steps.steps, case_or_steps.sm_covs) if sm_covs is None else (case_or_steps, sm_covs)
    return np.array([np.dot(steps[k]["K"], sP[k + 1]) for k in range(len(steps))]).reshape(len(steps), 4, 4)


def draws_to_deviations(covs, steps):
    """The linear map A of the sampler's recursion (wraps aside) from all draws to all row deviations: with xi the stacked
    draws (4 (ns + 1),), A xi stacks x_k - E x_k.  dev_ns = T_ns xi_ns, dev_k = K_k dev_{k+1} + T_k xi_k."""
    from oracle import ukf_oracle as orc

    nrows = covs.shape[0]
    A = np.zeros((4 * nrows, 4 * nrows))
    A[4 * (nrows - 1):, 4 * (nrows - 1):] = orc.sym_sqrt(covs[nrows - 1])
    for k in range(nrows - 2, -1, -1):
        A[4 * k:4 * k + 4] = np.dot(steps[k]["K"], A[4 * k + 4:4 * k + 8])
        A[4 * k:4 * k + 4, 4 * k:4 * k + 4] = orc.sym_sqrt(steps[k]["C"])
    return A


def blend(u, A, B, L):
    """P(u) entry by entry as the header writes it; A, B, L (4, 4) (or any square block), u a float -> same shape."""
    u = np.float64(u)
    w1, w0 = u, np.float64(1.0) - u
    w00, w11, w01 = w0 * w0, w1 * w1, w0 * w1
    n = A.shape[0]
    out = np.empty((n, n))
    for r in range(n):
        for c in range(n):
            out[r, c] = (w00 * A[r, c] + w11 * B[r, c]) + w01 * (L[r, c] + L[c, r])
    return out


def blend_without_cross(u, A, B):
    """What interpolating sm_cov alone gives: the formula without its lag-one term."""
    return blend(u, A, B, np.zeros_like(A))


def position_cov(cov, lag1, nsteps, dt, qtrack, qtime, t0=None, full=False):
    """The restatement of ste_track_position_cov_f64: cov (N+1, 4, 4, B) (the upper triangle is read), lag1 (N, 4, 4, B) ->
    dict(pcov (3 or 10, Q), step, frac, status (Q,)); the locate step is position_cases.locate on position_cases.knot_times."""
    cov, lag1 = np.asarray(cov, dtype=np.float64), np.asarray(lag1, dtype=np.float64)
    B = cov.shape[-1]
    qtrack, qtime = np.asarray(qtrack), np.asarray(qtime, dtype=np.float64)
    Q = len(qtrack)
    T = pc.knot_times(nsteps, dt)
    entries = PACKED if full else POSITION
    out = dict(pcov=np.full((len(entries), Q), np.nan), step=np.full(Q, -1, dtype=np.int32), frac=np.full(Q, np.nan),
               status=np.zeros(Q, dtype=np.int32))
    with np.errstate(all="ignore"):
        for q in range(Q):
            t = int(qtrack[q])
            if t < 0 or t >= B:
                out["status"][q] = pc.BAD_INDEX
                continue
            t0v = np.float64(0.0) if t0 is None else np.float64(t0[t])
            status, row, u, interior = pc.locate(qtime[q], t0v, T[:, t], int(nsteps[t]))
            out["status"][q], out["step"][q], out["frac"][q] = status, row, u
            if row < 0:
                continue
            A = cov[row, :, :, t]
            if not interior:
                out["pcov"][:, q] = [A[r, c] for r, c in entries]
                continue
            Bn, L = cov[row + 1, :, :, t], lag1[row, :, :, t]
            w1, w0 = u, np.float64(1.0) - u
            w00, w11, w01 = w0 * w0, w1 * w1, w0 * w1
            out["pcov"][:, q] = [(w00 * A[r, c] + w11 * Bn[r, c]) + w01 * (L[r, c] + L[c, r]) for r, c in entries]
    return out


def packed_rows(cov):
    """(rows, 4, 4, B) symmetric -> (rows, 10, B), the layout of STE_FLAG_PACKED_COV."""
    return np.ascontiguousarray(np.stack([cov[:, r, c] for r, c in PACKED], axis=1))


def random_covariances(nrows, B, seed):
    """Seeded random inputs of the query kernel's tests: cov (nrows, 4, 4, B) symmetric, lag1 (nrows - 1, 4, 4, B) not."""
    rng = np.random.default_rng(seed)
    cov = rng.standard_normal((nrows, 4, 4, B))
    cov = cov + cov.transpose(0, 2, 1, 3)
    lag1 = rng.standard_normal((max(nrows - 1, 0), 4, 4, B))
    return cov, lag1


def stat_samples():
    """4096 restated samples of each of the eight tracks from the host draws of the statistics tests, as deviations from the
    smoothed mean (heading through wrap180): list of (S, Nmax+1, 4), computed once."""
    if "dev" not in _CACHE:
        xi = np.random.default_rng(STAT_SEED).standard_normal((STAT_S, tsc.NMAX + 1, 4, 8))
        out = []
        for b, case in enumerate(tsc.oracle_cases()):
            s = tsc.sample_track(case.means, case.covs, case.steps, np.ascontiguousarray(xi[..., b]))
            d = s - case.sm_means[None]
            d[..., 3] = tsc.wrap180(d[..., 3])
            d.setflags(write=False)
            out.append(d)
        _CACHE["dev"] = out
    return _CACHE["dev"]


def ensemble_check(var, cxy, var_s, cxy_s, S):
    """The two 5-sigma checks of an analytic 2 x 2 (var (2,), cxy) against an ensemble's (var_s, cxy_s): worst
    |var_S / var - 1| and |cov_S - cov| as a fraction of 5 sqrt((var_x var_y + cov^2) / (S - 1))."""
    ratio = float(np.max(np.abs(np.asarray(var_s) / np.asarray(var) - 1.0)))
    cbound = 5.0 * np.sqrt((var[0] * var[1] + cxy * cxy) / (S - 1))
    return ratio, float(abs(cxy_s - cxy) / cbound)
