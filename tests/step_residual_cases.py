"""Row-by-row residuals of the filter and smoother step loops against a 50-digit step: the pairs, the references, the host
baseline, the metrics and the exclusions that tests/test_step_residuals.py (GPU) and tests/test_mp_reference.py (CPU) share.

A history is never compared with another history.  A pair (track b, step k) takes the rows a pass itself wrote as the
INPUT of one step and asks what that step must give:

  forward    filtered row k          -> filtered row k + 1   (predict, then the update where one fires; on k = 0 of a batch with
                                                               an initial update, that update first: row 0 is the prior)
  smoother   filtered row k,
             smoothed row k + 1      -> smoothed row k

in 50 digits (oracle/mp_reference.py) and, for the bar, in float64 with the reference's own calls (oracle/ukf_oracle.py:
predict_track, update_track, one turn of backward_track's loop).  Nothing accumulates, so the differences are those of ONE
step: E_dev (the pass under test against the 50-digit step) is held to 4 E_host + 8 * 2^-52, E_host being the float64
oracle's step against the same 50-digit step on the same inputs.

Everything a step reads comes out of the HostBatch, in slot order: dt, the rates the forward pass gathered per step, the
smoother's own rates where the batch has them, the update index and its observation, recorded noise, per-track Q / R.
"""
import functools
import types

import numpy as np

from oracle import mp_reference as mpr
from oracle import ukf_oracle as orc

EPS = 2.0**-52
MAX_PAIRS = 200
RESTART = 64  # the step loops restart their warm eigenvector basis every 64 steps
ROW_CLASSES = {"first": (0, 1, 2), "restart": (RESTART - 2, RESTART - 1, RESTART)}  # and "last": a track's last step
MIDDLE_SLOTS = (20, 31, 42, 53)
PINV_RCOND = 1e-15  # np.linalg.pinv's cutoff relative to the largest singular value
COND_PB_MAX = 1e8  # beyond this tests/golden/ukf_illcond.npz holds the smoother at bounds of its own


# ----------------------------------------------------------------------------------------------------------------------
# pairs
# ----------------------------------------------------------------------------------------------------------------------
def chosen_tracks(ntracks):
    """Slots 0-7 (the short tracks of step_loop_cases.ragged_lengths), 62, 63 (the end of the first wave), 64 (the one-lane
    second wave) and four from the middle."""
    return [b for b in sorted(set(range(8)) | {62, 63, 64} | set(MIDDLE_SLOTS)) if b < ntracks]


def chosen_steps(n):
    """Steps of a track of n steps: 0, 1, 2 and 62, 63, 64 where they exist, the last, and every 7th between."""
    ks = set(ROW_CLASSES["first"]) | set(ROW_CLASSES["restart"]) | {n - 1} | set(range(7, n, 7))
    return sorted(k for k in ks if 0 <= k < n)


def pairs(nsteps):
    """The deterministic list of (track, step) pairs of a batch with these track lengths."""
    out = [(b, k) for b in chosen_tracks(len(nsteps)) for k in chosen_steps(int(nsteps[b]))]
    assert 0 < len(out) <= MAX_PAIRS, len(out)
    return out


def row_classes(pair, nsteps):
    b, k = pair
    return [name for name, rows in ROW_CLASSES.items() if k in rows] + (["last"] if k == int(nsteps[b]) - 1 else [])


# ----------------------------------------------------------------------------------------------------------------------
# what one step reads
# ----------------------------------------------------------------------------------------------------------------------
_TRI = np.triu_indices(4)  # HostBatch.Q_tracks / R_tracks: (10, B) upper triangles, row-major


def _track_matrix(shared, tri, b):
    if tri is None:
        return np.array(shared, dtype=np.float64)
    M = np.zeros((4, 4))
    M[_TRI] = tri[:, b]
    return M + np.triu(M, 1).T


def step_inputs(hb, pair):
    """Everything step k of track b reads, from the HostBatch."""
    b, k = pair
    s = types.SimpleNamespace(b=b, k=k, H=hb.H, Q=_track_matrix(hb.Q, hb.Q_tracks, b), R=_track_matrix(hb.R, hb.R_tracks, b),
                              dt=float(hb.dt[k, b]))
    s.sog_rate, s.cog_rate = float(hb.sog_rate[k, b]), float(hb.cog_rate[k, b])
    s.sog_rate_rts = s.sog_rate if hb.sog_rate_rts is None else float(hb.sog_rate_rts[k, b])
    s.cog_rate_rts = s.cog_rate if hb.cog_rate_rts is None else float(hb.cog_rate_rts[k, b])
    ui = int(hb.upd_idx[k, b])
    s.z = hb.z[ui, :, b].copy() if ui >= 0 else None  # the observation the update after this step consumes, or None
    s.z0 = hb.z[0, :, b].copy() if (k == 0 and hb.initial_update) else None  # the initial update sits between row 0 and step 0
    s.noise_pred = None if hb.noise_pred is None else hb.noise_pred[k, :, b].copy()
    s.noise_upd = None if hb.noise_upd is None else hb.noise_upd[k + 1, :, b].copy()
    s.noise_upd0 = None if hb.noise_upd is None else hb.noise_upd[0, :, b].copy()
    s.noise_rts = None if hb.noise_rts is None else hb.noise_rts[k, :, b].copy()
    return s


def _f(v):
    return np.array([float(e) for e in v])


# ----------------------------------------------------------------------------------------------------------------------
# references (50 digits) and host baselines (float64, the reference's own calls)
# ----------------------------------------------------------------------------------------------------------------------
def forward_reference(hb, rows_k, pair):
    """Filtered row k + 1 of a pair in 50 digits from ``rows_k`` = (x_k, P_k), rounded to doubles, and the eigenvalues the
    exclusions look at.  Returns (x (4,), P (4, 4), info)."""
    s, info = step_inputs(hb, pair), {}
    x, P = rows_k
    eig_S = []
    if s.z0 is not None:
        eig_Pk = mpr.eigsy(P)[0]
        x, P = mpr.ukf_update(x, P, s.H, s.R, s.z0, s.noise_upd0, info)
        eig_S.append(info["eig_S"])
    x, P = mpr.ukf_predict(x, P, s.Q, s.dt, s.sog_rate, s.cog_rate, s.noise_pred, info)
    info["eig_Pk"] = eig_Pk if s.z0 is not None else info["eig_P"]  # eig_P: of the scaled P the fan was taken from
    info.pop("heading_unwrapped", None)  # of the initial update: the row's own heading comes out of the predict, unreduced
    if s.z is not None:
        x, P = mpr.ukf_update(x, P, s.H, s.R, s.z, s.noise_upd, info)
        eig_S.append(info["eig_S"])
    info["eig_S"] = eig_S
    return _f(x), mpr.to_np(P), info


def forward_host(hb, rows_k, pair):
    """The same step with ukf_oracle.update_track / predict_track (scipy.linalg.sqrtm, np.linalg.pinv)."""
    s = step_inputs(hb, pair)
    x, P = np.array(rows_k[0], dtype=np.float64).reshape(4, 1), np.array(rows_k[1], dtype=np.float64)
    W = orc.weight_matrix(4)
    if s.z0 is not None:
        x, P = orc.update_track(x, P, s.H, s.R, s.z0, s.noise_upd0)
    x, P = orc.predict_track(x, P, s.Q, W, s.dt, s.sog_rate, s.cog_rate, s.noise_pred)
    if s.z is not None:
        x, P = orc.update_track(x, P, s.H, s.R, s.z, s.noise_upd)
    return x[:, 0], P


_GAINS = {}


def _gain(s, xk, Pk):
    """urts_gain needs the filtered row alone, and every smoother form of a case reads the same filtered rows: keep it."""
    key = (s.b, s.k, xk.tobytes(), Pk.tobytes(), s.Q.tobytes(), s.dt, s.sog_rate_rts, s.cog_rate_rts,
           None if s.noise_rts is None else s.noise_rts.tobytes())
    if key not in _GAINS:
        if len(_GAINS) > 4 * MAX_PAIRS:
            _GAINS.clear()
        info = {}
        _GAINS[key] = mpr.urts_gain(xk, Pk, s.Q, s.dt, s.sog_rate_rts, s.cog_rate_rts, s.noise_rts, info) + (info,)
    return _GAINS[key]


def smoother_reference(hb, filt, smoothed_next, pair):
    """Smoothed row k of a pair in 50 digits from ``filt`` = (x_k, P_k) and ``smoothed_next`` = (x_s, P_s) of row k + 1.
    Returns (x (4,), P (4, 4), info)."""
    s = step_inputs(hb, pair)
    xk, Pk = np.ascontiguousarray(filt[0], dtype=np.float64), np.ascontiguousarray(filt[1], dtype=np.float64)
    xb, Pb, K, info = _gain(s, xk, Pk)
    info = dict(info, eig_Pk=info["eig_P"], eig_S=[])
    x, P = mpr.urts_combine(xk, Pk, smoothed_next[0], smoothed_next[1], xb, Pb, K, info)
    return _f(x), mpr.to_np(P), info


def smoother_host(hb, filt, smoothed_next, pair):
    """One turn of ukf_oracle.backward_track's loop: a history of two rows."""
    s = step_inputs(hb, pair)
    means = np.array([filt[0], smoothed_next[0]], dtype=np.float64)
    covs = np.array([filt[1], smoothed_next[1]], dtype=np.float64)
    x, P = orc.backward_track(means, covs, s.Q, [s.dt], 1, [s.sog_rate_rts], [s.cog_rate_rts],
                              None if s.noise_rts is None else [s.noise_rts])
    return x[0], P[0]


# ----------------------------------------------------------------------------------------------------------------------
# exclusions
# ----------------------------------------------------------------------------------------------------------------------
def _near_cutoff(w):
    """Is an eigenvalue within a factor 10 of pinv's cutoff, rcond * the largest?  (Exact zeros -- the rows H leaves out --
    are far below it.)"""
    big = max(abs(v) for v in w)
    cut = mpr.mpf(PINV_RCOND) * big
    return any(cut / 10 < abs(v) < cut * 10 for v in w)


def excluded(pair, status, info):
    """The reason a pair is left out, or None.  Only these: the track is flagged; P_k is not positive definite in 50 digits
    (the square root's clamp is held by tests/test_math_probe.py); the rank decision of a pseudo-inverse is a coin toss in
    any arithmetic; P_b is conditioned beyond 1e8."""
    if int(status[pair[0]]) != 0:
        return "status 0x%x" % int(status[pair[0]])
    if min(info["eig_Pk"]) <= 0:
        return "P_k has an eigenvalue <= 0"
    for w in info["eig_S"] + ([info["eig_Pb"]] if "eig_Pb" in info else []):
        if _near_cutoff(w):
            return "an eigenvalue at the pseudo-inverse's cutoff"
    if "eig_Pb" in info:
        w = [abs(v) for v in info["eig_Pb"]]
        if min(w) == 0 or max(w) / min(w) > COND_PB_MAX:
            return "cond(P_b) > 1e8"
    return None


def check_caps(kind, all_pairs, left_out, nsteps):
    """``kind`` 'synthetic': no pair may be excluded.  'regime': at most 5 % of the pairs, and no row class (steps 0-2,
    62-64, a track's last) may lose all its pairs.  ``left_out``: dict pair -> reason."""
    if kind == "synthetic":
        assert not left_out, f"pairs excluded from a synthetic case: {left_out}"
        return
    assert len(left_out) <= 0.05 * len(all_pairs), f"{len(left_out)} of {len(all_pairs)} pairs excluded: {left_out}"
    for cls in list(ROW_CLASSES) + ["last"]:
        members = [p for p in all_pairs if cls in row_classes(p, nsteps)]
        assert not members or any(p not in left_out for p in members), f"every pair of row class {cls!r} is excluded"


# ----------------------------------------------------------------------------------------------------------------------
# metrics and the comparison
# ----------------------------------------------------------------------------------------------------------------------
def mean_errs(got, want, heading_unwrapped=None):
    """Element-wise |got - want| / max(|want|, 1e-3) (tests/test_regimes.py: _errs), the heading's difference wrapped to
    +-180 so that 359.999... against 0.000... is not an error of 360.

    ``heading_unwrapped``: the 50-digit heading u of this row before the step reduced it mod 360 (an update's or a smoother
    step's last operation; None where the step ends in a predict, which reduces nothing).  The step computes u = x[3] +
    (K y)[3], a sum of terms of the size of u, and then takes away a multiple of 360, which is exact in doubles: whatever
    absolute error d the arithmetic left in u is the error of the heading h = u mod 360.  Relative to h it is
    (d / |u|) * |u| / |h|: the reduction amplifies the relative error of what was computed by A = |u| / max(|h|, 1e-3), for
    any float64 evaluation, the reference's own included (each sigma point's heading goes through degrees -> radians ->
    degrees there, non_linear_process.py:52,83, and comes back an ulp of 360 off; the weighted mean adds them with weights
    of both signs).  A heading of 0.155 reduced from 360.155 has A = 2 300: 1 ulp of u is 3.7e-13 of h.  So where u is
    given, the heading's error is measured against max(|u|, |h|, 1e-3): in units of the number the arithmetic produced.
    This applies to E_dev and E_host alike, and only moves the heading of rows whose reduction took something away."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = got - want
    if d[3] > 180.0:  # got - 360 and want - 360 are exact for headings in [180, 360]: the small difference is not rounded away
        d[3] = (got[3] - 360.0) - want[3]
    elif d[3] < -180.0:
        d[3] = got[3] - (want[3] - 360.0)
    scale = np.maximum(np.abs(want), 1e-3)
    if heading_unwrapped is not None:
        scale[3] = max(scale[3], abs(float(heading_unwrapped)))
    return np.abs(d) / scale


def cov_errs(got, want):
    """|got - want| per entry against max |want| of the matrix"""
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.max(np.abs(want))


def bound(e_host):
    return 4 * e_host + 8 * EPS


def measure(kept, got, ref, host):
    """``got``, ``host``: dict pair -> (x, P); ``ref``: dict pair -> (x, P, heading before its reduction or None).  Returns
    E_dev and E_host for means and covariances with the pair and element of the largest E_dev.  A non-finite value anywhere
    counts as infinitely wrong."""
    r = types.SimpleNamespace(npairs=len(kept))
    def errs(name, rows, want):
        e = mean_errs(rows[0], want[0], want[2]) if name == "mean" else cov_errs(rows[1], want[1])
        return np.nan_to_num(e, nan=np.inf)

    for name in ("mean", "cov"):
        e_dev, e_host, worst = 0.0, 0.0, None
        for p in kept:
            ed, eh = errs(name, got[p], ref[p]), errs(name, host[p], ref[p])
            if worst is None or ed.max() > e_dev:
                e_dev = float(ed.max())
                worst = (p, tuple(int(v) for v in np.unravel_index(int(ed.argmax()), ed.shape)))
            e_host = max(e_host, float(eh.max()))
        setattr(r, name, types.SimpleNamespace(e_dev=e_dev, e_host=e_host, bound=bound(e_host), worst=worst))
    return r


def report(label, what, r):
    print(f"\n[step residual] {label} {what}: {r.npairs} pairs | mean E_dev = {r.mean.e_dev:.3e}, E_host = {r.mean.e_host:.3e} | "
          f"cov E_dev = {r.cov.e_dev:.3e}, E_host = {r.cov.e_host:.3e}")


def check(label, what, r):
    """E_dev <= 4 E_host + 8 * 2^-52 for the means and for the covariances; a failure names the pair and the entry."""
    for name in ("mean", "cov"):
        m = getattr(r, name)
        (b, k), at = m.worst
        assert m.e_dev <= m.bound, (f"{label} {what} {name}: E_dev = {m.e_dev:.3e} > 4 x {m.e_host:.3e} + 8 eps = {m.bound:.3e} "
                                    f"at track {b}, step {k}, entry {at}")


def residuals(hb, hist, status, which):
    """Every pair of ``hb`` through reference and host baseline, from the rows of ``hist`` (means, covs, means_smoothed,
    covs_smoothed: (B, N + 1, ...)).  ``which``: 'forward' or 'smoother'.  Returns (measure(...), pairs, dict pair -> reason
    it was left out, (got, ref, host, pairs kept) as ``measure`` takes them)."""
    all_pairs = pairs(hb.nsteps)
    got, ref, host, left_out = {}, {}, {}, {}
    m, P = hist["means"], hist["covs"]
    for p in all_pairs:
        b, k = p
        if int(status[b]) != 0:  # the rows of a flagged track need not be finite: nothing to decompose
            left_out[p] = excluded(p, status, None)
            continue
        if which == "forward":
            x, C, info = forward_reference(hb, (m[b, k], P[b, k]), p)
            host[p] = forward_host(hb, (m[b, k], P[b, k]), p)
            got[p] = (m[b, k + 1], P[b, k + 1])
        else:
            nxt = (hist["means_smoothed"][b, k + 1], hist["covs_smoothed"][b, k + 1])
            x, C, info = smoother_reference(hb, (m[b, k], P[b, k]), nxt, p)
            host[p] = smoother_host(hb, (m[b, k], P[b, k]), nxt, p)
            got[p] = (hist["means_smoothed"][b, k], hist["covs_smoothed"][b, k])
        ref[p] = (x, C, info.get("heading_unwrapped"))
        why = excluded(p, status, info)
        if why is not None:
            left_out[p] = why
    kept = [p for p in all_pairs if p not in left_out]
    return measure(kept, got, ref, host), all_pairs, left_out, (got, ref, host, kept)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
STEP_LOOP_CASES = ("quarter", "every", "none_noinit", "noise", "shift", "track_noise")
REGIME_CASES = ("arctic", "fast_long_steps", "heading_seam", "unwrapped_heading")
CASES = STEP_LOOP_CASES + ("general",) + REGIME_CASES


def case_kind(name):
    return "regime" if name in REGIME_CASES else "synthetic"


def general_matrices():
    """A dense H and R, so that the update takes the 4 x 4 route: H within 0.1 of the identity, R positive definite."""
    rng = np.random.default_rng(6161)
    H = np.eye(4) + 0.1 * rng.uniform(-1, 1, (4, 4))
    A = 0.1 * rng.normal(size=(4, 4))
    R = A @ A.T + np.diag([0.25, 0.25, 0.5, 2.0])
    return H, 0.5 * (R + R.T)


@functools.lru_cache(None)
def build_case(name):
    """HostBatch of a case (lanes left to the caller: dataclasses.replace(hb, lanes=...))."""
    import dataclasses

    import step_loop_cases as slc
    from track_estimators import batch, synthetic

    if name in STEP_LOOP_CASES:
        return slc.build_case(name)
    if name == "general":
        hb = slc.build_case("quarter")
        H, R = general_matrices()
        z = np.ascontiguousarray(np.einsum("ij,tjb->tib", H, hb.z))  # observations of H x, not of x
        return dataclasses.replace(hb, H=np.ascontiguousarray(H), R=np.ascontiguousarray(R), z=z)
    from test_regimes import REGIMES, _regime_batch

    H, Q, R, P0 = synthetic.example_matrices()
    sb = _regime_batch(65, 9, seed=sum(map(ord, name)), **REGIMES[name])
    return batch.pack_uniform(sb, 2, H, Q, R, P0)


def oracle_history(hb):
    """The float64 oracle's filtered and smoothed histories of a HostBatch (ukf_oracle.predict_batch / update_batch /
    backward_batch), with a status word that flags the tracks it left non-finite.  For the checks that need no GPU."""
    B, N = hb.B, hb.Nmax
    from track_estimators import batch

    Qs, Rs = (np.array(M) for M in batch.track_matrices(hb))
    x = np.array(hb.x0.T, dtype=np.float64)
    P = (np.broadcast_to(hb.P0.reshape(4, 4), (B, 4, 4)) if hb.shared_p0 else hb.P0.T.reshape(B, 4, 4)).copy()
    means, covs = np.empty((B, N + 1, 4)), np.empty((B, N + 1, 4, 4))
    means[:, 0], covs[:, 0] = x, P
    ar = np.arange(B)
    nz = lambda a, k: None if a is None else a[k].T  # noqa: E731
    with np.errstate(all="ignore"):
        if hb.initial_update:
            x, P = orc.update_batch(x, P, hb.H, Rs, hb.z[0].T.copy(), nz(hb.noise_upd, 0))
        for k in range(N):
            xp, Pp = orc.predict_batch(x, P, Qs, hb.dt[k], hb.sog_rate[k], hb.cog_rate[k], nz(hb.noise_pred, k))
            f = hb.upd_idx[k] >= 0
            if f.any():
                zi = np.where(f, hb.upd_idx[k], 0)
                xu, Pu = orc.update_batch(xp, Pp, hb.H, Rs, hb.z[zi, :, ar].copy(), nz(hb.noise_upd, k + 1))
                xp, Pp = np.where(f[:, None], xu, xp), np.where(f[:, None, None], Pu, Pp)
            live = k < hb.nsteps
            x, P = np.where(live[:, None], xp, x), np.where(live[:, None, None], Pp, P)
            means[:, k + 1], covs[:, k + 1] = x, P
        sr = hb.sog_rate if hb.sog_rate_rts is None else hb.sog_rate_rts
        cr = hb.cog_rate if hb.cog_rate_rts is None else hb.cog_rate_rts
        idx = np.broadcast_to(np.arange(N), (B, N))
        sm, sP = orc.backward_batch(means, covs, Qs, hb.dt.T, idx, sr.T, cr.T, nsteps=hb.nsteps,
                                    noise_rts=None if hb.noise_rts is None else hb.noise_rts.transpose(2, 0, 1))
    fin = np.isfinite(means).all(axis=(1, 2)) & np.isfinite(covs).all(axis=(1, 2, 3)) & np.isfinite(sm).all(axis=(1, 2)) & \
        np.isfinite(sP).all(axis=(1, 2, 3))
    return dict(means=means, covs=covs, means_smoothed=sm, covs_smoothed=sP), (~fin).astype(np.int32)
