"""
Batched UKF + URTSS over many independent ship tracks on one MI355X.

This is the host side of the hot path: it turns B ``ShipTrack``-like objects into the structure-of-arrays batch
that include/ste.h describes (track index fastest), precomputes the per-step update schedule with the same float
accumulation the reference driver performs (kalman_filter.py:73,98-102), launches the HIP kernels through the C ABI
and hands back per-track histories shaped like the reference's return values.

PyTorch is used only for device memory and streams.  There is no CPU fallback.

Reference call sites replaced (relative to /root/reference):
  examples/example_ukf_rts_smoother_batch.py:19-90   the per-ship Python loop -> one batched launch
  src/track_estimators/kalman_filters/kalman_filter.py:36-137   run / run_rts_smoother
"""
from __future__ import annotations

import atexit
import ctypes as C
import dataclasses
import weakref
from typing import Optional, Sequence

import numpy as np

from ._hip import binding


# ----------------------------------------------------------------------------------------------------------------
# host-side logic (pure NumPy, no arithmetic of the filter itself)
# ----------------------------------------------------------------------------------------------------------------
def sigma_constants(n: int, weights_computed: bool = True):
    """(fan_scale, w0, wi) as unscented.py:95,125,132 computes them in Python floats."""
    w0 = 1 - n / 3.0
    wi = (1 - w0) / (2 * n)
    fan_scale = n / (1 - (w0 if weights_computed else 0.0))
    return fan_scale, w0, wi


def _isin_exact(times: np.ndarray, cums: np.ndarray) -> np.ndarray:
    """``np.isin(times, cums)`` for 1-D float arrays (exact equality, NaN never a member) by sort + binary search; an
    order of magnitude cheaper per call than np.isin's concatenate/unique path, which matters once per track."""
    if len(cums) == 0 or len(times) == 0:
        return np.zeros(len(times), dtype=bool)
    cs = np.sort(cums)
    pos = np.searchsorted(cs, times)
    np.minimum(pos, len(cs) - 1, out=pos)
    return cs[pos] == times


def update_schedule(dt, dts, t0=0):
    """
    Float-equality update trigger of the reference driver (kalman_filter.py:73,98-102), precomputed.

    Returns ``upd_idx`` (int32[N]: observation column consumed after step k, -1 = none), ``rate_idx`` (int64[N]:
    index into sog_rate/cog_rate that predict uses at step k, kalman_filter.py:93-94) and the final time.
    The running time is accumulated by sequential float addition exactly like ``self.time += dt``.
    """
    dt = np.asarray(dt, dtype=np.float64)
    cums = np.cumsum(np.asarray(dts, dtype=np.float64))
    times = np.cumsum(np.concatenate([[np.float64(t0)], dt]))[1:]
    fires = _isin_exact(times, cums)
    after = np.cumsum(fires)
    upd_idx = np.where(fires, after, -1).astype(np.int32)
    rate_idx = after - fires
    return upd_idx, rate_idx, (times[-1] if len(times) else np.float64(t0))


def rts_rate_index(nrows: int, dts_len: int, T: int) -> np.ndarray:
    """Index into the length-T rate arrays read by the smoother at step k (unscented.py:287-292, 310-311)."""
    rep = int(nrows / dts_len)
    idx = np.repeat(np.arange(T), rep)
    if len(idx) < nrows - 1:
        raise IndexError(
            f"smoother rate expansion too short: np.repeat(rate[{T}], {rep}) has {len(idx)} entries for {nrows - 1} steps"
        )
    return idx[: nrows - 1]


def draw_reference_noise(Q, R, dt, dts, t0=0):
    """
    Noise arrays for one track drawn from NumPy's global generator with the reference's calls in the reference's order
    (unscented.py:198,232,320): initial update, then per step the predict draw (+ an update draw when the trigger
    fires), then the smoother's draws for k = N-1 ... 0.  Returns the dict ``pack_tracks(noise=[...])`` expects.
    """
    N = len(dt)
    upd_idx, _, _ = update_schedule(dt, dts, t0)
    sq, sr = np.sqrt(np.diag(Q)), np.sqrt(np.diag(R))
    npred, nupd, nrts = np.zeros((N, 4)), np.zeros((N + 1, 4)), np.zeros((N, 4))
    nupd[0] = np.random.normal(scale=sr, size=(4))
    for k in range(N):
        npred[k] = np.random.normal(scale=sq, size=(4))
        if upd_idx[k] >= 0:
            nupd[k + 1] = np.random.normal(scale=sr, size=(4))
    for k in range(N - 1, -1, -1):
        nrts[k] = np.random.normal(scale=sq, size=(4))
    return dict(noise_pred=npred, noise_upd=nupd, noise_rts=nrts)


@dataclasses.dataclass
class HostBatch:
    """NumPy image of ``struct ste_ukf_batch_f64``; arrays are C-contiguous with the track index last.

    ``Q`` / ``R`` are the shared 4 x 4 matrices.  Per-track noise (include/ste.h: ``ste_ukf_noise_f64``) travels in
    ``Q_tracks`` / ``R_tracks``: (10, B) upper triangles (row-major 00 01 02 03 11 12 13 22 23 33) in slot order, or None.
    Where ``Q_tracks`` (``R_tracks``) is set the kernels do not read ``Q`` (``R``): the 4 x 4 field is the fallback only for
    whichever of the two was not stacked.  ``pack_tracks`` / ``pack_uniform`` leave the stack's first matrix (the caller's
    track 0) in it, ``with_track_noise`` whatever ``hb`` held before.  ``track_matrices`` gives every track's effective pair."""

    B: int
    Nmax: int
    Tmax: int
    H: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    nsteps: np.ndarray  # (B,) int32
    x0: np.ndarray  # (4, B)
    P0: np.ndarray  # (16,) shared or (16, B)
    dt: np.ndarray  # (Nmax, B)
    sog_rate: np.ndarray
    cog_rate: np.ndarray
    sog_rate_rts: Optional[np.ndarray]
    cog_rate_rts: Optional[np.ndarray]
    upd_idx: np.ndarray  # (Nmax, B) int32
    z: np.ndarray  # (Tmax, 4, B)
    noise_pred: Optional[np.ndarray] = None  # (Nmax, 4, B)
    noise_upd: Optional[np.ndarray] = None  # (Nmax+1, 4, B)
    noise_rts: Optional[np.ndarray] = None  # (Nmax, 4, B)
    weights_computed: bool = True
    initial_update: bool = True
    robust: bool = False  # opt-in Mahalanobis robust update (not on the reference's shipped path)
    chi_alpha: float = 50.0
    host_status: Optional[np.ndarray] = None  # (B,) int32 bits set while packing (STATUS_HOST_INDEX)
    order: Optional[np.ndarray] = None  # (B,) batch slot -> index of the caller's track (length-bucketed packing)
    lanes: Optional[int] = None  # forward-kernel lane mapping for this batch: 1, 4, 0 = by batch size; None = default_lanes
    Q_tracks: Optional[np.ndarray] = None  # (10, B) per-track Q, upper triangles, or None = Q for every track
    R_tracks: Optional[np.ndarray] = None  # (10, B) per-track R, upper triangles, or None = R for every track

    @property
    def track_noise(self) -> bool:
        return self.Q_tracks is not None or self.R_tracks is not None

    @property
    def shared_p0(self) -> bool:
        return self.P0.ndim == 1

    @property
    def track_steps(self) -> int:
        return int(self.nsteps.sum())


SYMMETRY_RTOL = 1e-12  # |M - M^T| above this fraction of max|M| is "not symmetric" (rounding leaves ~1e-16)


def require_symmetric(M, name):
    """Raise ValueError unless every (.., 4, 4) matrix in ``M`` is symmetric to rounding.

    The kernels treat Q, R and every covariance as symmetric matrices (symmetric square root, eigenvalue pseudo-inverse,
    packed triangles); the reference calls scipy.linalg.sqrtm / np.linalg.pinv on whatever it is given, and for a
    non-symmetric argument those are a different computation (Schur form, SVD).  Such input is not a covariance, so it
    is refused rather than silently symmetrised (hard part 1)."""
    M = np.asarray(M, dtype=np.float64)
    asym = np.abs(M - np.swapaxes(M, -1, -2))
    scale = np.max(np.abs(M), axis=(-1, -2), keepdims=True)
    bad = ~(asym <= SYMMETRY_RTOL * scale) & np.isfinite(M) & np.isfinite(np.swapaxes(M, -1, -2))
    if np.any(bad):
        raise ValueError(f"{name} must be symmetric: max |{name} - {name}^T| = {float(np.max(np.where(bad, asym, 0.0))):.3e}; "
                         "the HIP path works on symmetric covariances (scipy.linalg.sqrtm / np.linalg.pinv of a "
                         "non-symmetric matrix, unscented.py:97,243, is a different computation)")
    return M


def _as44(M, name, symmetric: bool = False):
    M = np.ascontiguousarray(np.asarray(M, dtype=np.float64))
    if M.shape != (4, 4):
        raise ValueError(f"{name} must be 4x4 for the HIP path (got {M.shape}); the reference hard-codes the heading at "
                         "index 3 (unscented.py:250)")
    if symmetric:
        require_symmetric(M, name)
    return M


_TRI = np.triu_indices(4)  # row-major upper triangle: 00 01 02 03 11 12 13 22 23 33 (STE_FLAG_PACKED_COV's order)


def _noise_arg(M, name, B, order=None):
    """One 4 x 4 matrix, or a stack (B, 4, 4) / sequence of B matrices in the caller's track order (``order``: slot ->
    caller's track).  Returns (the shared 4 x 4, (10, B) upper triangles in slot order or None)."""
    A = np.asarray(M, dtype=np.float64)
    if A.ndim == 2:
        return _as44(A, name, True), None
    if A.shape != (B, 4, 4):
        raise ValueError(f"{name} must be one 4x4 matrix or a stack of one per track, ({B}, 4, 4); got {A.shape}")
    for i in range(B):
        require_symmetric(A[i], f"{name}[{i}]")  # the message names the track
    first = np.ascontiguousarray(A[0])
    if order is not None:
        A = A[order]
    return first, np.ascontiguousarray(A[:, _TRI[0], _TRI[1]].T)


def r_tracks_block2(R_tracks) -> bool:
    """Is every track's R zero outside its leading 2 x 2 block (entries 00, 01, 11 of the triangle)?  What
    ``STE_NOISE_R_BLOCK2`` promises to the library, which cannot look into device memory before a launch."""
    rest = np.delete(np.asarray(R_tracks), (0, 1, 4), axis=0)
    return bool(np.all(rest == 0.0))


def track_matrices(hb: "HostBatch"):
    """(Q, R) as (B, 4, 4) stacks in slot order: what every track of ``hb`` filters with -- its own triangle expanded where
    ``Q_tracks`` / ``R_tracks`` is set, the shared matrix otherwise."""
    full = np.zeros((4, 4), dtype=np.intp)
    full[_TRI] = np.arange(10)
    full = np.maximum(full, full.T)  # position of (r, c) in the packed triangle
    out = []
    for shared, tri in ((hb.Q, hb.Q_tracks), (hb.R, hb.R_tracks)):
        out.append(np.broadcast_to(shared, (hb.B, 4, 4)) if tri is None else np.ascontiguousarray(tri.T[:, full]))
    return out[0], out[1]


def with_track_noise(hb: "HostBatch", Q=None, R=None) -> "HostBatch":
    """A copy of ``hb`` (arrays shared) with per-track noise: ``Q`` / ``R`` are stacks (B, 4, 4) in SLOT order (the order
    of ``hb``'s arrays; ``hb.order`` maps slots to the caller's tracks), each checked for symmetry per matrix; None leaves
    that one as it is in ``hb`` (shared, or the stack ``hb`` already carries).  ``hb.Q`` / ``hb.R`` are not touched."""
    new = {}
    for name, M in (("Q", Q), ("R", R)):
        if M is None:
            continue
        A = np.asarray(M, dtype=np.float64)
        if A.shape != (hb.B, 4, 4):
            raise ValueError(f"{name} must be a stack of one 4x4 matrix per track, ({hb.B}, 4, 4); got {A.shape}")
        new[name + "_tracks"] = _noise_arg(A, name, hb.B)[1]
    return dataclasses.replace(hb, **new)


def apply_noise_choice(hb: "HostBatch", candidates: Sequence, choice: "NoiseChoice") -> "HostBatch":
    """The step after ``log_likelihood_grid`` and ``best_noise(grid, per_track=True)``: a copy of ``hb`` in which track
    (slot) b filters and smooths with ``candidates[choice.index[b]]``; a track with index -1 keeps the pair it has in
    ``hb``: the shared one, or its own if ``hb`` already carries stacks (``track_matrices``)."""
    cands = [(_as44(Q, "Q", True), _as44(R, "R", True)) for Q, R in candidates]
    idx = np.asarray(choice.index)
    if idx.shape != (hb.B,):
        raise ValueError(f"choice.index must hold one candidate index per track, ({hb.B},): take it from "
                         f"best_noise(grid, per_track=True); got shape {idx.shape}")
    if ((idx < -1) | (idx >= len(cands))).any():
        raise ValueError(f"choice.index out of range for {len(cands)} candidates")
    Q0, R0 = track_matrices(hb)
    Qs = np.stack([cands[i][0] if i >= 0 else Q0[b] for b, i in enumerate(idx)])
    Rs = np.stack([cands[i][1] if i >= 0 else R0[b] for b, i in enumerate(idx)])
    return with_track_noise(hb, Qs, Rs)


STATUS_HOST_INDEX = binding.STE_STATUS_HOST_INDEX  # the reference would raise IndexError for this track (update index past the last observation)

# Lane mapping used by batches that do not name one (HostBatch.lanes is None): 0 = the library picks by batch size.
# A per-call flag of the C ABI underneath (STE_FLAG_LANES_1 / _4); the tests set this to run every case in both mappings.
default_lanes = 0
# ste_ukf_batch_f64.tuning of batches that do not name one (DeviceBatch(tuning=0)).  Bits (include/ste.h): 0x100 every smoother
# gain by the eigenvalue route, 0x200 / 0x400 the two-kernel / one-kernel smoother whatever the batch size, 0x800 the
# two-kernel form's recurrence with a lane instead of a quad per track.  Tests set it.
default_tuning = 0


def pack_tracks(tracks: Sequence, dts_per_track: Sequence, x0s: Sequence, H, Q, R, P0, t0s=None,
                noise: Optional[Sequence[dict]] = None, on_error: str = "flag",
                bucket_by_length: bool = True) -> HostBatch:
    """
    Pack B tracks (objects carrying ``z`` (4,T), ``dts`` (T-1,), ``sog_rate`` (T,), ``cog_rate`` (T,) like a
    reference ``ShipTrack``, ship_track.py:70-83) with their per-track ``dt`` arrays and priors into a HostBatch.
    Ragged batches are padded to the longest track.  ``P0`` is one 4x4 shared matrix or a sequence of B matrices.
    ``Q`` and ``R`` likewise: one shared 4x4 matrix each, or a stack (B, 4, 4) / sequence of B matrices -- per-track noise,
    checked per matrix and laid out like the tracks (``HostBatch.Q_tracks`` / ``R_tracks``).
    ``noise`` (test-only) is a per-track list of dicts with ``noise_pred`` (N,4), ``noise_upd`` (N+1,4), ``noise_rts`` (N,4).
    ``on_error``: a track whose update index runs past its last observation (duplicate timestamps make the
    float-equality trigger fire twice per gap) raises IndexError in the reference (kalman_filter.py:105).  "raise" does
    the same; "flag" (default, the batch example's try/except/continue) truncates that track at the offending step and
    sets STATUS_HOST_INDEX in ``host_status``.
    ``bucket_by_length``: tracks are laid out longest first, so that the 16 or 64 tracks sharing a wave have similar
    step counts and the wave does not idle through the tail of one long track (real data: 30 .. 9 619 observations per
    ship).  ``HostBatch.order`` records the permutation; ``run_batch`` returns results in the caller's order.
    """
    B = len(tracks)
    if B == 0:
        raise ValueError("empty batch")
    Q_in, R_in = Q, R
    order = None
    if bucket_by_length and B > 1:
        lens = np.array([len(d) for d in dts_per_track])
        if len(set(lens.tolist())) > 1:
            order = np.argsort(-lens, kind="stable")
            tracks = [tracks[i] for i in order]
            dts_per_track = [dts_per_track[i] for i in order]
            x0s = [x0s[i] for i in order]
            t0s = None if t0s is None else [t0s[i] for i in order]
            noise = None if noise is None else [noise[i] for i in order]
            P0a = np.asarray(P0, dtype=np.float64)
            if P0a.ndim == 3:
                P0 = P0a[order]
    H = _as44(H, "H")
    (Q, Qt), (R, Rt) = _noise_arg(Q_in, "Q", B, order), _noise_arg(R_in, "R", B, order)
    Ns = [len(d) for d in dts_per_track]
    Ts = [np.asarray(tr.z).shape[1] for tr in tracks]
    Nmax, Tmax = max(Ns), max(Ts)
    nsteps = np.asarray(Ns, dtype=np.int32)
    host_status = np.zeros(B, dtype=np.int32)
    x0 = np.zeros((4, B))
    dt = np.zeros((Nmax, B))
    sr = np.zeros((Nmax, B))
    cr = np.zeros((Nmax, B))
    srr = np.zeros((Nmax, B))
    crr = np.zeros((Nmax, B))
    ui = np.full((Nmax, B), -1, dtype=np.int32)
    z = np.zeros((Tmax, 4, B))
    P0 = require_symmetric(P0, "P0")
    if P0.shape == (4, 4):
        P0p = np.ascontiguousarray(P0.reshape(16))
    elif P0.shape == (B, 4, 4):
        P0p = np.ascontiguousarray(P0.reshape(B, 16).T)
    else:
        raise ValueError(f"P0 must be (4,4) or (B,4,4), got {P0.shape}")
    have_noise = noise is not None
    npred = np.zeros((Nmax, 4, B)) if have_noise else None
    nupd = np.zeros((Nmax + 1, 4, B)) if have_noise else None
    nrts = np.zeros((Nmax, 4, B)) if have_noise else None
    for b, tr in enumerate(tracks):
        zb = np.asarray(tr.z, dtype=np.float64)
        if zb.shape[0] != 4:
            raise ValueError("measurement matrix z must have 4 rows (lon, lat, sog, cog): call "
                             "get_measurements(include_sog=True, include_cog=True)")
        T, N = Ts[b], Ns[b]
        d = np.asarray(dts_per_track[b], dtype=np.float64)
        dts = np.asarray(tr.dts, dtype=np.float64)
        sog_rate = np.asarray(tr.sog_rate, dtype=np.float64)
        cog_rate = np.asarray(tr.cog_rate, dtype=np.float64)
        u, ridx, _ = update_schedule(d, dts, 0 if t0s is None else t0s[b])
        if N and (u.max() >= T or ridx.max() >= len(sog_rate)):
            if on_error == "raise":
                raise IndexError("update index runs past the last observation (kalman_filter.py:105)")
            bad = np.flatnonzero((u >= T) | (ridx >= len(sog_rate)))[0]
            N = int(bad)
            Ns[b] = N
            nsteps[b] = N
            host_status[b] |= STATUS_HOST_INDEX
            d, u, ridx = d[:N], u[:N], ridx[:N]
        x0[:, b] = np.asarray(x0s[b], dtype=np.float64).reshape(-1)
        z[:T, :, b] = zb.T
        dt[:N, b] = d
        ui[:N, b] = u
        sr[:N, b] = sog_rate[ridx]
        cr[:N, b] = cog_rate[ridx]
        if N and len(dts) and not host_status[b]:
            try:
                rr = rts_rate_index(N + 1, len(dts), len(sog_rate))
                srr[:N, b] = sog_rate[rr]
                crr[:N, b] = cog_rate[rr]
            except IndexError:
                # only the smoother needs these; surface the reference's IndexError when it is called
                srr[:N, b] = np.nan
                crr[:N, b] = np.nan
        if have_noise:
            nb = noise[b]
            npred[:N, :, b] = np.asarray(nb["noise_pred"])[:N]
            nupd[: N + 1, :, b] = np.asarray(nb["noise_upd"])[: N + 1]
            nrts[:N, :, b] = np.asarray(nb["noise_rts"])[:N]
    same_rts = np.array_equal(sr, srr) and np.array_equal(cr, crr)
    return HostBatch(B=B, Nmax=Nmax, Tmax=Tmax, H=H, Q=Q, R=R, nsteps=nsteps, x0=x0, P0=P0p, dt=dt, sog_rate=sr,
                     cog_rate=cr, sog_rate_rts=None if same_rts else srr, cog_rate_rts=None if same_rts else crr,
                     upd_idx=ui, z=z, noise_pred=npred, noise_upd=nupd, noise_rts=nrts, host_status=host_status,
                     order=order, Q_tracks=Qt, R_tracks=Rt)


def pack_uniform(sb, substeps: int, H, Q, R, P0) -> HostBatch:
    """
    Fast path for a batch where every track has the same number of observations (``synthetic.SyntheticBatch``):
    vectorised over tracks.  x0 = z[:, 0] (example_ukf_rts_smoother_batch.py:60); dt = generate_dts(dts, substeps).
    ``Q`` / ``R``: one 4x4 matrix each or a stack (B, 4, 4), as in ``pack_tracks``.
    """
    B, T = sb.lon.shape
    H = _as44(H, "H")
    (Q, Qt), (R, Rt) = _noise_arg(Q, "Q", B), _noise_arg(R, "R", B)
    s = int(substeps)
    N = s * (T - 1)
    dt = np.repeat(sb.dts / s, s, axis=1)  # (B, N): utils.py:194-198
    cums = np.cumsum(sb.dts, axis=1)
    times = np.cumsum(dt, axis=1)  # sequential per row, starting from 0 + dt[0] == dt[0]
    fires = np.empty((B, N), dtype=bool)
    for b in range(B):
        fires[b] = _isin_exact(times[b], cums[b])
    after = np.cumsum(fires, axis=1, dtype=np.int32)
    upd_idx = np.where(fires, after, np.int32(-1))
    ridx = after - fires
    if upd_idx.max() >= T:
        raise IndexError("update index runs past the last observation (kalman_filter.py:105)")
    # everything below is produced directly in the device layout [step][track] (gathers with transposed index views)
    c = np.ascontiguousarray
    cols = np.arange(B)[None, :]
    sog_t, cog_t = c(sb.sog_rate.T), c(sb.cog_rate.T)  # (T, B)
    ridx_t = ridx.T
    sr = sog_t[ridx_t, cols]
    cr = cog_t[ridx_t, cols]
    rr = rts_rate_index(N + 1, T - 1, T)
    same_rts = bool(np.array_equal(ridx, np.broadcast_to(rr, (B, N))))
    if not same_rts:
        srr, crr = sog_t[rr], cog_t[rr]
        same_rts = np.array_equal(sr, srr) and np.array_equal(cr, crr)
    P0 = require_symmetric(_as44(P0, "P0"), "P0")
    return HostBatch(
        B=B, Nmax=N, Tmax=T, H=H, Q=Q, R=R, nsteps=np.full(B, N, dtype=np.int32), x0=c(sb.z[:, :, 0].T),
        P0=c(P0.reshape(16)), dt=np.repeat(c(sb.dts.T) / s, s, axis=0), sog_rate=sr, cog_rate=cr,
        sog_rate_rts=None if same_rts else srr, cog_rate_rts=None if same_rts else crr,
        upd_idx=c(upd_idx.T), z=c(sb.z.transpose(2, 1, 0)), Q_tracks=Qt, R_tracks=Rt,
    )


# ----------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------
def states_in_place(shape, strides, Nmax: int, ld: int) -> bool:
    """Are the rows of a (S, Nmax+1, 4, B) tensor with these strides (in elements) the rows of a fleet ``ld`` tracks wide, so
    that a metric call can read it where it lies?  The stride of a dimension of size 1 is never used and is ignored."""
    fleet_strides = ((Nmax + 1) * 4 * ld, 4 * ld, ld, 1)
    return all(n == 1 or sd == fd for n, sd, fd in zip(shape, strides, fleet_strides))


def _metric_model(model) -> int:
    """STE_PREP_* of a leg function's name."""
    if model not in DeviceBatch._PATH_MODELS:
        raise ValueError(f"model must be one of {sorted(DeviceBatch._PATH_MODELS)}, got {model!r}")
    return DeviceBatch._PATH_MODELS[model]


def _index_tensor(x, name: str, tail_shape: tuple, limit: int):
    """A list of track indices (``pairs`` (P, 2), ``qtrack`` (Q,)) given as an integer array or tensor, as an integer
    tensor of shape (n,) + ``tail_shape`` with 1 <= n <= ``limit``; an array comes back as int64 on the host."""
    import torch

    letter = name[0].upper()
    shape = "(" + ", ".join([letter] + [str(n) for n in tail_shape]) + ("," if not tail_shape else "") + ")"
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
        if x.dtype.kind not in "iu":
            raise ValueError(f"{name} must be a {shape} integer array or tensor, got dtype {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x.astype(np.int64)))
    elif x.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"{name} must be a {shape} integer array or tensor, got dtype {x.dtype}")
    if x.dim() != 1 + len(tail_shape) or tuple(x.shape[1:]) != tuple(tail_shape) or not 1 <= x.shape[0] <= limit:
        raise ValueError(f"{name} must have shape {shape} with 1 <= {letter} <= {limit}, got {tuple(x.shape)}")
    return x


def _index_int32(x):
    """An integer tensor as contiguous int32 for a kernel: an index that does not fit 32 bits stays outside [0, B)."""
    import torch

    return x.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()


def column_pointer(ten, col: int) -> int:
    """The address of column ``col`` of a tensor whose last dimension is the track: what a kernel takes as the first track
    of a window that reads or writes rows as wide as the tensor's."""
    return ten.data_ptr() + ten.element_size() * col


def track_outputs(struct, width: int, col: int, B: int, spec, device) -> dict:
    """The per-track outputs of a metric call.  ``spec``: (field, leading shape, dtype, fill) per output; ``fill`` None leaves
    the tensor as allocated (``torch.empty``), 0 zeroes it, anything else (NaN, -1) fills it.  Each is allocated
    ``leading + (width,)`` on ``device``, ``struct.<field>`` is set to its column ``col``, and the dict returned holds the
    views ``[..., col:col + B]``: for a window read in place (``_fleet_layout``) the call writes this window's columns of rows
    as wide as the fleet's and nothing else."""
    import torch

    out = {}
    for field, leading, dtype, fill in spec:
        shape = tuple(leading) + (width,)
        if fill is None:
            ten = torch.empty(shape, dtype=dtype, device=device)
        elif fill == 0:
            ten = torch.zeros(shape, dtype=dtype, device=device)
        else:
            ten = torch.full(shape, fill, dtype=dtype, device=device)
        setattr(struct, field, column_pointer(ten, col))
        out[field] = ten[..., col:col + B]
    return out


def track_input(x, B: int, width: int, col: int, keep: list, device, expect: str, scalar: bool = False):
    """A per-track input of a metric call -- None, a scalar or one value per track, (B,) -- as the pointer the kernel
    takes: column ``col`` of a zeroed float64 row ``width`` tracks wide that holds the values in this batch's columns (the
    row is appended to ``keep``); None for None.  ``scalar``: the kernel takes a scalar beside the pointer, and the result is
    the pair (pointer, value): (None, the float) for a 0-d value, (pointer, None) for (B,).  ``expect``: how the message
    for any other shape begins, which differs between the callers."""
    import torch

    if x is None:
        return (None, None) if scalar else None
    tv = torch.as_tensor(x, dtype=torch.float64)
    if tv.dim() == 0:
        if scalar:
            return None, float(tv)
    elif tuple(tv.shape) != (B,):
        raise ValueError(f"{expect}, got {tuple(tv.shape)}")
    tv = tv.to(device).expand(B)
    row = torch.zeros((width,), dtype=torch.float64, device=device)
    row[col:col + B] = tv
    keep.append(row)
    ptr = column_pointer(row, col)
    return (ptr, None) if scalar else ptr


class DeviceBatch:
    """A HostBatch resident in HBM plus its output buffers; ``forward`` / ``backward`` / ``run`` launch the kernels."""

    _IN = ("nsteps", "x0", "P0", "dt", "sog_rate", "cog_rate", "sog_rate_rts", "cog_rate_rts", "upd_idx", "z",
           "noise_pred", "noise_upd", "noise_rts")
    _NOISE_IN = ("Q_tracks", "R_tracks")  # per-track noise: inputs like the others, named by ``noise`` instead of ``struct``

    # position of (r, c) in a packed upper triangle, for all 16 entries of the full matrix (include/ste.h: STE_FLAG_PACKED_COV)
    _PACKED_INDEX = [min(r, c) * 4 - (min(r, c) * (min(r, c) - 1)) // 2 + abs(r - c) for r in range(4) for c in range(4)]

    def __init__(self, hb: HostBatch, device="cuda:0", alloc_smoothed: bool = True, fuse_gains: bool = True,
                 tuning: int = 0, packed_cov: bool = True, sm_pos: bool = False, upload: bool = True,
                 histories: bool = True):
        """``sm_pos``: also allocate the smoother's optional [N+1][2][B] output of smoothed lon / lat (what a multi-GPU
        run exchanges).  ``upload=False``: allocate the input tensors without filling them -- ``upload_tracks(lo, hi)``
        then brings the host batch up window by window (``run_fleet``).  ``histories=False``: no history, smoother or
        work buffers at all -- a batch for ``log_likelihood`` alone (``log_likelihood_grid``); ``forward`` / ``run``
        refuse it."""
        import torch

        self.lib = binding.require_gpu()
        self.torch = torch
        self.hb = hb
        self.device = torch.device(device)
        self.t = {}
        lanes = default_lanes if hb.lanes is None else hb.lanes
        if lanes == 4 and hb.track_noise:
            raise ValueError("per-track noise (Q_tracks / R_tracks) runs the lane-per-track mapping only: the quad forward "
                             "kernel has none, so lanes=4 is refused for this batch")
        for name in self._IN + self._NOISE_IN:
            a = getattr(hb, name)
            if a is None:
                self.t[name] = None
            elif upload:
                self.t[name] = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            else:
                self.t[name] = torch.empty(a.shape, dtype=torch.from_numpy(a[..., :0]).dtype, device=self.device)
        B, N = hb.B, hb.Nmax
        self.ntracks, self.lo, self.parent = B, 0, None
        f64 = dict(dtype=torch.float64, device=self.device)
        if not histories:
            alloc_smoothed = False
        self.fwd_mean = torch.empty((N + 1, 4, B), **f64) if histories else None
        # covariance histories as upper triangles on the device (they are symmetric by construction); download()
        # expands them to the reference's (.., 4, 4).  packed_cov=False keeps full matrices in HBM.
        self.packed_cov = bool(packed_cov)
        cov_rows = 10 if self.packed_cov else 16
        self.fwd_cov = torch.empty((N + 1, cov_rows, B), **f64) if histories else None
        self.sm_mean = torch.empty((N + 1, 4, B), **f64) if alloc_smoothed else None
        self.sm_cov = torch.empty((N + 1, cov_rows, B), **f64) if alloc_smoothed else None
        # rows past a short track's end are never written: zeros, so that a gathered tensor is defined everywhere
        self.sm_pos = torch.zeros((N + 1, 2, B), **f64) if (alloc_smoothed and sm_pos) else None
        self.status = torch.zeros((B,), dtype=torch.int32, device=self.device)
        # workspace for the smoother gains the forward pass can produce on the way (include/ste.h: rts_work)
        self.rts_work = None
        if alloc_smoothed and fuse_gains and N > 0:
            self.rts_work = torch.empty((N * binding.STE_RTS_WORK_ROWS + 1, B), **f64)  # include/ste.h: rts_work
        fan_scale, w0, wi = sigma_constants(4, hb.weights_computed)
        self._keep = (hb.H, hb.Q, hb.R)
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.Tmax, s.n = B, N, hb.Tmax, 4
        if lanes not in (0, 1, 4):
            raise ValueError(f"lanes must be 0 (automatic), 1 or 4, got {lanes!r}")
        s.flags = (binding.STE_FLAG_SHARED_P0 if hb.shared_p0 else 0) | (
            0 if hb.initial_update else binding.STE_FLAG_NO_INITIAL_UPDATE) | (
            binding.STE_FLAG_ROBUST if hb.robust else 0) | {0: 0, 1: binding.STE_FLAG_LANES_1, 4: binding.STE_FLAG_LANES_4}[lanes] | (
            binding.STE_FLAG_PACKED_COV if self.packed_cov else 0)
        s.tuning = int(tuning) if tuning else int(default_tuning)
        s.chi_alpha, s.robust_max_iter = float(hb.chi_alpha), 50
        s.fan_scale, s.w0, s.wi = fan_scale, w0, wi
        s.H, s.Q, s.R = hb.H.ctypes.data, hb.Q.ctypes.data, hb.R.ctypes.data
        for name in self._IN:
            ten = self.t[name]
            setattr(s, name, None if ten is None else ten.data_ptr())
        s.fwd_mean = None if self.fwd_mean is None else self.fwd_mean.data_ptr()
        s.fwd_cov = None if self.fwd_cov is None else self.fwd_cov.data_ptr()
        s.sm_mean = None if self.sm_mean is None else self.sm_mean.data_ptr()
        s.sm_cov = None if self.sm_cov is None else self.sm_cov.data_ptr()
        s.status = self.status.data_ptr()
        s.rts_work = None if self.rts_work is None else self.rts_work.data_ptr()
        s.track_stride = 0
        s.sm_pos = None if self.sm_pos is None else self.sm_pos.data_ptr()
        s.step_begin = s.step_end = 0
        self.struct = s
        # per-track noise beside the batch struct (include/ste.h: ste_ukf_noise_f64), or None
        self.noise = None
        tq, tr = self.t["Q_tracks"], self.t["R_tracks"]
        if tq is not None or tr is not None:
            block2 = tr is not None and r_tracks_block2(hb.R_tracks)
            self.noise = binding.SteUkfNoiseF64(None if tq is None else tq.data_ptr(), None if tr is None else tr.data_ptr(),
                                                binding.STE_NOISE_R_BLOCK2 if block2 else 0, 0)
        # The uploads above were queued on the current stream.  One event, recorded now, is what other streams wait on
        # before the first launch (SmootherPipeline.submit): waiting on the current stream *at submit time* would put a
        # marker on the legacy default stream, which every blocking stream synchronises with -- a device-wide barrier in
        # the middle of a pipelined sequence (two of them cost a --steps 20 --warmup 5 run 10 of its 32 ms in round 2).
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))
        self._pipeline_done = None
        self._last_use = None  # event after the last forward / backward / run issued outside a pipeline
        self._reader_done = None  # event an after_smoother hook returned: something (a collective) still reads the outputs

    # -- windows of a resident batch ----------------------------------------------------------------------------
    _PER_TRACK_F64 = ("x0", "dt", "sog_rate", "cog_rate", "sog_rate_rts", "cog_rate_rts", "z", "noise_pred",
                      "noise_upd", "noise_rts", "fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "rts_work", "sm_pos")
    _PER_TRACK_I32 = ("nsteps", "upd_idx", "status")

    def window(self, lo: int, hi: int) -> "DeviceBatch":
        """Tracks [lo, hi) of this resident batch as a batch of their own: same tensors, a batch struct whose pointers
        name track ``lo`` and whose ``track_stride`` is this batch's width (include/ste.h) -- nothing is copied.  The
        windows of a fleet go through ``SmootherPipeline`` like separate batches and write straight into the fleet's
        histories (``run_fleet``)."""
        if not (0 <= lo < hi <= self.ntracks):
            raise ValueError(f"window [{lo}, {hi}) outside the batch's {self.ntracks} tracks")
        w = object.__new__(DeviceBatch)
        w.__dict__.update(self.__dict__)
        w.parent = self if self.parent is None else self.parent
        w.lo, w.ntracks = self.lo + lo, hi - lo
        s = binding.SteUkfBatchF64.from_buffer_copy(self.struct)
        s.B = hi - lo
        s.track_stride = self.struct.track_stride or self.struct.B
        for name in self._PER_TRACK_F64 + self._PER_TRACK_I32:
            ptr = getattr(s, name)
            if ptr:
                setattr(s, name, ptr + lo * (4 if name in self._PER_TRACK_I32 else 8))
        if not self.hb.shared_p0:
            s.P0 = s.P0 + lo * 8
        w.struct = s
        if self.noise is not None:  # the two triangles are [10][track_stride] like every per-track array
            w.noise = binding.SteUkfNoiseF64((self.noise.Q + lo * 8) if self.noise.Q else None,
                                             (self.noise.R + lo * 8) if self.noise.R else None, self.noise.flags, 0)
        for name in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "sm_pos"):
            t = getattr(self, name)
            setattr(w, name, None if t is None else t[..., lo:hi])
        w.status = self.status[lo:hi]
        # the copied __dict__ leaves the window the parent's _uploaded and a pending _reader_done: its first submit waits for both
        w._pipeline_done = None
        w._last_use = None
        return w

    def upload_tracks(self, lo: int, hi: int, stream=None):
        """Bring tracks [lo, hi) of the host batch into the (``upload=False``) input tensors: page-locked staging, filled by
        a few threads (the strided slice copies release the GIL; one thread moves ~12 GB/s, and direct strided DMA from
        page-locked NumPy memory was measured far slower: 0.3 GB/s), then asynchronous copies on ``stream``; returns the event
        that marks them resident."""
        torch = self.torch
        stream = stream or torch.cuda.current_stream(self.device)
        jobs = []
        for name in self._IN + self._NOISE_IN:
            ten = self.t[name]
            if ten is None or (name == "P0" and self.hb.shared_p0):
                continue
            src = getattr(self.hb, name)[..., lo:hi]
            stage = torch.empty(src.shape, dtype=ten.dtype, pin_memory=True)
            jobs.append((ten, stage, src))

        def fill(job):
            job[1].numpy()[...] = job[2]

        if sum(j[2].nbytes for j in jobs) > (64 << 20):
            list(_staging_pool().map(fill, jobs))
        else:
            for j in jobs:
                fill(j)
        with torch.cuda.stream(stream):
            for ten, stage, _ in jobs:
                ten[..., lo:hi].copy_(stage, non_blocking=True)
            if self.hb.shared_p0 and lo == 0:
                self.t["P0"].copy_(torch.from_numpy(np.ascontiguousarray(self.hb.P0)))
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev

    def _stream(self, stream):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device)
        return C.c_void_p(stream.cuda_stream)

    def _mark_use(self, stream):
        # kernels issued outside a pipeline: a later SmootherPipeline.submit of this batch orders itself behind them
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device)
        if not stream.cuda_stream:
            return  # the legacy default stream orders itself against every blocking stream (the pipeline's included)
        self._last_use = self.torch.cuda.Event()
        self._last_use.record(stream)

    # -- the front end the metric calls share ("Metric front end") ---------------------------------------
    _PATH_MODELS = {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}
    _PATH_AXES = {"lon": 0, "lat": 1}

    def _ordered_stream(self, stream):
        """The stream a call runs on (default: the current one), ordered after the current stream's work, the batch's
        upload and the pipeline that last ran it."""
        cur = self.torch.cuda.current_stream(self.device)
        st = cur if stream is None else stream
        if st is not cur:
            st.wait_stream(cur)  # whatever the caller queued on the current stream (inputs, histories) comes first
        st.wait_event(self._uploaded)
        if self._pipeline_done is not None:
            st.wait_event(self._pipeline_done)
        return st

    def _metric_states(self, states):
        """``states`` of a metric call as (S, Nmax+1, 4, B), and S."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        want = f"states must be a float64 tensor of shape (S, {N + 1}, 4, {B}) or ({N + 1}, 4, {B}) on {self.device}"
        if not isinstance(states, torch.Tensor) or states.dtype != torch.float64 or states.device != self.device:
            raise ValueError(want)
        if states.dim() == 3:
            states = states.unsqueeze(0)
        if states.dim() != 4 or tuple(states.shape[1:]) != (N + 1, 4, B) or states.shape[0] < 1:
            raise ValueError(want + f", got {tuple(states.shape)}")
        return states, int(states.shape[0])

    def _fleet_layout(self, states, keep, needs_dt: bool):
        """How a metric call reads ``states``: in place when the tensor's rows are the fleet's (ld tracks wide, this window's
        columns), else as a batch of its own, made contiguous.  Returns (a copy of the batch struct for the call, states,
        the width of a row of per-track outputs, this batch's first column in it).  ``needs_dt``: the call reads ``dt``,
        the one batch array read in rows of track_stride, so a window that is not read in place gets a copy of its
        columns.  Inside the stream context; what the call must outlive is appended to ``keep``."""
        N, B = int(self.struct.Nmax), self.ntracks
        ld = int(self.struct.track_stride or self.struct.B)
        s = binding.SteUkfBatchF64.from_buffer_copy(self.struct)
        keep.append(states)
        if states_in_place(states.shape, states.stride(), N, ld):
            return s, states, ld, self.lo
        states = states.contiguous()
        s.track_stride = 0
        keep.append(states)
        if needs_dt and ld != B:
            dt = self.t["dt"][:, self.lo:self.lo + B].contiguous()
            s.dt = dt.data_ptr()
            keep.append(dt)
        return s, states, B, 0

    def _track_clock(self, t0, width, col, keep, name: str = "t0"):
        """``t0`` of a metric call (None, a scalar or one clock time per track) as the pointer the kernel takes, or None.
        Inside the stream context.  ``name``: what the value is called in the message (another per-track input of the
        same form, such as ``track_margin_km``)."""
        B = self.ntracks
        return track_input(t0, B, width, col, keep, self.device, f"{name} must be None, a scalar or have shape ({B},)")

    def _track_outputs(self, struct, width, col, spec):
        """``track_outputs`` for this batch's tracks on its device.  Inside the stream context."""
        return track_outputs(struct, width, col, self.ntracks, spec, self.device)

    def _finish(self, st, keep, out):
        """After the launch: inputs and outputs stay allocated until ``st`` has passed it."""
        for ten in keep:
            ten.record_stream(st)
        self._mark_use(st)
        for ten in out.values():
            ten.record_stream(st)
        return out

    @staticmethod
    def slice_bounds(nsteps: int, slices: int):
        """Step ranges of a forward pass cut into ``slices`` time slices: boundaries on multiples of STE_SLICE_ALIGN (64
        steps), where the eigen-solve's warm start restarts anyway, so the slices reproduce the whole pass bit for bit."""
        a = binding.STE_SLICE_ALIGN
        if slices <= 1 or nsteps <= a:
            return [(0, nsteps)]
        step = -(-nsteps // (slices * a)) * a
        cuts = list(range(0, nsteps, step)) + [nsteps]
        return list(zip(cuts[:-1], cuts[1:]))

    def _require_histories(self, what):
        if self.fwd_mean is None:
            raise ValueError(f"{what} needs the filtered histories, and this batch was built with histories=False (a batch "
                             "for log_likelihood alone)")

    def forward(self, stream=None, slices: int = 1, mark: bool = True):
        """The forward pass; ``slices`` > 1 issues it as that many launches over consecutive step ranges (include/ste.h:
        step_begin / step_end), bit-identical to the single launch."""
        self._require_histories("forward()")
        s = self.struct
        try:
            for k0, k1 in self.slice_bounds(int(s.Nmax), int(slices)):
                s.step_begin, s.step_end = k0, k1
                if self.noise is not None:
                    binding.check(self.lib.ste_ukf_forward_noise_f64(C.byref(s), C.byref(self.noise), None, self._stream(stream)),
                                  "ste_ukf_forward_noise_f64")
                    continue
                binding.check(self.lib.ste_ukf_forward_f64(C.byref(s), self._stream(stream)), "ste_ukf_forward_f64")
        finally:
            s.step_begin = s.step_end = 0
        if mark:
            self._mark_use(stream)

    def backward(self, stream=None, mark: bool = True):
        self._require_histories("backward()")
        if self.noise is not None:
            binding.check(self.lib.ste_urtss_backward_noise_f64(C.byref(self.struct), C.byref(self.noise), self._stream(stream)),
                          "ste_urtss_backward_noise_f64")
        else:
            binding.check(self.lib.ste_urtss_backward_f64(C.byref(self.struct), self._stream(stream)),
                          "ste_urtss_backward_f64")
        if mark:
            self._mark_use(stream)

    def run(self, stream=None):
        self._require_histories("run()")
        if self.noise is not None:
            binding.check(self.lib.ste_ukf_urtss_noise_f64(C.byref(self.struct), C.byref(self.noise), self._stream(stream)),
                          "ste_ukf_urtss_noise_f64")
        else:
            binding.check(self.lib.ste_ukf_urtss_f64(C.byref(self.struct), self._stream(stream)), "ste_ukf_urtss_f64")
        self._mark_use(stream)

    def log_likelihood(self, stream=None, nis: bool = False) -> "LogLikelihood":
        """The forward pass with the innovation log-likelihood (include/ste.h: ste_ukf_forward_loglik_f64), on this batch's
        own histories: with histories allocated it writes the same bits as ``forward`` with the lane-per-track mapping
        (rts_work and status included, so ``backward`` may follow).  It always uses the lane-per-track mapping, whatever
        ``lanes`` the batch was built with: the quad mapping has no likelihood.  Returns a ``LogLikelihood`` of NumPy
        arrays in this batch's track order (HostBatch slots, ``hb.order`` maps them to the caller's tracks).
        ``nis``: also the normalised innovation squared per history row, (B, Nmax+1), NaN where no update fired and past
        a track's last step.  ``stream``: the stream the pass runs on (default: the current one); it is ordered after the
        current stream's work and the batch's upload, and the results are read back on it once the pass is done."""
        torch = self.torch
        st = self._ordered_stream(stream)
        B, N = self.ntracks, int(self.struct.Nmax)
        ld = int(self.struct.track_stride or self.struct.B)
        col = self.lo  # a window's first column in rows of `ld` (0 for a batch of its own)
        dev = dict(device=self.device)
        with torch.cuda.stream(st):  # outputs allocated, filled, written and read back on `st`, in that order
            ll = torch.empty((B,), dtype=torch.float64, **dev)
            dof = torch.empty((B,), dtype=torch.int32, **dev)
            nupd = torch.empty((B,), dtype=torch.int32, **dev)
            lk = binding.SteUkfLoglikF64(ll.data_ptr(), dof.data_ptr(), nupd.data_ptr(), None)
            nis_t = self._track_outputs(lk, ld, col, [("nis", (N + 1,), torch.float64, float("nan"))])["nis"] if nis else None
            s = binding.SteUkfBatchF64.from_buffer_copy(self.struct)
            s.flags = (s.flags & ~binding.STE_FLAG_LANES_4) | binding.STE_FLAG_LANES_1
            if self.noise is not None:
                binding.check(self.lib.ste_ukf_forward_noise_f64(C.byref(s), C.byref(self.noise), C.byref(lk), self._stream(st)),
                              "ste_ukf_forward_noise_f64")
            else:
                binding.check(self.lib.ste_ukf_forward_loglik_f64(C.byref(s), C.byref(lk), self._stream(st)),
                              "ste_ukf_forward_loglik_f64")
            self._mark_use(st)
            return LogLikelihood(loglik=ll.cpu().numpy(), dof=dof.cpu().numpy(), nupd=nupd.cpu().numpy(),
                                 status=self.status.cpu().numpy(),
                                 nis=None if nis_t is None else nis_t.T.cpu().numpy())

    # -- measurement noise fitted to the data ("Noise fit") -------------------------------------------
    _NOISE_STRUCTURES = {"scalar": binding.STE_NOISE_FIT_SCALAR, "diag2": binding.STE_NOISE_FIT_DIAG2,
                         "block2": binding.STE_NOISE_FIT_BLOCK2}

    def measurement_moments(self, stream=None):
        """Per-track sums of the M-step for R (include/ste.h: ste_ukf_noise_moments_f64), from the forward pass and the
        smoother this batch holds: over a track's updates, the residual of the observation against the smoothed row the
        update produced, as v v^T + H P^s H^T.  Returns device tensors: ``moments`` (10, B) upper triangles, ``count`` (B,)
        int32, ``vsum`` (4, B) the summed residuals, ``track_status`` (B,) int32 STE_NOISE_TRACK_* bits; an unusable track
        (a NaN status, a non-finite term) has count 0 and zero sums.  For a window the tensors are views of rows as wide as
        the fleet's, which is what ``update_measurement_noise`` takes."""
        if self.sm_mean is None:
            raise ValueError("measurement_moments() needs the smoothed track, and this batch was built with alloc_smoothed=False")
        torch = self.torch
        st = self._ordered_stream(stream)
        B, ld, col = self.ntracks, int(self.struct.track_stride or self.struct.B), self.lo
        with torch.cuda.stream(st):
            nm = binding.SteNoiseMomentsF64()
            out = self._track_outputs(nm, ld, col, [("moments", (10,), torch.float64, 0), ("count", (), torch.int32, 0),
                                                    ("vsum", (4,), torch.float64, 0)])
            out["track_status"] = torch.zeros((B,), dtype=torch.int32, device=self.device)
            nm.track_status = out["track_status"].data_ptr()
            binding.check(self.lib.ste_ukf_noise_moments_f64(C.byref(self.struct), C.byref(nm), self._stream(st)),
                          "ste_ukf_noise_moments_f64")
            return self._finish(st, [], out)

    def update_measurement_noise(self, moments, groups=None, structure: str = "scalar", stream=None):
        """The M-step for R (include/ste.h: ste_ukf_noise_mstep_f64) into this batch's own per-track R: the sums of
        ``moments`` (what ``measurement_moments`` returned) over every group, in a fixed order, divided by the group's count,
        projected onto ``structure`` ("scalar", "diag2" or "block2") and stored for every member.  ``groups``: None -- every
        track a group of its own -- or ``(offsets, members)``, int32 CSR over this batch's slots (offsets (G + 1,), members
        (offsets[G],)), each slot in at most one group.  A group without updates or with an unusable variance keeps its R.
        The batch must carry an R stack (``with_track_noise``).  Returns device tensors ``R_group`` (10, G), ``n_group`` (G,),
        ``group_status`` (G,) STE_NOISE_GROUP_* bits.  The next ``forward`` / ``run`` / ``log_likelihood`` filters with the new R."""
        torch = self.torch
        if self.noise is None or not self.noise.R:
            raise ValueError("update_measurement_noise() writes the batch's per-track R: build the batch from "
                             "with_track_noise(hb, R=...) so that it carries one")
        if structure not in self._NOISE_STRUCTURES:
            raise ValueError(f"structure must be one of {sorted(self._NOISE_STRUCTURES)}, got {structure!r}")
        B, ld = self.ntracks, int(self.struct.track_stride or self.struct.B)
        mom, count = moments["moments"], moments["count"]
        if tuple(mom.shape) != (10, B) or tuple(count.shape) != (B,) or mom.stride() != (ld, 1) or mom.dtype != torch.float64 \
                or count.dtype != torch.int32 or count.stride() != (1,):
            raise ValueError(f"moments must be what measurement_moments() of this batch returned: moments (10, {B}) float64 in "
                             f"rows of {ld}, count ({B},) int32")
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            keep = [mom, count]
            if groups is None:
                G, nmem, off_p, mem_p = B, 0, None, None
            else:
                off, mem = (np.asarray(g) for g in groups)
                if off.dtype.kind not in "iu" or (mem.size and mem.dtype.kind not in "iu"):
                    raise ValueError("groups must be (offsets, members), two integer arrays")
                off, mem = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(mem, dtype=np.int32)
                if off.ndim != 1 or mem.ndim != 1 or off.size < 2 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != mem.size:
                    raise ValueError("groups must be (offsets, members): offsets (G + 1,) ascending from 0 to len(members)")
                if mem.size and (mem.min() < 0 or mem.max() >= B or np.unique(mem).size != mem.size):
                    raise ValueError(f"groups: members must be distinct slots in [0, {B})")
                G, nmem = off.size - 1, int(mem.size)
                off_t = torch.from_numpy(off).to(self.device)
                mem_t = torch.from_numpy(mem if mem.size else np.zeros(1, dtype=np.int32)).to(self.device)
                keep += [off_t, mem_t]
                off_p, mem_p = off_t.data_ptr(), mem_t.data_ptr()
            Rg = torch.empty((10, G), dtype=torch.float64, device=self.device)
            ng = torch.empty((G,), dtype=torch.int32, device=self.device)
            gs = torch.empty((G,), dtype=torch.int32, device=self.device)
            ms = binding.SteNoiseMstepF64(B, G, nmem, self._NOISE_STRUCTURES[structure], ld, mom.data_ptr(), count.data_ptr(),
                                          off_p, mem_p, Rg.data_ptr(), ng.data_ptr(), gs.data_ptr(), self.noise.R, 0)
            binding.check(self.lib.ste_ukf_noise_mstep_f64(C.byref(ms), self._stream(st)), "ste_ukf_noise_mstep_f64")
            if not self.noise.flags & binding.STE_NOISE_R_BLOCK2:
                # the promise covers every track, and a group that failed (or a slot in no group) keeps the R it had: look
                Rt = self.t["R_tracks"][:, self.lo:self.lo + B].cpu().numpy()
                if r_tracks_block2(Rt):
                    self.noise.flags |= binding.STE_NOISE_R_BLOCK2
            return self._finish(st, keep, dict(R_group=Rg, n_group=ng, group_status=gs))

    # -- posterior tracks ----------------------------------------------------------------------------------------
    def _sample_struct(self, samples, nsamples: int):
        """The ``ste_ukf_sample_f64`` of this batch (or window) for ``samples`` [S][N+1][4][ld], with a coefficient workspace
        and a status array of its own; returns (struct, status tensor, tensors to keep alive)."""
        torch = self.torch
        N, ld = int(self.struct.Nmax), int(self.struct.track_stride or self.struct.B)
        coef = torch.empty((N + 1, binding.STE_SAMPLE_COEF_ROWS, ld), dtype=torch.float64, device=self.device)
        status = torch.zeros((self.ntracks,), dtype=torch.int32, device=self.device)
        sm = binding.SteUkfSampleF64(int(nsamples), 0, column_pointer(samples, self.lo), column_pointer(coef, self.lo),
                                     status.data_ptr())
        return sm, status, (samples, coef)

    def sample_smoothed(self, nsamples: int, seed: int = 0, draws=None, stream=None):
        """``nsamples`` tracks drawn from the joint smoothing posterior (include/ste.h: ste_urtss_sample_f64), as a device
        tensor (S, Nmax+1, 4, B); rows past ``nsteps[b]`` hold whatever they held (the draws).  Needs a completed
        ``forward()`` of this batch; ``backward()`` may or may not have run.  ``draws``: a float64 device tensor of that
        shape with standard normal draws, consumed in place (it comes back holding the samples); None = ``torch.randn``
        from a ``torch.Generator`` on the batch's device seeded with ``seed``.  A window of a resident batch
        (``window(lo, hi)``) samples its own tracks, B = hi - lo; given columns [lo, hi) of the draws of a whole-batch call
        it returns the same bits as that call.  The sampler's status (STE_STATUS_* per track) is left in
        ``self.sample_status`` (a device tensor)."""
        torch = self.torch
        if self.rts_work is None:
            raise ValueError("sample_smoothed() draws tracks from the work rows the forward pass leaves for the smoother "
                             "(rts_work), and this batch has none: it was built with fuse_gains=False, histories=False or "
                             "alloc_smoothed=False")
        S, N, B = int(nsamples), int(self.struct.Nmax), self.ntracks
        if S < 1:
            raise ValueError(f"nsamples must be >= 1, got {nsamples!r}")
        ld = int(self.struct.track_stride or self.struct.B)
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            if draws is None:
                gen = torch.Generator(device=self.device)
                gen.manual_seed(int(seed))
                out = torch.randn((S, N + 1, 4, B), generator=gen, dtype=torch.float64, device=self.device)
            else:
                if tuple(draws.shape) != (S, N + 1, 4, B) or draws.dtype != torch.float64 or draws.device != self.device:
                    raise ValueError(f"draws must be a float64 tensor of shape {(S, N + 1, 4, B)} on {self.device}")
                out = draws
            if ld == B and self.lo == 0 and out.is_contiguous():
                full, view = out, out
            else:  # a window: rows of the fleet's width, this window's columns filled with its draws
                full = torch.empty((S, N + 1, 4, ld), dtype=torch.float64, device=self.device)
                view = full[..., self.lo:self.lo + B]
                view.copy_(out)
            sm, status, keep = self._sample_struct(full, S)
            noise = None if self.noise is None else C.byref(self.noise)
            binding.check(self.lib.ste_urtss_sample_f64(C.byref(self.struct), noise, C.byref(sm), self._stream(st)),
                          "ste_urtss_sample_f64")
            if view is not out:
                out.copy_(view)
            for ten in keep:
                ten.record_stream(st)
            self.sample_status = status
            self._mark_use(st)
        return out

    # -- lag-one covariance ---------------------------------------------------------------------------------------
    def lag_one_covariance(self, position_only: bool = False, stream=None):
        """The lag-one cross-covariance of the smoother, L_k = Cov(x_k, x_{k+1} | all data) = K_k P^s_{k+1} (include/ste.h:
        ste_urtss_lag_one_f64; DESIGN.md, "Lag-one covariance"), as a device tensor (Nmax, 16, B): entry 4 r + c of row k is
        L_k[r][c].  ``position_only``: (Nmax, 4, B), the entries L[0][0], L[0][1], L[1][0], L[1][1] -- what the covariance of a
        position needs, with the same bits.  Rows k >= ``nsteps[b]`` hold zeros.  Needs a completed ``run()`` of this batch (the
        forward pass's work rows and the smoothed covariances); the batch is only read.  Returns ``(lag1, status)``, status
        (B,) int32 on the device: STE_STATUS_* bits of the gain solve and STE_STATUS_NAN for a non-finite entry.  A window of a
        resident batch computes its own tracks."""
        torch = self.torch
        if self.rts_work is None:
            raise ValueError("lag_one_covariance() forms the smoother gains from the work rows the forward pass leaves for the "
                             "smoother (rts_work), and this batch has none: it was built with fuse_gains=False, "
                             "histories=False or alloc_smoothed=False")
        N, B = int(self.struct.Nmax), self.ntracks
        ld = int(self.struct.track_stride or self.struct.B)
        rows = binding.STE_LAG1_POSITION_ROWS if position_only else binding.STE_LAG1_ROWS
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            full = torch.zeros((N, rows, ld), dtype=torch.float64, device=self.device)
            status = torch.zeros((B,), dtype=torch.int32, device=self.device)
            lg = binding.SteLagOneF64(column_pointer(full, self.lo), status.data_ptr(),
                                      binding.STE_LAG1_POSITION if position_only else 0, 0)
            noise = None if self.noise is None else C.byref(self.noise)
            binding.check(self.lib.ste_urtss_lag_one_f64(C.byref(self.struct), noise, C.byref(lg), self._stream(st)),
                          "ste_urtss_lag_one_f64")
            out = self._finish(st, [full], {"lag1": full[..., self.lo:self.lo + B] if ld != B else full, "status": status})
        return out["lag1"], out["status"]

    def position_covariance_at(self, qtrack, qtime, t0=None, lag_one=None, knots=None, full: bool = False, sort: bool = True,
                               stream=None):
        """The exact covariance of the smoothed position at given clock times, without samples (include/ste.h:
        ste_track_position_cov_f64; DESIGN.md, "Lag-one covariance"): ``positions_at`` interpolates linearly inside a step, so
        at fraction u of step k the covariance is (1-u)^2 P^s_k + u^2 P^s_{k+1} + (1-u) u (L_k + L_k^T), with P^s this batch's
        ``sm_cov`` and L its lag-one covariance.  ``qtrack``, ``qtime``, ``t0``, ``sort`` and ``stream`` as in ``positions_at``.
        ``lag_one``: what ``lag_one_covariance`` returned, in either form (``full`` needs the 16-entry one); None computes it
        (the position form unless ``full``).  ``knots``: what ``positions_at`` or ``track_knots`` returned; None sums them.
        Returns a dict of device tensors: ``pcov`` (3, Q) -- lon-lon, lon-lat, lat-lat in degrees squared -- or with ``full``
        (10, Q), the upper triangle of the 4 x 4 (00 01 02 03 11 12 13 22 23 33); a knot hit gives that row of ``sm_cov``, a
        query that is not located NaN.  ``step``, ``frac``, ``status`` as in ``positions_at``; ``lag_one`` and ``knots`` to pass
        back in; ``lag_status`` (B,) when the lag-one covariance was computed here.  Where the sampler clamps a negative
        eigenvalue of a conditional covariance (STE_STATUS_CLAMPED) its ensemble departs from ``sm_cov``; this follows
        ``sm_cov``."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        if self.sm_cov is None:
            raise ValueError("position_covariance_at() reads the smoothed covariances, and this batch was built with "
                             "alloc_smoothed=False")
        qtrack = _index_tensor(qtrack, "qtrack", (), binding.STE_POSITIONS_MAX_QUERIES)
        Q = int(qtrack.shape[0])
        qtime = torch.as_tensor(qtime, dtype=torch.float64)
        if tuple(qtime.shape) != (Q,):
            raise ValueError(f"qtime must have shape ({Q},) like qtrack, got {tuple(qtime.shape)}")
        if knots is not None and not (isinstance(knots, torch.Tensor) and knots.dtype == torch.float64 and knots.device == self.device
                                      and tuple(knots.shape) == (N + 1, B)):
            raise ValueError(f"knots must be the float64 ({N + 1}, {B}) tensor a previous call on this batch returned")
        lag_rows = (binding.STE_LAG1_ROWS, binding.STE_LAG1_POSITION_ROWS)
        if lag_one is not None and not (isinstance(lag_one, torch.Tensor) and lag_one.dtype == torch.float64
                                        and lag_one.device == self.device and lag_one.dim() == 3
                                        and (lag_one.shape[0], lag_one.shape[2]) == (N, B) and lag_one.shape[1] in lag_rows):
            raise ValueError(f"lag_one must be the float64 ({N}, 16 or 4, {B}) tensor lag_one_covariance() returned")
        if full and lag_one is not None and lag_one.shape[1] != binding.STE_LAG1_ROWS:
            raise ValueError("full=True needs the 16-entry lag-one covariance (lag_one_covariance(position_only=False))")
        ld = int(self.struct.track_stride or self.struct.B)
        lag_status = None
        if lag_one is None:
            lag_one, lag_status = self.lag_one_covariance(position_only=not full, stream=stream)
        if knots is None:
            knots = self.track_knots(stream=stream)
        st = self._ordered_stream(stream)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        with torch.cuda.stream(st):
            qt = _index_int32(qtrack.to(self.device))
            tq = qtime.to(self.device).contiguous()
            perm = None
            if sort and Q > 1:
                by_time = torch.sort(tq, stable=True).indices
                perm = by_time[torch.sort(qt[by_time], stable=True).indices]
                qt, tq = qt[perm].contiguous(), tq[perm].contiguous()
            keep = [qt, tq, self.sm_cov]
            pc = binding.StePositionCovF64()
            rows = int(lag_one.shape[1])
            pc.flags = (binding.STE_PCOV_FULL if full else 0) | (binding.STE_PCOV_LAG1_POSITION if rows == lag_rows[1] else 0)
            pc.nqueries, pc.qtrack, pc.qtime = Q, qt.data_ptr(), tq.data_ptr()
            pc.t0 = self._track_clock(t0, ld, self.lo, keep)
            # knots and lag1 are read in rows of this batch's track_stride, at the window's first column: in place when that
            # is how the tensor lies (what track_knots / lag_one_covariance return), else through a copy of that shape
            if knots.stride() == (ld, 1):
                pc.knots = knots.data_ptr()
            else:
                ws = torch.empty((N + 1, ld), **f64)
                ws[:, self.lo:self.lo + B].copy_(knots)
                pc.knots = column_pointer(ws, self.lo)
                keep.append(ws)
            if N == 0 or lag_one.stride() == (rows * ld, ld, 1):
                pc.lag1 = lag_one.data_ptr() if N > 0 else None
            else:
                lw = torch.empty((N, rows, ld), **f64)
                lw[..., self.lo:self.lo + B].copy_(lag_one)
                pc.lag1 = column_pointer(lw, self.lo)
                keep.append(lw)
            keep += [knots, lag_one]
            pc.cov = self.struct.sm_cov
            out = {"pcov": torch.empty((10 if full else 3, Q), **f64), "step": torch.empty((Q,), **i32),
                   "frac": torch.empty((Q,), **f64), "status": torch.empty((Q,), **i32)}
            for k, ten in out.items():
                setattr(pc, k, ten.data_ptr())
            binding.check(self.lib.ste_track_position_cov_f64(C.byref(self.struct), C.byref(pc), self._stream(st)),
                          "ste_track_position_cov_f64")
            if perm is not None:  # back to the caller's order
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(Q, device=self.device)
                out = {k: v[..., inv].contiguous() for k, v in out.items()}
                keep += [perm, inv]
            out["knots"], out["lag_one"] = knots, lag_one
            if lag_status is not None:
                out["lag_status"] = lag_status
            return self._finish(st, keep, out)

    # -- path quantities ------------------------------------------------------------------------------------------
    def path_metrics(self, states, model: str = "sphere", cumulative: bool = False, line_axis=None, line_value=None,
                     stream=None):
        """Distance sailed and, given a line, the time of its first crossing, for tracks that are on the device
        (include/ste.h: ste_path_metrics_f64; DESIGN.md, "Path quantities").  ``states``: a float64 device tensor
        (S, Nmax+1, 4, B) or (Nmax+1, 4, B) -- what ``sample_smoothed`` returned, ``self.sm_mean``, ``self.fwd_mean`` -- of which
        rows 0 .. nsteps[b] of components 0 (lon) and 1 (lat) are read.  ``model``: "sphere" (haversine, 6378.137 km) or
        "wgs84" (Karney's inverse geodesic), the leg functions of ``prepare_observations``.  ``line_axis``: "lon" (a
        meridian) or "lat" (a parallel) at ``line_value`` degrees, a scalar or one value per track ((B,) array or tensor).
        Returns a dict of device tensors: ``distance`` (S, B) in km; with ``cumulative`` also ``cumulative`` (S, Nmax+1, B),
        row k = the first k legs, NaN past ``nsteps[b]``; with a line ``cross_time`` (S, B), hours from row 0 to the first
        crossing, NaN where the track never crosses, and ``ncross`` (S, B) int32, the number of crossing steps.
        A window of a resident batch (``window(lo, hi)``) takes its own tracks, B = hi - lo; a tensor that already is a view
        of the fleet's full-width rows (``window.sm_mean``) is read in place, anything else is made contiguous first.  Every
        value depends on its own track's rows alone, so a window, a slice of the samples or a call without the line give the
        same bits.  ``stream`` is ordered as in ``sample_smoothed``."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        if line_axis is not None and line_axis not in self._PATH_AXES:
            raise ValueError(f"line_axis must be None, 'lon' or 'lat', got {line_axis!r}")
        if (line_axis is None) != (line_value is None):
            raise ValueError("line_axis and line_value go together: a line is an axis ('lon' / 'lat') and its value in degrees")
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            keep = []
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=line_axis is not None)
            pm = binding.StePathF64()
            pm.nstates, pm.model, pm.states = S, model_id, states.data_ptr()
            pm.line_axis, pm.reserved = -1, 0
            spec = [("dist", (S,), f64, None)] + ([("cumdist", (S, N + 1), f64, float("nan"))] if cumulative else [])
            out = self._track_outputs(pm, width, col, spec)
            if line_axis is not None:
                pm.line_axis = self._PATH_AXES[line_axis]
                pm.line_value = track_input(line_value, B, width, col, keep, self.device,
                                            f"line_value must be a scalar or have shape ({B},)")
                out.update(self._track_outputs(pm, width, col, [("cross_time", (S,), f64, None), ("ncross", (S,), i32, None)]))
            binding.check(self.lib.ste_path_metrics_f64(C.byref(s), C.byref(pm), self._stream(st)), "ste_path_metrics_f64")
            names = {"dist": "distance", "cumdist": "cumulative"}
            return self._finish(st, keep, {names.get(k, k): ten for k, ten in out.items()})

    # -- regions --------------------------------------------------------------------------------------------------
    def region_metrics(self, states, polygon, model: str = "sphere", distance: bool = False, mask: bool = False, stream=None):
        """Tracks that are on the device against a polygon (include/ste.h: ste_region_metrics_f64; DESIGN.md, "Regions"):
        time inside, first entry, entries.  ``states`` as in ``path_metrics``.  ``polygon``: a (V, 2) array of lon / lat in
        degrees, planar as in GeoJSON, or what ``region_polygon`` made of one; a repeated closing vertex is dropped, a
        clockwise ring reversed and the longitudes unwrapped (``region_polygon`` has the rules and the refusals).  Returns a
        dict of device tensors: ``time_inside`` (S, B) in hours; ``first_entry`` (S, B), hours from row 0 to the first entry,
        0 for a track that starts inside, NaN for one that never is inside; ``nenter`` (S, B) int32, the number of entries;
        ``nbroken`` (S, B) int32, the steps left out because they have a NaN latitude or span 90 degrees of longitude or more;
        with ``distance`` also ``dist_inside`` (S, B), km sailed inside under ``model`` ("sphere" or "wgs84", the legs of
        ``path_metrics``); with ``mask`` also ``inside`` (S, Nmax+1, B) uint8, 1 where the row is inside, 0 past ``nsteps[b]``.
        Windows, in-place views and ``stream`` as in ``path_metrics``; every value depends on its own track's rows and the
        polygon alone."""
        torch = self.torch
        N = int(self.struct.Nmax)
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        poly = polygon if isinstance(polygon, RegionPolygon) else region_polygon(polygon)
        V = int(poly.vert.shape[1])
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            vert = torch.from_numpy(poly.vert).to(self.device)
            keep = [vert]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            rg = binding.SteRegionF64()
            rg.nstates, rg.model, rg.states = S, model_id, states.data_ptr()
            rg.nvert, rg.reserved, rg.vert, rg.lon_ref = V, 0, vert.data_ptr(), float(poly.lon_ref)
            spec = [("time_inside", (S,), f64, None), ("first_entry", (S,), f64, None), ("nenter", (S,), i32, None),
                    ("nbroken", (S,), i32, None)]
            spec += [("dist_inside", (S,), f64, None)] if distance else []
            spec += [("inside", (S, N + 1), torch.uint8, 0)] if mask else []
            out = self._track_outputs(rg, width, col, spec)
            binding.check(self.lib.ste_region_metrics_f64(C.byref(s), C.byref(rg), self._stream(st)), "ste_region_metrics_f64")
            return self._finish(st, keep, out)

    # -- grids ----------------------------------------------------------------------------------------------------
    def grid_metrics(self, states, grid, entries: bool = False, out=None, stream=None):
        """Tracks that are on the device on a regular lon / lat grid (include/ste.h: ste_grid_metrics_f64; DESIGN.md, "Grids"):
        the time spent in every cell, summed over all tracks of the call, in exact integer ticks of 2^-20 h.  ``states`` as in
        ``path_metrics``; ``grid`` a ``TrackGrid`` (``track_grid`` makes one).  Returns a dict of device tensors: ``ticks``
        (ny, nx) int64; ``hours`` = ticks / 2^20 as float64; with ``entries`` also ``entries`` (ny, nx) int64, the number of
        runs of a track in the cell; ``outside`` and ``total`` (S, B) int64, the ticks of a track's sound steps spent off the
        grid and altogether; ``nbroken`` (S, B) int32, the steps left out (a non-finite latitude, 90 degrees of longitude or
        more in one step, a negative or non-finite dt).  ``out``: a previous result whose ``ticks`` (and ``entries``) this call
        adds to, so that windows and sample chunks sum into one grid; otherwise fresh zeroed tensors.  The sums are integers:
        the grid's bits do not depend on how the tracks were split into calls.  Windows, in-place views and ``stream`` as in
        ``path_metrics``."""
        torch = self.torch
        states, S = self._metric_states(states)
        if not isinstance(grid, TrackGrid):
            raise ValueError("grid must be a TrackGrid (track_estimators.batch.track_grid makes one)")
        nx, ny = grid.nx, grid.ny
        i64 = dict(dtype=torch.int64, device=self.device)
        if out is not None:
            ticks, ent = out.get("ticks"), out.get("entries")
            for name, ten in (("ticks", ticks),) + ((("entries", ent),) if entries else ()):
                if (not isinstance(ten, torch.Tensor) or ten.dtype != torch.int64 or ten.device != self.device
                        or tuple(ten.shape) != (ny, nx) or not ten.is_contiguous()):
                    raise ValueError(f"out[{name!r}] must be a contiguous int64 tensor of shape ({ny}, {nx}) on {self.device}")
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            if out is None:
                ticks = torch.zeros((ny, nx), **i64)
                ent = torch.zeros((ny, nx), **i64) if entries else None
            elif not entries:
                ent = None
            keep = [ticks] + ([ent] if ent is not None else [])
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            g = binding.SteGridF64()
            g.nstates, g.flags, g.states = S, binding.STE_GRID_PERIODIC_LON if grid.periodic else 0, states.data_ptr()
            g.nx, g.ny, g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref = nx, ny, grid.lon0, grid.lat0, grid.dlon, grid.dlat, grid.lon_ref
            g.ticks, g.entries = ticks.data_ptr(), None if ent is None else ent.data_ptr()
            per_track = self._track_outputs(g, width, col, [("outside", (S,), torch.int64, 0), ("total", (S,), torch.int64, 0),
                                                            ("nbroken", (S,), torch.int32, 0)])
            binding.check(self.lib.ste_grid_metrics_f64(C.byref(s), C.byref(g), self._stream(st)), "ste_grid_metrics_f64")
            res = {"ticks": ticks, "hours": ticks.to(torch.float64) / float(binding.STE_GRID_TICKS_PER_HOUR), **per_track}
            if ent is not None:
                res["entries"] = ent
            return self._finish(st, keep, res)

    # -- rasters --------------------------------------------------------------------------------------------------
    def raster_metrics(self, states, raster, threshold=None, below: bool = False, min_hours: float = 0.0, rows: bool = False,
                       stream=None):
        """Tracks that are on the device against a gridded field (include/ste.h: ste_raster_metrics_f64; DESIGN.md,
        "Rasters"): a land mask, a depth, a density, one value per cell of a ``TrackGrid``, NaN = no data.  ``states`` as in
        ``path_metrics``; ``raster`` a ``TrackRaster`` (``track_raster`` makes one) on this batch's device.  Time is counted in
        the integer ticks of ``grid_metrics`` (2^-20 h), over the same pieces and runs.  Returns a dict of device tensors,
        (S, B) each: ``total``, ``outside`` int64 and ``nbroken`` int32 as in ``grid_metrics``; ``valid`` and ``nodata`` int64,
        the ticks in cells with and without a value (valid + nodata + outside = total); ``wsum``, the sum of ticks x value over
        the track's runs, and ``mean`` = wsum / valid, NaN where valid is 0; ``vmin``, ``vmax`` and ``tmin``, ``tmax`` int64, the
        extremes and the tick at which the first run that attains them starts (NaN and -1 without a valid run).  With
        ``threshold`` a run is a hit when its value is >= ``threshold`` (<= with ``below``), an excursion is a stretch of
        consecutive hits, and the dict also has ``hit_ticks``, ``hit_first`` (-1 = never), ``hit_longest`` int64, ``nhit`` and
        ``nhit_long`` int32, the excursions and those of at least ``min_hours`` (``min_ticks`` = rint(min_hours 2^20)).
        Hours = ticks / 2^20: ``valid_hours``, ``tmin_hours``, ``tmax_hours``, ``hit_hours``, ``hit_first_hours``,
        ``hit_longest_hours``, NaN where the tick is -1.  With ``rows`` also ``row_value`` (S, Nmax+1, B), the value of the cell
        each row lies in, NaN off the grid and past ``nsteps[b]``.  Windows, in-place views and ``stream`` as in
        ``grid_metrics``; every value depends on its own track's rows and the raster alone."""
        torch = self.torch
        N = int(self.struct.Nmax)
        states, S = self._metric_states(states)
        if not isinstance(raster, TrackRaster):
            raise ValueError("raster must be a TrackRaster (track_estimators.batch.track_raster makes one)")
        if raster.values.device != self.device:
            raise ValueError(f"the raster's values are on {raster.values.device}, this batch is on {self.device}")
        flags, thr, min_ticks = _raster_threshold(threshold, below, min_hours)
        grid = raster.grid
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            keep = [raster.values]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            r = binding.SteRasterF64()
            r.nstates, r.states = S, states.data_ptr()
            r.flags = flags | (binding.STE_GRID_PERIODIC_LON if grid.periodic else 0)
            r.nx, r.ny, r.lon0, r.lat0, r.dlon, r.dlat, r.lon_ref = (grid.nx, grid.ny, grid.lon0, grid.lat0, grid.dlon, grid.dlat,
                                                                     grid.lon_ref)
            r.values, r.threshold, r.min_ticks = raster.values.data_ptr(), thr, min_ticks
            names = _RASTER_OUTPUTS + (_RASTER_HIT_OUTPUTS if threshold is not None else ())
            spec = [(k, (S,), getattr(torch, dt), None) for k, dt in names]
            spec += [("row_value", (S, N + 1), torch.float64, float("nan"))] if rows else []
            out = self._track_outputs(r, width, col, spec)
            binding.check(self.lib.ste_raster_metrics_f64(C.byref(s), C.byref(r), self._stream(st)), "ste_raster_metrics_f64")
            tph = float(binding.STE_GRID_TICKS_PER_HOUR)
            nan = torch.full((), float("nan"), dtype=torch.float64, device=self.device)
            hours = {"valid": "valid_hours", "tmin": "tmin_hours", "tmax": "tmax_hours", "hit_ticks": "hit_hours",
                     "hit_first": "hit_first_hours", "hit_longest": "hit_longest_hours"}
            for k, name in hours.items():
                if k in out:
                    out[name] = torch.where(out[k] < 0, nan, out[k].to(torch.float64) / tph)
            out["mean"] = torch.where(out["valid"] > 0, out["wsum"] / out["valid"].to(torch.float64), nan)
            if rows:
                out["row_value"] = out.pop("row_value")  # after the derived values, where it always was
            return self._finish(st, keep, out)

    # -- encounters -----------------------------------------------------------------------------------------------
    def encounter_metrics(self, states, pairs, radius_km, t0=None, model: str = "sphere", stream=None):
        """Pairs of tracks that are on the device against each other (include/ste.h: ste_encounter_metrics_f64; DESIGN.md,
        "Encounters"): closest approach and time within ``radius_km``.  ``states`` as in ``path_metrics``; sample s of one
        ship is held against sample s of the other.  ``pairs``: a (P, 2) integer array or device tensor of track indices
        (i, j) of this batch (of this window, counted from its first track); only its shape and dtype are checked here, an
        index outside [0, B) comes back as STE_ENC_BAD_INDEX in ``status``.  ``t0``: the clock time of row 0 in hours, None
        (0 for every track), a scalar or one value per track ((B,) array or tensor); every track's clock then runs on its own
        ``dt``.  ``model``: the leg function of ``min_dist``, "sphere" or "wgs84".  Returns a dict of device tensors, (S, P)
        each: ``min_dist`` in km, NaN where the two clocks share no sound time; ``min_time``, its clock time; ``time_within``,
        hours with the planar distance <= ``radius_km``; ``first_within``, the clock time the first such run starts, NaN =
        never; ``nwithin`` int32, the number of runs; ``overlap``, the hours of common clock time examined; ``nbroken`` int32,
        the pieces left out (a NaN latitude, or 90 degrees of longitude or more in one step); and ``status`` (P,) int32,
        STE_ENC_BAD_INDEX / STE_ENC_BAD_TIME (a non-finite ``t0``, a ``dt`` that is not finite and >= 0).  The geometry of the
        search is planar in (lon, lat): it is meant for ships close together (``radius_km`` <= 1000).  Windows, in-place
        views and ``stream`` as in ``path_metrics``; every value depends on the two tracks' rows, ``dt``, ``t0`` and the
        radius alone."""
        torch = self.torch
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        radius_km = float(radius_km)
        if not (np.isfinite(radius_km) and 0.0 <= radius_km <= binding.STE_ENCOUNTER_MAX_RADIUS_KM):
            raise ValueError(f"radius_km must be finite and between 0 and {binding.STE_ENCOUNTER_MAX_RADIUS_KM:g}, got {radius_km!r}")
        pairs = _index_tensor(pairs, "pairs", (2,), binding.STE_ENCOUNTER_MAX_PAIRS)
        P = int(pairs.shape[0])
        st = self._ordered_stream(stream)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        with torch.cuda.stream(st):
            pr = _index_int32(pairs.to(self.device))
            keep = [pr]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            en = binding.SteEncounterF64()
            en.nstates, en.model, en.states = S, model_id, states.data_ptr()
            en.npairs, en.pairs, en.radius_km, en.flags, en.reserved = P, pr.data_ptr(), radius_km, 0, 0
            en.t0 = self._track_clock(t0, width, col, keep)
            out = {k: torch.empty((S, P), **f64) for k in ("min_dist", "min_time", "time_within", "first_within", "overlap")}
            out.update({k: torch.empty((S, P), **i32) for k in ("nwithin", "nbroken")})
            out["status"] = torch.empty((P,), **i32)
            for k, ten in out.items():
                setattr(en, k, ten.data_ptr())
            binding.check(self.lib.ste_encounter_metrics_f64(C.byref(s), C.byref(en), self._stream(st)),
                          "ste_encounter_metrics_f64")
            return self._finish(st, keep, out)

    # -- candidate pairs for encounters -----------------------------------------------------------------------------
    def _clock_range(self, t0):
        """(earliest start, latest end) in hours over the tracks of this batch whose clock is sound (a finite ``t0``, every
        ``dt`` of its steps finite and >= 0), as two floats: one host read.  None when no track has one.  Inside the stream
        context."""
        torch, B, N = self.torch, self.ntracks, int(self.struct.Nmax)
        ns = self.t["nsteps"][self.lo:self.lo + B].to(torch.int64).clamp(0, N)
        dt = self.t["dt"][:, self.lo:self.lo + B]
        live = torch.arange(N, device=self.device)[:, None] < ns[None, :]
        d = torch.where(live, dt, torch.zeros_like(dt))
        if t0 is None:
            start = torch.zeros((B,), dtype=torch.float64, device=self.device)
        else:
            start = torch.as_tensor(t0, dtype=torch.float64).to(self.device).expand(B)
        end = start + d.sum(dim=0)
        sound = torch.isfinite(start) & torch.isfinite(end) & (torch.isfinite(d) & (d >= 0.0)).all(dim=0)
        inf = torch.full_like(start, float("inf"))
        first, last = (float(v) for v in torch.stack([torch.where(sound, start, inf).min(),
                                                      torch.where(sound, end, -inf).max()]).cpu())
        return (first, last) if first <= last else None

    def encounter_candidates(self, reach_km, window_h, states=None, t0=None, time0=None, nwindows=None, track_margin_km=None,
                             details: bool = False, stream=None):
        """The pairs of this batch worth giving to ``encounter_metrics``, found on the device (include/ste.h: CANDIDATES,
        ste_encounter_candidates_mask_f64 / _list_f64; DESIGN.md, "Candidates"): an int32 (P, 2) device tensor of (i, j),
        i < j, sorted by (i, j), of the tracks that can have been within ``reach_km`` of each other at one instant.  The clock
        is cut into ``nwindows`` windows of ``window_h`` hours from ``time0``; a track gets a box around its rows per window,
        and a pair is kept when two boxes of one window are closer than the reach.  Every pair that ``encounter_metrics``
        on these ``states`` brings within ``reach_km`` (true distance) is in the list, whatever the windows; smaller windows
        prune more and cost more.  ``states``: ONE state set, (Nmax+1, 4, B) or (1, Nmax+1, 4, B); None = ``sm_mean``, else
        ``fwd_mean``.  A list for several samples is not built: widen ``reach_km`` or give ``track_margin_km`` (None, a scalar
        or one value per track, km, added to the reach of every pair the track is in; ``batch.position_spread_km``).  ``t0``
        as in ``encounter_metrics``.  ``time0`` / ``nwindows`` None: the earliest start and the latest end over the sound
        clocks, found on the device (one host read); times outside the windows are merged into the edge windows, never
        lost.  Between the two kernels' calls the number of pairs is read on the host (it sizes the result).  Returns
        ``pairs``; with ``details`` a dict of ``pairs``, ``wfirst`` and ``nwin`` (P,) int32 -- the first window in which
        the pair is near and the number of such windows: it can only be within reach inside those -- ``track_status`` (B,)
        int32 with the STE_CAND_* bits, and the ``time0``, ``window_h`` and ``nwindows`` used."""
        torch = self.torch
        if states is None:
            states = self.sm_mean if self.sm_mean is not None else self.fwd_mean
            if states is None:
                raise ValueError("encounter_candidates() needs states, sm_mean or fwd_mean, and this batch was built without histories")
        states, S = self._metric_states(states)
        if S != 1:
            raise ValueError(f"encounter_candidates() takes one state set, got S = {S}: a list for several samples is not built "
                             "(widen reach_km or give track_margin_km)")
        reach_km, window_h = float(reach_km), float(window_h)
        if not (np.isfinite(reach_km) and 0.0 <= reach_km <= binding.STE_CANDIDATES_MAX_REACH_KM):
            raise ValueError(f"reach_km must be finite and between 0 and {binding.STE_CANDIDATES_MAX_REACH_KM:g}, got {reach_km!r}")
        if not (np.isfinite(window_h) and window_h > 0.0):
            raise ValueError(f"window_h must be finite and > 0, got {window_h!r}")
        B, top = self.ntracks, binding.STE_CANDIDATES_MAX_WINDOWS
        if B > binding.STE_CANDIDATES_MAX_TRACKS:
            raise ValueError(f"encounter_candidates() takes at most {binding.STE_CANDIDATES_MAX_TRACKS} tracks, got {B}")
        if time0 is not None and not np.isfinite(float(time0)):
            raise ValueError(f"time0 must be finite, got {time0!r}")
        if nwindows is not None and not 1 <= int(nwindows) <= top:
            raise ValueError(f"nwindows must be between 1 and {top}, got {nwindows!r}")
        st = self._ordered_stream(stream)
        i32 = dict(dtype=torch.int32, device=self.device)
        with torch.cuda.stream(st):
            if time0 is None or nwindows is None:
                span = self._clock_range(t0)
                first, last = span if span is not None else (0.0, 0.0)
                time0 = first if time0 is None else float(time0)
                if nwindows is None:
                    count = max(np.floor((last - time0) / window_h), 0.0) + 1.0
                    if count > top:
                        raise ValueError(f"{last - time0:g} hours of clock in windows of {window_h:g} h are {count:.0f} windows, "
                                         f"above STE_CANDIDATES_MAX_WINDOWS = {top}: window_h >= {(last - time0) / (top - 1):.6g} "
                                         "would fit (or give time0 and nwindows)")
                    nwindows = int(count)
            time0, nwindows = float(time0), int(nwindows)
            keep = []
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            cd = binding.SteCandidatesF64()
            cd.states, cd.reach_km, cd.time0, cd.window_h, cd.nwindows = states.data_ptr(), reach_km, time0, window_h, nwindows
            cd.flags, cd.reserved = 0, 0
            cd.t0 = self._track_clock(t0, width, col, keep)
            cd.track_margin_km = self._track_clock(track_margin_km, width, col, keep, name="track_margin_km")
            nbytes = int(self.lib.ste_encounter_candidates_workspace(B, nwindows))
            work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=self.device)
            out = {"track_status": torch.empty((B,), **i32)}
            cd.workspace, cd.workspace_bytes, cd.track_status = work.data_ptr(), 8 * work.numel(), out["track_status"].data_ptr()
            binding.check(self.lib.ste_encounter_candidates_mask_f64(C.byref(s), C.byref(cd), self._stream(st)),
                          "ste_encounter_candidates_mask_f64")
            at = 2 * (7 * nwindows * B + B * ((B + 63) // 64)) + 2 * B  # count[B], after boxes, mask, wlo and whi (include/ste.h)
            counts = work.view(torch.int32)[at:at + B]
            ends = torch.cumsum(counts, dim=0, dtype=torch.int64)
            P = int(ends[-1])  # the one host read: it sizes the result
            if P > binding.STE_ENCOUNTER_MAX_PAIRS:
                raise ValueError(f"{P} candidate pairs, above STE_ENCOUNTER_MAX_PAIRS = {binding.STE_ENCOUNTER_MAX_PAIRS}: "
                                 "use smaller windows, a smaller reach, or a window of the fleet")
            out["pairs"] = torch.empty((P, 2), **i32)
            if details:
                out["wfirst"], out["nwin"] = torch.empty((P,), **i32), torch.empty((P,), **i32)
            if P > 0:
                offsets = ends - counts
                keep.append(offsets)
                cd.row_offset, cd.npairs, cd.pairs = offsets.data_ptr(), P, out["pairs"].data_ptr()
                if details:
                    cd.wfirst, cd.nwin = out["wfirst"].data_ptr(), out["nwin"].data_ptr()
                binding.check(self.lib.ste_encounter_candidates_list_f64(C.byref(s), C.byref(cd), self._stream(st)),
                              "ste_encounter_candidates_list_f64")
            keep.append(work)
            self._finish(st, keep, out)
            if not details:
                return out["pairs"]
            return dict(out, time0=time0, window_h=window_h, nwindows=nwindows)

    # -- positions at query times ---------------------------------------------------------------------------------
    def positions_at(self, states, qtrack, qtime, t0=None, velocity: bool = False, anchor=None, accumulate=None, knots=None,
                     stream=None, sort: bool = True):
        """Where tracks that are on the device were at given clock times (include/ste.h: ste_track_positions_f64; DESIGN.md,
        "Positions").  ``states`` as in ``path_metrics``.  ``qtrack``: (Q,) integer array or device tensor of track indices of
        this batch (of this window, counted from its first track); ``qtime``: (Q,) clock times in hours.  ``t0`` as in
        ``encounter_metrics``: the clock time of row 0, None (0), a scalar or one value per track.  A position is linear in time
        inside a step and a query at a knot returns that row; nothing is extrapolated.  Returns a dict of device tensors:
        ``lon``, ``lat`` (S, Q) and with ``velocity`` also ``speed``, ``heading`` (S, Q), NaN where the query is not located or
        its step is broken; ``step`` (Q,) int32, the row of a knot hit or the step, -1 = not located; ``frac`` (Q,), the
        fraction of the step, 0 on a knot hit; ``status`` (Q,) int32, STE_POS_BAD_INDEX / STE_POS_BAD_TIME / STE_POS_OUTSIDE;
        and ``knots`` (Nmax+1, B), the knot times the call summed from ``dt``: passed back in as ``knots=`` they are reused
        (STE_POS_REUSE_KNOTS) instead of summed again.  With ``anchor``, a (2, Q) array or tensor of lon / lat degrees, also
        ``count`` (Q,) int32 and ``moments`` (5, Q): the number of samples with a finite position and the sums over the samples
        of dx, dy, dx dx, dx dy, dy dy, dx = wrap180(lon - anchor lon), dy = lat - anchor lat, in degrees.  They start from zero,
        or with ``accumulate=(count, moments)`` from those two tensors, which are updated in place and returned: S samples in
        one call and the same samples in several calls give the same bits.  The queries are sorted by (track, time) for the
        kernel (lanes that share a track share cache lines) and the outputs come back in the caller's order; ``sort=False``
        takes the list as it is.  No value depends on the order.  Windows, in-place views and ``stream`` as in ``path_metrics``."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        states, S = self._metric_states(states)
        qtrack = _index_tensor(qtrack, "qtrack", (), binding.STE_POSITIONS_MAX_QUERIES)
        Q = int(qtrack.shape[0])
        qtime = torch.as_tensor(qtime, dtype=torch.float64)
        if tuple(qtime.shape) != (Q,):
            raise ValueError(f"qtime must have shape ({Q},) like qtrack, got {tuple(qtime.shape)}")
        if anchor is not None:
            anchor = torch.as_tensor(anchor, dtype=torch.float64)
            if tuple(anchor.shape) != (2, Q):
                raise ValueError(f"anchor must have shape (2, {Q}): lon and lat per query, got {tuple(anchor.shape)}")
        if accumulate is not None:
            if anchor is None:
                raise ValueError("accumulate continues the moments about an anchor: give the anchor they were started with")
            count, moments = accumulate
            ok = (isinstance(count, torch.Tensor) and isinstance(moments, torch.Tensor) and count.device == self.device
                  and moments.device == self.device and count.dtype == torch.int32 and moments.dtype == torch.float64
                  and tuple(count.shape) == (Q,) and tuple(moments.shape) == (5, Q))
            if not ok:
                raise ValueError(f"accumulate must be (count, moments): an int32 ({Q},) and a float64 (5, {Q}) tensor on {self.device}")
        if knots is not None and not (isinstance(knots, torch.Tensor) and knots.dtype == torch.float64 and knots.device == self.device
                                      and tuple(knots.shape) == (N + 1, B)):
            raise ValueError(f"knots must be the float64 ({N + 1}, {B}) tensor a previous call on this batch returned")
        st = self._ordered_stream(stream)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        with torch.cuda.stream(st):
            qt = _index_int32(qtrack.to(self.device))
            tq = qtime.to(self.device).contiguous()
            perm = None
            if sort and Q > 1:
                by_time = torch.sort(tq, stable=True).indices
                perm = by_time[torch.sort(qt[by_time], stable=True).indices]
                qt, tq = qt[perm].contiguous(), tq[perm].contiguous()
            keep = [qt, tq]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=knots is None)  # given knots, dt is not read
            po = binding.StePositionsF64()
            po.nstates, po.flags, po.states = S, 0, states.data_ptr()
            po.nqueries, po.qtrack, po.qtime = Q, qt.data_ptr(), tq.data_ptr()
            po.t0 = self._track_clock(t0, width, col, keep)
            if knots is not None and knots.stride() == (width, 1):
                kn = knots  # the view a call of the same kind returned: read where it lies
                po.knots = kn.data_ptr()
            else:
                kn = self._track_outputs(po, width, col, [("knots", (N + 1,), torch.float64, None)])["knots"]
                if knots is not None:
                    kn.copy_(knots)
            if knots is not None:
                po.flags = binding.STE_POS_REUSE_KNOTS
            keep.append(kn)
            names = ("lon", "lat", "speed", "heading") if velocity else ("lon", "lat")
            out = {k: torch.empty((S, Q), **f64) for k in names}
            out.update(step=torch.empty((Q,), **i32), frac=torch.empty((Q,), **f64), status=torch.empty((Q,), **i32))
            for k, ten in out.items():
                setattr(po, k, ten.data_ptr())
            cnt = mom = None
            if anchor is not None:
                an = anchor.to(self.device)
                an = (an if perm is None else an[:, perm]).contiguous()
                if accumulate is None:
                    cnt, mom = torch.zeros((Q,), **i32), torch.zeros((5, Q), **f64)
                elif perm is None:
                    cnt, mom = accumulate[0].contiguous(), accumulate[1].contiguous()
                else:
                    cnt, mom = accumulate[0][perm].contiguous(), accumulate[1][:, perm].contiguous()
                po.anchor, po.count, po.moments = an.data_ptr(), cnt.data_ptr(), mom.data_ptr()
                keep += [an, cnt, mom]
            binding.check(self.lib.ste_track_positions_f64(C.byref(s), C.byref(po), self._stream(st)), "ste_track_positions_f64")
            if perm is not None:  # back to the caller's order
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(Q, device=self.device)
                out = {k: v[..., inv].contiguous() for k, v in out.items()}
                if cnt is not None:
                    cnt, mom = cnt[inv].contiguous(), mom[:, inv].contiguous()
                keep += [perm, inv]
            if cnt is not None:
                if accumulate is not None:
                    if cnt.data_ptr() != accumulate[0].data_ptr():
                        accumulate[0].copy_(cnt)
                    if mom.data_ptr() != accumulate[1].data_ptr():
                        accumulate[1].copy_(mom)
                    cnt, mom = accumulate
                out["count"], out["moments"] = cnt, mom
            out["knots"] = kn
            return self._finish(st, keep, out)

    # -- a space-time gridded field at query times ----------------------------------------------------------------
    def track_knots(self, stream=None):
        """The knot times of this batch's tracks, (Nmax+1, B) on the device: the in-order sums of ``dt`` that
        ``positions_at`` returns as ``knots``, from one positions call with a single query that reads no track (its index is
        -1) and ``status`` as the only output.  Row 0 holds 0, or NaN for a track with a ``dt`` that is not finite and >= 0;
        rows past ``nsteps[b]`` are NaN.  ``field_at`` and ``positions_at`` take it as ``knots=``."""
        torch = self.torch
        N = int(self.struct.Nmax)
        ld = int(self.struct.track_stride or self.struct.B)
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            s = binding.SteUkfBatchF64.from_buffer_copy(self.struct)
            po = binding.StePositionsF64()
            out = self._track_outputs(po, ld, self.lo, [("knots", (N + 1,), torch.float64, float("nan"))])
            qt = torch.full((1,), -1, dtype=torch.int32, device=self.device)
            tq = torch.zeros((1,), dtype=torch.float64, device=self.device)  # also stands in for `states`: nothing reads it
            status = torch.empty((1,), dtype=torch.int32, device=self.device)
            po.nstates, po.flags, po.states = 1, 0, tq.data_ptr()
            po.nqueries, po.qtrack, po.qtime, po.status = 1, qt.data_ptr(), tq.data_ptr(), status.data_ptr()
            binding.check(self.lib.ste_track_positions_f64(C.byref(s), C.byref(po), self._stream(st)), "ste_track_positions_f64")
            return self._finish(st, [qt, tq, status], out)["knots"]

    def field_at(self, states, field, qtrack, qtime, t0=None, nearest: bool = False, min_cover: float = 0.0, vanchor=None,
                 accumulate=None, knots=None, per_sample: bool = True, stream=None, sort: bool = True):
        """The values of a space-time gridded field where tracks that are on the device were at given clock times
        (include/ste.h: ste_field_values_f64; DESIGN.md, "Fields").  ``states``, ``qtrack``, ``qtime``, ``t0``, ``sort`` and
        ``stream`` as in ``positions_at``; ``field`` a ``TrackField`` (``track_field`` makes one) on this batch's device.  Per
        (sample, query) the position of ``positions_at`` is formed and the field is read there: trilinear in (time, lat, lon)
        between the nodes at the cell centres, NaN nodes left out and the weights of the others renormalised, the value NaN
        where their weight ``cover`` is 0 or below ``min_cover``; with ``nearest`` the value of the node of the cell the
        position lies in, in the slab nearest in time (categorical fields).  Nothing is extrapolated in time: a located query
        off the field's time axis has STE_FLD_TIME_OUTSIDE in ``status`` and NaN values.  ``knots``: the tensor
        ``track_knots()`` or a previous call returned; None sums them once more.  Returns a dict of device tensors: with
        ``per_sample`` ``value`` and ``cover`` (S, Q); ``status`` (Q,) int32; ``knots``.  With ``vanchor``, a (Q,) array or
        tensor, also ``count`` (3, Q) int32 -- the samples with a finite value, those on the grid without one, those off the
        grid --, ``moments`` (2, Q), the sums over the samples of d and d d, d = value - vanchor, and ``vmin``, ``vmax`` (Q,),
        NaN where no sample has a value.  They start from zero and NaN, or with ``accumulate=(count, moments, vmin, vmax)``
        from those tensors, which are updated in place and returned: S samples in one call and the same samples in several
        calls give the same bits."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        states, S = self._metric_states(states)
        if not isinstance(field, TrackField):
            raise ValueError("field must be a TrackField (track_estimators.batch.track_field makes one)")
        if field.values.device != self.device:
            raise ValueError(f"the field's values are on {field.values.device}, this batch is on {self.device}")
        min_cover = float(min_cover)
        if not 0.0 <= min_cover <= 1.0:
            raise ValueError(f"min_cover must lie in [0, 1], got {min_cover!r}")
        qtrack = _index_tensor(qtrack, "qtrack", (), binding.STE_POSITIONS_MAX_QUERIES)
        Q = int(qtrack.shape[0])
        qtime = torch.as_tensor(qtime, dtype=torch.float64)
        if tuple(qtime.shape) != (Q,):
            raise ValueError(f"qtime must have shape ({Q},) like qtrack, got {tuple(qtime.shape)}")
        if vanchor is not None:
            vanchor = torch.as_tensor(vanchor, dtype=torch.float64)
            if tuple(vanchor.shape) != (Q,):
                raise ValueError(f"vanchor must have shape ({Q},): one value per query, got {tuple(vanchor.shape)}")
        acc_shapes = (("count", torch.int32, (3, Q)), ("moments", torch.float64, (2, Q)), ("vmin", torch.float64, (Q,)),
                      ("vmax", torch.float64, (Q,)))
        if accumulate is not None:
            if vanchor is None:
                raise ValueError("accumulate continues the moments about an anchor: give the vanchor they were started with")
            ok = len(accumulate) == 4 and all(isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == dt
                                              and tuple(a.shape) == shape for a, (_, dt, shape) in zip(accumulate, acc_shapes))
            if not ok:
                raise ValueError(f"accumulate must be (count, moments, vmin, vmax): an int32 (3, {Q}), a float64 (2, {Q}) and two "
                                 f"float64 ({Q},) tensors on {self.device}")
        if knots is not None and not (isinstance(knots, torch.Tensor) and knots.dtype == torch.float64 and knots.device == self.device
                                      and tuple(knots.shape) == (N + 1, B)):
            raise ValueError(f"knots must be the float64 ({N + 1}, {B}) tensor a previous call on this batch returned")
        if knots is None:
            knots = self.track_knots(stream=stream)
        grid = field.grid
        st = self._ordered_stream(stream)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        with torch.cuda.stream(st):
            qt = _index_int32(qtrack.to(self.device))
            tq = qtime.to(self.device).contiguous()
            perm = None
            if sort and Q > 1:
                by_time = torch.sort(tq, stable=True).indices
                perm = by_time[torch.sort(qt[by_time], stable=True).indices]
                qt, tq = qt[perm].contiguous(), tq[perm].contiguous()
            keep = [qt, tq, field.values]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=False)  # the knots stand in for dt
            f = binding.SteFieldF64()
            f.nstates, f.states = S, states.data_ptr()
            f.flags = ((binding.STE_GRID_PERIODIC_LON if grid.periodic else 0) | (binding.STE_FLD_NEAREST if nearest else 0)
                       | (binding.STE_FLD_VALUES_F32 if field.values.dtype == torch.float32 else 0))
            f.nqueries, f.qtrack, f.qtime = Q, qt.data_ptr(), tq.data_ptr()
            f.t0 = self._track_clock(t0, width, col, keep)
            if knots.stride() == (width, 1):
                kn = knots  # the view a call on this layout returned: read where it lies
                f.knots = kn.data_ptr()
            else:
                kn = self._track_outputs(f, width, col, [("knots", (N + 1,), torch.float64, None)])["knots"]
                kn.copy_(knots)
            keep.append(kn)
            f.nx, f.ny, f.nt, f.reserved = grid.nx, grid.ny, field.nt, 0
            f.lon0, f.lat0, f.dlon, f.dlat, f.lon_ref = grid.lon0, grid.lat0, grid.dlon, grid.dlat, grid.lon_ref
            f.time0, f.dtime, f.min_cover = field.time0, field.dtime, min_cover
            f.values = field.values.data_ptr()
            out = {k: torch.empty((S, Q), **f64) for k in (("value", "cover") if per_sample else ())}
            out["status"] = torch.empty((Q,), **i32)
            for k, ten in out.items():
                setattr(f, k, ten.data_ptr())
            acc = None
            if vanchor is not None:
                an = vanchor.to(self.device)
                an = (an if perm is None else an[perm]).contiguous()
                if accumulate is None:
                    acc = [torch.zeros((3, Q), **i32), torch.zeros((2, Q), **f64), torch.full((Q,), float("nan"), **f64),
                           torch.full((Q,), float("nan"), **f64)]
                elif perm is None:
                    acc = [a.contiguous() for a in accumulate]
                else:
                    acc = [a[..., perm].contiguous() for a in accumulate]
                f.vanchor = an.data_ptr()
                for (k, _, _), a in zip(acc_shapes, acc):
                    setattr(f, k, a.data_ptr())
                keep += [an] + acc
            binding.check(self.lib.ste_field_values_f64(C.byref(s), C.byref(f), self._stream(st)), "ste_field_values_f64")
            if perm is not None:  # back to the caller's order
                inv = torch.empty_like(perm)
                inv[perm] = torch.arange(Q, device=self.device)
                out = {k: v[..., inv].contiguous() for k, v in out.items()}
                if acc is not None:
                    acc = [a[..., inv].contiguous() for a in acc]
                keep += [perm, inv]
            if acc is not None:
                if accumulate is not None:
                    for a, given in zip(acc, accumulate):
                        if a.data_ptr() != given.data_ptr():
                            given.copy_(a)
                    acc = list(accumulate)
                for (k, _, _), a in zip(acc_shapes, acc):
                    out[k] = a
            out["knots"] = kn
            return self._finish(st, keep, out)

    # -- fixed sites ----------------------------------------------------------------------------------------------
    _SITE_OUT3 = ("min_dist", "min_time", "time_within", "first_within", "longest")

    def site_metrics(self, states, sites, radius_km, t0=None, model: str = "sphere", stream=None):
        """Tracks that are on the device against fixed sites -- ports, anchorages, buoys -- (include/ste.h:
        ste_site_metrics_f64; DESIGN.md, "Sites"): every ship against every site, a dense block.  ``states`` as in
        ``path_metrics``.  ``sites``: an (M, 2) array or tensor of (lon, lat) in degrees, 1 <= M <= 65536.  ``radius_km``: a
        scalar or one radius per site, (M,).  ``t0`` and ``model`` as in ``encounter_metrics``.  Returns a dict of device
        tensors: ``min_dist`` (S, M, B) in km, NaN where the track has no sound step; ``min_time``, its clock time;
        ``time_within``, hours with the planar distance <= the site's radius; ``first_within``, the clock time the first such
        run starts, NaN = never; ``longest``, the hours of the longest run; ``nwithin`` int32, the number of runs;
        ``sound_time`` (S, B), the hours of sound steps, and ``nbroken`` (S, B) int32, the steps left out (a NaN latitude, or 90
        degrees of longitude or more in one step); ``track_status`` (B,) int32, STE_SITE_BAD_TIME (a non-finite ``t0``, a ``dt``
        that is not finite and >= 0), and ``site_status`` (M,) int32, STE_SITE_BAD_SITE (a non-finite coordinate, or a radius
        that is not finite and between 0 and 1000): neither is refused, a bad track or site gives NaN / 0.  Windows, in-place
        views and ``stream`` as in ``path_metrics``; for a window read in place the per-track outputs are views of rows as
        wide as the fleet's.  Every value depends on the track's rows, ``dt``, ``t0`` and the site's three numbers alone."""
        torch = self.torch
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        sv = torch.as_tensor(sites, dtype=torch.float64)
        if sv.dim() != 2 or sv.shape[1] != 2 or not 1 <= sv.shape[0] <= binding.STE_SITES_MAX:
            raise ValueError(f"sites must have shape (M, 2) (lon, lat) with 1 <= M <= {binding.STE_SITES_MAX}, got {tuple(sv.shape)}")
        M = int(sv.shape[0])
        rv = torch.as_tensor(radius_km, dtype=torch.float64)
        if rv.dim() == 0:
            rv = rv.expand(M)
        if tuple(rv.shape) != (M,):
            raise ValueError(f"radius_km must be a scalar or have shape ({M},), got {tuple(rv.shape)}")
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            xy = sv.to(self.device).t().contiguous()  # [2][M]: lon then lat
            rad = rv.to(self.device).contiguous()
            keep = [xy, rad]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            si = binding.SteSiteF64()
            si.nstates, si.model, si.states = S, model_id, states.data_ptr()
            si.nsites, si.sites, si.radius_km, si.flags, si.reserved = M, xy.data_ptr(), rad.data_ptr(), 0, 0
            si.t0 = self._track_clock(t0, width, col, keep)
            # rows as wide as the states': the window's columns are what the call writes and what is returned
            spec = [(k, (S, M), f64, None) for k in self._SITE_OUT3]
            spec += [("nwithin", (S, M), i32, None), ("sound_time", (S,), f64, None), ("nbroken", (S,), i32, None),
                     ("track_status", (), i32, None)]
            out = self._track_outputs(si, width, col, spec)
            out["site_status"] = torch.empty((M,), dtype=i32, device=self.device)
            si.site_status = out["site_status"].data_ptr()
            binding.check(self.lib.ste_site_metrics_f64(C.byref(s), C.byref(si), self._stream(st)), "ste_site_metrics_f64")
            return self._finish(st, keep, out)

    # -- polylines ------------------------------------------------------------------------------------------------
    _LINE_OUT3 = {"min_dist": False, "min_time": False, "min_seg": True, "min_frac": False}  # name -> int32?
    _LINE_CROSS = {"ncross": True, "net_cross": True, "first_cross": False, "last_cross": False}

    def line_metrics(self, states, lines, t0=None, model: str = "sphere", crossings: bool = True, stream=None):
        """Tracks that are on the device against polylines -- coasts, cables, planned routes, gates -- (include/ste.h:
        ste_line_metrics_f64; DESIGN.md, "Lines"): every ship against every line, a dense block.  ``states`` as in
        ``path_metrics``.  ``lines``: a list of (n_i, 2) arrays of (lon, lat) in degrees, n_i >= 2, or what ``track_lines``
        made of one (which has the rules and the refusals).  ``t0`` and ``model`` as in ``site_metrics``.  Returns a dict of
        device tensors: ``min_dist`` (S, M, B) in km, the distance of ``model`` between the ship and the line where the planar
        distance is least, NaN where the track has no sound step; ``min_time``, its clock time; ``min_seg`` int32, the
        segment of the line that is closest (-1 = none) and ``min_frac``, where along it (0 at its first vertex, 1 at its
        second); with ``crossings`` also ``ncross`` int32, the number of crossings, ``net_cross`` int32, those from the right
        of the line's direction to its left minus the others (for a counter-clockwise ring: entries minus exits), and
        ``first_cross`` and ``last_cross``, the clock times of the earliest and the latest, NaN = none; ``sound_time`` (S, B)
        and ``nbroken`` (S, B) int32 as in ``site_metrics``; ``track_status`` (B,) int32, STE_LINE_BAD_TIME, and
        ``line_status`` (M,) int32, STE_LINE_BAD_LINE.  Windows, in-place views and ``stream`` as in ``site_metrics``.  Every
        value depends on the track's rows, ``dt``, ``t0`` and the line's vertices alone."""
        torch = self.torch
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        tl = lines if isinstance(lines, TrackLines) else track_lines(lines)
        M, V = tl.nlines, int(tl.vert.shape[1])
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            vert, first, ref = tl.on(self.device)
            keep = [vert, first, ref]
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            li = binding.SteLineF64()
            li.nstates, li.model, li.states = S, model_id, states.data_ptr()
            li.nlines, li.nvert, li.vert, li.first, li.lon_ref = M, V, vert.data_ptr(), first.data_ptr(), ref.data_ptr()
            li.flags, li.reserved = 0, 0
            li.t0 = self._track_clock(t0, width, col, keep)
            # rows as wide as the states': the window's columns are what the call writes and what is returned
            names = dict(self._LINE_OUT3)
            if crossings:
                names.update(self._LINE_CROSS)
            spec = [(k, (S, M), i32 if isint else f64, None) for k, isint in names.items()]
            spec += [("sound_time", (S,), f64, None), ("nbroken", (S,), i32, None), ("track_status", (), i32, None)]
            out = self._track_outputs(li, width, col, spec)
            out["line_status"] = torch.empty((M,), dtype=i32, device=self.device)
            li.line_status = out["line_status"].data_ptr()
            binding.check(self.lib.ste_line_metrics_f64(C.byref(s), C.byref(li), self._stream(st)), "ste_line_metrics_f64")
            return self._finish(st, keep, out)

    # -- routes: pairs of tracks as curves ------------------------------------------------------------------------
    def route_metrics(self, states, pairs, dtw: bool = False, band: int = 0, reverse: bool = False, model: str = "sphere",
                      stream=None):
        """Pairs of tracks that are on the device against each other as curves, without a clock (include/ste.h:
        ste_route_metrics_f64; DESIGN.md, "Routes"): the discrete Frechet distance and, with ``dtw``, the time-warping cost.
        ``states`` and ``pairs`` as in ``encounter_metrics``; sample s of one ship is held against sample s of the other, rows
        0 .. nsteps of each, and no ``dt`` is read.  ``band``: 0, or the Sakoe-Chiba band |a - b| <= band on the row indices.
        ``reverse``: track j is read from its last row to its first (ships on one lane in opposite directions).  ``model``: the
        leg function of ``frechet``, "sphere" or "wgs84".  Returns a dict of device tensors: ``frechet`` (S, P) in km;
        ``frechet_at`` (S, P, 2) int32, the rows of i and j whose distance it is; ``status`` (S, P) int32, STE_ROUTE_BAD_INDEX /
        STE_ROUTE_NO_PATH (the lengths differ by more than the band) / STE_ROUTE_NOT_FINITE, any of which gives NaN and
        (-1, -1); and with ``dtw`` ``dtw`` (S, P) in km, the summed great-circle gaps on the cheapest warping path, and
        ``dtw_len`` (S, P) int32, the cells on that path (0 with a status bit).  The scratch the kernel needs for tracks of
        more than ``ste_route_lds_cols()`` rows is allocated here.  Windows, in-place views and ``stream`` as in
        ``path_metrics``; every value depends on the two tracks' rows, ``band`` and ``reverse`` alone."""
        torch = self.torch
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        band = int(band)
        if not 0 <= band < 2 ** 31:
            raise ValueError(f"band must be >= 0 (0 = no band) and below 2^31, got {band!r}")
        pairs = _index_tensor(pairs, "pairs", (2,), binding.STE_ROUTE_MAX_PAIRS)
        st = self._ordered_stream(stream)
        with torch.cuda.stream(st):
            pr = _index_int32(pairs.to(self.device))
            keep = [pr]
            s, states, _, _ = self._fleet_layout(states, keep, needs_dt=False)  # a curve has no clock
            out = _route_call(self.lib, torch, s, states, S, pr, dtw, band, reverse, model_id, self.device, self._stream(st),
                              keep)
            return self._finish(st, keep, out)

    # -- speeds ---------------------------------------------------------------------------------------------------
    _SPEED_OUT = ("dist", "sound_time", "vmax", "vmax_time")
    _SPEED_RUNS = {"cond_time": False, "run_time": False, "first_run": False, "longest": False, "longest_start": False,
                   "nruns": True}  # name -> int32?

    def speed_metrics(self, states, bands=None, threshold=None, above: bool = False, min_run_h: float = 0.0,
                      model: str = "sphere", per_step: bool = False, stream=None):
        """How fast tracks that are on the device went (include/ste.h: ste_speed_metrics_f64; DESIGN.md, "Speeds"): the speed
        made good of a step is its leg over its ``dt``, in km/h (``KNOT_KMH`` km/h to the knot).  ``states`` and ``model`` as in
        ``path_metrics``.  ``bands``: None, or nbands + 1 <= 33 band edges in km/h, finite, >= 0 and strictly ascending.
        ``threshold``: None, a scalar or one speed per track ((B,) array or tensor), km/h: a step qualifies at or below it
        (stops, loitering), with ``above`` at or above it (sustained speed), and consecutive qualifying steps form a run that
        counts when it lasts ``min_run_h`` hours or longer.  Returns a dict of device tensors, (S, B) unless said otherwise:
        ``dist`` (km) and ``sound_time`` (hours) over the sound steps; ``vmax`` and ``vmax_time``, the largest speed and the
        hours from row 0 to the start of its step, NaN without a sound step; ``nbroken`` int32, the steps left out (a
        coordinate that is not finite); ``track_status`` (B,) int32, STE_SPEED_BAD_TIME (a ``dt`` that is not finite and >= 0)
        and STE_SPEED_BAD_LIMIT (such a threshold): neither is refused, a bad track gives NaN / 0; with ``bands``
        ``band_time`` (S, nbands, B), the hours with edges[j] <= v < edges[j+1]; with ``threshold`` ``cond_time`` (hours of
        qualifying steps), ``run_time`` (hours in runs that count), ``nruns`` int32, ``first_run`` (hours from row 0 to the start
        of the first run that counts, NaN = none), ``longest`` and ``longest_start`` (the longest run, counting or not); with
        ``per_step`` ``speed`` (S, Nmax, B), NaN for a step of zero ``dt``, a broken step and past ``nsteps[b]``.  Windows,
        in-place views and ``stream`` as in ``path_metrics``; every value depends on its own track's rows, ``dt`` and threshold
        alone, and ``dist`` has the bits of ``path_metrics`` where every step is sound."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        edges = None
        if bands is not None:
            edges = np.ascontiguousarray(bands.cpu().numpy() if isinstance(bands, torch.Tensor) else bands, dtype=np.float64)
            if edges.ndim != 1 or not 2 <= edges.size <= binding.STE_SPEED_MAX_BANDS + 1:
                raise ValueError(f"bands must be None or 2 .. {binding.STE_SPEED_MAX_BANDS + 1} band edges, got shape {edges.shape}")
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            keep = []
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=True)
            sp = binding.SteSpeedF64()
            sp.nstates, sp.model, sp.states = S, model_id, states.data_ptr()
            sp.flags, sp.min_run_h = (binding.STE_SPEED_ABOVE if above else 0), float(min_run_h)
            sp.nbands, sp.band_edges = (0, None) if edges is None else (edges.size - 1, edges.ctypes.data)
            sp.threshold, sp.threshold_all = None, float("nan")
            if threshold is not None:
                sp.threshold, scalar = track_input(threshold, B, width, col, keep, self.device,
                                                   f"threshold must be None, a scalar or have shape ({B},)", scalar=True)
                if scalar is not None:
                    sp.threshold_all = scalar
            # rows as wide as the states': the window's columns are what the call writes and what is returned
            spec = [(k, (S,), f64, None) for k in self._SPEED_OUT]
            spec += [("nbroken", (S,), i32, None), ("track_status", (), i32, None)]
            if edges is not None:
                spec.append(("band_time", (S, edges.size - 1), f64, None))
            if threshold is not None:
                spec += [(k, (S,), i32 if int32 else f64, None) for k, int32 in self._SPEED_RUNS.items()]
            if per_step:
                spec.append(("speed", (S, N), f64, float("nan")))
            out = self._track_outputs(sp, width, col, spec)
            binding.check(self.lib.ste_speed_metrics_f64(C.byref(s), C.byref(sp), self._stream(st)), "ste_speed_metrics_f64")
            return self._finish(st, keep, out)

    # -- errors ---------------------------------------------------------------------------------------------------
    _ERROR_OUT = {"sum_err": False, "sum_sq": False, "max_err": False, "n": True, "max_row": True, "nbroken": True}  # name -> int32?
    _ERROR_COURSE = {"sum_along": False, "sum_along_sq": False, "sum_cross": False, "sum_cross_sq": False, "ncoursed": True}
    _ERROR_NEES = {"sum_nees": False, "nscored": True, "ninside": True}

    def _track_rows(self, x, name: str, mid, width, col, keep):
        """A per-row input of a metric call that does not depend on the sample -- (Nmax+1, B), or (Nmax+1, r, B) with r in
        ``mid`` -- as (the pointer the kernel takes, r): an array is uploaded; a device tensor whose rows already are ``width``
        tracks wide and start at this batch's column (``window.sm_cov`` beside ``window.sm_mean``) is read where it lies,
        anything else is copied into such rows.  Inside the stream context."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        shapes = [(N + 1, B)] if mid is None else [(N + 1, r, B) for r in mid]
        if x.dtype != torch.float64 or tuple(x.shape) not in shapes:
            raise ValueError(f"{name} must be float64 of shape {' or '.join(str(s) for s in shapes)}, got {x.dtype} {tuple(x.shape)}")
        r = 1 if mid is None else int(x.shape[1])
        x = x.to(self.device)
        rows_strides = (r * width, 1) if mid is None else (r * width, width, 1)
        if all(n == 1 or sd == fd for n, sd, fd in zip(x.shape, x.stride(), rows_strides)):
            keep.append(x)
            return x.data_ptr(), r
        wide = torch.full(x.shape[:-1] + (width,), float("nan"), dtype=torch.float64, device=self.device)
        wide[..., col:col + B] = x
        keep.append(wide)
        return column_pointer(wide, col), r

    def track_errors(self, states, truth, course=None, cov=None, coverage: float = 0.95, model: str = "sphere", rows: bool = False,
                     cumulative: bool = False, stream=None):
        """How far tracks that are on the device are from where the ship really was (include/ste.h: ste_track_errors_f64;
        DESIGN.md, "Errors").  ``states`` and ``model`` as in ``path_metrics``.  ``truth``: (Nmax+1, 2, B), lon and lat in
        degrees at the tracks' own rows, track last, NaN where there is no truth (``observation_rows`` and ``hold_out`` make
        one); the error of a row is the leg of ``model`` from the truth to the state, in km.  ``course``: None or (Nmax+1, B),
        the true course over ground in degrees (``truth_course``), which splits the error into ``along`` (positive when the
        state is ahead of the truth: timing) and ``cross`` (positive to starboard: route).  ``cov``: None, "sm" or "fwd" (this
        batch's smoothed or filtered covariance) or a (Nmax+1, 10 or 16, B) tensor, upper triangles or full matrices, for S = 1
        only: q = d^T C^-1 d of the position error d in degrees against the 2 x 2 position block C is the NEES of a row, and
        a row is inside when q <= -2 ln(1 - ``coverage``), the chi-square quantile for 2 degrees of freedom.

        Returns a dict of device tensors, (S, B): ``sum_err`` (km; cum_abs_diff's last value), ``sum_sq``, ``max_err`` and
        ``max_row`` int32 (NaN and -1 without a sound row), ``n`` int32 (the rows with truth and a finite error) and
        ``nbroken`` int32 (rows with truth whose state or leg is not finite), and derived from them ``rmse`` =
        sqrt(sum_sq / n) and ``mean_err``; with ``course`` ``sum_along``, ``sum_along_sq``, ``sum_cross``, ``sum_cross_sq``,
        ``ncoursed`` int32, ``mean_along`` and ``rms_cross``; with ``cov`` ``sum_nees``, ``nscored`` and ``ninside`` int32,
        ``mean_nees`` and ``coverage`` = ninside / nscored.  A derived value is NaN where its count is 0.  With ``rows`` the
        per-row values (S, Nmax+1, B) ``err``, and ``along``, ``cross``, ``nees`` where they exist, NaN where the row has none
        and past ``nsteps[b]``; with ``cumulative`` ``cumerr``, the running sum_err, NaN past ``nsteps[b]``.  Windows, in-place
        views and ``stream`` as in ``path_metrics``; every value depends on its own track's rows, truth, course and covariance
        alone."""
        import math

        torch = self.torch
        N = int(self.struct.Nmax)
        states, S = self._metric_states(states)
        model_id = _metric_model(model)
        if isinstance(cov, str):
            if cov not in ("sm", "fwd"):
                raise ValueError(f"cov must be None, 'sm', 'fwd' or a tensor, got {cov!r}")
            cov = self.sm_cov if cov == "sm" else self.fwd_cov
            if cov is None:
                raise ValueError("this batch holds no such covariance history (alloc_smoothed=False or histories=False)")
        if cov is not None:
            if S != 1:
                raise ValueError(f"cov goes with one track per ship (a covariance belongs to one track, not to its samples), got S = {S}")
            if not 0.0 < float(coverage) < 1.0:
                raise ValueError(f"coverage must lie strictly between 0 and 1, got {coverage!r}")
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            keep = []
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=False)
            er = binding.SteErrorsF64()
            er.nstates, er.model, er.states, er.reserved = S, model_id, states.data_ptr(), 0
            er.truth, _ = self._track_rows(truth, "truth", (2,), width, col, keep)
            names = dict(self._ERROR_OUT)
            per_row = ["err"] if rows else []
            if course is not None:
                er.course, _ = self._track_rows(course, "course", None, width, col, keep)
                names.update(self._ERROR_COURSE)
                per_row += ["along", "cross"] if rows else []
            if cov is not None:
                er.cov, er.cov_rows = self._track_rows(cov, "cov", (binding.STE_ERRORS_COV_PACKED, binding.STE_ERRORS_COV_FULL),
                                                       width, col, keep)
                er.nees_limit = -2.0 * math.log(1.0 - float(coverage))
                names.update(self._ERROR_NEES)
                per_row += ["nees"] if rows else []
            per_row += ["cumerr"] if cumulative else []
            # rows as wide as the states': the window's columns are what the call writes and what is returned
            spec = [(k, (S,), i32 if int32 else f64, None) for k, int32 in names.items()]
            spec += [(k, (S, N + 1), f64, float("nan")) for k in per_row]
            out = self._track_outputs(er, width, col, spec)
            binding.check(self.lib.ste_track_errors_f64(C.byref(s), C.byref(er), self._stream(st)), "ste_track_errors_f64")
            out["rmse"], out["mean_err"] = torch.sqrt(out["sum_sq"] / out["n"]), out["sum_err"] / out["n"]  # 0 / 0 = NaN
            if course is not None:
                out["mean_along"] = out["sum_along"] / out["ncoursed"]
                out["rms_cross"] = torch.sqrt(out["sum_cross_sq"] / out["ncoursed"])
            if cov is not None:
                out["mean_nees"], out["coverage"] = out["sum_nees"] / out["nscored"], out["ninside"].double() / out["nscored"]
            return self._finish(st, keep, out)

    # -- simplification -------------------------------------------------------------------------------------------
    def _track_limit(self, x, name: str, width, col, keep):
        """A limit of a metric call given as a scalar or one value per track, (B,), as (the pointer the kernel takes or None,
        the scalar it takes beside it).  Inside the stream context."""
        B = self.ntracks
        if not isinstance(x, self.torch.Tensor):
            x = np.asarray(x, dtype=np.float64)
        ptr, scalar = track_input(x, B, width, col, keep, self.device, f"{name} must be a scalar or have shape ({B},)", scalar=True)
        return ptr, 0.0 if scalar is None else scalar

    def track_lon_scale(self, states):
        """cos of the smallest |latitude| over the rows <= nsteps of all samples of each track, (B,) on the device: the
        ``lon_scale="track"`` of ``simplify_tracks``.  It never measures an east-west extent of the track short."""
        torch = self.torch
        states, _ = self._metric_states(states)
        N, B = int(self.struct.Nmax), self.ntracks
        ns = self.t["nsteps"][self.lo:self.lo + B]
        past = torch.arange(N + 1, device=self.device)[:, None] > ns[None, :]  # (N+1, B)
        lat = states[:, :, 1, :].abs().masked_fill(past[None], float("inf"))
        return torch.cos(torch.deg2rad(lat.amin(dim=(0, 1))))

    def simplify_tracks(self, states, tolerance_km, shape: bool = False, lon_scale="track", compact: bool = True, max_rows=None,
                        stream=None):
        """Tracks that are on the device made smaller within a tolerance (include/ste.h: ste_track_simplify_f64; DESIGN.md,
        "Simplification"): the time-aware Douglas-Peucker rule, which drops a row when the position interpolated at that row's
        own time between the surviving neighbours is within ``tolerance_km`` of it, so that ``positions_at`` on the result stays
        within the tolerance at every row time; with ``shape`` the classic rule on the perpendicular distance, without a clock
        (what ``route_metrics`` and ``line_metrics`` ask about).  ``states`` as in ``path_metrics``.  ``tolerance_km``: a scalar
        or one value per track, km, divided by ``KM_PER_DEG``.  ``lon_scale``: what a degree of longitude counts against a
        degree of latitude: "track" (``track_lon_scale``: the tolerance is honoured in the local equirectangular sense), a
        float (1.0 = plain degrees) or one value per track.

        Returns a dict of device tensors: ``keep`` (S, Nmax+1, B) uint8, 1 for a kept row, 0 otherwise and past ``nsteps[b]``;
        ``nkeep`` (S, B) int32; ``worst_km`` (S, B), the largest deviation of a dropped row from its chord (NaN for a track
        kept whole because of a status bit); ``status`` (S, B) int32, STE_SIMPLIFY_BAD_TIME / BAD_LIMIT / BROKEN (the track is
        kept whole) and TRUNCATED; ``lon_scale`` (B,), as given to the kernel (absent for a float); and with ``compact`` the
        kept rows as a fleet of their own, narrowed to the largest ``nkeep`` (one small read-back, no second launch) or to
        ``max_rows``: ``rows`` (S, M, B) int32, -1 past ``nkeep``; ``states`` (S, M, 4, B), NaN past ``nkeep``; ``dt``
        (S, M-1, B), the hours between kept rows, 0 past ``nkeep``.  Windows, in-place views and ``stream`` as in
        ``path_metrics``; every value depends on its own track's rows, ``dt``, tolerance and scale alone."""
        torch = self.torch
        N, B = int(self.struct.Nmax), self.ntracks
        states, S = self._metric_states(states)
        cap = N + 1 if max_rows is None else int(max_rows)
        if compact and not 1 <= cap <= N + 1:
            raise ValueError(f"max_rows must be None or between 1 and Nmax + 1 = {N + 1}, got {max_rows!r}")
        st = self._ordered_stream(stream)
        f64, i32 = torch.float64, torch.int32
        with torch.cuda.stream(st):
            keep = []
            scale_t = None
            if isinstance(lon_scale, str):
                if lon_scale != "track":
                    raise ValueError(f"lon_scale must be 'track', a float or have shape ({B},), got {lon_scale!r}")
                lon_scale = scale_t = self.track_lon_scale(states)
            s, states, width, col = self._fleet_layout(states, keep, needs_dt=not shape or compact)
            sf = binding.SteSimplifyF64()
            sf.nstates, sf.flags, sf.reserved, sf.states = S, (binding.STE_SIMPLIFY_SHAPE if shape else 0), 0, states.data_ptr()
            tol = tolerance_km / KM_PER_DEG if isinstance(tolerance_km, torch.Tensor) else np.asarray(tolerance_km, dtype=np.float64) / KM_PER_DEG
            sf.tolerance, sf.tolerance_all = self._track_limit(tol, "tolerance_km", width, col, keep)
            sf.lon_scale, sf.lon_scale_all = self._track_limit(lon_scale, "lon_scale", width, col, keep)
            if sf.lon_scale and scale_t is None:
                scale_t = keep[-1][col:col + B]
            need = int(self.lib.ste_track_simplify_workspace(N, S, B))
            if need:
                work = torch.empty(((need + 7) // 8,), dtype=f64, device=self.device)
                keep.append(work)
                sf.work, sf.work_bytes = work.data_ptr(), need
            # rows as wide as the states': the window's columns are what the call writes and what is returned
            spec = [("keep", (S, N + 1), torch.uint8, 0), ("nkeep", (S,), i32, None), ("worst_sq", (S,), f64, None),
                    ("status", (S,), i32, None)]
            if compact:
                sf.cap = cap
                spec += [("rows", (S, cap), i32, -1), ("out_states", (S, cap, 4), f64, float("nan")),
                         ("out_dt", (S, max(cap - 1, 0)), f64, 0)]
            out = self._track_outputs(sf, width, col, spec)
            binding.check(self.lib.ste_track_simplify_f64(C.byref(s), C.byref(sf), self._stream(st)), "ste_track_simplify_f64")
            out["worst_km"] = torch.sqrt(out.pop("worst_sq")) * KM_PER_DEG
            if scale_t is not None:
                out["lon_scale"] = scale_t
            if compact:
                m = min(int(out["nkeep"].max()), cap)  # the read-back: how many rows the longest simplified track keeps
                out["rows"], out["states"], out["dt"] = out["rows"][:, :m], out.pop("out_states")[:, :m], out.pop("out_dt")[:, :m - 1]
            return self._finish(st, keep, out)

    # -- results ------------------------------------------------------------------------------------------------
    _OUT = {"means": ("fwd_mean", 4), "covs": ("fwd_cov", 16), "means_smoothed": ("sm_mean", 4),
            "covs_smoothed": ("sm_cov", 16)}

    def download(self, names=("means", "covs", "means_smoothed", "covs_smoothed"), track_index=None):
        """Histories as NumPy arrays shaped like the reference's return values, track first: ``means*`` (B, Nmax+1, 4),
        ``covs*`` (B, Nmax+1, 4, 4); rows past nsteps[b] are padding.  ``track_index`` (device int64 tensor) reorders /
        selects tracks on the device.  Each tensor is transposed on the device (one pass at HBM speed) and copied into
        page-locked host memory with an asynchronous copy; the arrays returned are views of that memory (PyTorch's
        host allocator recycles it once they are dropped, so only a process's first large download pays for pinning).
        10 000 x 500 with all four histories: 1.6 GB, ~35 ms over PCIe gen 5 instead of ~170 ms through pageable memory."""
        torch = self.torch
        self._require_histories("download()")
        if self._pipeline_done is not None:  # results of a SmootherPipeline.submit still in flight on another stream
            torch.cuda.current_stream(self.device).wait_event(self._pipeline_done)
        out, pending = {}, []
        for name in names:
            attr, width = self._OUT[name]
            t = getattr(self, attr)
            if t is None:
                raise ValueError(f"{name} was not computed for this batch (alloc_smoothed=False)")
            if track_index is not None:
                t = t.index_select(2, track_index)
            if width == 16 and self.packed_cov:  # upper triangles -> full symmetric matrices, still on the device
                if getattr(self, "_packed_index_t", None) is None:
                    self._packed_index_t = torch.tensor(self._PACKED_INDEX, dtype=torch.int64, device=self.device)
                t = t.index_select(1, self._packed_index_t)
            dev_t = t.permute(2, 0, 1).contiguous()  # (B, N+1, width) on the device
            host = torch.empty(dev_t.shape, dtype=dev_t.dtype, pin_memory=True)
            host.copy_(dev_t, non_blocking=True)
            pending.append(dev_t)  # keep the source alive until the copy has run
            a = host.numpy()
            out[name] = a.reshape(a.shape[0], a.shape[1], 4, 4) if width == 16 else a
        torch.cuda.current_stream(self.device).synchronize()
        return out

    def _download_into(self, names, host, lo, hi):
        """Asynchronous part of ``download`` for one window of a fleet: each history, track-major, into rows [lo, hi) of the
        page-locked tensors ``host[name]`` on the current stream.  Returns the device temporaries (to be kept alive until
        the stream has been synchronised)."""
        torch = self.torch
        pending = []
        for name in names:
            attr, width = self._OUT[name]
            t = getattr(self, attr)
            if width == 16 and self.packed_cov:
                if getattr(self, "_packed_index_t", None) is None:
                    self._packed_index_t = torch.tensor(self._PACKED_INDEX, dtype=torch.int64, device=self.device)
                t = t.index_select(1, self._packed_index_t)
            dev_t = t.permute(2, 0, 1).contiguous()
            host[name][lo:hi].copy_(dev_t, non_blocking=True)
            pending.append(dev_t)
        return pending

    def filtered(self):
        """(means (B, Nmax+1, 4), covs (B, Nmax+1, 4, 4)) as NumPy arrays (rows past nsteps[b] are padding)."""
        d = self.download(("means", "covs"))
        return d["means"], d["covs"]

    def smoothed(self):
        d = self.download(("means_smoothed", "covs_smoothed"))
        return d["means_smoothed"], d["covs_smoothed"]

    def status_host(self):
        if self._pipeline_done is not None:
            self._pipeline_done.synchronize()
        return self.status.cpu().numpy()


def forward_schedule(ntiles: Sequence[int], nslices: Sequence[int], nwaves: int, stagger: float = 0.0) -> np.ndarray:
    """
    The item table of a scheduled forward launch (include/ste.h: ``ste_fwd_sched_f64.items``): which (window, tile) every
    one of ``nwaves`` resident waves runs in every round, a round being one time slice of one 64-track tile.

    Window w has ``ntiles[w]`` tiles of ``nslices[w]`` slices each; a tile's slices run in order, one per round at most (a
    slice starts from the history row the one before it left).  With whole forward waves per tile -- one launch per window --
    W windows of T tiles cost ceil(W T / nwaves) pass times; here the makespan is R = ceil(total slices / nwaves) rounds
    (at least the longest tile): McNaughton's bound for preemptive scheduling of chains of unit jobs.  It is reached by list
    scheduling with two rules: a tile whose remaining slices equal the rounds left until its deadline runs now ("critical"),
    and the other waves go to the unfinished tiles in window order.

    ``stagger``: 0 gives every window the deadline R -- windows then finish in generations of as many as fill the chip,
    like whole launches do, only the last generation is spread under the ones before it.  1 spreads the deadlines of the
    windows evenly from the first possible finish to R, so that smoothers find forward passes to hide behind from the
    first finished window to the last.  Values between interpolate.

    Returns int32 [R][nwaves][2]; entries (-1, 0) are idle waves.  A tile stays on its wave from round to round when it
    keeps running.
    """
    ntiles = np.asarray(ntiles, dtype=np.int64)
    nslices = np.asarray(nslices, dtype=np.int64)
    if ntiles.ndim != 1 or ntiles.shape != nslices.shape or len(ntiles) == 0 or (ntiles < 1).any() or (nslices < 1).any():
        raise ValueError("ntiles and nslices: one positive entry per window")
    nwaves = int(nwaves)
    if nwaves < 1:
        raise ValueError("nwaves must be >= 1")
    nwin = len(ntiles)
    win = np.repeat(np.arange(nwin), ntiles)            # window of every job (tile), window order
    tile = np.concatenate([np.arange(n) for n in ntiles])
    remaining = nslices[win].copy()
    njobs = len(win)
    total = int(remaining.sum())
    R = max(-(-total // nwaves), int(nslices.max()))
    # deadline of window w: by then all work of windows <= w must fit on the chip, and no tile ends before its own length
    cum = np.cumsum(ntiles * nslices)
    earliest = np.maximum(np.ceil(cum / nwaves), np.maximum.accumulate(nslices)).astype(np.int64)
    first, span = int(earliest[0]), R - int(earliest[0])
    even = first + np.ceil(span * (np.arange(nwin) + 1 - 1) / max(nwin - 1, 1)).astype(np.int64) if nwin > 1 else np.array([R])
    dl_w = np.minimum(R, np.maximum(earliest, np.round(stagger * even + (1.0 - stagger) * R).astype(np.int64)))
    dl_w = np.maximum.accumulate(dl_w)
    dl = dl_w[win]
    items = np.full((R, nwaves, 2), (-1, 0), dtype=np.int32)
    wave_of = np.full(njobs, -1, dtype=np.int64)  # wave a job ran on in the previous round, -1: it did not run
    order = np.arange(njobs)
    r = 0
    while remaining.any():
        if r >= len(items):  # deadlines were too tight for the list scheduler somewhere: one more round
            items = np.concatenate([items, np.full((1, nwaves, 2), (-1, 0), dtype=np.int32)])
        live = order[remaining > 0]
        crit = (dl[live] - r) <= remaining[live]
        # critical tiles first, then earliest deadline, then window / tile order (np.lexsort: last key is the primary one)
        pick = live[np.lexsort((live, dl[live], ~crit))][:nwaves]
        keep = pick[wave_of[pick] >= 0]
        used = np.zeros(nwaves, dtype=bool)
        used[wave_of[keep]] = True
        new = pick[wave_of[pick] < 0]
        free = np.flatnonzero(~used)[: len(new)]
        ran = np.full(njobs, -1, dtype=np.int64)
        ran[keep] = wave_of[keep]
        ran[new] = free
        items[r, ran[pick], 0] = win[pick]
        items[r, ran[pick], 1] = tile[pick]
        remaining[pick] -= 1
        ran[remaining == 0] = -1
        wave_of = ran
        r += 1
    return items[:r]


def smoother_tile_order(items: np.ndarray, ntiles: Sequence[int]) -> np.ndarray:
    """The tile list of a sequence's one-launch smoother (include/ste.h: ``ste_bwd_sched_f64.items``): every (window, tile)
    of the item table ``items`` (``forward_schedule``) once, in the order the schedule finishes them -- by the last round in
    which a tile appears, ties in window / tile order (a stable sort).  Returns int32 [sum(ntiles)][2]."""
    tile0 = np.concatenate(([0], np.cumsum(ntiles)))
    last = np.full(int(tile0[-1]), -1, dtype=np.int64)
    live = items[..., 0] >= 0
    rr = np.broadcast_to(np.arange(items.shape[0])[:, None], items.shape[:2])[live]
    flat = tile0[items[..., 0][live]] + items[..., 1][live]
    np.maximum.at(last, flat, rr)
    idx = np.argsort(last, kind="stable")
    win = np.searchsorted(tile0, idx, side="right") - 1
    return np.ascontiguousarray(np.stack([win, idx - tile0[win]], axis=1).astype(np.int32))


# What decides between the smoother's two forms (csrc/ste_smooth.hip: kLeanSmootherMaxTracks and the tuning bits that
# lean_smoother() looks at; include/ste.h: STE_TUNING_*)
LEAN_SMOOTHER_MAX_TRACKS = 4096  # up to this many tracks: two kernels (all gains, then a lean recurrence); one kernel above
TUNING_TWO_KERNEL_SMOOTHER = binding.STE_TUNING_TWO_KERNEL_SMOOTHER  # ... two kernels whatever the batch size
TUNING_ONE_KERNEL_SMOOTHER = binding.STE_TUNING_ONE_KERNEL_SMOOTHER  # ... one kernel whatever the batch size


def _one_kernel_smoother(st) -> bool:
    """Does the batch struct ``st`` smooth from its work rows in one kernel?  Mirrors ``lean_smoother()`` in
    csrc/ste_smooth.hip: true where that is false for a batch with work rows and steps."""
    return bool(st.rts_work and st.Nmax > 0 and not (st.tuning & TUNING_TWO_KERNEL_SMOOTHER)
                and ((st.tuning & TUNING_ONE_KERNEL_SMOOTHER) or st.B > LEAN_SMOOTHER_MAX_TRACKS))


@dataclasses.dataclass(slots=True)
class _SequencePlan:
    """Shape and schedule of one ``submit_sequence`` call."""

    step: int  # steps per time slice
    ntiles: list  # per window: 64-track tiles
    nslices: list  # per window: time slices
    nwaves: int  # resident forward waves: one per SIMD the pipeline's forward streams may use
    key: tuple  # of the item table in SmootherPipeline._schedules
    items: np.ndarray  # forward_schedule's table

    def table_shape(self):
        """What the library sizes a forward launch's workspace by (ste_ukf_forward_sched_workspace / _progress_offset)."""
        return len(self.ntiles), max(self.nslices), sum(self.ntiles), self.items.shape[0], self.nwaves


@dataclasses.dataclass(slots=True)
class _TileSmootherLaunch:
    """Tables of a sequence's one-launch smoother; they live as long as the forward launch's record."""

    host_ws: object
    dev_ws: object
    order: np.ndarray  # smoother_tile_order's list, which the library reads at launch


@dataclasses.dataclass(slots=True)
class _ScheduledLaunch:
    """Everything one scheduled forward launch reads, kept alive until the pipeline is synchronised, or every gate and
    smoother that looks at it has finished (the error word is read then)."""

    host_ws: object  # page-locked (or pageable: _sched_pinned) image of the launch's tables
    dev_ws: object  # the tables on the device, and the per-tile progress counters behind them
    counters_all: object  # int32: [0 .. n) window_done, [n] error, [n + 1] waves of the launch that have begun
    counters: object  # its [:n + 1] view
    structs: object  # ctypes array of the windows' batch structs
    items: np.ndarray  # the schedule
    ready: object = None  # event behind the forward kernel
    events: list = dataclasses.field(default_factory=list)  # the windows' completion events
    prev_counters: object = None  # counters of the launch before this one while this launch's residency gate reads them
    smoother: Optional[_TileSmootherLaunch] = None  # set when the smoothers ran as one launch, a wave per tile

    def finished(self) -> bool:
        return all(ev.query() for ev in [self.ready] + self.events)

    def error_word(self) -> int:
        """0, or what could not progress: 1 = a forward wave, 2 = a smoother gate (synchronises with the device)."""
        return int(self.counters[-1].item())


@dataclasses.dataclass(slots=True)
class _LastScheduled:
    """The most recent scheduled forward launch on a device, of any pipeline of this process: what the next one's
    residency gate waits for (SmootherPipeline._wait_for_residency)."""

    counters: object  # the launch's counters_all
    started: int  # index of its started-waves word
    nwaves: int
    ready: object  # event behind its kernel
    owner: int  # id() of its pipeline


_last_scheduled = {}  # device index -> _LastScheduled


def _forget_scheduled(owner: int):
    """Drop ``owner``'s launches from ``_last_scheduled`` (its streams are drained and about to go: nothing to wait for)."""
    for dkey in [k for k, v in _last_scheduled.items() if v.owner == owner]:
        del _last_scheduled[dkey]


class _WorkspacePool:
    """Host / device table pairs (and counters) of retired scheduled launches, kept for the next ones: an allocation on the
    launch path -- pinned host memory above all -- is a driver call of unbounded length in the middle of a sequence of
    launches.  ``take`` allocates on the current stream, so call it with the launch's stream current."""

    def __init__(self, torch, device, min_bytes: int):
        self.torch, self.device, self.min_bytes = torch, device, int(min_bytes)
        self.free = []  # (host_ws, dev_ws, counters or None), most recently retired first

    def take(self, nbytes: int, ncounters: int = 0, pinned: bool = True):
        """(host_ws, dev_ws, counters) of at least ``nbytes`` bytes and ``ncounters`` int32 words (0: no counters, None):
        the first retired entry that fits, else new ones -- a power of two, so that the next launch fits as well."""
        for j, (host_ws, dev_ws, counters) in enumerate(self.free):
            if host_ws.numel() >= nbytes and (not ncounters or counters.numel() >= ncounters):
                del self.free[j]
                return host_ws, dev_ws, counters
        torch = self.torch
        cap = max(self.min_bytes, 1 << (nbytes - 1).bit_length())
        host_ws = torch.empty(cap, dtype=torch.uint8, pin_memory=pinned)
        dev_ws = torch.empty(cap, dtype=torch.uint8, device=self.device)
        counters = torch.empty(max(64, ncounters), dtype=torch.int32, device=self.device) if ncounters else None
        return host_ws, dev_ws, counters

    def give(self, entries):
        self.free = (list(entries) + self.free)[:16]


class SmootherPipeline:
    """
    Forward passes and smoothers of consecutive batches side by side on the GPU, several of each in flight.

    A batch of BASELINE size (10 000 tracks) is 157 long-running forward waves on 1 024 SIMDs followed by a smoother that
    is a latency chain (one wave per 64 tracks, ~1.5 us per step); run back to back they leave most of the chip idle.
    Two ways to overlap consecutive batches, both on streams that own a hardware queue each
    (``ste_stream_create_cu_range``; ordinary HIP streams share a handful of queues and their launches serialise):

    ``shared=True`` (default)  every stream may use every compute unit.  A lane-per-track forward wave is built to hold
        264 registers -- one per SIMD, never two -- and a smoother wave 240, so the smoothers of earlier batches slot in
        beside the forward waves of later ones and take the issue slots those leave (a forward wave issues ~80 % of its
        cycles; a smoother wave mostly waits for memory).  ``forward_streams`` forward passes fill the chip's SIMDs
        (seven at 10 000 tracks), ``smoother_streams`` smoothers hide each other's latency (six).
    ``shared=False``  round 1-2's split: forward passes on the first ``forward_cus`` compute units, smoothers on the rest.

    ``sequence_only=True``: a pipeline that will only see ``submit_sequence`` (one scheduled forward launch per sequence)
    keeps two forward streams.  Every stream here is a hardware queue, the device has about two dozen for everything that
    runs on it (measured: this pipeline's 14 plus nine idle ones elsewhere in the process and launches start to take turns),
    and scheduled launches -- long-lived kernels beside one-wave gates that never leave their queues idle -- are the first
    to suffer when they run out.

    Each ``DeviceBatch`` owns its histories and work rows; a batch is not resubmitted before its previous smoother has
    finished (events), so the caller rotates through ``buffers_needed`` or more of them.

        with SmootherPipeline(device, ntracks=hb.B) as pipe:
            dbs = [DeviceBatch(hb, device) for _ in range(pipe.buffers_needed)]
            for k in range(nbatches):
                pipe.submit(dbs[k % len(dbs)], final=(k == nbatches - 1))
            pipe.synchronize()

    The CU-masked streams are destroyed by ``close()`` (the context manager, ``__del__``, and at the latest an atexit
    hook): left to the HIP runtime's static destructors they outlive any profiler tool.
    """

    def __init__(self, device="cuda:0", forward_cus: Optional[int] = None, ntracks: Optional[int] = None,
                 forward_streams: Optional[int] = None, smoother_streams: Optional[int] = None, forward_lanes: int = 1,
                 shared: Optional[bool] = None, reserve_cus: int = 0, slices: Optional[int] = None, sequence_only: bool = False):
        import torch

        self.torch = torch
        self.lib = binding.require_gpu()
        self.device = torch.device(device)
        if forward_lanes not in (0, 1, 4):
            raise ValueError(f"forward_lanes must be 0 (the library's choice by batch size), 1 or 4, got {forward_lanes!r}")
        self.forward_lanes = int(forward_lanes)
        ncu = torch.cuda.get_device_properties(self.device).multi_processor_count
        quad = forward_lanes == 4 or (forward_lanes == 0 and (ntracks or 10_000) <= 32_768)
        if shared is None:  # naming a forward partition asks for the split; otherwise everything shares the chip
            shared = forward_cus is None
        self.shared = bool(shared)
        if shared:
            # no partition: forward passes and smoothers on streams that each own a hardware queue but may use every CU.
            # A lane-per-track forward wave holds 264 registers (one per SIMD by construction), a smoother wave 240, so
            # the smoother of one batch slots in beside the forward waves of the next ones and takes the issue slots they
            # leave (its waves mostly wait for memory).
            forward_cus = ncu
        if forward_cus is None:
            # shared=False, the round 1-2 split (kept for measurements): the fraction of the chip the forward passes get was
            # sized then, against a workgroup smoother that no longer exists -- five eighths for lane-per-track passes
            # (160 + 96 CUs), three quarters for quad-per-track ones (192 + 64).  With today's kernels the same split
            # measured 0.86 ms per step at 10 000 tracks against 0.68 shared; it is not re-tuned.
            forward_cus = (ncu * (3 if quad else 5) // (4 if quad else 8)) // 8 * 8
            # small devices / partitioned compute modes: keep at least one CU on either side of the split
            forward_cus = max(1, min(forward_cus if forward_cus > 0 else ncu // 2, ncu - 1))
        if forward_streams is None:
            # as many forward passes in flight as fill the partition's wave slots: a lane-per-track wave holds a SIMD's
            # whole register file, quad-per-track waves (256 VGPRs) fit two to a SIMD.  Quad passes: rounded up (the waves
            # of the last pass start as slots come free: 3 on 192 CUs beat 2).  Lane-per-track passes: rounded to nearest
            # (10 000 tracks on 160 CUs: 4.08 -> 4, 1.02 ms per step with 4 or 5; 12 500 tracks: 3.27 -> 3, 1.53 ms
            # against 1.68 with 4).
            nt = ntracks or 10_000
            waves = -(-nt * 4 // 64) if quad else -(-nt // 64)
            slots = forward_cus * (8 if quad else 4)
            if shared:  # fill the SIMDs (rounded up: the waves of the last pass start as slots come free), at most eight
                forward_streams = max(1, min(8, -(-slots // waves)))
            else:
                forward_streams = max(1, min(3, -(-slots // waves)) if quad else min(8, (2 * slots + waves) // (2 * waves)))
        if smoother_streams is None:
            # shared: measured at 10 000 and 12 500 tracks (profiles/r03_pipeline_sweeps.txt): six smoothers in flight keep
            # up with the forward passes (five were enough until the forward kernel lost its last lane reads: 6.96 against
            # 7.43e9 track-steps/s at 10 000 tracks); seven or eight change nothing.  A larger batch fills the chip with
            # fewer forward passes and needs as few smoothers beside them (and each buffer set is the larger for it:
            # 224 + 240 B per track-step, 23 GB at 100 000 x 500): never more smoother streams than forward streams, at least two.
            smoother_streams = max(2, min(6, forward_streams)) if shared else 2
        if sequence_only:
            # a pipeline for submit_sequence alone: a scheduled launch is one kernel on one stream however many windows it
            # covers (two streams: the next sequence's launch starts as the waves of this one leave), and every stream not
            # created is a hardware queue left to whatever else runs on the device
            forward_streams = min(forward_streams, 2)
        if not (0 < forward_cus < ncu) and not shared:
            raise ValueError(f"forward_cus must be in 1..{ncu - 1} (got {forward_cus}): the smoother needs CUs of its own")
        if forward_streams < 1 or smoother_streams < 1:
            raise ValueError("forward_streams and smoother_streams must be >= 1")
        self.forward_cus, self.smoother_cus = int(forward_cus), int(ncu if shared else ncu - forward_cus)
        self._raw = []
        self.fwd_streams, self.bwd_streams = [], []
        # unrestricted stream for the smoother of the last batch of a sequence; created here, not at first use, so
        # that a timed sequence never pays for it
        self._tail_stream = torch.cuda.Stream(self.device)
        self._count = 0
        self._batches = []  # weak references to the DeviceBatches that carry one of this pipeline's events
        self._schedules = {}  # item tables of scheduled forward launches, by shape (submit_sequence)
        self._sched_live = []  # _ScheduledLaunch records of the scheduled launches not yet synchronised
        self._sched_free = _WorkspacePool(torch, self.device, 1 << 20)  # tables and counters of retired launches
        self._sched_pinned = True  # page-locked host workspaces: the table is uploaded by a kernel (False: staged copy; tests)
        self._sched_free_bwd = _WorkspacePool(torch, self.device, 1 << 18)  # the same for the sequences' smoother launches
        self._sched_tile_smoothers = True  # one smoother launch per sequence, a wave per tile (False: a launch per window; tests)
        self.buffers_needed = forward_streams + smoother_streams + 1
        # time slices per forward pass (DeviceBatch.forward): the waves of the passes in flight re-balance over the SIMDs at
        # every slice boundary instead of once per pass (3.6-4.5 ms at 500 steps) -- what a short sequence of batches, or
        # a fleet of a few windows, loses at its ends
        self.slices = DEFAULT_SLICES if slices is None else int(slices)
        if self.slices < 1:
            raise ValueError("slices must be >= 1")
        # shared mode only: the last ``reserve_cus`` compute units (spread over the XCDs: mask bit n is CU n / 8 of XCD n % 8)
        # stay free of this pipeline's kernels -- room that a collective's own kernels can always find (multi-GPU runs)
        self.reserve_cus = int(reserve_cus) if shared else 0
        if not 0 <= self.reserve_cus < ncu:
            raise ValueError(f"reserve_cus must be in 0..{ncu - 1}, got {reserve_cus!r}")
        try:
            with torch.cuda.device(self.device):
                for first, count, n, out in ((0, self.forward_cus - self.reserve_cus, forward_streams, self.fwd_streams),
                                             (0 if shared else self.forward_cus, self.smoother_cus - self.reserve_cus,
                                              smoother_streams, self.bwd_streams)):
                    for _ in range(n):
                        h = C.c_void_p()
                        binding.check(self.lib.ste_stream_create_cu_range(first, count, C.byref(h)),
                                      "ste_stream_create_cu_range")
                        self._raw.append(h)
                        out.append(torch.cuda.ExternalStream(h.value, device=self.device))
        except BaseException:
            self.close()  # do not leak the streams created before the failing one
            raise
        # CU-masked streams own HSA queues of their own.  Left alive until the process exits they are torn down by the
        # HIP runtime's static destructors, after Python, torch and any profiler tool have finalised -- under rocprofv3
        # that order ended every pipelined run of round 1 in a SIGSEGV inside __cxa_finalize.  So the streams are
        # destroyed while everything is still up: close() / the context manager / __del__, and at the latest atexit.
        _live_pipelines.add(self)
        _register_atexit()
        # Every stream of a pipeline owns a hardware queue.  Past ~16 of them in a process the firmware multiplexes queues and
        # launches crawl (a 100 000-track fleet: 8.9 ms on 10 + 6 streams, 12.0 on 13 + 8, 28 on 16 + 8; profiles/r04_fleet_sweep.txt).
        nq = sum(len(q.fwd_streams) + len(q.bwd_streams) for q in _live_pipelines)
        if nq > MAX_PIPELINE_QUEUES:
            import warnings

            warnings.warn(f"{nq} pipeline streams are alive in this process (more than {MAX_PIPELINE_QUEUES}): each owns a hardware "
                          "queue, and beyond that many the GPU multiplexes them and every launch slows down; close() the "
                          "pipelines that are no longer used", RuntimeWarning, stacklevel=2)

    # single-stream names kept for callers that look at them
    @property
    def fwd_stream(self):
        return self.fwd_streams[0]

    @property
    def bwd_stream(self):
        return self.bwd_streams[0]

    def submit(self, db: "DeviceBatch", after_smoother=None, timing=None, final: bool = False, smooth: bool = True,
               slices: Optional[int] = None):
        """Queue forward + smoother of ``db``; returns the event that marks its smoother (and ``after_smoother``) done.

        ``after_smoother(stream)``: optional callable run with the smoother stream current, right after the smoother
        kernels are queued (the multi-GPU driver starts its all-gather of the smoothed positions there).  It may return
        an event; the next use of ``db``'s buffers then waits for that event too (a collective still reading them).
        ``smooth=False``: forward pass only.  ``slices``: time slices of this batch's forward pass (default: the pipeline's).
        ``timing``: optional list of four timing-enabled events, recorded before / after the forward kernel on its
        forward stream and before / after the smoother kernels on its smoother stream.
        ``final``: nothing follows this batch, so its smoother gets an unrestricted stream (the whole chip) instead of the
        smoother partition."""
        torch = self.torch
        self._require_open()
        if (db.noise is not None and self.forward_lanes == 4
                and not (db.struct.flags & (binding.STE_FLAG_LANES_1 | binding.STE_FLAG_LANES_4))):
            raise ValueError("this pipeline was built with forward_lanes=4 and the batch has per-track noise (Q_tracks / "
                             "R_tracks), which runs the lane-per-track mapping only: give the batch lanes=1 or use a "
                             "lane-per-track pipeline")
        k = self._count
        self._count += 1
        fwd_stream = self.fwd_streams[k % len(self.fwd_streams)]
        bwd_stream = self.bwd_streams[k % len(self.bwd_streams)]
        if final:
            bwd_stream = self._tail_stream
        self._wait_for_previous_use(db, fwd_stream)
        if timing is not None:
            timing[0].record(fwd_stream)
        # Lane mapping of the forward pass: with several passes sharing the partition a lane per track is the better
        # shape even for small batches -- half the instructions per track of the quad mapping, and the other passes'
        # waves fill the SIMDs a 157-wave pass leaves empty.  A mapping named by the batch itself (HostBatch.lanes) wins.
        flags = db.struct.flags
        if self.forward_lanes and not (flags & (binding.STE_FLAG_LANES_1 | binding.STE_FLAG_LANES_4)):
            db.struct.flags = flags | (binding.STE_FLAG_LANES_1 if self.forward_lanes == 1 else binding.STE_FLAG_LANES_4)
        try:
            db.forward(fwd_stream, slices=self.slices if slices is None else int(slices), mark=False)
        finally:
            db.struct.flags = flags
        ready = timing[1] if timing is not None else torch.cuda.Event()
        ready.record(fwd_stream)
        if not smooth:
            return self._set_done(db, ready)
        bwd_stream.wait_event(ready)
        if timing is not None:
            timing[2].record(bwd_stream)
        db.backward(bwd_stream, mark=False)
        if timing is not None:
            timing[3].record(bwd_stream)
        if after_smoother is not None:
            with torch.cuda.stream(bwd_stream):
                db._reader_done = after_smoother(bwd_stream)
        done = torch.cuda.Event()
        done.record(bwd_stream)
        return self._set_done(db, done)

    # -- steps that submit and submit_sequence share -----------------------------------------------------------------------
    def _require_open(self):
        if self.closed:
            raise RuntimeError("SmootherPipeline is closed")

    def _wait_for_previous_use(self, db: "DeviceBatch", stream):
        """``stream`` waits for whatever used ``db``'s buffers last."""
        if db._pipeline_done is not None:
            stream.wait_event(db._pipeline_done)  # the previous use of these buffers has drained
        else:
            # uploads queued by the constructor: an event it recorded then.  (Not wait_stream(current stream): that
            # records on the legacy default stream, which drains every blocking stream -- this pipeline's included.)
            stream.wait_event(db._uploaded)
        for name in ("_last_use", "_reader_done"):
            # kernels issued on this batch outside the pipeline (forward / backward / run on a stream of the caller's), or a
            # collective started by an earlier after_smoother that may still be reading its outputs
            e = getattr(db, name)
            if e is not None:
                stream.wait_event(e)
                setattr(db, name, None)

    def _set_done(self, db: "DeviceBatch", event):
        """``event`` marks ``db``'s buffers free again; close() / shrink() find the batch to take the event back."""
        if db._pipeline_done is None:
            self._batches.append(weakref.ref(db))
        db._pipeline_done = event
        return event

    def _drop_batch_events(self):
        """Take this pipeline's events off the batches that carry one (their streams are about to go)."""
        for ref in self._batches:
            db = ref()
            if db is not None:
                db._pipeline_done = None
        self._batches = []

    # -- many batches (or windows of a fleet) as ONE scheduled forward launch ---------------------------------------------
    def submit_sequence(self, dbs: Sequence["DeviceBatch"], smooth: bool = True, after_smoother=None, timing=None,
                        final: bool = True, stagger: float = 0.0, slice_steps: int = 0, timeout_s: float = 4.0,
                        tile_smoothers: Optional[bool] = None):
        """Queue forward + smoother of every batch of ``dbs`` -- distinct buffer sets, or the windows of one resident fleet --
        with ALL their forward passes as one launch of resident waves that work through a schedule of (64-track tile, time
        slice) items (``forward_schedule``; include/ste.h: ``ste_ukf_forward_sched_f64``).  One launch per batch makes a
        forward wave indivisible for a whole pass, so W batches of T tiles on S SIMDs cost ceil(W T / S) pass times; scheduled,
        they cost W T / S (rounded up to a slice).  Results are those of ``submit`` on every batch, bit for bit.

        Each batch's smoother goes on a smoother stream behind a one-wave gate that leaves when the batch's last tile has
        finished its last slice.  ``after_smoother(k, stream)``: optional, called for batch k with its smoother stream current,
        may return an event the batch's next use must wait for.  ``timing``: optional dict, gets ``forward`` = (start, end)
        timing events around the scheduled launch and ``smoothers`` = (start, end) around the smoother of every
        ``timing["every"]``-th batch (default 4: every record is a packet on the stream's queue between two launches).
        ``final``: nothing follows this sequence: its last smoother gets the unrestricted stream.
        ``tile_smoothers``: the smoothers of the whole sequence as ONE launch, a wave per 64-track tile that waits for its own
        tile's forward pass (``ste_urtss_backward_sched_f64``) instead of a gate and a launch per batch; needs batches of more
        than 4 096 tracks (the one-kernel smoother) and no ``after_smoother``.  Default: when ``final`` and no scheduled launch
        is in flight in front of this one (a job that is one sequence: a fleet, a short run).  Same bits either way.
        Returns the list of the batches' completion events."""
        self._require_open()
        dbs = list(dbs)
        if not dbs:
            return []
        self._validate_sequence(dbs)
        self._prune_finished()
        k = self._count
        self._count += 1
        fwd_stream = self.fwd_streams[k % len(self.fwd_streams)]
        for db in dbs:
            self._wait_for_previous_use(db, fwd_stream)
        structs = self._window_structs(dbs)
        plan = self._plan(structs, int(slice_steps) or binding.STE_SLICE_ALIGN, stagger)
        nbytes = int(self.lib.ste_ukf_forward_sched_workspace(*plan.table_shape()))
        launch, zeroed = self._take_workspace(nbytes, structs, plan.items, fwd_stream)
        self._wait_for_residency(launch, fwd_stream, timeout_s)
        self._launch_scheduled_forward(launch, plan, nbytes, fwd_stream, timeout_s, timing)
        if tile_smoothers is None:
            # measured (profiles/r05_scheduled_forward.txt): ONE sequence of 20 batches 14.5-14.7 ms with tile smoothers against
            # 15.0-15.5 with a smoother per window, a fleet the same either way; sequences that overlap (7 + 13) 15.1-15.3
            # against 14.5-14.7 -- so: when nothing follows this sequence and none is in flight before it
            tile_smoothers = self._sched_tile_smoothers and final and launch.prev_counters is None
        # One smoother launch for the whole sequence -- when every window takes the one-kernel smoother and nothing has to
        # happen behind individual windows; otherwise a gate and a smoother launch per window.
        if (smooth and after_smoother is None and tile_smoothers and all(_one_kernel_smoother(st) for st in structs)
                and len({bool(st.sog_rate_rts or st.cog_rate_rts) for st in structs}) == 1):
            bwd_stream = self._tail_stream if final else self.bwd_streams[k % len(self.bwd_streams)]
            return self._launch_tile_smoothers(dbs, launch, plan, zeroed, bwd_stream, timeout_s, timing)
        return self._launch_window_smoothers(dbs, launch, plan, zeroed, k, final, smooth, after_smoother, timeout_s, timing)

    def _validate_sequence(self, dbs):
        if self.forward_lanes == 4:
            raise ValueError("scheduled forward launches are lane-per-track (this pipeline was built with forward_lanes=4)")
        if any(db.noise is not None for db in dbs):
            raise ValueError("scheduled launches have no per-track noise (Q_tracks / R_tracks): submit() the batches one by one")
        seen = set()
        for db in dbs:
            key = (db.fwd_mean.data_ptr(), db.ntracks)
            if key in seen:
                raise ValueError("submit_sequence: every batch of a sequence needs histories of its own (a buffer set appears twice)")
            seen.add(key)

    def _prune_finished(self):
        """For a caller that never synchronises the pipeline: retire the launches that have long finished (their tables and
        counters are only kept for the error word, which is looked at now)."""
        if len(self._sched_live) <= 8:
            return
        done_ones = [e for e in self._sched_live if e.finished()]
        if done_ones:
            keep = [e for e in self._sched_live if not any(e is d for d in done_ones)]
            self._sched_live = done_ones
            try:
                self._check_scheduled()
            finally:
                self._sched_live = keep

    @staticmethod
    def _window_structs(dbs):
        """The batch structs of a scheduled launch's windows: copies, lane-per-track, no step range of their own."""
        structs = (binding.SteUkfBatchF64 * len(dbs))()
        for i, db in enumerate(dbs):
            st = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
            st.flags = (st.flags & ~binding.STE_FLAG_LANES_4) | binding.STE_FLAG_LANES_1
            st.step_begin = st.step_end = 0
            structs[i] = st
        return structs

    def _plan(self, structs, step: int, stagger: float) -> _SequencePlan:
        """Tiles, slices and waves of a sequence, and ``forward_schedule``'s item table for them, cached by shape."""
        ntiles = [-(-int(st.B) // 64) for st in structs]
        nslices = [max(1, -(-int(st.Nmax) // step)) for st in structs]
        nwaves = 4 * (self.forward_cus - self.reserve_cus)  # one per SIMD this pipeline's forward streams may use
        key = (tuple(ntiles), tuple(nslices), nwaves, float(stagger))
        items = self._schedules.get(key)
        if items is None:
            items = np.ascontiguousarray(forward_schedule(ntiles, nslices, nwaves, stagger=stagger))
            if len(self._schedules) > 16:
                self._schedules.clear()
            self._schedules[key] = items
        return _SequencePlan(step, ntiles, nslices, nwaves, key, items)

    def _tile_order(self, plan: _SequencePlan):
        """``smoother_tile_order`` of the plan's table, cached beside it."""
        okey = ("order",) + plan.key
        order = self._schedules.get(okey)
        if order is None:
            order = self._schedules[okey] = smoother_tile_order(plan.items, plan.ntiles)
        return order

    def _take_workspace(self, nbytes, structs, items, fwd_stream):
        """Tables and counters for a launch, from the launches retired before (synchronize / _prune_finished), the counters
        zeroed on the forward stream.  Returns the launch's record and the event behind the zeroing."""
        torch, n = self.torch, len(structs)
        with torch.cuda.stream(fwd_stream):
            host_ws, dev_ws, counters_all = self._sched_free.take(nbytes, n + 2, pinned=self._sched_pinned)
            counters_all[:n + 2].zero_()
            zeroed = torch.cuda.Event()
            zeroed.record(fwd_stream)
        return _ScheduledLaunch(host_ws, dev_ws, counters_all, counters_all[:n + 1], structs, items), zeroed

    def _wait_for_residency(self, launch: _ScheduledLaunch, fwd_stream, timeout_s):
        """One scheduled launch becomes resident at a time: every wave of a launch may wait for any other, so two launches
        dispatched together -- this one while the one before it (of this or another pipeline) is still finding its SIMDs
        behind a backlog of smoother waves -- could each hold part of the chip and wait for the rest.  The launch before
        this one counts its waves as they begin; a one-wave gate on this launch's stream waits for all of them, and this
        launch's record keeps the counters that gate reads."""
        prev = _last_scheduled.get(self.device.index or 0)
        if prev is None or prev.ready.query():
            return
        launch.prev_counters = prev.counters
        binding.check(self.lib.ste_stream_wait_counter(prev.counters.data_ptr() + 4 * prev.started, prev.nwaves,
                                                       launch.counters.data_ptr() + 4 * len(launch.structs),
                                                       float(timeout_s) * 4, C.c_void_p(fwd_stream.cuda_stream)),
                      "ste_stream_wait_counter")

    def _launch_scheduled_forward(self, launch: _ScheduledLaunch, plan: _SequencePlan, nbytes, fwd_stream, timeout_s, timing):
        """The forward launch itself; records it as live and as the device's last scheduled launch."""
        torch, n, items = self.torch, len(launch.structs), plan.items
        counters = launch.counters.data_ptr()
        sc = binding.SteFwdSchedF64()
        sc.nwindows, sc.windows, sc.slice_steps = n, C.addressof(launch.structs), plan.step
        sc.nwaves, sc.nrounds, sc.items = plan.nwaves, int(items.shape[0]), items.ctypes.data
        sc.host_ws, sc.dev_ws, sc.ws_bytes = launch.host_ws.data_ptr(), launch.dev_ws.data_ptr(), nbytes
        sc.window_done, sc.error, sc.timeout_s = counters, counters + 4 * n, float(timeout_s)
        sc.started = launch.counters_all.data_ptr() + 4 * (n + 1)
        if timing is not None:
            timing["forward"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            timing["smoothers"] = []
            timing["forward"][0].record(fwd_stream)
        binding.check(self.lib.ste_ukf_forward_sched_f64(C.byref(sc), C.c_void_p(fwd_stream.cuda_stream)),
                      "ste_ukf_forward_sched_f64")
        if timing is not None:
            timing["forward"][1].record(fwd_stream)
        launch.ready = torch.cuda.Event()
        launch.ready.record(fwd_stream)
        self._sched_live.append(launch)
        _last_scheduled[self.device.index or 0] = _LastScheduled(launch.counters_all, n + 1, plan.nwaves, launch.ready, id(self))

    def _launch_tile_smoothers(self, dbs, launch: _ScheduledLaunch, plan: _SequencePlan, zeroed, bwd_stream, timeout_s, timing):
        """The smoothers of the whole sequence as ONE launch on ``bwd_stream``, a wave per tile that waits for ITS tile's
        forward pass (include/ste.h: ste_urtss_backward_sched_f64).  Returns the windows' completion events."""
        torch, n = self.torch, len(dbs)
        order = self._tile_order(plan)
        error = launch.counters.data_ptr() + 4 * n
        bwd_stream.wait_event(zeroed)
        # behind the forward launch's residency: a waiting smoother wave must not sit where a forward wave still has to go
        binding.check(self.lib.ste_stream_wait_counter(launch.counters_all.data_ptr() + 4 * (n + 1), plan.nwaves, error,
                                                       float(timeout_s) * 4, C.c_void_p(bwd_stream.cuda_stream)),
                      "ste_stream_wait_counter")
        sbytes = int(self.lib.ste_urtss_backward_sched_workspace(n, int(order.shape[0])))
        with torch.cuda.stream(bwd_stream):
            s_host, s_dev, _ = self._sched_free_bwd.take(sbytes, pinned=self._sched_pinned)
        bs = binding.SteBwdSchedF64()
        bs.nwindows, bs.windows, bs.slice_steps = n, C.addressof(launch.structs), plan.step
        bs.nitems, bs.items = int(order.shape[0]), order.ctypes.data
        bs.host_ws, bs.dev_ws, bs.ws_bytes = s_host.data_ptr(), s_dev.data_ptr(), sbytes
        bs.progress = launch.dev_ws.data_ptr() + int(self.lib.ste_ukf_forward_sched_progress_offset(*plan.table_shape()))
        bs.error, bs.timeout_s = error, float(timeout_s) * 4
        if timing is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            timing["smoothers"].append(ev)
            timing["tile_smoothers"] = True
            ev[0].record(bwd_stream)
        binding.check(self.lib.ste_urtss_backward_sched_f64(C.byref(bs), C.c_void_p(bwd_stream.cuda_stream)),
                      "ste_urtss_backward_sched_f64")
        if timing is not None:
            ev[1].record(bwd_stream)
        done = torch.cuda.Event()
        done.record(bwd_stream)
        launch.smoother = _TileSmootherLaunch(s_host, s_dev, order)
        for db in dbs:
            launch.events.append(self._set_done(db, done))
        return launch.events

    def _launch_window_smoothers(self, dbs, launch: _ScheduledLaunch, plan: _SequencePlan, zeroed, k, final, smooth,
                                 after_smoother, timeout_s, timing):
        """A one-wave gate and a smoother launch per window, round-robin over the smoother streams (``smooth=False``: none, a
        window is done when the forward launch is).  Returns the windows' completion events."""
        torch, n = self.torch, len(dbs)
        counters = launch.counters.data_ptr()
        waited = set()
        for i, db in enumerate(dbs):
            if not smooth:
                launch.events.append(self._set_done(db, launch.ready))
                continue
            bwd_stream = self.bwd_streams[(k + i) % len(self.bwd_streams)]
            if final and i == n - 1:
                bwd_stream = self._tail_stream
            if id(bwd_stream) not in waited:  # the counters were zeroed on the forward stream: no gate may read them earlier
                bwd_stream.wait_event(zeroed)
                waited.add(id(bwd_stream))
            binding.check(self.lib.ste_stream_wait_counter(counters + 4 * i, plan.ntiles[i], counters + 4 * n,
                                                           float(timeout_s) * 4, C.c_void_p(bwd_stream.cuda_stream)),
                          "ste_stream_wait_counter")
            timed = timing is not None and i % int(timing.get("every", 4)) == 0
            if timed:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                timing["smoothers"].append(ev)
                ev[0].record(bwd_stream)
            db.backward(bwd_stream, mark=False)
            if timed:
                ev[1].record(bwd_stream)
            if after_smoother is not None:
                with torch.cuda.stream(bwd_stream):
                    db._reader_done = after_smoother(i, bwd_stream)
            done = torch.cuda.Event()
            done.record(bwd_stream)
            launch.events.append(self._set_done(db, done))
        return launch.events

    def _check_scheduled(self):
        """After a synchronisation: the error words of the scheduled launches issued since the last one; their tables and
        counters go back to the pools."""
        live, self._sched_live = self._sched_live, []
        bad = [e.error_word() for e in live]
        self._sched_free.give((e.host_ws, e.dev_ws, e.counters_all) for e in live)
        self._sched_free_bwd.give((e.smoother.host_ws, e.smoother.dev_ws, None) for e in live if e.smoother is not None)
        if any(bad):
            raise binding.SteError("a scheduled forward launch could not progress (error word %s: 1 = a forward wave, 2 = a smoother "
                                   "gate waited longer than its bound); results of that sequence are incomplete" % bad)

    def synchronize(self):
        for s in self.fwd_streams + self.bwd_streams:
            s.synchronize()
        if self._tail_stream is not None:
            self._tail_stream.synchronize()
        if self._sched_live:
            self._check_scheduled()

    def shrink(self, forward_streams: int, smoother_streams: int):
        """Drain the pipeline and destroy all but its first ``forward_streams`` forward and ``smoother_streams`` smoother
        streams: the hardware queues of a pipeline that goes on with scheduled launches only (they need two forward streams,
        one when sequences do not overlap; tile smoothers need one smoother stream) go back to the device without a new
        pipeline -- new queues -- being built."""
        if forward_streams < 1 or smoother_streams < 1:
            raise ValueError("forward_streams and smoother_streams must be >= 1")
        self.synchronize()
        self._drop_batch_events()
        _forget_scheduled(id(self))
        drop = self.fwd_streams[forward_streams:] + self.bwd_streams[smoother_streams:]
        self.fwd_streams, self.bwd_streams = self.fwd_streams[:forward_streams], self.bwd_streams[:smoother_streams]
        gone = {int(st.cuda_stream) for st in drop}
        del drop
        keep = []
        for h in self._raw:
            if h is not None and h.value and int(h.value) in gone:
                self.lib.ste_stream_destroy(h)
            else:
                keep.append(h)
        self._raw = keep
        self.buffers_needed = len(self.fwd_streams) + len(self.bwd_streams) + 1

    @property
    def closed(self) -> bool:
        return not self._raw and not self.fwd_streams and not self.bwd_streams

    def close(self):
        """Drain and destroy the CU-masked streams.  Idempotent; the pipeline cannot be used afterwards."""
        try:
            if self.fwd_streams or self.bwd_streams or self._tail_stream is not None:
                self.synchronize()
        finally:
            # the events recorded on these streams and the ExternalStream wrappers go first, then the streams themselves
            self._drop_batch_events()
            self._sched_live = []
            self._sched_free.free, self._sched_free_bwd.free = [], []
            _forget_scheduled(id(self))
            self.fwd_streams, self.bwd_streams, self._tail_stream = [], [], None
            raw, self._raw = self._raw, []
            for h in raw:
                if h is not None and h.value:
                    self.lib.ste_stream_destroy(h)
            _live_pipelines.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: nothing left to report to
            pass


_live_pipelines = weakref.WeakSet()
_atexit_registered = False
_pool = None


def _staging_pool():
    """A few threads for the host-side staging copies of fleet uploads (NumPy slice copies release the GIL)."""
    global _pool
    if _pool is None:
        import os
        from concurrent.futures import ThreadPoolExecutor

        _pool = ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0)) // 2)), thread_name_prefix="ste-stage")
    return _pool
# Time slices per pipelined forward pass when SmootherPipeline is not told.  One: slices are bit-identical and let the waves
# of the passes in flight re-balance at every boundary, but a stream's next slice waits for ALL waves of the one before, and
# with every window advancing in step no smoother has anything to do until the end -- measured (10 000-track batches, 7 + 6
# streams): 0.672 / 0.715 / 0.768 ms per step at 1 / 2 / 4 slices over 100 steps, 0.804 / 0.781 / 0.819 at the driver's 20;
# a 100 000-track fleet: 8.6 / 8.6 / 8.5 ms (profiles/r04_pipeline_sweeps.txt, r04_fleet_sweep.txt).
DEFAULT_SLICES = 1
MAX_PIPELINE_QUEUES = 16


def _close_live_pipelines():
    for pipe in list(_live_pipelines):
        try:
            pipe.close()
        except Exception:
            pass


def _register_atexit():
    # Registered when the first pipeline is built, i.e. after torch has been imported: atexit runs handlers in reverse
    # order of registration, so this one runs BEFORE torch's own teardown and the streams are destroyed while the HIP
    # runtime, torch and any profiler tool are still up.
    global _atexit_registered
    if not _atexit_registered:
        atexit.register(_close_live_pipelines)
        _atexit_registered = True


FIR_MAX_WINDOW, SAVGOL_MAX_ORDER = 128, 8  # include/ste.h: ste_fir_f64.window; the order is a limit of the host tables


@dataclasses.dataclass(frozen=True)
class FirFilter:
    """A linear smoother in the form of ``struct ste_fir_f64`` (include/ste.h): interior row i is
    ``sum_k taps[k] y[i - left + k]`` with zeros outside the series; with ``nedge = h > 0`` row i < h is
    ``sum_k edge[i][k] y[k]`` over the first ``window`` samples and row n - 1 - r its mirror image over the last."""

    window: int
    left: int
    nedge: int
    taps: np.ndarray  # (window,)
    edge: np.ndarray  # (nedge, window)


def _check_window(w, who):
    if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 2 <= w <= FIR_MAX_WINDOW:
        raise ValueError(f"{who}: the window must be an integer in 2..{FIR_MAX_WINDOW}, got {w!r}")
    return int(w)


def box_filter(w: int) -> FirFilter:
    """The centred moving average of the reference's ``utils.smooth``: ``np.convolve(y, ones(w) / w, "same")``, zero padded at
    both ends (utils.py:150-172).  Output i of "same" is element i + (w - 1) // 2 of the full convolution, the sum over
    y[i - w // 2 .. i + (w - 1) // 2]: ``left = w // 2``, for even w too."""
    w = _check_window(w, "box_filter")
    return FirFilter(window=w, left=w // 2, nedge=0, taps=np.full(w, 1.0 / w), edge=np.zeros((0, w)))


def _polyfit_weights(w: int, p: int, x0):
    """Weights c with ``sum_k c[k] y[k]`` = the least-squares polynomial of degree p through (k, y[k]), k < w, evaluated at
    x0 -- in exact rational arithmetic by the normal equations, each weight rounded once to double."""
    from fractions import Fraction

    x0 = Fraction(x0)
    G = [[Fraction(sum(k ** (a + b) for k in range(w))) for b in range(p + 1)] + [x0 ** a] for a in range(p + 1)]
    for c in range(p + 1):  # Gauss-Jordan on [A^T A | x0^a]; A^T A is positive definite for p < w, so no pivot is zero
        piv = G[c][c]
        G[c] = [v / piv for v in G[c]]
        for r in range(p + 1):
            if r != c and G[r][c] != 0:
                f = G[r][c]
                G[r] = [vr - f * vc for vr, vc in zip(G[r], G[c])]
    u = [G[a][p + 1] for a in range(p + 1)]
    return np.array([float(sum(u[a] * Fraction(k) ** a for a in range(p + 1))) for k in range(w)])


def savgol_filter_table(w: int, p: int) -> FirFilter:
    """``scipy.signal.savgol_filter(y, w, p)`` (``deriv=0``, ``mode="interp"``) as a table.  Edge rows (h = w // 2 at either
    end): the polynomial of degree p fitted to the first (last) w samples, evaluated at the row.  Interior rows: the fit over
    the window evaluated at its centre node for odd w (``left = h``); for even w scipy's output is the fit over
    y[i - h + 1 .. i + h] evaluated at h - 1/2 in window coordinates, half a sample before row i (``left = h - 1``), and this
    reproduces it.  The weights are exact rationals rounded once, so the table depends on no LAPACK."""
    from fractions import Fraction

    w = _check_window(w, "savgol_filter_table")
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= p <= SAVGOL_MAX_ORDER or p >= w:
        raise ValueError(f"savgol_filter_table: the order must be an integer in 0..{SAVGOL_MAX_ORDER} and below the window, got {p!r}")
    p, h = int(p), w // 2
    centre, left = (Fraction(h), h) if w % 2 else (Fraction(2 * h - 1, 2), h - 1)
    return FirFilter(window=w, left=left, nedge=h, taps=_polyfit_weights(w, p, centre),
                     edge=np.stack([_polyfit_weights(w, p, i) for i in range(h)]))


def _fir_struct(f: FirFilter, circular: bool, dev, keep: list):
    """``ste_fir_f64`` of a FirFilter with its tables uploaded to ``dev``; ``keep`` holds the tensors alive."""
    import torch

    taps = np.ascontiguousarray(f.taps, dtype=np.float64)
    edge = np.ascontiguousarray(f.edge, dtype=np.float64).reshape(-1, f.window)
    if taps.shape != (f.window,) or edge.shape[0] != f.nedge:
        raise ValueError("filter: taps must have `window` entries and edge `nedge` rows of `window`")
    s = binding.SteFirF64()
    s.window, s.left, s.nedge, s.circular = int(f.window), int(f.left), int(f.nedge), int(bool(circular))
    t_taps = torch.from_numpy(taps).to(dev)
    keep.append(t_taps)
    s.taps = t_taps.data_ptr()
    if f.nedge > 0:
        t_edge = torch.from_numpy(edge).to(dev)
        keep.append(t_edge)
        s.edge = t_edge.data_ptr()
    return s


def prepare_observations(lons: Sequence, lats: Sequence, gaps: Sequence, model: str = "wgs84", device="cuda:0", *,
                         smooth_sog: Optional[FirFilter] = None, smooth_cog: Optional[FirFilter] = None,
                         cog_circular: bool = False):
    """Speed / course over ground and their rates for many tracks in one launch (``ste_track_prep_f64``).

    ``lons[b]``, ``lats[b]`` (length T_b, degrees) and ``gaps[b]`` (length T_b - 1, hours) are what ``ShipTrack.read_csv``
    returns.  ``model`` is ``"wgs84"`` (the ShipTrack defaults, geographiclib_distance / _heading) or ``"sphere"``
    (haversine_formula / heading).  Returns one dict per track with ``sog, cog, sog_rate, cog_rate`` (length T_b),
    ``z`` (4, T_b) = the result of ``get_measurements(include_sog=True, include_cog=True)`` (ship_track.py:197-338) and
    ``status`` (always 0 since 0.3.1: the WGS84 model is Karney's solver, which converges on every leg).

    ``smooth_sog`` / ``smooth_cog`` (a ``FirFilter``: ``box_filter(k)`` is the reference CLI's ``"smooth": k``,
    ``savgol_filter_table(w, p)`` scipy's ``savgol_filter``) smooth that series on the device BEFORE the rates and ``z`` are
    formed (``ste_track_prep_smooth_f64``); the dicts then also hold the unsmoothed ``raw_sog`` and ``raw_cog``.
    ``cog_circular`` makes the course filter work on differences wrapped into [-180, 180], so that a course through north is
    not averaged through south; off, courses are plain numbers as in the reference.  A track shorter than a filter's window
    raises ``ValueError``.
    """
    import torch

    if cog_circular and smooth_cog is None:
        raise ValueError("cog_circular needs smooth_cog")
    lib = binding.require_gpu()
    models = {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}
    if model not in models:
        raise ValueError(f"model must be one of {sorted(models)}, got {model!r}")
    B = len(lons)
    if B == 0:
        return []
    nobs = np.asarray([len(v) for v in lons], dtype=np.int32)
    for b in range(B):
        if len(lats[b]) != nobs[b] or len(gaps[b]) != nobs[b] - 1:
            raise ValueError(f"track {b}: need len(lat) == len(lon) and len(gaps) == len(lon) - 1")
        if nobs[b] < 2:
            raise IndexError(f"track {b} has fewer than 2 observations (ship_track.py:220 indexes sog[-1])")
    for name, f in (("smooth_sog", smooth_sog), ("smooth_cog", smooth_cog)):
        if f is not None and nobs.min() < f.window:
            b = int(np.argmax(nobs < f.window))
            raise ValueError(f"track {b} has {nobs[b]} observations, fewer than the window of {name} ({f.window})")
    T = int(nobs.max())
    lon = np.zeros((T, B))
    lat = np.zeros((T, B))
    gap = np.ones((max(T - 1, 1), B))
    for b in range(B):
        lon[: nobs[b], b] = lons[b]
        lat[: nobs[b], b] = lats[b]
        gap[: nobs[b] - 1, b] = gaps[b]
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    t_n, t_lon, t_lat, t_gap = up(nobs), up(lon), up(lat), up(gap)
    outs = torch.empty((4, T, B), dtype=torch.float64, device=dev)
    z = torch.empty((T, 4, B), dtype=torch.float64, device=dev)
    s = binding.StePrepBatchF64()
    s.B, s.Tmax, s.model = B, T, models[model]
    s.nobs, s.lon, s.lat, s.gap = t_n.data_ptr(), t_lon.data_ptr(), t_lat.data_ptr(), t_gap.data_ptr()
    s.sog, s.cog, s.sog_rate, s.cog_rate = (outs[i].data_ptr() for i in range(4))
    s.z = z.data_ptr()
    st = torch.zeros((B,), dtype=torch.int32, device=dev)
    s.status = st.data_ptr()
    stream = torch.cuda.current_stream(dev)
    raw = None
    if smooth_sog is None and smooth_cog is None:
        binding.check(lib.ste_track_prep_f64(C.byref(s), C.c_void_p(stream.cuda_stream)), "ste_track_prep_f64")
    else:
        keep = []
        firs = [None if f is None else C.byref(_fir_struct(f, circ, dev, keep))
                for f, circ in ((smooth_sog, False), (smooth_cog, cog_circular))]
        raw = torch.empty((2, T, B), dtype=torch.float64, device=dev)
        binding.check(lib.ste_track_prep_smooth_f64(C.byref(s), firs[0], firs[1], raw[0].data_ptr(), raw[1].data_ptr(),
                                                    C.c_void_p(stream.cuda_stream)), "ste_track_prep_smooth_f64")
        raw = raw.cpu().numpy()  # synchronises: the tables in `keep` have been read
        del keep
    h = outs.cpu().numpy()
    zh = z.cpu().numpy()
    sth = st.cpu().numpy()
    if sth.any():
        import warnings

        warnings.warn(f"observation preparation flagged track(s) {np.flatnonzero(sth).tolist()} (status {sth[sth != 0].tolist()})",
                      RuntimeWarning, stacklevel=2)
    res = []
    for b in range(B):
        n = nobs[b]
        res.append({"sog": h[0, :n, b].copy(), "cog": h[1, :n, b].copy(), "sog_rate": h[2, :n, b].copy(),
                    "cog_rate": h[3, :n, b].copy(), "z": np.ascontiguousarray(zh[:n, :, b].T), "status": int(sth[b])})
        if raw is not None:
            res[-1].update(raw_sog=raw[0, :n, b].copy(), raw_cog=raw[1, :n, b].copy())
    return res


def prepare_ship_tracks(ship_tracks: Sequence, device="cuda:0", *, smooth_sog: Optional[FirFilter] = None,
                        smooth_cog: Optional[FirFilter] = None, cog_circular: bool = False):
    """Fill ``sog, cog, sog_rate, cog_rate, z`` of every ShipTrack (already ``read_csv``'d) in one launch -- what the
    reference does per ship with calculate_cog / calculate_sog / calculate_*_rate / get_measurements(True, True)
    (examples/example_ukf_rts_smoother_batch.py:33-40).  The distance / heading pair configured on each ShipTrack
    selects the model; anything but the two pairs the reference ships raises.  ``smooth_sog``, ``smooth_cog`` and
    ``cog_circular`` are those of ``prepare_observations``: the fields then hold the smoothed series and what is built on
    them, as after the reference CLI's ``"smooth"`` step (cli/main_cli.py:99-109)."""
    from . import utils

    pairs = {(utils.geographiclib_distance, utils.geographiclib_heading): "wgs84",
             (utils.haversine_formula, utils.heading): "sphere"}
    groups = {}
    for i, st in enumerate(ship_tracks):
        key = pairs.get((st.calc_distance_func, st.calc_heading_func))
        if key is None:
            raise ValueError("prepare_ship_tracks supports the (geographiclib_distance, geographiclib_heading) and "
                             "(haversine_formula, heading) pairs only; call ShipTrack.calculate_* for custom functions")
        groups.setdefault(key, []).append(i)
    for model, idx in groups.items():
        res = prepare_observations([ship_tracks[i].lon for i in idx], [ship_tracks[i].lat for i in idx],
                                   [ship_tracks[i].dts for i in idx], model=model, device=device, smooth_sog=smooth_sog,
                                   smooth_cog=smooth_cog, cog_circular=cog_circular)
        for i, r in zip(idx, res):
            st = ship_tracks[i]
            st.sog, st.cog, st.sog_rate, st.cog_rate, st.z = r["sog"], r["cog"], r["sog_rate"], r["cog_rate"], r["z"]
    return ship_tracks


def run_batch(hb: HostBatch, device="cuda:0", smooth: bool = True, fuse_gains: bool = True, outputs=None,
              sm_pos: bool = False):
    """Convenience: upload, run forward (+ smoother) as ONE launch each, download.  Returns a dict of NumPy arrays (tracks
    in the caller's order).  ``outputs``: which histories to bring back -- any of "means", "covs", "means_smoothed",
    "covs_smoothed" (default: all that were computed); "status" and "nsteps" always come along.  A fleet larger than a
    chip-full of waves belongs in ``run_fleet``."""
    return _run_batch(hb, device, smooth, fuse_gains, outputs, sm_pos)[0]


def _run_batch(hb, device, smooth, fuse_gains, outputs, sm_pos):
    db = DeviceBatch(hb, device=device, alloc_smoothed=smooth, fuse_gains=fuse_gains, sm_pos=sm_pos)
    if smooth:
        if hb.sog_rate_rts is not None and np.isnan(hb.sog_rate_rts[:, (hb.host_status == 0) if hb.host_status is not None else slice(None)]).any():
            raise IndexError("smoother rate expansion too short for at least one track (unscented.py:287-292,310)")
        db.run()
    else:
        db.forward()
    if outputs is None:
        outputs = ("means", "covs") + (("means_smoothed", "covs_smoothed") if smooth else ())
    inv = None
    if hb.order is not None:  # back to the caller's track order, on the device
        inv = np.empty_like(hb.order)
        inv[hb.order] = np.arange(len(hb.order))
    out = db.download(outputs, None if inv is None else db.torch.from_numpy(inv).to(db.device))
    status = db.status_host()
    if hb.host_status is not None:
        status = status | hb.host_status
    nsteps = hb.nsteps.copy()
    out["status"], out["nsteps"] = (status, nsteps) if inv is None else (status[inv], nsteps[inv])
    return out, db


def sample_tracks(hb_or_db, nsamples: int, seed: int = 0, device="cuda:0"):
    """``nsamples`` posterior tracks per track of a batch, drawn from the joint smoothing posterior on the device
    (``DeviceBatch.sample_smoothed``).  Given a ``HostBatch`` it uploads it and runs the forward pass first; given a
    ``DeviceBatch`` (or a window of one) it samples from the forward pass that batch holds.  Returns
    ``(samples, status)``: samples (S, B, Nmax+1, 4) as NumPy, track-major like ``download`` and in the batch's slot
    order (``hb.order`` maps slots to the caller's tracks), rows past ``nsteps[b]`` are padding; status (B,) int32, the
    sampler's own STE_STATUS_* bits per track."""
    if isinstance(hb_or_db, DeviceBatch):
        db = hb_or_db
    else:
        db = DeviceBatch(hb_or_db, device=device)
        db.forward()
    t = db.sample_smoothed(nsamples, seed=seed)
    dev_t = t.permute(0, 3, 1, 2).contiguous()
    status = db.sample_status.cpu().numpy()
    return dev_t.cpu().numpy(), status


def _posterior_batch(hb_or_db, nsamples, chunk, device, who: str):
    """What a ``*_statistics`` function samples from: a ``HostBatch`` is uploaded and ``run()``, a ``DeviceBatch`` (or a
    window of one) is taken to hold a completed ``run()``.  Returns (batch, nsamples, chunk), the two as checked ints."""
    nsamples, chunk = int(nsamples), int(chunk)
    if nsamples < 1 or chunk < 1:
        raise ValueError(f"nsamples and chunk must be >= 1, got {nsamples!r} and {chunk!r}")
    if isinstance(hb_or_db, DeviceBatch):
        db = hb_or_db
    else:
        db = DeviceBatch(hb_or_db, device=device)
        db.run()
    if db.sm_mean is None:
        raise ValueError(f"{who}() needs the smoothed track, and this batch was built with alloc_smoothed=False")
    return db, nsamples, chunk


class _PosteriorChunks:
    """The posterior-sampling loop of the ``*_statistics`` functions: ``nsamples`` posterior tracks of ``db``, ``chunk`` at
    a time.  Iterating yields (i, n, samples): samples i .. i+n-1 as ``sample_smoothed`` returned them, in the one draw
    buffer of ``min(chunk, nsamples)`` samples, so a chunk is gone when the next is drawn.  One generator, seeded once,
    fills the buffer chunk after chunk: the draws depend on ``(seed, chunk)``, and with ``chunk >= nsamples`` they are those
    of ``sample_smoothed(nsamples, seed)``.  ``draws(z, i)``, if given, fills a chunk's buffer ``z`` with the standard
    normal draws of samples i .. i+n-1 in place of the generator.  ``status`` (B,) int32 gathers the sampler's STE_STATUS_*
    bits, after the loop body has run for the chunk."""

    def __init__(self, db: DeviceBatch, nsamples: int, seed: int, chunk: int, draws=None):
        torch = db.torch
        self.db, self.nsamples, self.chunk, self.draws = db, nsamples, chunk, draws
        self.gen = torch.Generator(device=db.device)
        self.gen.manual_seed(int(seed))
        self.buf = torch.empty((min(chunk, nsamples), int(db.struct.Nmax) + 1, 4, db.ntracks), dtype=torch.float64,
                               device=db.device)
        self.status = torch.zeros((db.ntracks,), dtype=torch.int32, device=db.device)

    def __iter__(self):
        for i in range(0, self.nsamples, self.chunk):
            n = min(self.chunk, self.nsamples - i)
            z = self.buf[:n]
            if self.draws is None:
                z.normal_(generator=self.gen)
            else:
                self.draws(z, i)
            yield i, n, self.db.sample_smoothed(n, draws=z)
            self.status |= self.db.sample_status


def path_statistics(hb_or_db, nsamples: int, seed: int = 0, chunk: int = 16, model: str = "sphere", line_axis=None,
                    line_value=None, quantiles=(0.05, 0.5, 0.95), device="cuda:0"):
    """Distance sailed -- and, given a line, the time of its first crossing -- with the uncertainty of the smoothing posterior,
    per track: ``nsamples`` posterior tracks are drawn (``DeviceBatch.sample_smoothed``), reduced to their path quantities
    (``DeviceBatch.path_metrics``) and discarded, ``chunk`` samples at a time, so ``nsamples`` is not bounded by memory (one
    draw buffer of ``min(chunk, nsamples)`` samples is allocated once and refilled from one generator; what stays is
    (nsamples, B)).  Given a ``HostBatch`` it uploads it and runs the forward pass and the smoother first; a ``DeviceBatch``
    (or a window of one) is taken to hold a completed ``run()``.  ``model``, ``line_axis`` and ``line_value`` as in
    ``path_metrics``.

    Returns a dict of NumPy arrays in the batch's slot order (``hb.order`` maps slots to the caller's tracks):
    ``distance_smoothed`` (B,), the distance of the smoothed track ``sm_mean``; ``distance`` (nsamples, B);
    ``distance_mean``, ``distance_std`` (B,; ddof = 1, 0 for a single sample) and ``distance_quantiles`` (len(quantiles), B);
    with a line ``cross_time`` (nsamples, B), NaN where a sample never crosses, ``cross_prob`` (B,), the fraction of samples
    that cross, and ``cross_time_quantiles`` (len(quantiles), B) over the samples that cross, NaN where none does; and
    ``status`` (B,), the sampler's STE_STATUS_* bits.

    The draws depend on ``(seed, chunk)``: the generator is seeded once and every chunk takes the next draws in the layout of
    a ``chunk``-sample buffer.  With ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``."""
    import warnings

    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "path_statistics")
    torch = db.torch
    B = db.ntracks
    line = dict(line_axis=line_axis, line_value=line_value)
    smoothed = db.path_metrics(db.sm_mean, model=model)["distance"][0]
    dist = torch.empty((nsamples, B), dtype=torch.float64, device=db.device)
    ctime = torch.empty((nsamples, B), dtype=torch.float64, device=db.device) if line_axis is not None else None
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for i, n, samples in chunks:
        m = db.path_metrics(samples, model=model, **line)
        dist[i:i + n] = m["distance"]
        if ctime is not None:
            ctime[i:i + n] = m["cross_time"]
    status = chunks.status
    q = np.asarray(quantiles, dtype=np.float64)
    d = dist.cpu().numpy()
    out = {"distance_smoothed": smoothed.cpu().numpy(), "distance": d, "distance_mean": d.mean(axis=0),
           "distance_std": d.std(axis=0, ddof=1 if nsamples > 1 else 0), "distance_quantiles": np.quantile(d, q, axis=0)}
    if ctime is not None:
        ct = ctime.cpu().numpy()
        out["cross_time"], out["cross_prob"] = ct, (~np.isnan(ct)).mean(axis=0)
        with warnings.catch_warnings():  # a track that no sample takes across the line: all-NaN column, NaN quantiles
            warnings.simplefilter("ignore", RuntimeWarning)
            out["cross_time_quantiles"] = np.nanquantile(ct, q, axis=0)
    out["status"] = status.cpu().numpy()
    return out


KNOT_KMH = 1.852  # km/h to the knot: speeds here are km/h


def speed_statistics(hb_or_db, nsamples: int, seed: int = 0, chunk: int = 16, bands=None, threshold=None, above: bool = False,
                     min_run_h: float = 0.0, limit_kmh=None, quantiles=(0.05, 0.5, 0.95), model: str = "sphere",
                     device="cuda:0", draws=None):
    """How fast the ships went, with the uncertainty of the smoothing posterior, per track: ``nsamples`` posterior tracks are
    drawn (``DeviceBatch.sample_smoothed``), reduced to their speeds (``DeviceBatch.speed_metrics``) and discarded, ``chunk``
    samples at a time, with the generator discipline of ``path_statistics`` (``draws`` as in ``site_statistics``).  What stays
    is (nsamples, B) for the largest speed and the mean speed, and sums per track that take their terms in sample order, so
    for given draws they do not depend on ``chunk``.  Given a ``HostBatch`` it uploads it and runs the forward pass and the
    smoother first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``bands``, ``threshold``,
    ``above``, ``min_run_h`` and ``model`` as in ``speed_metrics``; ``limit_kmh``: None, a scalar or one speed per track, the
    speed the ship cannot make.

    Returns a dict of NumPy arrays in the batch's slot order: every output of ``speed_metrics`` for the smoothed track
    ``sm_mean`` under ``*_smoothed`` names ((B,), ``band_time_smoothed`` (nbands, B)) with ``mean_speed_smoothed`` =
    dist / sound_time (NaN without a sound step); ``mean_speed`` and ``vmax`` (nsamples, B) with ``*_mean``, ``*_std`` (ddof = 1,
    0 for a single sample) and ``*_quantiles`` (len(quantiles), B) over the samples that have a value; with ``limit_kmh``
    ``exceed_prob`` (B,), the fraction of samples with vmax > limit_kmh; with ``threshold`` ``run_prob``, the fraction with a
    run that counts, ``cond_time_mean`` and ``run_time_mean``; with ``bands`` ``band_time_mean`` (nbands, B);
    ``track_status`` (B,) and ``status`` (B,), the sampler's STE_STATUS_* bits."""
    import warnings

    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "speed_statistics")
    torch = db.torch
    B = db.ntracks
    limit = None
    if limit_kmh is not None:
        limit = np.asarray(limit_kmh.cpu().numpy() if isinstance(limit_kmh, torch.Tensor) else limit_kmh, dtype=np.float64)
        if limit.ndim and limit.shape != (B,):
            raise ValueError(f"limit_kmh must be None, a scalar or have shape ({B},), got {limit.shape}")
    kw = dict(bands=bands, threshold=threshold, above=above, min_run_h=min_run_h, model=model)
    smoothed = db.speed_metrics(db.sm_mean, **kw)
    f64 = dict(dtype=torch.float64, device=db.device)
    kept = {k: torch.empty((nsamples, B), **f64) for k in ("mean_speed", "vmax")}
    sums = {k: torch.zeros_like(smoothed[k][0]) for k in ("band_time", "cond_time", "run_time") if k in smoothed}
    with_run = torch.zeros((B,), dtype=torch.int32, device=db.device) if threshold is not None else None
    chunks = _PosteriorChunks(db, nsamples, seed, chunk, draws=draws)
    for i, n, samples in chunks:
        m = db.speed_metrics(samples, **kw)
        kept["mean_speed"][i:i + n] = m["dist"] / m["sound_time"]  # 0 / 0 = NaN: no sound step
        kept["vmax"][i:i + n] = m["vmax"]
        for s in range(n):  # sample by sample: the sums take their terms in sample order whatever the chunk
            for k in sums:
                sums[k] += m[k][s]
            if with_run is not None:
                with_run += m["nruns"][s] > 0
    status = chunks.status
    out = {k + "_smoothed": v[0].cpu().numpy() for k, v in smoothed.items() if k != "track_status"}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["mean_speed_smoothed"] = out["dist_smoothed"] / out["sound_time_smoothed"]
    q = np.asarray(quantiles, dtype=np.float64)
    with warnings.catch_warnings():  # a track no sample gives a sound step: all-NaN column, NaN out
        warnings.simplefilter("ignore", RuntimeWarning)
        for k, ten in kept.items():
            a = ten.cpu().numpy()
            out[k], out[k + "_mean"], out[k + "_quantiles"] = a, np.nanmean(a, axis=0), np.nanquantile(a, q, axis=0)
            out[k + "_std"] = np.nanstd(a, axis=0, ddof=1) if nsamples > 1 else np.where(np.isnan(a[0]), np.nan, 0.0)
    if limit is not None:
        with np.errstate(invalid="ignore"):
            out["exceed_prob"] = (out["vmax"] > limit).mean(axis=0)
    if with_run is not None:
        out["run_prob"] = with_run.cpu().numpy() / float(nsamples)
    for k, ten in sums.items():
        out[k + "_mean"] = ten.cpu().numpy() / float(nsamples)
    out["track_status"] = smoothed["track_status"].cpu().numpy()
    out["status"] = status.cpu().numpy()
    return out


def observation_rows(hb: "HostBatch", upd_idx=None) -> np.ndarray:
    """The truth array (Nmax+1, 2, B) that a batch's own observations define, for ``DeviceBatch.track_errors``: row 0 is
    column 0 of ``hb.z`` (lon, lat) when ``hb.initial_update``; row k + 1 is column ``upd_idx[k]`` of ``z`` where
    0 <= ``upd_idx[k]`` < Tmax (``upd_idx``: (Nmax, B), default ``hb.upd_idx``): the report that step k's update used.
    Everything else is NaN."""
    upd = np.asarray(hb.upd_idx if upd_idx is None else upd_idx)
    if upd.shape != (hb.Nmax, hb.B):
        raise ValueError(f"upd_idx must have shape ({hb.Nmax}, {hb.B}), got {upd.shape}")
    truth = np.full((hb.Nmax + 1, 2, hb.B), np.nan)
    if hb.initial_update:
        truth[0] = hb.z[0, :2]
    k, b = np.nonzero((upd >= 0) & (upd < hb.Tmax))
    truth[k + 1, :, b] = hb.z[upd[k, b], :2, b]
    return truth


def hold_out(hb: "HostBatch", every: int, offset: int = 0):
    """Withhold every ``every``-th report from the filter and keep it as truth: returns ``(hb_thin, truth)``.  In every track
    the updates after the initial one (the steps with 0 <= ``upd_idx`` < Tmax) are counted in step order from 0; those whose
    ordinal is ``offset`` modulo ``every`` get ``upd_idx`` = -1 in a copy of the batch, and ``truth`` (Nmax+1, 2, B, as
    ``observation_rows``) holds the positions of exactly those withheld reports at their rows, NaN everywhere else.  The
    initial update stays; ``every=1`` withholds all the others.

    What this does not withhold: ``sog_rate`` / ``cog_rate`` (and their smoother counterparts) and the SOG / COG columns of
    ``z`` were prepared from ALL reports, the withheld ones included, so the dynamics between two kept reports still carry
    information from the report in between.  A stricter experiment thins the reports first and packs the batch again from
    what is left."""
    every, offset = int(every), int(offset)
    if every < 1 or not 0 <= offset < every:
        raise ValueError(f"every must be >= 1 and 0 <= offset < every, got every = {every} and offset = {offset}")
    fires = (hb.upd_idx >= 0) & (hb.upd_idx < hb.Tmax)
    ordinal = np.cumsum(fires, axis=0) - 1  # of the update of step k among its track's updates
    withheld = fires & (ordinal % every == offset)
    thin = dataclasses.replace(hb, upd_idx=np.ascontiguousarray(np.where(withheld, -1, hb.upd_idx).astype(hb.upd_idx.dtype)))
    truth = observation_rows(hb, np.where(withheld, hb.upd_idx, -1))
    truth[0] = np.nan
    return thin, truth


def truth_course(truth, model: str = "sphere", device="cuda:0") -> np.ndarray:
    """The true course over ground (Nmax+1, B) that a truth array (Nmax+1, 2, B) implies, for ``DeviceBatch.track_errors``:
    at a row with truth, the heading from it to the track's next row with truth; the last such row takes its predecessor's;
    NaN at rows without truth and for a track with fewer than two of them.  It is the COG of ``prepare_observations``
    (``ste_track_prep_f64``) for the rows with truth taken as consecutive reports, so the leg function is the project's."""
    truth = np.asarray(truth, dtype=np.float64)
    if truth.ndim != 3 or truth.shape[1] != 2:
        raise ValueError(f"truth must have shape (Nmax+1, 2, B), got {truth.shape}")
    _metric_model(model)
    have = np.isfinite(truth[:, 0]) & np.isfinite(truth[:, 1])  # (Nmax+1, B)
    course = np.full((truth.shape[0], truth.shape[2]), np.nan)
    tracks = [b for b in range(truth.shape[2]) if have[:, b].sum() >= 2]
    if not tracks:
        return course
    rows = [np.flatnonzero(have[:, b]) for b in tracks]
    res = prepare_observations([truth[r, 0, b] for r, b in zip(rows, tracks)], [truth[r, 1, b] for r, b in zip(rows, tracks)],
                               [np.ones(len(r) - 1) for r in rows], model=model, device=device)
    for r, b, got in zip(rows, tracks, res):
        course[r, b] = got["cog"]
    return course


def error_statistics(hb_or_db, truth, nsamples: int, seed: int = 0, chunk: int = 16, course=None, model: str = "sphere",
                     within_km=None, quantiles=None, rows: bool = False, draws=None, device="cuda:0"):
    """The error against truth positions with the uncertainty of the smoothing posterior, per track: ``nsamples`` posterior
    tracks are drawn (``DeviceBatch.sample_smoothed``), held against ``truth`` (``DeviceBatch.track_errors``) and discarded,
    ``chunk`` samples at a time, with the generator discipline of ``path_statistics`` (``draws`` as in ``site_statistics``), so
    memory does not grow with ``nsamples``: what stays is (nsamples, B) for the rmse and, with ``rows``, one sum per row that
    takes its terms in sample order, so for given draws nothing depends on ``chunk``.  Given a ``HostBatch`` it uploads it and
    runs the forward pass and the smoother first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed
    ``run()``.  ``truth``, ``course`` and ``model`` as in ``track_errors``; ``within_km``: None, a scalar or one distance per
    track.

    Returns a dict of NumPy arrays in the batch's slot order.  Over the samples: ``rmse`` (nsamples, B), ``rmse_mean``,
    ``rmse_std`` (ddof = 1, 0 for a single sample), with ``quantiles`` ``rmse_quantiles`` (len(quantiles), B), with
    ``within_km`` ``within_prob``, the fraction of samples with rmse <= within_km, and with ``rows`` ``err_rows_mean``
    (Nmax+1, B), the mean error of each row over the samples that have one (NaN where none has).  A track without a sound row
    has NaN.  Beside them the smoothed track's own figures, scored against ``sm_cov``: ``n``, ``rmse_smoothed``,
    ``mean_err_smoothed``, ``mean_nees_smoothed``, ``coverage_smoothed`` (at 0.95) and, with ``course``,
    ``mean_along_smoothed`` and ``rms_cross_smoothed``; and ``status`` (B,), the sampler's STE_STATUS_* bits."""
    import warnings

    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "error_statistics")
    torch = db.torch
    B, N = db.ntracks, int(db.struct.Nmax)
    limit = None
    if within_km is not None:
        limit = np.asarray(within_km.cpu().numpy() if isinstance(within_km, torch.Tensor) else within_km, dtype=np.float64)
        if limit.ndim and limit.shape != (B,):
            raise ValueError(f"within_km must be None, a scalar or have shape ({B},), got {limit.shape}")
    up = lambda a: a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a, dtype=np.float64)).to(db.device)
    truth, course = up(truth), up(course)  # uploaded once, not once per chunk
    smoothed = db.track_errors(db.sm_mean, truth, course=course, cov="sm", model=model)
    f64 = dict(dtype=torch.float64, device=db.device)
    rmse = torch.empty((nsamples, B), **f64)
    row_sum = torch.zeros((N + 1, B), **f64) if rows else None
    row_cnt = torch.zeros((N + 1, B), dtype=torch.int32, device=db.device) if rows else None
    chunks = _PosteriorChunks(db, nsamples, seed, chunk, draws=draws)
    for i, n, samples in chunks:
        m = db.track_errors(samples, truth, model=model, rows=rows)
        rmse[i:i + n] = m["rmse"]
        for s in range(n if rows else 0):  # sample by sample: the sums take their terms in sample order whatever the chunk
            has = ~torch.isnan(m["err"][s])
            row_sum += torch.where(has, m["err"][s], torch.zeros_like(row_sum))
            row_cnt += has
    status = chunks.status
    a = rmse.cpu().numpy()
    out = {"rmse": a, "n": smoothed["n"][0].cpu().numpy()}
    with warnings.catch_warnings():  # a track without truth: all-NaN column, NaN out
        warnings.simplefilter("ignore", RuntimeWarning)
        out["rmse_mean"] = np.nanmean(a, axis=0)
        out["rmse_std"] = np.nanstd(a, axis=0, ddof=1) if nsamples > 1 else np.where(np.isnan(a[0]), np.nan, 0.0)
        if quantiles is not None:
            out["rmse_quantiles"] = np.nanquantile(a, np.asarray(quantiles, dtype=np.float64), axis=0)
    if limit is not None:
        with np.errstate(invalid="ignore"):
            out["within_prob"] = np.where(np.isnan(a).all(axis=0), np.nan, (a <= limit).mean(axis=0))
    if rows:
        out["err_rows_mean"] = (row_sum / row_cnt).cpu().numpy()  # 0 / 0 = NaN: no sample has an error in that row
    for k in ("rmse", "mean_err", "mean_along", "rms_cross", "mean_nees", "coverage"):
        if k in smoothed:
            out[k + "_smoothed"] = smoothed[k][0].cpu().numpy()
    out["status"] = status.cpu().numpy()
    return out


@dataclasses.dataclass(frozen=True)
class RegionPolygon:
    """A polygon as ``ste_region_metrics_f64`` wants it (``region_polygon`` makes one): ``vert`` (2, V) float64, px then py,
    counter-clockwise, longitudes unwrapped and within ``lon_ref`` +- 90."""

    vert: np.ndarray
    lon_ref: float


def region_polygon(polygon) -> RegionPolygon:
    """Normalise a (V, 2) array of lon / lat degrees (a GeoJSON ring; planar in lon / lat) for ``region_metrics``.  The
    longitudes are unwrapped about the first vertex (lon_0 + wrap180(lon_i - lon_0)), so a ring may straddle the antimeridian
    stored either way; a repeated closing vertex is dropped; a clockwise ring is reversed; ``lon_ref`` is the midpoint of the
    unwrapped longitude range.  ``ValueError``: not (V, 2); a non-finite coordinate; V outside [3, 1024] after the closing
    vertex is dropped; a longitude extent above 180 degrees; zero area.  That the ring is simple is not checked."""
    p = np.asarray(polygon, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"polygon must be a (V, 2) array of lon / lat degrees, got shape {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("polygon has a non-finite coordinate")
    V = p.shape[0]
    lon, lat = p[:, 0], p[:, 1]
    if V:
        lon = lon[0] + ((lon - lon[0] + 180.0) % 360.0 - 180.0)
    if V > 1 and lon[0] == lon[-1] and lat[0] == lat[-1]:
        lon, lat, V = lon[:-1], lat[:-1], V - 1
    if V < 3 or V > binding.STE_REGION_MAX_VERT:
        raise ValueError(f"polygon must have between 3 and {binding.STE_REGION_MAX_VERT} vertices (a repeated closing vertex "
                         f"not counted), got {V}")
    lo, hi = float(lon.min()), float(lon.max())
    if hi - lo > 180.0:
        raise ValueError(f"polygon spans {hi - lo:.6g} degrees of longitude; at most 180 are supported")
    area2 = float(np.sum(lon * np.roll(lat, -1) - np.roll(lon, -1) * lat))
    if area2 == 0.0:
        raise ValueError("polygon has zero area")
    if area2 < 0.0:
        lon, lat = lon[::-1], lat[::-1]
    return RegionPolygon(vert=np.ascontiguousarray(np.stack([lon, lat])), lon_ref=0.5 * (lo + hi))


def region_statistics(hb_or_db, polygon, nsamples: int, seed: int = 0, chunk: int = 16, model: str = "sphere",
                      distance: bool = False, quantiles=(0.05, 0.5, 0.95), device="cuda:0"):
    """Time in a polygon, entry and occupancy with the uncertainty of the smoothing posterior, per track: ``nsamples`` posterior
    tracks are drawn (``DeviceBatch.sample_smoothed``), reduced (``DeviceBatch.region_metrics``) and discarded, ``chunk``
    samples at a time, with the generator discipline of ``path_statistics``: one draw buffer refilled from one generator, so
    the draws depend on ``(seed, chunk)`` and with ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.
    Given a ``HostBatch`` it uploads it and runs the forward pass and the smoother first; a ``DeviceBatch`` (or a window of one)
    is taken to hold a completed ``run()``.  ``polygon``, ``model`` and ``distance`` as in ``region_metrics``.

    Returns a dict of NumPy arrays in the batch's slot order: ``time_inside_smoothed`` (B,) and ``inside_smoothed``
    (Nmax+1, B) bool, of the smoothed track ``sm_mean``; ``time_inside`` (nsamples, B) with ``time_inside_mean``,
    ``time_inside_std`` (ddof = 1, 0 for a single sample) and ``time_inside_quantiles`` (len(quantiles), B); ``nenter``
    (nsamples, B); ``entry_prob`` (B,), the fraction of samples that are inside at some time; ``first_entry`` (nsamples, B), NaN
    where a sample never is, and ``first_entry_quantiles`` over the samples that enter, NaN where none does; ``occupancy``
    (Nmax+1, B), the fraction of samples inside at each row, summed on the device chunk by chunk from the masks, NaN past
    ``nsteps``; with ``distance`` also ``dist_inside_smoothed`` (B,) and ``dist_inside`` (nsamples, B); and ``status`` (B,),
    the sampler's STE_STATUS_* bits."""
    import warnings

    poly = polygon if isinstance(polygon, RegionPolygon) else region_polygon(polygon)
    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "region_statistics")
    torch = db.torch
    N, B = int(db.struct.Nmax), db.ntracks
    kw = dict(model=model, distance=distance, mask=True)
    smoothed = db.region_metrics(db.sm_mean, poly, **kw)
    f64 = dict(dtype=torch.float64, device=db.device)
    tin, first = torch.empty((nsamples, B), **f64), torch.empty((nsamples, B), **f64)
    nent = torch.empty((nsamples, B), dtype=torch.int32, device=db.device)
    din = torch.empty((nsamples, B), **f64) if distance else None
    count = torch.zeros((N + 1, B), dtype=torch.int32, device=db.device)
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for i, n, samples in chunks:
        m = db.region_metrics(samples, poly, **kw)
        tin[i:i + n], first[i:i + n], nent[i:i + n] = m["time_inside"], m["first_entry"], m["nenter"]
        if din is not None:
            din[i:i + n] = m["dist_inside"]
        count += m["inside"].sum(dim=0, dtype=torch.int32)
    status = chunks.status
    q = np.asarray(quantiles, dtype=np.float64)
    t, fe, ne = tin.cpu().numpy(), first.cpu().numpy(), nent.cpu().numpy()
    nsteps = db.t["nsteps"][db.lo:db.lo + B].cpu().numpy()
    live = np.arange(N + 1)[:, None] <= nsteps[None, :]
    out = {"time_inside_smoothed": smoothed["time_inside"][0].cpu().numpy(),
           "inside_smoothed": smoothed["inside"][0].cpu().numpy().astype(bool),
           "time_inside": t, "time_inside_mean": t.mean(axis=0), "time_inside_std": t.std(axis=0, ddof=1 if nsamples > 1 else 0),
           "time_inside_quantiles": np.quantile(t, q, axis=0), "nenter": ne, "entry_prob": (ne > 0).mean(axis=0),
           "first_entry": fe, "occupancy": np.where(live, count.cpu().numpy() / float(nsamples), np.nan)}
    with warnings.catch_warnings():  # a track that no sample takes into the region: all-NaN column, NaN quantiles
        warnings.simplefilter("ignore", RuntimeWarning)
        out["first_entry_quantiles"] = np.nanquantile(fe, q, axis=0)
    if din is not None:
        out["dist_inside_smoothed"], out["dist_inside"] = smoothed["dist_inside"][0].cpu().numpy(), din.cpu().numpy()
    out["status"] = status.cpu().numpy()
    return out


@dataclasses.dataclass(frozen=True)
class TrackGrid:
    """A regular lon / lat grid as ``ste_grid_metrics_f64`` wants it (``track_grid`` makes one): cell (ix, iy) is
    [lon0 + ix dlon, lon0 + (ix + 1) dlon) x [lat0 + iy dlat, lat0 + (iy + 1) dlat); ``periodic``: the columns wrap (the grid
    is exactly 360 degrees wide); ``lon_ref``: the meridian longitudes are unwrapped about, the grid's mid-longitude."""

    lon0: float
    lat0: float
    dlon: float
    dlat: float
    nx: int
    ny: int
    periodic: bool
    lon_ref: float

    @property
    def lon_edges(self) -> np.ndarray:
        """(nx + 1,) cell edges in longitude, unwrapped (they run on past 180), for plotting."""
        return self.lon0 + self.dlon * np.arange(self.nx + 1)

    @property
    def lat_edges(self) -> np.ndarray:
        """(ny + 1,) cell edges in latitude."""
        return self.lat0 + self.dlat * np.arange(self.ny + 1)


def track_grid(lon0, lat0, dlon, dlat, nx, ny) -> TrackGrid:
    """A regular grid of ``nx`` x ``ny`` cells of ``dlon`` x ``dlat`` degrees whose cell (0, 0) has its west and south edge at
    (``lon0``, ``lat0``), for ``DeviceBatch.grid_metrics``.  It is periodic in longitude when ``nx * dlon == 360.0`` exactly;
    any other grid may be at most 180 degrees wide (one copy of it is then exact for steps of less than 90 degrees).
    ``lon_ref`` is the grid's mid-longitude.  ``ValueError``: nx or ny not an integer >= 1, or nx * ny above 2^26 cells; a
    non-finite lon0 or lat0; dlon or dlat not finite or below 1e-6 degrees; a grid wider than 180 degrees that is not
    periodic."""
    if int(nx) != nx or int(ny) != ny or int(nx) < 1 or int(ny) < 1:
        raise ValueError(f"nx and ny must be integers >= 1, got {nx!r} and {ny!r}")
    nx, ny = int(nx), int(ny)
    if nx * ny > binding.STE_GRID_MAX_CELLS:
        raise ValueError(f"a grid may have at most {binding.STE_GRID_MAX_CELLS} cells (2^26), got {nx} x {ny}")
    lon0, lat0, dlon, dlat = float(lon0), float(lat0), float(dlon), float(dlat)
    if not (np.isfinite(lon0) and np.isfinite(lat0)):
        raise ValueError(f"lon0 and lat0 must be finite, got {lon0!r} and {lat0!r}")
    if not (np.isfinite(dlon) and np.isfinite(dlat) and dlon >= 1e-6 and dlat >= 1e-6):
        raise ValueError(f"dlon and dlat must be finite and >= 1e-6 degrees, got {dlon!r} and {dlat!r}")
    width = float(nx) * dlon
    periodic = width == 360.0
    lon_ref = lon0 + 0.5 * width
    if not periodic and not (lon0 - lon_ref >= -90.0 and (lon0 + width) - lon_ref <= 90.0):
        raise ValueError(f"a grid that is not periodic (nx * dlon == 360) may be at most 180 degrees wide, got {width!r}")
    return TrackGrid(lon0=lon0, lat0=lat0, dlon=dlon, dlat=dlat, nx=nx, ny=ny, periodic=periodic, lon_ref=lon_ref)


def grid_statistics(hb_or_db, grid: TrackGrid, nsamples: int, seed: int = 0, chunk: int = 16, entries: bool = False,
                    device="cuda:0"):
    """Ship-hours per cell of ``grid`` with the uncertainty of the smoothing posterior, summed over the tracks: ``nsamples``
    posterior tracks per ship are drawn (``DeviceBatch.sample_smoothed``), laid on the grid (``DeviceBatch.grid_metrics``) and
    discarded, ``chunk`` samples at a time, every chunk accumulating into one grid, with the generator discipline of
    ``region_statistics``: one draw buffer refilled from one generator, so the draws depend on ``(seed, chunk)`` and with
    ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.  Given a ``HostBatch`` it uploads it and runs
    the forward pass and the smoother first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``; a
    list or tuple of ``DeviceBatch`` windows of a fleet is summed into one grid, every window drawing from a generator seeded
    alike, and the per-track outputs follow the order of the list.

    Returns a dict of NumPy arrays: ``hours_smoothed`` (ny, nx), the map of the smoothed tracks ``sm_mean``; ``hours_mean``
    (ny, nx) = ticks / (2^20 nsamples), the posterior mean of the map; ``ticks`` (ny, nx) int64, the samples' exact sum; with
    ``entries`` also ``entries_mean`` (ny, nx), entries per cell and sample; ``outside_hours`` (nsamples, B), the time of
    each sampled track off the grid; ``total_ticks`` (nsamples, B) int64, the ticks of each sampled track's sound steps;
    ``nbroken`` (nsamples, B) int32; and ``status`` (B,), the sampler's STE_STATUS_* bits."""
    if not isinstance(grid, TrackGrid):
        raise ValueError("grid must be a TrackGrid (track_estimators.batch.track_grid makes one)")
    if isinstance(hb_or_db, (list, tuple)):
        dbs = list(hb_or_db)
        if not dbs or not all(isinstance(d, DeviceBatch) for d in dbs):
            raise ValueError("a list given to grid_statistics() must hold DeviceBatch windows, and at least one")
    else:
        dbs = [hb_or_db]
    smoothed = acc = None
    per_track = []
    for db in dbs:
        db, nsamples, chunk = _posterior_batch(db, nsamples, chunk, device, "grid_statistics")
        torch = db.torch
        B = db.ntracks
        smoothed = db.grid_metrics(db.sm_mean, grid, out=smoothed)
        outside = torch.empty((nsamples, B), dtype=torch.int64, device=db.device)
        total = torch.empty((nsamples, B), dtype=torch.int64, device=db.device)
        nbrk = torch.empty((nsamples, B), dtype=torch.int32, device=db.device)
        chunks = _PosteriorChunks(db, nsamples, seed, chunk)
        for i, n, samples in chunks:
            acc = db.grid_metrics(samples, grid, entries=entries, out=acc)
            outside[i:i + n], total[i:i + n], nbrk[i:i + n] = acc["outside"], acc["total"], acc["nbroken"]
        per_track.append((outside.cpu().numpy(), total.cpu().numpy(), nbrk.cpu().numpy(), chunks.status.cpu().numpy()))
    tph = float(binding.STE_GRID_TICKS_PER_HOUR)
    ticks = acc["ticks"].cpu().numpy()
    out = {"hours_smoothed": smoothed["ticks"].cpu().numpy() / tph, "hours_mean": ticks / (tph * nsamples), "ticks": ticks}
    if entries:
        out["entries_mean"] = acc["entries"].cpu().numpy() / float(nsamples)
    out["outside_hours"] = np.concatenate([p[0] for p in per_track], axis=1) / tph
    out["total_ticks"] = np.concatenate([p[1] for p in per_track], axis=1)
    out["nbroken"] = np.concatenate([p[2] for p in per_track], axis=1)
    out["status"] = np.concatenate([p[3] for p in per_track])
    return out


_RASTER_OUTPUTS = (("total", "int64"), ("outside", "int64"), ("nbroken", "int32"), ("valid", "int64"), ("nodata", "int64"),
                   ("wsum", "float64"), ("vmin", "float64"), ("vmax", "float64"), ("tmin", "int64"), ("tmax", "int64"))
_RASTER_HIT_OUTPUTS = (("hit_ticks", "int64"), ("hit_first", "int64"), ("nhit", "int32"), ("nhit_long", "int32"),
                       ("hit_longest", "int64"))


@dataclasses.dataclass(frozen=True)
class TrackRaster:
    """A gridded field as ``ste_raster_metrics_f64`` wants it (``track_raster`` makes one): ``grid``, a ``TrackGrid``, and
    ``values``, a contiguous float64 device tensor (ny, nx), one value per cell, NaN = no data."""

    grid: TrackGrid
    values: object


def track_raster(grid: TrackGrid, values, device="cuda:0") -> TrackRaster:
    """A field on ``grid`` for ``DeviceBatch.raster_metrics``: ``values`` (ny, nx), an array or a tensor, one value per cell,
    row iy at latitude lat0 + iy dlat upwards, NaN = no data.  A float64 contiguous tensor that already is on a GPU is used
    where it lies -- ``grid_metrics(...)["hours"]`` goes back in without leaving the device --; anything else is converted to
    float64 and copied to ``device``.  ``ValueError``: ``grid`` is no ``TrackGrid``; ``values`` is not (ny, nx); a dtype that
    is neither real nor integer nor bool."""
    import torch

    if not isinstance(grid, TrackGrid):
        raise ValueError("grid must be a TrackGrid (track_estimators.batch.track_grid makes one)")
    if isinstance(values, torch.Tensor):
        ten = values
        if ten.is_complex():
            raise ValueError(f"a raster's values must be real numbers, got a tensor of {ten.dtype}")
    else:
        a = np.asarray(values)
        if a.dtype.kind not in "fiub":
            raise ValueError(f"a raster's values must be real numbers, got an array of dtype {a.dtype}")
        ten = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if tuple(ten.shape) != (grid.ny, grid.nx):
        raise ValueError(f"a raster's values must have shape (ny, nx) = ({grid.ny}, {grid.nx}), got {tuple(ten.shape)}")
    if not (ten.is_cuda and ten.dtype == torch.float64 and ten.is_contiguous()):
        ten = ten.to(device=ten.device if ten.is_cuda else device, dtype=torch.float64).contiguous()
    return TrackRaster(grid=grid, values=ten)


@dataclasses.dataclass(frozen=True)
class TrackField:
    """A space-time gridded field as ``ste_field_values_f64`` wants it (``track_field`` makes one): ``grid``, a ``TrackGrid``
    whose cell centres are the field's nodes; ``values``, a contiguous float64 or float32 device tensor (nt, ny, nx), NaN = no
    data; slab j is valid at ``time0 + j * dtime`` hours on the clock of the queries."""

    grid: TrackGrid
    values: object
    time0: float
    dtime: float

    @property
    def nt(self) -> int:
        return int(self.values.shape[0])


def track_field(grid: TrackGrid, values, time0: float = 0.0, dtime: float = 1.0, device="cuda:0") -> TrackField:
    """A field on ``grid`` for ``DeviceBatch.field_at``: ``values`` (ny, nx), a static field, or (nt, ny, nx), an array or a
    tensor, one value per cell centre, row iy at latitude lat0 + (iy + 0.5) dlat, slab j valid at ``time0 + j * dtime`` hours,
    NaN = no data.  float32 stays float32 (half the bytes of every read); every other real, integer or bool dtype becomes
    float64.  A contiguous tensor of one of the two types that already is on a GPU is used where it lies.  ``ValueError``:
    ``grid`` is no ``TrackGrid``; a shape other than those two; more than 65536 slabs; a dtype that is not real; a non-finite
    ``time0``; ``dtime`` not finite or <= 0 with more than one slab."""
    import torch

    if not isinstance(grid, TrackGrid):
        raise ValueError("grid must be a TrackGrid (track_estimators.batch.track_grid makes one)")
    if isinstance(values, torch.Tensor):
        ten = values
        if ten.is_complex():
            raise ValueError(f"a field's values must be real numbers, got a tensor of {ten.dtype}")
    else:
        a = np.asarray(values)
        if a.dtype.kind not in "fiub":
            raise ValueError(f"a field's values must be real numbers, got an array of dtype {a.dtype}")
        ten = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64))
    if ten.dim() == 2:
        ten = ten.unsqueeze(0)
    if ten.dim() != 3 or tuple(ten.shape[1:]) != (grid.ny, grid.nx) or not 1 <= ten.shape[0] <= binding.STE_FIELD_MAX_SLABS:
        raise ValueError(f"a field's values must have shape (ny, nx) = ({grid.ny}, {grid.nx}) or (nt, ny, nx) with 1 <= nt <= "
                         f"{binding.STE_FIELD_MAX_SLABS}, got {tuple(ten.shape)}")
    time0, dtime = float(time0), float(dtime)
    if not np.isfinite(time0):
        raise ValueError(f"time0 must be finite, got {time0!r}")
    if ten.shape[0] > 1 and not (np.isfinite(dtime) and dtime > 0.0):
        raise ValueError(f"dtime must be finite and > 0 for a field of more than one slab, got {dtime!r}")
    dtype = torch.float32 if ten.dtype == torch.float32 else torch.float64
    if not (ten.is_cuda and ten.dtype == dtype and ten.is_contiguous()):
        ten = ten.to(device=ten.device if ten.is_cuda else device, dtype=dtype).contiguous()
    return TrackField(grid=grid, values=ten, time0=time0, dtime=dtime)


def _raster_threshold(threshold, below, min_hours):
    """(flags, threshold, min_ticks) of ``ste_raster_f64`` for the arguments of ``raster_metrics``."""
    min_hours = float(min_hours)
    if not (min_hours >= 0.0 and np.isfinite(min_hours)):
        raise ValueError(f"min_hours must be finite and >= 0, got {min_hours!r}")
    if threshold is None:
        return binding.STE_RASTER_NO_THRESHOLD, 0.0, 0
    threshold = float(threshold)
    if np.isnan(threshold):
        raise ValueError("threshold must not be NaN (None: no threshold)")
    return (binding.STE_RASTER_BELOW if below else 0, threshold,
            int(np.rint(min_hours * float(binding.STE_GRID_TICKS_PER_HOUR))))


def raster_statistics(hb_or_db, raster: TrackRaster, nsamples: int, seed: int = 0, chunk: int = 16, threshold=None,
                      below: bool = False, min_hours: float = 0.0, quantiles=(0.05, 0.5, 0.95), device="cuda:0"):
    """The values of a gridded field along the ships' tracks with the uncertainty of the smoothing posterior, per track:
    ``nsamples`` posterior tracks are drawn (``DeviceBatch.sample_smoothed``), held against the raster
    (``DeviceBatch.raster_metrics``) and discarded, ``chunk`` samples at a time, with the generator discipline of
    ``grid_statistics``: one draw buffer refilled from one generator, so the draws depend on ``(seed, chunk)`` and with
    ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.  What stays is (nsamples, B) columns: memory
    does not otherwise grow with ``nsamples``.  Given a ``HostBatch`` it uploads it and runs the forward pass and the smoother
    first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``threshold``, ``below`` and
    ``min_hours`` as in ``raster_metrics``.

    Returns a dict of NumPy arrays in the batch's slot order: every output of ``raster_metrics`` for the smoothed track
    ``sm_mean`` under ``*_smoothed`` names, (B,) each; ``mean`` (nsamples, B) and ``mean_quantiles`` (len(quantiles), B) over
    the samples that have a mean, NaN where none has; with ``threshold`` ``hit_hours`` (nsamples, B), ``hit_hours_mean`` (B,),
    ``hit_hours_quantiles``, ``p_hit``, the share of samples with an excursion, and ``p_hit_long``, with one of at least
    ``min_hours``; ``nbroken`` (nsamples, B) int32; and ``status`` (B,), the sampler's STE_STATUS_* bits."""
    import warnings

    if not isinstance(raster, TrackRaster):
        raise ValueError("raster must be a TrackRaster (track_estimators.batch.track_raster makes one)")
    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "raster_statistics")
    torch = db.torch
    B = db.ntracks
    kw = dict(threshold=threshold, below=below, min_hours=min_hours)
    smoothed = db.raster_metrics(db.sm_mean, raster, **kw)
    names = ("mean", "nbroken") + (("hit_hours", "nhit", "nhit_long") if threshold is not None else ())
    kept = {k: torch.empty((nsamples, B), dtype=smoothed[k].dtype, device=db.device) for k in names}
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for i, n, samples in chunks:
        m = db.raster_metrics(samples, raster, **kw)
        for k, ten in kept.items():
            ten[i:i + n] = m[k]
    status = chunks.status
    out = {k + "_smoothed": v[0].cpu().numpy() for k, v in smoothed.items()}
    q = np.asarray(quantiles, dtype=np.float64)
    host = {k: v.cpu().numpy() for k, v in kept.items()}
    out["mean"] = host["mean"]
    with warnings.catch_warnings():  # a track no sample takes onto the data: all-NaN column, NaN quantiles
        warnings.simplefilter("ignore", RuntimeWarning)
        out["mean_quantiles"] = np.nanquantile(host["mean"], q, axis=0)
    if threshold is not None:
        out["hit_hours"] = host["hit_hours"]
        out["hit_hours_mean"] = host["hit_hours"].mean(axis=0)
        out["hit_hours_quantiles"] = np.quantile(host["hit_hours"], q, axis=0)
        out["p_hit"] = (host["nhit"] > 0).mean(axis=0)
        out["p_hit_long"] = (host["nhit_long"] > 0).mean(axis=0)
    out["nbroken"] = host["nbroken"]
    out["status"] = status.cpu().numpy()
    return out


EARTH_RADIUS_KM = 6378.137  # the sphere of the haversine leg and of the encounter kernel's planar metric


def candidate_pairs(mean, nsteps, dt, radius_km, margin_km: float = 0.0, t0=None, chunk: int = 2048):
    """The pair test of ``encounter_candidates`` on plain tensors of any one device: ``mean`` (Nmax+1, 4, B) float64,
    ``nsteps`` (B,) integer, ``dt`` (Nmax, B) float64, ``t0`` None, a scalar or (B,).  Returns an int32 (P, 2) tensor of
    (i, j), i < j, sorted by (i, j)."""
    import torch

    rows, _, B = mean.shape
    dev = mean.device
    ns = nsteps.to(dev).to(torch.int64).clamp(0, rows - 1)
    live = torch.arange(rows, device=dev)[:, None] <= ns[None, :]                     # (rows, B)
    lon, lat = torch.deg2rad(mean[:, 0]), torch.deg2rad(mean[:, 1])
    unit = torch.stack([torch.cos(lat) * torch.cos(lon), torch.cos(lat) * torch.sin(lon), torch.sin(lat)])  # (3, rows, B)
    finite = torch.isfinite(unit).all(dim=0)
    ok = (ns > 0) & (finite | ~live).all(dim=0)
    unit = torch.where(live[None], unit, torch.zeros_like(unit))
    centre = unit.sum(dim=1)
    norm = centre.norm(dim=0)
    ok = ok & (norm > 0.0)
    centre = centre / torch.where(norm > 0.0, norm, torch.ones_like(norm))           # (3, B)
    # angles from chords: 2 asin(|u - v| / 2), which keeps its precision for small angles
    chord = (unit - centre[:, None, :]).norm(dim=0)
    chord = torch.where(live, chord, torch.zeros_like(chord))
    cap = 2.0 * torch.asin((0.5 * chord).clamp(max=1.0)).max(dim=0).values            # (B,)
    if t0 is None:
        start = torch.zeros((B,), dtype=torch.float64, device=dev)
    else:
        start = torch.as_tensor(t0, dtype=torch.float64).to(dev).expand(B)
    steps_live = torch.arange(rows - 1, device=dev)[:, None] < ns[None, :]
    end = start + torch.where(steps_live, dt.to(dev), torch.zeros_like(dt)).sum(dim=0)
    ok = ok & torch.isfinite(start) & torch.isfinite(end)
    # 1e-7 rad (0.6 m): the rounding of an angle taken from a dot product of unit vectors is below sqrt(2^-52) = 1.5e-8
    reach = (float(radius_km) + float(margin_km)) / EARTH_RADIUS_KM + 1e-7
    idx = torch.arange(B, device=dev)
    found = []
    for lo in range(0, B, int(chunk)):
        hi = min(lo + int(chunk), B)
        dot = centre[:, lo:hi].T @ centre                                             # (hi - lo, B)
        angle = 2.0 * torch.asin(torch.sqrt((0.5 * (1.0 - dot)).clamp(0.0, 1.0)))
        near = angle <= cap[lo:hi, None] + cap[None, :] + reach
        clocks = torch.maximum(start[lo:hi, None], start[None, :]) <= torch.minimum(end[lo:hi, None], end[None, :])
        keep = near & clocks & ok[lo:hi, None] & ok[None, :] & (idx[None, :] > idx[lo:hi, None])
        ij = keep.nonzero()                                                           # row-major: sorted by (i, j)
        ij[:, 0] += lo
        found.append(ij)
    return torch.cat(found).to(torch.int32)


def encounter_candidates(db: "DeviceBatch", radius_km, margin_km: float = 0.0, t0=None, chunk: int = 2048, window_h=None,
                         track_margin_km=None):
    """The pairs of a resident batch worth giving to ``DeviceBatch.encounter_metrics``: an int32 (P, 2) device tensor of
    (i, j), i < j, sorted by (i, j), on the batch's device.  Torch plumbing without a kernel, on ``sm_mean`` (``fwd_mean`` when
    the batch has no smoother).  Every track gets a bounding cap on the unit sphere (centre: the normalised sum of its rows'
    unit vectors; angular radius: the largest angle to one of its rows 0 .. nsteps) and a clock span [t0, t0 + sum of its dt];
    a pair is kept when the clock spans overlap and the angle between the centres is at most the sum of the two radii plus
    (``radius_km`` + ``margin_km``) / 6378.137.  The B x B test runs in blocks of ``chunk`` rows, so memory stays at a few
    times chunk x B doubles.  Tracks with ``nsteps == 0`` or a non-finite row pair with nothing; the test is on unit vectors,
    so the antimeridian is no special case.  ``margin_km`` must cover what the tested track does not show: the posterior spread
    when the pairs are then used on samples of the posterior (a few standard deviations of position), and the 0.2 % by which
    the kernel's planar distance may differ from the true one.

    ``window_h`` (hours): the pairs come from ``DeviceBatch.encounter_candidates`` instead, the kernels of include/ste.h
    CANDIDATES, with reach = ``radius_km`` + ``margin_km``, windows of ``window_h`` over the fleet's clock, and
    ``track_margin_km`` (``position_spread_km``) as a margin per track; ``chunk`` is not used.  Which one: the caps above
    prune only ships that stay in one place for their whole life (a fleet in separate basins, short tracks); voyages that
    cross an ocean have caps thousands of kilometres wide and clocks that all overlap, and there the windowed list, which
    asks where the two ships were in the same few hours, is a small fraction of this one ("Candidates").  Both
    hold every pair that comes within ``radius_km``; a day is a reasonable ``window_h`` for ships."""
    if window_h is not None:
        return db.encounter_candidates(float(radius_km) + float(margin_km), window_h, t0=t0, track_margin_km=track_margin_km)
    if track_margin_km is not None:
        raise ValueError("track_margin_km belongs to the windowed list: give window_h as well")
    mean = db.sm_mean if db.sm_mean is not None else db.fwd_mean
    if mean is None:
        raise ValueError("encounter_candidates() needs sm_mean or fwd_mean, and this batch was built without histories")
    B = db.ntracks
    nsteps = db.t["nsteps"][db.lo:db.lo + B]
    dt = db.t["dt"][:, db.lo:db.lo + B]
    with db.torch.cuda.device(db.device):
        return candidate_pairs(mean, nsteps, dt, radius_km, margin_km, t0, chunk)


def position_spread_km(db: "DeviceBatch", nsigma: float = 3.0):
    """How far a posterior sample of each track may lie from its smoothed position, in km: per track, ``nsigma`` times the
    square root of the largest eigenvalue of the (lon, lat) block of ``sm_cov`` over its rows 0 .. nsteps, longitude scaled
    by cos(lat) and both by 6378.137 pi / 180 km per degree.  A (B,) float64 device tensor; torch on the device, no kernel.
    It is the ``track_margin_km`` of ``encounter_candidates`` for a list that is to be used on posterior samples
    (``encounter_statistics``).  NaN where a covariance of the track is not finite (such a track then pairs with nothing)."""
    if db.sm_cov is None or db.sm_mean is None:
        raise ValueError("position_spread_km() needs sm_mean and sm_cov: a batch with histories and a smoother")
    torch = db.torch
    with torch.cuda.device(db.device):
        cov, B = db.sm_cov, db.ntracks
        c00, c01, c11 = cov[:, 0], cov[:, 1], cov[:, 4 if db.packed_cov else 5]
        kd = EARTH_RADIUS_KM * np.pi / 180.0
        kx = kd * torch.cos(torch.deg2rad(db.sm_mean[:, 1]))
        a, b, d = c00 * kx * kx, c01 * kx * kd, c11 * kd * kd
        lam = 0.5 * ((a + d) + torch.sqrt((a - d) * (a - d) + 4.0 * b * b))        # (Nmax+1, B)
        ns = db.t["nsteps"][db.lo:db.lo + B].to(torch.int64).clamp(0, cov.shape[0] - 1)
        live = torch.arange(cov.shape[0], device=db.device)[:, None] <= ns[None, :]
        worst = torch.where(live, lam, torch.zeros_like(lam)).max(dim=0).values
        return float(nsigma) * torch.sqrt(worst.clamp(min=0.0))


def encounter_statistics(hb_or_db, pairs, radius_km, nsamples: int, seed: int = 0, chunk: int = 16, t0=None,
                         model: str = "sphere", quantiles=(0.05, 0.5, 0.95), device="cuda:0"):
    """Closest approach and time within ``radius_km`` of pairs of ships with the uncertainty of the smoothing posterior:
    ``nsamples`` posterior tracks per ship are drawn (``DeviceBatch.sample_smoothed``), sample s of one ship held against
    sample s of the other (``DeviceBatch.encounter_metrics``) and discarded, ``chunk`` samples at a time, with the generator
    discipline of ``region_statistics``: one draw buffer refilled from one generator, so the draws depend on ``(seed, chunk)``
    and with ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.  The ships' posteriors are taken as
    independent (each is smoothed on its own).  Given a ``HostBatch`` it uploads it and runs the forward pass and the smoother
    first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``pairs``, ``radius_km``, ``t0``
    and ``model`` as in ``encounter_metrics``.  A pair list that holds every pair a sample can bring within ``radius_km``
    comes from ``encounter_candidates`` with ``track_margin_km=position_spread_km(db)``.

    Returns a dict of NumPy arrays per pair: ``min_dist_smoothed``, ``min_time_smoothed``, ``time_within_smoothed``,
    ``overlap_smoothed`` (P,) and ``status`` (P,; STE_ENC_* bits), of the smoothed tracks ``sm_mean``; ``min_dist``
    (nsamples, P) with ``min_dist_mean``, ``min_dist_std`` (ddof = 1, 0 for a single sample) and ``min_dist_quantiles``
    (len(quantiles), P), over the samples that have a distance; ``min_time`` and ``min_time_quantiles``; ``time_within``
    with ``time_within_mean`` and ``time_within_quantiles``; ``nwithin`` (nsamples, P); ``encounter_prob`` (P,), the fraction
    of samples that come within ``radius_km``; ``first_within``, NaN where a sample never does, and
    ``first_within_quantiles`` over the samples that do, NaN where none does; and ``sample_status`` (B,), the sampler's
    STE_STATUS_* bits per track."""
    import warnings

    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "encounter_statistics")
    torch = db.torch
    kw = dict(t0=t0, model=model)
    smoothed = db.encounter_metrics(db.sm_mean, pairs, radius_km, **kw)
    P = int(smoothed["status"].shape[0])
    f64 = dict(dtype=torch.float64, device=db.device)
    names = ("min_dist", "min_time", "time_within", "first_within")
    acc = {k: torch.empty((nsamples, P), **f64) for k in names}
    nwit = torch.empty((nsamples, P), dtype=torch.int32, device=db.device)
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for i, n, samples in chunks:
        m = db.encounter_metrics(samples, pairs, radius_km, **kw)
        for k in names:
            acc[k][i:i + n] = m[k]
        nwit[i:i + n] = m["nwithin"]
    status = chunks.status
    q = np.asarray(quantiles, dtype=np.float64)
    host = {k: v.cpu().numpy() for k, v in acc.items()}
    nw = nwit.cpu().numpy()
    out = {k + "_smoothed": smoothed[k][0].cpu().numpy() for k in ("min_dist", "min_time", "time_within", "overlap")}
    out["status"] = smoothed["status"].cpu().numpy()
    with warnings.catch_warnings():  # a pair no sample gives a distance (or brings within the radius): all-NaN column, NaN out
        warnings.simplefilter("ignore", RuntimeWarning)
        d = host["min_dist"]
        out.update({"min_dist": d, "min_dist_mean": np.nanmean(d, axis=0),
                    "min_dist_std": np.nanstd(d, axis=0, ddof=1) if nsamples > 1 else np.where(np.isnan(d[0]), np.nan, 0.0),
                    "min_dist_quantiles": np.nanquantile(d, q, axis=0),
                    "min_time": host["min_time"], "min_time_quantiles": np.nanquantile(host["min_time"], q, axis=0),
                    "time_within": host["time_within"], "time_within_mean": host["time_within"].mean(axis=0),
                    "time_within_quantiles": np.quantile(host["time_within"], q, axis=0),
                    "nwithin": nw, "encounter_prob": (nw > 0).mean(axis=0),
                    "first_within": host["first_within"],
                    "first_within_quantiles": np.nanquantile(host["first_within"], q, axis=0)})
    out["sample_status"] = status.cpu().numpy()
    return out


def nearest_site(min_dist):
    """The closest site per (sample, track) from the ``min_dist`` (S, M, B) of ``DeviceBatch.site_metrics``: torch on the
    tensor's own device, no kernel of this library.  Returns ``(index, distance)``, (S, B) each: the index of the smallest
    distance that is not NaN (the first of equal ones) as int64 and that distance in km; -1 and NaN where every site's is NaN
    (a track without a sound step, a bad clock, bad sites only)."""
    import torch

    if min_dist.dim() != 3:
        raise ValueError(f"min_dist must have shape (S, M, B), got {tuple(min_dist.shape)}")
    nan = torch.isnan(min_dist)
    dist, index = torch.where(nan, torch.full_like(min_dist, float("inf")), min_dist).min(dim=1)
    none = nan.all(dim=1)
    return torch.where(none, torch.full_like(index, -1), index), torch.where(none, torch.full_like(dist, float("nan")), dist)


def site_statistics(hb_or_db, sites, radius_km, nsamples: int, seed: int = 0, chunk: int = 16, min_stay_h: float = 0.0,
                    quantiles=None, max_bytes: int = 2 ** 31, t0=None, model: str = "sphere", draws=None, device="cuda:0"):
    """Which ships called at which sites, with the uncertainty of the smoothing posterior: ``nsamples`` posterior tracks per
    ship are drawn (``DeviceBatch.sample_smoothed``), held against every site (``DeviceBatch.site_metrics``) and discarded,
    ``chunk`` samples at a time, with the generator discipline of ``region_statistics``: one draw buffer refilled from one
    generator, so the draws depend on ``(seed, chunk)`` and with ``chunk >= nsamples`` they are those of
    ``sample_smoothed(nsamples, seed)``.  What is kept between chunks are counts and sums per (site, track) on the device,
    added to sample by sample in sample order: memory does not grow with ``nsamples``, and for given draws the result does not
    depend on ``chunk``, bit for bit.  ``draws``: None, or a callable ``draws(buf, first)`` that fills the (n, Nmax+1, 4, B)
    float64 device tensor ``buf`` with the standard normal draws of samples ``first .. first + n`` in place of the generator
    (zeros give the smoothed track n times over).  Given a ``HostBatch`` it uploads it and runs the forward pass and the
    smoother first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``sites``, ``radius_km``,
    ``t0`` and ``model`` as in ``site_metrics``.

    Returns a dict of NumPy arrays per (site, track), (M, B): ``min_dist_smoothed``, ``min_time_smoothed``,
    ``time_within_smoothed``, ``first_within_smoothed``, ``longest_smoothed``, ``nwithin_smoothed``, of the smoothed tracks
    ``sm_mean``; ``visit_prob``, the fraction of samples that come within the site's radius (``nwithin`` > 0); ``call_prob``,
    the fraction whose longest stay is at least ``min_stay_h`` hours and that come within at all; ``min_dist_mean`` over the
    samples that have a distance (NaN where none has) with their number ``min_dist_count``; ``time_within_mean`` and
    ``longest_mean`` over all samples; ``track_status`` (B,), ``site_status`` (M,) and ``sample_status`` (B,), the
    sampler's STE_STATUS_* bits.  With ``quantiles`` (a sequence of probabilities) also ``min_dist_quantiles``,
    ``time_within_quantiles`` and ``longest_quantiles`` (len(quantiles), M, B): these keep every sample's value, nsamples x M x
    B doubles per quantity, and are refused when that exceeds ``max_bytes``."""
    import warnings

    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "site_statistics")
    torch = db.torch
    B = db.ntracks
    M = int(np.shape(sites)[0]) if not isinstance(sites, torch.Tensor) else int(sites.shape[0])
    qnames = ("min_dist", "time_within", "longest")
    if quantiles is not None:
        need = 8 * nsamples * M * B
        if need > int(max_bytes):
            raise ValueError(f"quantiles keep nsamples x M x B = {nsamples} x {M} x {B} doubles per quantity, {need} bytes, above "
                             f"max_bytes = {int(max_bytes)}: lower nsamples, split the sites, raise max_bytes or pass quantiles=None")
    kw = dict(t0=t0, model=model)
    smoothed = db.site_metrics(db.sm_mean, sites, radius_km, **kw)
    f64 = dict(dtype=torch.float64, device=db.device)
    visits, calls, have = (torch.zeros((M, B), dtype=torch.int32, device=db.device) for _ in range(3))
    sums = {k: torch.zeros((M, B), **f64) for k in qnames}
    kept = {k: torch.empty((nsamples, M, B), **f64) for k in qnames} if quantiles is not None else None
    stay = float(min_stay_h)
    chunks = _PosteriorChunks(db, nsamples, seed, chunk, draws=draws)
    for i, n, samples in chunks:
        m = db.site_metrics(samples, sites, radius_km, **kw)
        came = m["nwithin"] > 0
        found = ~torch.isnan(m["min_dist"])
        dist = torch.where(found, m["min_dist"], torch.zeros_like(m["min_dist"]))
        for s in range(n):  # sample by sample: the sums take their terms in sample order whatever the chunk
            visits += came[s]
            calls += came[s] & (m["longest"][s] >= stay)
            have += found[s]
            sums["min_dist"] += dist[s]
            sums["time_within"] += m["time_within"][s]
            sums["longest"] += m["longest"][s]
        if kept is not None:
            for k in qnames:
                kept[k][i:i + n] = m[k]
    status = chunks.status
    out = {k + "_smoothed": smoothed[k][0].cpu().numpy() for k in DeviceBatch._SITE_OUT3 + ("nwithin",)}
    count = have.cpu().numpy()
    out["visit_prob"] = visits.cpu().numpy() / float(nsamples)
    out["call_prob"] = calls.cpu().numpy() / float(nsamples)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["min_dist_mean"] = np.where(count > 0, sums["min_dist"].cpu().numpy() / count, np.nan)
    out["min_dist_count"] = count
    out["time_within_mean"] = sums["time_within"].cpu().numpy() / float(nsamples)
    out["longest_mean"] = sums["longest"].cpu().numpy() / float(nsamples)
    if kept is not None:
        q = np.asarray(quantiles, dtype=np.float64)
        with warnings.catch_warnings():  # a (site, track) no sample gives a distance: all-NaN column, NaN out
            warnings.simplefilter("ignore", RuntimeWarning)
            for k in qnames:
                out[k + "_quantiles"] = np.nanquantile(kept[k].cpu().numpy(), q, axis=0)
    out["track_status"], out["site_status"] = smoothed["track_status"].cpu().numpy(), smoothed["site_status"].cpu().numpy()
    out["sample_status"] = status.cpu().numpy()
    return out


@dataclasses.dataclass(frozen=True)
class TrackLines:
    """Polylines as ``ste_line_metrics_f64`` wants them (``track_lines`` makes one): ``vert`` (2, V) float64, lon then lat,
    the longitudes of each line unwrapped from its first vertex; ``first`` (M + 1,) int32, line m owns vertices first[m] ..
    first[m+1] - 1; ``lon_ref`` (M,), the middle of each line's unwrapped extent.  ``on(device)`` gives the three as device
    tensors, uploaded once per device."""

    vert: np.ndarray
    first: np.ndarray
    lon_ref: np.ndarray
    _dev: dict = dataclasses.field(default_factory=dict, repr=False, compare=False)

    @property
    def nlines(self) -> int:
        return int(self.lon_ref.shape[0])

    def line(self, m: int) -> np.ndarray:
        """(n_m, 2) lon / lat of line m as stored."""
        return self.vert[:, self.first[m]:self.first[m + 1]].T

    def on(self, device):
        import torch

        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.vert, self.first, self.lon_ref))
        return self._dev[key]


def track_lines(lines) -> TrackLines:
    """Normalise a list of (n_i, 2) arrays of lon / lat degrees (planar in lon / lat, as a GeoJSON LineString) for
    ``DeviceBatch.line_metrics``.  The longitudes of each line are unwrapped from its first vertex by wrap180 differences
    (lon_{i+1} = lon_i + wrap180(lon_{i+1} - lon_i)), so a line may straddle the antimeridian stored either way; ``lon_ref`` is
    the middle of the unwrapped extent.  ``ValueError``: no line or more than 4096; a line that is not (n, 2) or has fewer than
    2 vertices; a non-finite coordinate; a segment with |delta lon| >= 90 degrees; a line wider than 180 degrees; more than
    2^20 vertices in all.  A closed ring is a line whose last vertex repeats its first."""
    if isinstance(lines, TrackLines):
        return lines
    lines = list(lines)
    if not 1 <= len(lines) <= binding.STE_LINES_MAX:
        raise ValueError(f"lines must be a list of 1 to {binding.STE_LINES_MAX} (n, 2) arrays, got {len(lines)}")
    xs, ys, refs, first = [], [], [], [0]
    for m, ln in enumerate(lines):
        p = np.asarray(ln.detach().cpu().numpy() if hasattr(ln, "detach") else ln, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"line {m} must be an (n, 2) array of lon / lat degrees, got shape {p.shape}")
        if p.shape[0] < 2:
            raise ValueError(f"line {m} has fewer than 2 vertices ({p.shape[0]})")
        if not np.isfinite(p).all():
            raise ValueError(f"line {m} has a non-finite coordinate")
        step = (np.diff(p[:, 0]) + 180.0) % 360.0 - 180.0
        if (np.abs(step) >= 90.0).any():
            raise ValueError(f"line {m} has a segment of {float(np.abs(step).max()):.6g} degrees of longitude; a segment must span "
                             "less than 90")
        lon = p[0, 0] + np.concatenate([[0.0], np.cumsum(step)])
        lo, hi = float(lon.min()), float(lon.max())
        if hi - lo > 180.0:
            raise ValueError(f"line {m} spans {hi - lo:.6g} degrees of longitude; at most 180 are supported")
        xs.append(lon)
        ys.append(p[:, 1])
        refs.append(0.5 * (lo + hi))
        first.append(first[-1] + p.shape[0])
    if first[-1] > binding.STE_LINE_MAX_VERT_TOTAL:
        raise ValueError(f"the lines have {first[-1]} vertices in all; at most {binding.STE_LINE_MAX_VERT_TOTAL} are supported")
    vert = np.ascontiguousarray(np.stack([np.concatenate(xs), np.concatenate(ys)]))
    return TrackLines(vert=vert, first=np.asarray(first, dtype=np.int32), lon_ref=np.asarray(refs, dtype=np.float64))


def line_chainage(lines, min_seg, min_frac, model: str = "sphere"):
    """Where along each line the closest point lies, in km from the line's first vertex: the lengths of the segments before
    ``min_seg`` plus ``min_frac`` times the length of that segment, NaN where ``min_seg`` < 0.  ``lines`` as in
    ``DeviceBatch.line_metrics``; ``min_seg`` and ``min_frac`` its (S, M, B) outputs (or any (..., M, B) tensors).  The segment
    lengths are the legs of ``model`` ("sphere" or "wgs84"), computed once on the host; the rest is torch on the tensors' own
    device, no kernel of this library."""
    import torch

    from . import utils

    _metric_model(model)
    tl = track_lines(lines)
    M = tl.nlines
    if min_seg.dim() < 2 or min_seg.shape[-2] != M or min_seg.shape != min_frac.shape:
        raise ValueError(f"min_seg and min_frac must have one shape (..., {M}, B), got {tuple(min_seg.shape)} and {tuple(min_frac.shape)}")
    x, y = tl.vert
    V = x.shape[0]
    seglen, before = np.zeros(V), np.zeros(V)  # per vertex: the segment that starts there, and the km before it on its line
    for m in range(M):
        a, b = int(tl.first[m]), int(tl.first[m + 1])
        if model == "sphere":
            leg = np.asarray(utils.haversine_formula(x[a:b - 1], y[a:b - 1], x[a + 1:b], y[a + 1:b]), dtype=np.float64)
        else:
            leg = np.array([utils.geographiclib_distance(x[i], y[i], x[i + 1], y[i + 1]) for i in range(a, b - 1)])
        seglen[a:b - 1] = leg
        before[a:b] = np.concatenate([[0.0], np.cumsum(leg)])
    dev = min_seg.device
    seglen_d, before_d = torch.from_numpy(seglen).to(dev), torch.from_numpy(before).to(dev)
    start = torch.from_numpy(tl.first[:-1].astype(np.int64)).to(dev).reshape((M, 1))
    none = min_seg < 0
    idx = start + torch.where(none, torch.zeros_like(min_seg), min_seg).to(torch.int64)
    km = before_d[idx] + min_frac * seglen_d[idx]
    return torch.where(none, torch.full_like(km, float("nan")), km)


def line_statistics(hb_or_db, lines, nsamples: int, seed: int = 0, chunk: int = 16, within_km=None, quantiles=None,
                    max_bytes: int = 2 ** 31, t0=None, model: str = "sphere", draws=None, device="cuda:0"):
    """Which ships crossed which lines and how close they came, with the uncertainty of the smoothing posterior: ``nsamples``
    posterior tracks per ship are drawn (``DeviceBatch.sample_smoothed``), held against every line
    (``DeviceBatch.line_metrics``) and discarded, ``chunk`` samples at a time, with the generator discipline of
    ``site_statistics``: one draw buffer refilled from one generator, so the draws depend on ``(seed, chunk)`` and with
    ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.  What is kept between chunks are counts and sums
    per (line, track) on the device, added to sample by sample in sample order: memory does not grow with ``nsamples``, and for
    given draws the result does not depend on ``chunk``, bit for bit.  ``draws`` as in ``site_statistics``.  Given a
    ``HostBatch`` it uploads it and runs the forward pass and the smoother first; a ``DeviceBatch`` (or a window of one) is
    taken to hold a completed ``run()``.  ``lines``, ``t0`` and ``model`` as in ``line_metrics``.

    Returns a dict of NumPy arrays per (line, track), (M, B): ``min_dist_smoothed``, ``min_time_smoothed``,
    ``min_seg_smoothed``, ``min_frac_smoothed``, ``ncross_smoothed``, ``net_cross_smoothed``, ``first_cross_smoothed`` and
    ``last_cross_smoothed`` of the smoothed tracks ``sm_mean``; ``cross_prob``, the fraction of samples that cross the line
    (``ncross`` > 0); ``net_prob``, the fraction that end on its other side (``net_cross`` != 0); ``first_cross_mean`` over the
    samples that cross (NaN where none does) with their number ``first_cross_count``; ``min_dist_mean`` over the samples that
    have a distance (NaN where none has) with their number ``min_dist_count``; with ``within_km`` (a scalar or one per line)
    ``approach_prob``, the fraction of samples with ``min_dist`` <= ``within_km``; ``track_status`` (B,), ``line_status`` (M,)
    and ``sample_status`` (B,), the sampler's STE_STATUS_* bits.  With ``quantiles`` (a sequence of probabilities) also
    ``min_dist_quantiles`` and ``first_cross_quantiles`` (len(quantiles), M, B), over the samples that have a value: these keep
    every sample's value, nsamples x M x B doubles per quantity, and are refused when that exceeds ``max_bytes``."""
    import warnings

    tl = track_lines(lines)
    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "line_statistics")
    torch = db.torch
    B, M = db.ntracks, tl.nlines
    qnames = ("min_dist", "first_cross")
    if quantiles is not None:
        need = 8 * nsamples * M * B
        if need > int(max_bytes):
            raise ValueError(f"quantiles keep nsamples x M x B = {nsamples} x {M} x {B} doubles per quantity, {need} bytes, above "
                             f"max_bytes = {int(max_bytes)}: lower nsamples, split the lines, raise max_bytes or pass quantiles=None")
    f64 = dict(dtype=torch.float64, device=db.device)
    near = None
    if within_km is not None:
        near = torch.as_tensor(within_km, dtype=torch.float64).to(db.device)
        if near.dim() == 0:
            near = near.expand(M)
        if tuple(near.shape) != (M,):
            raise ValueError(f"within_km must be None, a scalar or have shape ({M},), got {tuple(near.shape)}")
        near = near.reshape((M, 1))
    kw = dict(t0=t0, model=model)
    smoothed = db.line_metrics(db.sm_mean, tl, **kw)
    crossed, net, have, close = (torch.zeros((M, B), dtype=torch.int32, device=db.device) for _ in range(4))
    sums = {k: torch.zeros((M, B), **f64) for k in qnames}
    kept = {k: torch.empty((nsamples, M, B), **f64) for k in qnames} if quantiles is not None else None
    chunks = _PosteriorChunks(db, nsamples, seed, chunk, draws=draws)
    for i, n, samples in chunks:
        m = db.line_metrics(samples, tl, **kw)
        found = ~torch.isnan(m["min_dist"])
        dist = torch.where(found, m["min_dist"], torch.zeros_like(m["min_dist"]))
        came = m["ncross"] > 0
        when = torch.where(came, m["first_cross"], torch.zeros_like(m["first_cross"]))
        for s in range(n):  # sample by sample: the sums take their terms in sample order whatever the chunk
            crossed += came[s]
            net += m["net_cross"][s] != 0
            have += found[s]
            sums["min_dist"] += dist[s]
            sums["first_cross"] += when[s]
            if near is not None:
                close += m["min_dist"][s] <= near
        if kept is not None:
            for k in qnames:
                kept[k][i:i + n] = m[k]
    status = chunks.status
    names = tuple(DeviceBatch._LINE_OUT3) + tuple(DeviceBatch._LINE_CROSS)
    out = {k + "_smoothed": smoothed[k][0].cpu().numpy() for k in names}
    count, ncount = have.cpu().numpy(), crossed.cpu().numpy()
    out["cross_prob"] = ncount / float(nsamples)
    out["net_prob"] = net.cpu().numpy() / float(nsamples)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["first_cross_mean"] = np.where(ncount > 0, sums["first_cross"].cpu().numpy() / ncount, np.nan)
        out["min_dist_mean"] = np.where(count > 0, sums["min_dist"].cpu().numpy() / count, np.nan)
    out["first_cross_count"], out["min_dist_count"] = ncount, count
    if near is not None:
        out["approach_prob"] = close.cpu().numpy() / float(nsamples)
    if kept is not None:
        q = np.asarray(quantiles, dtype=np.float64)
        with warnings.catch_warnings():  # a (line, track) no sample gives a value: all-NaN column, NaN out
            warnings.simplefilter("ignore", RuntimeWarning)
            for k in qnames:
                out[k + "_quantiles"] = np.nanquantile(kept[k].cpu().numpy(), q, axis=0)
    out["track_status"], out["line_status"] = smoothed["track_status"].cpu().numpy(), smoothed["line_status"].cpu().numpy()
    out["sample_status"] = status.cpu().numpy()
    return out


def _route_call(lib, torch, s, states, S, pr, dtw, band, reverse, model_id, device, stream_ptr, keep):
    """One ste_route_metrics_f64 launch on the current stream: ``s`` the batch struct (B, Nmax, track_stride and nsteps are all
    it needs), ``states`` (S, Nmax+1, 4, ld) and ``pr`` (P, 2) int32 on ``device``.  Allocates the outputs and the scratch;
    tensors the launch reads are appended to ``keep``."""
    P = int(pr.shape[0])
    f64 = dict(dtype=torch.float64, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    ro = binding.SteRouteF64()
    ro.nstates, ro.model, ro.states = S, model_id, states.data_ptr()
    ro.npairs, ro.pairs = P, pr.data_ptr()
    ro.band, ro.flags = int(band), binding.STE_ROUTE_REVERSE_J if reverse else 0
    need = int(lib.ste_route_workspace(int(s.Nmax), S, P))
    if need:
        work = torch.empty(((need + 7) // 8,), **f64)
        ro.work, ro.work_bytes = work.data_ptr(), need
        keep.append(work)
    out = {"frechet": torch.empty((S, P), **f64), "frechet_at": torch.empty((S, P, 2), **i32),
           "status": torch.empty((S, P), **i32)}
    if dtw:
        out["dtw"] = torch.empty((S, P), **f64)
        out["dtw_len"] = torch.empty((S, P), **i32)
    for k, ten in out.items():
        setattr(ro, k, ten.data_ptr())
    binding.check(lib.ste_route_metrics_f64(C.byref(s), C.byref(ro), stream_ptr), "ste_route_metrics_f64")
    return out


def route_endpoint_pairs(mean, nsteps, within_km, margin_km: float = 0.0, reverse: bool = False, chunk: int = 2048):
    """The pair test of ``route_candidates`` on plain tensors of any one device: ``mean`` (Nmax+1, 4, B) float64 and
    ``nsteps`` (B,) integer.  Returns an int32 (P, 2) tensor of (i, j), i < j, sorted by (i, j)."""
    import torch

    rows, _, B = mean.shape
    dev = mean.device
    ns = nsteps.to(dev).to(torch.int64).clamp(0, rows - 1)
    col = torch.arange(B, device=dev)

    def unit(row):  # (3, B): the unit vectors of one row per track
        lon, lat = torch.deg2rad(mean[row, 0, col]), torch.deg2rad(mean[row, 1, col])
        return torch.stack([torch.cos(lat) * torch.cos(lon), torch.cos(lat) * torch.sin(lon), torch.sin(lat)])

    first, last = unit(torch.zeros_like(ns)), unit(ns)
    ok = torch.isfinite(first).all(dim=0) & torch.isfinite(last).all(dim=0)
    # 1e-7 rad (0.6 m) for the rounding of the chords, as candidate_pairs
    reach = (float(within_km) + float(margin_km)) / EARTH_RADIUS_KM + 1e-7
    found = []
    for lo in range(0, B, int(chunk)):
        hi = min(lo + int(chunk), B)

        def angle(u, v):  # (hi - lo, B) angles from chords: 2 asin(|u - v| / 2)
            chord = (u[:, lo:hi, None] - v[:, None, :]).norm(dim=0)
            return 2.0 * torch.asin((0.5 * chord).clamp(max=1.0))

        if reverse:
            far = torch.maximum(angle(first, last), angle(last, first))
        else:
            far = torch.maximum(angle(first, first), angle(last, last))
        keep = (far <= reach) & ok[lo:hi, None] & ok[None, :] & (col[None, :] > col[lo:hi, None])
        ij = keep.nonzero()                                                           # row-major: sorted by (i, j)
        ij[:, 0] += lo
        found.append(ij)
    return torch.cat(found).to(torch.int32)


def route_candidates(db: "DeviceBatch", within_km, margin_km: float = 0.0, reverse: bool = False, chunk: int = 2048):
    """The pairs of a resident batch worth giving to ``DeviceBatch.route_metrics`` when the question is "Frechet distance at
    most ``within_km``": an int32 (P, 2) device tensor of (i, j), i < j, sorted by (i, j).  Torch plumbing without a kernel, on
    ``sm_mean`` (``fwd_mean`` when the batch has no smoother).  Every monotone coupling matches first row with first and last
    with last, so the Frechet distance is at least the larger of the two endpoint distances (with ``reverse``: first against
    last and last against first); a pair is kept when that is at most ``within_km`` + ``margin_km``.  For the tested tracks the
    pruning is exact; ``margin_km`` is the allowance for samples of the posterior (a few standard deviations of position).
    The B x B test runs in blocks of ``chunk`` rows.  Tracks with a non-finite end pair with nothing."""
    mean = db.sm_mean if db.sm_mean is not None else db.fwd_mean
    if mean is None:
        raise ValueError("route_candidates() needs sm_mean or fwd_mean, and this batch was built without histories")
    B = db.ntracks
    nsteps = db.t["nsteps"][db.lo:db.lo + B]
    with db.torch.cuda.device(db.device):
        return route_endpoint_pairs(mean, nsteps, within_km, margin_km, reverse, chunk)


def route_statistics(hb_or_db, pairs, within_km, nsamples: int, seed: int = 0, chunk: int = 16, band: int = 0,
                     reverse: bool = False, model: str = "sphere", quantiles=None, dtw: bool = False, device="cuda:0"):
    """How sure one can be that two ships followed one route: ``nsamples`` posterior tracks per ship are drawn
    (``DeviceBatch.sample_smoothed``), sample s of one ship held against sample s of the other as curves
    (``DeviceBatch.route_metrics``) and discarded, ``chunk`` samples at a time, with the generator discipline of
    ``encounter_statistics``: one draw buffer refilled from one generator, so the draws depend on ``(seed, chunk)`` and with
    ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.  What is kept between chunks are counts and
    sums per pair, added to sample by sample: memory does not grow with ``nsamples`` unless ``quantiles`` are asked for, which
    keep nsamples x P doubles.  Given a ``HostBatch`` it uploads it and runs the forward pass and the smoother first; a
    ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``pairs``, ``band``, ``reverse`` and
    ``model`` as in ``route_metrics``.

    Returns a dict of NumPy arrays per pair, (P,): ``frechet_smoothed``, ``frechet_at_smoothed`` (P, 2) and ``status`` of the
    smoothed tracks ``sm_mean``; ``prob_within``, the share of samples with frechet <= ``within_km``; ``frechet_mean`` over the
    samples without a status bit (NaN where there is none); ``nbad``, the number of samples with a status bit; with
    ``quantiles`` ``frechet_quantiles`` (len(quantiles), P); with ``dtw`` ``dtw_smoothed``, ``dtw_len_smoothed`` and
    ``dtw_per_cell_mean``, the mean of dtw / dtw_len; and ``sample_status`` (B,), the sampler's STE_STATUS_* bits."""
    import warnings

    within_km = float(within_km)
    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "route_statistics")
    torch = db.torch
    kw = dict(dtw=dtw, band=band, reverse=reverse, model=model)
    smoothed = db.route_metrics(db.sm_mean, pairs, **kw)
    P = int(smoothed["status"].shape[1])
    f64 = dict(dtype=torch.float64, device=db.device)
    within, nbad = (torch.zeros((P,), dtype=torch.int32, device=db.device) for _ in range(2))
    fsum, wsum = torch.zeros((P,), **f64), torch.zeros((P,), **f64)
    kept = torch.empty((nsamples, P), **f64) if quantiles is not None else None
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for i, n, samples in chunks:
        m = db.route_metrics(samples, pairs, **kw)
        good = m["status"] == 0
        fre = torch.where(good, m["frechet"], torch.zeros_like(m["frechet"]))
        for s in range(n):  # sample by sample: the sums take their terms in sample order whatever the chunk
            within += good[s] & (m["frechet"][s] <= within_km)
            nbad += ~good[s]
            fsum += fre[s]
            if dtw:
                wsum += torch.where(good[s], m["dtw"][s] / m["dtw_len"][s].clamp(min=1), torch.zeros_like(fsum))
        if kept is not None:
            kept[i:i + n] = m["frechet"]
    status = chunks.status
    count = nsamples - nbad.cpu().numpy()
    out = {"frechet_smoothed": smoothed["frechet"][0].cpu().numpy(), "frechet_at_smoothed": smoothed["frechet_at"][0].cpu().numpy(),
           "status": smoothed["status"][0].cpu().numpy(), "prob_within": within.cpu().numpy() / float(nsamples),
           "nbad": nsamples - count}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["frechet_mean"] = np.where(count > 0, fsum.cpu().numpy() / count, np.nan)
        if dtw:
            out["dtw_smoothed"], out["dtw_len_smoothed"] = smoothed["dtw"][0].cpu().numpy(), smoothed["dtw_len"][0].cpu().numpy()
            out["dtw_per_cell_mean"] = np.where(count > 0, wsum.cpu().numpy() / count, np.nan)
    if kept is not None:
        with warnings.catch_warnings():  # a pair no sample gives a value: all-NaN column, NaN out
            warnings.simplefilter("ignore", RuntimeWarning)
            out["frechet_quantiles"] = np.nanquantile(kept.cpu().numpy(), np.asarray(quantiles, dtype=np.float64), axis=0)
    out["sample_status"] = status.cpu().numpy()
    return out


def curve_distance(curves_a, curves_b, dtw: bool = False, band: int = 0, reverse: bool = False, model: str = "sphere",
                   device="cuda:0"):
    """Frechet distance (and, with ``dtw``, time-warping cost) of pairs of curves that are no tracks of a batch: a filtered
    track against its observations, a GP track, a Savitzky-Golay track.  ``curves_a`` and ``curves_b``: equally long lists of
    (n, 2) lon / lat arrays in degrees, of any lengths n >= 1 (a single (n, 2) array is a list of one); pair k is (a_k, b_k).
    They are packed into a ``states`` tensor whose track 2k is a_k and track 2k + 1 is b_k and given to
    ste_route_metrics_f64 through a batch struct that carries nothing but B, Nmax and nsteps: the call reads nothing else.
    ``band``, ``reverse`` and ``model`` as in ``DeviceBatch.route_metrics``.  Returns a dict of NumPy arrays per pair:
    ``frechet`` (K,) km, ``frechet_at`` (K, 2), the rows of a_k and b_k whose distance it is, ``status`` (K,) and with ``dtw``
    ``dtw`` and ``dtw_len``."""
    import torch

    def as_list(c):
        if isinstance(c, np.ndarray) and c.ndim == 2:
            return [c]
        return list(c)

    ca = [np.asarray(c, dtype=np.float64) for c in as_list(curves_a)]
    cb = [np.asarray(c, dtype=np.float64) for c in as_list(curves_b)]
    if len(ca) != len(cb) or not ca:
        raise ValueError(f"curves_a and curves_b must be equally long, non-empty lists, got {len(ca)} and {len(cb)}")
    for c in ca + cb:
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1:
            raise ValueError(f"a curve must be an (n, 2) array of lon / lat with n >= 1, got shape {c.shape}")
    model_id = _metric_model(model)
    band = int(band)
    if not 0 <= band < 2 ** 31:
        raise ValueError(f"band must be >= 0 (0 = no band) and below 2^31, got {band!r}")
    lib = binding.require_gpu()
    dev = torch.device(device)
    K = len(ca)
    B, rows = 2 * K, max(c.shape[0] for c in ca + cb)
    host = np.zeros((1, rows, 4, B))
    nsteps = np.empty((B,), dtype=np.int32)
    for k in range(K):
        for t, c in ((2 * k, ca[k]), (2 * k + 1, cb[k])):
            host[0, :c.shape[0], :2, t] = c
            nsteps[t] = c.shape[0] - 1
    with torch.cuda.device(dev):
        states = torch.from_numpy(host).to(dev)
        ns = torch.from_numpy(nsteps).to(dev)
        pr = torch.arange(B, dtype=torch.int32, device=dev).reshape(K, 2)
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.nsteps = B, rows - 1, ns.data_ptr()
        keep = [states, ns, pr]
        out = _route_call(lib, torch, s, states, 1, pr, dtw, band, reverse, model_id, dev,
                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), keep)
        res = {k: v[0].cpu().numpy() for k, v in out.items()}  # the download waits for the launch
    return res


KM_PER_DEG = 6378.137 * np.pi / 180.0  # Kd: km per degree of a great circle on the sphere of the leg functions


class SimplifiedTrack(dict):
    """The kept rows of one ship (``simplified_tracks``): ``rows``, ``lon``, ``lat``, ``speed``, ``heading``, ``time`` as (n,)
    arrays, and ``worst_km`` and ``status`` of the simplification."""

    def curve(self) -> np.ndarray:
        """(n, 2) lon / lat: what ``curve_distance`` and ``track_lines`` take."""
        return np.column_stack([self["lon"], self["lat"]])

    def curves(self):
        return [self.curve()]


class SimplifiedTracks:
    """The kept rows of every ship of a batch (``simplified_tracks``), in the batch's slot order: a sequence of
    ``SimplifiedTrack``, made on access as views of the flat arrays that came from the device (``rows``, ``lon``, ``lat``,
    ``speed``, ``heading``, ship after ship; ship b owns ``offsets[b]:offsets[b + 1]``); a ship's ``time`` is summed from the
    host batch's ``dt`` (Nmax, B) when the ship is asked for."""

    FIELDS = ("rows", "lon", "lat", "speed", "heading")

    def __init__(self, flat: dict, offsets: np.ndarray, worst_km: np.ndarray, status: np.ndarray, dt: np.ndarray):
        self.flat, self.offsets, self.worst_km, self.status, self.dt = flat, offsets, worst_km, status, dt

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def __getitem__(self, b: int) -> SimplifiedTrack:
        n = len(self)
        if not -n <= b < n:
            raise IndexError(f"ship {b} of {n}")
        b %= n
        sl = slice(int(self.offsets[b]), int(self.offsets[b + 1]))
        clock = np.concatenate([[0.0], np.cumsum(self.dt[:, b])])  # T_0 = 0, T_{k+1} = T_k + dt_k, in order: the kernel's clock
        return SimplifiedTrack({k: self.flat[k][sl] for k in self.FIELDS}, time=clock[self.flat["rows"][sl]],
                               worst_km=float(self.worst_km[b]), status=int(self.status[b]))

    def __iter__(self):
        return (self[b] for b in range(len(self)))

    def curves(self):
        """A list of (n, 2) lon / lat arrays, one per ship: what ``curve_distance`` and ``track_lines`` take."""
        return [t.curve() for t in self]


def simplified_tracks(hb_or_db, tolerance_km, which: str = "smoothed", shape: bool = False, lon_scale="track",
                      device="cuda:0") -> SimplifiedTracks:
    """The smoothed (``which="smoothed"``) or filtered (``"filtered"``) tracks of a batch, simplified within ``tolerance_km``
    on the device (``DeviceBatch.simplify_tracks``), kept rows only: per ship a ``SimplifiedTrack`` with ``rows`` (the
    indices of the kept rows), ``lon``, ``lat``, ``speed``, ``heading`` (the kept rows of the history, their bits) and ``time``
    (hours from row 0, ``dt`` summed in order).  A ``HostBatch`` is uploaded and ``run()``; a ``DeviceBatch`` (or a window of
    one) is taken to hold its histories.  The gather is a masked select on the device, and one copy of the kept rows crosses
    PCIe where ``download`` ships every row of every history."""
    import torch

    if which not in ("smoothed", "filtered"):
        raise ValueError(f"which must be 'smoothed' or 'filtered', got {which!r}")
    if isinstance(hb_or_db, DeviceBatch):
        db = hb_or_db
    else:
        db = DeviceBatch(hb_or_db, device=device, alloc_smoothed=which == "smoothed")
        db.run() if which == "smoothed" else db.forward()
    mean = db.sm_mean if which == "smoothed" else db.fwd_mean
    if mean is None:
        raise ValueError(f"this batch holds no {which} history")
    out = db.simplify_tracks(mean, tolerance_km, shape=shape, lon_scale=lon_scale, compact=False)
    B, lo = db.ntracks, db.lo
    flags = out["keep"][0].T.bool()  # (B, Nmax+1)
    kept = mean.permute(2, 0, 1)[flags]  # (K, 4), ship after ship
    row = flags.nonzero()[:, 1]
    packed = torch.cat([kept, row.to(torch.float64)[:, None]], dim=1).cpu().numpy()  # the one copy of the kept rows
    small = torch.stack([out["nkeep"][0].double(), out["status"][0].double(), out["worst_km"][0]]).cpu().numpy()
    counts = small[0].astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    lon, lat, speed, heading, rowf = np.ascontiguousarray(packed.T)
    rows = rowf.astype(np.int64)
    return SimplifiedTracks(dict(rows=rows, lon=lon, lat=lat, speed=speed, heading=heading), offsets, small[2], small[1],
                            db.hb.dt[:, lo:lo + B])


def position_ellipse(count, moments, anchor_lat, prob: float = 0.95):
    """Mean offset, covariance and error ellipse in km from the moments of ``DeviceBatch.positions_at``: NumPy on (Q,) arrays.
    ``count`` (Q,), ``moments`` (5, Q) = sums of dx, dy, dx dx, dx dy, dy dy in degrees about the anchor, ``anchor_lat`` (Q,)
    degrees.  East is dx times Kd cos(anchor lat) and north dy times Kd, Kd = 6378.137 pi / 180.  Returns a dict:
    ``mean_east_km``, ``mean_north_km`` (NaN where count is 0); ``cov_km`` (Q, 2, 2), ddof = 1, NaN where count < 2;
    ``semi_major_km``, ``semi_minor_km``, the square roots of the eigenvalues of ``cov_km`` times sqrt(-2 ln(1 - prob)) -- the
    ellipse that holds ``prob`` of a bivariate normal -- and ``orientation_deg`` in [0, 180), the major axis clockwise from
    north."""
    prob = float(prob)
    if not 0.0 < prob < 1.0:
        raise ValueError(f"prob must lie strictly between 0 and 1, got {prob!r}")
    n = np.asarray(count, dtype=np.float64)
    m = np.asarray(moments, dtype=np.float64)
    lat = np.asarray(anchor_lat, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != 5 or n.shape != m.shape[1:] or lat.shape != n.shape:
        raise ValueError(f"count (Q,), moments (5, Q) and anchor_lat (Q,) are wanted, got {n.shape}, {m.shape} and {lat.shape}")
    ke, kn = KM_PER_DEG * np.cos(np.radians(lat)), KM_PER_DEG
    with np.errstate(divide="ignore", invalid="ignore"):
        mx, my = m[0] / n, m[1] / n
        dof = np.where(n >= 2, n - 1.0, np.nan)
        cxx, cxy, cyy = (m[2] - m[0] * mx) / dof, (m[3] - m[0] * my) / dof, (m[4] - m[1] * my) / dof
        a, b, c = cxx * ke * ke, cxy * ke * kn, cyy * kn * kn
        half, mid = np.hypot(0.5 * (a - c), b), 0.5 * (a + c)
        scale = np.sqrt(-2.0 * np.log1p(-prob))
        major, minor = scale * np.sqrt(np.maximum(mid + half, 0.0)), scale * np.sqrt(np.maximum(mid - half, 0.0))
        # the major axis makes 0.5 atan2(2 b, a - c) with east, counter-clockwise: 90 degrees minus that from north, clockwise
        orient = np.where(np.isnan(half), np.nan, (90.0 - 0.5 * np.degrees(np.arctan2(2.0 * b, a - c))) % 180.0)
    cov = np.stack([np.stack([a, b], axis=-1), np.stack([b, c], axis=-1)], axis=-2)
    return {"mean_east_km": mx * ke, "mean_north_km": my * kn, "cov_km": cov, "semi_major_km": major, "semi_minor_km": minor,
            "orientation_deg": orient}


def position_statistics(hb_or_db, qtrack, qtime, nsamples: int, seed: int = 0, chunk: int = 16, t0=None, prob: float = 0.95,
                        device="cuda:0"):
    """Position at given clock times with the uncertainty of the smoothing posterior, per query: ``nsamples`` posterior tracks
    are drawn (``DeviceBatch.sample_smoothed``), interpolated (``DeviceBatch.positions_at``) and discarded, ``chunk`` samples at
    a time, with the generator discipline of ``region_statistics``: one draw buffer refilled from one generator, so the draws
    depend on ``(seed, chunk)`` and with ``chunk >= nsamples`` they are those of ``sample_smoothed(nsamples, seed)``.  Only the
    count and the five moments per query survive a chunk, continued on the device with the bits of one pass, so memory does not
    grow with ``nsamples``.  The anchor of the moments is the smoothed position, ``positions_at(db.sm_mean, ...)``; the knot
    times are summed once and reused; the queries are sorted once.  Given a ``HostBatch`` it uploads it and runs the forward pass
    and the smoother first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``qtrack``,
    ``qtime`` and ``t0`` as in ``positions_at``.

    Returns a dict of NumPy arrays per query: ``lon``, ``lat``, ``speed``, ``heading``, ``step``, ``frac``, ``status`` of the
    smoothed track; ``count``, the samples with a finite position; and what ``position_ellipse`` makes of the moments:
    ``mean_east_km``, ``mean_north_km`` (the samples' mean about the smoothed position), ``cov_km`` (Q, 2, 2),
    ``semi_major_km``, ``semi_minor_km``, ``orientation_deg`` for ``prob``; and ``sample_status`` (B,), the sampler's
    STE_STATUS_* bits per track."""
    if not 0.0 < float(prob) < 1.0:
        raise ValueError(f"prob must lie strictly between 0 and 1, got {prob!r}")
    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "position_statistics")
    torch = db.torch
    smoothed = db.positions_at(db.sm_mean, qtrack, qtime, t0=t0, velocity=True)
    Q = int(smoothed["status"].shape[0])
    # the kernel's order once, for every chunk: by (track, time)
    qt = torch.as_tensor(np.asarray(qtrack) if not isinstance(qtrack, torch.Tensor) else qtrack).to(db.device)
    tq = torch.as_tensor(qtime, dtype=torch.float64).to(db.device)
    by_time = torch.sort(tq, stable=True).indices
    perm = by_time[torch.sort(qt[by_time], stable=True).indices]
    qt, tq = qt[perm], tq[perm]
    anchor = torch.stack([smoothed["lon"][0], smoothed["lat"][0]])[:, perm].contiguous()
    knots = smoothed["knots"]
    acc = (torch.zeros((Q,), dtype=torch.int32, device=db.device), torch.zeros((5, Q), dtype=torch.float64, device=db.device))
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for _, _, samples in chunks:
        db.positions_at(samples, qt, tq, t0=t0, anchor=anchor, accumulate=acc, knots=knots, sort=False)
    status = chunks.status
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(Q, device=db.device)
    count, moments = acc[0][inv].cpu().numpy(), acc[1][:, inv].cpu().numpy()
    out = {k: smoothed[k][0].cpu().numpy() for k in ("lon", "lat", "speed", "heading")}
    out.update({k: smoothed[k].cpu().numpy() for k in ("step", "frac", "status")})
    out["count"] = count
    out.update(position_ellipse(count, moments, out["lat"], prob))
    out["sample_status"] = status.cpu().numpy()
    return out


def covariance_ellipse(cxx, cxy, cyy, anchor_lat, prob: float = 0.95):
    """Covariance and error ellipse in km from a position covariance in degrees squared (``DeviceBatch.position_covariance_at``:
    lon-lon, lon-lat, lat-lat): NumPy on (Q,) arrays, with the km scaling, the ellipse and the orientation of
    ``position_ellipse`` -- east is dx times Kd cos(anchor lat) and north dy times Kd, Kd = 6378.137 pi / 180.  Returns a dict:
    ``cov_km`` (Q, 2, 2); ``semi_major_km``, ``semi_minor_km``, the square roots of its eigenvalues times
    sqrt(-2 ln(1 - prob)); ``orientation_deg`` in [0, 180), the major axis clockwise from north.  NaN in, NaN out."""
    prob = float(prob)
    if not 0.0 < prob < 1.0:
        raise ValueError(f"prob must lie strictly between 0 and 1, got {prob!r}")
    cxx, cxy, cyy = (np.asarray(v, dtype=np.float64) for v in (cxx, cxy, cyy))
    lat = np.asarray(anchor_lat, dtype=np.float64)
    if not (cxx.shape == cxy.shape == cyy.shape == lat.shape) or cxx.ndim != 1:
        raise ValueError(f"cxx, cxy, cyy and anchor_lat are wanted as (Q,) arrays, got {cxx.shape}, {cxy.shape}, {cyy.shape} and "
                         f"{lat.shape}")
    ke, kn = KM_PER_DEG * np.cos(np.radians(lat)), KM_PER_DEG
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b, c = cxx * ke * ke, cxy * ke * kn, cyy * kn * kn
        half, mid = np.hypot(0.5 * (a - c), b), 0.5 * (a + c)
        scale = np.sqrt(-2.0 * np.log1p(-prob))
        major, minor = scale * np.sqrt(np.maximum(mid + half, 0.0)), scale * np.sqrt(np.maximum(mid - half, 0.0))
        orient = np.where(np.isnan(half), np.nan, (90.0 - 0.5 * np.degrees(np.arctan2(2.0 * b, a - c))) % 180.0)
    cov = np.stack([np.stack([a, b], axis=-1), np.stack([b, c], axis=-1)], axis=-2)
    return {"cov_km": cov, "semi_major_km": major, "semi_minor_km": minor, "orientation_deg": orient}


def position_covariance(hb_or_db, qtrack, qtime, t0=None, prob: float = 0.95, device="cuda:0"):
    """Position at given clock times with its exact covariance under the smoothing posterior, per query, without samples: the
    sample-free sibling of ``position_statistics`` ("Lag-one covariance").  The smoothed track is interpolated
    (``DeviceBatch.positions_at``) and its covariance follows in closed form from ``sm_cov`` and the smoother's lag-one
    covariance (``DeviceBatch.position_covariance_at``, in its position-only form: memory of order Nmax B 4 + Q).  Given a
    ``HostBatch`` it uploads it and runs the forward pass and the smoother first; a ``DeviceBatch`` (or a window of one) is
    taken to hold a completed ``run()``.  ``qtrack``, ``qtime`` and ``t0`` as in ``positions_at``.

    Returns a dict of NumPy arrays per query: ``lon``, ``lat``, ``speed``, ``heading``, ``step``, ``frac``, ``status`` of the
    smoothed track; what ``covariance_ellipse`` makes of the covariance: ``cov_km`` (Q, 2, 2), ``semi_major_km``,
    ``semi_minor_km``, ``orientation_deg`` for ``prob``, NaN where the smoothed position is (a query that is not located, a
    broken step); and ``lag_status`` (B,), the STE_STATUS_* bits of the lag-one call per track."""
    if not 0.0 < float(prob) < 1.0:
        raise ValueError(f"prob must lie strictly between 0 and 1, got {prob!r}")
    db = _posterior_batch(hb_or_db, 1, 1, device, "position_covariance")[0]
    smoothed = db.positions_at(db.sm_mean, qtrack, qtime, t0=t0, velocity=True)
    pc = db.position_covariance_at(qtrack, qtime, t0=t0, knots=smoothed["knots"])
    out = {k: smoothed[k][0].cpu().numpy() for k in ("lon", "lat", "speed", "heading")}
    out.update({k: smoothed[k].cpu().numpy() for k in ("step", "frac", "status")})
    pcov = pc["pcov"].cpu().numpy()
    pcov[:, np.isnan(out["lon"]) | np.isnan(out["lat"])] = np.nan
    out.update(covariance_ellipse(pcov[0], pcov[1], pcov[2], out["lat"], prob))
    out["lag_status"] = pc["lag_status"].cpu().numpy()
    return out


def field_statistics(hb_or_db, field: "TrackField", qtrack, qtime, nsamples: int, seed: int = 0, chunk: int = 16, t0=None,
                     nearest: bool = False, min_cover: float = 0.0, device="cuda:0"):
    """The value of a space-time gridded field at given clock times with the uncertainty of the smoothing posterior, per query
    (an observation hour of a ship): ``nsamples`` posterior tracks are drawn (``DeviceBatch.sample_smoothed``), the field is
    read where each was (``DeviceBatch.field_at``) and they are discarded, ``chunk`` samples at a time, with the generator
    discipline of ``position_statistics``: the draws depend on ``(seed, chunk)`` and with ``chunk >= nsamples`` they are those
    of ``sample_smoothed(nsamples, seed)``.  Only the counts, the two moments and the extremes per query survive a chunk,
    continued on the device with the bits of one pass: no (nsamples, Q) array exists anywhere and memory is of order Q.  The
    anchor of the moments is the value at the smoothed track, ``field_at(db.sm_mean, ...)``, 0.0 where that is NaN; the knot
    times are summed once and the queries sorted once.  Given a ``HostBatch`` it uploads it and runs the forward pass and the
    smoother first; a ``DeviceBatch`` (or a window of one) is taken to hold a completed ``run()``.  ``field``, ``qtrack``,
    ``qtime``, ``t0``, ``nearest`` and ``min_cover`` as in ``field_at``.

    Returns a dict of NumPy arrays per query: ``anchor``, the value at the smoothed track (NaN where it has none); ``mean`` and
    ``std`` (ddof 1, NaN below two) of the samples' values; ``min``, ``max``; ``n``, the samples with a value; ``p_nodata`` and
    ``p_off``, the shares of the samples on the grid without a value and off the grid; ``status``, the STE_POS_* bits and
    STE_FLD_TIME_OUTSIDE; and ``sample_status`` (B,), the sampler's STE_STATUS_* bits per track."""
    db, nsamples, chunk = _posterior_batch(hb_or_db, nsamples, chunk, device, "field_statistics")
    torch = db.torch
    knots = db.track_knots()
    kw = dict(t0=t0, nearest=nearest, min_cover=min_cover, knots=knots)
    smoothed = db.field_at(db.sm_mean, field, qtrack, qtime, **kw)
    Q = int(smoothed["status"].shape[0])
    # the kernel's order once, for every chunk: by (track, time)
    qt = torch.as_tensor(np.asarray(qtrack) if not isinstance(qtrack, torch.Tensor) else qtrack).to(db.device)
    tq = torch.as_tensor(qtime, dtype=torch.float64).to(db.device)
    by_time = torch.sort(tq, stable=True).indices
    perm = by_time[torch.sort(qt[by_time], stable=True).indices]
    qt, tq = qt[perm], tq[perm]
    anchor = smoothed["value"][0]
    vanchor = torch.where(torch.isnan(anchor), torch.zeros_like(anchor), anchor)[perm].contiguous()
    f64 = dict(dtype=torch.float64, device=db.device)
    acc = (torch.zeros((3, Q), dtype=torch.int32, device=db.device), torch.zeros((2, Q), **f64),
           torch.full((Q,), float("nan"), **f64), torch.full((Q,), float("nan"), **f64))
    chunks = _PosteriorChunks(db, nsamples, seed, chunk)
    for _, _, samples in chunks:
        db.field_at(samples, field, qt, tq, vanchor=vanchor, accumulate=acc, per_sample=False, sort=False, **kw)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(Q, device=db.device)
    count, moments, vmin, vmax = (a[..., inv].cpu().numpy() for a in acc)
    van = vanchor[inv].cpu().numpy()
    n = count[0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        md = moments[0] / n
        var = (moments[1] - moments[0] * md) / np.where(n >= 2, n - 1.0, np.nan)
        std = np.sqrt(np.maximum(var, 0.0))
    return {"anchor": anchor.cpu().numpy(), "mean": van + md, "std": std, "min": vmin, "max": vmax, "n": count[0],
            "p_nodata": count[1] / float(nsamples), "p_off": count[2] / float(nsamples), "status": smoothed["status"].cpu().numpy(),
            "sample_status": chunks.status.cpu().numpy()}


@dataclasses.dataclass
class LogLikelihood:
    """Innovation log-likelihood of a forward pass per track (include/ste.h: ste_ukf_loglik_f64).  ``loglik``: sum over the
    track's updates of l_u = -1/2 (y^T S^+ y + sum log lambda_i + r log 2 pi) ("Innovation log-likelihood");
    ``dof``: sum of the ranks r; ``nupd``: updates summed; ``status``: the pass's STE_STATUS_* bits; ``nis``: y^T S^+ y per
    history row, or None.  From ``log_likelihood_grid`` every array has a leading candidate axis."""

    loglik: np.ndarray
    dof: np.ndarray
    nupd: np.ndarray
    status: np.ndarray
    nis: Optional[np.ndarray] = None


def log_likelihood_grid(hb: HostBatch, candidates: Sequence, device="cuda:0", nis: bool = False) -> LogLikelihood:
    """
    Score candidate noise models on the device: one forward pass that writes no histories per (Q, R) pair of
    ``candidates``, over every track of ``hb`` (uploaded once).  Each pair is checked like ``pack_tracks`` checks its
    matrices (4 x 4, symmetric); the rest of the filter (H, P0, flags, recorded noise) is the HostBatch's.  A candidate
    whose R leaves the closed-form structure (H = diag(1, 1, 0, 0), R confined to the leading 2 x 2 block) takes the
    general update route.  Returns a ``LogLikelihood`` whose arrays are [K, B] (``nis``: [K, B, Nmax+1]), tracks in the
    HostBatch's slot order.  ``best_noise`` picks from it.
    """
    import torch

    cands = [(_as44(Q, "Q", True), _as44(R, "R", True)) for Q, R in candidates]
    if not cands:
        raise ValueError("no candidates")
    db = DeviceBatch(hb, device=device, alloc_smoothed=False, fuse_gains=False, histories=False)
    K, B, N = len(cands), hb.B, hb.Nmax
    dev = dict(device=db.device)
    ll = torch.empty((K, B), dtype=torch.float64, **dev)
    dof = torch.empty((K, B), dtype=torch.int32, **dev)
    nupd = torch.empty((K, B), dtype=torch.int32, **dev)
    status = torch.empty((K, B), dtype=torch.int32, **dev)
    nis_t = torch.full((K, N + 1, B), float("nan"), dtype=torch.float64, **dev) if nis else None
    _launch_loglik_grid(db, cands, ll, dof, nupd, status, nis_t)
    return LogLikelihood(loglik=ll.cpu().numpy(), dof=dof.cpu().numpy(), nupd=nupd.cpu().numpy(),
                         status=status.cpu().numpy(),
                         nis=None if nis_t is None else nis_t.permute(0, 2, 1).cpu().numpy())


# Streams the candidates of a grid are spread over.  A likelihood-only pass is one wave per 64 tracks for the whole pass, so
# a 10 000-track batch is 157 waves on 1 024 SIMDs: candidates on separate streams run side by side.  Four: the hardware
# queues a process opens by default.
GRID_STREAMS = 4


def _launch_loglik_grid(db: DeviceBatch, cands, ll, dof, nupd, status, nis_t=None, streams=None):
    """One likelihood-only launch per candidate (Q, R) of ``cands`` on ``db`` (a ``histories=False`` batch), candidate k
    writing row k of the [K, B] tensors (``nis_t``: [K, Nmax+1, B]); launches go round-robin over ``streams`` (default:
    ``GRID_STREAMS`` new ones), which wait for the batch's upload, and the current stream waits for all of them."""
    torch = db.torch
    cur = torch.cuda.current_stream(db.device)
    if streams is None:
        streams = [torch.cuda.Stream(db.device) for _ in range(min(len(cands), GRID_STREAMS))]
    for st in streams:
        st.wait_event(db._uploaded)
        st.wait_stream(cur)  # the output tensors were allocated / filled on the current stream
    s = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
    s.flags = (s.flags & ~binding.STE_FLAG_LANES_4) | binding.STE_FLAG_LANES_1
    for k, (Q, R) in enumerate(cands):  # Q and R are host pointers, read at call time: `cands` holds them
        s.Q, s.R = Q.ctypes.data, R.ctypes.data
        s.status = status[k].data_ptr()
        lk = binding.SteUkfLoglikF64(ll[k].data_ptr(), dof[k].data_ptr(), nupd[k].data_ptr(),
                                     None if nis_t is None else nis_t[k].data_ptr())
        binding.check(db.lib.ste_ukf_forward_loglik_f64(C.byref(s), C.byref(lk), db._stream(streams[k % len(streams)])),
                      "ste_ukf_forward_loglik_f64")
    for st in streams:
        cur.wait_stream(st)


@dataclasses.dataclass
class NoiseChoice:
    """``best_noise``'s answer.  Fleet: ``index`` is the candidate with the largest fleet-summed loglik (-1, with NaN sums,
    when every track was left out), ``loglik`` the [K] sums, ``excluded`` the number of tracks left out of every sum.  Per track: ``index`` [B] (-1 where no candidate gave a
    usable value), ``loglik`` [B] the chosen values, ``excluded`` the number of tracks without any."""

    index: object
    loglik: np.ndarray
    excluded: int


def best_noise(grid: LogLikelihood, per_track: bool = False) -> NoiseChoice:
    """The candidate of ``log_likelihood_grid`` with the largest log-likelihood, summed over the fleet or per track.  A
    (candidate, track) value is unusable when the track's status carries STE_STATUS_NAN or its loglik is not finite.  For
    the fleet sum a track is left out of every candidate's sum if any candidate's value for it is unusable -- otherwise a
    candidate would gain by losing tracks --; ``excluded`` says how many were left out."""
    ll = np.asarray(grid.loglik, dtype=np.float64)
    ok = np.isfinite(ll) & ((np.asarray(grid.status) & binding.STE_STATUS_NAN) == 0)
    if per_track:
        masked = np.where(ok, ll, -np.inf)
        idx = np.argmax(masked, axis=0)
        none = ~ok.any(axis=0)
        idx = np.where(none, -1, idx)
        return NoiseChoice(index=idx, loglik=np.where(none, np.nan, masked[np.maximum(idx, 0), np.arange(ll.shape[1])]),
                           excluded=int(none.sum()))
    keep = ok.all(axis=0)
    if not keep.any():  # nothing to compare: no candidate wins
        return NoiseChoice(index=-1, loglik=np.full(ll.shape[0], np.nan), excluded=int(keep.size))
    sums = np.where(keep[None, :], ll, 0.0).sum(axis=1)
    return NoiseChoice(index=int(np.argmax(sums)), loglik=sums, excluded=int((~keep).sum()))


@dataclasses.dataclass
class NoiseFit:
    """``fit_measurement_noise``'s answer, G groups.  ``R`` (G, 4, 4): the winning iterate's R of every group (for a group
    whose winner is iterate 0, the R its first member started with); ``R_trace`` (iterations + 1, G, 4, 4): every iterate, a
    stopped group repeating its last.  ``groups`` (B,): the group of every SLOT of
    ``host_batch`` (``host_batch.order`` maps slots to the caller's tracks); ``labels`` (G,): the caller's label of every
    group.  ``loglik`` (iterations + 1, G): the group's log-likelihood under every iterate, iterate 0 being the R the batch
    came with, summed over the tracks that were usable under every iterate.  ``best_iter``, ``converged``, ``nobs`` (G,): the
    winning iterate, whether the group's R settled within ``rtol`` before ``max_iter``, and the updates the group's last
    M-step summed.  ``excluded``: slots left out of every sum (a NaN log-likelihood or an unusable status under some
    iterate).  ``host_batch``: the batch with the fitted ``R_tracks``; ``device_batch``: the resident batch after a ``run()``
    with them."""

    R: np.ndarray
    R_trace: np.ndarray
    groups: np.ndarray
    labels: np.ndarray
    loglik: np.ndarray
    best_iter: np.ndarray
    converged: np.ndarray
    nobs: np.ndarray
    excluded: np.ndarray
    host_batch: HostBatch
    device_batch: "DeviceBatch"


def _noise_fit_groups(hb: HostBatch, groups):
    """``groups`` of ``fit_measurement_noise`` as (group of every slot (B,), the caller's label of every group (G,))."""
    B = hb.B
    order = np.arange(B) if hb.order is None else np.asarray(hb.order)
    if groups is None:
        return np.zeros(B, dtype=np.int64), np.zeros(1, dtype=np.int64)
    if isinstance(groups, str):
        if groups != "track":
            raise ValueError(f"groups must be None (one group), 'track' or an integer array ({B},), got {groups!r}")
        return order.astype(np.int64), np.arange(B)
    lab = np.asarray(groups)
    if lab.shape != (B,) or lab.dtype.kind not in "iu":
        raise ValueError(f"groups must be None (one group), 'track' or an integer array of one label per track, ({B},); got "
                         f"shape {lab.shape}, dtype {lab.dtype}")
    labels, index = np.unique(lab, return_inverse=True)
    return index.reshape(B)[order].astype(np.int64), labels


def _ordered_sum(x) -> float:
    """x[0] + x[1] + ... in that order (np.sum adds pairwise)."""
    return float(np.cumsum(np.asarray(x, dtype=np.float64))[-1]) if len(x) else 0.0


def fit_measurement_noise(hb: HostBatch, groups=None, structure: str = "scalar", max_iter: int = 20, rtol: float = 1e-3,
                          device="cuda:0") -> NoiseFit:
    """
    Fit the measurement noise R to the data by EM on the device ("Noise fit"), one R per group of tracks.

    ``groups``: None (the whole batch is one group), ``"track"`` (every track its own) or an integer array (B,) of labels in
    the caller's track order.  ``structure``: what R may be -- ``"scalar"`` r diag(1, 1, 0, 0), ``"diag2"``
    diag(r0, r1, 0, 0) or ``"block2"`` a full leading 2 x 2 block.  Q, H and P0 stay the batch's.

    Every iteration is an E-step (``log_likelihood`` + ``backward``: the smoothed track under the current R, and the
    log-likelihood of that R), ``measurement_moments`` and ``update_measurement_noise``.  A group stops when the largest
    relative change of the non-zero entries of its R falls below ``rtol`` (or its M-step fails); the loop ends when every
    group has stopped or after ``max_iter`` M-steps, and one more E-step scores the last iterate.  EM with an unscented
    smoother is not strictly monotone, so per group the iterate with the highest log-likelihood is returned, not the last
    one; iterate 0 is the R the batch came with and can win.  The batch ends holding the histories of the returned R.

    Raises ValueError, before the device is touched, for a robust batch (R is rescaled per update), for recorded noise, for
    ``lanes=4`` (per-track noise has no quad kernel) and for an initial R outside the leading 2 x 2 block.
    """
    if hb.robust:
        raise ValueError("fit_measurement_noise: a robust batch rescales R at every update; the M-step is not defined for it")
    if hb.noise_pred is not None or hb.noise_upd is not None or hb.noise_rts is not None:
        raise ValueError("fit_measurement_noise: recorded noise is refused (the residuals are taken from z, the update saw z + noise)")
    if (default_lanes if hb.lanes is None else hb.lanes) == 4:
        raise ValueError("fit_measurement_noise: per-track noise runs the lane-per-track mapping only, lanes=4 is refused")
    if structure not in DeviceBatch._NOISE_STRUCTURES:
        raise ValueError(f"structure must be one of {sorted(DeviceBatch._NOISE_STRUCTURES)}, got {structure!r}")
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError(f"max_iter must be >= 1, got {max_iter!r}")
    gslot, labels = _noise_fit_groups(hb, groups)
    G, B = len(labels), hb.B
    hbt = with_track_noise(hb, R=track_matrices(hb)[1])
    R_start = hbt.R_tracks.copy()  # (10, B)
    if not r_tracks_block2(R_start):
        raise ValueError("fit_measurement_noise: the batch's R must be zero outside its leading 2 x 2 block (the structures "
                         "the fit knows are confined to it)")
    members = [np.flatnonzero(gslot == g).astype(np.int32) for g in range(G)]  # ascending slots: the order of every sum
    first = np.array([m[0] if len(m) else 0 for m in members])

    import torch

    db = DeviceBatch(hbt, device=device)
    active = np.array([len(m) > 0 for m in members])
    converged = np.zeros(G, dtype=bool)
    nobs = np.zeros(G, dtype=np.int64)
    R_iter = [R_start[:, first]]  # iterate i as (10, G)
    ll_tracks, ok_tracks = [], []

    def e_step():
        lk = db.log_likelihood()
        db.backward()
        ll_tracks.append(lk.loglik)
        ok_tracks.append(np.isfinite(lk.loglik) & ((lk.status & binding.STE_STATUS_NAN) == 0))

    for _ in range(max_iter):
        e_step()
        mom = db.measurement_moments()
        bad = ~np.logical_and.reduce(ok_tracks)
        if bad.any():  # a track some iterate could not score stays out of the moments too
            idx = torch.from_numpy(np.flatnonzero(bad)).to(db.device)
            mom["moments"][:, idx] = 0.0
            mom["count"][idx] = 0
        act = [members[g] if active[g] else members[g][:0] for g in range(G)]  # a stopped group has no members: its R stays
        offsets = np.concatenate([[0], np.cumsum([len(m) for m in act])]).astype(np.int32)
        res = db.update_measurement_noise(mom, groups=(offsets, np.concatenate(act)), structure=structure)
        Rg, ng, gs = (res[k].cpu().numpy() for k in ("R_group", "n_group", "group_status"))
        new = R_iter[-1].copy()
        for g in np.flatnonzero(active):
            if gs[g]:
                active[g] = False  # nothing to fit from, or no usable variance: the group keeps the R it has
                continue
            old, new[:, g], nobs[g] = new[:, g].copy(), Rg[:, g], ng[g]
            nz = Rg[:, g] != 0.0
            if np.max(np.abs(Rg[nz, g] - old[nz]) / np.abs(Rg[nz, g])) < rtol:
                active[g], converged[g] = False, True
        R_iter.append(new)
        if not active.any():
            break
    e_step()  # the last iterate's score

    keep = np.logical_and.reduce(ok_tracks)
    loglik = np.array([[_ordered_sum(ll[members[g]][keep[members[g]]]) for g in range(G)] for ll in ll_tracks])
    best = np.argmax(np.where(np.isfinite(loglik), loglik, -np.inf), axis=0)
    final = R_start.copy()
    for g in range(G):
        if best[g] > 0:
            final[:, members[g]] = R_iter[best[g]][:, g:g + 1]
    fitted = dataclasses.replace(hbt, R_tracks=final)
    db.hb = fitted
    db.t["R_tracks"].copy_(torch.from_numpy(final))
    db.noise.flags |= binding.STE_NOISE_R_BLOCK2  # every iterate is confined to the block, the start was checked
    db.run()
    full = np.zeros((4, 4), dtype=np.intp)
    full[_TRI] = np.arange(10)
    full = np.maximum(full, full.T)
    trace = np.stack(R_iter).transpose(0, 2, 1)[:, :, full]  # (iterations + 1, G, 4, 4)
    return NoiseFit(R=trace[best, np.arange(G)], R_trace=trace, groups=gslot, labels=labels, loglik=loglik, best_iter=best,
                    converged=converged, nobs=nobs, excluded=np.flatnonzero(~keep), host_batch=fitted, device_batch=db)


def fleet_windows(ntracks: int, chunk: int):
    """[lo, hi) ranges that cut ``ntracks`` into ceil(ntracks / chunk) windows of nearly equal size, each a whole number of
    64-track waves (but the last)."""
    n = max(1, -(-ntracks // max(int(chunk), 1)))
    w = -(-ntracks // (n * 64)) * 64
    return [(lo, min(lo + w, ntracks)) for lo in range(0, ntracks, w)]


# Window size of run_fleet when the caller names none: 256 waves of 64 tracks, a quarter of the chip's 1 024 SIMDs, so that
# whole windows make up a chip-full of forward waves.  Measured on a resident 100 000 x 500 fleet
# (profiles/r04_fleet_sweep.txt): 7 windows of 14 336 tracks 8.5 ms, 10 of 10 048 9.1 ms, 13 of 7 744 9.2 ms, one launch 9.5 ms.
FLEET_CHUNK = 16_384
# run_fleet's default: a resident fleet of at most this many windows runs its forward passes as one scheduled launch
SCHEDULED_FLEET_MAX_WINDOWS = 24


def run_fleet(fleet, chunk: int = FLEET_CHUNK, device="cuda:0", smooth: bool = True, outputs=None, pipeline=None,
              slices: Optional[int] = None, sm_pos: bool = False, scheduled: Optional[bool] = None):
    """
    UKF + URTSS over a fleet of any size -- the batch dimension of the reference's example loop
    (examples/example_ukf_rts_smoother_batch.py:19-90, one ship at a time) at the rate the pipelined kernels sustain.

    The fleet is cut into windows of at most ``chunk`` tracks, all nearly the same size (length-bucketed: ``pack_tracks`` lays tracks out longest
    first).  Windows are not copies: a window is the fleet's own tensors seen through a batch struct with
    ``track_stride`` = the fleet's width (include/ste.h), so every window's kernels read the fleet's inputs and write the
    fleet's histories in place.  The windows go through a ``SmootherPipeline``: the forward passes of several windows share
    the chip with the smoothers of the windows before them.

    ``fleet``: a ``HostBatch`` -- window k + 1 is uploaded (page-locked staging, a copy stream) while window k filters,
        and each window's histories come down as soon as its smoother has finished, overlapped with the windows behind it
        -- or a ``DeviceBatch`` that is already resident: nothing moves, the results stay in its tensors.
    ``outputs``: histories to bring back as NumPy arrays (any of "means", "covs", "means_smoothed", "covs_smoothed");
        default for a HostBatch: all that were computed, for a DeviceBatch: none.  "status" and "nsteps" always come along,
        and ``"device_batch"`` is the resident fleet.
    ``pipeline``: a ``SmootherPipeline`` to reuse (otherwise one is built for this call and closed at its end).
    ``scheduled``: a resident fleet's windows go through ``SmootherPipeline.submit_sequence`` -- all their forward passes as
        one launch of resident waves over (tile, time slice) items -- instead of one forward launch per window (same bits;
        measured on a 100 000-track fleet: 7.9-8.1 against 8.4-8.6 ms).  Default (None): yes for a
        resident fleet of up to ``SCHEDULED_FLEET_MAX_WINDOWS`` windows on a lane-per-track pipeline -- a job that is mostly
        fill and drain --, no for longer ones (a long stream of windows re-balances by itself) and for a ``HostBatch``
        (its windows arrive one upload at a time); never for a fleet with per-track noise (``Q_tracks`` / ``R_tracks``:
        the scheduled launches have none, and an explicit True raises ValueError for it).
    Results are those of ``run_batch`` on the same tracks with the lane-per-track mapping, bit for bit.
    """
    import torch

    if isinstance(fleet, DeviceBatch):
        db, hb, resident = fleet, fleet.hb, True
        if smooth and db.sm_mean is None:
            raise ValueError("this DeviceBatch was built without smoothed outputs (alloc_smoothed=False)")
        outputs = () if outputs is None else tuple(outputs)
        if len(fleet_windows(db.ntracks, chunk)) == 1:  # one window: one launch, the mapping the library picks for its size
            db.run() if smooth else db.forward()
            out = db.download(outputs) if outputs else {}
            out["status"], out["nsteps"], out["device_batch"] = db.status_host(), hb.nsteps.copy(), db
            return out
    else:
        hb, resident = fleet, False
        if len(fleet_windows(hb.B, chunk)) == 1:
            out, db = _run_batch(hb, device, smooth, True, outputs, sm_pos)
            out["device_batch"] = db
            return out
        if smooth and hb.sog_rate_rts is not None and np.isnan(
                hb.sog_rate_rts[:, (hb.host_status == 0) if hb.host_status is not None else slice(None)]).any():
            raise IndexError("smoother rate expansion too short for at least one track (unscented.py:287-292,310)")
        if outputs is None:
            outputs = ("means", "covs") + (("means_smoothed", "covs_smoothed") if smooth else ())
        outputs = tuple(outputs)
        db = DeviceBatch(hb, device=device, alloc_smoothed=smooth, sm_pos=sm_pos, upload=False)
    dev = db.device
    B = db.ntracks
    wins = fleet_windows(B, chunk)
    own_pipe = pipeline is None
    if db.noise is not None:  # per-track noise: per-window launches (the scheduled launches have no per-track form)
        if scheduled:
            raise ValueError("run_fleet(scheduled=True): scheduled launches have no per-track noise (Q_tracks / R_tracks)")
        scheduled = False
    if scheduled is None:
        scheduled = (resident and 1 < len(wins) <= SCHEDULED_FLEET_MAX_WINDOWS and (pipeline is None or pipeline.forward_lanes != 4))
    # (a pipeline built for scheduled launches needs two forward streams, not seven: every stream is a hardware queue, the device has
    #  about two dozen for everything that runs on it, and scheduled launches are the first to suffer when they run out --
    #  DESIGN.md section 5)
    pipe = pipeline or SmootherPipeline(dev, ntracks=wins[0][1] - wins[0][0], slices=slices,
                                        sequence_only=bool(scheduled and resident and len(wins) > 1))
    inv = None
    if hb.order is not None:  # back to the caller's track order
        inv = np.empty_like(hb.order)
        inv[hb.order] = np.arange(len(hb.order))
    # a window's histories come down while the next windows filter -- when tracks stay in place; a length-bucketed fleet
    # is reordered on the device in one pass at the end (DeviceBatch.download)
    stream_down = bool(outputs) and inv is None and len(wins) > 1
    host = {}
    try:
        up = torch.cuda.Stream(dev) if not resident else None
        down = torch.cuda.Stream(dev) if stream_down else None
        if stream_down:
            for name in outputs:
                attr, width = DeviceBatch._OUT[name]
                host[name] = torch.empty((B, hb.Nmax + 1, width), dtype=torch.float64, pin_memory=True)
        keep = []

        def collect(win, lo, hi, done):
            """A submitted window: its histories come down behind ``done``; it stays alive until the pipeline has drained."""
            if stream_down:
                down.wait_event(done)
                with torch.cuda.stream(down):
                    keep.append(win._download_into(outputs, host, lo, hi))
            keep.append(win)

        if scheduled and resident and len(wins) > 1:
            ws = [db.window(lo, hi) for lo, hi in wins]
            dones = pipe.submit_sequence(ws, smooth=smooth)
            for (lo, hi), win, done in zip(wins, ws, dones):
                collect(win, lo, hi, done)
            wins_left = []
        else:
            wins_left = wins
        for i, (lo, hi) in enumerate(wins_left):
            win = db.window(lo, hi) if len(wins) > 1 else db
            if not resident:
                win._uploaded = db.upload_tracks(lo, hi, up)
            collect(win, lo, hi, pipe.submit(win, final=(i == len(wins) - 1), smooth=smooth))
        pipe.synchronize()
        if down is not None:
            down.synchronize()
        db._pipeline_done = None
    finally:
        if own_pipe:
            pipe.close()
    out = {}
    if stream_down:
        for name in outputs:
            a = host[name].numpy()
            out[name] = a.reshape(a.shape[0], a.shape[1], 4, 4) if DeviceBatch._OUT[name][1] == 16 else a
    elif outputs:
        out = db.download(outputs, None if inv is None else torch.from_numpy(inv).to(dev))
    status = db.status.cpu().numpy()
    if hb.host_status is not None:
        status = status | hb.host_status
    nsteps = hb.nsteps.copy()
    out["status"], out["nsteps"] = (status, nsteps) if inv is None else (status[inv], nsteps[inv])
    out["device_batch"] = db
    return out
