"""The batches, launch forms and digests that tests/test_step_loop_waits.py shares with the recorder of
tests/golden/step_loop_bits_parent.npz.

The fixture pins the BITS of the lane-per-track forward pass and of the one-kernel smoother -- filtered and smoothed
histories, the smoother's work rows with the first-bad word behind them, the status words -- as the commit BEFORE the
step loops' loads and stores were reordered wrote them on the GPU.  That reordering ("Store drain")
moves loads across the stores of the previous row and issues the x_b / P_b loads of a full work row a row ahead; what can
go wrong is a load that is issued for the wrong row, under the wrong predicate, or past a track's end.  The cases are the
smallest at which each of those shows:

  * 65 tracks: a full wave and a wave of one lane;
  * ragged lengths in the first wave, among them tracks of 0, 1, 2 and 3 steps and tracks that end exactly on and one
    past the 64-step restart of the eigenvector basis;
  * 65 steps, so that a pass in two time slices (0-64, 64-65) and the scheduled launch cross that restart;
  * an update on every step (every work row full), none after the initial one (no row full but row 0), one in four;
  * with and without the initial update (row 0 full or not);
  * recorded noise (every row full, rows 2-3 of D stored);
  * smoother rates of its own (the kShift instantiations);
  * per-track Q and R (the _tn instantiations);
  * priors that are indefinite (the square root is clamped at step 0: the first-bad word is 0 and the smoother takes columns
    2-3 of D from the work rows, the cold branch of its gain), NaN and infinite (non-finite bits travel through every
    operation of both loops: NaN payloads would show an operand order that changed).

The arrays of one case are ~2 MB of incompressible bits, so the file keeps 64-bit position-weighted digests of the bit
patterns -- one per row and one per track for every array, a mismatch names both -- plus SHA-256 of each whole array, the
status words and the first-bad words themselves.
"""
import dataclasses
import hashlib

import numpy as np

NTRACKS, NSTEPS = 65, 65
ARRAYS = ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "rts_work")
SENTINEL = -7.0  # what the output buffers hold before a launch: rows past a track's end and unused parts of a work row keep it
ONE_KERNEL, TWO_KERNEL, LANE_RECURRENCE = 0x400, 0x200, 0x800  # include/ste.h: STE_TUNING_*_SMOOTHER, STE_TUNING_LANE_RECURRENCE

CASES = ("quarter", "every", "none", "quarter_noinit", "none_noinit", "noise", "shift", "track_noise", "bad_prior")
BAD_PRIOR = {9: "indefinite", 20: "NaN in P0", 30: "inf in x0", 64: "indefinite"}  # slot -> what is wrong with the prior


def ragged_lengths():
    """Track lengths of the 65 slots: 0, 1, 2, 3 first, then the restart's neighbours, then a spread; the lone lane of the
    second wave runs the whole length."""
    n = (NSTEPS - (np.arange(NTRACKS) * 7) % 40).astype(np.int32)
    n[:8] = (0, 1, 2, 3, 63, 64, 65, 4)
    n[64] = NSTEPS
    return n


def build_case(name):
    """HostBatch of the case `name` (lanes=1)."""
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sub = 1 if name == "every" else 4
    nobs = -(-NSTEPS // sub) + 1
    sb = synthetic.make_batch(NTRACKS, nobs=nobs, gap_h=1.0, seed0=6100 + 13 * CASES.index(name))
    hb = batch.pack_uniform(sb, sub, H, Q, R, P0)
    cut = {}
    for field in ("dt", "sog_rate", "cog_rate", "sog_rate_rts", "cog_rate_rts", "upd_idx"):
        a = getattr(hb, field)
        cut[field] = None if a is None else np.ascontiguousarray(a[:NSTEPS])
    hb = dataclasses.replace(hb, Nmax=NSTEPS, nsteps=ragged_lengths(), lanes=1, **cut)
    if name in ("none", "none_noinit"):
        hb = dataclasses.replace(hb, upd_idx=np.full_like(hb.upd_idx, -1))
    if name.endswith("_noinit"):
        hb = dataclasses.replace(hb, initial_update=False)
    if name == "noise":
        rng = np.random.default_rng(61)
        hb = dataclasses.replace(hb, noise_pred=1e-3 * rng.standard_normal((NSTEPS, 4, NTRACKS)),
                                 noise_upd=1e-3 * rng.standard_normal((NSTEPS + 1, 4, NTRACKS)),
                                 noise_rts=1e-3 * rng.standard_normal((NSTEPS, 4, NTRACKS)))
    if name == "shift":
        hb = dataclasses.replace(hb, sog_rate_rts=hb.sog_rate * 1.25 + 0.01, cog_rate_rts=hb.cog_rate * 0.75 - 0.02)
    if name == "bad_prior":
        P0t = np.repeat(np.eye(4)[None], NTRACKS, 0)
        P0t[9] = P0t[64] = np.diag([1.0, -0.3, 1.0, 1.0])
        P0t[20, 1, 1] = np.nan
        x0 = hb.x0.copy()
        x0[2, 30] = np.inf
        hb = dataclasses.replace(hb, P0=np.ascontiguousarray(P0t.reshape(NTRACKS, 16).T), x0=x0)
    if name == "track_noise":
        scale = 1.0 + 0.01 * np.arange(NTRACKS)
        hb = batch.with_track_noise(hb, Q=Q[None] * scale[:, None, None], R=R[None] / scale[:, None, None])
    return hb


def device_batch(hb, tuning=ONE_KERNEL):
    from track_estimators import batch

    db = batch.DeviceBatch(hb, device="cuda:0", tuning=tuning)
    for name in ARRAYS:
        getattr(db, name).fill_(SENTINEL)
    return db


def outputs(db):
    """The raw device arrays as NumPy, [row][component][track] (rts_work: [row][track], the first-bad words last)."""
    db.torch.cuda.synchronize()
    out = {name: getattr(db, name).cpu().numpy() for name in ARRAYS}
    out["status"] = db.status.cpu().numpy()
    return out


def run_whole(hb, tuning=ONE_KERNEL):
    db = device_batch(hb, tuning)
    db.run()
    return outputs(db)


def run_sliced(hb, slices=2):
    db = device_batch(hb)
    db.forward(slices=slices)
    db.backward()
    return outputs(db)


def run_scheduled(hb, pipe):
    """Forward pass and smoother as the scheduled launches of a sequence of one batch (no per-track noise there)."""
    db = device_batch(hb)
    db.torch.cuda.synchronize()
    pipe.submit_sequence([db], tile_smoothers=True)
    pipe.synchronize()
    return outputs(db)


def digests(a):
    """(per row, per track, sha256) of the bit patterns of a [row][...][track] array of doubles."""
    bits = np.ascontiguousarray(a).view(np.uint64).reshape(a.shape[0], -1, a.shape[-1])
    nrow, ncomp, ntrack = bits.shape
    with np.errstate(over="ignore"):
        w = (np.arange(nrow, dtype=np.uint64)[:, None] * np.uint64(64) + np.arange(ncomp, dtype=np.uint64)[None, :]) * np.uint64(
            0x9E3779B97F4A7C15) | np.uint64(1)  # odd multipliers that depend on (row, component)
        mixed = bits * w[:, :, None]
        mixed ^= mixed >> np.uint64(29)
        per_track = mixed.sum(axis=(0, 1), dtype=np.uint64)
        per_row = (mixed * (np.arange(ntrack, dtype=np.uint64) * np.uint64(2) + np.uint64(1))[None, None, :]).sum(
            axis=(1, 2), dtype=np.uint64)
    return per_row, per_track, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record_case(name, out):
    """The fixture's entries of one case."""
    rec = {f"{name}_status": out["status"], f"{name}_first_bad": out["rts_work"][-1].copy()}
    for arr in ARRAYS:
        per_row, per_track, sha = digests(out[arr])
        rec[f"{name}_{arr}_rows"] = per_row
        rec[f"{name}_{arr}_tracks"] = per_track
        rec[f"{name}_{arr}_sha256"] = np.array(sha)
    return rec
