"""Recorder of tests/golden/forward_step_bits.npz, and the batch / digests tests/test_forward_step_bits.py shares with it.

The fixture pins the BITS the forward step writes -- the filtered and smoothed histories, the smoother's work rows and the
status words -- as one commit's build wrote them on the GPU, so that a change of the step's instruction stream (range
guards, loop shape, selects) can be shown to move none of them.  Run it on the GPU from the commit whose bits are to be kept:

    python tests/golden/make_forward_step_bits.py --commit <hash of that commit>

One batch of 130 tracks x 130 filter steps (two full waves and a wave of two lanes; 4 sub-steps, so update and predict-only
steps alternate; the eigenvector basis restarts at steps 64 and 128), synthetic.make_batch tracks plus crafted ones that
leave the validity range of the branch-free transcendentals, stay just inside it, or are non-finite from the start
(CRAFTED).  The first wave of the lane-per-track mapping (tracks 0-63) never takes the fallback fan, the other two do.

The arrays hold 130 x 131 x (4 + 10 + 4 + 10) + 130 x 3 901 doubles per lane mapping, 8 MB of incompressible bits against
the 1 MiB a committed file may have, so the file keeps 64-bit position-weighted digests of the bit patterns instead: one
per history row and one per track for every array (a mismatch names its row and its track), plus SHA-256 of each whole
array.  The per-track digest does not depend on the track's slot, so a batch without the crafted tracks can be compared
track by track.
"""
import argparse
import dataclasses
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "ship-track-estimators_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NTRACKS, NSTEPS, SUBSTEPS = 130, 130, 4
# slot -> what is wrong with the track.  Lane-per-track waves: 0-63, 64-127, 128-129.  The "just under" track sits in the
# first wave, which must never take the fallback; the "just over" track is the only crafted one of the third wave, so that
# wave takes the fallback because of that lane's verdict alone; the others share the second wave.
CRAFTED = {
    10: "heading variance puts a pair delta just under pi/4 at the first fan (in range: no fallback)",
    70: "starts at latitude 89.9999",
    90: "a step of tens of degrees (16 000 km/h)",
    91: "a step of tens of degrees (24 000 km/h)",
    100: "NaN in P0",
    110: "inf in x0",
    129: "heading variance puts a pair delta just over pi/4 at the first fan",
}
FALLBACK = (70, 90, 91, 129)  # finite tracks that leave the range of the branch-free transcendentals
ARRAYS = ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "rts_work")
SENTINEL = -7.0  # what the output buffers hold before the launch (some work rows are written for flagged tracks only)


def pair_delta_p33(rel):
    """P0[3][3] for which the first fan's heading column gives the pair delta T[3][3] pi / 180 = (pi/4) (1 + rel): the prior
    is diagonal, so T = sqrt(fan_scale P0) entry by entry (to an ulp or two -- rel is 1e-6, far outside that).  The heading
    column, not the speed column: a speed variance that brings T[2][2] dt / R to pi/4 (2e4 km/h) spreads the NEXT fan's
    positions over tens of degrees, so no such track stays in range; a heading variance of (26 deg)^2 moves nothing else.
    Q adds 1e-6 deg^2 per step, 2e-7 of it over the 130 steps, and an update only shrinks it: a track set 1e-6 under the
    limit stays under it for the whole pass ((sqrt A)_33^2 <= A_33 for a positive semi-definite A)."""
    from track_estimators import batch

    fan_scale = batch.sigma_constants(4)[0]
    t33 = 0.78539816339744828 * (1.0 + rel) / 0.017453292519943295
    return t33 * t33 / fan_scale


def build_batch():
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    nobs = -(-NSTEPS // SUBSTEPS) + 1  # 34 observations: 132 steps, cut to 130 below
    sb = synthetic.make_batch(NTRACKS, nobs=nobs, gap_h=1.0, seed0=4200)
    sb.z[70, 1, :] = 89.9999 - 1e-3 * np.arange(nobs)
    sb.z[90, 2, :] = 16000.0
    sb.z[91, 2, :] = 24000.0
    hb = batch.pack_uniform(sb, SUBSTEPS, H, Q, R, P0)
    cut = {}
    for name in ("dt", "sog_rate", "cog_rate", "sog_rate_rts", "cog_rate_rts", "upd_idx"):
        a = getattr(hb, name)
        cut[name] = None if a is None else np.ascontiguousarray(a[:NSTEPS])
    P0t = np.ascontiguousarray(np.repeat(hb.P0.reshape(16, 1), NTRACKS, axis=1))
    P0t[15, 10] = pair_delta_p33(-1e-6)
    P0t[15, 129] = pair_delta_p33(+1e-6)
    P0t[5, 100] = np.nan
    x0 = hb.x0.copy()
    x0[2, 110] = np.inf
    return dataclasses.replace(hb, Nmax=NSTEPS, nsteps=np.full(NTRACKS, NSTEPS, dtype=np.int32), P0=P0t, x0=x0, **cut)


def take_tracks(hb, idx):
    """The batch of the tracks `idx` alone (every per-track array has the track index last)."""
    idx = np.asarray(idx)
    new = {}
    for name in ("nsteps", "x0", "P0", "dt", "sog_rate", "cog_rate", "sog_rate_rts", "cog_rate_rts", "upd_idx", "z"):
        a = getattr(hb, name)
        new[name] = None if a is None else np.ascontiguousarray(a[..., idx])
    return dataclasses.replace(hb, B=len(idx), **new)


def run(hb, lanes):
    """Forward pass + smoother on cuda:0 with the given lane mapping; the raw device arrays as NumPy, [row][component][track]
    (rts_work: [row][track])."""
    from track_estimators import batch

    db = batch.DeviceBatch(dataclasses.replace(hb, lanes=lanes), device="cuda:0")
    for name in ARRAYS:
        getattr(db, name).fill_(SENTINEL)
    db.run()
    db.torch.cuda.synchronize()
    out = {name: getattr(db, name).cpu().numpy() for name in ARRAYS}
    out["status"] = db.status.cpu().numpy()
    return out


def digests(a):
    """(per row, per track, sha256) of the bit patterns of a [row][...][track] array of doubles."""
    bits = np.ascontiguousarray(a).view(np.uint64).reshape(a.shape[0], -1, a.shape[-1])
    nrow, ncomp, _ = bits.shape
    with np.errstate(over="ignore"):
        # odd multipliers that depend on (row, component): position-weighted sums modulo 2^64
        w = (np.arange(nrow, dtype=np.uint64)[:, None] * np.uint64(64) + np.arange(ncomp, dtype=np.uint64)[None, :]) * np.uint64(
            0x9E3779B97F4A7C15) | np.uint64(1)
        mixed = bits * w[:, :, None]
        mixed ^= mixed >> np.uint64(29)
        per_track = mixed.sum(axis=(0, 1), dtype=np.uint64)
        per_row = (mixed * (np.arange(bits.shape[-1], dtype=np.uint64) * np.uint64(2) + np.uint64(1))[None, None, :]).sum(
            axis=(1, 2), dtype=np.uint64)
    return per_row, per_track, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(commit):
    hb = build_batch()
    rec = {"commit": np.array(commit), "ntracks": np.int64(NTRACKS), "nsteps": np.int64(NSTEPS)}
    for lanes in (1, 4):
        out = run(hb, lanes)
        rec[f"l{lanes}_status"] = out["status"]
        for name in ARRAYS:
            per_row, per_track, sha = digests(out[name])
            rec[f"l{lanes}_{name}_rows"] = per_row
            rec[f"l{lanes}_{name}_tracks"] = per_track
            rec[f"l{lanes}_{name}_sha256"] = np.array(sha)
        print(f"lanes={lanes}: status bits seen {sorted(set(out['status'].tolist()))}, non-finite final means "
              f"{int((~np.isfinite(out['fwd_mean'][-1])).any(axis=0).sum())} tracks")
    path = os.path.join(HERE, "forward_step_bits.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
    return path


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is being recorded")
    ap.add_argument("--out", default=None, help="also copy the file here (a directory)")
    a = ap.parse_args()
    p = record(a.commit)
    if a.out:
        import shutil

        os.makedirs(a.out, exist_ok=True)
        shutil.copy(p, a.out)
