#!/usr/bin/env python3
"""Per-track noise (ste_ukf_forward_noise_f64 / ste_urtss_backward_noise_f64) against the shared calls at the bench batch:
10 000 tracks x 500 steps, lane per track, packed covariances, rts_work.  Every track is given the SAME Q and R through
stacks, so that the per-track and the shared call do identical arithmetic (and must write identical bits: checked once,
before anything is timed).  HIP events after a warm-up, the two versions alternating in one process, median of --rounds
timed calls each:

  forward_gains     ste_ukf_forward_f64 (STE_FLAG_LANES_1, rts_work)        | ste_ukf_forward_noise_f64, l = NULL
  smoother_1kernel  ste_urtss_backward_f64 (tuning 0x400: one kernel)       | ste_urtss_backward_noise_f64
  loglik_only       ste_ukf_forward_loglik_f64 without histories            | ste_ukf_forward_noise_f64, l given, no histories

One JSON line per figure (shared time, per-track time, their ratio, the spread of each), appended to --out.

usage: tools/ukf_track_noise_timing.py [--tracks 10000] [--rounds 9] [--out profiles/ukf_track_noise_timing.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ship-track-estimators_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

NOBS, SUBSTEPS = 126, 4  # bench.py: 125 gaps of 4 filter steps = 500 steps per track


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=9, help="timed calls per version and figure (median), at least 7")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ukf_track_noise_timing.jsonl"))
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")

    import torch
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(args.tracks, nobs=NOBS, gap_h=1.0, seed0=0)
    hb = batch.pack_uniform(sb, SUBSTEPS, H, Q, R, P0)
    hb.lanes = 1
    B = hb.B
    hbt = batch.with_track_noise(hb, Q=np.broadcast_to(Q, (B, 4, 4)), R=np.broadcast_to(R, (B, 4, 4)))
    shared = batch.DeviceBatch(hb, tuning=0x400)
    track = batch.DeviceBatch(hbt, tuning=0x400)
    assert track.noise is not None and track.noise.flags == binding.STE_NOISE_R_BLOCK2 and shared.rts_work is not None
    lib = shared.lib
    s = shared._stream(None)
    dev = dict(device=shared.device)

    def lik_struct(db):
        ll = torch.empty(B, dtype=torch.float64, **dev)
        dof = torch.empty(B, dtype=torch.int32, **dev)
        nupd = torch.empty(B, dtype=torch.int32, **dev)
        only = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
        only.fwd_mean = only.fwd_cov = only.rts_work = None
        return only, binding.SteUkfLoglikF64(ll.data_ptr(), dof.data_ptr(), nupd.data_ptr(), None), (ll, dof, nupd)

    s_only, s_lk, s_out = lik_struct(shared)
    t_only, t_lk, t_out = lik_struct(track)

    def check(rc, what):
        binding.check(rc, what)

    figures = {
        "forward_gains": (lambda: check(lib.ste_ukf_forward_f64(C.byref(shared.struct), s), "ste_ukf_forward_f64"),
                          lambda: check(lib.ste_ukf_forward_noise_f64(C.byref(track.struct), C.byref(track.noise), None, s),
                                        "ste_ukf_forward_noise_f64")),
        "smoother_1kernel": (lambda: check(lib.ste_urtss_backward_f64(C.byref(shared.struct), s), "ste_urtss_backward_f64"),
                             lambda: check(lib.ste_urtss_backward_noise_f64(C.byref(track.struct), C.byref(track.noise), s),
                                           "ste_urtss_backward_noise_f64")),
        "loglik_only": (lambda: check(lib.ste_ukf_forward_loglik_f64(C.byref(s_only), C.byref(s_lk), s), "ste_ukf_forward_loglik_f64"),
                        lambda: check(lib.ste_ukf_forward_noise_f64(C.byref(t_only), C.byref(track.noise), C.byref(t_lk), s),
                                      "ste_ukf_forward_noise_f64")),
    }

    # warm-up of every call, and the check that the two versions write the same bits
    for fa, fb in figures.values():
        fa()
        fb()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(getattr(shared, n).view(torch.int64), getattr(track, n).view(torch.int64)))
               for n in ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "rts_work"))
    same = same and bool(torch.equal(shared.status, track.status)) and bool(torch.equal(s_out[0].view(torch.int64), t_out[0].view(torch.int64)))
    if not same:
        sys.exit("the per-track and the shared call disagree on identical matrices: nothing timed")

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once(fn):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for name, (fa, fb) in figures.items():
            a, b = [], []
            for _ in range(args.rounds):  # alternating: drifts of clock and temperature hit both alike
                a.append(once(fa))
                b.append(once(fb))
            ma, mb = float(np.median(a)), float(np.median(b))
            row = {"figure": name, "tracks": B, "steps": hb.Nmax, "rounds": args.rounds, "shared_ms": round(ma, 4),
                   "per_track_ms": round(mb, 4), "ratio": round(mb / ma, 4),
                   "shared_spread": round((max(a) - min(a)) / ma, 4), "per_track_spread": round((max(b) - min(b)) / mb, 4),
                   "shared_samples": [round(v, 3) for v in a], "per_track_samples": [round(v, 3) for v in b],
                   "bits_equal": True,
                   "what": "HIP events on the current stream, alternating calls, median after one warm-up; every track carries "
                           "the same Q and R; spread = (max - min) / median"}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
