#!/usr/bin/env python3
"""Innovation log-likelihood of the UKF forward pass (ste_ukf_forward_loglik_f64) at the bench batch, timed with HIP events
after a warm-up; each figure is the median of --rounds timed calls.  Calls on one resident batch (lane per track):

  forward         ste_ukf_forward_f64 with STE_FLAG_LANES_1, no rts_work (histories written)
  loglik_hist     the likelihood call with histories (same histories, plus loglik / dof / nupd)
  loglik_only     the likelihood call without histories
  grid            --candidates likelihood-only calls, one per (Q, R) candidate (R's lon / lat variance on a log grid), as
                  batch.log_likelihood_grid issues them: round-robin over batch.GRID_STREAMS streams
  grid_serial     the same calls back to back on one stream

The grid's best_noise over the fleet is reported too, for the bench's Q (synthetic.example_matrices()).  One JSON line.

usage: tools/ukf_loglik_timing.py [--tracks 10000] [--rounds 7] [--candidates 16]
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
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--candidates", type=int, default=16)
    args = ap.parse_args()

    import torch
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(args.tracks, nobs=NOBS, gap_h=1.0, seed0=0)
    hb = batch.pack_uniform(sb, SUBSTEPS, H, Q, R, P0)
    hb.lanes = 1
    db = batch.DeviceBatch(hb, alloc_smoothed=False)
    lib, B = db.lib, hb.B
    dev = dict(device=db.device)
    ll = torch.empty(B, dtype=torch.float64, **dev)
    dof = torch.empty(B, dtype=torch.int32, **dev)
    nupd = torch.empty(B, dtype=torch.int32, **dev)
    lk = binding.SteUkfLoglikF64(ll.data_ptr(), dof.data_ptr(), nupd.data_ptr(), None)
    hist = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
    assert not hist.rts_work
    only = binding.SteUkfBatchF64.from_buffer_copy(hist)
    only.fwd_mean = only.fwd_cov = None
    s = db._stream(None)

    # 16 candidates by default: R's lon / lat variance from 1e-4 to 1 deg^2 (log-spaced), the bench's Q
    rs = np.logspace(-4, 0, args.candidates)
    cands = [(np.ascontiguousarray(Q), np.diag([r, r, 0.0, 0.0])) for r in rs]

    def forward():
        binding.check(lib.ste_ukf_forward_f64(C.byref(hist), s), "ste_ukf_forward_f64")

    def loglik_hist():
        binding.check(lib.ste_ukf_forward_loglik_f64(C.byref(hist), C.byref(lk), s), "ste_ukf_forward_loglik_f64")

    def loglik_only():
        binding.check(lib.ste_ukf_forward_loglik_f64(C.byref(only), C.byref(lk), s), "ste_ukf_forward_loglik_f64")

    gdb = batch.DeviceBatch(hb, alloc_smoothed=False, fuse_gains=False, histories=False)
    K = len(cands)
    gout = [torch.empty((K, B), dtype=t, **dev) for t in (torch.float64, torch.int32, torch.int32, torch.int32)]
    streams = [torch.cuda.Stream(db.device) for _ in range(min(K, batch.GRID_STREAMS))]
    one = [torch.cuda.Stream(db.device)]

    def grid():
        batch._launch_loglik_grid(gdb, cands, *gout, streams=streams)

    def grid_serial():
        batch._launch_loglik_grid(gdb, cands, *gout, streams=one)

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        samples = []
        for _ in range(args.rounds):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1))
        return float(np.median(samples)), [round(v, 3) for v in samples]

    out = {"tracks": B, "steps": hb.Nmax, "candidates": K, "grid_streams": len(streams), "rounds": args.rounds}
    for name, fn in (("forward", forward), ("loglik_hist", loglik_hist), ("loglik_only", loglik_only), ("grid", grid),
                     ("grid_serial", grid_serial)):
        ms, samples = timed(fn)
        out[name + "_ms"] = ms
        out[name + "_samples"] = samples
    # where the bench fleet's likelihood peaks under the bench's Q (the same grid, through the public API)
    g = batch.log_likelihood_grid(hb, cands)
    choice = batch.best_noise(g)
    shipped = batch.best_noise(batch.log_likelihood_grid(hb, [(Q, R)]))
    out.update({"grid_r": [float(v) for v in rs], "grid_fleet_loglik": [round(float(v), 3) for v in choice.loglik],
                "best_r": float(rs[choice.index]), "best_fleet_loglik": float(choice.loglik[choice.index]),
                "shipped_r": float(R[0, 0]), "shipped_fleet_loglik": float(shipped.loglik[0]),
                "excluded_tracks": choice.excluded,
                "what": "HIP events on the current stream, median of rounds after one warm-up; grid = all candidates"})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
