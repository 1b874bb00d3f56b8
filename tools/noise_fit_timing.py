#!/usr/bin/env python3
"""The two kernels of the noise fit (ste_ukf_noise_moments_f64, ste_ukf_noise_mstep_f64) beside the E-step they follow, at the
bench batch: 10 000 tracks x 500 steps, per-track R, packed covariances, rts_work.  HIP events after a warm-up, the figures
alternating in one process, median of --rounds timed calls each:

  e_step          ste_ukf_forward_noise_f64 with the likelihood and histories, then ste_urtss_backward_noise_f64
  moments         ste_ukf_noise_moments_f64
  mstep_null      ste_ukf_noise_mstep_f64, every track a group of its own (NULL groups: a lane per track)
  mstep_16        ... 16 groups of tracks b % 16 (a wave per group)
  mstep_per_track ... one CSR group per track (a wave per track)

and the wall time of a whole fit_measurement_noise of 10 iterations, 16 groups (host clock, the call ends synchronised).  The
M-steps write a scratch copy of R, so every E-step filters with the same noise.  One JSON line per figure, appended to --out.
Figures are recorded, not asserted.

usage: tools/noise_fit_timing.py [--tracks 10000] [--rounds 9] [--out profiles/noise_fit_timing.jsonl]
"""
import argparse
import ctypes as C
import os
import time

import metrics_timing_common as mtc
import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=9, help="timed calls per figure (median), at least 7")
    ap.add_argument("--out", default=os.path.join(mtc.ROOT, "profiles", "noise_fit_timing.jsonl"))
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")

    import torch
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(args.tracks, nobs=mtc.NOBS, gap_h=1.0, seed0=0)
    hb = batch.pack_uniform(sb, mtc.SUBSTEPS, H, Q, R, P0)
    B = hb.B
    db = batch.DeviceBatch(batch.with_track_noise(hb, R=np.broadcast_to(R, (B, 4, 4))))
    lib, s, dev = db.lib, db._stream(None), dict(device=db.device)
    ll = torch.empty(B, dtype=torch.float64, **dev)
    lk = binding.SteUkfLoglikF64(ll.data_ptr(), None, None, None)
    fwd = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
    fwd.flags |= binding.STE_FLAG_LANES_1

    def e_step():
        binding.check(lib.ste_ukf_forward_noise_f64(C.byref(fwd), C.byref(db.noise), C.byref(lk), s), "ste_ukf_forward_noise_f64")
        binding.check(lib.ste_urtss_backward_noise_f64(C.byref(db.struct), C.byref(db.noise), s), "ste_urtss_backward_noise_f64")

    e_step()
    mom = db.measurement_moments()
    scratch = db.t["R_tracks"].clone()
    nm = binding.SteNoiseMomentsF64(mom["moments"].data_ptr(), mom["count"].data_ptr(), mom["vsum"].data_ptr(),
                                    mom["track_status"].data_ptr(), 0, 0)

    def moments():
        binding.check(lib.ste_ukf_noise_moments_f64(C.byref(db.struct), C.byref(nm), s), "ste_ukf_noise_moments_f64")

    def mstep(groups):
        if groups is None:
            G, nmem, off, mem = B, 0, None, None
        else:
            order = np.argsort(groups, kind="stable").astype(np.int32)
            offsets = np.concatenate([[0], np.cumsum(np.bincount(groups))]).astype(np.int32)
            off, mem = torch.from_numpy(offsets).to(db.device), torch.from_numpy(order).to(db.device)
            G, nmem = len(offsets) - 1, B
        Rg = torch.empty((10, G), dtype=torch.float64, **dev)
        ng, gs = torch.empty(G, dtype=torch.int32, **dev), torch.empty(G, dtype=torch.int32, **dev)
        ms = binding.SteNoiseMstepF64(B, G, nmem, binding.STE_NOISE_FIT_SCALAR, 0, mom["moments"].data_ptr(), mom["count"].data_ptr(),
                                      None if off is None else off.data_ptr(), None if mem is None else mem.data_ptr(),
                                      Rg.data_ptr(), ng.data_ptr(), gs.data_ptr(), scratch.data_ptr(), 0)
        keep = (off, mem, Rg, ng, gs)
        return lambda: (keep, binding.check(lib.ste_ukf_noise_mstep_f64(C.byref(ms), s), "ste_ukf_noise_mstep_f64"))

    figures = {"e_step": e_step, "moments": moments, "mstep_null": mstep(None), "mstep_16": mstep(np.arange(B) % 16),
               "mstep_per_track": mstep(np.arange(B))}
    for fn in figures.values():  # warm-up of every call
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = {name: [] for name in figures}
    for _ in range(args.rounds):  # alternating: drifts of clock and temperature hit every figure alike
        for name, fn in figures.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1))
    base = float(np.median(samples["e_step"]))
    for name, v in samples.items():
        med = float(np.median(v))
        mtc.append_json(args.out, {"figure": name, "tracks": B, "steps": hb.Nmax, "rounds": args.rounds, "ms": round(med, 4),
                                   "of_e_step": round(med / base, 4), "spread": round((max(v) - min(v)) / med, 4),
                                   "samples": [round(x, 3) for x in v],
                                   "what": "HIP events on the current stream, figures alternating, median after one warm-up; "
                                           "spread = (max - min) / median"})

    def fit():
        return batch.fit_measurement_noise(hb, groups=np.arange(B) % 16, max_iter=10, rtol=0.0)

    fit()  # warm-up
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        f = fit()
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    mtc.append_json(args.out, {"figure": "fit_10_iterations_16_groups", "tracks": B, "steps": hb.Nmax, "ms": round(float(np.median(walls)), 2),
                               "samples": [round(x, 2) for x in walls], "iterations": int(f.loglik.shape[0] - 1),
                               "r": [float(x) for x in f.R[:, 0, 0]], "fleet_loglik": [round(float(x), 2) for x in f.loglik.sum(axis=1)],
                               "what": "host clock around fit_measurement_noise (upload, 11 E-steps, 10 M-steps, the final run(), "
                                       "the host's group sums), synchronised; median of 3 after one warm-up"})


if __name__ == "__main__":
    main()
