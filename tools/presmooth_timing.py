#!/usr/bin/env python3
"""Observation preparation with SOG / COG smoothed on the device (ste_track_prep_smooth_f64) against the existing call
(ste_track_prep_f64) on the same tracks in the same run, timed with HIP events after a warm-up; each figure is the median of
--rounds timed calls through the C ABI on buffers allocated once.  The tracks are seeded random walks of --obs reports
(default: the bench batch's 10 000 x 126), sphere and WGS84:

  none      ste_track_prep_f64: one launch, 24 B in and 64 B out per observation (the yardstick)
  box5      box_filter(5) on both series: the reference CLI's "smooth": 5
  savgol    savgol_filter_table(20, 4) on SOG and (4, 2) on COG: the reference's Savitzky-Golay example
  ratio     the smoothed call over the existing one

One JSON line per case, appended to --out (default profiles/presmooth_timing.jsonl).  Nothing gates on these.

usage: tools/presmooth_timing.py [--tracks 10000] [--obs 126] [--rounds 9] [--label direct] [--out FILE]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import NOBS, ROOT, append_json, timed  # and the import path of the package


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--obs", type=int, default=NOBS)
    ap.add_argument("--rounds", type=int, default=9, help="timed calls per figure (median)")
    ap.add_argument("--label", default="direct", help="the build: 'direct' reads the w rows of a window from global memory")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "presmooth_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    lib = binding.require_gpu()
    dev = torch.device("cuda:0")
    B, T = args.tracks, args.obs
    rng = np.random.default_rng(0)
    lon = rng.uniform(-170, 170, B) + np.cumsum(rng.normal(0, 0.1, (T, B)), axis=0)
    lat = rng.uniform(-60, 60, B) + np.cumsum(rng.normal(0, 0.07, (T, B)), axis=0)
    gap = rng.choice([0.5, 1.0, 2.0], (T - 1, B))
    t_lon, t_lat, t_gap = (torch.from_numpy(a).to(dev) for a in (lon, lat, gap))
    outs = torch.empty((4, T, B), dtype=torch.float64, device=dev)
    z = torch.empty((T, 4, B), dtype=torch.float64, device=dev)
    raw = torch.empty((2, T, B), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    keep = []
    cases = {"none": None,
             "box5": (batch.box_filter(5), batch.box_filter(5)),
             "savgol": (batch.savgol_filter_table(20, 4), batch.savgol_filter_table(4, 2))}

    for model, code in (("sphere", binding.STE_PREP_SPHERE), ("wgs84", binding.STE_PREP_WGS84)):
        s = binding.StePrepBatchF64()
        s.B, s.Tmax, s.model = B, T, code
        s.lon, s.lat, s.gap = t_lon.data_ptr(), t_lat.data_ptr(), t_gap.data_ptr()
        s.sog, s.cog, s.sog_rate, s.cog_rate = (outs[i].data_ptr() for i in range(4))
        s.z = z.data_ptr()
        yard = None
        for name, firs in cases.items():
            if firs is None:
                def call():
                    binding.check(lib.ste_track_prep_f64(C.byref(s), stream), "ste_track_prep_f64")
            else:
                fs, fc = (batch._fir_struct(f, False, dev, keep) for f in firs)

                def call():
                    binding.check(lib.ste_track_prep_smooth_f64(C.byref(s), C.byref(fs), C.byref(fc), raw[0].data_ptr(),
                                                                raw[1].data_ptr(), stream), "ste_track_prep_smooth_f64")
            ms, samples = timed(call, args.rounds)
            yard = ms if firs is None else yard
            append_json(args.out, {
                "label": args.label, "case": name, "model": model, "tracks": B, "obs": T, "rounds": args.rounds,
                "windows": None if firs is None else [firs[0].window, firs[1].window], "ms": round(ms, 4), "samples": samples,
                "ratio_to_none": round(ms / yard, 3), "finite": bool(torch.isfinite(outs).all().item()),
                "what": "HIP events on the current stream, median of rounds after one warm-up, through the C ABI on buffers "
                        "allocated once; none = ste_track_prep_f64, the others ste_track_prep_smooth_f64 (its three launches)"})


if __name__ == "__main__":
    main()
