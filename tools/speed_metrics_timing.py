#!/usr/bin/env python3
"""Speeds (ste_speed_metrics_f64) at the bench batch against the distance of path_metrics on the same tracks in the same run,
timed with HIP events after a warm-up; each figure is the median of --rounds timed calls on S posterior tracks per ship that
the sampler left on the device, for the sphere and WGS84:

  path_ms          DeviceBatch.path_metrics, distance only: the yardstick (the same leg, one column less to read)
  speed_ms         ste_speed_metrics_f64 on outputs allocated once, three cases:
                     all8    every output, 8 bands       (edges at the quantiles of the smoothed tracks' speeds: every step lands
                     all32   every output, 32 bands       in a band; one threshold per track, the fleet's median speed)
                     vmax    vmax alone: the kernel without band and run state, and without the per-step store
  ratio            speed_ms / path_ms per case

One JSON line per sample count S, appended to --out (default profiles/speed_metrics_timing.jsonl).  Nothing gates on these.

usage: tools/speed_metrics_timing.py [--tracks 10000] [--rounds 7] [--samples 16] [--out FILE]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package

OUTPUTS = ("speed", "dist", "sound_time", "vmax", "vmax_time", "band_time", "cond_time", "run_time", "first_run", "longest",
           "longest_start", "nruns", "nbroken", "track_status")
INT32 = ("nruns", "nbroken", "track_status")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speed_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, N = db.lib, hb.B, hb.Nmax
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    v = db.speed_metrics(db.sm_mean, per_step=True)["speed"].cpu().numpy()
    v = np.sort(v[np.isfinite(v)])
    edges = {nb: np.unique(np.quantile(v, np.linspace(0.0, 1.0, nb + 1))) for nb in (8, 32)}
    assert all(len(e) == nb + 1 for nb, e in edges.items())
    limit = torch.full((B,), float(np.median(v)), **f64)

    for S in args.samples:
        tracks, sm, status, keep, _ = posterior_draws(db, S)
        shape = {"speed": (S, N, B), "track_status": (B,)}
        res = {k: torch.empty(shape.get(k, (S, B)), **(i32 if k in INT32 else f64)) for k in OUTPUTS if k != "band_time"}
        bands = {nb: torch.empty((S, nb, B), **f64) for nb in edges}
        out = {"tracks": B, "rows": N + 1, "nsamples": S, "rounds": args.rounds, "threshold_kmh": float(limit[0].item()),
               "path_ms": {}, "path_samples": {}, "speed_ms": {}, "speed_samples": {}, "ratio": {}}
        for model, code in (("sphere", binding.STE_PREP_SPHERE), ("wgs84", binding.STE_PREP_WGS84)):
            ms, samples = timed(lambda: db.path_metrics(tracks, model=model), args.rounds)
            out["path_ms"][model], out["path_samples"][model] = ms, samples
            for case, nb in (("all8", 8), ("all32", 32), ("vmax", 0)):
                sp = binding.SteSpeedF64()
                sp.nstates, sp.model, sp.states, sp.flags = S, code, tracks.data_ptr(), 0
                sp.threshold_all, sp.min_run_h = float("nan"), 1.0
                if nb:
                    sp.nbands, sp.band_edges, sp.threshold = nb, edges[nb].ctypes.data, limit.data_ptr()
                    for k, ten in res.items():
                        setattr(sp, k, ten.data_ptr())
                    sp.band_time = bands[nb].data_ptr()
                else:
                    sp.vmax = res["vmax"].data_ptr()

                def speed():
                    binding.check(lib.ste_speed_metrics_f64(C.byref(db.struct), C.byref(sp), s), "ste_speed_metrics_f64")

                key = model + ":" + case
                out["speed_ms"][key], out["speed_samples"][key] = timed(speed, args.rounds)
                out["ratio"][key] = round(out["speed_ms"][key] / ms, 3)
        out["mean_vmax_kmh"] = float(res["vmax"].mean().item())
        out["band_hours"] = [round(x, 1) for x in bands[8].sum(dim=(0, 2)).cpu().numpy().tolist()]
        out["runs"] = int(res["nruns"].sum().item())
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = ("HIP events on the current stream, median of rounds after one warm-up; path_ms through DeviceBatch.path_metrics, "
                       "speed_ms through the C ABI on outputs allocated once, keyed by model:case")
        append_json(args.out, out)
        del tracks, sm, keep, res, bands


if __name__ == "__main__":
    main()
