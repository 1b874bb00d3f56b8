#!/usr/bin/env python3
"""Simplification (ste_track_simplify_f64) at the bench batch against the distance of path_metrics (sphere) on the same states in
the same process -- that call reads the same rows once -- timed with HIP events after a warm-up; each figure is the median of
--rounds timed calls.  S = 1 is the smoothed track (sm_mean), S > 1 posterior tracks that the sampler left on the device:

  path_ms          DeviceBatch.path_metrics, distance only: the yardstick
  simplify_ms      ste_track_simplify_f64 on outputs allocated once, keyed mode:tolerance_km:case with mode clock / shape and
                     flags     keep, nkeep, worst_sq and status
                     compact   those and rows, out_states, out_dt with cap = Nmax + 1
  kept_fraction    kept rows over rows, keyed mode:tolerance_km
  ratio            simplify_ms / path_ms

and, once per run, the wall time of batch.simplified_tracks (1 km, clock) beside db.download(("means_smoothed",)) of the same
batch, the way to get the same track without this call, with the bytes each moves to the host.

One JSON line per sample count S, appended to --out (default profiles/simplify_timing.jsonl).  Nothing gates on these.

usage: tools/simplify_timing.py [--tracks 10000] [--rounds 7] [--samples 1 16] [--out FILE]
"""
import argparse
import ctypes as C
import os
import time

import numpy as np

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package

TOLERANCES_KM = (0.1, 1.0, 10.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, N = db.lib, hb.B, hb.Nmax
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)

    def wall(fn, rounds=3):
        fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            best.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(best)), res

    down_ms, down = wall(lambda: db.download(("means_smoothed",)))
    simp_ms, ships = wall(lambda: batch.simplified_tracks(db, 1.0))
    kept = sum(len(t["rows"]) for t in ships)
    front = {"download_ms": round(down_ms, 3), "download_bytes": int(down["means_smoothed"].nbytes),
             "simplified_tracks_ms": round(simp_ms, 3), "simplified_tracks_bytes": kept * 40 + 24 * B, "simplified_tracks_rows": kept}
    del down, ships

    for S in args.samples:
        if S == 1:
            tracks, status = db.sm_mean.unsqueeze(0), None
        else:
            tracks, sm, status, keep_alive, _ = posterior_draws(db, S)
        scale = db.track_lon_scale(tracks).contiguous()
        res = {"keep": torch.zeros((S, N + 1, B), dtype=torch.uint8, device=db.device), "nkeep": torch.empty((S, B), **i32),
               "worst_sq": torch.empty((S, B), **f64), "status": torch.empty((S, B), **i32)}
        comp = {"rows": torch.empty((S, N + 1, B), **i32), "out_states": torch.empty((S, N + 1, 4, B), **f64),
                "out_dt": torch.empty((S, N, B), **f64)}
        out = {"tracks": B, "rows": N + 1, "nsamples": S, "rounds": args.rounds, "simplify_ms": {}, "simplify_samples": {},
               "kept_fraction": {}, "worst_km_max": {}, "ratio": {}}
        out["path_ms"], out["path_samples"] = timed(lambda: db.path_metrics(tracks, model="sphere"), args.rounds)
        total_rows = float(S) * float((hb.nsteps.astype(np.int64) + 1).sum())
        for mode, flag in (("clock", 0), ("shape", binding.STE_SIMPLIFY_SHAPE)):
            for tol_km in TOLERANCES_KM:
                for case in ("flags", "compact"):
                    sf = binding.SteSimplifyF64()
                    sf.nstates, sf.flags, sf.states = S, flag, tracks.data_ptr()
                    sf.tolerance_all, sf.lon_scale = tol_km / batch.KM_PER_DEG, scale.data_ptr()
                    for k, ten in res.items():
                        setattr(sf, k, ten.data_ptr())
                    if case == "compact":
                        sf.cap = N + 1
                        for k, ten in comp.items():
                            setattr(sf, k, ten.data_ptr())

                    def simplify():
                        binding.check(lib.ste_track_simplify_f64(C.byref(db.struct), C.byref(sf), s), "ste_track_simplify_f64")

                    key = f"{mode}:{tol_km:g}:{case}"
                    out["simplify_ms"][key], out["simplify_samples"][key] = timed(simplify, args.rounds)
                    out["ratio"][key] = round(out["simplify_ms"][key] / out["path_ms"], 3)
                out["kept_fraction"][f"{mode}:{tol_km:g}"] = round(float(res["nkeep"].sum().item()) / total_rows, 5)
                out["worst_km_max"][f"{mode}:{tol_km:g}"] = float(torch.sqrt(res["worst_sq"].max()).item() * batch.KM_PER_DEG)
        out["status_any"] = int(res["status"].cpu().numpy().any())
        out["sampler_status_any"] = 0 if status is None else int(status.cpu().numpy().any())
        out.update(front)
        out["what"] = ("HIP events on the current stream, median of rounds after one warm-up; path_ms through DeviceBatch.path_metrics, "
                       "simplify_ms through the C ABI on outputs allocated once with lon_scale per track (track_lon_scale); "
                       "download_ms and simplified_tracks_ms are wall times, synchronised, median of 3 after a warm-up")
        append_json(args.out, out)
        del tracks, res, comp


if __name__ == "__main__":
    main()
