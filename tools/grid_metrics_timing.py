#!/usr/bin/env python3
"""Grid quantities (ste_grid_metrics_f64) at the bench batch, timed with HIP events after a warm-up; each figure is the median
of --rounds timed calls on S posterior tracks per ship that the sampler left on the device:

  grid_ms          keyed by case: ticks, outside, total and nbroken
                     global1   the periodic 1-degree grid of the globe, 360 x 180
                     quarter   a grid of 0.25-degree cells 180 degrees wide (720 columns) and 90 degrees high about the fleet's
                               median start
                     global5   the periodic 5-degree grid, 72 x 36 (2 592 cells: small enough for a copy in LDS)
                     onecell   one periodic cell that holds the globe: every flush of every lane goes to one address
                     clear     32 x 32 cells of 0.25 degrees on the far side of the globe: no track gets there
  grid_entries_ms  the same with `entries` too (a second atomic add per run)
  path_ms          ste_path_metrics_f64 (sphere, dist alone) for the same S in the same run, for scale
  adds_per_step    atomic adds to `ticks` per track-step, from the outputs alone: the sum of `entries` (one add per run in a
                   cell) over S x the sum of nsteps; runs off the grid cost no add (they go to the lane's own `outside`)
  outside_share    the share of the tracks' ticks spent off the grid

One JSON line per sample count S, appended to --out (default profiles/grid_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when two builds of the library are compared (STE_LIB_PATH picks one).

usage: tools/grid_metrics_timing.py [--tracks 10000] [--rounds 7] [--samples 1 4 16] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i64 = dict(dtype=torch.int64, device=db.device)
    steps = int(np.asarray(hb.nsteps, dtype=np.int64).sum())

    start = db.sm_mean[0, :2].cpu().numpy()  # (2, B)
    lon_c, lat_c = (float(np.floor(v)) for v in np.median(start, axis=1))
    far = lon_c + 180.0
    grids = {"global1": batch.track_grid(-180.0, -90.0, 1.0, 1.0, 360, 180),
             "quarter": batch.track_grid(lon_c - 90.0, max(lat_c - 45.0, -90.0), 0.25, 0.25, 720, 360),
             "global5": batch.track_grid(-180.0, -90.0, 5.0, 5.0, 72, 36),
             "onecell": batch.track_grid(-180.0, -90.0, 360.0, 180.0, 1, 1),
             "clear": batch.track_grid(far - 4.0, lat_c - 4.0, 0.25, 0.25, 32, 32)}

    for S in args.samples:
        draws, sm, status, keep, _ = posterior_draws(db, S)
        outside, total = torch.empty((S, B), **i64), torch.empty((S, B), **i64)
        nbrk = torch.empty((S, B), dtype=torch.int32, device=db.device)
        dist = torch.empty((S, B), **f64)

        out = {"label": args.label, "tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "track_steps": S * steps,
               "grid_ms": {}, "grid_entries_ms": {}, "grid_samples": {}, "adds_per_step": {}, "outside_share": {},
               "broken_steps": {}, "cells": {k: [g.nx, g.ny] for k, g in grids.items()}}
        for name, tg in grids.items():
            ticks, ent = torch.zeros((tg.ny, tg.nx), **i64), torch.zeros((tg.ny, tg.nx), **i64)
            g = binding.SteGridF64()
            g.nstates, g.flags, g.states = S, binding.STE_GRID_PERIODIC_LON if tg.periodic else 0, draws.data_ptr()
            g.nx, g.ny, g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref = tg.nx, tg.ny, tg.lon0, tg.lat0, tg.dlon, tg.dlat, tg.lon_ref
            g.ticks, g.outside, g.total, g.nbroken = ticks.data_ptr(), outside.data_ptr(), total.data_ptr(), nbrk.data_ptr()

            def call():
                binding.check(lib.ste_grid_metrics_f64(C.byref(db.struct), C.byref(g), s), "ste_grid_metrics_f64")

            out["grid_ms"][name], out["grid_samples"][name] = timed(call, args.rounds)
            g.entries = ent.data_ptr()
            out["grid_entries_ms"][name] = timed(call, args.rounds)[0]
            ticks.zero_()
            ent.zero_()
            call()
            torch.cuda.synchronize()
            nt, no, ntot = int(ticks.sum().item()), int(outside.sum().item()), int(total.sum().item())
            assert nt + no == ntot, (name, nt, no, ntot)  # the identity of the header, on the whole call
            out["adds_per_step"][name] = int(ent.sum().item()) / float(S * steps)
            out["outside_share"][name] = no / float(ntot)
            out["broken_steps"][name] = int(nbrk.sum().item())
            del ticks, ent
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, binding.STE_PREP_SPHERE, draws.data_ptr(), dist.data_ptr(), -1

        def path():
            binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

        out["path_ms"], out["path_samples"] = timed(path, args.rounds)
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; grid_ms keyed by case"
        append_json(args.out, out)
        del draws, sm, keep


if __name__ == "__main__":
    main()
