#!/usr/bin/env python3
"""Raster quantities (ste_raster_metrics_f64) at the bench batch, timed with HIP events after a warm-up; each figure is the
median of --rounds timed calls on S posterior tracks per ship that the sampler left on the device.  The grids are the five of
tools/grid_metrics_timing.py (global1 360 x 180 periodic, 0.5 MB of values; quarter 720 x 360, 2 MB; global5 72 x 36; onecell;
clear, which no track reaches) and a sixth, eighth (0.125-degree cells, 1440 x 720 about the fleet, 8 MB: more than an L2);
the values are integers in -8 .. 8 from default_rng(11) with a tenth of the cells NaN, the threshold is 3.

  raster_ms        keyed by grid: every per-track output (threshold outputs and row_value included)
  raster_hits_ms   the threshold outputs alone (hit_ticks, hit_first, nhit, nhit_long, hit_longest)
  raster_wsum_ms   wsum alone
  grid_ms          ste_grid_metrics_f64 (ticks, outside, total, nbroken) on the same grid in the same run: the scatter half
  path_ms          ste_path_metrics_f64 (sphere, dist alone) for the same S in the same run, for scale
  runs_per_step    runs on the grid per track-step = gathers per track-step, from the grid call's `entries`
  checksum         per grid, one integer over the bit patterns of every output of the full call: two builds that print the
                   same integers computed the same bits

One JSON line per sample count S, appended to --out (default profiles/raster_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when builds of the library are compared (STE_LIB_PATH picks one); a form of
the kernel is a build of csrc/ste_raster.hip with -DSTE_RASTER_EAGER=1 or -DSTE_RASTER_LDS_CELLS=256, linked with the other
objects of the library.

usage: tools/raster_metrics_timing.py [--tracks 10000] [--rounds 7] [--samples 1 4 16] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package

INT64 = ("total", "outside", "valid", "nodata", "tmin", "tmax", "hit_ticks", "hit_first", "hit_longest")
INT32 = ("nbroken", "nhit", "nhit_long")
FLOAT = ("wsum", "vmin", "vmax")
HIT = ("hit_ticks", "hit_first", "nhit", "nhit_long", "hit_longest")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i64 = dict(dtype=torch.int64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    steps = int(np.asarray(hb.nsteps, dtype=np.int64).sum())

    start = db.sm_mean[0, :2].cpu().numpy()  # (2, B)
    lon_c, lat_c = (float(np.floor(v)) for v in np.median(start, axis=1))
    far = lon_c + 180.0
    grids = {"global1": batch.track_grid(-180.0, -90.0, 1.0, 1.0, 360, 180),
             "quarter": batch.track_grid(lon_c - 90.0, max(lat_c - 45.0, -90.0), 0.25, 0.25, 720, 360),
             "global5": batch.track_grid(-180.0, -90.0, 5.0, 5.0, 72, 36),
             "onecell": batch.track_grid(-180.0, -90.0, 360.0, 180.0, 1, 1),
             "clear": batch.track_grid(far - 4.0, lat_c - 4.0, 0.25, 0.25, 32, 32),
             "eighth": batch.track_grid(lon_c - 90.0, max(lat_c - 45.0, -90.0), 0.125, 0.125, 1440, 720)}

    for S in args.samples:
        draws, sm, status, keep, _ = posterior_draws(db, S)
        new = lambda: {**{k: torch.empty((S, B), **i64) for k in INT64}, **{k: torch.empty((S, B), **i32) for k in INT32},  # noqa: E731
                       **{k: torch.empty((S, B), **f64) for k in FLOAT}, "row_value": torch.empty((S, rows, B), **f64)}
        outs = new()
        dist = torch.empty((S, B), **f64)

        out = {"label": args.label, "tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "track_steps": S * steps,
               "raster_ms": {}, "raster_hits_ms": {}, "raster_wsum_ms": {}, "grid_ms": {}, "raster_samples": {},
               "grid_samples": {}, "runs_per_step": {}, "share": {}, "cells": {k: [g.nx, g.ny] for k, g in grids.items()}}
        out["checksum"] = {}
        for name, tg in grids.items():
            rng = np.random.default_rng(11)
            v = rng.integers(-8, 9, (tg.ny, tg.nx)).astype(np.float64)
            v[rng.random((tg.ny, tg.nx)) < 0.1] = np.nan
            values = torch.from_numpy(v).to(db.device)
            flags = binding.STE_GRID_PERIODIC_LON if tg.periodic else 0

            def raster(which, into):
                r = binding.SteRasterF64()
                r.nstates, r.flags, r.states, r.nx, r.ny = S, flags, draws.data_ptr(), tg.nx, tg.ny
                r.lon0, r.lat0, r.dlon, r.dlat, r.lon_ref = tg.lon0, tg.lat0, tg.dlon, tg.dlat, tg.lon_ref
                r.values, r.threshold, r.min_ticks = values.data_ptr(), 3.0, 1 << 18
                if not set(which) & set(HIT):
                    r.flags |= binding.STE_RASTER_NO_THRESHOLD
                for k in which:
                    setattr(r, k, into[k].data_ptr())
                return r

            for key, which in (("raster_ms", tuple(outs)), ("raster_hits_ms", HIT), ("raster_wsum_ms", ("wsum",))):
                r = raster(which, outs)

                def call():
                    binding.check(lib.ste_raster_metrics_f64(C.byref(db.struct), C.byref(r), s), "ste_raster_metrics_f64")

                out[key][name], samples = timed(call, args.rounds)
                if key == "raster_ms":
                    out["raster_samples"][name] = samples
            for ten in outs.values():  # rows past nsteps are not written: the same bits there for every build
                ten.view(torch.int32).fill_(-7)
            r = raster(tuple(outs), outs)
            binding.check(lib.ste_raster_metrics_f64(C.byref(db.struct), C.byref(r), s), "ste_raster_metrics_f64")
            chk = 0
            for ten in outs.values():  # wrapping 64-bit arithmetic: position-weighted sum of the bit patterns
                flat = ten.reshape(-1)
                flat = flat.view(torch.int64) if flat.element_size() == 8 else flat.to(torch.int64)
                weight = torch.arange(flat.numel(), dtype=torch.int64, device=db.device) * 2654435761 + 1
                chk = (chk * 31 + int((flat * weight).sum().item())) % (1 << 63)
                del weight
            out["checksum"][name] = chk
            torch.cuda.synchronize()
            total = float(outs["total"].sum().item())
            out["share"][name] = {k: float(outs[k].sum().item()) / total for k in ("valid", "nodata", "outside")}

            ticks, ent = torch.zeros((tg.ny, tg.nx), **i64), torch.zeros((tg.ny, tg.nx), **i64)
            g = binding.SteGridF64()
            g.nstates, g.flags, g.states, g.nx, g.ny = S, flags, draws.data_ptr(), tg.nx, tg.ny
            g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref = tg.lon0, tg.lat0, tg.dlon, tg.dlat, tg.lon_ref
            gout, gtot = torch.empty((S, B), **i64), torch.empty((S, B), **i64)
            gbrk = torch.empty((S, B), **i32)
            g.ticks, g.outside, g.total, g.nbroken = ticks.data_ptr(), gout.data_ptr(), gtot.data_ptr(), gbrk.data_ptr()

            def grid():
                binding.check(lib.ste_grid_metrics_f64(C.byref(db.struct), C.byref(g), s), "ste_grid_metrics_f64")

            out["grid_ms"][name], out["grid_samples"][name] = timed(grid, args.rounds)
            g.entries = ent.data_ptr()
            ent.zero_()
            grid()
            torch.cuda.synchronize()
            assert torch.equal(gout, outs["outside"]) and torch.equal(gtot, outs["total"]), name  # the two walks agree
            out["runs_per_step"][name] = int(ent.sum().item()) / float(S * steps)
            del ticks, ent, values
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, binding.STE_PREP_SPHERE, draws.data_ptr(), dist.data_ptr(), -1

        def path():
            binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

        out["path_ms"], out["path_samples"] = timed(path, args.rounds)
        out["ratio_to_grid"] = {k: round(out["raster_ms"][k] / out["grid_ms"][k], 3) for k in grids}
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; keyed by grid"
        append_json(args.out, out)
        del draws, sm, keep, outs


if __name__ == "__main__":
    main()
