#!/usr/bin/env python3
"""Region quantities (ste_region_metrics_f64) at the bench batch, timed with HIP events after a warm-up; each figure is the
median of --rounds timed calls on S posterior tracks per ship that the sampler left on the device:

  region_ms       keyed "V<vertices>/<where>": time_inside, first_entry, nenter and nbroken against an ellipse of V vertices.
                  <where> = home: centred on the fleet's median start and sized to hold half of the starts; east60: the same
                  polygon 60 degrees east (the fleet's starts span 120 degrees of longitude, so part of it is still there);
                  clear: 180 degrees east, where no track gets, so that every step takes the bounding-box skip
  region_dist_ms  V = 64, home, with dist_inside too, keyed by model; region_mask_ms: V = 64, home, with the inside mask too
  path_ms         ste_path_metrics_f64 (sphere, dist alone) for the same S in the same run, for scale
  inside_share    the share of (sample, track) pairs with nenter > 0 at V = 64, per <where>

One JSON line per sample count S, appended to --out (default profiles/region_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when two builds of the library are compared (STE_LIB_PATH picks one).

usage: tools/region_metrics_timing.py [--tracks 10000] [--rounds 7] [--samples 1 4 16] [--vertices 8 64 512] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package

WHERE = {"home": 0.0, "east60": 60.0, "clear": 180.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--vertices", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)

    # an ellipse about the median start with the proportions of the starts' spread, scaled to hold half of the starts
    start = db.sm_mean[0, :2].cpu().numpy()  # (2, B)
    centre, spread = np.median(start, axis=1), np.maximum(start.std(axis=1), 1e-6)
    scale = np.median(np.hypot(*((start - centre[:, None]) / spread[:, None])))

    def polygon(V, east):
        th = 2.0 * np.pi * np.arange(V) / V
        ring = np.stack([centre[0] + east + scale * spread[0] * np.cos(th), centre[1] + scale * spread[1] * np.sin(th)], axis=1)
        poly = batch.region_polygon(ring)
        return poly, torch.from_numpy(poly.vert).to(db.device)

    for S in args.samples:
        draws, sm, status, keep, _ = posterior_draws(db, S)
        tin, first, dist = torch.empty((S, B), **f64), torch.empty((S, B), **f64), torch.empty((S, B), **f64)
        nent, nbrk = torch.empty((S, B), **i32), torch.empty((S, B), **i32)
        mask = torch.zeros((S, rows, B), dtype=torch.uint8, device=db.device)

        def region(V, east, model=None, flags=False):
            poly, vert = polygon(V, east)
            rg = binding.SteRegionF64()
            rg.nstates, rg.states, rg.nvert, rg.vert, rg.lon_ref = S, draws.data_ptr(), V, vert.data_ptr(), poly.lon_ref
            rg.time_inside, rg.first_entry, rg.nenter, rg.nbroken = tin.data_ptr(), first.data_ptr(), nent.data_ptr(), nbrk.data_ptr()
            if model is not None:
                rg.model, rg.dist_inside = model, dist.data_ptr()
            if flags:
                rg.inside = mask.data_ptr()

            def call():
                binding.check(lib.ste_region_metrics_f64(C.byref(db.struct), C.byref(rg), s), "ste_region_metrics_f64")

            ms, samples = timed(call, args.rounds)
            del vert
            return ms, samples

        out = {"label": args.label, "tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "region_ms": {},
               "region_samples": {}, "inside_share": {}, "polygon_extent_deg": [round(2 * scale * v, 2) for v in spread]}
        for V in args.vertices:
            for where, east in WHERE.items():
                key = f"V{V}/{where}"
                out["region_ms"][key], out["region_samples"][key] = region(V, east)
                if V == 64 or len(args.vertices) == 1:
                    out["inside_share"][where] = float((nent > 0).double().mean().item())
                    out.setdefault("broken_steps", {})[where] = int(nbrk.sum().item())
        out["region_dist_ms"] = {name: region(64, 0.0, model=code)[0]
                                 for name, code in (("sphere", binding.STE_PREP_SPHERE), ("wgs84", binding.STE_PREP_WGS84))}
        out["region_mask_ms"] = region(64, 0.0, flags=True)[0]
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, binding.STE_PREP_SPHERE, draws.data_ptr(), dist.data_ptr(), -1

        def path():
            binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

        out["path_ms"], out["path_samples"] = timed(path, args.rounds)
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; region_ms keyed V<vertices>/<where>"
        append_json(args.out, out)
        del draws, sm, keep


if __name__ == "__main__":
    main()
