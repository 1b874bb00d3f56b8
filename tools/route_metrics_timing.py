#!/usr/bin/env python3
"""Route quantities (ste_route_metrics_f64) on a clustered fleet, timed with HIP events after a warm-up; each figure is the median
of --rounds timed calls on S tracks per ship that lie on the device:

  fleet            --tracks ships x --steps steps in clusters of --cluster ships: cluster centres spread over the globe, starts
                   within a box of 3 degrees, a drift of N(0, 0.004) degrees per step per ship plus N(0, 0.002) noise; samples
                   1 .. S - 1 are sample 0 plus N(0, 0.01) degrees
  pairs            batch.route_endpoint_pairs (the tensor core of route_candidates) at --within km, the first --max-pairs of them
  route_ms         keyed by what is asked for and the band: `frechet` (frechet, frechet_at, status) and `dtw` (all five outputs),
                   each with band 0 and band --band, sphere
  cells            cells of the tables per sample: P x rows x rows without a band, the admissible ones with it
  cells_per_s      S x cells / time, per key of route_ms
  path_ms          ste_path_metrics_f64 (sphere, dist alone) on the same states in the same run: the yardstick
  checksum         sha256 of the five outputs of the `dtw` call per band: equal between builds whose bits are equal

One JSON line per sample count S, appended to --out (default profiles/route_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when two builds of the library are compared (STE_LIB_PATH picks one).

usage: tools/route_metrics_timing.py [--tracks 10000] [--steps 500] [--rounds 7] [--samples 1 16] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bare_batch, timed  # and the import path of the package

OUTPUTS = ("frechet", "frechet_at", "dtw", "dtw_len", "status")
FRECHET = ("frechet", "frechet_at", "status")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--cluster", type=int, default=100)
    ap.add_argument("--within", type=float, default=100.0)
    ap.add_argument("--max-pairs", type=int, default=10_000)
    ap.add_argument("--band", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    B, N = args.tracks, args.steps
    rng = np.random.default_rng(0)
    ncl = (B + args.cluster - 1) // args.cluster
    centre = np.stack([rng.uniform(-170.0, 170.0, ncl), rng.uniform(-60.0, 60.0, ncl)])[:, np.arange(B) // args.cluster]
    start = centre + rng.uniform(-1.5, 1.5, (2, B))
    steps = rng.normal(0.0, 0.004, (2, B))[None] + rng.normal(0.0, 0.002, (N, 2, B))
    track = np.concatenate([start[None], start[None] + np.cumsum(steps, axis=0)])  # (N + 1, 2, B)
    db = bare_batch(np.full(B, N), np.full((N, B), 0.1))
    lib, s = db.lib, db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    base = torch.zeros((N + 1, 4, B), **f64)
    base[:, :2] = torch.from_numpy(track).to(db.device)
    found = batch.route_endpoint_pairs(base, db.t["nsteps"], args.within)
    pairs = found[:args.max_pairs].contiguous()
    P = int(pairs.shape[0])
    gen = torch.Generator(device=db.device)
    gen.manual_seed(1)
    rows = N + 1
    a = np.arange(rows)
    cells = {0: P * rows * rows, args.band: P * int((np.abs(a[:, None] - a[None, :]) <= args.band).sum())}

    need = int(lib.ste_route_workspace(N, max(args.samples), P))
    work = torch.empty((max(need, 8) // 8,), **f64)

    def route(states, S, band, out):
        ro = binding.SteRouteF64()
        ro.nstates, ro.model, ro.states = S, binding.STE_PREP_SPHERE, states.data_ptr()
        ro.npairs, ro.pairs, ro.band, ro.flags = P, pairs.data_ptr(), band, 0
        ro.work, ro.work_bytes = work.data_ptr(), need
        for k, ten in out.items():
            setattr(ro, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_route_metrics_f64(C.byref(db.struct), C.byref(ro), s), "ste_route_metrics_f64")

    for S in args.samples:
        states = base[None].repeat(S, 1, 1, 1)
        if S > 1:
            states[1:, :, :2] += 0.01 * torch.randn((S - 1, N + 1, 2, B), generator=gen, **f64)
        out = {"label": args.label, "tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "pairs": P,
               "candidates": int(found.shape[0]), "within_km": args.within, "band": args.band, "lds_cols": int(lib.ste_route_lds_cols()),
               "work_bytes": need, "cells": {str(k): v for k, v in cells.items()}, "route_ms": {}, "route_samples": {},
               "cells_per_s": {}, "checksum": {}}
        res = {k: torch.empty((S, P, 2) if k == "frechet_at" else (S, P), **(f64 if k in ("frechet", "dtw") else i32)) for k in OUTPUTS}
        for band in (0, args.band):
            for name, want in (("frechet", FRECHET), ("dtw", OUTPUTS)):
                key = f"{name}_band{band}"
                ms, samples = timed(route(states, S, band, {k: res[k] for k in want}), args.rounds)
                out["route_ms"][key], out["route_samples"][key] = ms, samples
                out["cells_per_s"][key] = S * cells[band] / (ms * 1e-3)
            torch.cuda.synchronize()  # res holds the `dtw` call of this band
            h = hashlib.sha256()
            for k in OUTPUTS:
                h.update(res[k].cpu().numpy().tobytes())
            out["checksum"][str(band)] = h.hexdigest()
            out.setdefault("frechet_median_km", {})[str(band)] = float(res["frechet"][0].nanmedian().item())
            out.setdefault("pairs_with_status", {})[str(band)] = int((res["status"][0] != 0).sum().item())
        dist = torch.empty((S, B), **f64)
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, binding.STE_PREP_SPHERE, states.data_ptr(), dist.data_ptr(), -1

        def path():
            binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

        out["path_ms"], out["path_samples"] = timed(path, args.rounds)
        out["ratio_to_path"] = {k: v / out["path_ms"] for k, v in out["route_ms"].items()}
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; route_ms keyed by outputs and band"
        append_json(args.out, out)
        del states, res, dist


if __name__ == "__main__":
    main()
