#!/usr/bin/env python3
"""Errors against truth positions (ste_track_errors_f64) at the bench batch against the distance of path_metrics on the same
tracks in the same run, timed with HIP events after a warm-up; each figure is the median of --rounds timed calls on S posterior
tracks per ship that the sampler left on the device, for the sphere and WGS84.  The truth is the smoothed track displaced by
0.05 degrees in both coordinates, at every row (the dense case: every row costs a leg), the course the smoothed track's heading:

  path_ms          DeviceBatch.path_metrics, distance only, on the S tracks and on the smoothed track alone (S = 1): the yardsticks
                   (the same leg function once per row; 16 bytes per row where the error call reads 32)
  error_ms         ste_track_errors_f64 on outputs allocated once:
                     dist     sum_err, sum_sq, max_err, n: the kernel without heading arithmetic and covariance loads
                     sparse   the same with the batch's own reports as truth (batch.observation_rows: one row in --substeps)
                     course   the sums along and across the course as well (no per-row output)
                     rows     dist plus the per-row err and cumerr
                     nees     S = 1, the smoothed track against sm_cov: every sum, along / cross and NEES
  ratio            error_ms / path_ms per case (nees against the S = 1 yardstick)

One JSON line per sample count S, appended to --out (default profiles/error_metrics_timing.jsonl); --label names the build
(STE_ERROR_TILE of csrc/ste_error.hip).  Nothing gates on these.

usage: tools/error_metrics_timing.py [--tracks 10000] [--rounds 7] [--samples 16] [--label tile1] [--out FILE]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package

SUMS = ("sum_err", "sum_sq", "max_err", "n")
COURSE = ("sum_along", "sum_along_sq", "sum_cross", "sum_cross_sq", "ncoursed")
NEES = ("sum_nees", "nscored", "ninside")
INT32 = ("n", "ncoursed", "nscored", "ninside")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[16])
    ap.add_argument("--label", default="tile1", help="the build: STE_ERROR_TILE of csrc/ste_error.hip")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, N = db.lib, hb.B, hb.Nmax
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    dense = (db.sm_mean[:, :2] + 0.05).contiguous()
    sparse = torch.from_numpy(batch.observation_rows(hb)).to(db.device)
    course = db.sm_mean[:, 3].contiguous()

    for S in args.samples:
        tracks, sm, status, keep, _ = posterior_draws(db, S)
        res = {k: torch.empty((S, B), **(i32 if k in INT32 else f64)) for k in SUMS + COURSE + NEES}
        rows = {k: torch.empty((S, N + 1, B), **f64) for k in ("err", "cumerr")}
        out = {"label": args.label, "tracks": B, "rows": N + 1, "nsamples": S, "rounds": args.rounds, "truthed_rows_sparse":
               int(torch.isfinite(sparse[:, 0]).sum().item()), "path_ms": {}, "path_samples": {}, "error_ms": {}, "error_samples": {},
               "ratio": {}}
        for model, code in (("sphere", binding.STE_PREP_SPHERE), ("wgs84", binding.STE_PREP_WGS84)):
            yard = {}
            for name, st in ((model, tracks), (model + ":S1", db.sm_mean)):
                yard[name], out["path_samples"][name] = timed(lambda: db.path_metrics(st, model=model), args.rounds)
                out["path_ms"][name] = yard[name]
            for case in ("dist", "sparse", "course", "rows", "nees"):
                er = binding.SteErrorsF64()
                one = case == "nees"
                er.nstates, er.model, er.states = (1 if one else S), code, (db.sm_mean if one else tracks).data_ptr()
                er.truth = (sparse if case == "sparse" else dense).data_ptr()
                names = SUMS + (COURSE if case in ("course", "nees") else ()) + (NEES if one else ())
                for k in names:
                    setattr(er, k, res[k].data_ptr())
                if case in ("course", "nees"):
                    er.course = course.data_ptr()
                if one:
                    er.cov, er.cov_rows, er.nees_limit = db.sm_cov.data_ptr(), int(db.sm_cov.shape[1]), 5.991464547107979
                if case == "rows":
                    er.err, er.cumerr = rows["err"].data_ptr(), rows["cumerr"].data_ptr()

                def errors():
                    binding.check(lib.ste_track_errors_f64(C.byref(db.struct), C.byref(er), s), "ste_track_errors_f64")

                key = model + ":" + case
                out["error_ms"][key], out["error_samples"][key] = timed(errors, args.rounds)
                out["ratio"][key] = round(out["error_ms"][key] / yard[model + ":S1" if one else model], 3)
                if case == "dist":
                    out.setdefault("mean_rmse_km", {})[model] = float(torch.sqrt(res["sum_sq"] / res["n"]).mean().item())
                if one:
                    out.setdefault("coverage_smoothed", {})[model] = float((res["ninside"][0].sum() / res["nscored"][0].sum()).item())
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = ("HIP events on the current stream, median of rounds after one warm-up; path_ms through DeviceBatch.path_metrics "
                       "(name:S1 = the smoothed track alone), error_ms through the C ABI on outputs allocated once, keyed by model:case")
        append_json(args.out, out)
        del tracks, sm, keep, res, rows


if __name__ == "__main__":
    main()
