#!/usr/bin/env python3
"""Path quantities (ste_path_metrics_f64) at the bench batch, timed with HIP events after a warm-up; each figure is the median
of --rounds timed calls on S posterior tracks per ship that the sampler left on the device:

  path_ms         path_metrics<model, line>: distance (dist alone) and, with a line, cross_time and ncross too, for the sphere
                  and WGS84, without a line and with a parallel through every ship's first smoothed position
  draw_ms         ste_urtss_sample_draw_f64 for the same S in the same run: what producing the tracks costs, for scale
  path_gbs        effective bandwidth under the bytes model: 16 B per (sample, track, row) -- lon and lat; the other two
                  components are not read -- plus 8 B per (sample, track) out (with a line: 8 B per (track, step) of dt per
                  sample and 12 B more out)

One JSON line per sample count S, appended to --out (default profiles/path_metrics_timing.jsonl).  Nothing gates on these.

usage: tools/path_metrics_timing.py [--tracks 10000] [--rounds 7] [--samples 1 4 16] [--out FILE]
"""
import argparse
import ctypes as C
import os

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    line_value = db.sm_mean[0, 1].clone()  # every ship's first smoothed latitude: the tracks cross it or hover about it

    for S in args.samples:
        draws, sm, status, keep, gen = posterior_draws(db, S, sample=False)
        binding.check(lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), None, C.byref(sm), s), "ste_urtss_sample_prepare_f64")

        def draw():
            binding.check(lib.ste_urtss_sample_draw_f64(C.byref(db.struct), C.byref(sm), s), "ste_urtss_sample_draw_f64")

        out = {"tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds}
        # timed first, on the fresh draws and then on what the call before left; the last call's output is not a set of tracks
        out["draw_ms"], out["draw_samples"] = timed(draw, args.rounds)
        draws.normal_(generator=gen)
        draw()  # the tracks the path kernels are timed on: one draw from fresh normal deviates
        dist = torch.empty((S, B), **f64)
        ctime = torch.empty((S, B), **f64)
        ncross = torch.empty((S, B), dtype=torch.int32, device=db.device)
        out["path_ms"], out["path_gbs"], out["path_samples"] = {}, {}, {}
        for model, code in (("sphere", binding.STE_PREP_SPHERE), ("wgs84", binding.STE_PREP_WGS84)):
            for line in (False, True):
                pm = binding.StePathF64()
                pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, code, draws.data_ptr(), dist.data_ptr(), -1
                if line:
                    pm.line_axis, pm.line_value = 1, line_value.data_ptr()
                    pm.cross_time, pm.ncross = ctime.data_ptr(), ncross.data_ptr()

                def path():
                    binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

                key = model + ("+line" if line else "")
                ms, samples = timed(path, args.rounds)
                nbytes = S * B * (16 * rows + 8) + (S * B * (8 * (rows - 1) + 12) if line else 0)
                out["path_ms"][key], out["path_samples"][key] = ms, samples
                out["path_gbs"][key] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        out["mean_distance_km"] = float(dist.mean().item())
        out["cross_fraction"] = float((~torch.isnan(ctime)).double().mean().item())
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; path_* keyed by model (+line)"
        append_json(args.out, out)
        del draws, sm, keep


if __name__ == "__main__":
    main()
