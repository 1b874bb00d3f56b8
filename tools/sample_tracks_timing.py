#!/usr/bin/env python3
"""Posterior track sampling (ste_urtss_sample_prepare_f64 / ste_urtss_sample_draw_f64) at the bench batch, timed with HIP
events after a warm-up; each figure is the median of --rounds timed calls on one resident batch after its forward pass:

  prepare_ms      urtss_sample_coef: the coefficients (K, x_b, T) of every (row, track), work rows in D form
  recur_ms        urtss_sample_recur: the recurrence for S samples, forced to 1, 2 and 4 samples per lane, and "library": the
                  library's own choice by launch size, which is what callers get
  recur_gbs       effective bandwidth of the recurrence under its bytes model: 64 B per (track, row, sample) -- four draws
                  read, four states written -- plus 240 B per (track, row) once (the 30 coefficients; the 32 B of the
                  filtered mean are left out of the model, as are the re-reads of the coefficients by every sample group)

One JSON line per sample count S, appended to --out (default profiles/track_sampling_timing.jsonl).  For scale: the one-kernel
smoother moves 4.9 TB/s at this batch (README.md).  Repeated draw calls run on the buffer the call before left (samples, not
fresh draws); the kernel's work does not depend on the values.

usage: tools/sample_tracks_timing.py [--tracks 10000] [--rounds 7] [--samples 1 4 16] [--out FILE]
"""
import argparse
import ctypes as C
import os

from metrics_timing_common import ROOT, append_json, bench_batch, posterior_draws, timed  # and the import path of the package

SMOOTHER_TBS = 4.9  # README.md: what the one-kernel smoother moves at this batch


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_sampling_timing.jsonl"))
    args = ap.parse_args()

    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks, smooth=False)
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    lib.ste_dbg_sample_lanes.restype = C.c_int
    lib.ste_dbg_sample_lanes.argtypes = [C.c_int]

    for S in args.samples:
        draws, sm, status, keep, _ = posterior_draws(db, S, sample=False)

        def prepare():
            binding.check(lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), None, C.byref(sm), s), "ste_urtss_sample_prepare_f64")

        def draw():
            binding.check(lib.ste_urtss_sample_draw_f64(C.byref(db.struct), C.byref(sm), s), "ste_urtss_sample_draw_f64")

        model_bytes = B * rows * (64 * S + 240)
        out = {"tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "model_bytes": model_bytes,
               "smoother_tbs": SMOOTHER_TBS}
        out["prepare_ms"], out["prepare_samples"] = timed(prepare, args.rounds)
        out["recur_ms"], out["recur_gbs"], out["recur_samples"] = {}, {}, {}
        for spl in (1, 2, 4, 0):  # 0: the library's own choice by launch size, what callers get
            lib.ste_dbg_sample_lanes(spl)
            ms, samples = timed(draw, args.rounds)
            key = str(spl) if spl else "library"
            out["recur_ms"][key], out["recur_samples"][key] = ms, samples
            out["recur_gbs"][key] = round(model_bytes / (ms * 1e-3) / 1e9, 1)
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; recur_* keyed by samples per lane"
        append_json(args.out, out)
        del draws, sm, keep


if __name__ == "__main__":
    main()
