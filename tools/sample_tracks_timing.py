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
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ship-track-estimators_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

NOBS, SUBSTEPS = 126, 4  # bench.py: 125 gaps of 4 filter steps = 500 steps per track
SMOOTHER_TBS = 4.9  # README.md: what the one-kernel smoother moves at this batch


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_sampling_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(args.tracks, nobs=NOBS, gap_h=1.0, seed0=0)
    hb = batch.pack_uniform(sb, SUBSTEPS, H, Q, R, P0)
    db = batch.DeviceBatch(hb)
    db.forward()
    torch.cuda.synchronize()
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    lib.ste_dbg_sample_lanes.restype = C.c_int
    lib.ste_dbg_sample_lanes.argtypes = [C.c_int]

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        samples = []
        for _ in range(args.rounds):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1))
        return float(np.median(samples)), [round(v, 3) for v in samples]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for S in args.samples:
        gen = torch.Generator(device=db.device)
        gen.manual_seed(0)
        draws = torch.randn((S, rows, 4, B), generator=gen, dtype=torch.float64, device=db.device)
        sm, status, keep = db._sample_struct(draws, S)

        def prepare():
            binding.check(lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), None, C.byref(sm), s), "ste_urtss_sample_prepare_f64")

        def draw():
            binding.check(lib.ste_urtss_sample_draw_f64(C.byref(db.struct), C.byref(sm), s), "ste_urtss_sample_draw_f64")

        model_bytes = B * rows * (64 * S + 240)
        out = {"tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "model_bytes": model_bytes,
               "smoother_tbs": SMOOTHER_TBS}
        out["prepare_ms"], out["prepare_samples"] = timed(prepare)
        out["recur_ms"], out["recur_gbs"], out["recur_samples"] = {}, {}, {}
        for spl in (1, 2, 4, 0):  # 0: the library's own choice by launch size, what callers get
            lib.ste_dbg_sample_lanes(spl)
            ms, samples = timed(draw)
            key = str(spl) if spl else "library"
            out["recur_ms"][key], out["recur_samples"][key] = ms, samples
            out["recur_gbs"][key] = round(model_bytes / (ms * 1e-3) / 1e9, 1)
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; recur_* keyed by samples per lane"
        line = json.dumps(out)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del draws, sm, keep


if __name__ == "__main__":
    main()
