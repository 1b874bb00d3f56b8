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
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ship-track-estimators_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

NOBS, SUBSTEPS = 126, 4  # bench.py: 125 gaps of 4 filter steps = 500 steps, 501 rows per track


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch, synthetic
    from track_estimators._hip import binding

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(args.tracks, nobs=NOBS, gap_h=1.0, seed0=0)
    hb = batch.pack_uniform(sb, SUBSTEPS, H, Q, R, P0)
    db = batch.DeviceBatch(hb)
    db.run()
    torch.cuda.synchronize()
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    line_value = db.sm_mean[0, 1].clone()  # every ship's first smoothed latitude: the tracks cross it or hover about it

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
        draws = torch.randn((S, rows, 4, B), generator=gen, **f64)
        sm, status, keep = db._sample_struct(draws, S)
        binding.check(lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), None, C.byref(sm), s), "ste_urtss_sample_prepare_f64")

        def draw():
            binding.check(lib.ste_urtss_sample_draw_f64(C.byref(db.struct), C.byref(sm), s), "ste_urtss_sample_draw_f64")

        out = {"tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds}
        # timed first, on the fresh draws and then on what the call before left; the last call's output is not a set of tracks
        out["draw_ms"], out["draw_samples"] = timed(draw)
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
                ms, samples = timed(path)
                nbytes = S * B * (16 * rows + 8) + (S * B * (8 * (rows - 1) + 12) if line else 0)
                out["path_ms"][key], out["path_samples"][key] = ms, samples
                out["path_gbs"][key] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        out["mean_distance_km"] = float(dist.mean().item())
        out["cross_fraction"] = float((~torch.isnan(ctime)).double().mean().item())
        out["sampler_status_any"] = int(status.cpu().numpy().any())
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; path_* keyed by model (+line)"
        line_json = json.dumps(out)
        print(line_json, flush=True)
        with open(args.out, "a") as f:
            f.write(line_json + "\n")
        del draws, sm, keep


if __name__ == "__main__":
    main()
