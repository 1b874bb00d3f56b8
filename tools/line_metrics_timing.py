#!/usr/bin/env python3
"""Line quantities (ste_line_metrics_f64) against the nearest route that existed before them, on one fleet in one process, timed
with HIP events after a warm-up; each figure is the median of --rounds timed calls on S tracks per ship that lie on the device:

  fleet            that of tools/encounter_metrics_timing.py and tools/site_metrics_timing.py: --tracks ships x --steps steps in
                   clusters of --cluster ships (centres spread over the globe, starts within a box of 3 degrees, a drift of
                   N(0, 0.004) degrees per step per ship plus N(0, 0.002) noise, dt U(0.05, 0.15) h, t0 U(0, 5) h; samples
                   1 .. S - 1 are sample 0 plus N(0, 0.01))
  lines            --lines lines of --segments segments, line m through the box of cluster m modulo the number of clusters: from
                   its west side to its east side in equal steps of longitude, a random walk of N(0, 0.01) degrees in latitude
  line_ms          ste_line_metrics_f64, all twelve outputs, sphere; line_no_cross_ms without the four crossing outputs,
                   line_no_leg_ms without min_dist
  pairs            tracks x lines x segments x steps per sample; pairs_per_s = S x pairs / line time
  site_ms          the yardstick: ste_site_metrics_f64 on the same states with every vertex of every line as a site (radius
                   --radius km), all ten outputs; site_no_within_ms without the within-R outputs, the form nearest to what the
                   line call computes.  It answers a coarser question: the nearest VERTEX, not the nearest point of the line.
  site_pieces      tracks x vertices x steps per sample; site_pieces_per_s = S x site_pieces / site time
  checksum         sha256 of the line call's outputs: equal between builds whose bits are equal

One JSON line per sample count S, appended to --out (default profiles/line_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when two builds of the library are compared (STE_LIB_PATH picks one);
--no-site leaves the yardstick out (for comparing builds).

usage: tools/line_metrics_timing.py [--tracks 10000] [--steps 500] [--lines 16] [--segments 256] [--rounds 7] [--samples 1 16]
"""
import argparse
import ctypes as C
import hashlib
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bare_batch, timed  # and the import path of the package

LINE3 = ("min_dist", "min_time", "min_seg", "min_frac", "ncross", "net_cross", "first_cross", "last_cross")
LINE_OUTPUTS = LINE3 + ("sound_time", "nbroken", "track_status", "line_status")
SITE3 = ("min_dist", "min_time", "time_within", "first_within", "longest", "nwithin")
SITE_OUTPUTS = SITE3 + ("sound_time", "nbroken", "track_status", "site_status")
INT32 = ("min_seg", "ncross", "net_cross", "nwithin", "nbroken", "track_status", "line_status", "site_status")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--cluster", type=int, default=100)
    ap.add_argument("--lines", type=int, default=16)
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--radius", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--no-site", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    B, N, M, L = args.tracks, args.steps, args.lines, args.segments
    rng = np.random.default_rng(0)
    ncl = (B + args.cluster - 1) // args.cluster
    centres = np.stack([rng.uniform(-170.0, 170.0, ncl), rng.uniform(-60.0, 60.0, ncl)])
    start = centres[:, np.arange(B) // args.cluster] + rng.uniform(-1.5, 1.5, (2, B))
    steps = rng.normal(0.0, 0.004, (2, B))[None] + rng.normal(0.0, 0.002, (N, 2, B))
    track = np.concatenate([start[None], start[None] + np.cumsum(steps, axis=0)])  # (N + 1, 2, B)
    dt = rng.uniform(0.05, 0.15, (N, B))
    t0h = rng.uniform(0.0, 5.0, B)
    lrng = np.random.default_rng(2)
    lines = []
    for m in range(M):
        c = centres[:, m % ncl]
        lat = c[1] + lrng.uniform(-1.0, 1.0) + np.concatenate([[0.0], np.cumsum(lrng.normal(0.0, 0.01, L))])
        lines.append(np.stack([c[0] + np.linspace(-1.5, 1.5, L + 1), lat], axis=1))
    tl = batch.track_lines(lines)
    V = int(tl.vert.shape[1])

    db = bare_batch(np.full(B, N), dt)
    lib, s = db.lib, db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    base = torch.zeros((N + 1, 4, B), **f64)
    base[:, :2] = torch.from_numpy(track).to(db.device)
    t0 = torch.from_numpy(t0h).to(db.device)
    vert, first, ref = tl.on(db.device)
    rad = torch.full((V,), args.radius, **f64)
    gen = torch.Generator(device=db.device)
    gen.manual_seed(1)

    def line_call(states, S, out):
        li = binding.SteLineF64()
        li.nstates, li.model, li.states = S, binding.STE_PREP_SPHERE, states.data_ptr()
        li.nlines, li.nvert, li.vert, li.first, li.lon_ref, li.t0 = M, V, vert.data_ptr(), first.data_ptr(), ref.data_ptr(), t0.data_ptr()
        for k, ten in out.items():
            setattr(li, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_line_metrics_f64(C.byref(db.struct), C.byref(li), s), "ste_line_metrics_f64")

    def site_call(states, S, out):
        si = binding.SteSiteF64()
        si.nstates, si.model, si.states = S, binding.STE_PREP_SPHERE, states.data_ptr()
        si.nsites, si.sites, si.radius_km, si.t0 = V, vert.data_ptr(), rad.data_ptr(), t0.data_ptr()
        for k, ten in out.items():
            setattr(si, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_site_metrics_f64(C.byref(db.struct), C.byref(si), s), "ste_site_metrics_f64")

    def outputs(names, S, width):
        shape = {"sound_time": (S, B), "nbroken": (S, B), "track_status": (B,), "line_status": (M,), "site_status": (V,)}
        return {k: torch.empty(shape.get(k, (S, width, B)), **(i32 if k in INT32 else f64)) for k in names}

    for S in args.samples:
        states = base[None].repeat(S, 1, 1, 1)
        if S > 1:
            states[1:, :, :2] += 0.01 * torch.randn((S - 1, N + 1, 2, B), generator=gen, **f64)
        out = {"label": args.label, "tracks": B, "rows": N + 1, "lines": M, "segments": L, "nsamples": S, "rounds": args.rounds,
               "line_chunk": int(lib.ste_line_chunk()), "pairs": B * M * L * N}
        res = outputs(LINE_OUTPUTS, S, M)
        out["line_ms"], out["line_samples"] = timed(line_call(states, S, res), args.rounds)
        h = hashlib.sha256()
        for k in LINE_OUTPUTS:
            h.update(res[k].cpu().numpy().tobytes())
        out["checksum"] = h.hexdigest()
        out["pairs_crossed"] = int((res["ncross"][0] > 0).sum().item())
        out["line_no_cross_ms"] = timed(line_call(states, S, {k: v for k, v in res.items() if k not in (
            "ncross", "net_cross", "first_cross", "last_cross")}), args.rounds)[0]
        out["line_no_leg_ms"] = timed(line_call(states, S, {k: v for k, v in res.items() if k != "min_dist"}), args.rounds)[0]
        out["pairs_per_s"] = S * out["pairs"] / (out["line_ms"] * 1e-3)
        del res
        if not args.no_site:
            sres = outputs(SITE_OUTPUTS, S, V)
            out["sites"], out["radius_km"], out["site_tile"] = V, args.radius, int(lib.ste_site_tile())
            out["site_pieces"] = B * V * N
            out["site_ms"], out["site_samples"] = timed(site_call(states, S, sres), args.rounds)
            out["site_no_within_ms"] = timed(site_call(states, S, {k: v for k, v in sres.items() if k not in (
                "time_within", "first_within", "longest", "nwithin")}), args.rounds)[0]
            out["site_pieces_per_s"] = S * out["site_pieces"] / (out["site_ms"] * 1e-3)
            out["site_pieces_per_s_no_within"] = S * out["site_pieces"] / (out["site_no_within_ms"] * 1e-3)
            out["pairs_per_s_over_site_pieces_per_s"] = out["pairs_per_s"] / out["site_pieces_per_s"]
            del sres
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up"
        append_json(args.out, out)
        del states


if __name__ == "__main__":
    main()
