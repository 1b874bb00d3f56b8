#!/usr/bin/env python3
"""Site quantities (ste_site_metrics_f64) against the route that existed before them, on one fleet in one process, timed with HIP
events after a warm-up; each figure is the median of --rounds timed calls on S tracks per ship that lie on the device:

  fleet            that of tools/encounter_metrics_timing.py: --tracks ships x --steps steps in clusters of --cluster ships
                   (centres spread over the globe, starts within a box of 3 degrees, a drift of N(0, 0.004) degrees per step per
                   ship plus N(0, 0.002) noise, dt U(0.05, 0.15) h, t0 U(0, 5) h; samples 1 .. S - 1 are sample 0 plus N(0, 0.01))
  sites            --sites points, site m in the box of cluster m modulo the number of clusters; --radius km each
  site_ms          ste_site_metrics_f64, all ten outputs, sphere; site_no_leg_ms without min_dist, site_no_within_ms without
                   the within-R outputs
  enc_ms           ste_encounter_metrics_f64 on the same states with one stationary column per site appended (nsteps 1, one step
                   that holds every clock) and the full tracks x sites pair list sorted by (track, site), all eight outputs
  enc_setup_ms     wall time to build those columns, the batch that holds them and the pair list: reported, in no figure
  ratio            enc_ms / site_ms
  pieces           tracks x sites x steps per sample; pieces_per_s = S x pieces / site time
  agree            whether the outputs the two calls share are equal bit for bit (min_dist, min_time, time_within,
                   first_within, nwithin; overlap against sound_time)
  checksum         sha256 of the site call's outputs: equal between builds whose bits are equal

One JSON line per sample count S, appended to --out (default profiles/site_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when two builds of the library are compared (STE_LIB_PATH picks one);
--no-encounter leaves the yardstick out (for comparing builds).

usage: tools/site_metrics_timing.py [--tracks 10000] [--steps 500] [--sites 256] [--rounds 7] [--samples 1 16] [--label X]
"""
import argparse
import ctypes as C
import hashlib
import os
import time

import numpy as np

from metrics_timing_common import ROOT, append_json, bare_batch, timed  # and the import path of the package

SITE3 = ("min_dist", "min_time", "time_within", "first_within", "longest", "nwithin")
SITE_OUTPUTS = SITE3 + ("sound_time", "nbroken", "track_status", "site_status")
ENC_OUTPUTS = ("min_dist", "min_time", "time_within", "first_within", "nwithin", "overlap", "nbroken", "status")
INT32 = ("nwithin", "nbroken", "status", "track_status", "site_status")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--cluster", type=int, default=100)
    ap.add_argument("--sites", type=int, default=256)
    ap.add_argument("--radius", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--no-encounter", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators._hip import binding

    B, N, M = args.tracks, args.steps, args.sites
    rng = np.random.default_rng(0)
    ncl = (B + args.cluster - 1) // args.cluster
    centres = np.stack([rng.uniform(-170.0, 170.0, ncl), rng.uniform(-60.0, 60.0, ncl)])
    start = centres[:, np.arange(B) // args.cluster] + rng.uniform(-1.5, 1.5, (2, B))
    steps = rng.normal(0.0, 0.004, (2, B))[None] + rng.normal(0.0, 0.002, (N, 2, B))
    track = np.concatenate([start[None], start[None] + np.cumsum(steps, axis=0)])  # (N + 1, 2, B)
    dt = rng.uniform(0.05, 0.15, (N, B))
    t0h = rng.uniform(0.0, 5.0, B)
    srng = np.random.default_rng(2)
    sites = (centres[:, np.arange(M) % ncl] + srng.uniform(-1.5, 1.5, (2, M)))  # [2][M]: lon then lat

    db = bare_batch(np.full(B, N), dt)
    lib, s = db.lib, db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    base = torch.zeros((N + 1, 4, B), **f64)
    base[:, :2] = torch.from_numpy(track).to(db.device)
    t0 = torch.from_numpy(t0h).to(db.device)
    xy = torch.from_numpy(np.ascontiguousarray(sites)).to(db.device)
    rad = torch.full((M,), args.radius, **f64)
    gen = torch.Generator(device=db.device)
    gen.manual_seed(1)

    def site_call(states, S, out):
        si = binding.SteSiteF64()
        si.nstates, si.model, si.states = S, binding.STE_PREP_SPHERE, states.data_ptr()
        si.nsites, si.sites, si.radius_km, si.t0 = M, xy.data_ptr(), rad.data_ptr(), t0.data_ptr()
        for k, ten in out.items():
            setattr(si, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_site_metrics_f64(C.byref(db.struct), C.byref(si), s), "ste_site_metrics_f64")

    def site_outputs(S):
        shape = {"sound_time": (S, B), "nbroken": (S, B), "track_status": (B,), "site_status": (M,)}
        return {k: torch.empty(shape.get(k, (S, M, B)), **(i32 if k in INT32 else f64)) for k in SITE_OUTPUTS}

    for S in args.samples:
        states = base[None].repeat(S, 1, 1, 1)
        if S > 1:
            states[1:, :, :2] += 0.01 * torch.randn((S - 1, N + 1, 2, B), generator=gen, **f64)
        out = {"label": args.label, "tracks": B, "rows": N + 1, "sites": M, "nsamples": S, "rounds": args.rounds,
               "radius_km": args.radius, "site_tile": int(lib.ste_site_tile()), "pieces": B * M * N}
        res = site_outputs(S)
        out["site_ms"], out["site_samples"] = timed(site_call(states, S, res), args.rounds)
        h = hashlib.sha256()
        for k in SITE_OUTPUTS:
            h.update(res[k].cpu().numpy().tobytes())
        out["checksum"] = h.hexdigest()
        out["pairs_within"] = int((res["nwithin"][0] > 0).sum().item())
        out["site_no_leg_ms"] = timed(site_call(states, S, {k: v for k, v in res.items() if k != "min_dist"}), args.rounds)[0]
        out["site_no_within_ms"] = timed(site_call(states, S, {k: v for k, v in res.items() if k not in (
            "time_within", "first_within", "longest", "nwithin")}), args.rounds)[0]
        out["pieces_per_s"] = S * out["pieces"] / (out["site_ms"] * 1e-3)
        if not args.no_encounter:
            # the route that existed: one stationary ship per site in every sample, and every (track, site) as a pair
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            span = float((t0h + dt.sum(axis=0)).max() - t0h.min())
            dt2 = np.ones((N, B + M))
            dt2[:, :B] = dt
            dt2[0, B:] = span + 2.0
            edb = bare_batch(np.concatenate([np.full(B, N), np.ones(M)]), dt2)
            est = torch.zeros((S, N + 1, 4, B + M), **f64)
            est[..., :B] = states
            est[:, :, 0, B:], est[:, :, 1, B:] = xy[0], xy[1]
            et0 = torch.cat([t0, torch.full((M,), float(t0h.min()) - 1.0, **f64)])
            i = torch.arange(B, device=db.device, dtype=torch.int32).repeat_interleave(M)
            j = torch.arange(B, B + M, device=db.device, dtype=torch.int32).repeat(B)
            pairs = torch.stack([i, j], dim=1).contiguous()
            torch.cuda.synchronize()
            out["enc_setup_ms"] = (time.perf_counter() - w0) * 1e3
            P = int(pairs.shape[0])
            eres = {k: torch.empty((P,) if k == "status" else (S, P), **(i32 if k in INT32 else f64)) for k in ENC_OUTPUTS}
            en = binding.SteEncounterF64()
            en.nstates, en.model, en.states = S, binding.STE_PREP_SPHERE, est.data_ptr()
            en.npairs, en.pairs, en.t0, en.radius_km = P, pairs.data_ptr(), et0.data_ptr(), args.radius
            for k, ten in eres.items():
                setattr(en, k, ten.data_ptr())
            es = edb._stream(None)

            def enc_call():
                binding.check(lib.ste_encounter_metrics_f64(C.byref(edb.struct), C.byref(en), es), "ste_encounter_metrics_f64")

            out["enc_ms"], out["enc_samples"] = timed(enc_call, args.rounds)
            out["enc_pairs"] = P
            out["ratio"] = out["enc_ms"] / out["site_ms"]
            agree = {}
            for k in ("min_dist", "min_time", "time_within", "first_within", "nwithin"):
                a, b = res[k].transpose(1, 2).reshape(S, P), eres[k]
                agree[k] = bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                            b.view(torch.int64) if b.dtype == torch.float64 else b))
                if not agree[k] and a.dtype == torch.float64:
                    agree[k + "_max_abs_diff"] = float(torch.nan_to_num(a - b).abs().max().item())
            agree["sound_time"] = bool(torch.equal(res["sound_time"][:, :, None].expand(S, B, M).reshape(S, P).contiguous().view(torch.int64),
                                                   eres["overlap"].view(torch.int64)))
            out["agree"] = agree
            del est, eres, pairs, edb
        out["what"] = ("HIP events on the current stream, median of rounds after one warm-up; enc_setup_ms by the wall clock, in no "
                       "other figure")
        append_json(args.out, out)
        del states, res


if __name__ == "__main__":
    main()
