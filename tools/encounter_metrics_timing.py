#!/usr/bin/env python3
"""Encounter quantities (ste_encounter_metrics_f64) on a clustered fleet, timed with HIP events after a warm-up; each figure is
the median of --rounds timed calls on S tracks per ship that lie on the device:

  fleet            --tracks ships x --steps steps in clusters of --cluster ships: cluster centres spread over the globe, starts
                   within a box of 3 degrees, a drift of N(0, 0.004) degrees per step per ship plus N(0, 0.002) noise, dt
                   U(0.05, 0.15) h, t0 U(0, 5) h; samples 1 .. S - 1 are sample 0 plus N(0, 0.01) degrees
  pairs            batch.candidate_pairs (the tensor core of encounter_candidates) at --radius km: sorted by (i, j)
  enc_ms           keyed by the order of the pair list: `sorted` as the candidates come, `shuffled` the same list permuted; all
                   eight outputs, sphere
  enc_no_leg_ms    the sorted list without min_dist (no leg function), and enc_no_within_ms without the within-R outputs
  path_ms          ste_path_metrics_f64 (sphere, dist alone) on the same states in the same run: the yardstick
  pieces           pieces examined per sample, counted by the call itself: on a copy of sample 0 with NaN latitudes every
                   piece is broken, so the sum of nbroken is the number of pieces
  pieces_per_s, bytes_per_s   S x pieces / time and 32 B x that (16 B of rows per piece and ship), for the sorted list
  checksum         sha256 of the eight outputs of the sorted call: equal between builds whose bits are equal

One JSON line per sample count S, appended to --out (default profiles/encounter_metrics_timing.jsonl).  Nothing gates on these.
--label goes into every line: it names the build when two builds of the library are compared (STE_LIB_PATH picks one).

usage: tools/encounter_metrics_timing.py [--tracks 10000] [--steps 500] [--rounds 7] [--samples 1 16] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bare_batch, timed  # and the import path of the package

OUTPUTS = ("min_dist", "min_time", "time_within", "first_within", "nwithin", "overlap", "nbroken", "status")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--cluster", type=int, default=100)
    ap.add_argument("--radius", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encounter_metrics_timing.jsonl"))
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
    dt = rng.uniform(0.05, 0.15, (N, B))
    db = bare_batch(np.full(B, N), dt)
    lib, s = db.lib, db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    base = torch.zeros((N + 1, 4, B), **f64)
    base[:, :2] = torch.from_numpy(track).to(db.device)
    t0 = torch.from_numpy(rng.uniform(0.0, 5.0, B)).to(db.device)
    pairs = batch.candidate_pairs(base, db.t["nsteps"], db.t["dt"], args.radius, t0=t0).contiguous()
    P = int(pairs.shape[0])
    gen = torch.Generator(device=db.device)
    gen.manual_seed(1)
    orders = {"sorted": pairs, "shuffled": pairs[torch.randperm(P, generator=gen, device=db.device)].contiguous()}

    def encounter(states, S, pr, out):
        en = binding.SteEncounterF64()
        en.nstates, en.model, en.states = S, binding.STE_PREP_SPHERE, states.data_ptr()
        en.npairs, en.pairs, en.t0, en.radius_km = int(pr.shape[0]), pr.data_ptr(), t0.data_ptr(), args.radius
        for k, ten in out.items():
            setattr(en, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_encounter_metrics_f64(C.byref(db.struct), C.byref(en), s), "ste_encounter_metrics_f64")

    def outputs(S, names=OUTPUTS):
        return {k: torch.empty((P,) if k == "status" else (S, P), **(i32 if k in ("nwithin", "nbroken", "status") else f64))
                for k in names}

    # the number of pieces, from the call itself: with every latitude NaN every piece is broken
    broken = base.clone()[None]
    broken[:, :, 1] = float("nan")
    count = outputs(1, ("nbroken",))
    encounter(broken, 1, pairs, count)()
    torch.cuda.synchronize()
    pieces = int(count["nbroken"].sum(dtype=torch.int64).item())
    del broken, count

    for S in args.samples:
        states = base[None].repeat(S, 1, 1, 1)
        if S > 1:
            states[1:, :, :2] += 0.01 * torch.randn((S - 1, N + 1, 2, B), generator=gen, **f64)
        out = {"label": args.label, "tracks": B, "rows": N + 1, "nsamples": S, "rounds": args.rounds, "pairs": P,
               "radius_km": args.radius, "pieces": pieces, "enc_ms": {}, "enc_samples": {}}
        res = outputs(S)
        for name, pr in orders.items():
            out["enc_ms"][name], out["enc_samples"][name] = timed(encounter(states, S, pr, res), args.rounds)
        call = encounter(states, S, pairs, res)
        call()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for k in OUTPUTS:
            h.update(res[k].cpu().numpy().tobytes())
        out["checksum"] = h.hexdigest()
        out["pairs_within"] = int((res["nwithin"][0] > 0).sum().item())
        out["pairs_with_overlap"] = int((res["overlap"][0] > 0).sum().item())
        out["enc_no_leg_ms"] = timed(encounter(states, S, pairs, {k: v for k, v in res.items() if k != "min_dist"}), args.rounds)[0]
        out["enc_no_within_ms"] = timed(encounter(states, S, pairs, {k: v for k, v in res.items() if k not in (
            "time_within", "first_within", "nwithin")}), args.rounds)[0]
        dist = torch.empty((S, B), **f64)
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, binding.STE_PREP_SPHERE, states.data_ptr(), dist.data_ptr(), -1

        def path():
            binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

        out["path_ms"], out["path_samples"] = timed(path, args.rounds)
        ms = out["enc_ms"]["sorted"]
        out["ratio_to_path"] = {k: v / out["path_ms"] for k, v in out["enc_ms"].items()}
        out["pieces_per_s"] = S * pieces / (ms * 1e-3)
        out["bytes_per_s"] = 32.0 * out["pieces_per_s"]
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; enc_ms keyed by pair order"
        append_json(args.out, out)
        del states, res, dist


if __name__ == "__main__":
    main()
