#!/usr/bin/env python3
"""Candidate pairs for encounters: the cap list (batch.candidate_pairs, torch) against the windowed list of the device
(ste_encounter_candidates_mask_f64 / _list_f64), and ste_encounter_metrics_f64 on either list.  HIP events on the current
stream; every figure is the median of --rounds calls after a warm-up, and the figures alternate: round r times every figure once
before round r + 1 does.

  fleets           `clustered`: the fleet of tools/encounter_metrics_timing.py (clusters of --cluster ships in boxes of 3 degrees,
                   500 steps of about 0.1 h); `voyage`: departures over ten days from anywhere between 50 S and 50 N, 15 to
                   30 km/h on a fixed heading with a random walk in longitude, steps of 0.5 to 1.5 h (the fleet of
                   tests/candidate_cases.voyage_fleet)
  cap              P and the time of batch.candidate_pairs at --radius km: the yardstick.  If the list is above
                   STE_ENCOUNTER_MAX_PAIRS the fleet is halved until it fits and `tracks` says what was timed.
  windowed[W]      per window length: P; mask_ms (cand_boxes + cand_mask + cand_count, one call), prefix_ms (torch.cumsum and
                   the host read of P), list_ms (cand_list without details), details_ms (cand_list with wfirst / nwin), call_ms
                   (DeviceBatch.encounter_candidates as a whole, allocation included); nwindows; tile_tests, the box tests
                   cand_mask makes when no tile leaves early (64 x 64 per tile and window of the tile's range), and pair_windows,
                   those between two live boxes of tracks i < j
  enc_ms           ste_encounter_metrics_f64 (sphere, all eight outputs) on each list for every S of --samples, and pairs_within,
                   the pairs of sample 0 with nwithin > 0: it must be the same from every list
  route_ms         candidates + encounters for each list and S

One JSON line per fleet, appended to --out (default profiles/encounter_candidates_timing.jsonl).  Nothing gates on these.
--only-candidates leaves the encounter calls out (a run under a kernel profiler, which splits mask_ms by kernel).

usage: tools/encounter_candidates_timing.py [--fleets clustered voyage] [--tracks 10000] [--steps 500] [--windows 6 24 96]
"""
import argparse
import ctypes as C
import os

import numpy as np

from metrics_timing_common import ROOT, append_json, bare_batch  # and the import path of the package


def clustered(B, N, cluster, rng):
    ncl = (B + cluster - 1) // cluster
    centre = np.stack([rng.uniform(-170.0, 170.0, ncl), rng.uniform(-60.0, 60.0, ncl)])[:, np.arange(B) // cluster]
    start = centre + rng.uniform(-1.5, 1.5, (2, B))
    steps = rng.normal(0.0, 0.004, (2, B))[None] + rng.normal(0.0, 0.002, (N, 2, B))
    track = np.concatenate([start[None], start[None] + np.cumsum(steps, axis=0)])  # (N + 1, 2, B)
    dt = rng.uniform(0.05, 0.15, (N, B))
    return track, dt, rng.uniform(0.0, 5.0, B)


def voyage(B, N, rng):
    dt = rng.uniform(0.5, 1.5, (N, B))
    t0 = rng.uniform(0.0, 240.0, B)
    lon0, lat0 = rng.uniform(-180.0, 180.0, B), rng.uniform(-50.0, 50.0, B)
    hd, v = rng.uniform(0.0, 2.0 * np.pi, B), rng.uniform(15.0, 30.0, B) / 111.0
    T = np.concatenate([np.zeros((1, B)), np.cumsum(dt, axis=0)])
    lon = (lon0 + np.cos(hd) * v * T + 0.02 * rng.standard_normal((N + 1, B)).cumsum(0) + 180.0) % 360.0 - 180.0
    lat = np.clip(lat0 + 0.4 * np.sin(hd) * v * T, -80.0, 80.0)
    return np.stack([lon, lat], axis=1), dt, t0


def alternating(figures, rounds):
    """{name: fn} -> {name: (median ms, every round's ms)}: a warm-up of each, then ``rounds`` rounds of every figure once."""
    import torch

    for fn in figures.values():
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = {k: [] for k in figures}
    for _ in range(rounds):
        for k, fn in figures.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            samples[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), [round(x, 3) for x in v]) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--fleets", nargs="+", default=["clustered", "voyage"], choices=["clustered", "voyage"])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--cluster", type=int, default=100)
    ap.add_argument("--radius", type=float, default=30.0)
    ap.add_argument("--windows", type=float, nargs="+", default=[6.0, 24.0, 96.0])
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--only-candidates", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encounter_candidates_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    for fleet in args.fleets:
        B, N, halved = args.tracks, args.steps, []
        while True:
            rng = np.random.default_rng(0 if fleet == "clustered" else 1)
            track, dt, t0h = clustered(B, N, args.cluster, rng) if fleet == "clustered" else voyage(B, N, rng)
            db = bare_batch(np.full(B, N), dt)
            f64, i32 = dict(dtype=torch.float64, device=db.device), dict(dtype=torch.int32, device=db.device)
            base = torch.zeros((N + 1, 4, B), **f64)
            base[:, :2] = torch.from_numpy(track).to(db.device)
            t0 = torch.from_numpy(t0h).to(db.device)
            cap = batch.candidate_pairs(base, db.t["nsteps"], db.t["dt"], args.radius, t0=t0).contiguous()
            if cap.shape[0] <= binding.STE_ENCOUNTER_MAX_PAIRS:
                break
            halved.append({"tracks": B, "cap_pairs": int(cap.shape[0])})
            B //= 2
        lib, s = db.lib, db._stream(None)
        rec = {"label": args.label, "fleet": fleet, "tracks": B, "rows": N + 1, "radius_km": args.radius, "rounds": args.rounds,
               "all_pairs": B * (B - 1) // 2, "cap_above_max_pairs": halved, "cap": {"pairs": int(cap.shape[0])}, "windowed": {}}
        figures = {"cap": lambda: batch.candidate_pairs(base, db.t["nsteps"], db.t["dt"], args.radius, t0=t0)}
        lists, keep = {"cap": cap}, []
        nwords = (B + 63) // 64
        for W in args.windows:
            det = db.encounter_candidates(args.radius, W, states=base, t0=t0, details=True)
            lists[f"W{W:g}"] = det["pairs"].contiguous()
            NW, P = det["nwindows"], int(det["pairs"].shape[0])
            cd = binding.SteCandidatesF64()
            cd.states, cd.t0, cd.reach_km, cd.time0, cd.window_h, cd.nwindows = base.data_ptr(), t0.data_ptr(), args.radius, det["time0"], W, NW
            work = torch.empty(((lib.ste_encounter_candidates_workspace(B, NW) + 7) // 8,), dtype=torch.int64, device=db.device)
            status, pairs = torch.empty((B,), **i32), torch.empty((max(P, 1), 2), **i32)
            wfirst, nwin = torch.empty((max(P, 1),), **i32), torch.empty((max(P, 1),), **i32)
            cd.workspace, cd.workspace_bytes, cd.track_status = work.data_ptr(), 8 * work.numel(), status.data_ptr()
            at = 2 * (7 * NW * B + B * nwords)
            ints = work.view(torch.int32)
            binding.check(lib.ste_encounter_candidates_mask_f64(C.byref(db.struct), C.byref(cd), s), "mask")
            counts = ints[at + 2 * B: at + 3 * B]
            offsets = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous()
            cd.row_offset, cd.npairs, cd.pairs = offsets.data_ptr(), max(P, 1), pairs.data_ptr()
            cdd = binding.SteCandidatesF64.from_buffer_copy(cd)
            cdd.wfirst, cdd.nwin = wfirst.data_ptr(), nwin.data_ptr()
            keep += [work, status, pairs, wfirst, nwin, offsets]
            # the box tests, from the window ranges the box kernel left in the workspace
            wlo, whi = ints[at: at + B].to(torch.int64), ints[at + B: at + 2 * B].to(torch.int64)
            live = wlo <= whi
            pad = nwords * 64 - B
            tlo = torch.nn.functional.pad(torch.where(live, wlo, torch.full_like(wlo, 1 << 40)), (0, pad), value=1 << 40).view(nwords, 64).min(1).values
            thi = torch.nn.functional.pad(torch.where(live, whi, torch.full_like(whi, -1)), (0, pad), value=-1).view(nwords, 64).max(1).values
            span = (torch.minimum(thi[:, None], thi[None, :]) - torch.maximum(tlo[:, None], tlo[None, :]) + 1).clamp(min=0)
            tile_tests = int(torch.triu(span).sum().item()) * 4096
            common = torch.zeros((), dtype=torch.int64, device=db.device)
            for a in range(0, B, 2048):
                c = (torch.minimum(whi[a:a + 2048, None], whi[None, :]) - torch.maximum(wlo[a:a + 2048, None], wlo[None, :]) + 1).clamp(min=0)
                c = c * (live[a:a + 2048, None] & live[None, :]) * (torch.arange(B, device=db.device)[None, :] > torch.arange(a, min(a + 2048, B), device=db.device)[:, None])
                common += c.sum()
            rec["windowed"][f"W{W:g}"] = {"window_h": W, "nwindows": NW, "pairs": P, "tile_tests": tile_tests, "pair_windows": int(common.item()),
                                          "status_counts": np.bincount(status.cpu().numpy(), minlength=16).tolist()}
            figures[f"W{W:g} mask"] = lambda cd=cd: binding.check(lib.ste_encounter_candidates_mask_f64(C.byref(db.struct), C.byref(cd), s), "mask")
            figures[f"W{W:g} prefix"] = lambda counts=counts: int(torch.cumsum(counts, 0, dtype=torch.int64)[-1])
            if P:
                figures[f"W{W:g} list"] = lambda cd=cd: binding.check(lib.ste_encounter_candidates_list_f64(C.byref(db.struct), C.byref(cd), s), "list")
                figures[f"W{W:g} details"] = lambda cdd=cdd: binding.check(lib.ste_encounter_candidates_list_f64(C.byref(db.struct), C.byref(cdd), s), "list")
            figures[f"W{W:g} call"] = lambda W=W: db.encounter_candidates(args.radius, W, states=base, t0=t0)
        enc_out = {}
        if not args.only_candidates:
            gen = torch.Generator(device=db.device)
            gen.manual_seed(1)
            for S in args.samples:
                states = base[None].repeat(S, 1, 1, 1)
                if S > 1:
                    states[1:, :, :2] += 0.01 * torch.randn((S - 1, N + 1, 2, B), generator=gen, **f64)
                keep.append(states)
                for name, pr in lists.items():
                    if pr.shape[0] == 0:
                        continue
                    P = int(pr.shape[0])
                    out = {k: torch.empty((S, P), **f64) for k in ("min_dist", "min_time", "time_within", "first_within", "overlap")}
                    out.update({k: torch.empty((S, P), **i32) for k in ("nwithin", "nbroken")})
                    out["status"] = torch.empty((P,), **i32)
                    en = binding.SteEncounterF64()
                    en.nstates, en.model, en.states = S, binding.STE_PREP_SPHERE, states.data_ptr()
                    en.npairs, en.pairs, en.t0, en.radius_km = P, pr.data_ptr(), t0.data_ptr(), args.radius
                    for k, ten in out.items():
                        setattr(en, k, ten.data_ptr())
                    enc_out[(name, S)] = out
                    figures[f"enc {name} S{S}"] = lambda en=en: binding.check(lib.ste_encounter_metrics_f64(C.byref(db.struct), C.byref(en), s), "enc")
        times = alternating(figures, args.rounds)
        rec["cap"]["ms"], rec["cap"]["samples"] = times["cap"]
        for key, w in rec["windowed"].items():
            for part in ("mask", "prefix", "list", "details", "call"):
                if f"{key} {part}" in times:
                    w[part + "_ms"], w[part + "_samples"] = times[f"{key} {part}"]
            w["tile_tests_per_s"] = w["tile_tests"] / (w["mask_ms"] * 1e-3)
        if not args.only_candidates:
            rec["enc_ms"], rec["route_ms"], rec["pairs_within"] = {}, {}, {}
            for (name, S), out in enc_out.items():
                ms = times[f"enc {name} S{S}"][0]
                rec["enc_ms"][f"{name} S{S}"] = ms
                rec["route_ms"][f"{name} S{S}"] = ms + (rec["cap"]["ms"] if name == "cap" else rec["windowed"][name]["call_ms"])
                if S == args.samples[0]:
                    rec["pairs_within"][name] = int((out["nwithin"][0] > 0).sum().item())
        rec["what"] = ("HIP events on the current stream, median of rounds after one warm-up, the figures alternating; call_ms is "
                       "DeviceBatch.encounter_candidates as a whole, route_ms = candidates + encounters")
        append_json(args.out, rec)
        del figures, lists, keep, enc_out, base, cap, db
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
