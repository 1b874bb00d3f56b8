#!/usr/bin/env python3
"""Positions at query times (ste_track_positions_f64) at the bench batch, timed with HIP events after a warm-up; each figure is
the median of --rounds timed calls on S posterior tracks per ship that the sampler left on the device:

  queries          --per-ship times per ship, uniform over the ship's own clock span: `sorted` by (track, time), which is what
                   the Python front ends hand to the call, and `shuffled`, the same list permuted
  pos_ms           keyed by order: lon, lat, speed, heading, step, frac and status, knots summed by the call (from 16 384
                   queries on a lane walks the samples itself; below, they go along blockIdx.y)
  pos_reuse_ms     the same with STE_POS_REUSE_KNOTS: the query pass alone; knots_ms is the difference
  pos_lonlat_ms    the sorted list without speed and heading
  mom_ms           keyed by order: count and moments alone (the sample loop inside the lane), knots reused, about the smoothed
                   position
  mom_all_ms       the sorted list with the seven outputs and the moments
  path_ms          ste_path_metrics_f64 (sphere, dist alone) on the same states in the same run: the yardstick
  values_per_s, bytes_per_s   S x Q / time for the sorted list with reuse, and that times the bytes model: 8 B per component and
                   row read (two rows for an interior query, which nearly all are) and 8 B per value written = 96 B
  checksum         sha256 of the seven outputs and of the moments of the sorted calls: equal between builds whose bits are equal

One JSON line per sample count S, appended to --out (default profiles/position_metrics_timing.jsonl).  Nothing gates on these.

usage: tools/position_metrics_timing.py [--tracks 10000] [--per-ship 100] [--rounds 7] [--samples 1 16] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os

from metrics_timing_common import ROOT, append_json, bench_batch, timed  # and the import path of the package

PLAIN = ("lon", "lat", "speed", "heading", "step", "frac", "status")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--per-ship", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_metrics_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, rows = db.lib, hb.B, hb.Nmax + 1
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    gen = torch.Generator(device=db.device)
    gen.manual_seed(1)
    Q = B * args.per_ship
    span = db.t["dt"].sum(dim=0)  # close enough to the in-order sum to stay inside the track
    qtrack = torch.arange(B, **i32).repeat_interleave(args.per_ship)
    qtime = torch.rand((Q,), generator=gen, **f64) * 0.999 * span[qtrack.long()]
    qtime = qtime.view(B, args.per_ship).sort(dim=1).values.reshape(Q).contiguous()  # by (track, time)
    perm = torch.randperm(Q, generator=gen, device=db.device)
    orders = {"sorted": (qtrack, qtime, None), "shuffled": (qtrack[perm].contiguous(), qtime[perm].contiguous(), perm)}
    knots = torch.empty((rows, B), **f64)

    def positions(states, S, order, out, reuse, anchor=None):
        po = binding.StePositionsF64()
        po.nstates, po.flags, po.states = S, binding.STE_POS_REUSE_KNOTS if reuse else 0, states.data_ptr()
        po.nqueries, po.qtrack, po.qtime, po.knots = Q, orders[order][0].data_ptr(), orders[order][1].data_ptr(), knots.data_ptr()
        if anchor is not None:
            po.anchor = anchor.data_ptr()
        for k, ten in out.items():
            setattr(po, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_track_positions_f64(C.byref(db.struct), C.byref(po), s), "ste_track_positions_f64")

    def outputs(S, names=PLAIN):
        return {k: torch.empty((Q,) if k in ("step", "frac", "status") else (S, Q), **(i32 if k in ("step", "status") else f64))
                for k in names}

    # the anchor of the moments: the smoothed position at each query (this call also leaves the knots for the reuse runs)
    sm = outputs(1)
    positions(db.sm_mean, 1, "sorted", sm, False)()
    torch.cuda.synchronize()
    anchors = {"sorted": torch.stack([sm["lon"][0], sm["lat"][0]]).contiguous()}
    anchors["shuffled"] = anchors["sorted"][:, perm].contiguous()
    located, interior = int((sm["step"] >= 0).sum().item()), int((sm["frac"] > 0).sum().item())

    for S in args.samples:
        states = db.sample_smoothed(S, seed=0)
        torch.cuda.synchronize()
        out = {"label": args.label, "tracks": B, "rows": rows, "nsamples": S, "rounds": args.rounds, "queries": Q,
               "located": located, "interior": interior, "pos_ms": {}, "pos_reuse_ms": {}, "mom_ms": {}, "samples_ms": {}}
        res = outputs(S)
        acc = {"count": torch.zeros((Q,), **i32), "moments": torch.zeros((5, Q), **f64)}
        for name in orders:
            out["pos_ms"][name], out["samples_ms"]["pos " + name] = timed(positions(states, S, name, res, False), args.rounds)
            out["pos_reuse_ms"][name], out["samples_ms"]["pos_reuse " + name] = timed(positions(states, S, name, res, True), args.rounds)
            out["mom_ms"][name], out["samples_ms"]["mom " + name] = timed(positions(states, S, name, acc, True, anchors[name]), args.rounds)
        out["knots_ms"] = out["pos_ms"]["sorted"] - out["pos_reuse_ms"]["sorted"]
        out["pos_lonlat_ms"] = timed(positions(states, S, "sorted", {k: v for k, v in res.items() if k not in ("speed", "heading")}, True), args.rounds)[0]
        out["mom_all_ms"] = timed(positions(states, S, "sorted", {**res, **acc}, True, anchors["sorted"]), args.rounds)[0]
        acc["count"].zero_()
        acc["moments"].zero_()
        positions(states, S, "sorted", {**res, **acc}, True, anchors["sorted"])()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for k in PLAIN + ("count", "moments"):
            h.update({**res, **acc}[k].cpu().numpy().tobytes())
        out["checksum"] = h.hexdigest()
        out["counted"] = int(acc["count"].sum(dtype=torch.int64).item())
        dist = torch.empty((S, B), **f64)
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.dist, pm.line_axis = S, binding.STE_PREP_SPHERE, states.data_ptr(), dist.data_ptr(), -1

        def path():
            binding.check(lib.ste_path_metrics_f64(C.byref(db.struct), C.byref(pm), s), "ste_path_metrics_f64")

        out["path_ms"], out["samples_ms"]["path"] = timed(path, args.rounds)
        out["ratio_to_path"] = {"pos " + k: v / out["path_ms"] for k, v in out["pos_reuse_ms"].items()}
        out["ratio_to_path"].update({"mom " + k: v / out["path_ms"] for k, v in out["mom_ms"].items()})
        out["values_per_s"] = S * Q / (out["pos_reuse_ms"]["sorted"] * 1e-3)
        out["bytes_per_s"] = 96.0 * out["values_per_s"]
        out["what"] = "HIP events on the current stream, median of rounds after one warm-up; keyed by the order of the query list"
        append_json(args.out, out)
        del states, res, acc, dist


if __name__ == "__main__":
    main()
