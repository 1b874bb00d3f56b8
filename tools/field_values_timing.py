#!/usr/bin/env python3
"""Values of a space-time gridded field at track positions and times (ste_field_values_f64) at the bench batch, timed with HIP
events; the calls of one sample count are timed ALTERNATING in one process, one round of every call after the other, after a
warm-up round, and each figure is the median of --rounds with the spread (min, max) beside it:

  queries          --per-ship times per ship, uniform over the ship's own clock span: `sorted` by (track, time), which is what
                   the Python front ends hand to the call, and `shuffled`, the same list permuted
  field            a global 0.25 degree grid (1440 x 720, periodic) of 8 slabs over the tracks' clock span, 5 % of the nodes
                   NaN, as double (66 MB) and as float (33 MB)
  acc_ms           keyed by `<type> <order>`: count, moments, vmin and vmax alone (the sample loop inside the lane)
  value_ms         keyed by `<type> sorted`: value and cover (S x Q each) and status
  nearest_ms       keyed by `<type> sorted`: the accumulators alone with STE_FLD_NEAREST (one read per sample instead of eight)
  pos_mom_ms       keyed by order: ste_track_positions_f64, count and moments alone, knots reused, on the same list: the yardstick
  ratio_to_pos_mom acc_ms over pos_mom_ms of the same order: what the eight scattered field reads cost beside the row gathers
  checksum         sha256 of the accumulators and of value and cover of the sorted double calls

One JSON line per sample count S, appended to --out (default profiles/field_values_timing.jsonl).  Nothing gates on these.

usage: tools/field_values_timing.py [--tracks 10000] [--per-ship 100] [--rounds 7] [--samples 1 16] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os

import numpy as np
from metrics_timing_common import ROOT, append_json, bench_batch  # and the import path of the package


def alternating(fns, rounds):
    """Every call of ``fns`` (name -> callable) once to warm up, then ``rounds`` rounds of all of them in turn, each call timed
    with HIP events.  Returns name -> (median ms, [min, max], every ms)."""
    import torch

    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), [round(min(v), 3), round(max(v), 3)], [round(x, 3) for x in v]) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--per-ship", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7, help="timed rounds per figure (median)")
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_values_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B = db.lib, hb.B
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
    orders = {"sorted": (qtrack, qtime), "shuffled": (qtrack[perm].contiguous(), qtime[perm].contiguous())}
    knots = db.track_knots()
    grid = batch.track_grid(-180.0, -90.0, 0.25, 0.25, 1440, 720)
    nt = 8
    values = 10.0 + 20.0 * torch.rand((nt, grid.ny, grid.nx), generator=gen, **f64)
    values[torch.rand(values.shape, generator=gen, device=db.device) < 0.05] = float("nan")
    dtime = float(span.max().item()) / (nt - 1)
    fields = {"f64": batch.track_field(grid, values, 0.0, dtime), "f32": batch.track_field(grid, values.to(torch.float32), 0.0, dtime)}

    def field(states, S, kind, order, out, vanchor=None, nearest=False):
        tf = fields[kind]
        f = binding.SteFieldF64()
        f.nstates, f.states, f.nqueries = S, states.data_ptr(), Q
        f.flags = (binding.STE_GRID_PERIODIC_LON | (binding.STE_FLD_VALUES_F32 if kind == "f32" else 0)
                   | (binding.STE_FLD_NEAREST if nearest else 0))
        f.qtrack, f.qtime, f.knots = orders[order][0].data_ptr(), orders[order][1].data_ptr(), knots.data_ptr()
        f.nx, f.ny, f.nt, f.lon0, f.lat0, f.dlon, f.dlat, f.lon_ref = grid.nx, grid.ny, nt, grid.lon0, grid.lat0, grid.dlon, grid.dlat, grid.lon_ref
        f.time0, f.dtime, f.min_cover, f.values = tf.time0, tf.dtime, 0.0, tf.values.data_ptr()
        if vanchor is not None:
            f.vanchor = vanchor.data_ptr()
        for k, ten in out.items():
            setattr(f, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_field_values_f64(C.byref(db.struct), C.byref(f), s), "ste_field_values_f64")

    def positions(states, S, order, out, anchor=None):
        po = binding.StePositionsF64()
        po.nstates, po.flags, po.states = S, binding.STE_POS_REUSE_KNOTS, states.data_ptr()
        po.nqueries, po.qtrack, po.qtime, po.knots = Q, orders[order][0].data_ptr(), orders[order][1].data_ptr(), knots.data_ptr()
        if anchor is not None:
            po.anchor = anchor.data_ptr()
        for k, ten in out.items():
            setattr(po, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_track_positions_f64(C.byref(db.struct), C.byref(po), s), "ste_track_positions_f64")

    def accumulators():
        return {"count": torch.zeros((3, Q), **i32), "moments": torch.zeros((2, Q), **f64),
                "vmin": torch.full((Q,), float("nan"), **f64), "vmax": torch.full((Q,), float("nan"), **f64)}

    # the anchors: the smoothed track's value and position at each query
    sm = {"value": torch.empty((1, Q), **f64), "status": torch.empty((Q,), **i32)}
    field(db.sm_mean, 1, "f64", "sorted", sm)()
    pos = {"lon": torch.empty((1, Q), **f64), "lat": torch.empty((1, Q), **f64)}
    positions(db.sm_mean, 1, "sorted", pos)()
    torch.cuda.synchronize()
    van = {"sorted": torch.nan_to_num(sm["value"][0]).contiguous()}
    van["shuffled"] = van["sorted"][perm].contiguous()
    anchors = {"sorted": torch.stack([pos["lon"][0], pos["lat"][0]]).contiguous()}
    anchors["shuffled"] = anchors["sorted"][:, perm].contiguous()
    located = int((sm["status"] == 0).sum().item())

    for S in args.samples:
        states = db.sample_smoothed(S, seed=0)
        torch.cuda.synchronize()
        acc = accumulators()
        val = {"value": torch.empty((S, Q), **f64), "cover": torch.empty((S, Q), **f64), "status": torch.empty((Q,), **i32)}
        mom = {"count": torch.zeros((Q,), **i32), "moments": torch.zeros((5, Q), **f64)}
        fns = {}
        for order in orders:
            fns["pos_mom " + order] = positions(states, S, order, mom, anchors[order])
            for kind in fields:
                fns[f"acc {kind} {order}"] = field(states, S, kind, order, acc, van[order])
        for kind in fields:
            fns[f"value {kind} sorted"] = field(states, S, kind, "sorted", val)
            fns[f"nearest {kind} sorted"] = field(states, S, kind, "sorted", acc, van["sorted"], nearest=True)
        res = alternating(fns, args.rounds)
        out = {"label": args.label, "tracks": B, "rows": hb.Nmax + 1, "nsamples": S, "rounds": args.rounds, "queries": Q,
               "located": located, "field": [nt, grid.ny, grid.nx], "acc_ms": {}, "value_ms": {}, "nearest_ms": {}, "pos_mom_ms": {},
               "spread_ms": {k: v[1] for k, v in res.items()}, "samples_ms": {k: v[2] for k, v in res.items()}}
        for k, v in res.items():
            head, rest = k.split(" ", 1)
            out[{"acc": "acc_ms", "value": "value_ms", "nearest": "nearest_ms", "pos_mom": "pos_mom_ms"}[head]][rest] = v[0]
        out["ratio_to_pos_mom"] = {k: v / out["pos_mom_ms"][k.split(" ")[1]] for k, v in out["acc_ms"].items()}
        out["values_per_s"] = S * Q / (out["acc_ms"]["f64 sorted"] * 1e-3)
        fresh = accumulators()
        field(states, S, "f64", "sorted", {**val, **fresh}, van["sorted"])()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for k in ("value", "cover", "status", "count", "moments", "vmin", "vmax"):
            h.update({**val, **fresh}[k].cpu().numpy().tobytes())
        out["checksum"] = h.hexdigest()
        out["counted"] = [int(v) for v in fresh["count"].sum(dim=1, dtype=torch.int64).tolist()]
        out["what"] = ("HIP events on the current stream; the calls alternate round by round in one process after one warm-up "
                       "round; medians, with [min, max] in spread_ms")
        append_json(args.out, out)
        del states, acc, val, mom, fresh


if __name__ == "__main__":
    main()
