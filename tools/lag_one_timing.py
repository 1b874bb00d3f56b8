#!/usr/bin/env python3
"""The lag-one covariance (ste_urtss_lag_one_f64) and the covariance of positions at query times (ste_track_position_cov_f64)
at the bench batch, timed with HIP events after a warm-up.  The figures of a group alternate call by call in one process, so
they see the same clocks; each is the median of --rounds timed calls on one resident batch after ``run()``:

  lag_ms           the lag-one kernel, keyed by output form (`full` 16 entries a row, `position` 4), against
  prepare_ms       ste_urtss_sample_prepare_f64 on the same work rows (D form): the same gain solve plus the symmetric root
  lag_gbs          lag_model_bytes over lag_ms: 8 B for each of the 32 doubles a (step, track) reads once and the 16 or 4 written
  pcov_ms          the query kernel on --per-ship sorted queries per ship, keyed by what it writes: `position` (3 entries, the
                   4-entry lag1: 10 gathers a query), `position_alone` (pcov without step, frac and status), `full` (10 entries
                   from the 16-entry lag1: 36 gathers), against
  mom_ms           ste_track_positions_f64 on sm_mean (S = 1) with count and moments alone, knots reused: 4 gathers a query
  whole_ms         batch.position_covariance on that list, device to NumPy, against batch.position_statistics with 16 and with
                   256 samples (chunks of 16), one call each after a warm-up call (--whole-rounds timed calls, median)
  checksum         sha256 of lag1 (full form) and of pcov (position form): equal between builds whose bits are equal

One JSON line, appended to --out (default profiles/lag_one_timing.jsonl).  Nothing gates on these.

usage: tools/lag_one_timing.py [--tracks 10000] [--per-ship 100] [--rounds 7] [--whole-rounds 3] [--label X] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import os

from metrics_timing_common import ROOT, append_json, bench_batch  # and the import path of the package

import numpy as np  # noqa: E402


def alternating(fns, rounds):
    """Every ``fns[name]()`` once to warm up, then ``rounds`` passes over all of them in turn, each call timed with HIP events
    on the current stream.  Returns ({name: median ms}, {name: every call's ms})."""
    import torch

    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            samples[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in samples.items()}, {k: [round(x, 3) for x in v] for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--per-ship", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7, help="timed calls per kernel figure (median)")
    ap.add_argument("--whole-rounds", type=int, default=3, help="timed calls per front-end figure (median)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lag_one_timing.jsonl"))
    args = ap.parse_args()

    import torch
    from track_estimators import batch
    from track_estimators._hip import binding

    db, hb = bench_batch(args.tracks)
    lib, B, N = db.lib, hb.B, hb.Nmax
    s = db._stream(None)
    f64 = dict(dtype=torch.float64, device=db.device)
    i32 = dict(dtype=torch.int32, device=db.device)
    out = {"label": args.label, "tracks": B, "rows": N + 1, "rounds": args.rounds, "whole_rounds": args.whole_rounds,
           "work_rows": "gains" if bool((db.rts_work[-1] < 0).all().item()) else "D"}

    # ---- the lag-one kernel against the sampler's coefficient kernel -------------------------------------------------------
    lag16, lag4 = torch.zeros((N, 16, B), **f64), torch.zeros((N, 4, B), **f64)
    status = torch.zeros((B,), **i32)
    lg16 = binding.SteLagOneF64(lag16.data_ptr(), status.data_ptr(), 0, 0)
    lg4 = binding.SteLagOneF64(lag4.data_ptr(), status.data_ptr(), binding.STE_LAG1_POSITION, 0)
    draws = torch.zeros((1, N + 1, 4, B), **f64)
    sm, sstatus, keep = db._sample_struct(draws, 1)

    def lag(lg):
        return lambda: binding.check(lib.ste_urtss_lag_one_f64(C.byref(db.struct), None, C.byref(lg), s), "ste_urtss_lag_one_f64")

    def prepare():
        binding.check(lib.ste_urtss_sample_prepare_f64(C.byref(db.struct), None, C.byref(sm), s), "ste_urtss_sample_prepare_f64")

    ms, samples = alternating({"full": lag(lg16), "position": lag(lg4), "prepare": prepare}, args.rounds)
    out["lag_ms"] = {"full": ms["full"], "position": ms["position"]}
    out["prepare_ms"] = ms["prepare"]
    out["samples_ms"] = {"lag " + k: v for k, v in samples.items()}
    out["lag_status_any"] = int(status.any().item())
    # bytes model, per (step, track): the work row in D form (8 of D; x_b and P_b of the quarter of the rows that store them are
    # left out), one filtered row (4 + 10, packed: lane k reads rows k and k + 1, so every row is wanted by two lanes and counted
    # once), 10 of sm_cov, and the entries written
    out["lag_model_bytes"] = {k: B * N * 8 * (8 + 14 + 10 + n) for k, n in (("full", 16), ("position", 4))}
    out["lag_gbs"] = {k: round(out["lag_model_bytes"][k] / (out["lag_ms"][k] * 1e-3) / 1e9, 1) for k in ("full", "position")}
    del draws, sm, keep

    # ---- the query kernel against positions with moments alone -------------------------------------------------------------
    gen = torch.Generator(device=db.device)
    gen.manual_seed(1)
    Q = B * args.per_ship
    span = db.t["dt"].sum(dim=0)  # close enough to the in-order sum to stay inside the track
    qtrack = torch.arange(B, **i32).repeat_interleave(args.per_ship)
    qtime = torch.rand((Q,), generator=gen, **f64) * 0.999 * span[qtrack.long()]
    qtime = qtime.view(B, args.per_ship).sort(dim=1).values.reshape(Q).contiguous()  # by (track, time)
    knots = db.track_knots()
    res = {"pcov": torch.empty((3, Q), **f64), "step": torch.empty((Q,), **i32), "frac": torch.empty((Q,), **f64),
           "status": torch.empty((Q,), **i32)}
    res10 = dict(res, pcov=torch.empty((10, Q), **f64))

    def pcov(outs, flags, lagt):
        pc = binding.StePositionCovF64()
        pc.flags, pc.nqueries, pc.qtrack, pc.qtime = flags, Q, qtrack.data_ptr(), qtime.data_ptr()
        pc.knots, pc.cov, pc.lag1 = knots.data_ptr(), db.struct.sm_cov, lagt.data_ptr()
        for k, ten in outs.items():
            setattr(pc, k, ten.data_ptr())
        return lambda: binding.check(lib.ste_track_position_cov_f64(C.byref(db.struct), C.byref(pc), s), "ste_track_position_cov_f64")

    sm_pos = {k: torch.empty((1, Q), **f64) for k in ("lon", "lat")}
    po = binding.StePositionsF64()
    po.nstates, po.flags, po.states = 1, binding.STE_POS_REUSE_KNOTS, db.sm_mean.data_ptr()
    po.nqueries, po.qtrack, po.qtime, po.knots = Q, qtrack.data_ptr(), qtime.data_ptr(), knots.data_ptr()
    po.lon, po.lat = sm_pos["lon"].data_ptr(), sm_pos["lat"].data_ptr()
    binding.check(lib.ste_track_positions_f64(C.byref(db.struct), C.byref(po), s), "ste_track_positions_f64")
    anchor = torch.stack([sm_pos["lon"][0], sm_pos["lat"][0]]).contiguous()
    acc = {"count": torch.zeros((Q,), **i32), "moments": torch.zeros((5, Q), **f64)}
    pm = binding.StePositionsF64()
    pm.nstates, pm.flags, pm.states = 1, binding.STE_POS_REUSE_KNOTS, db.sm_mean.data_ptr()
    pm.nqueries, pm.qtrack, pm.qtime, pm.knots = Q, qtrack.data_ptr(), qtime.data_ptr(), knots.data_ptr()
    pm.anchor, pm.count, pm.moments = anchor.data_ptr(), acc["count"].data_ptr(), acc["moments"].data_ptr()

    def moments():
        binding.check(lib.ste_track_positions_f64(C.byref(db.struct), C.byref(pm), s), "ste_track_positions_f64")

    P4 = binding.STE_PCOV_LAG1_POSITION
    ms, samples = alternating({"position": pcov(res, P4, lag4), "position_alone": pcov({"pcov": res["pcov"]}, P4, lag4),
                               "full": pcov(res10, binding.STE_PCOV_FULL, lag16), "moments": moments}, args.rounds)
    out["queries"] = Q
    out["located"] = int((res["step"] >= 0).sum().item())
    out["interior"] = int((res["frac"] > 0).sum().item())
    out["pcov_ms"] = {k: ms[k] for k in ("position", "position_alone", "full")}
    out["mom_ms"] = ms["moments"]
    out["samples_ms"].update({"query " + k: v for k, v in samples.items()})
    pcov(res, P4, lag4)()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    h.update(lag16.cpu().numpy().tobytes())
    h.update(res["pcov"].cpu().numpy().tobytes())
    out["checksum"] = h.hexdigest()
    del lag16, res10, acc

    # ---- the front ends, device to NumPy -------------------------------------------------------------------------------
    qt, tq = qtrack.cpu().numpy(), qtime.cpu().numpy()
    whole = {"position_covariance": lambda: batch.position_covariance(db, qt, tq),
             "position_statistics_16": lambda: batch.position_statistics(db, qt, tq, 16, chunk=16),
             "position_statistics_256": lambda: batch.position_statistics(db, qt, tq, 256, chunk=16)}
    ms, samples = alternating(whole, args.whole_rounds)
    out["whole_ms"] = ms
    out["samples_ms"].update({"whole " + k: v for k, v in samples.items()})
    out["what"] = ("HIP events on the current stream around each call, figures of a group alternating call by call, median of "
                   "rounds after one warm-up each")
    append_json(args.out, out)


if __name__ == "__main__":
    main()
