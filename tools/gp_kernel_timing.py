#!/usr/bin/env python3
"""One batched GP objective (LML + gradient) per kernel function, timed with HIP events: BASELINE configs[4] size by
default (1 000 tracks x 2 000 observations, the data and theta of bench_gp.measure).  The kinds run in turn on the same
batch, round after round, so that all of them see the same device state; one JSON line per kind.

usage: tools/gp_kernel_timing.py [--tracks 1000] [--nobs 2000] [--evals 3] [--rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ship-track-estimators_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--nobs", type=int, default=2000)
    ap.add_argument("--evals", type=int, default=3, help="objectives per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per kind (kinds alternate)")
    args = ap.parse_args()

    import torch
    from track_estimators import synthetic
    from track_estimators._hip import binding
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    B, n = args.tracks, args.nobs
    sb = synthetic.make_batch(B, nobs=n, gap_h=1.0, seed0=0)
    xs = [np.insert(np.cumsum(sb.dts[b]), 0, 0) for b in range(B)]
    ys = [np.column_stack([sb.lon[b], sb.lat[b]]) for b in range(B)]
    batch = GpDeviceBatch(xs, ys)
    theta = np.tile(np.log([50.0, 20.0, 0.01]), (B, 1))
    kinds = {"rbf": binding.STE_GP_KERNEL_RBF, "matern12": binding.STE_GP_KERNEL_MATERN12,
             "matern32": binding.STE_GP_KERNEL_MATERN32, "matern52": binding.STE_GP_KERNEL_MATERN52}
    samples = {k: [] for k in kinds}
    flagged = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for name, kind in kinds.items():
            batch.kernel = batch.struct.kernel = kind  # (the 68 GB of buffers are shared; only the kernel function changes)
            batch.objective(theta)  # warm-up of this kind's kernels
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.evals):
                _, _, status = batch.objective(theta)
            e1.record()
            torch.cuda.synchronize()
            samples[name].append(e0.elapsed_time(e1) / args.evals)
            flagged[name] = int((status != 0).sum())
    for name in kinds:
        s = samples[name]
        print(json.dumps({"kernel": name, "tracks": B, "nobs": n, "ms_per_objective": float(np.median(s)),
                          "ms_samples": [round(v, 3) for v in s], "status_flagged": flagged[name],
                          "what": "LML + gradient, one batched launch sequence (HIP events)"}), flush=True)


if __name__ == "__main__":
    main()
