#!/usr/bin/env python3
"""Posterior covariance of a batch of GP tracks (ste_gp_predict_cov_f64: Kstar, W = Kstar K^-1, cov = Kss + s I - W Kstar^T
on the lower tiles), timed with HIP events after a warm-up.  K^-1 and alpha come from one ste_gp_lml_f64 before the
timed window; the window holds the predict_cov call only.  One JSON line per size; rates from the shapes:
W 2 m n^2 and the lower cov tiles m^2 n per track (unpadded sizes), against bench_gp.py's fp64 MFMA peak.

usage: tools/gp_posterior_timing.py [--sizes 1000x2000x500,250x2000x2000] [--calls 3] [--rounds 3] [--kernel rbf]
(sizes are tracks x observations x query points)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="1000x2000x500,250x2000x2000")
    ap.add_argument("--calls", type=int, default=3, help="predict_cov calls per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per size")
    ap.add_argument("--kernel", default="rbf", choices=["rbf", "matern12", "matern32", "matern52"])
    args = ap.parse_args()

    import torch
    from bench_gp import FP64_MFMA_PEAK_TFLOPS
    from track_estimators import synthetic
    from track_estimators._hip import binding
    from track_estimators.gaussian_processes.device import GpDeviceBatch

    kind = {"rbf": binding.STE_GP_KERNEL_RBF, "matern12": binding.STE_GP_KERNEL_MATERN12,
            "matern32": binding.STE_GP_KERNEL_MATERN32, "matern52": binding.STE_GP_KERNEL_MATERN52}[args.kernel]
    for size in args.sizes.split(","):
        B, n, m = (int(v) for v in size.split("x"))
        sb = synthetic.make_batch(B, nobs=n, gap_h=1.0, seed0=0)
        xs = [np.insert(np.cumsum(sb.dts[b]), 0, 0) for b in range(B)]
        ys = [np.column_stack([sb.lon[b], sb.lat[b]]) for b in range(B)]
        batch = GpDeviceBatch(xs, ys, kernel=kind)
        theta = np.tile(np.log([50.0, 20.0, 0.01]), (B, 1))
        _, _, status = batch.objective(theta, eval_gradient=False, keep_kinv=True)
        dev = dict(dtype=torch.float64, device=batch.device)
        qh = np.stack([np.linspace(x[0], x[-1], m) for x in xs])
        t_m = torch.full((B,), m, dtype=torch.int32, device=batch.device)
        t_xs = torch.from_numpy(qh).to(batch.device)
        ks = torch.empty((B, 64 * ((m + 63) // 64), batch.ld), **dev)
        w = torch.empty_like(ks)
        mean = torch.zeros((B, batch.nout, m), **dev)
        cov = torch.empty((B, m, m), **dev)
        s = batch._stream()

        def call():
            binding.check(batch.lib.ste_gp_predict_cov_f64(C.byref(batch.struct), m, t_m.data_ptr(), t_xs.data_ptr(),
                                                           ks.data_ptr(), w.data_ptr(), mean.data_ptr(), cov.data_ptr(), s),
                          "ste_gp_predict_cov_f64")

        call()  # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        samples = []
        for _ in range(args.rounds):
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) / args.calls)
        ms = float(np.median(samples))
        flops = B * (2.0 * m * n * n + float(m) * m * n)
        gflops = flops / (ms * 1e-3) / 1e9
        c = cov[0].cpu().numpy()
        print(json.dumps({"call": "ste_gp_predict_cov_f64", "kernel": args.kernel, "tracks": B, "nobs": n, "queries": m,
                          "ms_per_call": ms, "ms_samples": [round(v, 3) for v in samples],
                          "gflop": flops / 1e9, "gflop_per_s": gflops, "share_of_fp64_mfma_peak": gflops / 1e3 / FP64_MFMA_PEAK_TFLOPS,
                          "status_flagged": int((status != 0).sum()), "cov0_symmetric": bool(np.array_equal(c, c.T)),
                          "cov0_min_diag": float(np.diag(c).min()),
                          "what": "predict_cov alone (K^-1 from a preceding ste_gp_lml_f64), HIP events"}), flush=True)
        del call, batch, ks, w, mean, cov
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
