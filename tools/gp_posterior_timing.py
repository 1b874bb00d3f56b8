#!/usr/bin/env python3
"""Posterior covariance of a batch of GP tracks (ste_gp_predict_cov_f64: Kstar, W = Kstar K^-1, cov = Kss + s I - W Kstar^T
on the lower tiles), timed with HIP events after a warm-up.  K^-1 and alpha come from one ste_gp_lml_f64 before the
timed window; the window holds the predict_cov call only.  One JSON line per size; rates from the shapes:
W 2 m n^2 and the lower cov tiles m^2 n per track (unpadded sizes), against bench_gp.py's fp64 MFMA peak.

With --deriv the same process also times ste_gp_predict_f64 and the derivative calls (ste_gp_predict_deriv_f64,
ste_gp_predict_deriv_cov_f64) on the same K^-1, shapes and workspaces, the four calls' windows alternating round by round,
and prints one more JSON line per call plus the ratios derivative / position (ste_gp_predict_f64 is W reduced against
Kstar on the fly, 2 m n^2 per track).

usage: tools/gp_posterior_timing.py [--sizes 1000x2000x500,250x2000x2000] [--calls 3] [--rounds 3] [--kernel rbf] [--deriv]
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
    ap.add_argument("--deriv", action="store_true", help="also time ste_gp_predict_f64 and the derivative calls")
    args = ap.parse_args()
    if args.deriv and args.kernel == "matern12":
        sys.exit("Matern 1/2 has no derivative")

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

        calls = {"ste_gp_predict_cov_f64": call}
        if args.deriv:
            var = torch.zeros((B, m), **dev)
            dmean = torch.zeros((B, batch.nout, m), **dev)
            dvar = torch.zeros((B, m), **dev)
            dcov = torch.empty((B, m, m), **dev)
            sp = (C.byref(batch.struct), m, t_m.data_ptr(), t_xs.data_ptr(), ks.data_ptr())
            lib = batch.lib
            calls["ste_gp_predict_f64"] = lambda: binding.check(
                lib.ste_gp_predict_f64(*sp, mean.data_ptr(), var.data_ptr(), s), "ste_gp_predict_f64")
            calls["ste_gp_predict_deriv_f64"] = lambda: binding.check(
                lib.ste_gp_predict_deriv_f64(*sp, dmean.data_ptr(), dvar.data_ptr(), s), "ste_gp_predict_deriv_f64")
            calls["ste_gp_predict_deriv_cov_f64"] = lambda: binding.check(
                lib.ste_gp_predict_deriv_cov_f64(*sp, w.data_ptr(), dmean.data_ptr(), dcov.data_ptr(), s),
                "ste_gp_predict_deriv_cov_f64")
        for f in calls.values():
            f()  # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for name, f in calls.items():  # (alternating: every call sees the same drift of the machine)
                e0.record()
                for _ in range(args.calls):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.calls)
        samples = times["ste_gp_predict_cov_f64"]
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
        if args.deriv:
            med = {k: float(np.median(v)) for k, v in times.items()}
            for name in ("ste_gp_predict_f64", "ste_gp_predict_deriv_f64", "ste_gp_predict_deriv_cov_f64"):
                fl = B * (2.0 * m * n * n + (float(m) * m * n if "cov" in name else 0.0))
                print(json.dumps({"call": name, "kernel": args.kernel, "tracks": B, "nobs": n, "queries": m,
                                  "ms_per_call": med[name], "ms_samples": [round(v, 3) for v in times[name]],
                                  "gflop": fl / 1e9, "gflop_per_s": fl / (med[name] * 1e-3) / 1e9,
                                  "what": "same process, shapes and K^-1 as the predict_cov line, windows alternating"}),
                      flush=True)
            d = dcov[0].cpu().numpy()
            print(json.dumps({"ratio": "derivative / position", "kernel": args.kernel, "tracks": B, "nobs": n, "queries": m,
                              "deriv_over_predict": med["ste_gp_predict_deriv_f64"] / med["ste_gp_predict_f64"],
                              "deriv_cov_over_predict_cov": med["ste_gp_predict_deriv_cov_f64"] / med["ste_gp_predict_cov_f64"],
                              "dcov0_symmetric": bool(np.array_equal(d, d.T)), "dcov0_min_diag": float(np.diag(d).min())}),
                  flush=True)
            del var, dmean, dvar, dcov, calls
        del call, batch, ks, w, mean, cov
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
