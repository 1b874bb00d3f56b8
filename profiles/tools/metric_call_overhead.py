#!/usr/bin/env python3
"""Host cost of seven metric methods of DeviceBatch on a window read in place (window(3, 70) of a fleet of 130 tracks, 6 steps,
S = 2: col = 3, so every per-track output and input goes through the column arithmetic): wall time per call in microseconds,
the median of five blocks of 100 calls that each end in a synchronise, after 20 warm-up calls, and a sha256 of everything the
calls returned (equal between two checkouts whose bits are equal).  At this size a call is host work and launch latency.  One
JSON line.  To compare two checkouts, run it alternately with each one's root (profiles/metric_columns_ab.md).

usage: profiles/tools/metric_call_overhead.py <root of the checkout to measure>"""
import hashlib
import json
import os
import sys
import time

tree = os.path.abspath(sys.argv[1])
sys.path[:0] = [tree, os.path.join(tree, "ship-track-estimators_amd"), os.path.join(tree, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from metrics_timing_common import bare_batch  # noqa: E402
from track_estimators import batch  # noqa: E402

assert os.path.abspath(batch.__file__).startswith(tree), batch.__file__
B, N, S, M = 130, 6, 2, 4
rng = np.random.default_rng(5)
dt = rng.uniform(0.05, 0.15, (N, B))
fleet = bare_batch(np.full(B, N), dt)
start = np.stack([rng.uniform(-10, 10, B), rng.uniform(40, 50, B)])
track = np.concatenate([start[None], start[None] + np.cumsum(rng.normal(0, 0.01, (N, 2, B)), axis=0)])
states = torch.zeros((S, N + 1, 4, B), dtype=torch.float64, device=fleet.device)
states[:, :, :2] = torch.from_numpy(track).to(fleet.device)
states[1, :, :2] += 0.001
lo, hi = 3, 70
win = fleet.window(lo, hi)
view = states[..., lo:hi]
sites = np.stack([rng.uniform(-10, 10, M), rng.uniform(40, 50, M)], axis=1)
lines = [np.array([[-10.0, 45.0], [0.0, 46.0], [10.0, 45.0]]), np.array([[0.0, 40.0], [0.5, 50.0]])]
tl = batch.track_lines(lines)
t0 = rng.uniform(0, 5, hi - lo)
thr = rng.uniform(5, 20, hi - lo)
calls = {
    "site_metrics": lambda: win.site_metrics(view, sites, 30.0, t0=t0),
    "line_metrics": lambda: win.line_metrics(view, tl, t0=t0),
    "speed_metrics": lambda: win.speed_metrics(view, bands=[0.0, 5.0, 10.0, 50.0], threshold=thr, per_step=True),
    "path_metrics": lambda: win.path_metrics(view, cumulative=True, line_axis="lat", line_value=45.0),
    "region_metrics": lambda: win.region_metrics(view, np.array([[-5.0, 42.0], [5.0, 42.0], [5.0, 48.0], [-5.0, 48.0]]), mask=True),
    "track_errors": lambda: win.track_errors(view, np.ascontiguousarray(track[:, :, lo:hi]) + 0.001, rows=True),
    "simplify_tracks": lambda: win.simplify_tracks(view, 0.5),
}
res = {"tree": sys.argv[1]}
h = hashlib.sha256()
for name, fn in calls.items():
    out = fn()
    for k in sorted(out):
        h.update(k.encode())
        h.update(np.ascontiguousarray(out[k].cpu().numpy()).tobytes())
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(100):
            fn()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t) / 100 * 1e6)
    res[name + "_us"] = round(float(np.median(blocks)), 1)
    res[name + "_us_blocks"] = [round(b, 1) for b in blocks]
res["checksum"] = h.hexdigest()
print(json.dumps(res))
