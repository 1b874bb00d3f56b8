#!/usr/bin/env python3
"""Alternating A/B of bench.py between builds of libste_hip.so on one box: one JSON line per run.

The library is chosen per process through STE_LIB_PATH (track_estimators/_hip/binding.py), so both builds run the same
Python, the same bench.py and the same batch.  Runs rotate parent, [further builds,] new, parent, ... for each of the two
commands, so that drift of the box (clock, neighbours) falls on all builds alike.

usage: profiles/tools/ab_bench_libs.py <parent libste_hip.so> <out.jsonl> [runs=5] [budget-seconds] [name=<libste_hip.so> ...]
(name=path: further builds, e.g. one item of a change on its own, timed between the parent and this tree's library)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
extra = [a for a in sys.argv[1:] if "=" in a]
pos = [a for a in sys.argv[1:] if "=" not in a]
parent_lib, out_path = pos[0], pos[1]
runs = int(pos[2]) if len(pos) > 2 else 5
t_end = time.time() + (float(pos[3]) if len(pos) > 3 else 1e9)
LIBS = {"parent": os.path.abspath(parent_lib)}
LIBS.update({a.split("=", 1)[0]: os.path.abspath(a.split("=", 1)[1]) for a in extra})
LIBS["new"] = os.path.join(ROOT, "ship-track-estimators_amd", "lib", "libste_hip.so")
CMDS = {"k100": ["--steps", "100", "--warmup", "10"], "driver": ["--gpus", "1", "--steps", "20", "--warmup", "5"]}
last = 60.0
for i in range(runs):
    for cmd in ("k100", "driver"):
        for build in LIBS:
            if time.time() + 1.5 * last > t_end:
                print("out of time before run", i, cmd, build, flush=True)
                sys.exit(0)
            t0 = time.time()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + CMDS[cmd], env=dict(os.environ, STE_LIB_PATH=LIBS[build]),
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
            last = time.time() - t0
            if r.returncode != 0:  # nothing more is started on the GPU after a failed run
                print("bench failed", build, cmd, r.returncode, r.stderr[-2000:], flush=True)
                sys.exit(1)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            keep = {k: res.get(k) for k in ("metric", "value", "unit", "ms_per_step", "steady_state")}
            with open(out_path, "a") as f:
                f.write(json.dumps({"build": build, "command": cmd, "args": " ".join(CMDS[cmd]), "run": i, "wall_s": round(last, 1), **keep}) + "\n")
            print(build, cmd, i, "ms_per_step %.4f" % keep["ms_per_step"], "steady", (keep["steady_state"] or {}).get("ms_per_step"),
                  "value %.4g" % keep["value"], "wall %.0f s" % last, flush=True)
