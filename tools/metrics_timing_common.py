"""What the tools/*_metrics_timing.py scripts and tools/sample_tracks_timing.py share: the import path of the package, the
bench batch, the HIP-event timer, posterior tracks on the device and the JSON line.  Importing it puts the repository and the
package on sys.path."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ship-track-estimators_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

NOBS, SUBSTEPS = 126, 4  # bench.py: 125 gaps of 4 filter steps = 500 steps, 501 rows per track


def bench_batch(tracks, Q=None, smooth=True):
    """The bench batch of ``tracks`` ships on the device after ``run()`` (``smooth=False``: after ``forward()``), synchronised;
    ``Q`` replaces the example's process noise.  Returns (DeviceBatch, HostBatch)."""
    import torch
    from track_estimators import batch, synthetic

    H, Q0, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(tracks, nobs=NOBS, gap_h=1.0, seed0=0)
    hb = batch.pack_uniform(sb, SUBSTEPS, H, Q0 if Q is None else Q, R, P0)
    db = batch.DeviceBatch(hb)
    if smooth:
        db.run()
    else:
        db.forward()
    torch.cuda.synchronize()
    return db, hb


def bare_batch(nsteps, dt):
    """A DeviceBatch that holds nothing but ``nsteps`` (B,) and ``dt`` (Nmax, B), without histories: what a metric kernel reads
    of a batch when the tracks come from elsewhere."""
    from track_estimators import batch

    N, B = dt.shape
    z = np.zeros((N, B))
    hb = batch.HostBatch(B=B, Nmax=N, Tmax=1, H=np.eye(4), Q=np.eye(4), R=np.eye(4), nsteps=np.asarray(nsteps).astype(np.int32),
                         x0=np.zeros((4, B)), P0=np.eye(4).reshape(16), dt=dt, sog_rate=z, cog_rate=z.copy(), sog_rate_rts=None,
                         cog_rate_rts=None, upd_idx=np.full((N, B), -1, dtype=np.int32), z=np.zeros((1, 4, B)))
    return batch.DeviceBatch(hb, histories=False)


def timed(fn, rounds):
    """``fn()`` once to warm up, then ``rounds`` calls timed one by one with HIP events on the current stream.  Returns
    (the median in ms, every call's ms rounded to 3 places)."""
    import torch

    fn()  # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = []
    for _ in range(rounds):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1))
    return float(np.median(samples)), [round(v, 3) for v in samples]


def posterior_draws(db, S, seed=0, sample=True):
    """``S`` posterior tracks per ship of ``db`` on the device: standard normal draws (S, Nmax+1, 4, B) from a generator seeded
    with ``seed``, turned into tracks in place by ste_urtss_sample_f64.  ``sample=False`` leaves the draws as they are, for
    a caller that times the sampler's two stages itself.  Returns (tracks, sampler struct, status tensor, tensors the struct
    points to, the generator)."""
    import torch
    from track_estimators._hip import binding

    gen = torch.Generator(device=db.device)
    gen.manual_seed(seed)
    draws = torch.randn((S, int(db.struct.Nmax) + 1, 4, db.ntracks), generator=gen, dtype=torch.float64, device=db.device)
    sm, status, keep = db._sample_struct(draws, S)
    if sample:
        binding.check(db.lib.ste_urtss_sample_f64(C.byref(db.struct), None, C.byref(sm), db._stream(None)), "ste_urtss_sample_f64")
    return draws, sm, status, keep, gen


def append_json(path, record):
    """Print ``record`` as one JSON line and append it to ``path``, whose directory is made if it is missing."""
    line = json.dumps(record)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")
