"""Round 5: the forward passes of many batches (or windows of a fleet) as ONE scheduled launch of resident waves over
(64-track tile, time slice) items -- include/ste.h 0.3.2 ``ste_ukf_forward_sched_f64``, ``batch.forward_schedule``,
``SmootherPipeline.submit_sequence``.  The reference's batch dimension is its per-ship loop
(/root/reference/examples/example_ukf_rts_smoother_batch.py:19-90); like windows and time slices, a schedule only moves
launch boundaries: every result is the per-batch launch's, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from track_estimators import batch, synthetic
from track_estimators._hip import binding


def _check_schedule(items, ntiles, nslices):
    """Every tile of every window runs exactly its slices, at most one per round; returns the completion round per window."""
    seen = {}
    done = np.zeros(len(ntiles), dtype=int)
    for r in range(items.shape[0]):
        this = set()
        for w, t in items[r]:
            if w < 0:
                continue
            assert 0 <= w < len(ntiles) and 0 <= t < ntiles[w]
            assert (w, t) not in this  # one slice of a tile per round
            this.add((w, t))
            seen[(w, t)] = seen.get((w, t), 0) + 1
            done[w] = r + 1
    assert len(seen) == sum(ntiles)
    for (w, t), c in seen.items():
        assert c == nslices[w], (w, t, c)
    return done


@pytest.mark.parametrize("ntiles,nslices,nwaves", [([157] * 20, [8] * 20, 1024), ([224] * 7, [8] * 7, 1024), ([3, 1, 7], [2, 9, 1], 4),
                                                    ([5], [4], 64), ([40, 40], [3, 5], 16)])
def test_forward_schedule_runs_every_slice_once_and_reaches_the_bound(ntiles, nslices, nwaves):
    items = batch.forward_schedule(ntiles, nslices, nwaves)
    done = _check_schedule(items, ntiles, nslices)
    total = sum(a * b for a, b in zip(ntiles, nslices))
    # McNaughton's bound for chains of unit jobs: total work over the waves, and no shorter than the longest chain
    assert items.shape[0] == max(-(-total // nwaves), max(nslices))
    if len(set(nslices)) == 1:
        assert (np.diff(done) >= 0).all()  # equal windows finish in order
    # a tile that keeps running stays on its wave
    moves = 0
    for r in range(1, items.shape[0]):
        prev = {tuple(v): i for i, v in enumerate(items[r - 1]) if v[0] >= 0}
        for i, v in enumerate(items[r]):
            if v[0] >= 0 and tuple(v) in prev and prev[tuple(v)] != i:
                moves += 1
    assert moves == 0


def test_forward_schedule_with_staggered_deadlines_is_still_complete():
    ntiles, nslices = [157] * 20, [8] * 20
    items = batch.forward_schedule(ntiles, nslices, 1024, stagger=1.0)
    done = _check_schedule(items, ntiles, nslices)
    assert len(set(done.tolist())) > 6  # the windows finish spread out, not in generations


def _rolled(ntiles, nslices, nwaves):
    """A table whose rounds are rotated, every round by another amount (the hand-over test's): tiles change waves, rounds stay."""
    items = batch.forward_schedule(ntiles, nslices, nwaves).copy()
    for r in range(items.shape[0]):
        items[r] = np.roll(items[r], 131 * (r + 1), axis=0)
    return items


_ORDER_3_1_7 = [[0, 0], [0, 1], [0, 2], [2, 0], [2, 1], [2, 2], [2, 3], [2, 4], [2, 5], [2, 6], [1, 0]]


@pytest.mark.parametrize("ntiles,nslices,nwaves,table,expected", [
    ([3, 1, 7], [2, 9, 1], 4, batch.forward_schedule, _ORDER_3_1_7), ([2, 2], [2, 2], 4, batch.forward_schedule, None),
    ([1], [1], 1024, batch.forward_schedule, None), ([94] * 3, [5] * 3, 1024, _rolled, None),
    ([157] * 20, [8] * 20, 1024, batch.forward_schedule, None)])
def test_smoother_tile_order_lists_every_tile_once_in_finishing_order(ntiles, nslices, nwaves, table, expected):
    """``batch.smoother_tile_order``: the tiles of a schedule sorted by the last round in which they appear, stably.  The
    literal is what ``submit_sequence`` computed inline before the function existed."""
    items = table(ntiles, nslices, nwaves)
    order = batch.smoother_tile_order(items, ntiles)
    assert order.dtype == np.int32 and order.flags.c_contiguous and order.shape == (sum(ntiles), 2)
    assert sorted(map(tuple, order.tolist())) == [(w, t) for w, n in enumerate(ntiles) for t in range(n)]  # each pair once
    last = {}
    for r in range(items.shape[0]):
        for w, t in items[r][items[r][:, 0] >= 0].tolist():
            last[(w, t)] = r
    tile0 = np.concatenate(([0], np.cumsum(ntiles)))
    keys = [(last[(w, t)], int(tile0[w]) + t) for w, t in order.tolist()]  # (last round, flat tile index)
    assert all(a[0] <= b[0] for a, b in zip(keys, keys[1:]))  # the last round never decreases
    assert all(a[1] < b[1] for a, b in zip(keys, keys[1:]) if a[0] == b[0])  # ties: ascending flat tile order (stable sort)
    if expected is not None:
        assert np.array_equal(order, np.array(expected, dtype=np.int32))


def _minimal_windows(n, B=128, Nmax=128, keep=None):
    arr = (binding.SteUkfBatchF64 * n)()
    m = np.eye(4)
    r = np.diag([0.25, 0.25, 0.0, 0.0])
    h = np.diag([1.0, 1.0, 0.0, 0.0])
    keep.extend([m, r, h])
    for s in arr:
        s.B, s.Nmax, s.Tmax, s.n = B, Nmax, 4, 4
        s.w0, s.wi, s.fan_scale = -1.0 / 3.0, 1.0 / 6.0, 3.0
        s.H, s.Q, s.R = h.ctypes.data, m.ctypes.data, r.ctypes.data
        for name in ("x0", "P0", "dt", "sog_rate", "cog_rate", "upd_idx", "z", "fwd_mean", "fwd_cov", "status"):
            setattr(s, name, 0x1000)
    return arr


def test_schedule_validation_refuses_tables_that_could_not_progress():
    """include/ste.h 0.3.2: the item table is checked on the host before anything is launched -- a tile short of a slice,
    scheduled twice in a round, or outside its window is an argument error (no GPU needed: the device is looked at last)."""
    lib, keep = binding.load(), []
    wins = _minimal_windows(2, keep=keep)  # 2 windows x 2 tiles x 2 slices
    ws = np.zeros(1 << 16, dtype=np.uint8)

    def call(items, nwaves, **kw):
        items = np.ascontiguousarray(items, dtype=np.int32)
        sc = binding.SteFwdSchedF64()
        sc.nwindows, sc.windows, sc.slice_steps = 2, C.addressof(wins), kw.get("slice_steps", 64)
        sc.nwaves, sc.nrounds, sc.items = nwaves, items.shape[0], items.ctypes.data
        sc.host_ws, sc.dev_ws, sc.ws_bytes = ws.ctypes.data, 0x1000, kw.get("ws_bytes", ws.nbytes)
        sc.window_done, sc.error = 0x1000, 0x1000
        rc = lib.ste_ukf_forward_sched_f64(C.byref(sc), None)
        return rc, lib.ste_last_error().decode()

    good = batch.forward_schedule([2, 2], [2, 2], 4)
    assert good.shape == (2, 4, 2)
    rc, msg = call(good, 4)
    assert (rc, msg) == (-3, "no HIP device") or rc == 0 or "nwaves exceeds" in msg  # valid table: only the device can object
    bad = good.copy()
    bad[1, 0] = (-1, 0)
    assert "missing slices" in call(bad, 4)[1]
    bad = good.copy()
    bad[0, 0] = bad[0, 1]
    rc, msg = call(bad, 4)
    assert rc == -1 and ("same round" in msg)
    bad = good.copy()
    bad[0, 0] = (1, 2)
    assert "outside its window" in call(bad, 4)[1]
    bad = good.copy()
    bad[0, 0] = (2, 0)
    assert "does not exist" in call(bad, 4)[1]
    three = np.concatenate([good, good[:1]])
    assert "more slices than it has" in call(three, 4)[1]
    assert "workspace too small" in call(good, 4, ws_bytes=64)[1]
    assert "multiple of STE_SLICE_ALIGN" in call(good, 4, slice_steps=96)[1]
    wins[1].rts_work = 0x1000  # one window leaves smoother rows, the other does not: two different kernels
    assert "must agree" in call(good, 4)[1]
    assert lib.ste_ukf_forward_sched_workspace(2, 2, 4, 2, 4) >= 4 * 64 + 8 * 16 + 16


def _align16(v):
    return (v + 15) & ~15


def test_scheduled_workspace_has_one_layout_for_windows_of_unequal_slice_counts():
    """include/ste.h: the launch lays its workspace out by the five numbers of ste_ukf_forward_sched_workspace -- room for
    max_slices (max_slices + 1) / 2 parameter blocks for EVERY window -- so that its per-tile counters sit at
    ste_ukf_forward_sched_progress_offset of the same numbers, where the tile smoothers look, for any mix of window lengths.
    Windows of 1, 2 and 3 slices need 1 + 3 + 6 = 10 blocks, the documented size holds 3 x 6 = 18: a library that sizes the
    launch by the 10 takes a workspace 16 bytes short of the documented size and keeps its counters 8 blocks in front of the
    documented offset.  No GPU needed and none reached: the table is also a slice short, which every build refuses on the host."""
    import types

    lib, keep = binding.load(), []
    wins = _minimal_windows(3, keep=keep)  # 3 windows x 2 tiles
    for w, nmax in zip(wins, (16, 68, 132)):
        w.Nmax = nmax
    ws = np.zeros(1 << 16, dtype=np.uint8)
    ntiles, nslices, nwaves = [2, 2, 2], [1, 2, 3], 4
    items = batch.forward_schedule(ntiles, nslices, nwaves).copy()
    _check_schedule(items, ntiles, nslices)
    last = np.argwhere(items[..., 0] == 2)[-1]
    items[last[0], last[1]] = (-1, 0)  # a tile of the longest window loses its last slice: never a launch, on any build
    items = np.ascontiguousarray(items, dtype=np.int32)
    total = lib.ste_ukf_forward_sched_workspace(3, 3, sum(ntiles), items.shape[0], nwaves)
    kparams = lib.ste_ukf_forward_sched_workspace(16, 1, 0, 0, 0) // 16  # bytes of a parameter block (16 of them: no rounding)
    assert lib.ste_ukf_forward_sched_workspace(1, 1, 0, 0, 0) == _align16(kparams)
    assert total == _align16(18 * kparams) + _align16(16 * items.shape[0] * nwaves) + _align16(4 * sum(ntiles))
    assert total <= ws.nbytes

    def call(ws_bytes):
        sc = binding.SteFwdSchedF64()
        sc.nwindows, sc.windows, sc.slice_steps = 3, C.addressof(wins), 64
        sc.nwaves, sc.nrounds, sc.items = nwaves, items.shape[0], items.ctypes.data
        sc.host_ws, sc.dev_ws, sc.ws_bytes = ws.ctypes.data, 0x1000, ws_bytes
        sc.window_done, sc.error = 0x1000, 0x1000
        rc = lib.ste_ukf_forward_sched_f64(C.byref(sc), None)
        return rc, lib.ste_last_error().decode()

    rc, msg = call(total)
    assert rc == -1 and "missing slices" in msg  # the documented size is enough; the table is what is wrong
    rc, msg = call(total - 16)
    assert rc == -1 and "workspace too small" in msg, msg  # ... and anything below it is refused, before the table is read

    # the offset: the workspace less the counters, and behind everything the launch uploads
    def off(*a):
        return lib.ste_ukf_forward_sched_progress_offset(*a)

    for nw, ms, nt, nr, nv in [(3, 3, 8, 3, 1024), (3, 3, 6, 3, 4), (2, 3, 130, 3, 1024), (2, 2, 132, 3, 128), (1, 1, 1, 1, 1),
                               (5, 255, 1000, 40, 64), (20, 8, 3140, 25, 1024)]:
        o = off(nw, ms, nt, nr, nv)
        assert o % 16 == 0 and o + _align16(4 * nt) == lib.ste_ukf_forward_sched_workspace(nw, ms, nt, nr, nv)
        assert o == _align16(nw * (ms * (ms + 1) // 2) * kparams) + _align16(16 * nr * nv)  # blocks by the bound, 16 bytes an item
        assert off(nw + 1, ms, nt, nr, nv) > o and off(nw, ms + 1, nt, nr, nv) > o
        assert off(nw, ms, nt, nr + 1, nv) > o and off(nw, ms, nt, nr, nv + 1) > o
        assert off(nw, ms, nt + 1000, nr, nv) == o  # the counters are last: their number moves nothing in front of them
    # the Python side hands the library the same five numbers (SmootherPipeline._plan on the windows above)
    fake = types.SimpleNamespace(forward_cus=1, reserve_cus=0, _schedules={})
    plan = batch.SmootherPipeline._plan(fake, wins, 64, 0.0)
    assert (plan.ntiles, plan.nslices, plan.nwaves) == (ntiles, nslices, nwaves)
    assert plan.table_shape() == (3, 3, 6, plan.items.shape[0], 4) and plan.items.shape[0] == 3
    plan = batch.SmootherPipeline._plan(fake, wins, 128, 0.0)
    assert plan.nslices == [1, 1, 2] and plan.table_shape() == (3, 2, 6, plan.items.shape[0], 4)


def test_scheduled_smoother_validation():
    """include/ste.h (STE_VERSION 321): ste_urtss_backward_sched_f64 checks windows and tile list before it launches anything
    (no GPU needed): every window must take the one-kernel smoother, every tile appears once."""
    lib, keep = binding.load(), []
    wins = _minimal_windows(2, B=4224, keep=keep)  # 2 windows x 66 tiles, above the two-kernel smoother's bound
    for w in wins:
        w.rts_work = w.sm_mean = w.sm_cov = 0x1000
    ws = np.zeros(1 << 16, dtype=np.uint8)
    tiles = np.array([(w, t) for w in range(2) for t in range(66)], dtype=np.int32)

    def call(items, **kw):
        items = np.ascontiguousarray(items, dtype=np.int32)
        sc = binding.SteBwdSchedF64()
        sc.nwindows, sc.windows, sc.slice_steps = 2, C.addressof(wins), kw.get("slice_steps", 64)
        sc.nitems, sc.items = items.shape[0], items.ctypes.data
        sc.host_ws, sc.dev_ws, sc.ws_bytes = ws.ctypes.data, 0x1000, kw.get("ws_bytes", ws.nbytes)
        sc.progress, sc.error = 0x1000, 0x1000
        rc = lib.ste_urtss_backward_sched_f64(C.byref(sc), None)
        return rc, lib.ste_last_error().decode()

    assert lib.ste_urtss_backward_sched_workspace(2, 132) <= ws.nbytes
    assert "every tile of every window once" in call(tiles[:-1])[1]
    bad = tiles.copy()
    bad[5] = bad[4]
    assert "appears twice" in call(bad)[1]
    bad = tiles.copy()
    bad[5] = (1, 66)
    assert "does not exist" in call(bad)[1]
    assert "workspace too small" in call(tiles, ws_bytes=64)[1]
    assert "multiple of STE_SLICE_ALIGN" in call(tiles, slice_steps=96)[1]
    wins[1].sog_rate_rts = 0x1000  # one window smooths with rates of its own, the other does not: two kernels
    assert "must agree on smoother rates" in call(tiles)[1]
    wins[1].sog_rate_rts = 0
    wins[1].B = 4096  # the two-kernel smoother's territory: other bits
    small = np.array([(0, t) for t in range(66)] + [(1, t) for t in range(64)], dtype=np.int32)
    assert "one-kernel smoother" in call(small)[1]
    # where the forward launch keeps its per-tile counters: behind its parameter blocks and its item table
    # (and nothing behind them: the workspace ends with one int32 per tile, rounded up to 16 bytes)
    off = lib.ste_ukf_forward_sched_progress_offset(2, 2, 132, 3, 128)
    assert off > 0 and off % 16 == 0 and off + _align16(4 * 132) == lib.ste_ukf_forward_sched_workspace(2, 2, 132, 3, 128)


def _uniform(B, seed0, nobs=33, substeps=4):
    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(B, nobs=nobs, gap_h=1.0, seed0=seed0)
    return sb, batch.pack_uniform(sb, substeps, H, Q, R, P0)


_OUT = ("fwd_mean", "fwd_cov", "sm_mean", "sm_cov", "status", "rts_work")


def _clear(db):
    """Histories and work rows are torch.empty: rows past a short track's end, and the parts of a work row a step does not
    need, are never written -- zero them so that two buffer sets can be compared whole."""
    for n in _OUT:
        getattr(db, n).zero_()
    return db


def _same(a, b):
    import torch

    for n in _OUT:
        x, y = getattr(a, n), getattr(b, n)
        if not torch.equal(torch.nan_to_num(x.double(), nan=1.25e300), torch.nan_to_num(y.double(), nan=1.25e300)):  # NaN is NaN
            return False
    return True


@pytest.mark.gpu
def test_sequence_of_batches_is_the_per_batch_launches_bit_for_bit():
    """Five batches of different sizes and lengths (tiles that do not fill a wave, 1 to 5 time slices) as one scheduled
    launch: histories, smoother work rows and status are those of DeviceBatch.run() on each."""
    import torch

    cases = [(700, 40, 4), (64, 9, 2), (1030, 81, 4), (130, 17, 1), (257, 33, 2)]  # (tracks, observations, sub-steps)
    refs, seqs = [], []
    for i, (B, nobs, sub) in enumerate(cases):
        _, hb = _uniform(B, 777_000 + 5000 * i, nobs=nobs, substeps=sub)
        hb.lanes = 1
        r = _clear(batch.DeviceBatch(hb))
        r.run()
        refs.append(r)
        seqs.append(_clear(batch.DeviceBatch(hb)))
    torch.cuda.synchronize()
    with batch.SmootherPipeline(ntracks=1030) as pipe:
        for stagger in (0.0, 1.0):
            for d in seqs:
                _clear(d)
            pipe.submit_sequence(seqs, stagger=stagger)
            pipe.synchronize()
            for r, d in zip(refs, seqs):
                assert _same(r, d), stagger
        # forward only, and a second use of the same buffer sets behind the first (events, not a device-wide wait)
        for d in seqs:
            _clear(d)
        pipe.submit_sequence(seqs, smooth=False)
        pipe.submit_sequence(seqs)
        pipe.synchronize()
        for r, d in zip(refs, seqs):
            assert _same(r, d)
        with pytest.raises(ValueError, match="histories of its own"):
            pipe.submit_sequence([seqs[0], seqs[0]])
        # workspaces of retired launches are kept and reused: the launches above were never more than two at a time
        assert 1 <= len(pipe._sched_free.free) <= 2 and not pipe._sched_live
        kept = {host_ws.data_ptr() for host_ws, _dev_ws, _counters in pipe._sched_free.free}
        for d in seqs:
            _clear(d)
        pipe.submit_sequence(seqs)
        assert pipe._sched_live[-1].host_ws.data_ptr() in kept
        pipe.synchronize()
        for r, d in zip(refs, seqs):
            assert _same(r, d)
        # a pageable host workspace (what a caller of the C ABI without page-locked memory hands over) takes the staged copy
        # instead of the upload kernel: same table, same bits
        pipe._sched_free.free, pipe._sched_pinned = [], False
        for d in seqs:
            _clear(d)
        pipe.submit_sequence(seqs)
        assert not pipe._sched_live[-1].host_ws.is_pinned()
        pipe.synchronize()
        for r, d in zip(refs, seqs):
            assert _same(r, d)


@pytest.mark.gpu
def test_scheduled_fleet_with_clamped_priors_and_recorded_noise_is_bit_identical():
    """A resident ragged fleet whose priors are indefinite (every square root clamped: the first-bad-step word, which a later
    slice reads back and which carries the slice's absolute offset) and that replays recorded noise, in windows through one
    scheduled launch: the bits of the one-launch run, and of run_fleet without a schedule."""
    import torch

    H, Q, R, P0 = synthetic.example_matrices()
    rng = np.random.default_rng(5)
    sb = synthetic.make_batch(900, nobs=60, gap_h=1.0, seed0=31_000)
    import types

    tr, dts = [], []
    for i in range(900):
        T = int(rng.integers(3, 61))
        tr.append(types.SimpleNamespace(z=sb.z[i][:, :T], dts=sb.dts[i][: T - 1], sog_rate=sb.sog_rate[i][:T], cog_rate=sb.cog_rate[i][:T]))
        dts.append(np.repeat(sb.dts[i][: T - 1] / 4, 4))
    Pbad = np.diag([1.0, 1.0, -0.5, 1.0])
    hb = batch.pack_tracks(tr, dts, [t.z[:, 0] for t in tr], H, Q, R, Pbad)
    N = hb.Nmax
    hb.noise_pred = rng.normal(0, 1e-3, (N, 4, hb.B))
    hb.noise_upd = rng.normal(0, 1e-3, (N + 1, 4, hb.B))
    hb.noise_rts = rng.normal(0, 1e-3, (N, 4, hb.B))
    hb.lanes = 1
    ref = _clear(batch.DeviceBatch(hb))
    ref.run()
    torch.cuda.synchronize()
    assert (ref.status_host() & binding.STE_STATUS_CLAMPED).all()
    db = _clear(batch.DeviceBatch(hb))
    res = batch.run_fleet(db, chunk=256, scheduled=True)
    assert len(batch.fleet_windows(hb.B, 256)) == 4 and _same(ref, db)
    db2 = _clear(batch.DeviceBatch(hb))
    batch.run_fleet(db2, chunk=256, scheduled=False)  # one forward launch per window
    assert _same(db, db2) and np.array_equal(res["status"], ref.status_host())


@pytest.mark.gpu
def test_slices_that_change_waves_every_round_hand_over_bit_for_bit():
    """The list scheduler keeps a running tile on its wave, so the in-kernel hand-over between waves (release of the history
    row, work rows, status and first-bad word at agent scope; acquire by the next slice -- possibly on another XCD) is
    exercised only by pre-empted tiles.  Here the table is rotated by a different amount every round: EVERY slice of every
    tile runs on another wave than the one before it, twenty times over, and the results must stay those of plain launches."""
    import torch

    _, hb = _uniform(6000, 4_100_000, nobs=81, substeps=4)  # 94 tiles x 5 slices per batch
    hb.lanes = 1
    ref = _clear(batch.DeviceBatch(hb))
    ref.run()
    torch.cuda.synchronize()
    seqs = [_clear(batch.DeviceBatch(hb)) for _ in range(3)]
    with batch.SmootherPipeline(ntracks=6000) as pipe:
        ntiles, nslices = [94] * 3, [5] * 3
        nwaves = 4 * (pipe.forward_cus - pipe.reserve_cus)
        items = batch.forward_schedule(ntiles, nslices, nwaves).copy()
        for r in range(items.shape[0]):
            items[r] = np.roll(items[r], 131 * (r + 1), axis=0)  # 131 waves = 32 compute units and a bit: another XCD, usually
        moved = 0
        for r in range(1, items.shape[0]):
            prev = {tuple(v): i for i, v in enumerate(items[r - 1]) if v[0] >= 0}
            moved += sum(1 for i, v in enumerate(items[r]) if v[0] >= 0 and prev.get(tuple(v), i) != i)
        assert moved >= 3 * 94 * 4  # every hand-over crosses waves
        pipe._schedules[(tuple(ntiles), tuple(nslices), nwaves, 0.0)] = np.ascontiguousarray(items)
        for rep in range(20):
            for d in seqs:
                _clear(d)
            # batches of 6 000 tracks, nothing in flight: the smoothers are ONE launch, a wave per tile waiting for its own
            # tile's last slice (every other repetition: a gate and a smoother launch per batch) -- same bits
            pipe.submit_sequence(seqs, tile_smoothers=None if rep % 2 == 0 else False)
            assert (pipe._sched_live[-1].smoother is not None) == (rep % 2 == 0)
            pipe.synchronize()
            for d in seqs:
                assert _same(ref, d), rep


@pytest.mark.gpu
def test_tile_smoothers_with_smoother_rates_of_their_own_are_the_per_batch_smoother_bit_for_bit():
    """The one-launch smoother of a sequence (ste_urtss_backward_sched_f64) for a window that smooths with rates of its own
    (sog_rate_rts / cog_rate_rts: the kShift instantiation of urtss_recur_sched, which no other test launches).  130 ragged
    tracks -- two full tiles and a partial one -- of up to 68 steps, so that every tile crosses a slice boundary; the
    one-kernel smoother forced by its tuning bit.  Histories, smoothed histories, work rows and status are those of
    DeviceBatch.run(), whose smoother is urtss_recur_l1<kShift> (tests/test_round3.py, tests/test_fleet.py)."""
    import dataclasses

    import torch

    _, hb = _uniform(130, 620_000, nobs=18, substeps=4)
    assert hb.Nmax == 68
    nsteps = (hb.Nmax - (np.arange(hb.B) * 7) % 40).astype(np.int32)
    hb = dataclasses.replace(hb, nsteps=nsteps, lanes=1, sog_rate_rts=hb.sog_rate * 1.25 + 0.01,
                             cog_rate_rts=hb.cog_rate * 0.75 - 0.02)
    ref = _clear(batch.DeviceBatch(hb, tuning=binding.STE_TUNING_ONE_KERNEL_SMOOTHER))
    ref.run()
    db = _clear(batch.DeviceBatch(hb, tuning=binding.STE_TUNING_ONE_KERNEL_SMOOTHER))
    assert db.struct.sog_rate_rts and db.struct.cog_rate_rts
    torch.cuda.synchronize()
    with batch.SmootherPipeline(ntracks=130) as pipe:
        pipe.submit_sequence([db], tile_smoothers=True)
        assert pipe._sched_live[-1].smoother is not None  # one smoother launch, a wave per tile
        pipe.synchronize()
    assert bool(ref.sm_mean.abs().sum() > 0) and _same(ref, db)


@pytest.mark.gpu
def test_scheduled_launches_of_two_pipelines_become_resident_one_at_a_time():
    """Every wave of a scheduled launch may wait for any other, so two launches dispatched together could each hold part of
    the chip.  The launch counts its waves as they begin (``started``, include/ste.h) and the next scheduled launch of the
    process -- here: of another pipeline, with nothing else ordering the two -- waits on its stream for all of them."""
    import torch

    cases = [(9000, 33, 4, 31), (7000, 33, 4, 57)]
    refs, seqs = [], []
    for B, nobs, sub, seed in cases:
        _, hb = _uniform(B, 9_000_000 + seed, nobs=nobs, substeps=sub)
        hb.lanes = 1
        r = _clear(batch.DeviceBatch(hb))
        r.run()
        refs.append(r)
        seqs.append([_clear(batch.DeviceBatch(hb)) for _ in range(8)])  # 8 x 141 / 8 x 110 tiles: more than a chip-full each
    torch.cuda.synchronize()
    # (sequence_only: one forward stream each -- two full pipelines would hold 28 of the device's ~24 hardware queues)
    with batch.SmootherPipeline(ntracks=9000, sequence_only=True) as pa, batch.SmootherPipeline(ntracks=7000, sequence_only=True) as pb:
        nwaves = 4 * (pa.forward_cus - pa.reserve_cus)
        for rep in range(3):
            for group in seqs:
                for d in group:
                    _clear(d)
            pa.submit_sequence(seqs[0])
            first = pa._sched_live[-1]
            pb.submit_sequence(seqs[1])
            # the second launch holds the first one's counters -- its gate reads them -- unless the first had already finished
            # when the second was submitted (a host that was held up for milliseconds between the two calls)
            assert pb._sched_live[-1].prev_counters is first.counters_all or first.ready.query()
            pb.submit_sequence(seqs[1][:3] + seqs[0][:0], smooth=False)  # (and a third behind the second, same pipeline)
            pa.synchronize()
            pb.synchronize()
            assert int(first.counters_all[len(seqs[0]) + 1].item()) == nwaves  # every wave of the launch counted itself in
            for r, group in zip(refs, seqs):
                for d in group:
                    assert _same(r, d), rep


@pytest.mark.gpu
def test_pipeline_shrinks_to_the_streams_scheduled_launches_need():
    """SmootherPipeline.shrink hands hardware queues back without building new ones (bench.py --sequence auto goes from the
    7 + 6 + 1 streams of per-step launches to 2 + 6 + 1 and 1 + 1 + 1 that way): same results on what is left."""
    import torch

    _, hb = _uniform(5000, 6_600_000, nobs=33, substeps=4)  # above the two-kernel smoother's bound: tile smoothers apply
    hb.lanes = 1
    ref = _clear(batch.DeviceBatch(hb))
    ref.run()
    torch.cuda.synchronize()
    seqs = [_clear(batch.DeviceBatch(hb)) for _ in range(4)]
    with batch.SmootherPipeline(ntracks=5000) as pipe:
        nf, nb = len(pipe.fwd_streams), len(pipe.bwd_streams)
        assert nf > 2 and nb > 1
        for i, d in enumerate(seqs):
            pipe.submit(d, final=(i == len(seqs) - 1))
        pipe.synchronize()
        assert all(_same(ref, d) for d in seqs)
        pipe.shrink(2, nb)
        assert (len(pipe.fwd_streams), len(pipe.bwd_streams), pipe.buffers_needed) == (2, nb, nb + 3) and len(pipe._raw) == nb + 2
        for d in seqs:
            _clear(d)
        pipe.submit_sequence(seqs[:2], final=False)
        pipe.submit_sequence(seqs[2:])
        pipe.synchronize()
        assert all(_same(ref, d) for d in seqs)
        pipe.shrink(1, 1)
        assert (len(pipe.fwd_streams), len(pipe.bwd_streams), pipe.buffers_needed) == (1, 1, 3) and len(pipe._raw) == 2
        for d in seqs:
            _clear(d)
        pipe.submit_sequence(seqs)
        assert pipe._sched_live[-1].smoother is not None  # one smoother launch, a wave per tile
        pipe.synchronize()
        assert all(_same(ref, d) for d in seqs)
        with pytest.raises(ValueError):
            pipe.shrink(0, 1)


# ---- windows with UNEQUAL slice counts through the one-launch ("tile") smoothers ----------------------------------------------
# The forward launch keeps a slice counter per tile in its workspace and the tile smoothers are handed their address:
# dev_ws + ste_ukf_forward_sched_progress_offset(the five numbers the workspace was sized by).  Windows of 16, 68 and 132 steps
# are 1, 2 and 3 slices of 64: 1 + 3 + 6 parameter blocks where the documented size holds 3 x 6, so a launch that lays its
# workspace out by what its windows need keeps its counters 8 blocks in front of the documented offset.  Every test below
# compares the bits with DeviceBatch.run() on each batch AND reads the counters back at the documented offset: each tile's
# must hold its window's slice count (what the tile's last run published), whatever stale memory let through or did not.
_UNEQUAL = ((130, 9, 2), (64, 18, 4), (200, 34, 4))  # (tracks, observations, sub-steps): 3 / 1 / 4 tiles, Nmax 16 / 68 / 132
_DEFAULT_PATH = ((4160, 18, 4), (4160, 34, 4))  # above the two-kernel smoother's bound: 65 tiles each, Nmax 68 / 132
_unequal_refs = {}


def _unequal_ref(case, ragged, tuning):
    """(host batch, its DeviceBatch.run()) for one (tracks, observations, sub-steps) case: computed once, never touched again."""
    import dataclasses

    import torch

    key = (case, ragged, tuning)
    if key not in _unequal_refs:
        B, nobs, sub = case
        _, hb = _uniform(B, 2_300_000 + 7000 * nobs, nobs=nobs, substeps=sub)
        assert hb.Nmax == (nobs - 1) * sub
        if ragged:  # tiles end slices early, the window's slice count (from Nmax) stays
            hb = dataclasses.replace(hb, nsteps=np.maximum(1, hb.Nmax - (np.arange(hb.B) * 7) % 40).astype(np.int32))
        hb = dataclasses.replace(hb, lanes=1)
        ref = _clear(batch.DeviceBatch(hb, tuning=tuning))
        ref.run()
        torch.cuda.synchronize()
        assert bool(ref.sm_mean.abs().sum() > 0)  # smoothed (and no NaN in it): zeros on both sides would compare equal
        _unequal_refs[key] = (hb, ref)
    return _unequal_refs[key]


def _unequal_sequence(order, cases=_UNEQUAL, ragged=False, tuning=binding.STE_TUNING_ONE_KERNEL_SMOOTHER):
    """References and fresh buffer sets for ``cases`` in ``order``, and the tiles per window."""
    refs, seqs = [], []
    for i in order:
        hb, ref = _unequal_ref(cases[i], ragged, tuning)
        refs.append(ref)
        seqs.append(batch.DeviceBatch(hb, tuning=tuning))
    return refs, seqs, [-(-cases[i][0] // 64) for i in order]


def _submit_and_read(pipe, refs, seqs, **kw):
    """One submit_sequence, synchronised before anything is looked at.  Returns what the assertions need: the launch, the
    five numbers of its workspace, the int32 words at the documented counter offset, and bit-identity per window."""
    import torch

    for d in seqs:
        _clear(d)
    torch.cuda.synchronize()
    pipe.submit_sequence(seqs, **kw)
    launch = pipe._sched_live[-1]
    pipe.synchronize()
    shape = pipe._plan(launch.structs, int(kw.get("slice_steps", 0)) or binding.STE_SLICE_ALIGN, kw.get("stagger", 0.0)).table_shape()
    off = int(pipe.lib.ste_ukf_forward_sched_progress_offset(*shape))
    assert off % 4 == 0 and off + 4 * shape[2] <= launch.dev_ws.numel()
    words = launch.dev_ws[off: off + 4 * shape[2]].view(torch.int32).cpu().numpy()
    return launch, shape, words, [_same(r, d) for r, d in zip(refs, seqs)]


def _assert_counters_and_bits(result, ntiles, nslices, what=None):
    launch, shape, words, same = result
    assert shape[:3] == (len(ntiles), max(nslices), sum(ntiles)) and shape[3] == launch.items.shape[0], (shape, what)
    assert launch.smoother is not None, what  # one smoother launch, a wave per tile
    # every tile's counter, at the documented offset, holds its window's slice count
    assert np.array_equal(words, np.repeat(nslices, ntiles)), (words.tolist(), what)
    assert all(same), (same, what)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (0, 2, 1)], ids=["ascending", "descending", "longest_in_the_middle"])
def test_tile_smoothers_of_windows_with_unequal_slice_counts_are_bit_identical(order):
    """Windows of 1, 2 and 3 slices (tiles that do and do not fill a wave) in three orders -- where a window's parameter blocks
    start, and how far the packed blocks end in front of the documented region's end, depends on the order -- with and
    without staggered deadlines."""
    refs, seqs, ntiles = _unequal_sequence(order)
    nslices = [(1, 2, 3)[i] for i in order]
    results = []
    with batch.SmootherPipeline(ntracks=200, sequence_only=True) as pipe:
        for stagger in (0.0, 1.0):
            results.append((stagger, _submit_and_read(pipe, refs, seqs, tile_smoothers=True, stagger=stagger)))
    for stagger, res in results:
        _assert_counters_and_bits(res, ntiles, nslices, stagger)


@pytest.mark.gpu
def test_tile_smoothers_of_ragged_tracks_in_windows_with_unequal_slice_counts_are_bit_identical():
    """The same windows with tracks of their own lengths (up to 39 steps short, at least one step): tracks end inside a slice,
    many have nothing to do in their window's last one, and every tile still publishes every slice of its window."""
    refs, seqs, ntiles = _unequal_sequence((0, 1, 2), ragged=True)
    assert seqs[2].hb.nsteps.min() < 128 < seqs[2].hb.nsteps.max() and seqs[0].hb.nsteps.min() == 1
    with batch.SmootherPipeline(ntracks=200, sequence_only=True) as pipe:
        res = _submit_and_read(pipe, refs, seqs, tile_smoothers=True)
    _assert_counters_and_bits(res, ntiles, [1, 2, 3])


@pytest.mark.gpu
def test_tile_smoothers_with_slices_of_128_steps_are_bit_identical():
    """slice_steps = 128: the same windows are 1, 1 and 2 slices -- the Python plan, the forward launch and the smoother launch
    each derive the slice counts from the step they are given, and must agree."""
    refs, seqs, ntiles = _unequal_sequence((0, 1, 2))
    with batch.SmootherPipeline(ntracks=200, sequence_only=True) as pipe:
        res = _submit_and_read(pipe, refs, seqs, tile_smoothers=True, slice_steps=128)
    _assert_counters_and_bits(res, ntiles, [1, 1, 2])


@pytest.mark.gpu
def test_tile_smoothers_on_a_reused_workspace_full_of_stale_bytes_are_bit_identical():
    """A pipeline's second sequence takes the first one's workspace from the pool.  The first (three windows of 3 slices) leaves
    tables and non-zero counters behind; here the pooled workspaces are overwritten with 0x7f on top, so every word a smoother
    wave may look at is a count no tile will ever reach unless this launch's own upload zeroed it."""
    import torch

    refs, seqs, ntiles = _unequal_sequence((0, 1, 2))
    urefs, useqs, untiles = _unequal_sequence((2, 2, 2))
    with batch.SmootherPipeline(ntracks=200, sequence_only=True) as pipe:
        first = _submit_and_read(pipe, urefs, useqs, tile_smoothers=True)
        pooled = list(pipe._sched_free.free)
        for _host_ws, dev_ws, _counters in pooled:
            dev_ws.fill_(0x7f)
        torch.cuda.synchronize()
        kept = {host_ws.data_ptr() for host_ws, _dev_ws, _counters in pooled}
        res = _submit_and_read(pipe, refs, seqs, tile_smoothers=True)
    _assert_counters_and_bits(first, untiles, [3, 3, 3], "uniform")
    assert len(pooled) == 1 and res[0].host_ws.data_ptr() in kept and res[0].dev_ws.data_ptr() == pooled[0][1].data_ptr()
    _assert_counters_and_bits(res, ntiles, [1, 2, 3], "reused")


@pytest.mark.gpu
def test_default_path_of_a_final_sequence_with_unequal_slice_counts_is_bit_identical():
    """What submit_sequence does by itself for a job that is one sequence: batches of more than 4 096 tracks, final, nothing in
    flight -- tile smoothers, no tuning bit -- at the smallest size that gets there, with windows of 2 and 3 slices."""
    refs, seqs, ntiles = _unequal_sequence((0, 1), cases=_DEFAULT_PATH, tuning=0)
    assert ntiles == [65, 65]
    with batch.SmootherPipeline(ntracks=4160) as pipe:
        res = _submit_and_read(pipe, refs, seqs)  # tile_smoothers=None, final=True
    _assert_counters_and_bits(res, ntiles, [2, 3])


@pytest.mark.gpu
def test_c_calls_as_the_header_documents_them_smooth_windows_with_unequal_slice_counts():
    """include/ste.h followed to the letter, without SmootherPipeline: ste_ukf_forward_sched_workspace, the forward launch with
    zeroed counters and `started`, ste_stream_wait_counter on the started word in front of ste_urtss_backward_sched_f64 with
    progress = dev_ws + ste_ukf_forward_sched_progress_offset(the same five numbers).  Two ordinary streams, pageable host
    workspaces (the staged copy), four forward waves -- so tiles wait for a wave and five rounds go by."""
    import torch

    lib = binding.require_gpu()
    refs, seqs, ntiles = _unequal_sequence((0, 1, 2))
    nslices, n, nwaves, dev = [1, 2, 3], 3, 4, seqs[0].device
    for d in seqs:
        _clear(d)
    structs = (binding.SteUkfBatchF64 * n)()
    for i, d in enumerate(seqs):
        st = binding.SteUkfBatchF64.from_buffer_copy(d.struct)
        st.flags = (st.flags & ~binding.STE_FLAG_LANES_4) | binding.STE_FLAG_LANES_1
        st.step_begin = st.step_end = 0
        structs[i] = st
    items = np.ascontiguousarray(batch.forward_schedule(ntiles, nslices, nwaves), dtype=np.int32)
    assert items.shape == (5, nwaves, 2)
    order = batch.smoother_tile_order(items, ntiles)
    shape = (n, max(nslices), sum(ntiles), items.shape[0], nwaves)
    nbytes = int(lib.ste_ukf_forward_sched_workspace(*shape))
    off = int(lib.ste_ukf_forward_sched_progress_offset(*shape))
    host_ws = np.zeros(nbytes, dtype=np.uint8)  # pageable
    dev_ws = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device=dev)  # the call fills it; nothing of this may show
    counters = torch.zeros(n + 2, dtype=torch.int32, device=dev)  # window_done[n], error, started
    sbytes = int(lib.ste_urtss_backward_sched_workspace(n, int(order.shape[0])))
    s_host = np.zeros(sbytes, dtype=np.uint8)
    s_dev = torch.empty(sbytes, dtype=torch.uint8, device=dev)
    fs, bs = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize()  # uploads, clearing and zeroed counters are in memory before either stream starts
    error, started = counters.data_ptr() + 4 * n, counters.data_ptr() + 4 * (n + 1)
    sc = binding.SteFwdSchedF64()
    sc.nwindows, sc.windows, sc.slice_steps = n, C.addressof(structs), 64
    sc.nwaves, sc.nrounds, sc.items = nwaves, items.shape[0], items.ctypes.data
    sc.host_ws, sc.dev_ws, sc.ws_bytes = host_ws.ctypes.data, dev_ws.data_ptr(), nbytes
    sc.window_done, sc.error, sc.started = counters.data_ptr(), error, started
    bw = binding.SteBwdSchedF64()
    bw.nwindows, bw.windows, bw.slice_steps = n, C.addressof(structs), 64
    bw.nitems, bw.items = int(order.shape[0]), order.ctypes.data
    bw.host_ws, bw.dev_ws, bw.ws_bytes = s_host.ctypes.data, s_dev.data_ptr(), sbytes
    bw.progress, bw.error = dev_ws.data_ptr() + off, error
    calls = [lambda: lib.ste_ukf_forward_sched_f64(C.byref(sc), C.c_void_p(fs.cuda_stream)),
             lambda: lib.ste_stream_wait_counter(started, nwaves, error, 0.0, C.c_void_p(bs.cuda_stream)),
             lambda: lib.ste_urtss_backward_sched_f64(C.byref(bw), C.c_void_p(bs.cuda_stream))]
    rcs = []
    for call in calls:  # (nothing goes behind a call that was refused)
        rcs.append((call(), lib.ste_last_error().decode()))
        if rcs[-1][0] != 0:
            break
    fs.synchronize()
    bs.synchronize()
    assert [rc for rc, _ in rcs] == [0, 0, 0], rcs
    words = counters.cpu().numpy()
    assert words[n] == 0  # error word: neither a forward wave nor a smoother wave gave up
    assert words[:n].tolist() == ntiles and words[n + 1] == nwaves  # window_done, started
    progress = dev_ws[off: off + 4 * sum(ntiles)].view(torch.int32).cpu().numpy()
    assert np.array_equal(progress, np.repeat(nslices, ntiles)), progress.tolist()
    same = [_same(r, d) for r, d in zip(refs, seqs)]
    assert all(same), same
    del host_ws, s_host, s_dev, structs, items, order  # (alive until here: the launches read them)
