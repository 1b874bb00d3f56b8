"""The "plain batch" forms of the two step loops (csrc/ste_ukf.h: plain_batch; DESIGN.md section 5, "Plain batches"): for a
batch with packed covariances, no recorded noise and no position copy the host launches kernels in which those three facts are
compiled in (ukf_forward_l1_plain, ukf_forward_sched_plain, urtss_recur_l1_plain, urtss_recur_sched_plain).  They remove scalar,
address and select instructions only, so every output must keep its bits:

  * plain against general: the same HostBatch as DeviceBatch(hb) -- plain -- and as DeviceBatch(hb, sm_pos=True), which
    allocates the position copy and so takes the general kernels, and changes nothing else;
  * plain against full covariances (packed_cov=False, general kernels): the downloaded (.., 4, 4) histories;
  * the launch forms of the plain path among themselves: whole pass, two time slices, scheduled launch;
  * a scheduled sequence of one plain and one general batch (the plain kernels run a table only if every parameter block of
    it is plain): each batch equals its own DeviceBatch.run().

The batches are those of tests/step_loop_cases.py (65 tracks x 65 steps: a full wave and a one-lane wave, lengths 0, 1, 2, 3,
63, 64, 65, both sides of the 64-step restart, updates on all / none / a quarter of the steps, with and without the initial
update, NaN / infinite / indefinite priors).  The cases that are not plain (`noise`, `track_noise`) and `shift` are held to
tests/golden/step_loop_bits_parent.npz by tests/test_step_loop_waits.py, which also holds the plain cases -- and with them the
plain kernels -- to the bits of the build that fixture was recorded from.  Both runs of a comparison use the one-kernel
smoother, so a NaN must equal the same NaN, payload included.
"""
import numpy as np
import pytest

import step_loop_cases as slc

PLAIN_CASES = ("every", "none", "quarter", "none_noinit", "bad_prior")
HISTORIES = ("means", "covs", "means_smoothed", "covs_smoothed")


def _device_batch(hb, **kw):
    from track_estimators import batch

    db = batch.DeviceBatch(hb, device="cuda:0", tuning=slc.ONE_KERNEL, **kw)
    for name in slc.ARRAYS + (("sm_pos",) if db.sm_pos is not None else ()):
        getattr(db, name).fill_(slc.SENTINEL)
    return db


def _same_bits(a, b, what, keys=slc.ARRAYS + ("status",)):
    for k in keys:
        x, y = a[k], b[k]
        assert x.shape == y.shape, f"{what}: {k} has shapes {x.shape} and {y.shape}"
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f"{what}: {k} differs at {np.argwhere(x != y)[:4].tolist()}"


@pytest.fixture(scope="module")
def plain():
    """Case -> (raw outputs, downloaded histories) of the plain path's whole pass, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            db = _device_batch(slc.build_case(name))
            assert db.packed_cov and db.sm_pos is None and db.noise is None
            db.run()
            cache[name] = (slc.outputs(db), {k: v.copy() for k, v in db.download(HISTORIES).items()})
        return cache[name]

    return get


def test_the_cases_are_plain_batches():
    """On the host: none of the five carries recorded noise, per-track noise or smoother rates of its own."""
    for name in PLAIN_CASES:
        hb = slc.build_case(name)
        assert hb.noise_pred is None and hb.noise_upd is None and hb.noise_rts is None, name
        assert hb.Q_tracks is None and hb.R_tracks is None and hb.sog_rate_rts is None and hb.cog_rate_rts is None, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN_CASES)
def test_plain_kernels_are_the_general_kernels(plain, name):
    """sm_pos=True forces the general kernels; histories, status and every work row (the first-bad row last) keep their bits,
    and the position copy the general smoother writes is the smoothed lon / lat."""
    db = _device_batch(slc.build_case(name), sm_pos=True)
    db.run()
    general = slc.outputs(db)
    _same_bits(plain(name)[0], general, f"{name}: plain against general (sm_pos)")
    pos = db.sm_pos.cpu().numpy()
    assert np.array_equal(pos.view(np.uint64), general["sm_mean"][:, :2].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN_CASES)
def test_plain_kernels_against_full_covariances(plain, name):
    """packed_cov=False keeps (.., 4, 4) matrices in memory and takes the general kernels: what comes down is what the plain
    path's packed histories expand to."""
    from track_estimators import batch

    db = batch.DeviceBatch(slc.build_case(name), device="cuda:0", tuning=slc.ONE_KERNEL, packed_cov=False)
    for attr in slc.ARRAYS:
        getattr(db, attr).fill_(slc.SENTINEL)
    db.run()
    full = db.download(HISTORIES)
    _same_bits(plain(name)[1], full, f"{name}: plain against full covariances", HISTORIES)
    assert np.array_equal(plain(name)[0]["status"], db.status.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN_CASES)
def test_plain_two_time_slices_are_the_whole_pass(plain, name):
    from track_estimators import batch

    assert batch.DeviceBatch.slice_bounds(slc.NSTEPS, 2) == [(0, 64), (64, 65)]
    _same_bits(plain(name)[0], slc.run_sliced(slc.build_case(name), 2), f"{name}: plain, 2 slices")


@pytest.mark.gpu
def test_plain_scheduled_launch_is_the_whole_pass(plain):
    from track_estimators import batch

    with batch.SmootherPipeline(ntracks=slc.NTRACKS, sequence_only=True) as pipe:
        for name in PLAIN_CASES:
            _same_bits(plain(name)[0], slc.run_scheduled(slc.build_case(name), pipe), f"{name}: plain, scheduled")


@pytest.mark.gpu
def test_a_sequence_of_a_plain_and_a_general_batch(plain):
    """One scheduled launch over two batches, the second with a position copy: the table is not all plain, so the general
    kernels run both.  Each batch equals its own DeviceBatch.run()."""
    from track_estimators import batch

    names, kws = ("quarter", "bad_prior"), ({}, {"sm_pos": True})
    with batch.SmootherPipeline(ntracks=slc.NTRACKS, sequence_only=True) as pipe:
        dbs = [_device_batch(slc.build_case(name), **kw) for name, kw in zip(names, kws)]
        dbs[0].torch.cuda.synchronize()
        pipe.submit_sequence(dbs, tile_smoothers=True)
        pipe.synchronize()
        outs = [slc.outputs(db) for db in dbs]
    for name, out in zip(names, outs):
        _same_bits(plain(name)[0], out, f"{name} in a sequence of a plain and a general batch")
    assert np.array_equal(dbs[1].sm_pos.cpu().numpy().view(np.uint64), outs[1]["sm_mean"][:, :2].view(np.uint64))
