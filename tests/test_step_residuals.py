"""Every row of the filter and smoother step loops against a 50-digit step.  Needs a real MI355X: run with ``pytest -m gpu``.

The whole-run tests hold the step loops at 1e-6 / 1e-5 (differences compound along a track) and the bit fixtures hold them to
their own past; the 50-digit tests of tests/test_math_probe.py and tests/test_single_step_batches.py stop at the leaves and
at the one-step entry points, while the loops inline code of their own: packed triangles, deviations from the propagated
centre point, the closed-form two-column update, a warm eigenvector basis restarted every 64 steps (csrc/ste_lane.h), the
quad-per-track form (csrc/ste_quad.h), and in the smoother P_b rebuilt as P- + b b^T on rows that are not full, the rate shift,
the LDL gain with its eigenvalue fallback and the lane recurrence (csrc/ste_smooth.h).

So this module compares row by row (tests/step_residual_cases.py): from the DEVICE'S OWN filtered row k a 50-digit step says
what its row k + 1 must be, and from its filtered row k and smoothed row k + 1 what its smoothed row k must be.  Nothing
accumulates.  Per (case, form), over the pairs kept, for the means and for the covariances:

    E_dev <= 4 E_host + 8 * 2^-52

E_host being the float64 oracle's step (scipy.linalg.sqrtm, np.linalg.pinv: the reference's own calls) against the same
50-digit step on the same inputs -- the rule of tests/test_single_step_batches.py; no constant is tuned to the device.
tests/test_mp_reference.py checks the reference, the exclusions' caps and the checker's teeth without a GPU.

One term of the bound carries a factor, derived in step_residual_cases.mean_errs: the heading of a row whose step ended by
reducing it mod 360 is measured in units of the unreduced heading u (taken from the 50-digit step), because the reduction
turns the rounding of u into an error |u| / |u mod 360| times larger relative to the result, in any float64 arithmetic.  The
quad-per-track predict adds the nine sigma headings as a tree of (plus, minus) pairs, four lanes wide
(csrc/ste_forward_quad.hip, quad_sum), where the lane-per-track form and NumPy add them in a row; on heading_seam, track 20,
step 7, that leaves 2.6 ulp of u = 360.155 against NumPy's 0.4, which the reduction to 0.155 shows as 9.4e-13 against 1.6e-13.
Held in units of u, the same pair is at 4.1e-16 and the case's bound drops from 6e-13 to 6e-15 for every other element.

Forms: the forward pass lane-per-track and quad-per-track; the smoother as one kernel, as two kernels, with the lane
recurrence, with every gain by the eigenvalue route (both), and stand-alone (no work rows: it recomputes what they hold).
Every form runs on ``quarter``; the other cases run the first two of each.  Per-track noise has no quad-per-track kernel
(DeviceBatch refuses lanes=4 for it), so that one combination does not exist.  The plain, sliced, scheduled and tile forms are
tied to these bit for bit by tests/test_plain_step_loops.py, test_step_loop_waits.py and test_scheduled_forward.py.

Measured values: profiles/step_loop_errors.md.
"""
import dataclasses
import functools

import numpy as np
import pytest

import step_residual_cases as sr

pytestmark = pytest.mark.gpu

ONE_KERNEL, TWO_KERNEL, LANE_RECURRENCE, EIGEN_GAINS = 0x400, 0x200, 0x800, 0x100  # include/ste.h: STE_TUNING_*

FORWARD_FORMS = {"lanes=1": 1, "lanes=4": 4}
SMOOTHER_FORMS = {  # name -> DeviceBatch arguments
    "one-kernel": dict(tuning=ONE_KERNEL),
    "two-kernel": dict(tuning=TWO_KERNEL),
    "lane-recurrence": dict(tuning=TWO_KERNEL | LANE_RECURRENCE),
    "one-kernel-eigen-gains": dict(tuning=ONE_KERNEL | EIGEN_GAINS),
    "two-kernel-eigen-gains": dict(tuning=TWO_KERNEL | EIGEN_GAINS),
    "stand-alone": dict(fuse_gains=False),
}
FORWARD_PARAMS = [(c, f) for c in sr.CASES for f in FORWARD_FORMS if not (c == "track_noise" and f == "lanes=4")]
SMOOTHER_PARAMS = [(c, f) for c in sr.CASES for f in (SMOOTHER_FORMS if c == "quarter" else ("one-kernel", "two-kernel"))]


@functools.lru_cache(None)
def _device_pass(case, lanes, form):
    """One device pass of a (case, form): (HostBatch, histories (B, N + 1, ...), status words)."""
    from track_estimators import batch

    hb = dataclasses.replace(sr.build_case(case), lanes=lanes)
    db = batch.DeviceBatch(hb, **SMOOTHER_FORMS[form])
    db.run()
    hist = {k: np.array(v) for k, v in db.download().items()}
    return hb, hist, np.array(db.status_host())


def _hold(case, form, which, hb, hist, status):
    r, all_pairs, left_out, _ = sr.residuals(hb, hist, status, which)
    sr.report(f"{case} {form}", which, r)
    if left_out:
        print(f"[step residual] {case} {form} {which}: left out {left_out}")
    sr.check_caps(sr.case_kind(case), all_pairs, left_out, hb.nsteps)
    assert all(status[p[0]] == 0 for p in all_pairs if p not in left_out)  # a pair kept belongs to a track not flagged
    if sr.case_kind(case) == "synthetic":
        assert not status.any(), np.flatnonzero(status)
    assert r.npairs > 0
    sr.check(f"{case} {form}", which, r)


@pytest.mark.parametrize("case,form", FORWARD_PARAMS, ids=["-".join(p) for p in FORWARD_PARAMS])
def test_forward_rows(case, form):
    """Filtered row k + 1 from the device's filtered row k: predict, the update where one fires, the initial update on row 0."""
    _hold(case, form, "forward", *_device_pass(case, FORWARD_FORMS[form], "one-kernel"))


@pytest.mark.parametrize("case,form", SMOOTHER_PARAMS, ids=["-".join(p) for p in SMOOTHER_PARAMS])
def test_smoother_rows(case, form):
    """Smoothed row k from the device's filtered row k and its smoothed row k + 1 (lane-per-track forward pass)."""
    _hold(case, form, "smoother", *_device_pass(case, 1, form))
