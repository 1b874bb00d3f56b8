"""The 50-digit reference (oracle/mp_reference.py) against NumPy / SciPy on the inputs the GPU tests use.  No GPU needed.

A reference that is itself wrong would pass wrong kernels, so it is checked here against independent float64 libraries:
libm-grade functions within 1 ulp, NumPy's floored modulo bit for bit, matrix functions and the UKF step to rounding.  The
same runs produce the host baselines (``e_host``) that tests/test_math_probe.py holds the device to; they are printed.

The last section does the same for tests/test_step_residuals.py: the smoother step against the oracle, the exclusions' caps
on the oracle's own histories of every case, and a checker that fails on a 1e-11 slip and names the pair.
"""
import math

import numpy as np
import pytest
import scipy.linalg

import math_probe_cases as mc
import step_residual_cases as sr
from oracle import mp_reference as mpr
from oracle import ukf_oracle as orc

EPS = 2.0**-52


def test_ulp_error_units():
    one = mpr.mpf(1)
    assert mpr.ulp_error(np.nextafter(1.0, 2.0), one) == 1.0
    assert mpr.ulp_error(np.nextafter(1.0, 0.0), one) == 0.5  # the spacing is that at the exact value, 2^-52
    assert mpr.ulp_error(1.0, one) == 0.0
    assert mpr.ulp_error(5e-324, mpr.mpf(0)) == 1.0 and mpr.ulp_error(1e-323, mpr.mpf(5e-324)) == 1.0
    assert mpr.ulp_error(0.75, mpr.mpf(0.75) + mpr.mpf(2) ** -54) == 0.5
    assert mpr.ulp_error(math.inf, one) == math.inf and mpr.ulp_error(math.nan, one) == math.inf
    assert mpr.ulp_error(-3.0, mpr.mpf(-3)) == 0.0 and mpr.ulp_error(np.nextafter(-3.0, 0), mpr.mpf(-3)) == 1.0
    assert mpr.ulp_error(np.nextafter(-4.0, 0), mpr.mpf(-4)) == 0.5


def test_floored_mod_is_numpys_bit_for_bit():
    a = mc.mod360_inputs()
    ours = np.array([mpr.floored_mod(v, 360.0) for v in a])
    assert mc.same_bits(ours, mc.np_mod360(a)).all(), a[~mc.same_bits(ours, mc.np_mod360(a))]
    y = mc.wrap180_inputs()
    ours = np.array([mpr.wrap180(v) for v in y])
    assert mc.same_bits(ours, mc.np_wrap180(y)).all(), y[~mc.same_bits(ours, mc.np_wrap180(y))]
    # the interval the device function used to get wrong: NumPy's answer there is 360.0 itself
    for v in (-1e-20, -1e-14, -1e-300, -(2.0**-45)):
        assert mpr.floored_mod(v) == 360.0 == float(np.mod(v, 360.0))
    assert mpr.floored_mod(-5e-14) == float(np.mod(-5e-14, 360.0)) < 360.0
    for b in (7.5, -7.5, 360.0, -360.0):  # other divisors and signs
        for v in (-1e-20, 1e-20, 22.5, -22.5, 1e10 + 0.5, -0.0, 0.0, 7.5, -15.0):
            got, want = mpr.floored_mod(v, b), float(np.mod(v, b))
            assert got == want and math.copysign(1, got) == math.copysign(1, want), (v, b)


@pytest.mark.parametrize("case", [mc.sincos_kernel_case, mc.atan_small_case, mc.asin_small_case, mc.sincos_fast_case,
                                  mc.sincos_delta_case, mc.atan2_case, mc.div_pos_case, mc.div_earth_radius_case,
                                  mc.rcp_refined_case], ids=lambda f: f.__name__)
def test_libm_within_one_ulp_of_the_reference(case):
    """NumPy's sin, cos, arctan, arcsin, arctan2 (glibc: below 1 ulp) and IEEE division (1/2 ulp) on the GPU tests' inputs."""
    c = case()
    print(f"\n[host baseline] {c.name}: E_host = {c.e_host} ulp over {c.in0.shape[-1]} inputs")
    assert all(e <= 1.0 for e in c.e_host), c.e_host
    if c.name in ("div_pos", "div_earth_radius", "rcp_refined"):
        assert all(e <= 0.5 for e in c.e_host), c.e_host


def test_host_baselines_of_the_composed_operations():
    """1 / np.sqrt(x) is two rounded operations (at most 1/2 ulp each, 1.5 ulp of the result next to a power of two); the
    great-circle step in float64 is ill-conditioned by 1 / cos(lat) near the poles, which is what the device's formula for
    the latitude avoids (csrc/ste_math.h, geodetic_finish)."""
    c = mc.rsqrt_case()
    print(f"\n[host baseline] {c.name}: E_host = {c.e_host}")
    assert c.e_host[0] <= 1.5
    g = mc.geodetic_case()
    lab = np.array(g.label)
    for name in ("ship", "polar"):
        sel = lab == name
        e = [mc.max_ulp(g.host[k], g.exact[k], sel) for k in (0, 1)]
        print(f"[host baseline] geodetic_finish, {name}: E_host (lon, lat) = {e}")
        assert e[0] < 64 and (e[1] < 64 or name == "polar")


def _fwd(a, ref):
    return float(np.max(np.abs(np.asarray(a) - ref)) / np.max(np.abs(ref)))


def test_matrix_functions_against_scipy_and_numpy():
    """sqrtm and pinv are backward stable; their forward errors are bounded by the condition of the problem: sqrt(cond) / 2
    for the square root of a symmetric positive definite matrix (Higham, Functions of Matrices, section 6.1), cond for the
    inverse.  100 eps times that is 'to rounding' with room for the constants of a 4 x 4 LAPACK call."""
    cls = mc.matrix_classes()
    for name, cond in (("example", 1e7), ("cond1", 1.0), ("cond1e4", 1e4), ("cond1e8", 1e8), ("repeated", 4e3)):
        for A in cls[name]:
            T, w = mpr.sym_sqrt(A)
            assert mpr.sqrt_residual(T, A) < 1e-45
            wn = np.linalg.eigvalsh(A)
            assert np.max(np.abs(wn - np.array([float(v) for v in w]))) <= 16 * EPS * np.max(np.abs(wn))
            if np.linalg.matrix_rank(A) == 4:
                assert _fwd(scipy.linalg.sqrtm(A).real, mpr.to_np(T)) <= 100 * EPS * max(1.0, math.sqrt(cond) / 2), name
                Si, _, rank = mpr.pinv_sym(A)
                assert rank == 4 and mpr.pinv_residual(A, Si) < 1e-30
                assert _fwd(np.linalg.pinv(A), mpr.to_np(Si)) <= 100 * EPS * cond, name
    for name, rank in (("rank2", 2), ("rank3", 3)):
        for A in cls[name]:
            Si, w, kept = mpr.pinv_sym(A)
            assert kept == rank == np.linalg.matrix_rank(A, tol=1e-15 * np.max(np.abs(np.linalg.eigvalsh(A))))
            assert _fwd(np.linalg.pinv(A, hermitian=False), mpr.to_np(Si)) <= 100 * EPS * 10, name
    for A in cls["negative_flagged"]:  # the clamp: the square root of the positive part
        T, w = mpr.sym_sqrt(A)
        assert w[0] < 0 and _fwd(orc.sym_sqrt(A), mpr.to_np(T)) <= 1e-6  # sqrt is not Lipschitz at 0: sqrt(1e-16) of slack


def test_ukf_step_against_the_float64_oracle():
    """predict / update / robust terms on the batch of tests/test_single_step_batches.py: the float64 oracle (the reference's
    own NumPy / SciPy calls) agrees with the 50-digit restatement to rounding.  With cond(P) <= 1e4 the fan's square root is
    good to ~1e-14 and nothing downstream amplifies it by more than the w0 = -1/3 weighting, so 1e-10 (four orders above)
    separates rounding from a wrong formula, which shows in the first digits."""
    import single_step_cases as ss

    b = ss.batch()
    for route in ("block", "dense"):
        e = ss.oracle_errors(route)
        print(f"\n[oracle baseline] {route}: {e}")
        assert all(v < 1e-10 for v in e.values()), e
    assert b.count == 130


# ----------------------------------------------------------------------------------------------------------------------
# the row-by-row residuals of tests/test_step_residuals.py: the smoother step, the exclusions and the checker, on the CPU
# ----------------------------------------------------------------------------------------------------------------------
def _history64():
    """Six full tracks of 64 steps (an update every fourth) and the float64 oracle's histories of them."""
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    hb = batch.pack_uniform(synthetic.make_batch(6, nobs=17, gap_h=1.0, seed0=6100), 4, H, Q, R, P0)
    return (hb,) + sr.oracle_history(hb)


def test_urts_step_against_the_float64_oracle():
    """One turn of ukf_oracle.backward_track's loop (the reference's own calls on a history of two rows) against urts_step on
    every third row of a 64-step history, at the bound of the predict / update test above: cond(P_b) stays below 1e2 here, so
    the pseudo-inverse amplifies nothing and 1e-10 separates rounding from a wrong term (P_b centred on x_b instead of x_k
    shows at 1e-3)."""
    hb, hist, status = _history64()
    assert hb.Nmax == 64 and not status.any()
    m, P, sm, sP = (hist[k] for k in ("means", "covs", "means_smoothed", "covs_smoothed"))
    em = ec = 0.0
    for b in range(hb.B):
        for k in range(0, hb.Nmax, 3):
            s = sr.step_inputs(hb, (b, k))
            x, C = mpr.urts_step(m[b, k], P[b, k], sm[b, k + 1], sP[b, k + 1], s.Q, s.dt, s.sog_rate_rts, s.cog_rate_rts)
            assert isinstance(C, mpr.mp.matrix) and len(x) == 4
            hx, hC = sr.smoother_host(hb, (m[b, k], P[b, k]), (sm[b, k + 1], sP[b, k + 1]), (b, k))
            em = max(em, sr.mean_errs(hx, np.array([float(v) for v in x])).max())
            ec = max(ec, sr.cov_errs(hC, mpr.to_np(C)).max())
    print(f"\n[oracle baseline] urts_step, 132 pairs: mean {em:.3e}, cov {ec:.3e}")
    assert em < 1e-10 and ec < 1e-10


def test_urts_step_with_noise_and_its_centring():
    """The recorded noise enters x_b and with it the innovation and D, not P_b, which stays centred on x_k."""
    hb, hist, _ = _history64()
    m, P, sm, sP = (hist[k] for k in ("means", "covs", "means_smoothed", "covs_smoothed"))
    b, k = 2, 30
    s = sr.step_inputs(hb, (b, k))
    nz = np.array([1e-3, -2e-3, 5e-4, 1e-2])
    xb0, Pb0, _ = mpr.urts_gain(m[b, k], P[b, k], s.Q, s.dt, s.sog_rate_rts, s.cog_rate_rts)
    xb1, Pb1, _ = mpr.urts_gain(m[b, k], P[b, k], s.Q, s.dt, s.sog_rate_rts, s.cog_rate_rts, nz)
    assert mpr.max_abs(Pb1 - Pb0) == 0 and all(abs(a - c - mpr.mpf(float(e))) < 1e-45 for a, c, e in zip(xb1, xb0, nz))
    x, C = mpr.urts_step(m[b, k], P[b, k], sm[b, k + 1], sP[b, k + 1], s.Q, s.dt, s.sog_rate_rts, s.cog_rate_rts, nz)
    hx, hC = orc.backward_track(np.array([m[b, k], sm[b, k + 1]]), np.array([P[b, k], sP[b, k + 1]]), s.Q, [s.dt], 1,
                                [s.sog_rate_rts], [s.cog_rate_rts], [nz])
    assert sr.mean_errs(hx[0], np.array([float(v) for v in x])).max() < 1e-10 and sr.cov_errs(hC[0], mpr.to_np(C)).max() < 1e-10


@pytest.mark.parametrize("name", sr.CASES)
def test_exclusion_caps_on_the_oracles_history(name):
    """The exclusions of tests/test_step_residuals.py, counted on the float64 oracle's history of every case it runs: none on
    the synthetic cases, at most 5 % on a regime and never a whole row class (steps 0-2, 62-64, a track's last).  The oracle's
    own rows also pass the comparison, batched (eigh) against per-track (sqrtm) arithmetic."""
    hb = sr.build_case(name)
    hist, status = sr.oracle_history(hb)
    assert len(sr.pairs(hb.nsteps)) <= sr.MAX_PAIRS
    for which in ("forward", "smoother"):
        r, all_pairs, left_out, _ = sr.residuals(hb, hist, status, which)
        sr.report(name + " (oracle)", which, r)
        sr.check_caps(sr.case_kind(name), all_pairs, left_out, hb.nsteps)
        assert r.npairs == len(all_pairs) - len(left_out) > 0
        sr.check(name + " (oracle)", which, r)


def test_pairs_cover_the_rows_they_name():
    import step_loop_cases as slc
    n = slc.ragged_lengths()
    ps = sr.pairs(n)
    assert len(ps) == len(set(ps)) <= sr.MAX_PAIRS and all(0 <= k < n[b] for b, k in ps)
    assert {b for b, _ in ps} == {1, 2, 3, 4, 5, 6, 7, 20, 31, 42, 53, 62, 63, 64}  # slot 0 has no step
    for b in (6, 64):  # the 65-step tracks: both sides of the restart, the last step, every 7th between
        assert [k for t, k in ps if t == b] == [0, 1, 2, 7, 14, 21, 28, 35, 42, 49, 56, 62, 63, 64]
    assert [k for t, k in ps if t == 4] == [0, 1, 2, 7, 14, 21, 28, 35, 42, 49, 56, 62]  # 63 steps: ends before the restart
    assert sr.row_classes((5, 63), n) == ["restart", "last"] and sr.row_classes((3, 2), n) == ["first", "last"]


PERTURB_MEAN, PERTURB_COV = 1e-11, 1e-10


def test_the_checker_has_teeth():
    """The oracle's rows as 'got', one element of one mean multiplied by 1 + 1e-11, one covariance entry moved by 1e-10 of
    max |P|: the comparison of tests/test_step_residuals.py fails and names the pair.  Unperturbed it passes."""
    hb, hist, status = _history64()
    for which, mkey, ckey, row in (("forward", "means", "covs", 1), ("smoother", "means_smoothed", "covs_smoothed", 0)):
        r, all_pairs, left_out, (got, ref, host, kept) = sr.residuals(hb, hist, status, which)
        sr.check("teeth", which, r)
        assert not left_out
        b, k = 4, 21
        assert (b, k) in kept
        for key, el, factor in ((mkey, (1,), 1 + PERTURB_MEAN), (ckey, (0, 1), None)):
            bent = {p: (v[0].copy(), v[1].copy()) for p, v in got.items()}
            a = bent[(b, k)][0 if key == mkey else 1]
            a[el] = a[el] * factor if factor is not None else a[el] + PERTURB_COV * np.max(np.abs(a))
            with pytest.raises(AssertionError, match=rf"track {b}, step {k}, entry \({el[0]},"):
                sr.check("teeth", which, sr.measure(kept, bent, ref, host))
