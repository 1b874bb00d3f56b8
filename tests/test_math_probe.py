"""The device math building blocks (csrc/ste_math.h) against a 50-digit reference, through the probe (csrc/ste_probe.hip).
Needs a real MI355X: run with ``pytest -m gpu``.

Every filter and smoother kernel is built from these functions, and before this module they were only reached through
whole filter runs compared at 1e-6: a polynomial coefficient wrong in its tenth digit, a guard off by one comparison or a
register-coefficient slot initialised from the wrong literal passed.  Here each function runs on a few thousand inputs --
dense over its interval plus its edges -- and is held to

  * the header's own claim where it makes one: ``floored_mod360`` / ``wrap180`` equal NumPy bit for bit; the polynomial
    kernels, ``div_pos`` and ``rsqrt_fast`` are within 1 ulp;
  * the host otherwise: E_dev <= 2 E_host + 1 ulp, E_host being the largest ulp error of plain NumPy float64 on the same
    inputs (tests/test_mp_reference.py computes and checks it on the CPU).  Two equally valid evaluation orders differ by
    about an ulp; a wrong coefficient, a lost reduction constant or a wrong guard shows as thousands;
  * for the 4 x 4 matrix functions, 4 x the same metric of NumPy / SciPy + 8 * 2^-52 (Jacobi and LAPACK accumulate
    differently over up to 12 sweeps), all metrics evaluated in 50-digit arithmetic.

Findings of the first run of this module, fixed with it (csrc/ste_math.h):
  * ``floored_mod360`` returned a itself for a in [-2^-45, 0) where NumPy returns 360.0;
  * ``sincos_fast`` / ``sincos_fast_n`` reduced with two constants of pi/2: next to a multiple of pi/2 the reduced argument
    was off by hundreds to tens of thousands of ulps (316 at the double nearest 29 pi/2, a heading of 2 610 degrees; 31 000
    at 204 551 pi/2).  A third constant closes it;
  * ``ldl_factor4``'s "bad" verdict missed a NaN in an off-diagonal entry (fmin drops a NaN operand);
  * the header's "< 1 ulp" did not hold for the cosine kernel (1.18 ulp next to pi/4): the header now says <= 1.5 ulp.
Measured maxima: profiles/math_probe_errors.md.
"""
import math

import numpy as np
import pytest

import math_probe_cases as mc
import probe_binding as pb
from oracle import mp_reference as mpr

pytestmark = pytest.mark.gpu

EPS = 2.0**-52


def _report(name, e_dev, e_host=None, bound=None):
    print(f"\n[probe] {name}: E_dev = {e_dev}" + ("" if e_host is None else f", E_host = {e_host}")
          + ("" if bound is None else f", bound = {bound}"))


# ------------------------------------------------------------------------------------------------------------------
# stated: bit for bit
# ------------------------------------------------------------------------------------------------------------------
def test_floored_mod360_is_numpys_bit_for_bit():
    a = mc.mod360_inputs()
    got = pb.run_scalar(pb.FLOORED_MOD360, a)[0]
    want = mc.np_mod360(a)
    bad = ~mc.same_bits(got, want)
    assert not bad.any(), list(zip(a[bad], got[bad], want[bad]))[:10]
    i = list(a).index(-1e-20)
    assert got[i] == 360.0  # the interval [-2^-45, 0): a + 360 rounds to 360.0


def test_wrap180_is_numpys_bit_for_bit():
    y = mc.wrap180_inputs()
    got = pb.run_scalar(pb.WRAP180, y)[0]
    want = mc.np_wrap180(y)
    bad = ~mc.same_bits(got, want)
    assert not bad.any(), list(zip(y[bad], got[bad], want[bad]))[:10]


# ------------------------------------------------------------------------------------------------------------------
# stated: 1 ulp
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,case", [(pb.SINCOS_KERNEL, mc.sincos_kernel_case), (pb.ATAN_SMALL, mc.atan_small_case),
                                     (pb.ASIN_SMALL, mc.asin_small_case), (pb.DIV_POS, mc.div_pos_case),
                                     (pb.RSQRT_FAST, mc.rsqrt_case)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_stated_one_ulp(op, case):
    """csrc/ste_math.h: '< 1 ulp on their intervals' (the fdlibm kernels), 'within an ulp' (div_pos); rsqrt_fast leaves
    ~2^-70 before its final rounding.  Ends of the interval, their neighbours, 0, denormals, exponents 1e-300 .. 1e300.

    The cosine of sincos_kernel did not hold the header's "< 1 ulp": 1.18 ulp next to pi/4 (its head 1 - z/2 is rounded before
    the tail is added).  The header now states what was measured, rounded up to the next half ulp -- cos <= 1.5 ulp -- and
    that is what is asserted; the sine holds 1 ulp (0.58)."""
    c = case()
    out = pb.run_scalar(op, c.in0, c.in1)
    e = [mc.max_ulp(out[k], c.exact[k]) for k in range(len(c.exact))]
    stated = [1.0, 1.5] if op == pb.SINCOS_KERNEL else [1.0]  # the cosine: see below
    _report(c.name, e, c.e_host, stated)
    assert all(v <= b for v, b in zip(e, stated)), e
    if op in (pb.SINCOS_KERNEL, pb.ATAN_SMALL, pb.ASIN_SMALL):  # odd functions of a denormal or a zero: the argument itself
        tiny = np.abs(c.in0) < 1e-300
        assert np.array_equal(out[0][tiny], c.in0[tiny])


# ------------------------------------------------------------------------------------------------------------------
# no stated bound: the host is the bar
# ------------------------------------------------------------------------------------------------------------------
def _assert_host_bar(name, outs, c, where=None):
    e = [mc.max_ulp(outs[k], c.exact[k], where) for k in range(len(c.exact))]
    bound = [2 * h + 1 for h in c.e_host]
    _report(name, e, c.e_host, bound)
    assert all(v <= b for v, b in zip(e, bound)), (name, e, bound)
    return e


@pytest.mark.parametrize("op,case", [(pb.SINCOS_FAST, mc.sincos_fast_case), (pb.SINCOS_DELTA, mc.sincos_delta_case),
                                     (pb.ATAN2_FAST, mc.atan2_case), (pb.DIV_EARTH_RADIUS, mc.div_earth_radius_case),
                                     (pb.RCP_REFINED, mc.rcp_refined_case)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_scalar_functions_against_the_host(op, case):
    """sincos_fast: the doubles nearest k pi/2 (all k <= 64, the 150 closest of all k < 2^20 * 2/pi, 500 more), headings of 0,
    90, ..., 3600 degrees times kDeg2Rad, both sides of 2^20 and beyond (the library path).  sincos_delta: both sides of its
    pi/4 literal.  atan2_fast: both sides of |a| = 0.4375 b where 0.4375 b is exact, b <= 0, b = 1e-300 and its neighbour."""
    c = case()
    out = pb.run_scalar(op, c.in0, c.in1)
    _assert_host_bar(c.name, out, c)


def _both(op_lit, op_reg, c):
    lit, reg = pb.run_scalar(op_lit, c.in0, c.in1), pb.run_scalar(op_reg, c.in0, c.in1)
    for k in (0, 1):
        bad = ~mc.same_bits(lit[k], reg[k])
        assert not bad.any(), ("literal and register coefficients differ", k, c.in0[bad][:5], lit[k][bad][:5], reg[k][bad][:5])
    assert np.array_equal(lit[2], reg[2])
    return lit


def test_sincos_fast_n_both_coefficient_sources():
    """sincos_fast_n<3> as the kernels instantiate it (TrigLit, and TrigReg after trig_reg_init): the two give the same bits,
    ok is |x| < 2^20 exactly, and where ok the values meet the host's bar.  A TrigReg slot filled from the wrong literal fails
    the first assertion on every input."""
    c = mc.sincos_fast_case()
    s, co, ok = _both(pb.SINCOS_FAST3_LIT, pb.SINCOS_FAST3_REG, c)
    assert np.array_equal(ok == 1, c.ok), c.in0[(ok == 1) != c.ok]
    _assert_host_bar("sincos_fast_n<3>", (s, co), c, where=c.ok)


def test_sincos_delta_n_both_coefficient_sources():
    c = mc.sincos_delta_case()
    s, co, ok = _both(pb.SINCOS_DELTA3_LIT, pb.SINCOS_DELTA3_REG, c)
    assert np.array_equal(ok == 1, c.ok), c.in0[(ok == 1) != c.ok]
    _assert_host_bar("sincos_delta_n<3>", (s, co), c, where=c.ok)


@pytest.mark.parametrize("lit,reg,case", [(pb.ATAN_SMALL3_LIT, pb.ATAN_SMALL3_REG, mc.atan_small_case),
                                          (pb.ASIN_SMALL3_LIT, pb.ASIN_SMALL3_REG, mc.asin_small_case)],
                         ids=["atan_small_n", "asin_small_n"])
def test_small_n_both_coefficient_sources(lit, reg, case):
    """atan_small_n / asin_small_n with GeoLit and with GeoReg after geo_reg_init: same bits, and the host's bar (the
    polynomials are the scalar functions'; only the contraction of the surrounding code differs)."""
    c = case()
    out = _both(lit, reg, c)
    e = mc.max_ulp(out[0], c.exact[0])
    _report(c.name + "_n<3>", e, c.e_host, 2 * c.e_host[0] + 1)
    assert e <= 2 * c.e_host[0] + 1


def test_atan2_fast_takes_the_fast_path_where_the_guard_says():
    """Inside the guard atan2_fast is atan_small(div_pos(a, b)) -- at most 1 ulp of the quotient and 1 of the polynomial --
    and outside it the library's atan2; a guard moved to the wrong side shows at the rows where |a| = 0.4375 b exactly and at
    the next double, whose quotients lie on either side of 7/16, the end of the polynomial's interval."""
    c = mc.atan2_case()
    got = pb.run_scalar(pb.ATAN2_FAST, c.in0, c.in1)[0]
    on = np.abs(c.in0) == 0.4375 * c.in1
    assert on.sum() >= 8 and c.fast[on].all()
    e_in, e_out = mc.max_ulp(got, c.exact[0], c.fast), mc.max_ulp(got, c.exact[0], ~c.fast)
    _report("atan2_fast inside / outside the guard", [e_in, e_out], c.e_host)
    assert e_in <= 2 * c.e_host[0] + 1 and e_out <= 2 * c.e_host[0] + 1


# ------------------------------------------------------------------------------------------------------------------
# geodetic_finish
# ------------------------------------------------------------------------------------------------------------------
def _geo_groups(c):
    lab = np.array(c.label)
    return [("ship", lab == "ship"), ("polar", lab == "polar"), ("edge", ~np.isin(lab, ("ship", "polar")))]


def test_geodetic_finish_scalar_takes_every_fallback():
    """The branching form on every row: ships, polar steps, and each fallback -- |a| > 0.4375 b, b <= 0, b = 1e-300, the pole
    (h2 = 0), |xs| > 0.5, cos(arc) <= 0 including the header's 150-degree case -- against the great-circle step in 50 digits.
    The bar is the host's error on the same group of rows."""
    c = mc.geodetic_case()
    lon, lat, _ = pb.run_scalar(pb.GEO_FINISH, c.in0)
    for name, sel in _geo_groups(c):
        e = [mc.max_ulp(lon, c.exact[0], sel), mc.max_ulp(lat, c.exact[1], sel)]
        h = [mc.max_ulp(c.host[0], c.exact[0], sel), mc.max_ulp(c.host[1], c.exact[1], sel)]
        _report("geodetic_finish " + name + " (lon, lat)", e, h, [2 * v + 1 for v in h])
        assert all(v <= 2 * w + 1 for v, w in zip(e, h)), (name, e, h)
    i = c.label.index("cd<0 only")
    assert abs(lat[i] + 80.0) < 1e-9  # 160 degrees south of 80 N; the unguarded identity says 60 N


def test_geodetic_finish_n_verdicts_values_and_variants():
    """geodetic_finish_n<1>, <2> and <3, GeoReg>: slot 0 carries the same bits in all three; ok is true on every ship and
    polar row and false on every row that leaves a fast path (each guard on its own); where ok, the values meet the host's bar."""
    c = mc.geodetic_case()
    o1, o2, o3 = (pb.run_scalar(op, c.in0) for op in (pb.GEO_FINISH1, pb.GEO_FINISH2, pb.GEO_FINISH3_REG))
    for other in (o2, o3):
        for k in (0, 1):
            bad = ~mc.same_bits(o1[k], other[k])
            assert not bad.any(), ("variants differ", k, np.array(c.label)[bad][:5])
        assert np.array_equal(o1[2], other[2])
    wrong = (o1[2] == 1) != c.ok
    assert not wrong.any(), np.array(c.label)[wrong]
    for name, sel in _geo_groups(c):
        sel = sel & c.ok
        e = [mc.max_ulp(o1[0], c.exact[0], sel), mc.max_ulp(o1[1], c.exact[1], sel)]
        h = [mc.max_ulp(c.host[0], c.exact[0], sel), mc.max_ulp(c.host[1], c.exact[1], sel)]
        _report("geodetic_finish_n " + name + " (lon, lat)", e, h, [2 * v + 1 for v in h])
        assert all(v <= 2 * w + 1 for v, w in zip(e, h)), (name, e, h)


# ------------------------------------------------------------------------------------------------------------------
# 4 x 4 matrix functions.  Metrics in 50 digits; bound = 4 * (the same metric of NumPy / SciPy) + 8 * 2^-52.
# ------------------------------------------------------------------------------------------------------------------
def _mbound(host):
    return 4 * host + 8 * EPS


def _eig_err(w, A):
    we, _ = mpr.eigsy(A)
    wmax = max(abs(v) for v in we)
    return float(max(abs(mpr.mpf(float(a)) - b) for a, b in zip(sorted(w), we)) / wmax) if wmax else float(np.max(np.abs(w)))


def _recon_err(V, w, A):
    V, A = mpr.mat(V), mpr.mat(A)
    D = mpr.mp.diag([mpr.mpf(float(v)) for v in w])
    return float(mpr.max_abs(V * D * V.T - A) / mpr.max_abs(A))


@pytest.mark.parametrize("cls", ["example", "cond1", "cond1e4", "cond1e8", "cond1e12", "repeated", "diagonal",
                                 "negative_flagged", "negative_silent", "rank2", "rank3", "block2"])
def test_jacobi_eig4(cls):
    A = mc.matrix_classes()[cls]
    V, w, out, st = pb.run_mat4(pb.JACOBI_EIG4, A)
    assert not st.any()  # 0x4: no class here needs more than 12 sweeps
    ee, eo, er, he, ho, hr = [], [], [], [], [], []
    for i, a in enumerate(A):
        wn, Vn = np.linalg.eigh(a)
        ee.append(_eig_err(w[i], a)), he.append(_eig_err(wn, a))
        eo.append(float(mpr.orth_defect(V[i]))), ho.append(float(mpr.orth_defect(Vn)))
        er.append(_recon_err(V[i], w[i], a)), hr.append(_recon_err(Vn, wn, a))
    _report(f"jacobi_eig4 {cls} (eigenvalues, |VtV - I|, |V w Vt - A|)", [max(ee), max(eo), max(er)], [max(he), max(ho), max(hr)])
    assert max(ee) <= _mbound(max(he)) and max(eo) <= _mbound(max(ho)) and max(er) <= _mbound(max(hr))
    if cls == "diagonal":  # no rotation may happen: the basis stays the identity and the matrix itself
        assert (V == np.eye(4)).all() and np.array_equal(out, A) and np.array_equal(w, np.diagonal(A, axis1=1, axis2=2))


@pytest.mark.parametrize("start", ["perturbed 1e-3", "perturbed 1e-9", "permuted"])
def test_jacobi_eig4_warm(start):
    """The warm start from the basis of a nearby matrix (and from that basis with its columns permuted) reaches the same
    decomposition as LAPACK to the same bound."""
    A, V0 = mc.warm_cases()[start]
    V, w, _, st = pb.run_mat4(pb.JACOBI_EIG4_WARM, A, V0)
    assert not st.any()
    ee, eo, er, he, ho, hr = [], [], [], [], [], []
    for i, a in enumerate(A):
        wn, Vn = np.linalg.eigh(a)
        ee.append(_eig_err(w[i], a)), he.append(_eig_err(wn, a))
        eo.append(float(mpr.orth_defect(V[i]))), ho.append(max(float(mpr.orth_defect(Vn)), float(mpr.orth_defect(V0[i]))))
        er.append(_recon_err(V[i], w[i], a)), hr.append(_recon_err(Vn, wn, a))
    _report(f"jacobi_eig4_warm {start}", [max(ee), max(eo), max(er)], [max(he), max(ho), max(hr)])
    assert max(ee) <= _mbound(max(he)) and max(eo) <= _mbound(max(ho)) and max(er) <= _mbound(max(hr))
    T, _, out, st = pb.run_mat4(pb.SYM_SQRT4_WARM, A, V0, scale=3.0)
    assert not st.any()
    import scipy.linalg

    e = max(float(mpr.sqrt_residual(out[i], a, 3.0)) for i, a in enumerate(A))
    h = max(float(mpr.sqrt_residual(scipy.linalg.sqrtm(3.0 * a).real, a, 3.0)) for a in A)
    _report(f"sym_sqrt4<true> {start} |T T - s P| / |s P|", e, h, _mbound(h))
    assert e <= _mbound(h)


@pytest.mark.parametrize("cls,flag", [("example", 0), ("cond1", 0), ("cond1e4", 0), ("cond1e8", 0), ("cond1e12", 0),
                                      ("repeated", 0), ("diagonal", 0), ("negative_flagged", 2), ("negative_silent", 0),
                                      ("rank2", 0), ("rank3", 0)])
def test_sym_sqrt4(cls, flag):
    """|T T - scale P+| / |scale P| with P+ the matrix with its negative eigenvalues clamped (in 50 digits), against
    scipy.linalg.sqrtm's real part, and the status bits: 0x2 exactly on the class built with an eigenvalue below
    -1e-12 max|diag|, 0x4 nowhere."""
    import scipy.linalg

    A = mc.matrix_classes()[cls]
    scale = 3.0
    _, _, T, st = pb.run_mat4(pb.SYM_SQRT4_COLD, A, scale=scale)
    assert (st == flag).all(), st
    e, h = [], []
    for i, a in enumerate(A):
        Te, _ = mpr.sym_sqrt(a, scale)
        Pp = Te * Te / scale  # the clamped matrix
        e.append(float(mpr.sqrt_residual(T[i], Pp, scale)))
        with np.errstate(all="ignore"):
            Th = np.real(scipy.linalg.sqrtm(scale * a))
        h.append(float(mpr.sqrt_residual(Th, Pp, scale)) if np.isfinite(Th).all() else math.inf)
    _report(f"sym_sqrt4 {cls} |T T - s P| / |s P|", max(e), max(h), _mbound(max(h)))
    assert max(e) <= _mbound(max(h))


@pytest.mark.parametrize("cls", ["example", "cond1", "cond1e4", "cond1e8", "cond1e12", "repeated", "diagonal", "rank2", "rank3",
                                 "block2"])
def test_sym_pinv4(cls):
    """|S S+ S - S| / |S|, the rank kept (NumPy's rcond = 1e-15 rule) and the eigenvalues returned, against np.linalg.pinv."""
    A = mc.matrix_classes()[cls]
    if cls == "diagonal":
        A = A[:4]  # without the singular ones, whose rank is decided at 1e-300
    _, w, Si, st = pb.run_mat4(pb.SYM_PINV4, A)
    assert not st.any()
    e, h, ee, he = [], [], [], []
    for i, a in enumerate(A):
        _, we, rank = mpr.pinv_sym(a)
        kept = int(np.sum(np.abs(w[i]) > 1e-15 * np.max(np.abs(w[i]))))
        assert kept == rank, (cls, i, w[i])
        e.append(float(mpr.pinv_residual(a, Si[i]))), h.append(float(mpr.pinv_residual(a, np.linalg.pinv(a))))
        ee.append(_eig_err(w[i], a)), he.append(_eig_err(np.linalg.eigvalsh(a), a))
    _report(f"sym_pinv4 {cls} (|S S+ S - S| / |S|, eigenvalues)", [max(e), max(ee)], [max(h), max(he)])
    assert max(e) <= _mbound(max(h)) and max(ee) <= _mbound(max(he))


def test_sym_pinv4_block2_against_sym_pinv4():
    """The 2 x 2 route and the general route on the same block matrices: the same rank, and each within the bound of the
    50-digit pseudo-inverse (forward error, so the two are compared with each other through it)."""
    A = mc.matrix_classes()["block2"]
    _, w2, S2, _ = pb.run_mat4(pb.SYM_PINV4_BLOCK2, A)
    _, w4, S4, st = pb.run_mat4(pb.SYM_PINV4, A)
    assert not st.any()
    e2, e4, h, r2, r4, hr = [], [], [], [], [], []
    for i, a in enumerate(A):
        Se, _, rank = mpr.pinv_sym(a)
        ref = mpr.to_np(Se)
        k2 = int(np.sum(np.abs(w2[i][:2]) > 1e-15 * np.max(np.abs(w2[i][:2]))))
        k4 = int(np.sum(np.abs(w4[i]) > 1e-15 * np.max(np.abs(w4[i]))))
        assert k2 == k4 == rank, (i, w2[i], w4[i])
        sc = np.max(np.abs(ref))
        e2.append(float(np.max(np.abs(S2[i] - ref)) / sc)), e4.append(float(np.max(np.abs(S4[i] - ref)) / sc))
        h.append(float(np.max(np.abs(np.linalg.pinv(a) - ref)) / sc))
        r2.append(float(mpr.pinv_residual(a, S2[i]))), r4.append(float(mpr.pinv_residual(a, S4[i])))
        hr.append(float(mpr.pinv_residual(a, np.linalg.pinv(a))))
        assert (S2[i][2:, :] == 0).all() and (S2[i][:, 2:] == 0).all() and (w2[i][2:] == 0).all()
    _report("sym_pinv4_block2 / sym_pinv4 forward error", [max(e2), max(e4)], max(h), _mbound(max(h)))
    _report("sym_pinv4_block2 / sym_pinv4 |S S+ S - S| / |S|", [max(r2), max(r4)], max(hr), _mbound(max(hr)))
    assert max(e2) <= _mbound(max(h)) and max(e4) <= _mbound(max(h))
    assert max(r2) <= _mbound(max(hr)) and max(r4) <= _mbound(max(hr))


def test_ldl_right_solve4():
    """K = D A^-1: the 'bad' verdict is true exactly where the smallest pivot is not above kLdlPivotTol = 1e-7 of the largest
    diagonal entry (pivots in 50 digits; no matrix within 1 % of the threshold) and for a NaN; where it is false,
    |K A - D| / |D| is within the bound of D pinv(A), the reference's own evaluation."""
    A, D, ratio = mc.ldl_cases()
    _, _, K, bad = pb.run_mat4(pb.LDL_RIGHT_SOLVE4, A, D)
    assert not np.any(np.abs(ratio / 1e-7 - 1) < 0.01)
    want = ~(ratio > 1e-7)  # NaN: bad
    assert np.array_equal(bad == 1, want), (ratio[(bad == 1) != want], bad)
    assert want.sum() >= 10 and (~want).sum() >= 30
    e, h = [], []
    for i in np.flatnonzero(~want):
        e.append(float(mpr.solve_residual(K[i], A[i], D[i])))
        h.append(float(mpr.solve_residual(D[i] @ np.linalg.pinv(A[i]), A[i], D[i])))
    _report("ldl_right_solve4 |K A - D| / |D|", max(e), max(h), _mbound(max(h)))
    assert max(e) <= _mbound(max(h))
