"""Inputs, 50-digit references and host baselines shared by tests/test_mp_reference.py (CPU) and tests/test_math_probe.py
(GPU).  Everything is built once per process (``functools.lru_cache``) and never modified afterwards.

Each scalar case is a ``Case``: the input arrays, the exact values (lists of mpf, one list per output), and the host's
values for the same inputs (plain NumPy float64), from which ``e_host`` -- the host's largest ulp error -- follows.
"""
import functools
import math
import types

import numpy as np

from oracle import mp_reference as mpr

mp, mpf = mpr.mp, mpr.mpf
PI4 = 0.78539816339744828  # the literal of sincos_delta's guard (= the double nearest pi/4)
DEG2RAD = 0.017453292519943295
TWO20 = 1048576.0
SEED = 20260


def _rng(k):
    return np.random.default_rng(SEED + k)


def nxt(x, toward=math.inf):
    return float(np.nextafter(x, toward))


def _case(name, in0, exact, host, in1=None, **extra):
    in0 = np.asarray(in0, dtype=np.float64)
    e_host = []
    for ex, h in zip(exact, host):
        sel = [i for i, v in enumerate(ex) if v is not None]
        e_host.append(float(np.max(mpr.ulp_errors(np.asarray(h)[sel], [ex[i] for i in sel]))))
    c = types.SimpleNamespace(name=name, in0=in0, in1=None if in1 is None else np.asarray(in1, dtype=np.float64),
                              exact=exact, host=host, e_host=e_host, **extra)
    for a in (c.in0, c.in1):
        if a is not None:
            a.setflags(write=False)
    return c


def max_ulp(got, exact, where=None):
    """Largest ulp error of ``got`` against the exact list (entries that are None, or where ``where`` is False, skipped)."""
    got = np.asarray(got)
    sel = [i for i, v in enumerate(exact) if v is not None and (where is None or where[i])]
    return float(np.max(mpr.ulp_errors(got[sel], [exact[i] for i in sel])))


def same_bits(a, b):
    """Equal bit for bit, sign of zero included; NaN equals NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------------------------------------------------------
# floored_mod360 / wrap180: the expectation is NumPy itself, bit for bit
# ------------------------------------------------------------------------------------------------------------------
_EPS = [0.0, 2.0**-46, -(2.0**-46), 2.0**-45, -(2.0**-45), 2.0**-44, -(2.0**-44), 1e-13, -1e-13]


@functools.lru_cache(None)
def mod360_inputs():
    r = _rng(1)
    ks = list(range(-6, 7)) + [-1000, 1000, -12345, 12345, 2777777, -2777777]
    near = [360.0 * k + e for k in ks for e in _EPS]
    special = [0.0, -0.0, 5e-324, -5e-324, -1e-300, 1e-300, -1e-20, 1e-20, -1e-14, -5e-14, 360.0, -360.0, nxt(360.0, 0), nxt(360.0),
               nxt(-360.0, 0), nxt(-360.0, -math.inf), 1e15, -1e15, nxt(1e15, 0), nxt(1e15), nxt(-1e15, 0), nxt(-1e15, -math.inf),
               1e300, -1e300, math.inf, -math.inf, math.nan, 180.0, -180.0, 720.0, 359.99999999999994]
    a = np.concatenate([r.uniform(-1e4, 1e4, 700), r.uniform(-1e14, 1e14, 700), near, special])
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def wrap180_inputs():
    r = _rng(2)
    ks = list(range(-6, 7)) + [-1000, 1000, -12345, 12345]
    near = [(360.0 * k - 180.0) + e for k in ks for e in _EPS]
    special = [0.0, -0.0, 5e-324, -5e-324, -1e-300, -1e-20, 1e-20, 180.0, -180.0, nxt(180.0, 0), nxt(180.0), nxt(-180.0, 0),
               nxt(-180.0, -math.inf), 360.0, -360.0, 540.0, -540.0, 1e15, -1e15, nxt(1e15, 0), nxt(1e15), 1e300, math.inf, -math.inf,
               math.nan, -180.0 - 1e-20, -180.00000000000003]
    a = np.concatenate([r.uniform(-1e4, 1e4, 700), r.uniform(-1e14, 1e14, 700), near, special])
    a.setflags(write=False)
    return a


def np_mod360(a):
    with np.errstate(invalid="ignore"):
        return np.mod(np.asarray(a, dtype=np.float64), 360.0)


def np_wrap180(y):
    with np.errstate(invalid="ignore"):
        return np.mod(np.asarray(y, dtype=np.float64) + 180.0, 360.0) - 180.0


# ------------------------------------------------------------------------------------------------------------------
# scalar functions
# ------------------------------------------------------------------------------------------------------------------
def _interval(r, lim, n=1500):
    """Dense values on [-lim, lim], small magnitudes down to the denormals, both ends and the doubles next to them."""
    small = r.choice([-1.0, 1.0], 300) * 10.0 ** r.uniform(-300, 0, 300) * lim
    edges = [lim, -lim, nxt(lim, 0), nxt(-lim, 0), nxt(lim), nxt(-lim, -math.inf), 0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.5e-308]
    return np.concatenate([r.uniform(-lim, lim, n), small, edges])


def _exponents(r, n=1500):
    """Normal positive doubles with exponents from 1e-300 to 1e300."""
    v = 10.0 ** r.uniform(-300, 300, n)
    return np.concatenate([v, [1e-300, 1e300, 1.0, 2.0, 4.0, 0.5, nxt(1.0, 0), nxt(1.0), nxt(2.0, 0), nxt(4.0, 0), 3.0, 1e-150, 1e150]])


@functools.lru_cache(None)
def sincos_kernel_case():
    x = _interval(_rng(3), PI4)
    return _case("sincos_kernel", x, [[mpr.sin(v) for v in x], [mpr.cos(v) for v in x]], [np.sin(x), np.cos(x)])


@functools.lru_cache(None)
def atan_small_case():
    x = _interval(_rng(4), 0.4375)
    return _case("atan_small", x, [[mpr.atan(v) for v in x]], [np.arctan(x)])


@functools.lru_cache(None)
def asin_small_case():
    x = _interval(_rng(5), 0.5)
    return _case("asin_small", x, [[mpr.asin(v) for v in x]], [np.arcsin(x)])


@functools.lru_cache(None)
def rsqrt_case():
    x = _exponents(_rng(6))
    return _case("rsqrt_fast", x, [[mpr.rsqrt(v) for v in x]], [1.0 / np.sqrt(x)])


@functools.lru_cache(None)
def div_pos_case():
    r = _rng(7)
    b = _exponents(r)
    a = b * r.choice([-1.0, 1.0], len(b)) * 10.0 ** r.uniform(-3, 3, len(b))  # quotients of ordinary size
    a[:4] = [0.0, -0.0, b[2], -b[3]]
    return _case("div_pos", a, [[mpr.div(u, v) for u, v in zip(a, b)]], [a / b], in1=b)


@functools.lru_cache(None)
def div_earth_radius_case():
    r = _rng(8)
    a = np.concatenate([r.choice([-1.0, 1.0], 1500) * 10.0 ** r.uniform(-8, 8, 1500), [0.0, -0.0, 6378.137, 1.0, 1e-300, 1e300, 5e-324]])
    return _case("div_earth_radius", a, [[mpr.div(v, 6378.137) for v in a]], [a / 6378.137])


@functools.lru_cache(None)
def rcp_refined_case():
    r = _rng(9)
    d = _exponents(r)
    d = d * r.choice([-1.0, 1.0], len(d))
    return _case("rcp_refined", d, [[mpr.div(1.0, v) for v in d]], [1.0 / d])


@functools.lru_cache(None)
def near_multiples_of_half_pi():
    """The doubles nearest k pi/2 for every k up to 2^20 * 2/pi, and how far each lies from k pi/2 (exact integers scaled by
    2^200).  Returned: (x[k-1], order of k by closeness)."""
    with mp.workdps(90):
        p = int(mp.floor(mp.pi / 2 * mpf(2) ** 200))
    kmax = int(TWO20 * 2 / math.pi)
    xs, res = np.empty(kmax), np.empty(kmax)
    for k in range(1, kmax + 1):
        v = k * p
        x = math.ldexp(float(v), -200)  # int -> float rounds to nearest, ldexp is exact
        xs[k - 1] = x
        res[k - 1] = float(abs(v - int(math.ldexp(x, 200))))
    return xs, np.argsort(res)


@functools.lru_cache(None)
def sincos_fast_case():
    r = _rng(10)
    xs, order = near_multiples_of_half_pi()
    pick = np.unique(np.concatenate([np.arange(64), order[:150], r.choice(len(xs), 500, replace=False)]))
    near = xs[pick]
    deg = np.array([0.0, 90.0, 180.0, 270.0, 360.0, 3600.0, 2610.0, 45.0, 135.0]) * DEG2RAD
    edge = [nxt(TWO20, 0), TWO20, nxt(TWO20), 1e7, 1e15, 1e22, 0.0, -0.0, 5e-324, 1e-310]
    x = np.concatenate([near, -near[::7], deg, -deg, r.uniform(-TWO20, TWO20, 600), r.uniform(-10, 10, 300), edge, [-v for v in edge]])
    fast = np.abs(x) < TWO20  # where sincos_fast_n's verdict must be true
    return _case("sincos_fast", x, [[mpr.sin(v) for v in x], [mpr.cos(v) for v in x]], [np.sin(x), np.cos(x)], ok=fast)


@functools.lru_cache(None)
def sincos_delta_case():
    r = _rng(11)
    edge = [PI4, nxt(PI4, 0), nxt(PI4), 0.79, 1.0, 1.5707963267948966, 3.0, 10.0, 100.0, 0.0, 5e-324, 1e-310]
    x = np.concatenate([r.uniform(-PI4, PI4, 1200), r.choice([-1.0, 1.0], 200) * 10.0 ** r.uniform(-300, 0, 200) * PI4,
                        r.uniform(-10, 10, 200), edge, [-v for v in edge]])
    return _case("sincos_delta", x, [[mpr.sin(v) for v in x], [mpr.cos(v) for v in x]], [np.sin(x), np.cos(x)],
                 ok=np.abs(x) <= PI4)


@functools.lru_cache(None)
def atan2_case():
    r = _rng(12)
    b = r.uniform(0.05, 1.0, 1500)
    a = b * r.uniform(-0.4375, 0.4375, 1500)
    ea, eb = [], []
    for bb in (1.0, 0.5, 0.75, 3.0):  # 0.4375 b is exact for these: the guard |a| <= 0.4375 b flips between neighbours
        t = 0.4375 * bb
        for aa in (t, nxt(t, 0), nxt(t), -t, nxt(-t, 0), nxt(-t, -math.inf)):
            ea.append(aa)
            eb.append(bb)
    for aa, bb in ((0.3, -1.0), (-0.3, -1.0), (0.3, 0.0), (-0.3, 0.0), (0.0, 1e-300), (1e-301, 1e-300), (0.0, nxt(1e-300)),
                   (1e-301, nxt(1e-300)), (2.0, 1.0), (-2.0, 1.0), (1.0, 1.0), (1e-300, 1.0), (0.0, 1.0), (-0.0, 1.0), (5e-324, 1.0),
                   (1.0, 1e-5), (0.0, -1.0), (1e-3, 1e3), (-1e300, 1e300), (0.44, 1.0), (-0.45, 1.0), (0.47, 1.0), (-0.5, 1.0),
                   (0.3, 0.5), (0.16, 0.35), (-0.55, 1.0)):  # the last rows: a band outside the guard where the polynomial is no longer good
        ea.append(aa)
        eb.append(bb)
    a, b = np.concatenate([a, ea]), np.concatenate([b, eb])
    fast = (b > 1e-300) & (np.abs(a) <= 0.4375 * b)  # 0.4375 b is exact here or far from |a|
    return _case("atan2_fast", a, [[mpr.atan2(u, v) for u, v in zip(a, b)]], [np.arctan2(a, b)], in1=b, fast=fast)


# ------------------------------------------------------------------------------------------------------------------
# geodetic_finish.  Inputs come as angles (lon, lat, course, arc in radians); the eight arguments of the device function are
# those two angles and the host's float64 sines and cosines.  The exact value is the great-circle step of the ANGLES, and the
# host's value NumPy's float64 evaluation of the reference's formulas, so both sides pay for the rounded sines and cosines.
# Rows built from sines and cosines directly (a guard exactly at its limit, the pole) are compared with the formulas applied
# to those values; they are chosen so that sin(lat') alone fixes the latitude.
# ------------------------------------------------------------------------------------------------------------------
def _pack(lon, lat, al, de):
    return np.array([lon, lat, np.sin(lat), np.cos(lat), np.sin(al), np.cos(al), np.sin(de), np.cos(de)])


def np_geodetic_finish(g):
    lon, lat, sp, cp, sa, ca, sd, cd = g
    with np.errstate(invalid="ignore"):
        lon2 = np.degrees(lon + np.arctan2(sd * sa, cp * cd - sp * sd * ca))
        lat2 = np.degrees(np.arcsin(sp * cd + cp * sd * ca))
    return lon2, lat2


@functools.lru_cache(None)
def geodetic_case():
    """Returns the case plus, per row, the expected verdict of the N-wide forms (None where a guard is too close to call on
    the host) and a label for the edge rows."""
    r = _rng(13)
    # ships: up to 60 degrees of latitude, any course, steps up to 0.1 rad (640 km); polar: 85 to 89.9 degrees, steps up to
    # 1e-4 rad -- every fast path applies to both.  A result much smaller than its input (a step that lands next to the
    # equator or the prime meridian) is a cancellation whose size is luck on either side; such rows are left out, so that
    # the largest error says something about the arithmetic and not about one draw.
    cols, exact_lon, exact_lat, ok, label = [], [], [], [], []
    for name, n, lat_lo, lat_hi, de_hi in (("ship", 1000, 0.0, 60.0, -1.0), ("polar", 200, 85.0, 89.9, -4.0)):
        lon = np.radians(r.uniform(-180, 180, 2 * n))
        lat = np.radians(r.choice([-1.0, 1.0], 2 * n) * r.uniform(lat_lo, lat_hi, 2 * n))
        al = np.radians(r.uniform(0, 360, 2 * n))
        de = r.choice([-1.0, 1.0], 2 * n) * 10.0 ** r.uniform(-8, de_hi, 2 * n)
        kept = 0
        for i in range(2 * n):
            e = mpr.great_circle(lon[i], lat[i], al[i], de[i])
            if kept == n or abs(e[0]) < 90 / math.pi * abs(lon[i]) or abs(e[1]) < 90 / math.pi * abs(lat[i]):
                continue
            kept += 1
            cols.append(_pack(lon[i:i + 1], lat[i:i + 1], al[i:i + 1], de[i:i + 1]))
            exact_lon.append(e[0]), exact_lat.append(e[1]), ok.append(True), label.append(name)
        assert kept == n

    def add_angles(name, lo, la, a, d, verdict):
        cols.append(_pack(np.array([lo]), np.array([la]), np.array([a]), np.array([d])))
        e = mpr.great_circle(lo, la, a, d)
        exact_lon.append(e[0]), exact_lat.append(e[1]), ok.append(verdict), label.append(name)

    def add_values(name, g, verdict):
        cols.append(np.array(g, dtype=np.float64).reshape(8, 1))
        e = mpr.great_circle_from_sincos(*g)
        exact_lon.append(e[0]), exact_lat.append(e[1]), ok.append(verdict), label.append(name)

    d30 = math.asin(0.5)
    # both sides of |xs| = 0.5: due north from 10 N by 30 degrees -/+ 1e-9 rad (1e7 times the rounding of xs)
    add_angles("xs<0.5", 0.3, math.radians(10), 0.0, d30 - 1e-9, True)
    add_angles("xs>0.5", 0.3, math.radians(10), 0.0, d30 + 1e-9, False)
    add_angles("xs<-0.5", 0.3, math.radians(10), math.pi, d30 + 1e-9, False)
    # |a| > 0.4375 b with everything else fine: due east on the equator by 25 degrees (tan 25 = 0.466)
    add_angles("a>0.4375b", 0.1, 0.0, math.pi / 2, math.radians(25), False)
    add_angles("a<0.4375b", 0.1, 0.0, math.pi / 2, math.radians(23), True)
    # b <= 0 (and cd <= 0): 100 degrees due east on the equator
    add_angles("b<0", 0.1, 0.0, math.pi / 2, math.radians(100), False)
    # cd <= 0 alone: 160 degrees due south from 80 N lands on 80 S; sin(lat' - lat) = -0.34 passes the |xs| test and
    # b = 0.17 > 0, so only the sign of cos(arc) tells that the identity lat + asin(xs) does not apply (the header's sin 150
    # case: 150 degrees itself sits on |xs| = 0.5)
    add_angles("cd<0 only", 0.1, math.radians(80), math.pi, math.radians(160), False)
    add_angles("150 degrees", 0.1, math.radians(80), math.pi, math.radians(150) + 1e-6, False)
    # the guard of the arctangent exactly at its limit: sp = 0, cp = 1, sa = 1, ca = 0 make a = sd and b = cd exactly
    for cd in (1.0, 0.5, 0.75):
        t = 0.4375 * cd
        add_values("a=0.4375b", [0.2, 0.0, 0.0, 1.0, 1.0, 0.0, t, cd], True)
        add_values("a=0.4375b+", [0.2, 0.0, 0.0, 1.0, 1.0, 0.0, nxt(t), cd], False)
        add_values("-a=0.4375b+", [0.2, 0.0, 0.0, 1.0, 1.0, 0.0, nxt(-t, -math.inf), cd], False)
    # b = 1e-300 (not above the limit), the next double (above it, but h2 = b^2 underflows to 0), b = 0 at the pole
    add_values("b=1e-300", [0.2, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1e-300], False)
    add_values("h2=0", [0.2, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, nxt(1e-300)], False)
    add_values("pole", [0.2, math.pi / 2, 1.0, 0.0, 0.6, 0.8, 0.0, 1.0], False)
    add_values("cd=0", [0.2, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0], False)
    g = np.concatenate(cols, axis=1)
    host = np_geodetic_finish(g)
    c = _case("geodetic_finish", g, [exact_lon, exact_lat], list(host), ok=np.array(ok), label=label)
    return c


# ------------------------------------------------------------------------------------------------------------------
# 4 x 4 symmetric matrices with known spectra
# ------------------------------------------------------------------------------------------------------------------
def _orth(r):
    q, rr = np.linalg.qr(r.normal(size=(4, 4)))
    return q * np.sign(np.diag(rr))


def _from_spectrum(r, w):
    q = _orth(r)
    a = (q * np.asarray(w, dtype=np.float64)) @ q.T
    return 0.5 * (a + a.T)


@functools.lru_cache(None)
def matrix_classes():
    """dict: class name -> (count, 4, 4) symmetric matrices.  Every array is read-only."""
    from track_estimators import synthetic

    r = _rng(20)
    H, Q, R, P0 = synthetic.example_matrices()
    out = {}
    ex = [np.asarray(m, dtype=np.float64) for m in (P0, Q, R + np.diag([0, 0, 1e-6, 1e-6]), P0 + Q)]
    for k in range(12):  # of that kind: dominant diagonals of very different sizes, small couplings
        d = 10.0 ** r.uniform(-6, 1, 4)
        c = r.uniform(-0.3, 0.3, (4, 4))
        c = 0.5 * (c + c.T)
        np.fill_diagonal(c, 1.0)
        ex.append(c * np.sqrt(np.outer(d, d)))
    out["example"] = np.array(ex)
    for name, cond in (("cond1", 1.0), ("cond1e4", 1e4), ("cond1e8", 1e8), ("cond1e12", 1e12)):
        ms = []
        for k in range(12):
            w = np.concatenate([[1.0, 1.0 / cond], 10.0 ** r.uniform(-math.log10(cond), 0, 2)]) * 10.0 ** r.uniform(-3, 3)
            ms.append(_from_spectrum(r, w))
        out[name] = np.array(ms)
    out["repeated"] = np.array([np.eye(4), 3.5 * np.eye(4)] + [_from_spectrum(r, w) for w in
                               ([2, 2, 1, 1], [1, 1, 1, 0.25], [5, 1, 1, 1], [2, 2, 2, 2], [1e-3, 1e-3, 4, 4], [7, 7, 7, 0.5])])
    out["diagonal"] = np.array([np.diag(d) for d in ([1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 2.0, 1.0], [1e-8, 1.0, 1e8, 5.0], [2.0, 2.0, 2.0, 2.0],
                                                     [0.0, 1.0, 0.0, 3.0], [1e-300, 1.0, 1e-3, 7.0])])
    # one negative eigenvalue: -1e-10 of the largest (flagged: below -1e-12 max|diag|) and -1e-14 (clamped silently)
    out["negative_flagged"] = np.array([_from_spectrum(r, [1.0, 0.5, 0.25, -1e-10]) * s for s in (1.0, 1e-4, 1e3, 7.0, 0.3, 42.0)]
                                       + [_from_spectrum(r, [1.0, 0.3, 0.2, -0.1])])
    out["negative_silent"] = np.array([_from_spectrum(r, [1.0, 0.5, 0.25, -1e-14]) * s for s in (1.0, 1e-4, 1e3, 7.0, 0.3, 42.0)])
    out["rank2"] = np.array([_from_spectrum(r, [1.0, 0.5, 0.0, 0.0]) * s for s in (1.0, 1e-4, 1e3, 7.0, 0.3, 42.0)])
    out["rank3"] = np.array([_from_spectrum(r, [1.0, 0.5, 0.1, 0.0]) * s for s in (1.0, 1e-4, 1e3, 7.0, 0.3, 42.0)])
    blk = []
    for k in range(12):
        w = np.array([1.0, 10.0 ** r.uniform(-4, 0)]) * 10.0 ** r.uniform(-3, 3)
        t = r.uniform(0, 2 * math.pi)
        q2 = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
        m = np.zeros((4, 4))
        m[:2, :2] = (q2 * w) @ q2.T
        m[0, 1] = m[1, 0] = 0.5 * (m[0, 1] + m[1, 0])
        blk.append(m)
    for b2 in ([[1.0, 1.0], [1.0, 1.0]], [[2.0, 0.0], [0.0, 0.5]], [[1e-5, 0.0], [0.0, 3e-5]], [[4.0, 2.0], [2.0, 1.0]], [[1.0, 0.5], [0.5, 1.0]]):
        m = np.zeros((4, 4))
        m[:2, :2] = b2
        blk.append(m)
    out["block2"] = np.array(blk)
    for v in out.values():
        v.setflags(write=False)
    return out


SPD_CLASSES = ("example", "cond1", "cond1e4", "cond1e8", "cond1e12", "repeated")


@functools.lru_cache(None)
def warm_cases():
    """(A, V) pairs for the warm start: V is the float64 eigenvector basis of A + t E for t = 1e-3 and 1e-9 (relative to
    |A|), and that basis with its columns permuted.  Returns dict name -> (A (n,4,4), V (n,4,4))."""
    r = _rng(21)
    mc = matrix_classes()
    base = np.concatenate([mc["example"][:6], mc["cond1e4"][:6], mc["repeated"][2:6]])
    out = {}
    for name, t in (("perturbed 1e-3", 1e-3), ("perturbed 1e-9", 1e-9)):
        vs = []
        for a in base:
            e = r.normal(size=(4, 4))
            e = 0.5 * (e + e.T) * np.max(np.abs(a)) * t
            vs.append(np.linalg.eigh(a + e)[1])
        out[name] = (base, np.array(vs))
    out["permuted"] = (base, out["perturbed 1e-9"][1][:, :, [2, 0, 3, 1]].copy())
    for a, v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def ldl_cases():
    """SPD matrices A, right-hand sides D, and per matrix the exact ratio (smallest |pivot| of the unpivoted L D L^T) /
    (largest diagonal entry).  The last rows are built to sit at ratios 1e-6 and 1e-8, either side of kLdlPivotTol = 1e-7, and
    one holds a NaN."""
    r = _rng(22)
    mc = matrix_classes()
    A = [m for k in SPD_CLASSES for m in mc[k][:8]]
    for ratio in (1e-6, 1e-8, 3e-7, 3e-8):
        L = np.tril(r.uniform(-0.5, 0.5, (4, 4)), -1) + np.eye(4)
        for pos in (1, 3):
            d = np.ones(4)
            d[pos] = ratio
            A.append((L * d) @ L.T)
    nan_row = np.eye(4)
    nan_row[1, 2] = nan_row[2, 1] = math.nan
    A.append(nan_row)
    A = np.array([0.5 * (a + a.T) for a in A])
    D = r.normal(size=A.shape)
    ratios = []
    for a in A:
        if np.isnan(a).any():
            ratios.append(math.nan)
            continue
        m = mpr.mat(a)
        piv = []
        for j in range(4):  # unpivoted elimination, exact to 50 digits
            piv.append(m[j, j])
            if m[j, j] == 0:
                piv += [mpf(0)] * (3 - j)
                break
            for i in range(j + 1, 4):
                f = m[i, j] / m[j, j]
                for c in range(4):
                    m[i, c] -= f * m[j, c]
        ratios.append(float(min(abs(p) for p in piv) / max(abs(a[i, i]) for i in range(4))))
    A.setflags(write=False), D.setflags(write=False)
    return A, D, np.array(ratios)
