"""
50-digit restatements of the device math building blocks and of one UKF step.  TEST INFRASTRUCTURE ONLY.

Every function here states an operation from its DEFINITION in ``mpmath`` arithmetic at 50 significant digits (about 166
bits, against the 53 of a double); none of it transcribes the device code (csrc/ste_math.h), whose polynomials, range
reductions and Jacobi sweeps never appear.  Inputs are doubles and enter exactly (``mp.mpf(float)`` is exact).

  * scalars ............. sin, cos, atan, atan2, asin, 1/sqrt, quotients
  * floored modulo ...... NumPy's ``npy_divmod``: the exact ``fmod`` and, where its sign differs from the divisor's, ONE
                          rounded addition of the divisor; an exact zero takes the divisor's sign.  The rounding is part of
                          the definition, so this one returns a double (exact rational arithmetic, then one ``float``)
  * great-circle step ... src/track_estimators/kalman_filters/non_linear_process.py:46-85 (c = None) of the reference
  * matrices ............ ``mp.eigsy``; principal square root with negative eigenvalues clamped; pseudo-inverse with NumPy's
                          ``rcond = 1e-15`` rule
  * one UKF step ........ predict / update (unscented.py:144-265) and the two robustification terms (:389-478)
  * one smoother step ... unscented.py:285-351 for one k, in the two halves ``urts_gain`` and ``urts_combine``

``ulp_error(got, exact)`` measures a double against such a value in units of the spacing of doubles at the exact value.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

mp = mpmath.mp.clone()  # a context of its own: the precision set here does not leak into other users of mpmath
mp.dps = 50
mpf = mp.mpf

EARTH_RADIUS = mpf("6378.137")  # constants.py:1 (the double 6378.137 is what the code divides by; see geodetic_step)
_R = mpf(6378.137)
_D2R = mp.pi / 180
_R2D = 180 / mp.pi


# --------------------------------------------------------------------------------------------------------------
# measuring
# --------------------------------------------------------------------------------------------------------------
def ulp_error(got, exact_mp) -> float:
    """|got - exact| in units of the spacing of doubles at ``exact`` (2^-1074 below the smallest normal number).
    A non-finite ``got`` is infinitely far from any finite exact value."""
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    exact = mpf(exact_mp)
    if exact == 0:
        e = -1074
    else:
        e = max(mp.frexp(abs(exact))[1] - 53, -1074)  # |exact| = m 2^E with m in [1/2, 1): spacing 2^(E - 53)
    return float(abs(mpf(got) - exact) / mp.ldexp(mpf(1), e))


def ulp_errors(got, exact_list) -> np.ndarray:
    got = np.asarray(got, dtype=np.float64).ravel()
    assert len(got) == len(exact_list)
    return np.array([ulp_error(g, e) for g, e in zip(got, exact_list)])


def to_float(v):
    return float(v)


# --------------------------------------------------------------------------------------------------------------
# scalars
# --------------------------------------------------------------------------------------------------------------
def sin(x):
    return mp.sin(mpf(x))


def cos(x):
    return mp.cos(mpf(x))


def atan(x):
    return mp.atan(mpf(x))


def atan2(y, x):
    return mp.atan2(mpf(y), mpf(x))


def asin(x):
    return mp.asin(mpf(x))


def rsqrt(x):
    return 1 / mp.sqrt(mpf(x))


def div(a, b):
    return mpf(a) / mpf(b)


def floored_mod(a, b=360.0) -> float:
    """``np.mod(a, b)`` for doubles, as ``npy_divmod`` defines it.  Exact rational arithmetic up to the one rounding the
    definition itself contains."""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b) or math.isinf(a) or b == 0.0:
        return math.nan
    if math.isinf(b):  # fmod(a, inf) = a
        return a if (a == 0.0 or (a < 0) == (b < 0)) else b
    r = abs(Fraction(a)) % abs(Fraction(b))  # fmod: magnitude below |b| ...
    if a < 0:
        r = -r  # ... and the sign of a; representable, so float(r) below is exact
    if r == 0:
        return math.copysign(0.0, b)
    if (b < 0) != (r < 0):
        return float(r) + b  # the one rounded operation
    return float(r)


def wrap180(y) -> float:
    """``(y + 180) % 360 - 180`` in double arithmetic (unscented.py:250, :340): three operations, each rounded once."""
    return floored_mod(float(y) + 180.0, 360.0) - 180.0


# --------------------------------------------------------------------------------------------------------------
# great-circle process model
# --------------------------------------------------------------------------------------------------------------
def great_circle(lon_r, lat_r, alpha_r, delta_r):
    """The destination of an arc ``delta_r`` on course ``alpha_r`` from (lon_r, lat_r), all in radians; returns
    (lon', lat') in degrees (non_linear_process.py:64-72)."""
    lon_r, lat_r, alpha_r, delta_r = mpf(lon_r), mpf(lat_r), mpf(alpha_r), mpf(delta_r)
    sd, cd = mp.sin(delta_r), mp.cos(delta_r)
    a = sd * mp.sin(alpha_r)
    b = mp.cos(lat_r) * cd - mp.sin(lat_r) * sd * mp.cos(alpha_r)
    sl = mp.sin(lat_r) * cd + mp.cos(lat_r) * sd * mp.cos(alpha_r)
    return (lon_r + mp.atan2(a, b)) * _R2D, mp.asin(sl) * _R2D


def great_circle_from_sincos(lon_r, lat_r, sp, cp, sa, ca, sd, cd):
    """The same from given sines and cosines (latitude, course, arc).  ``lat_r`` is not used: the latitude follows from
    sin(lat') alone, as the reference writes it."""
    lon_r, sp, cp, sa, ca, sd, cd = (mpf(v) for v in (lon_r, sp, cp, sa, ca, sd, cd))
    a = sd * sa
    b = cp * cd - sp * sd * ca
    sl = sp * cd + cp * sd * ca
    sl = max(min(sl, mpf(1)), mpf(-1))
    return (lon_r + mp.atan2(a, b)) * _R2D, mp.asin(sl) * _R2D


def geodetic_step(x, dt, sog_rate=0.0, cog_rate=0.0):
    """non_linear_process.py:46-85 with c = None; x = [lon deg, lat deg, speed km/h, heading deg] -> list of 4 mpf."""
    lon, lat, u, alpha = (mpf(v) for v in x)
    dt, sog_rate, cog_rate = mpf(dt), mpf(sog_rate), mpf(cog_rate)
    lon2, lat2 = great_circle(lon * _D2R, lat * _D2R, alpha * _D2R, u * dt / _R)
    return [lon2, lat2, u + sog_rate * dt, alpha + cog_rate * dt]


# --------------------------------------------------------------------------------------------------------------
# matrices
# --------------------------------------------------------------------------------------------------------------
def mat(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mpf(float(v)) for v in row] for row in a.reshape(a.shape[0], -1)])


def vec(a):
    return mp.matrix([mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()])


def to_np(m) -> np.ndarray:
    return np.array([[float(m[r, c]) for c in range(m.cols)] for r in range(m.rows)])


def max_abs(m):
    return max(abs(m[r, c]) for r in range(m.rows) for c in range(m.cols))


def eigsy(A):
    """Eigenvalues (ascending, list of mpf) and eigenvector matrix of the symmetric part of A."""
    A = A if isinstance(A, mp.matrix) else mat(A)
    E, Q = mp.eigsy((A + A.T) / 2)
    return [E[i] for i in range(len(E))], Q


def _recompose(Q, f):
    n = Q.rows
    out = mp.zeros(n, n)
    for r in range(n):
        for c in range(r, n):
            out[r, c] = out[c, r] = mp.fsum(Q[r, i] * f[i] * Q[c, i] for i in range(n))
    return out


def sym_sqrt(P, scale=1):
    """Principal square root of scale * sym(P) with negative eigenvalues clamped to zero: the real part of
    ``scipy.linalg.sqrtm`` on a symmetric matrix (unscented.py:95-97).  Returns (T, eigenvalues of scale * P)."""
    P = P if isinstance(P, mp.matrix) else mat(P)
    w, Q = eigsy(P * mpf(scale))
    return _recompose(Q, [mp.sqrt(v) if v > 0 else mpf(0) for v in w]), w


def pinv_sym(S, rcond=1e-15):
    """Moore-Penrose pseudo-inverse of the symmetric part of S with ``np.linalg.pinv``'s cutoff: singular values (the
    |eigenvalues|) not larger than rcond * the largest are dropped.  Returns (S^+, eigenvalues, rank kept)."""
    S = S if isinstance(S, mp.matrix) else mat(S)
    w, Q = eigsy(S)
    cut = mpf(rcond) * max(abs(v) for v in w)
    keep = [abs(v) > cut for v in w]
    return _recompose(Q, [1 / v if k else mpf(0) for v, k in zip(w, keep)]), w, sum(keep)


def orth_defect(V):
    """max |V^T V - I|"""
    V = V if isinstance(V, mp.matrix) else mat(V)
    return max_abs(V.T * V - mp.eye(V.rows))


def sqrt_residual(T, P, scale=1):
    """max |T T - scale P| / max |scale P|  (P with its negative part removed is the caller's business)"""
    T = T if isinstance(T, mp.matrix) else mat(T)
    P = (P if isinstance(P, mp.matrix) else mat(P)) * mpf(scale)
    return max_abs(T * T - P) / max_abs(P)


def pinv_residual(S, Si):
    """max |S S+ S - S| / max |S|"""
    S = S if isinstance(S, mp.matrix) else mat(S)
    Si = Si if isinstance(Si, mp.matrix) else mat(Si)
    return max_abs(S * Si * S - S) / max_abs(S)


def solve_residual(K, A, D):
    """max |K A - D| / max |D|"""
    K, A, D = (m if isinstance(m, mp.matrix) else mat(m) for m in (K, A, D))
    return max_abs(K * A - D) / max_abs(D)


# --------------------------------------------------------------------------------------------------------------
# one UKF step
# --------------------------------------------------------------------------------------------------------------
def sigma_weights(n=4):
    w0 = 1 - mpf(n) / 3
    return w0, (1 - w0) / (2 * n)


def sigma_points(x, P, scale, info=None):
    """unscented.py:95-105: the 2n + 1 points x, x + col_i(T), x - col_i(T), T = sqrtm(scale P) -> list of lists.
    ``info`` (a dict), where given, receives the eigenvalues of scale * P as ``eig_P``."""
    x = [v if isinstance(v, mpf) else mpf(float(v)) for v in (x if isinstance(x, list) else np.asarray(x).ravel())]
    n = len(x)
    T, w = sym_sqrt(P, scale)
    if info is not None:
        info["eig_P"] = w
    pts = [list(x)]
    pts += [[x[r] + T[r, i] for r in range(n)] for i in range(n)]
    pts += [[x[r] - T[r, i] for r in range(n)] for i in range(n)]
    return pts


def ukf_predict(x, P, Q, dt, sog_rate, cog_rate, noise=None, info=None):
    """unscented.py:178-207 for n = 4.  Returns (x_pred list of 4 mpf, P_pred 4 x 4 mp.matrix).  ``x`` and ``P`` may be
    doubles or values of this module's context (the output of another step); ``info``: see ``sigma_points``."""
    n = 4
    w0, wi = sigma_weights(n)
    sig = [geodetic_step(p, dt, sog_rate, cog_rate) for p in sigma_points(x, P, n / (1 - w0), info)]
    wts = [w0] + [wi] * (2 * n)
    xp = [mp.fsum(w * s[c] for w, s in zip(wts, sig)) for c in range(n)]
    if noise is not None:
        xp = [v + mpf(float(e)) for v, e in zip(xp, np.asarray(noise).ravel())]
    Qm = Q if isinstance(Q, mp.matrix) else mat(Q)
    Pp = mp.zeros(n, n)
    for r in range(n):
        for c in range(n):
            Pp[r, c] = mp.fsum(w * (s[r] - xp[r]) * (s[c] - xp[c]) for w, s in zip(wts, sig)) + Qm[r, c]
    return xp, Pp


def _mod360(v):
    return v - 360 * mp.floor(v / 360)


def ukf_update(x, P, H, R, z, noise=None, info=None):
    """unscented.py:219-265 (linear update, pinv gain, heading wraps, Joseph form).  Returns (x list, P mp.matrix).
    ``x`` and ``P`` may be doubles or values of this module's context (the output of ``ukf_predict``); ``info`` (a dict),
    where given, receives the eigenvalues of S as ``eig_S`` and the new heading before its reduction mod 360 as
    ``heading_unwrapped``."""
    n = 4
    xv = mp.matrix(list(x)) if isinstance(x, list) else vec(x)
    zv = vec(z)
    if noise is not None:
        zv = zv + vec(noise)
    Pm = P if isinstance(P, mp.matrix) else mat(P)
    Hm, Rm = mat(H), mat(R)
    S = Hm * Pm * Hm.T + Rm
    Si, w, _ = pinv_sym(S)
    if info is not None:
        info["eig_S"] = w
    K = Pm * Hm.T * Si
    y = zv - Hm * xv
    y[3] = _mod360(y[3] + 180) - 180
    xn = xv + K * y
    if info is not None:
        info["heading_unwrapped"] = xn[3]
    xn[3] = _mod360(xn[3])
    A = mp.eye(n) - K * Hm
    Pn = A * Pm * A.T + K * Rm * K.T
    return [xn[i] for i in range(n)], Pn


def urts_gain(xk, Pk, Q, dt, sog_rate, cog_rate, noise=None, info=None):
    """The half of one smoother step that needs the filtered row alone (unscented.py:300-336): the fan of (x_k, P_k), its
    propagation, x_b = the weighted mean (plus ``noise``), P_b centred on x_k -- not on x_b -- plus Q, D between the
    unpropagated deviations about x_k and the propagated deviations about x_b, and K = D pinv(P_b).
    Returns (x_b list of 4 mpf, P_b, K); ``info`` receives ``eig_P`` (of the scaled P_k) and ``eig_Pb``."""
    n = 4
    w0, wi = sigma_weights(n)
    wts = [w0] + [wi] * (2 * n)
    sig0 = sigma_points(xk, Pk, n / (1 - w0), info)
    sig = [geodetic_step(p, dt, sog_rate, cog_rate) for p in sig0]
    xb = [mp.fsum(w * s[c] for w, s in zip(wts, sig)) for c in range(n)]
    if noise is not None:
        xb = [v + mpf(float(e)) for v, e in zip(xb, np.asarray(noise).ravel())]
    x0 = sig0[0]
    Qm = Q if isinstance(Q, mp.matrix) else mat(Q)
    Pb, D = mp.zeros(n, n), mp.zeros(n, n)
    for r in range(n):
        for c in range(n):
            Pb[r, c] = mp.fsum(w * (s[r] - x0[r]) * (s[c] - x0[c]) for w, s in zip(wts, sig)) + Qm[r, c]
            D[r, c] = mp.fsum(w * (a[r] - x0[r]) * (s[c] - xb[c]) for w, a, s in zip(wts, sig0, sig))
    Pi, w, _ = pinv_sym(Pb)
    if info is not None:
        info["eig_Pb"] = w
    return xb, Pb, D * Pi


def urts_combine(xk, Pk, xs_next, Ps_next, xb, Pb, K, info=None):
    """The other half (unscented.py:338-349): the innovation against the smoothed row k + 1 with its heading wrapped to
    +-180, the new heading mod 360, and P_s = P_k + K (P_s,next - P_b) K^T.  ``info`` receives ``heading_unwrapped``."""
    y = vec(xs_next) - mp.matrix(xb)
    y[3] = _mod360(y[3] + 180) - 180
    xs = vec(xk) + K * y
    if info is not None:
        info["heading_unwrapped"] = xs[3]
    xs[3] = _mod360(xs[3])
    Ps = mat(Pk) + K * (mat(Ps_next) - Pb) * K.T
    return [xs[i] for i in range(4)], Ps


def urts_step(xk, Pk, xs_next, Ps_next, Q, dt, sog_rate, cog_rate, noise=None, info=None):
    """One step of the unscented RTS smoother (unscented.py:285-351 for one k, as ``ukf_oracle.backward_track`` restates
    it): from the filtered row k and the smoothed row k + 1 to the smoothed row k.  Returns (x_s list of 4 mpf, P_s)."""
    xb, Pb, K = urts_gain(xk, Pk, Q, dt, sog_rate, cog_rate, noise, info)
    return urts_combine(xk, Pk, xs_next, Ps_next, xb, Pb, K, info)


def robust_terms(x, P, H, R, z):
    """gamma = |y^T S^+ y| (criterion_index, unscented.py:420-428) and denom = y^T S^+ R S^+ y (update_lambda_factor,
    :468-478) with S = H P H^T + R and the reference's y = z - x."""
    y = vec(z) - vec(x)
    Pm, Hm, Rm = mat(P), mat(H), mat(R)
    Si, _, _ = pinv_sym(Hm * Pm * Hm.T + Rm)
    u = Si * y
    return abs((y.T * u)[0]), (u.T * Rm * u)[0]
