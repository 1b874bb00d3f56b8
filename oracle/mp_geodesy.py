"""
The DIRECT geodesic problem at 50 digits, from the definition of a geodesic.  TEST INFRASTRUCTURE ONLY.

A leg function (csrc/ste_geodesy.h on the device, track_estimators/geodesic.py and utils.py on the host) answers the inverse
problem: distance and initial heading from point 1 to point 2.  This module checks such an answer without restating the
solver: it walks the returned distance on the returned heading from point 1 and measures, in metres, how far the landing
point is from point 2 (``landing_miss_m``).  That miss is a chord between two points of the surface: it is well conditioned
everywhere, at the antipode too (where the heading alone is not), and by the triangle inequality it bounds the error of the
returned distance.

WGS84.  On an ellipsoid of revolution (a, f; b = (1 - f) a, e'^2 = (a^2 - b^2) / b^2) a geodesic is a great circle of the
auxiliary sphere: reduced latitude tan(beta) = (1 - f) tan(phi), azimuth alpha0 at the equator with
sin(alpha0) = sin(alpha1) cos(beta1), arc sigma from the northward equator crossing and spherical longitude omega.  Distance
and longitude along it are the two quadratures (Karney 2013, eqs. 7 and 8 before they are expanded into series)

    s / b  = int sqrt(1 + k^2 sin^2 sigma) d sigma                                       k^2 = e'^2 cos^2 alpha0
    lambda = omega - f sin(alpha0) int (2 - f) / (1 + (1 - f) sqrt(1 + k^2 sin^2 sigma)) d sigma

``direct_wgs84`` evaluates them by ``mp.quad`` and finds sigma2 by Newton's method on the first; none of the A / C series,
no lambda12, nothing of the inverse solver appears.  Angles enter as sines and cosines; a start AT a pole is stated
analytically (every geodesic from a pole is a meridian: longitude lon1 + 180 - azi1 from the north pole, lon1 + azi1 from the
south pole) rather than as the limit of a tiny cos(beta1).

Sphere.  ``direct_sphere`` is ``mp_reference.great_circle`` on the 6378.137 km sphere.

Precision: the context works at 50 significant digits (about 166 bits against the 53 of a double) like ``mp_reference``;
inputs are doubles and enter exactly.  ``tests/test_mp_geodesy.py`` checks the module against facts that do not come from
this project (the equator, the meridian quadrant, published solutions).
"""
from __future__ import annotations

from oracle import mp_reference as mpr

mp = mpr.mp  # one context, 50 digits
mpf = mp.mpf

WGS84_A = mpf(6378137)
WGS84_F = 1 / mpf("298.257223563")
WGS84_B = WGS84_A * (1 - WGS84_F)
_F1 = 1 - WGS84_F
_EP2 = WGS84_F * (2 - WGS84_F) / _F1**2
SPHERE_R_M = mpf(6378.137) * 1000  # the double 6378.137 (km) is what the code multiplies by
_D2R = mp.pi / 180
_R2D = 180 / mp.pi
# radians of sigma per panel of the quadrature (Gauss-Legendre; the integrands are analytic for |Im sigma| < 3)
_QUAD_PIECE = mpf("1.7")
_QUAD_TOL = mpf(10) ** -42  # accepted error estimate of a quadrature, relative


def _sincos_deg(x):
    r = mpf(x) * _D2R
    return mp.sin(r), mp.cos(r)


def _unit(x, y):
    r = mp.hypot(x, y)
    return x / r, y / r


def _reduced(lat_deg):
    """sin, cos of the reduced latitude of a geographic latitude in degrees."""
    s, c = _sincos_deg(lat_deg)
    return _unit(_F1 * s, c)


def _quad(fun, a, b, scale=0):
    """int_a^b fun, in panels of at most _QUAD_PIECE; the error estimate must be below _QUAD_TOL of the value (or of
    ``scale``, for a correction to a larger value)."""
    if a == b:
        return mpf(0)
    pieces = int(mp.ceil(abs(b - a) / _QUAD_PIECE)) + 1
    v, err = mp.quad(fun, mp.linspace(a, b, pieces), error=True, method="gauss-legendre")
    if not err <= _QUAD_TOL * max(abs(v), abs(scale)):
        raise ArithmeticError(f"quadrature over [{a}, {b}] did not converge: {v} +- {err}")
    return v


def _arc_for_distance(k2, sig1, s_over_b):
    """sigma2 with int_sig1^sigma2 sqrt(1 + k2 sin^2) = s_over_b: Newton's method, each step integrating only from the
    previous iterate, until the step is below 1e-45 rad (sigma itself is held to 50 digits, so for a short leg the step cannot
    shrink in proportion to the leg; 1e-45 rad is 1e-38 m).  A negative distance walks backwards."""
    w = lambda s: mp.sqrt(1 + k2 * mp.sin(s) ** 2)  # noqa: E731
    sig2 = sig1 + s_over_b / mp.sqrt(1 + k2 / 2)
    have = _quad(w, sig1, sig2)
    for _ in range(12):
        step = (s_over_b - have) / w(sig2)
        if abs(step) <= mpf(10) ** -45:
            return sig2 + step
        have += _quad(w, sig2, sig2 + step, 1)
        sig2 += step
    raise ArithmeticError("sigma2 did not converge")


def _landing_wgs84(lat1, lon1, azi1, s12):
    """-> (sin beta2, cos beta2 SIGNED, lon2 in radians): the point a (cos beta2 cos lon2, cos beta2 sin lon2, (1 - f) sin
    beta2).  A negative cos beta2 only appears for a start at a pole walked past the other pole (it is the far meridian)."""
    lat1, lon1, azi1, s12 = mpf(lat1), mpf(lon1), mpf(azi1), mpf(s12)
    if abs(lat1) > 90:
        raise ValueError("latitude outside [-90, 90]")
    if abs(lat1) == 90:
        # from a pole: along the meridian, theta = arc from the pole; sigma runs from pi/2 with alpha0 = 0
        north = lat1 > 0
        theta = _arc_for_distance(_EP2, mp.pi / 2, s12 / WGS84_B) - mp.pi / 2
        meridian = (lon1 + 180 - azi1) if north else (lon1 + azi1)
        return (mp.cos(theta) if north else -mp.cos(theta)), mp.sin(theta), meridian * _D2R
    sa1, ca1 = _sincos_deg(azi1)
    sb1, cb1 = _reduced(lat1)
    sa0, ca0 = sa1 * cb1, mp.hypot(ca1, sa1 * sb1)
    sig1 = mp.atan2(sb1, ca1 * cb1)
    omg1 = mp.atan2(sa0 * sb1, ca1 * cb1)
    k2 = _EP2 * ca0**2
    sig2 = _arc_for_distance(k2, sig1, s12 / WGS84_B)
    ss2, cs2 = mp.sin(sig2), mp.cos(sig2)
    sb2, cb2 = ca0 * ss2, mp.hypot(sa0, ca0 * cs2)
    omg2 = mp.atan2(sa0 * ss2, cs2)  # omega modulo 2 pi: only sin and cos of the longitude are used downstream
    i3 = _quad(lambda s: (2 - WGS84_F) / (1 + _F1 * mp.sqrt(1 + k2 * mp.sin(s) ** 2)), sig1, sig2)
    lam12 = (omg2 - omg1) - WGS84_F * sa0 * i3
    return sb2, cb2, lon1 * _D2R + lam12


def direct_wgs84(lat1, lon1, azi1, s12):
    """The point reached from (lat1, lon1) [degrees] after s12 metres on initial azimuth azi1 [degrees] on WGS84 ->
    (lat2, lon2) in degrees as mpf; lon2 = lon1 + the longitude travelled modulo 360 (it is not reduced to a range)."""
    sb2, cb2, lon2 = _landing_wgs84(lat1, lon1, azi1, s12)
    if cb2 < 0:  # past the other pole: the far meridian
        cb2, lon2 = -cb2, lon2 + mp.pi
    return mp.atan2(sb2, _F1 * cb2) * _R2D, lon2 * _R2D


def direct_sphere(lon1, lat1, heading, dist_km):
    """The same on the sphere of radius 6378.137 km -> (lon2, lat2) in degrees as mpf (note the argument order: the sphere
    functions of utils.py take longitude first)."""
    return mpr.great_circle(mpf(lon1) * _D2R, mpf(lat1) * _D2R, mpf(heading) * _D2R, mpf(dist_km) * 1000 / SPHERE_R_M)


def _chord(p, q):
    return mp.sqrt(sum((u - v) ** 2 for u, v in zip(p, q)))


def landing_miss_m(model, lon1, lat1, lon2, lat2, dist_km, head_deg):
    """The chord in metres between point 2 and the point reached from point 1 after ``dist_km`` on heading ``head_deg``;
    ``model`` is "wgs84" or "sphere".  Arguments in the order of the leg functions of utils.py."""
    if model == "wgs84":
        sb, cb, lon = _landing_wgs84(lat1, lon1, head_deg, mpf(dist_km) * 1000)
        got = (WGS84_A * cb * mp.cos(lon), WGS84_A * cb * mp.sin(lon), WGS84_B * sb)
        sb, cb = _reduced(lat2)
        sl, cl = _sincos_deg(lon2)
        want = (WGS84_A * cb * cl, WGS84_A * cb * sl, WGS84_B * sb)
    elif model == "sphere":
        lon, lat = direct_sphere(lon1, lat1, head_deg, dist_km)
        pts = []
        for lo, la in ((lon, lat), (mpf(lon2), mpf(lat2))):
            (sl, cl), (sp, cp) = _sincos_deg(lo), _sincos_deg(la)
            pts.append((SPHERE_R_M * cp * cl, SPHERE_R_M * cp * sl, SPHERE_R_M * sp))
        got, want = pts
    else:
        raise ValueError(f"model must be 'wgs84' or 'sphere', got {model!r}")
    return _chord(got, want)
