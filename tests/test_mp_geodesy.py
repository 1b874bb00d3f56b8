"""The 50-digit direct geodesic (oracle/mp_geodesy.py) on its own, and the HOST leg functions held to it.  CPU only.

1. The reference against facts that do not come from this project: an equatorial leg of lambda degrees is a lambda long; the
   WGS84 meridian quadrant is 10 001 965.7293 m; a start at a pole (stated analytically in the module) agrees with the
   general formulas walked back to the pole; the published (s12, azi1) of geographiclib's hard cases
   (tests/test_geodesic_karney.py::KNOWN) land on their point 2 to the precision published.
2. The host solver (track_estimators/geodesic.py through utils.geographiclib_distance / _heading, the functions the product
   calls) over every family of tests/geodesy_cases.py: the landing miss stays within 20 nm, and (0, 0) is returned exactly inside
   the zero square.  Measured here (worst over all families): 5.7e-9 m.
3. NumPy's evaluation of the sphere formulas (utils.haversine_formula / heading) over the sphere families: within the bound
   their own conditioning gives (geodesy_cases.numpy_sphere_bound_m); its worst miss per family is the yardstick the device is
   held to in tests/test_geodesy_landing.py.

Run with ``-s`` to see the worst miss per family and image.
"""
import math

import geodesy_cases as gc
import pytest
from test_geodesic_karney import KNOWN

from oracle import mp_geodesy as mg
from track_estimators import geodesic

mp, mpf = mg.mp, mg.mpf


# ----------------------------------------------------------------------------------------------------------------
# the reference on its own
# ----------------------------------------------------------------------------------------------------------------
def test_context_has_fifty_digits():
    assert mp.dps == 50


@pytest.mark.parametrize("lon1,lam,azi", [(0.0, 1.0, 90.0), (-30.0, 130.0, 90.0), (12.5, 179.9999, 90.0), (100.0, 75.0, 270.0),
                                          (359.5, 400.0, 90.0)])
def test_reference_equator_is_a_circle_of_radius_a(lon1, lam, azi):
    """The equator is a geodesic of radius a: lambda degrees of it are a lambda long (any lambda: the direct problem does not
    ask for the shortest way)."""
    s = mg.WGS84_A * mpf(lam) * mp.pi / 180
    lat2, lon2 = mg.direct_wgs84(0.0, lon1, azi, s)
    want = mpf(lon1) + (lam if azi == 90.0 else -lam)
    turns = (lon2 - want) / 360  # direct_wgs84 returns the longitude modulo 360
    assert abs(lat2) < mpf(10) ** -40 and abs(turns - mp.nint(turns)) < mpf(10) ** -40
    assert mg.landing_miss_m("wgs84", lon1, 0.0, float(want), 0.0, s / 1000, azi) < mpf(10) ** -30
    # and on the sphere, with its radius
    s = mg.SPHERE_R_M * mpf(lam) * mp.pi / 180
    assert mg.landing_miss_m("sphere", lon1, 0.0, float(want), 0.0, s / 1000, azi) < mpf(10) ** -30


def test_reference_meridian_quadrant():
    """Equator to pole along any meridian: 10 001 965.7293 m (WGS84; the figure is published to a tenth of a millimetre)."""
    q = mpf("10001965.7293")
    for lon in (0.0, 17.0, -133.0):
        lat2, _ = mg.direct_wgs84(0.0, lon, 0.0, q)
        # metres along the meridian left to the pole: its radius of curvature there is a^2 / b
        left = (90 - lat2) * mp.pi / 180 * mg.WGS84_A**2 / mg.WGS84_B
        assert abs(left) < mpf("0.5e-4"), left
        for pole_lat, back in ((90.0, 180.0), (-90.0, 0.0)):  # from a pole to the equator: the analytic start
            lat2, lon2 = mg.direct_wgs84(pole_lat, lon, back, q)
            turns = (lon2 - lon) / 360
            assert abs(lat2) * mp.pi / 180 * mg.WGS84_B < mpf("1e-4") and abs(turns - mp.nint(turns)) < mpf(10) ** -40
    # the sphere's quadrant is pi R / 2
    lon2, lat2 = mg.direct_sphere(5.0, 0.0, 0.0, mg.SPHERE_R_M * mp.pi / 2 / 1000)
    assert abs(lat2 - 90) < mpf(10) ** -20


@pytest.mark.parametrize("pole_lat,lon1,azi1,s12", [(90.0, 13.0, 143.0, 7789599.4751), (-90.0, -133.0, 37.0, 12214331.98),
                                                    (90.0, 0.0, 180.0, 111.7), (90.0, 77.0, 300.0, 1.9e7),
                                                    (-90.0, 5.0, 0.0, 20003931.4586)])
def test_reference_pole_start_agrees_with_the_general_formulas(pole_lat, lon1, azi1, s12):
    """direct_wgs84 states a start at a pole analytically (the meridian lon1 + 180 - azi1 from the north pole, lon1 + azi1 from
    the south pole).  The point it reaches, walked back the same distance along that meridian by the general formulas, is the
    pole; and the meridian is the one stated."""
    lat2, lon2 = mg.direct_wgs84(pole_lat, lon1, azi1, s12)
    meridian = lon1 + 180.0 - azi1 if pole_lat > 0 else lon1 + azi1
    d = (lon2 - meridian) / 180
    past = abs(d - mp.nint(d)) < mpf(10) ** -40 and int(mp.nint(d)) % 2 == 1  # beyond the other pole: the far meridian
    assert abs(d - mp.nint(d)) < mpf(10) ** -40
    if abs(lat2) > 90 - mpf(10) ** -20:
        return  # pole to pole: there is no way back by azimuth
    # heading back to the pole it came from: north (0) or south (180) -- unless it went over the other pole
    back = (0.0 if pole_lat > 0 else 180.0) if not past else (180.0 if pole_lat > 0 else 0.0)
    sb, cb, _ = mg._landing_wgs84(lat2, lon2, back, s12)
    assert abs(cb) < mpf(10) ** -40 and (sb > 0) == (pole_lat > 0)


@pytest.mark.parametrize("pts,want,tol", [k for k in KNOWN if k[1][1] is not None], ids=lambda v: None)
def test_reference_lands_the_published_solutions(pts, want, tol):
    """geographiclib's published (s12, azi1), fed to the direct problem, land on point 2 within what their published digits
    allow: the tolerance of s12 plus that of azi1 across the leg (the reduced length of a geodesic is at most a)."""
    lat1, lon1, lat2, lon2 = pts
    miss = mg.landing_miss_m("wgs84", lon1, lat1, lon2, lat2, mpf(want[0]) / 1000, want[1])
    allowed = tol[0] + math.radians(tol[1]) * 6378137.0
    print(f"\n[landing] published {pts}: miss {float(miss):.3e} m, allowed {allowed:.3e} m")
    assert miss <= allowed


# ----------------------------------------------------------------------------------------------------------------
# the host solver, through the functions the product calls
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", gc.FAMILY_NAMES)
def test_host_wgs84_lands_within_20nm(family):
    legs = gc.family_legs(family)
    outs = [gc.host_leg("wgs84", leg) for _, leg in legs]
    for (_, leg), (d, h) in zip(legs, outs):
        if gc.in_zero_square(leg):
            assert d == 0.0 and h == 0.0 and not math.copysign(1.0, d) < 0 and not math.copysign(1.0, h) < 0, leg
        if leg[1] == leg[3] and (leg[0] - leg[2]) % 360.0 == 0.0:  # coincident, however the longitude is written
            assert d == 0.0 and h in (0.0, 180.0), leg
    misses = gc.landing_misses("wgs84", family, outs)
    worst = gc.report("host", "wgs84", family, misses)
    its = sorted({geodesic.inverse(leg[1], leg[0], leg[3], leg[2])[3] for _, leg in legs})
    print(f"          iterations of the solver: {its}")
    assert max(worst) <= gc.WGS84_BOUND_M, [(leg, m) for _, leg, m in misses if m > gc.WGS84_BOUND_M]
    assert max(its) <= 20
    if family == "zero_square":
        assert sum(gc.in_zero_square(leg) for _, leg in legs) == 8 and len(misses) == 12
    if family == "published":
        assert max(its) >= 10  # the slowly converging cases are in


@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_host_returns_nan_for_what_is_not_a_point(model):
    for leg in gc.NAN_LEGS[model]:
        d, h = gc.host_leg(model, leg)
        assert math.isnan(d) and math.isnan(h), (model, leg, d, h)


# ----------------------------------------------------------------------------------------------------------------
# NumPy's sphere formulas: the device's yardstick
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", gc.FAMILY_NAMES)
def test_numpy_sphere_formulas_land_within_their_conditioning(family):
    legs = gc.family_legs(family)
    outs = [gc.host_leg("sphere", leg) for _, leg in legs]
    for (_, leg), (d, h) in zip(legs, outs):
        if gc.coincident(leg):
            assert d == 0.0 and h == 0.0, leg
    misses = gc.landing_misses("sphere", family, outs)
    worst = gc.report("NumPy", "sphere", family, misses)
    dropped = [leg for _, leg in legs if not gc.sphere_checked(leg)]
    print(f"          {len(dropped)} legs beyond {gc.SPHERE_MAX_ARC_DEG} degrees of arc are not held to the landing bound")
    frac = max(m / gc.numpy_sphere_bound_m(leg) for _, leg, m in misses)
    print(f"          worst miss as a fraction of the formulas' conditioning bound: {frac:.3f}")
    assert frac <= 1.0, [(leg, m, gc.numpy_sphere_bound_m(leg)) for _, leg, m in misses if m > gc.numpy_sphere_bound_m(leg)]
    assert max(worst) == gc.numpy_sphere_worst(family)  # the yardstick the GPU tests use is this number


def test_the_families_are_what_the_docstring_says():
    n = {f: len(gc.base_legs(f)) for f in gc.FAMILY_NAMES}
    assert n == {"zero_square": 5, "tiny": 32, "meridional": 12, "equatorial": 7, "seam": 4, "antipodal": 22, "published": 17,
                 "generic": 20}, n
    for f in gc.FAMILY_NAMES:
        assert len(gc.family_legs(f)) == 4 * n[f] <= 128
        arcs = [gc.sphere_arc_deg(leg) for leg in gc.base_legs(f)]
        assert any(a <= gc.SPHERE_MAX_ARC_DEG for a in arcs), f  # every family has sphere legs
    # mirror images and the reversal keep the arc: a leg is dropped from the sphere check in all its images or in none
    for f in gc.FAMILY_NAMES:
        for leg in gc.base_legs(f):
            assert len({gc.sphere_checked(img) for img in gc.images(leg)}) == 1, leg
    arcs = [gc.sphere_arc_deg(leg) for leg in gc.base_legs("antipodal")]
    assert sum(a > 179.0 for a in arcs) == 16 and min(arcs) > 176.0
    tiny = [gc.sphere_arc_deg(leg) for leg in gc.base_legs("tiny")]
    assert min(tiny) > 1.0e-8 and max(tiny) < 1.01e-3 and not any(gc.in_zero_square(leg) for _, leg in gc.family_legs("tiny"))
