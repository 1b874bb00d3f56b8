"""
track_estimators.geodesic: the WGS84 inverse problem by Karney's algorithm, the restatement of what the reference's
geographiclib calls compute (/root/reference/src/track_estimators/utils.py:36,68; geographiclib>=2.0 is a third-party
dependency, absent on both boxes, so parity with it cannot be run; the solver is pinned at the nanometre level to the definition
of a geodesic by tests/test_mp_geodesy.py -- its (s12, azi1), walked from point 1 by a 50-digit direct solution
(oracle/mp_geodesy.py), lands within 20 nm of point 2 -- and the device solver likewise by tests/test_geodesy_landing.py).  Pinned
here:

  * the values the reference holds: its utils tests (tests/test_utils.py:36-60,87-100) and the noise-free row 0 of its CLI
    example output -- reproduced to the last bit;
  * agreement with an independent solver (Vincenty's iteration, tests/vincenty_check.py) on 10^5 random legs wherever that
    converges, to Vincenty's own truncation error (~0.1 mm, ~2e-8 deg);
  * symmetry, and the nearly antipodal / meridional / equatorial cases of Karney (2013) section 5, checked through the DIRECT
    problem (Vincenty's direct formula: not iterative, valid at the antipode): the returned (s12, azi1) lands on point 2;
  * known answers of the algorithm's own published test set (GeodSolve cases of geographiclib's test suite, WGS84 ones).
"""
import math
import warnings

import numpy as np
import pytest
from vincenty_check import _WGS84_A, _WGS84_F, vincenty_inverse

from track_estimators import geodesic, utils


def vincenty_direct(lat1, lon1, azi1, s12):
    """Vincenty's direct formula (Survey Review XXIII, 176, 1975): test infrastructure, valid for any distance."""
    a, f = _WGS84_A, _WGS84_F
    b = a * (1 - f)
    al1 = math.radians(azi1)
    sa1, ca1 = math.sin(al1), math.cos(al1)
    tu1 = (1 - f) * math.tan(math.radians(lat1))
    cu1 = 1 / math.sqrt(1 + tu1 * tu1)
    su1 = tu1 * cu1
    sig1 = math.atan2(tu1, ca1)
    sal = cu1 * sa1
    c2al = 1 - sal * sal
    u2 = c2al * (a * a - b * b) / (b * b)
    A = 1 + u2 / 16384 * (4096 + u2 * (-768 + u2 * (320 - 175 * u2)))
    B = u2 / 1024 * (256 + u2 * (-128 + u2 * (74 - 47 * u2)))
    sig = s12 / (b * A)
    for _ in range(100):
        c2sm = math.cos(2 * sig1 + sig)
        ss, cs = math.sin(sig), math.cos(sig)
        dsig = B * ss * (c2sm + B / 4 * (cs * (-1 + 2 * c2sm ** 2) - B / 6 * c2sm * (-3 + 4 * ss ** 2) * (-3 + 4 * c2sm ** 2)))
        new = s12 / (b * A) + dsig
        if abs(new - sig) < 1e-15:
            sig = new
            break
        sig = new
    c2sm = math.cos(2 * sig1 + sig)
    ss, cs = math.sin(sig), math.cos(sig)
    t = su1 * ss - cu1 * cs * ca1
    lat2 = math.atan2(su1 * cs + cu1 * ss * ca1, (1 - f) * math.hypot(sal, t))
    lam = math.atan2(ss * sa1, cu1 * cs - su1 * ss * ca1)
    C = f / 16 * c2al * (4 + f * (4 - 3 * c2al))
    L = lam - (1 - C) * f * sal * (sig + C * ss * (c2sm + C * cs * (-1 + 2 * c2sm ** 2)))
    return math.degrees(lat2), (lon1 + math.degrees(L) + 540) % 360 - 180


def test_reference_held_values():
    """tests/test_utils.py:36-60 (NYC - LA, Porto - Lisbon, rtol 1e-2), :87-100 (Kansas City -> St Louis, rtol 1e-3) and the
    CLI fixture's row 0 (examples/cli_example/output_01203823_predictions.txt: sog = s12 / 24 h, cog = azi1) -- the last to
    the last bit, which no other solver tried here achieves (Vincenty: 8e-13)."""
    assert np.isclose(utils.geographiclib_distance(-74.0060, 40.7128, -118.2437, 34.0522), 3933.96, rtol=1e-2)
    assert np.isclose(utils.geographiclib_distance(-9.13333, 38.7167, -8.6291, 41.1579), 273.59, rtol=1e-2)
    assert np.isclose(utils.geographiclib_heading(-94.581213, 39.099912, -90.200203, 38.627089), 96.51, rtol=1e-3)
    assert utils.geographiclib_distance(-30.5, -0.5, -31.5, -3.5) / 24.0 == 14.578418614021368
    assert utils.geographiclib_heading(-30.5, -0.5, -31.5, -3.5) == 198.52495095065817
    assert utils.geographiclib_distance(12.5, -33.0, 12.5, -33.0) == 0.0 and utils.geographiclib_heading(3.0, 4.0, 3.0, 4.0) == 0.0


# (lat1, lon1, lat2, lon2) -> (s12 m, azi1 deg, azi2 deg); None = not checked.  WGS84 cases of geographiclib's published
# test set (GeodSolve0, 6, 9, 10, 11, 29/33, 59, 74, 76, 78, 92; tolerances as published there)
KNOWN = [
    ((40.6, -73.8, 49.01666667, 2.55), (5853226.0, 53.47022, 111.59367), (0.5, 0.5e-5)),
    ((88.202499451857, 0, -88.202499451857, 179.981022032992859592), (20003898.214, None, None), (0.5e-3, None)),
    ((89.262080389218, 0, -89.262080389218, 179.992207982775375662), (20003925.854, None, None), (0.5e-3, None)),
    ((89.333123580033, 0, -89.333123580032997687, 179.99295812360148422), (20003926.881, None, None), (0.5e-3, None)),
    ((56.320923501171, 0, -56.320923501171, 179.664747671772880215), (19993558.287, None, None), (0.5e-3, None)),
    ((52.784459512564, 0, -52.784459512563990912, 179.634407464943777557), (19991596.095, None, None), (0.5e-3, None)),
    ((48.522876735459, 0, -48.52287673545898293, 179.599720456223079643), (19989144.774, None, None), (0.5e-3, None)),
    ((0, 0, 0, 179), (19926189.0, 90.0, 90.0), (0.5, 0.5e-5)),
    ((0, 0, 0, 179.5), (19980862.0, 55.96650, 124.03350), (0.5, 0.5e-5)),
    ((0, 0, 0, 180), (20003931.0, 0.0, 180.0), (0.5, 0.5e-5)),
    ((0, 0, 1, 180), (19893357.0, 0.0, 180.0), (0.5, 0.5e-5)),
    ((5, 0.00000000000001, 10, 180), (18345191.174332713, 0.000000000000035, 179.99999999999996), (5e-9, 1.5e-14)),
    ((54.1589, 15.3872, 54.1591, 15.3877), (39.527686385, 55.723110355, 55.723515675), (5e-9, 5e-9)),
    ((-(41 + 19 / 60), 174 + 49 / 60, 40 + 58 / 60, -(5 + 30 / 60)), (19960543.857179, 160.39137649664, 19.50042925176), (0.5e-6, 0.5e-11)),
    ((27.2, 0, -27.1, 179.5), (19974354.765767, 45.82468716758, 134.22776532670), (0.5e-6, 0.5e-11)),
    ((37.757540000000006, -122.47018, 37.75754, -122.470177), (0.264, 89.99999923, 90.00000106), (0.5e-3, 1e-7)),
    ((90, 0, -90, 0), (20003931.4586, 180.0, None), (1e-4, 1e-12)),
]


@pytest.mark.parametrize("pts,want,tol", KNOWN)
def test_known_answers_of_the_published_algorithm(pts, want, tol):
    s12, azi1, azi2, it = geodesic.inverse(*pts)
    assert abs(s12 - want[0]) <= tol[0]
    for got, w in ((azi1, want[1]), (azi2, want[2])):
        if w is not None:
            assert abs((abs(got) if abs(w) == 180 else got) - w) <= tol[1]
    assert it <= 20  # Newton, never the bisection tail (Karney 2013: 16 at most over his WGS84 test set)


def test_agrees_with_vincenty_wherever_vincenty_converges():
    """10^5 random legs over the whole globe.  Vincenty's series are truncated at O(f^3): 0.1 mm and 2e-8 deg of its own error
    on 20 000 km legs; Karney's solution is good to 15 nm.  Legs Vincenty cannot solve (nearly antipodal) are skipped here
    and covered by the direct-problem test below."""
    rng = np.random.default_rng(20261004)
    worst_s = worst_a = 0.0
    n = skipped = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for la1, lo1, la2, lo2 in zip(rng.uniform(-89.9, 89.9, 100_000), rng.uniform(-180, 180, 100_000),
                                      rng.uniform(-89.9, 89.9, 100_000), rng.uniform(-180, 180, 100_000)):
            try:
                sv, av = vincenty_inverse(la1, lo1, la2, lo2)
            except RuntimeWarning:
                skipped += 1
                continue
            sk, ak, _, it = geodesic.inverse(la1, lo1, la2, lo2)
            assert it <= 20
            n += 1
            worst_s = max(worst_s, abs(sv - sk))
            worst_a = max(worst_a, abs((av - ak + 180.0) % 360.0 - 180.0) * math.sin(min(sk, 2.0e7 - sk) / 6.4e6))
    assert n > 99_000 and skipped < 1_000
    assert worst_s < 2e-4, worst_s  # metres = 2e-7 km
    assert worst_a < 5e-8, worst_a  # degrees, weighted by sin(arc): the azimuth of a nearly antipodal leg is ill-conditioned


def test_symmetry_and_the_hard_cases_through_the_direct_problem():
    """distance(1 -> 2) = distance(2 -> 1); azi2(1 -> 2) = azi1(2 -> 1) +- 180; and for nearly antipodal, meridional, equatorial
    and polar legs the solution, fed to the direct problem, lands on point 2 (the geodesic need not be unique, the endpoint
    is)."""
    rng = np.random.default_rng(7)
    legs = [(rng.uniform(-80, 80), rng.uniform(-180, 180)) for _ in range(300)]
    cases = []
    for la, lo in legs:  # nearly antipodal: the antipode moved by up to 0.6 deg (inside the astroid)
        cases.append((la, lo, -la + rng.uniform(-0.6, 0.6), lo + 180 + rng.uniform(-0.6, 0.6)))
    cases += [(0.0, 0.0, 0.2, 179.7), (0.0, 0.0, 0.0, 179.9999), (10.0, 20.0, -10.0, -160.0), (30.0, 0.0, -30.0, 179.9),
              (-40.0, 5.0, 60.0, 5.0), (89.9, 0.0, 89.9, 180.0), (0.0, -30.0, 0.0, 100.0), (1e-9, 0.0, -1e-9, 180.0)]
    worst = 0.0
    for la1, lo1, la2, lo2 in cases:
        s12, azi1, azi2, it = geodesic.inverse(la1, lo1, la2, lo2)
        r12, bzi1, bzi2, _ = geodesic.inverse(la2, lo2, la1, lo1)
        assert 0 < s12 < 20_003_932 and it <= 83
        assert abs(s12 - r12) < 1e-7  # metres
        la, lo = vincenty_direct(la1, lo1, azi1, s12)
        worst = max(worst, abs(la - la2), abs((lo - lo2 + 180) % 360 - 180) * math.cos(math.radians(la2)))
    assert worst < 5e-9, worst  # degrees ~ 0.5 mm: the direct formula's own accuracy


def test_ship_track_defaults_use_it(tmp_path):
    """ShipTrack's default distance / heading functions (ship_track.py:20-22) reach the solver; a nearly antipodal leg, which the
    Vincenty fallback of rounds 1-3 could not solve, is an ordinary leg now -- silently."""
    from track_estimators.ship_track import ShipTrack

    st = ShipTrack()
    st.lon, st.lat, st.dts = np.array([0.0, 179.7, 179.9]), np.array([0.0, 0.2, 0.4]), np.array([24.0, 24.0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sog = st.calculate_sog()
    assert np.all(np.isfinite(sog)) and abs(sog[0] * 24.0 - geodesic.inverse(0.0, 0.0, 0.2, 179.7)[0] * 1e-3) < 1e-9
