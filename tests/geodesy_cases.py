"""The legs on which the leg functions (csrc/ste_geodesy.h: sphere_leg, sphere_dist_km, wgs84_leg; on the host
track_estimators/geodesic.py and utils.py) are held to the 50-digit direct solution of oracle/mp_geodesy.py.  Shared by
tests/test_mp_geodesy.py (CPU: the host solver and NumPy's sphere formulas) and tests/test_geodesy_landing.py (GPU).

A leg is (lon1, lat1, lon2, lat2) in degrees, the argument order of utils.py.  Every base leg of a family appears in four
IMAGES -- as given, latitudes mirrored, longitudes mirrored, reversed -- which is what sends it through the three reflections
of wgs84_leg (latsign, lonsign, swapp) and, on the equator, through a negative zero.

Families (``base_legs(name)``; the comments name the branch of wgs84_leg a leg is there for):

  zero_square   the 1e-8 degree square of utils.geographiclib_distance / _heading: both differences just under it (-> exactly
                (0, 0)), one of them just over it (-> a leg of about a millimetre, solved), coincident points, and coincident
                points written 360 degrees apart (359.5 and -0.5: outside the square, so the solver sees a zero leg; it
                returns distance 0 and, as the published algorithm does for coincident points, heading 180 on the northern
                hemisphere and 0 on the southern)
  tiny          arcs of 1.01e-8 .. 1e-3 degrees with 1.9e-6 and 2.3e-6 on either side of the closed-form short line (etol2, about
                3.6e-8 rad = 2.1e-6 degrees of arc), along the meridian, along the parallel and oblique, at latitudes 0, 33.3,
                67.1 and 89.5 (the longitude difference is arc / cos(lat): 115 times the arc at 89.5)
  meridional    equal longitudes; longitudes exactly 180 apart (over the pole); starts at +90 and -90 with an arbitrary lon1;
                pole to pole; 111 m from a pole; (5, 1e-14) -> (10, 180)
  equatorial    both latitudes 0 with longitude differences on either side of (1 - f) 180 = 179.3965: 130, 179.39, 179.40,
                179.5, 179.9999; and (1e-9, 0) -> (-1e-9, 180)
  seam          179.9 -> -179.9, 179.9 -> 180.1, 359.5 -> 0.5, -720.25 -> 721
  antipodal     16 seeded legs with the antipode moved by up to 0.6 degrees, half of them by less than 0.1 cos(lat) degrees
                (well inside the astroid), four moved by 1.2 .. 3 degrees (nearly antipodal still, and short enough for the
                sphere check below), and two on either side of the hand-over from the spherical start to the astroid
  published     the points of tests/test_geodesic_karney.py::KNOWN (geographiclib's published hard cases)
  generic       20 seeded legs over the globe

SPHERE.  The sphere functions are checked on the same families minus the legs whose great-circle arc exceeds 179 degrees
(``sphere_checked``).  Beyond that the reference's own haversine formula loses digits -- sqrt(1 - a) cancels; NumPy misses the
landing point by 0.1 um at 179.0 degrees and by 0.5 mm at 179.9999 -- and that loss is the formula's, which the device
reproduces operation for operation: those legs stay with the device-against-NumPy tests of tests/test_track_prep.py and
tests/test_path_metrics.py.  The arc is decided here by the vector formula atan2(|p1 x p2|, p1 . p2), which has no such
cancellation, not by the code under test.

The Newton / bisection tail of wgs84_leg (more than 20 iterations) is not reached by any of these legs, nor by any WGS84 leg
known to the authors (Karney 2013: at most 16 iterations over his test set); tests/test_mp_geodesy.py prints the iteration
counts the host solver needed per family.
"""
import math

import numpy as np

IMAGES = ("as given", "latitudes mirrored", "longitudes mirrored", "reversed")
SPHERE_MAX_ARC_DEG = 179.0
ZERO_SQUARE = 1e-8


def images(leg):
    """The four images of a base leg, in the order of IMAGES."""
    lon1, lat1, lon2, lat2 = leg
    return [(lon1, lat1, lon2, lat2), (lon1, -lat1, lon2, -lat2), (-lon1, lat1, -lon2, lat2), (lon2, lat2, lon1, lat1)]


def _zero_square():
    lo, la, under, over = 10.0, 33.0, 0.99e-8, 1.01e-8
    return [(lo, la, lo + under, la + under), (lo, la, lo + under, la + over), (lo, la, lo + over, la + under),
            (lo, la, lo, la), (359.5, 20.0, -0.5, 20.0)]


TINY_SIZES = (1.01e-8, 1e-7, 1.9e-6, 2.3e-6, 3e-5, 1e-3)  # the leg's arc in degrees
TINY_LATS = (0.0, 33.3, 67.1, 89.5)
_TINY_DIRS = ((0.0, 1.0), (1.0, 0.0), (0.6, 0.8))  # (east, north) of the unit arc: along the meridian, the parallel, oblique
_TINY_OBLIQUE_MIN = 1.3e-8  # an oblique leg of 1.01e-8 degrees has both differences below 1e-8: it would be in the zero square


def _tiny():
    legs = []
    for i, size in enumerate(TINY_SIZES):
        for j, lat in enumerate(TINY_LATS):
            # one direction per (size, latitude), rotating; all three at 33.3 and 67.1 for the two sizes around the short line
            # (on the equator a leg along the parallel takes the equatorial branch, and one along the meridian never reaches
            # the short line at any latitude)
            every = size in (1.9e-6, 2.3e-6) and lat in (33.3, 67.1)
            for east, north in (_TINY_DIRS if every else (_TINY_DIRS[(i + j) % 3],)):
                arc = max(size, _TINY_OBLIQUE_MIN) if east * north != 0.0 else size
                legs.append((-41.5, lat, -41.5 + east * arc / math.cos(math.radians(lat)), lat + north * arc))
    return legs


def _meridional():
    return [(5.0, -40.0, 5.0, 60.0), (-73.25, 10.5, -73.25, 11.5),  # equal longitudes
            (0.0, 89.9, 180.0, 89.9), (20.0, 60.0, -160.0, 70.0), (10.0, 20.0, -170.0, -10.0),  # 180 apart, over the pole
            (13.0, 90.0, 50.0, 20.0), (-133.0, -90.0, 50.0, 20.0), (77.0, 90.0, -20.0, -35.5),  # from a pole, any lon1
            (13.0, 90.0, 50.0, -90.0),  # pole to pole
            (0.0, 89.999, 180.0, 89.999), (30.0, 89.999, 100.0, 89.999),  # 111 m from a pole, over it and past it
            (1e-14, 5.0, 180.0, 10.0)]


def _equatorial():
    legs = [(0.0, 0.0, d, 0.0) for d in (130.0, 179.39, 179.40, 179.5, 179.9999)]
    return legs + [(-30.0, 0.0, 100.0, 0.0), (0.0, 1e-9, 180.0, -1e-9)]


def _seam():
    return [(179.9, 10.0, -179.9, 12.0), (179.9, -35.0, 180.1, -35.2), (359.5, 50.0, 0.5, 49.0), (-720.25, 5.0, 721.0, -8.0)]


def _antipodal():
    rng = np.random.default_rng(20261019)
    legs = []
    for k in range(20):
        lat, lon = float(rng.uniform(-80.0, 80.0)), float(rng.uniform(-180.0, 180.0))
        if k < 8:
            r = 0.6
        elif k < 16:
            r = 0.1 * math.cos(math.radians(lat))
        else:
            r = None
        if r is not None:
            dlat, dlon = (float(v) for v in rng.uniform(-r, r, 2))
        else:
            dlat, dlon = (float(s * v) for s, v in zip(rng.choice([-1.0, 1.0], 2), rng.uniform(1.2, 3.0, 2)))
        legs.append((lon, lat, lon + 180.0 + dlon, -lat + dlat))
    # the hand-over from the spherical starting guess to the astroid, sin(arc) = 6 n pi cos^2(beta1): 1.36 degrees from the
    # antipode at latitude 30
    return legs + [(20.0, 30.0, 200.4, -28.75), (20.0, 30.0, 200.4, -28.62)]


def _published():
    from test_geodesic_karney import KNOWN

    return [(float(lon1), float(lat1), float(lon2), float(lat2)) for (lat1, lon1, lat2, lon2), _, _ in KNOWN]


def _generic():
    rng = np.random.default_rng(20261020)
    draw = lambda: (rng.uniform(-180, 180), rng.uniform(-89.5, 89.5), rng.uniform(-180, 180), rng.uniform(-89.5, 89.5))  # noqa: E731
    return [tuple(float(v) for v in draw()) for _ in range(20)]


_BUILDERS = {"zero_square": _zero_square, "tiny": _tiny, "meridional": _meridional, "equatorial": _equatorial, "seam": _seam,
             "antipodal": _antipodal, "published": _published, "generic": _generic}
FAMILY_NAMES = tuple(_BUILDERS)
_CACHE = {}


def base_legs(family):
    if family not in _CACHE:
        _CACHE[family] = [tuple(float(v) for v in leg) for leg in _BUILDERS[family]()]
    return _CACHE[family]


def family_legs(family):
    """[(image index, leg)] of a family: every base leg in its four images, base leg by base leg."""
    return [(i, img) for leg in base_legs(family) for i, img in enumerate(images(leg))]


def sphere_arc_deg(leg):
    """The great-circle arc of a leg in degrees by atan2(|p1 x p2|, p1 . p2)."""
    lon1, lat1, lon2, lat2 = (math.radians(v) for v in leg)
    p = np.array([math.cos(lat1) * math.cos(lon1), math.cos(lat1) * math.sin(lon1), math.sin(lat1)])
    q = np.array([math.cos(lat2) * math.cos(lon2), math.cos(lat2) * math.sin(lon2), math.sin(lat2)])
    return math.degrees(math.atan2(float(np.linalg.norm(np.cross(p, q))), float(p @ q)))


def sphere_checked(leg):
    """Whether the sphere functions are held to the landing bound on this leg (see SPHERE above)."""
    return sphere_arc_deg(leg) <= SPHERE_MAX_ARC_DEG


def in_zero_square(leg):
    """utils.geographiclib_distance's test, in the same double arithmetic."""
    lon1, lat1, lon2, lat2 = leg
    return abs(lat1 - lat2) < ZERO_SQUARE and abs(lon1 - lon2) < ZERO_SQUARE


def coincident(leg):
    return leg[0] == leg[2] and leg[1] == leg[3]


# Legs on which the host returns NaN (distance and heading) and the device must too.  On the sphere a latitude beyond 90 is an
# ordinary angle; on WGS84 it is not a latitude (geodesic.inverse: NaN).
_NAN_COORDINATE = [(math.nan, 10.0, 20.0, 30.0), (5.0, math.nan, 20.0, 30.0), (5.0, 10.0, math.nan, 30.0), (5.0, 10.0, 20.0, math.nan)]
NAN_LEGS = {"sphere": _NAN_COORDINATE,
            "wgs84": _NAN_COORDINATE + [(5.0, 90.5, 20.0, 30.0), (5.0, 10.0, 20.0, -91.0), (5.0, -100.0, 20.0, 95.0)]}

# ---- bounds (tests/test_mp_geodesy.py and tests/test_geodesy_landing.py) ---------------------------------------------------
# WGS84, host and device alike: 15 nm is the accuracy Karney (2013) publishes for the algorithm; about 5 nm is what rounding the
# two outputs to doubles costs on the longest legs (half an ulp of a heading in [256, 360) degrees is 5e-16 rad, across up to
# 6.4e6 m; half an ulp of a distance near 2e4 km is 1.8e-9 m).
WGS84_BOUND_M = 2e-8
# Sphere: the device evaluates the fp64 expressions of utils.haversine_formula / heading with another libm; its worst miss per
# family may be at most SPHERE_FACTOR times NumPy's worst on that family (the same distribution of error, not the same error
# leg by leg; 4 leaves room for a few ulp of sin / atan2) and is never required to be below SPHERE_FLOOR_M.
SPHERE_FACTOR = 4.0
SPHERE_FLOOR_M = 5e-9


def host_leg(model, leg):
    """(distance km, heading degrees) of a leg by the functions the product calls on the host."""
    from track_estimators import utils

    fd, fh = ((utils.geographiclib_distance, utils.geographiclib_heading) if model == "wgs84"
              else (utils.haversine_formula, utils.heading))
    with np.errstate(all="ignore"):
        return float(fd(*leg)), float(fh(*leg))


def numpy_sphere_worst(family):
    """The worst landing miss [m] of NumPy's evaluation of utils.haversine_formula / heading over the checked legs of a
    family: the yardstick of the device's sphere functions.  Computed once."""
    key = ("np-sphere", family)
    if key not in _CACHE:
        from oracle import mp_geodesy as mg

        _CACHE[key] = max(float(mg.landing_miss_m("sphere", *leg, *host_leg("sphere", leg)))
                          for _, leg in family_legs(family) if sphere_checked(leg))
    return _CACHE[key]


def numpy_sphere_bound_m(leg):
    """What NumPy's evaluation of the sphere formulas may miss the landing point by, from the formulas' own conditioning, in
    units of u R = 2^-53 * 6378137 m = 0.71 nm (u: the relative rounding error of one double operation):

      * distance: a = sin^2(dlat / 2) + cos cos sin^2(dlon / 2) carries about 4 u absolutely (a <= 1), and the arc
        theta = 2 atan2(sqrt(a), sqrt(1 - a)) moves by 2 da / sin(theta): 8 u R / sin(theta) <= 6 u R / cos(theta / 2) beyond 90
        degrees (the cancellation in 1 - a; 0.5 um at 179 degrees), at most 8 u R below; the two final products add
        2 u pi R = 6 u R;
      * heading: ``north`` is a difference of products with about 3 u absolute error and atan2 turns it into 3 u / sin(theta)
        radians, which the arc scales back to 3 u R across the track; converting to degrees, adding 360 and the modulo round a
        number below 360 three times: 3 * 2^-53 * 360 degrees = 2e-15 rad, 2e-15 R sin(theta) <= 19 u R;
      * np.radians rounds each coordinate once, relatively: u |lon| R per point, which matters for unwrapped longitudes
        (721 degrees are 12.6 rad); the differences dlon / 2, dlon then carry it into sin and cos: 4 u (|lon1| + |lon2|) R.

    Together: u R (36 + 6 / cos(theta / 2) + 4 (|lon1| + |lon2|) [rad])."""
    ur = 2.0**-53 * 6378137.0
    theta = math.radians(sphere_arc_deg(leg))
    return ur * (36.0 + 6.0 / math.cos(theta / 2.0) + 4.0 * (abs(math.radians(leg[0])) + abs(math.radians(leg[2]))))


def landing_misses(model, family, outs):
    """``outs``: (distance km, heading degrees) per leg of ``family_legs(family)``, in that order.  Returns
    [(image index, leg, miss in metres as float)] of the legs that are held to the landing bound: all of them on WGS84 except
    those inside the zero square (whose (0, 0) the callers assert exactly), on the sphere those with an arc of at most 179
    degrees."""
    from oracle import mp_geodesy as mg

    legs = family_legs(family)
    assert len(outs) == len(legs)
    res = []
    for (img, leg), (d, h) in zip(legs, outs):
        if (model == "wgs84" and in_zero_square(leg)) or (model == "sphere" and not sphere_checked(leg)):
            continue
        assert math.isfinite(d) and math.isfinite(h) and d >= 0.0 and 0.0 <= h < 360.0, (family, leg, d, h)
        res.append((img, leg, float(mg.landing_miss_m(model, *leg, d, h))))
    return res


def worst_per_image(misses):
    """[worst miss of image 0, .., 3]; every image must have contributed a leg."""
    per = [[m for img, _, m in misses if img == i] for i in range(len(IMAGES))]
    assert all(per), "an image of the family contributed no checked leg"
    return [max(p) for p in per]


def report(who, model, family, misses):
    worst = worst_per_image(misses)
    print(f"\n[landing] {who}, {model}, {family}: {len(misses)} legs, worst miss [m] "
          + ", ".join(f"{name} {w:.2e}" for name, w in zip(IMAGES, worst)))
    return worst
