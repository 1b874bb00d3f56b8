"""The device leg functions (csrc/ste_geodesy.h: sphere_leg, sphere_dist_km, wgs84_leg) held to the definition of a geodesic:
the (distance, heading) a kernel returns, walked from point 1 by the 50-digit direct solution of oracle/mp_geodesy.py, must
land on point 2.  Needs a real MI355X: run with ``pytest -m gpu``; ``-s`` prints the worst miss per family, model and image.

  * through ``batch.prepare_observations`` (ste_track_prep_f64): every family of tests/geodesy_cases.py as two-observation tracks
    with gap 1.0, one launch per family and model, so that sog[0] is the distance in km and cog[0] the heading.  WGS84: the
    landing miss is at most 20 nm (the bound of the host solver, tests/test_mp_geodesy.py).  Sphere: the worst miss of a family
    is at most 4 times that of NumPy's evaluation of the same formulas on the same legs (never required below 5 nm); legs
    beyond 179 degrees of arc are not held to it (geodesy_cases: SPHERE).  Status 0, no warning; exactly (0, 0) inside the zero
    square and for coincident points; NaN where the host returns NaN;
  * through ``DeviceBatch.path_metrics`` (ste_path_metrics_f64): the same legs as two-row tracks; ``distance`` equals prep's
    sog[0] bit for bit on both models -- on the sphere that is sphere_dist_km against sphere_leg, "operation for operation";
  * in one ragged launch: all families in tracks of 2 to 5 observations, B no multiple of 64: a leg's values do not depend on
    where it sits.

Measured on an MI355X ("Geodesy against the definition", has the table): WGS84 worst 6.9e-9 m (antipodal family; the
host's worst is 5.7e-9); sphere equal to NumPy's worst to three digits on six families, 4.57e-9 against 4.49e-9 on the meridional
and 2.3e-9 against 5.2e-10 on the equatorial one (below the 5 nm floor); no bit differs between path_metrics and prep, nor between
the ragged and the two-observation launch.
"""
import math
import warnings

import geodesy_cases as gc
import numpy as np
import path_metrics_cases as pmc
import pytest

pytestmark = pytest.mark.gpu

MODELS = ("sphere", "wgs84")
_DEV = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Equal bit for bit, a NaN being equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _prepare(lons, lats, gaps, model):
    from track_estimators import batch

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = batch.prepare_observations(lons, lats, gaps, model=model)
    assert [r["status"] for r in res] == [0] * len(res)
    return res


def _two_observation_launch(model, legs):
    """(n, 2): sog[0] (= the distance in km, the gap being 1.0) and cog[0] of every leg as a track of its own."""
    lons, lats = [np.array([l[0], l[2]]) for l in legs], [np.array([l[1], l[3]]) for l in legs]
    res = _prepare(lons, lats, [np.ones(1)] * len(legs), model)
    for r in res:  # the last observation repeats the last leg, and z carries the same numbers
        assert _same(r["sog"][1:], r["sog"][:1]) and _same(r["cog"][1:], r["cog"][:1])
        assert _same(r["z"][2], r["sog"]) and _same(r["z"][3], r["cog"])
    return np.array([(r["sog"][0], r["cog"][0]) for r in res])


def device_outs(model, family):
    """The device's (distance, heading) of ``gc.family_legs(family)`` -- or of the NaN legs, family "nan" -- one launch, kept."""
    key = (model, family)
    if key not in _DEV:
        legs = gc.NAN_LEGS[model] if family == "nan" else [leg for _, leg in gc.family_legs(family)]
        _DEV[key] = _two_observation_launch(model, legs)
    return _DEV[key]


def all_legs(model):
    """Every leg of every family, then the NaN legs, with the device's two-observation results in the same order."""
    legs, outs = [], []
    for family in gc.FAMILY_NAMES:
        legs += [leg for _, leg in gc.family_legs(family)]
        outs.append(device_outs(model, family))
    legs += gc.NAN_LEGS[model]
    outs.append(device_outs(model, "nan"))
    return legs, np.concatenate(outs)


@pytest.mark.parametrize("family", gc.FAMILY_NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_device_leg_lands_on_point_2(model, family):
    legs = gc.family_legs(family)
    outs = device_outs(model, family)
    for (_, leg), (d, h) in zip(legs, outs):
        if gc.coincident(leg) or (model == "wgs84" and gc.in_zero_square(leg)):
            assert _bits(d) == 0 and _bits(h) == 0, (leg, d, h)  # +0.0, +0.0
        elif model == "wgs84" and leg[1] == leg[3] and (leg[0] - leg[2]) % 360.0 == 0.0:
            # coincident points written 360 degrees apart reach the solver: distance 0, the heading the host gives (180 on the
            # northern hemisphere, 0 on the southern)
            assert _bits(d) == 0 and _bits(h) == _bits(gc.host_leg(model, leg)[1]), (leg, d, h)
    misses = gc.landing_misses(model, family, [tuple(o) for o in outs])
    worst = gc.report("device", model, family, misses)
    if model == "wgs84":
        bound = gc.WGS84_BOUND_M
        assert len(misses) == len(legs) - sum(gc.in_zero_square(leg) for _, leg in legs)
    else:
        yard = gc.numpy_sphere_worst(family)
        bound = max(gc.SPHERE_FACTOR * yard, gc.SPHERE_FLOOR_M)
        print(f"          NumPy's worst miss on these legs: {yard:.2e} m; bound {bound:.2e} m")
        assert len(misses) == sum(gc.sphere_checked(leg) for _, leg in legs)
    assert max(worst) <= bound, [(leg, m) for _, leg, m in misses if m > bound]


@pytest.mark.parametrize("model", MODELS)
def test_device_returns_nan_where_the_host_does(model):
    outs = device_outs(model, "nan")
    for leg, (d, h) in zip(gc.NAN_LEGS[model], outs):
        hd, hh = gc.host_leg(model, leg)
        assert math.isnan(hd) and math.isnan(hh)
        assert math.isnan(d) and math.isnan(h), (model, leg, d, h)


@pytest.mark.parametrize("model", MODELS)
def test_path_metrics_distance_is_preps_bit_for_bit(model):
    """Every leg as a two-row track (nsteps = 1) through ste_path_metrics_f64.  WGS84: the same wgs84_leg.  Sphere:
    sphere_dist_km, which csrc/ste_geodesy.h documents as operation for operation the dist_km of sphere_leg."""
    from track_estimators import batch

    legs, outs = all_legs(model)
    B = len(legs)
    assert B % 64 != 0
    states = pmc.states_of([[[l[0], l[1]], [l[2], l[3]]] for l in legs])
    db = batch.DeviceBatch(pmc.bare_batch(np.ones(B, dtype=np.int32), np.ones((1, B))), histories=False)
    got = db.path_metrics(db.torch.from_numpy(states).to(db.device), model=model, cumulative=True)
    dist, cum = got["distance"].cpu().numpy()[0], got["cumulative"].cpu().numpy()[0]
    assert np.array_equal(_bits(cum[1]), _bits(dist)) and (cum[0] == 0.0).all()
    want = outs[:, 0]
    nan = np.isnan(want)
    assert nan.sum() == len(gc.NAN_LEGS[model]) and np.array_equal(np.isnan(dist), nan)
    differ = np.flatnonzero(~nan & (_bits(dist) != _bits(want)))
    print(f"\n[landing] path_metrics against prep, {model}: {B} legs, {differ.size} differ in their bits")
    assert differ.size == 0, [(legs[i], dist[i], want[i]) for i in differ[:10]]


@pytest.mark.parametrize("model", MODELS)
def test_ragged_launch_gives_the_same_bits(model):
    """All legs in one launch of tracks of 2, 3, 4 and 5 observations (1, 1, 2 and 2 legs of the families each, the legs between
    them and the odd last one being fillers with other gaps): sog, cog and z at a leg's place equal the two-observation launch
    bit for bit."""
    legs, outs = all_legs(model)
    lons, lats, gaps, where = [], [], [], []  # where: (track, observation index) of leg k
    k, size = 0, 2
    while k < len(legs):
        take = legs[k:k + size // 2]
        lon, lat = [], []
        for j, l in enumerate(take):
            where.append((len(lons), 2 * j))
            lon += [l[0], l[2]]
            lat += [l[1], l[3]]
        if size % 2 and len(take) == size // 2:  # an odd last observation: somewhere else
            lon.append(lon[0] + 0.37)
            lat.append(0.5 * lat[0])
        n = len(lon)
        gaps.append(np.array([1.0 if j % 2 == 0 else 0.5 + j for j in range(n - 1)]))
        lons.append(np.array(lon))
        lats.append(np.array(lat))
        k += len(take)
        size = 2 + (size - 1) % 4
    assert len(where) == len(legs) and {len(v) for v in lons} == {2, 3, 4, 5}
    if len(lons) % 64 == 0:  # B must not be a multiple of the wave
        lons.append(np.array([1.0, 2.0, 3.0])), lats.append(np.array([4.0, 5.0, 6.0])), gaps.append(np.array([2.0, 3.0]))
    res = _prepare(lons, lats, gaps, model)
    assert len(res) % 64 != 0
    bad = []
    for (t, j), leg, (d, h) in zip(where, legs, outs):
        r = res[t]
        if not (_same(r["sog"][j], d) and _same(r["cog"][j], h) and _same(r["z"][2, j], d) and _same(r["z"][3, j], h)):
            bad.append((leg, (t, j), (r["sog"][j], r["cog"][j]), (d, h)))
        assert _same(r["z"][:2, j], leg[:2]) and _same(r["z"][:2, j + 1], leg[2:])
    print(f"\n[landing] ragged launch, {model}: {len(res)} tracks, {len(legs)} legs, {len(bad)} differ from their own launch")
    assert not bad, bad[:10]
