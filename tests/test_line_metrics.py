"""Tracks on the device against polylines (include/ste.h: ste_line_f64, ste_line_metrics_f64; DESIGN.md, "Lines"): declaration
and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers and against three independent
oracles (the region restatement on a closed ring, the site restatement on a line of two identical vertices, a brute-force grid
of (u, v)), and the conditions of the line fleet that the device comparison rests on (CPU); on the GPU the hand-made ships for
both leg functions, the line fleet against the restatement, independence of the surroundings bit for bit, the region and the
site kernels on the same data, the Python front ends on a real run, and the refusals on the device build."""
import ctypes as C
import os
import re

import line_cases as lc
import numpy as np
import path_metrics_cases as pmc
import pytest
import region_metrics_cases as rmc
import site_cases as sc
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "nlines", "nvert", "vert", "first", "lon_ref", "t0", "flags", "reserved", "min_dist",
          "min_time", "min_seg", "min_frac", "ncross", "net_cross", "first_cross", "last_cross", "sound_time", "nbroken",
          "track_status", "line_status"]
OUTPUTS = FIELDS[11:]
PER_LINE = lc.FLOAT_OUTPUTS + lc.INT_OUTPUTS  # (S, M, B)
CROSS = ("ncross", "net_cross", "first_cross", "last_cross")
APPROACH = ("min_dist", "min_time", "min_seg", "min_frac")
INT32 = ("min_seg", "ncross", "net_cross", "nbroken", "track_status", "line_status")
FRAC_ATOL = 1e-9


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bits(a):
    return _u64(np.asarray(a).astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_line_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_line_f64\* li, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    assert re.search(r"^int ste_line_chunk\(void\);", hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_line_f64 {"): hdr.index("} ste_line_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteLineF64._fields_] == FIELDS
    # the layout of the C struct by hand: nstates and model share a word, nlines and nvert one, flags and reserved one, every
    # pointer takes one
    offsets = {"nstates": 0, "model": 4, "states": 8, "nlines": 16, "nvert": 20, "vert": 24, "first": 32, "lon_ref": 40, "t0": 48,
               "flags": 56, "reserved": 60}
    offsets.update({name: 64 + 8 * k for k, name in enumerate(OUTPUTS)})
    assert {f: getattr(binding.SteLineF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteLineF64) == 160 and re.search(r"} ste_line_f64;\s*/\* 160 bytes \*/", hdr)
    assert "ste_line_metrics_f64" in binding.SYMBOLS and "ste_line_chunk" in binding.SYMBOLS
    lib = binding.load()
    assert hasattr(lib, "ste_line_metrics_f64") and 1 <= lib.ste_line_chunk() <= 1024
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert "(ste_line_metrics_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the line arguments travel beside the batch
    assert int(re.search(r"#define STE_LINES_MAX (\d+)", hdr).group(1)) == binding.STE_LINES_MAX == 4096
    assert re.search(r"#define STE_LINE_MAX_VERT_TOTAL \(1 << 20\)", hdr) and binding.STE_LINE_MAX_VERT_TOTAL == 1 << 20
    assert int(re.search(r"#define STE_LINE_BAD_TIME 0x(\d+)", hdr).group(1), 16) == binding.STE_LINE_BAD_TIME == lc.BAD_TIME == 1
    assert int(re.search(r"#define STE_LINE_BAD_LINE 0x(\d+)", hdr).group(1), 16) == binding.STE_LINE_BAD_LINE == lc.BAD_LINE == 1
    comment = hdr[hdr.index("LINES:"): hdr.index("#define STE_LINES_MAX")]
    for word in ("Clock.", "Bad clock.", "Pieces.", "Soundness.", "Frame", "Bad line.", "Crossing", "Closest approach", "Accuracy.",
                 "PIECE", "BROKEN", "CROSSING", "CANDIDATES", "PRECONDITION", "wrap180", "clamp01", "wins a tie", "without contraction",
                 "No crossing is sorted", "squared norm of the difference", "upper bound", "Refused with STE_EINVAL"):
        assert word in comment, word


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The pointers below are not memory: nothing may be launched, with a GPU or without one."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.dt, s.nsteps = 0x1000, 0x2000
        return s

    def good_line():
        e = binding.SteLineF64()
        e.nstates, e.model, e.states, e.nlines, e.nvert = 3, binding.STE_PREP_WGS84, 0x3000, 5, 40
        e.vert, e.first, e.lon_ref, e.t0 = 0x4000, 0x4800, 0x4c00, 0x5000
        e.flags, e.reserved = 0, 0
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x6000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_line()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc = lib.ste_line_metrics_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_line_metrics_f64" in msg, (fields, rc, msg)

    for s, e, reason in ((None, good_line(), "batch pointer is NULL"), (good_batch(), None, "line arguments (li) are NULL")):
        assert lib.ste_line_metrics_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_line_metrics_f64" in msg
    refused("li->states is required", states=None)
    refused("li->vert is required", vert=None)
    refused("li->first is required", first=None)
    refused("li->lon_ref is required", lon_ref=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1, 4097, 1 << 30):
        refused("between 1 and STE_LINES_MAX", nlines=n)
    for n in (1, 0, -1, (1 << 20) + 1):
        refused("between 2 and STE_LINE_MAX_VERT_TOTAL", nvert=n)
    for m in (-1, 2, 7):
        refused("STE_PREP_SPHERE or STE_PREP_WGS84 when min_dist is asked for", model=m)
    for f in (1, 0x80000000):
        refused("li->flags must be 0", flags=f)
        refused("li->reserved must be 0", reserved=f)
    refused("batch's dt is required", dt=None)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
    refused("2^31 - 1 blocks", B=2 ** 31 - 1, nlines=4096)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_hand_answers():
    """Fourteen hand-made ships against eighteen lines, every coordinate a dyadic number (line_cases.HAND_SHIPS and HAND_LINES
    name them): a ship crossing a two-vertex gate in the middle of a step (0 km at the known time, +1, and -1 for the reversed
    line); one crossing at the vertex two segments share (once); one parallel to a line at a known offset; a vertex that is
    closest as a segment's first and as its second one; a ship's own knot that is closest as the end of a step and as the start
    of one; a zigzag with three crossings; a stationary ship; a ship stored wrapped against a gate across the antimeridian
    under both of its names (the same bits); a segment of zero length; a NaN latitude that hides a crossing; nsteps 0 and 1; a
    negative and a NaN dt inside nsteps, a NaN dt past them, a NaN t0; a step of zero length; and every kind of bad line: a
    range that starts below 0 (line 0, whose block walks the tracks) or ends above V, one vertex, a NaN lon_ref, a NaN
    longitude, an infinite latitude, a vertex more than 90 degrees from lon_ref."""
    h = lc.hand_batch()
    res = {}
    for model in ("sphere", "wgs84"):
        res[model] = lc.line_metrics(h["states"], h["nsteps"], h["dt"], h["vert"], h["first"], h["lon_ref"], h["t0"], model)
        lc.check_hand_answers(res[model], f"restatement, {model}", model)
    r, s = res["wgs84"], res["sphere"]  # the model touches min_dist alone, and that by the ellipsoid's scales
    for k in PER_LINE[1:] + lc.TRACK_OUTPUTS + ("track_status", "line_status"):
        assert np.array_equal(_bits(r[k]), _bits(s[k])), k
    both = np.isfinite(s["min_dist"])
    assert np.array_equal(both, np.isfinite(r["min_dist"]))
    assert np.allclose(r["min_dist"][both], s["min_dist"][both], rtol=7e-3, atol=1e-9)  # atol: a ship on a line, 0 or a rounding


def _ring_reference():
    """The ring of the line fleet alone with t0 = 0, and the region restatement on its polygon (the closing vertex dropped)."""
    if "ring" not in lc._CACHE:
        w = lc.fleet()
        ring = w["lines"][lc.RING]
        vert, first = lc.pack([ring])
        ref = np.array([w["lon_ref"][lc.RING]])
        line = lc.line_metrics(w["states"], w["nsteps"], w["dt"], vert, first, ref)
        poly = np.ascontiguousarray(ring[:-1].T)
        region = rmc.region_metrics(w["states"], w["nsteps"], w["dt"], poly, ref[0])
        lc._CACHE["ring"] = (vert, first, ref, poly, line, region)
    return lc._CACHE["ring"]


def _check_ring_against_region(line, region, what):
    """Tracks that start outside and have no broken step: the crossings with +1 are the region's entries, and the earliest
    crossing is the first entry, bit for bit (t0 = 0 and every dt a multiple of 2^-6 h: hi - lo is dt to the bit)."""
    outside = region["inside"][:, 0] == 0
    assert not region["nbroken"].any() and 60 < outside.sum() < outside.size
    plus = (line["ncross"][:, 0] + line["net_cross"][:, 0]) // 2
    if "ncrossings" in region:  # the restatement counts the crossings of either kind as well
        assert np.array_equal(line["ncross"][:, 0], region["ncrossings"]), what
    assert np.array_equal(plus[outside], region["nenter"][outside]), what
    assert np.array_equal(_bits(line["first_cross"][:, 0][outside]), _bits(region["first_entry"][outside])), what
    entered = outside & (region["nenter"] > 0)
    assert entered.sum() > 50 and (region["nenter"][outside] > 1).any(), what
    return int(entered.sum())


def test_restatement_against_the_region_restatement():
    """Oracle (a): the closed counter-clockwise star of the line fleet as a line, with the same lon_ref, against
    region_metrics_cases.region_metrics on the same vertices as a polygon."""
    vert, first, ref, poly, line, region = _ring_reference()
    assert np.sum(poly[0] * np.roll(poly[1], -1) - np.roll(poly[0], -1) * poly[1]) > 0.0  # counter-clockwise
    n = _check_ring_against_region(line, region, "restatements")
    print(f"ring against region: {n} (sample, track) pairs start outside and enter")


def _site_points():
    """Five points some kilometres off rows of the line fleet's sample 0, two of them across the antimeridian."""
    w = lc.fleet()
    pts = [w["states"][0, 2, :2, b] + off for b, off in ((3, (0.03, -0.05)), (12, (-0.06, 0.02)), (40, (0.05, 0.04)),
                                                         (77, (-0.02, -0.07)), (101, (0.08, 0.01)))]
    return np.array(pts)


def _point_lines(pts):
    """Each point as a line of two identical vertices, unwrapped about itself."""
    vert, first = lc.pack([np.stack([p, p]) for p in pts])
    return vert, first, pts[:, 0].copy()


def _check_points_against_sites(line, site, span, what):
    nan = np.isnan(site["min_dist"])
    assert np.array_equal(np.isnan(line["min_dist"]), nan) and np.array_equal(np.isnan(line["min_time"]), nan), what
    assert not sc.near_tie(site).any(), what
    derr = np.abs(line["min_dist"] - site["min_dist"])[~nan] / site["min_dist"][~nan]
    terr = (np.abs(line["min_time"] - site["min_time"]) / np.broadcast_to(span, nan.shape))[~nan]
    print(f"{what}: min_dist deviates by at most {derr.max() / pmc.DIST_RTOL:.3g} of its tolerance, min_time by {terr.max() / pmc.TIME_RTOL:.3g} "
          f"({int((~nan).sum())} values, distances {site['min_dist'][~nan].min():.3g} .. {site['min_dist'][~nan].max():.3g} km)")
    assert derr.max() <= pmc.DIST_RTOL and terr.max() <= pmc.TIME_RTOL, (what, derr.max(), terr.max())
    assert not line["ncross"].any() and (line["min_seg"][~nan] == 0).all(), what


def test_restatement_against_the_site_restatement():
    """Oracle (b): a line of two identical vertices is a site.  min_dist within 1e-10 relative and min_time within 1e-12 of the
    clock span of site_cases.site_metrics at that point, the site tests' own tolerances; the frames differ (the ship is
    unwrapped about the line's lon_ref here, the site about the ship there), so the bits need not be equal."""
    w, pts = lc.fleet(), _site_points()
    vert, first, ref = _point_lines(pts)
    line = lc.line_metrics(w["states"], w["nsteps"], w["dt"], vert, first, ref, w["t0"])
    site = sc.site_metrics(w["states"], w["nsteps"], w["dt"], pts, 10.0, w["t0"])
    _check_points_against_sites(line, site, lc.clock_span(w["nsteps"], w["dt"]) + 1e-300, "point lines against sites")


def test_restatement_against_brute_force():
    """Oracle (c): per (step, segment) of twelve ships of the line fleet against its lines of 1, 2 and 3 segments and the one
    with the doubled vertex, the planar distance on a 257 x 257 grid of (u, v).  No sampled distance lies below sqrt(best_q) by
    more than 1e-9 km, and the best sampled one lies within the grid spacing's bound of it: a move of 1/512 in u and in v moves
    the two points by at most (|dk| + |ek|) / 512."""
    w, ref = lc.fleet(), lc.fleet_reference()
    g = np.linspace(0.0, 1.0, 257)
    U, W = np.meshgrid(g, g, indexing="ij")
    checked = 0
    for b in (0, 5, 9, 15, 20, 35, 44, 61, 70, 88, 107, 129):
        ns = int(w["nsteps"][b])
        lon, lat = w["states"][0, :, 0, b], w["states"][0, :, 1, b]
        for m in (0, 1, 2, 8):
            x, y = w["vert"][:, w["first"][m]:w["first"][m + 1]]
            r0 = w["lon_ref"][m]
            best, bound = np.inf, 0.0
            for k in range(ns):
                delta = lc.wrap180(lon[k + 1] - lon[k])
                x0, y0 = r0 + lc.wrap180(lon[k] - r0), lat[k]
                dx, dy = delta, lat[k + 1] - y0
                for j in range(x.shape[0] - 1):
                    kc = lc.KD * np.cos(np.radians(0.25 * ((y0 + lat[k + 1]) + (y[j] + y[j + 1]))))
                    sx = kc * ((x[j] - x0) + W * (x[j + 1] - x[j]) - U * dx)
                    sy = lc.KD * ((y[j] - y0) + W * (y[j + 1] - y[j]) - U * dy)
                    d = np.sqrt(sx * sx + sy * sy).min()
                    if d < best:
                        best = d
                    bound = max(bound, (np.hypot(kc * dx, lc.KD * dy) + np.hypot(kc * (x[j + 1] - x[j]), lc.KD * (y[j + 1] - y[j]))) / 512.0)
            if ns == 0:
                assert ref["best_q"][0, m, b] == np.inf
                continue
            exact = np.sqrt(ref["best_q"][0, m, b])
            assert best >= exact - 1e-9, (b, m, best, exact)
            assert best <= exact + bound + 1e-9, (b, m, best, exact, bound)
            checked += 1
    assert checked >= 40


def test_conditions_of_the_line_fleet():
    """The restatement alone on all three samples of the line fleet: what the device comparison assumes of it.  No value is a
    near tie (another candidate's q <= best q (1 + 1e-9): time, segment and fraction could come from either) and no knot or
    vertex is within 1e-9 of deciding a crossing (u or v that close to 0 or 1 with the other parameter in reach), so no case is
    excluded from any comparison.  Every kind of row is there: crossings of every line, lines never crossed, tracks without a
    step, closest points inside segments, on vertices and on knots."""
    from track_estimators._hip import binding

    c = binding.load().ste_line_chunk()
    w, ref = lc.fleet(c), lc.fleet_reference("sphere", c)
    S, M, B = lc.FLEET_S, lc.FLEET_M, lc.FLEET_B
    assert w["states"].shape == (S, lc.FLEET_N + 1, 4, B) and B == 2 * 64 + 2 and M == 9 and len(w["lon_ref"]) == M
    nseg = np.diff(w["first"]) - 1
    assert nseg.tolist() == [1, 2, 3, c - 1, c, c + 1, 2 * c + 1, 12, 4]
    ring, dbl = w["lines"][lc.RING], w["lines"][8]
    assert np.array_equal(ring[0], ring[-1]) and np.array_equal(dbl[1], dbl[2])
    assert set(w["nsteps"][16:].tolist()) == set(range(9)) and (w["nsteps"][:16] == lc.FLEET_N).all()
    assert (np.abs(w["states"][:, :, 0, :8]) <= 180.0).all() and (w["states"][:, :, 0, 8:16] > 180.0).any()
    assert np.array_equal(w["dt"] * 64.0, np.round(w["dt"] * 64.0)) and np.array_equal(w["t0"] * 64.0, np.round(w["t0"] * 64.0))
    for b, ns in enumerate(w["nsteps"]):  # garbage past nsteps
        assert ns == lc.FLEET_N or np.abs(w["states"][:, ns + 1:, :2, b]).max() > 90.0
    tie, knot = lc.near_tie(ref), lc.knot_decides(ref)
    found = np.isfinite(ref["min_dist"])
    fr = ref["min_frac"][found]
    print(f"line fleet: crossings per (sample, line, track) {np.bincount(ref['ncross'].ravel()).tolist()}; lines crossed by some track "
          f"{(ref['ncross'] > 0).any(axis=(0, 2)).tolist()}; {int((~found[0]).sum())} pairs of sample 0 without a sound step; min_dist "
          f"{ref['min_dist'][found].min():.3g} .. {ref['min_dist'][found].max():.3g} km; closest at a vertex {int(((fr == 0) | (fr == 1)).sum())}, "
          f"inside a segment {int(((fr > 0) & (fr < 1)).sum())}; near ties {int(tie.sum())} and deciding knots {int(knot.sum())} of "
          f"{S * M * B}; least knot margin {ref['knot_margin'].min():.3g}")
    assert int(tie.sum()) == 0 and int(knot.sum()) == 0
    assert not ref["track_status"].any() and not ref["line_status"].any() and not ref["nbroken"].any()
    assert (~found[0]).sum() == M * int((w["nsteps"] == 0).sum())
    assert (ref["ncross"] > 0).any(axis=(0, 2)).all() and (ref["ncross"] == 0).any(axis=(0, 2)).all()
    assert (ref["ncross"] > 2).any() and (ref["net_cross"] > 0).any() and (ref["net_cross"] < 0).any()
    assert ((fr > 0) & (fr < 1)).sum() > 100 and ((fr == 0) | (fr == 1)).sum() > 100
    assert (ref["min_seg"][:, 6] >= c).any() and (0 <= ref["min_seg"][:, 6]).any() and (ref["min_seg"][:, 6] < c).any()  # more than one chunk of the longest line
    assert np.array_equal(np.isnan(ref["first_cross"]), ref["ncross"] == 0) and (ref["last_cross"][ref["ncross"] > 1] > ref["first_cross"][ref["ncross"] > 1]).all()
    assert np.array_equal(_bits(ref["last_cross"][ref["ncross"] == 1]), _bits(ref["first_cross"][ref["ncross"] == 1]))


def test_track_lines_normalises_and_refuses():
    """batch.track_lines: unwrapping from the first vertex, lon_ref in the middle of the extent, the CSR arrays, and its
    ValueErrors (no GPU is needed for them)."""
    from track_estimators import batch

    tl = batch.track_lines([[(179.5, 0.0), (-179.5, 1.0), (-178.0, 2.0)], np.array([[10.0, 50.0], [10.0, 50.0]])])
    assert tl.nlines == 2 and tl.first.tolist() == [0, 3, 5] and tl.first.dtype == np.int32
    assert tl.vert[0].tolist() == [179.5, 180.5, 182.0, 10.0, 10.0] and tl.lon_ref.tolist() == [180.75, 10.0]
    assert np.array_equal(tl.line(1), [[10.0, 50.0], [10.0, 50.0]]) and batch.track_lines(tl) is tl
    for bad, msg in (([], "1 to 4096"), ([[(0.0, 0.0)]], "fewer than 2 vertices"), ([np.zeros((3, 3))], r"\(n, 2\) array"),
                     ([[(0.0, 0.0), (np.nan, 1.0)]], "non-finite"), ([[(0.0, 0.0), (90.0, 1.0)]], "less than 90"),
                     ([[(0.0, 0.0), (80.0, 0.0), (160.0, 0.0), (200.0, 0.0)]], "at most 180")):
        with pytest.raises(ValueError, match=msg):
            batch.track_lines(bad)


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _lines_of(vert, first, lon_ref):
    from track_estimators import batch

    return batch.TrackLines(vert=np.ascontiguousarray(vert), first=np.asarray(first, dtype=np.int32), lon_ref=np.asarray(lon_ref, dtype=np.float64))


def _abi_call(db, states, vert, first, lon_ref, t0, model="sphere", want=OUTPUTS):
    """ste_line_metrics_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor; ``want``: the outputs asked for (the
    others are NULL); -> dict of NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    S, B, M = int(states.shape[0]), int(states.shape[3]), len(lon_ref)
    xy, fi, ref = _dev(db, vert), _dev(db, np.asarray(first, dtype=np.int32)), _dev(db, np.asarray(lon_ref, dtype=np.float64))
    clock = None if t0 is None else _dev(db, np.asarray(t0, dtype=np.float64))
    shape = {"sound_time": (S, B), "nbroken": (S, B), "track_status": (B,), "line_status": (M,)}
    out = {}
    li = binding.SteLineF64()
    li.nstates, li.model, li.states = S, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model], states.data_ptr()
    li.nlines, li.nvert, li.vert, li.first, li.lon_ref = M, int(vert.shape[1]), xy.data_ptr(), fi.data_ptr(), ref.data_ptr()
    li.t0 = None if clock is None else clock.data_ptr()
    for k in want:
        out[k] = torch.empty(shape.get(k, (S, M, B)), dtype=torch.int32 if k in INT32 else torch.float64, device=db.device)
        setattr(li, k, out[k].data_ptr())
    binding.check(db.lib.ste_line_metrics_f64(C.byref(db.struct), C.byref(li), db._stream(None)), "ste_line_metrics_f64")
    torch.cuda.synchronize()
    return _host(out)


def _compare(got, ref, span, what):
    """The device against the restatement: integers, min_seg and statuses equal, sound_time bit for bit, NaN patterns identical,
    min_dist within pmc.DIST_RTOL / DIST_ATOL, the times within pmc.TIME_RTOL of the track's clock span (``span``, (B,)),
    min_frac within 1e-9.  Nothing is left out.  Returns the largest deviations as fractions of their tolerances."""
    for k in ("track_status", "line_status", "nbroken") + lc.INT_OUTPUTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    assert np.array_equal(_u64(got["sound_time"]), _u64(ref["sound_time"])), (what, "sound_time")
    worst = {}
    for k in lc.FLOAT_OUTPUTS:
        assert got[k].dtype == np.float64
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k]), nan), (what, k, "NaN pattern")
        err = np.abs(got[k] - ref[k])
        if k == "min_dist":
            tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref[k])
        elif k == "min_frac":
            tol = np.full(err.shape, FRAC_ATOL)
        else:
            tol = np.broadcast_to(pmc.TIME_RTOL * span, err.shape)
        frac = (err / tol)[~nan]
        worst[k] = float(frac.max()) if frac.size else 0.0
        at = np.unravel_index(np.argmax(np.where(~nan, err / np.where(tol > 0, tol, 1.0), 0.0)), err.shape)
        print(f"{what}: {k} deviates by at most {worst[k]:.3g} of its tolerance ({int((~nan).sum())} values); worst at "
              f"{tuple(int(v) for v in at)}: {got[k][at]!r} against {ref[k][at]!r}")
        assert worst[k] <= 1.0, (what, k, worst[k], np.argwhere(~nan & (err > tol))[:5].tolist())
        if k == "min_dist":
            worst["min_dist_km"] = float(err[~nan].max()) if frac.size else 0.0
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_hand_made_ships_on_the_device(model):
    """The fourteen hand-made ships and eighteen lines through the C ABI: the known answers, and the restatement."""
    from track_estimators import batch

    h = lc.hand_batch()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    got = _abi_call(db, _dev(db, h["states"]), h["vert"], h["first"], h["lon_ref"], h["t0"], model)
    lc.check_hand_answers(got, f"device, {model}", model)
    ref = lc.line_metrics(h["states"], h["nsteps"], h["dt"], h["vert"], h["first"], h["lon_ref"], h["t0"], model)
    # the planted NaN and negative dt belong to tracks that have no time to compare: their span only has to be a number
    span = lc.clock_span(h["nsteps"], np.abs(np.nan_to_num(h["dt"]))) + 1.0
    _compare(got, ref, span, f"hand-made ships, {model}")


def _fleet_batch():
    from track_estimators import batch
    from track_estimators._hip import binding

    c = binding.load().ste_line_chunk()
    w = lc.fleet(c)
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"]), _lines_of(w["vert"], w["first"], w["lon_ref"]), c


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_line_fleet_against_the_restatement(model):
    """S = 3, Nmax = 8, B = 130 (two waves plus two lanes), M = 9 lines of 1, 2, 3, c - 1, c, c + 1 and 2 c + 1 segments, a closed
    ring and a doubled vertex: integers, min_seg and statuses equal, sound_time bit for bit, NaN patterns identical, min_dist
    within 1e-10 relative, times within 1e-12 of the track's clock span, min_frac within 1e-9, nothing left out; NaN in the rows
    past nsteps changes nothing.  On WGS84 the leg is held to 4e-11 km as in the site tests: the device's solver and
    track_estimators.geodesic are two evaluations of Karney's inverse.  The largest deviations measured on an MI355X are in
    DESIGN.md, "Lines"."""
    w, db, full, tl, c = _fleet_batch()
    ref = lc.fleet_reference(model, c)
    assert not lc.near_tie(ref).any() and not lc.knot_decides(ref).any()
    got = _host(db.line_metrics(full, tl, t0=w["t0"], model=model))
    S, M, B = lc.FLEET_S, lc.FLEET_M, lc.FLEET_B
    assert set(got) == set(OUTPUTS) and got["min_dist"].shape == (S, M, B) and got["sound_time"].shape == (S, B)
    assert got["track_status"].shape == (B,) and got["line_status"].shape == (M,)
    worst = _compare(got, ref, lc.clock_span(w["nsteps"], w["dt"]) + 1e-300, f"line fleet, {model}")
    km = worst.pop("min_dist_km")
    if model == "wgs84":
        assert km <= 4e-11, km
    for k in ("first_cross", "last_cross"):  # a crossing is planar in degrees: no cos, the same bits
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.line_metrics(_dev(db, poisoned), tl, t0=w["t0"], model=model))
    for k in OUTPUTS:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, "rows past nsteps were read")


def _same_bits(a, b, what, keys=OUTPUTS, line_a=slice(None), line_b=slice(None), track_b=slice(None), sample_b=slice(None)):
    """``a`` against ``b`` restricted to the given lines (of either), tracks and samples (of ``b``)."""
    for k in keys:
        x, y = a[k], b[k]
        if k in PER_LINE:
            x, y = x[:, line_a], y[sample_b][:, line_b][..., track_b]
        elif k in lc.TRACK_OUTPUTS:
            y = y[sample_b][..., track_b]
        elif k == "track_status":
            y = y[track_b]
        else:
            x, y = x[line_a], y[line_b]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit: the line list reversed and shuffled; each line alone (M = 1); the lines re-packed at other offsets of vert
    (a line of three vertices in front of them); S = 1 slices against S = 3; each output alone and two subsets; crossings off
    against on, for the closest-approach outputs; the window [3, 70) in place on the fleet's rows and as a contiguous copy; t0
    NULL against zeros; the model changes min_dist alone."""
    w, db, full, tl, c = _fleet_batch()
    lines, refs, t0 = w["lines"], w["lon_ref"], w["t0"]
    M = lc.FLEET_M
    whole = _host(db.line_metrics(full, tl, t0=t0))

    def some(index):
        vert, first = lc.pack([lines[i] for i in index])
        return _lines_of(vert, first, refs[list(index)])

    for name, perm in (("reversed", np.arange(M)[::-1]), ("shuffled", np.random.default_rng(3).permutation(M))):
        _same_bits(_host(db.line_metrics(full, some(perm), t0=t0)), whole, name, line_b=perm)
    for m in range(M):
        _same_bits(_host(db.line_metrics(full, some([m]), t0=t0)), whole, f"line {m} alone", line_b=slice(m, m + 1))
    vert, first = lc.pack([np.array([[11.0, 51.0], [11.5, 51.5], [12.0, 51.0]])] + lines)
    moved = _host(db.line_metrics(full, _lines_of(vert, first, np.concatenate([[11.5], refs])), t0=t0))
    _same_bits(moved, whole, "other offsets of vert", line_a=slice(1, None))
    for s in range(lc.FLEET_S):
        _same_bits(_host(db.line_metrics(full[s], tl, t0=t0)), whole, f"sample {s} alone", sample_b=slice(s, s + 1))
    for want in [(k,) for k in OUTPUTS] + [("min_time", "sound_time", "nbroken", "track_status"), ("min_dist", "last_cross", "line_status")]:
        got = _abi_call(db, full, w["vert"], w["first"], refs, t0, want=want)
        _same_bits(got, whole, f"outputs {want}", keys=want)
    off = _host(db.line_metrics(full, tl, t0=t0, crossings=False))
    assert set(off) == set(OUTPUTS) - set(CROSS)
    _same_bits(off, whole, "crossings off", keys=[k for k in OUTPUTS if k not in CROSS])
    lo, hi = lc.FLEET_WINDOW
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == lc.FLEET_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _host(win.line_metrics(view, tl, t0=t0[lo:hi]))
        assert got["min_dist"].shape == (lc.FLEET_S, M, hi - lo)
        _same_bits(got, whole, f"window, copied={copied}", track_b=slice(lo, hi))
    wgs = _host(db.line_metrics(full, tl, t0=t0, model="wgs84"))
    _same_bits(wgs, whole, "the model touches min_dist alone", keys=[k for k in OUTPUTS if k != "min_dist"])
    assert not np.array_equal(_bits(wgs["min_dist"]), _bits(whole["min_dist"]))
    zeros = _abi_call(db, full, w["vert"], w["first"], refs, np.zeros(lc.FLEET_B))
    null = _abi_call(db, full, w["vert"], w["first"], refs, None)
    _same_bits(null, zeros, "t0 NULL against zeros")
    _same_bits(_host(db.line_metrics(full, tl)), zeros, "t0=None through the front end")
    assert not np.array_equal(_u64(zeros["min_time"]), _u64(whole["min_time"]))
    with pytest.raises(ValueError, match="t0 must be None, a scalar or have shape"):
        db.line_metrics(full, tl, t0=np.zeros(3))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.line_metrics(full[:, :, :3], tl)
    with pytest.raises(ValueError, match="model must be one of"):
        db.line_metrics(full, tl, model="flat")


@pytest.mark.gpu
def test_ring_against_the_region_kernel_on_the_device():
    """Oracle (a) on the device: the ring of the line fleet through ste_line_metrics_f64 with t0 = 0 and its polygon through
    DeviceBatch.region_metrics; nenter and first_entry for the tracks that start outside."""
    from track_estimators import batch

    w, db, full, tl, c = _fleet_batch()
    vert, first, ref, poly, line_ref, region_ref = _ring_reference()
    line = _host(db.line_metrics(full, _lines_of(vert, first, ref)))
    region = _host(db.region_metrics(full, batch.RegionPolygon(vert=poly, lon_ref=float(ref[0])), mask=True))
    assert np.array_equal(region["nenter"], region_ref["nenter"]) and np.array_equal(region["inside"], region_ref["inside"])
    n = _check_ring_against_region(line, region, "device")
    print(f"ring against region on the device: {n} (sample, track) pairs start outside and enter")


@pytest.mark.gpu
def test_point_lines_against_the_site_kernel_on_the_device():
    """Oracle (b) on the device: lines of two identical vertices through ste_line_metrics_f64 and the same points through
    DeviceBatch.site_metrics, held to the site tests' tolerances."""
    w, db, full, tl, c = _fleet_batch()
    pts = _site_points()
    vert, first, ref = _point_lines(pts)
    line = _host(db.line_metrics(full, _lines_of(vert, first, ref), t0=w["t0"]))
    site = _host(db.site_metrics(full, pts, 10.0, t0=w["t0"]))
    site_ref = sc.site_metrics(w["states"], w["nsteps"], w["dt"], pts, 10.0, w["t0"])
    site["best_q"], site["runner_up_q"] = site_ref["best_q"], site_ref["runner_up_q"]
    _check_points_against_sites(line, site, lc.clock_span(w["nsteps"], w["dt"]) + 1e-300, "point lines against the site kernel")


def _real_batch():
    """Four synthetic tracks of 20 steps through the filter and the smoother; track 1 is a copy of track 0 and track 3 is short."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(4, nobs=11, seed0=100)
    arrays = {f.name: getattr(sb, f.name).copy() for f in dataclasses.fields(sb)}
    for a in arrays.values():
        a[1] = a[0]
    hb = batch.pack_uniform(synthetic.SyntheticBatch(**arrays), 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 20, 13], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    return hb, db


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    """line_metrics on sm_mean and on the sampler's output of a real run against the restatement; line_chainage against a NumPy
    sum; line_statistics with zero draws gives the smoothed track's values and probabilities of 0 or 1; for given draws chunk =
    2 and chunk = 5 agree bit for bit; with the generator and one chunk it is sample_smoothed + line_metrics; the quantile path
    is refused above max_bytes and agrees with NumPy below it; track_lines' ValueErrors."""
    from track_estimators import batch

    hb, db = _real_batch()
    torch = db.torch
    sm = db.sm_mean.cpu().numpy()[None]
    p7, p12, end = sm[0, 7, :2, 0], sm[0, 12, :2, 0], sm[0, 20, :2, 2]
    # a gate across track 0 (and its copy) between rows 7 and 8, a bent line beside track 2's end, and a line 60 degrees away
    mid = 0.5 * (sm[0, 7, :2, 0] + sm[0, 8, :2, 0])
    way = sm[0, 8, :2, 0] - sm[0, 7, :2, 0]
    normal = np.array([-way[1], way[0]]) / np.hypot(*way)
    lines = [np.stack([mid - 0.3 * normal, mid + 0.3 * normal]),
             np.stack([end + (0.05, 0.3), end + (0.04, 0.0), end + (0.3, -0.2), end + (0.5, -0.2)]),
             np.stack([p7 + (60.0, 0.0), p12 + (60.0, 0.5), p12 + (61.0, 0.0)])]
    tl = batch.track_lines(lines)
    t0 = np.array([0.0, 0.25, 0.0, 1.5])
    span = lc.clock_span(hb.nsteps, hb.dt)
    got = _host(db.line_metrics(db.sm_mean, lines, t0=t0))
    ref = lc.line_metrics(sm, hb.nsteps, hb.dt, tl.vert, tl.first, tl.lon_ref, t0)
    assert not lc.near_tie(ref).any() and not lc.knot_decides(ref).any()
    _compare(got, ref, span, "smoothed tracks")
    assert got["ncross"][0, 0, 0] == 1 and got["ncross"][0, 0, 1] == 1 and not got["ncross"][0, 2].any() and not got["line_status"].any()
    nsamples = 5
    samples = db.sample_smoothed(nsamples, seed=4)
    dev = db.line_metrics(samples, tl, t0=t0)
    direct = _host(dev)
    sref = lc.line_metrics(samples.cpu().numpy(), hb.nsteps, hb.dt, tl.vert, tl.first, tl.lon_ref, t0)
    assert not lc.near_tie(sref).any() and not lc.knot_decides(sref).any()
    _compare(direct, sref, span, "sampled tracks")
    # chainage against a NumPy sum of the legs before the segment plus the fraction of its own
    for model in ("sphere", "wgs84"):
        km = batch.line_chainage(tl, dev["min_seg"], dev["min_frac"], model=model).cpu().numpy()
        want = np.full(km.shape, np.nan)
        for m in range(tl.nlines):
            ln = tl.line(m)
            legs = np.array([pmc.leg_km(model, *ln[i], *ln[i + 1]) for i in range(len(ln) - 1)])
            before = np.concatenate([[0.0], np.cumsum(legs)])
            seg, fr = direct["min_seg"][:, m], direct["min_frac"][:, m]
            ok = seg >= 0
            want[:, m][ok] = before[seg[ok]] + fr[ok] * legs[seg[ok]]
        assert np.array_equal(np.isnan(km), np.isnan(want)) and np.allclose(km, want, rtol=1e-12, atol=1e-9, equal_nan=True), model
    assert bool(torch.isnan(batch.line_chainage(tl, torch.full_like(dev["min_seg"], -1), dev["min_frac"])).all())
    # zero draws: every sample is the smoothed track
    kw = dict(t0=t0, within_km=30.0)
    zero = batch.line_statistics(db, tl, nsamples, chunk=2, draws=lambda buf, first: buf.zero_(), **kw)
    zsm = _host(db.line_metrics(db.sample_smoothed(1, draws=torch.zeros((1, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, device=db.device)),
                                tl, t0=t0))
    for k in PER_LINE:
        assert np.array_equal(_bits(zero[k + "_smoothed"]), _bits(got[k][0])), k
    for k in ("cross_prob", "net_prob", "approach_prob"):
        assert set(np.unique(zero[k]).tolist()) <= {0.0, 1.0}, k
    assert np.array_equal(zero["cross_prob"], (zsm["ncross"][0] > 0).astype(np.float64))
    assert np.array_equal(zero["net_prob"], (zsm["net_cross"][0] != 0).astype(np.float64))
    assert np.array_equal(zero["approach_prob"], (zsm["min_dist"][0] <= 30.0).astype(np.float64))
    assert zero["cross_prob"][0, 0] == 1.0 and zero["cross_prob"][2].sum() == 0.0 and zero["approach_prob"][2].sum() == 0.0
    assert np.array_equal(zero["min_dist_count"], np.where(np.isnan(zsm["min_dist"][0]), 0, nsamples))
    crossed = zsm["ncross"][0] > 0
    assert np.allclose(zero["first_cross_mean"][crossed], zsm["first_cross"][0][crossed], rtol=1e-14) and np.isnan(zero["first_cross_mean"][~crossed]).all()
    # given draws, sample by sample: the chunk changes nothing, bit for bit
    noise = torch.randn((nsamples, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(db.device)
    fill = lambda buf, first: buf.copy_(noise[first:first + buf.shape[0]])  # noqa: E731
    a = batch.line_statistics(db, tl, nsamples, chunk=2, draws=fill, **kw)
    b = batch.line_statistics(db, tl, nsamples, chunk=5, draws=fill, **kw)
    assert set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    each = _host(db.line_metrics(db.sample_smoothed(nsamples, draws=noise.clone()), tl, t0=t0))
    assert np.array_equal(a["cross_prob"], (each["ncross"] > 0).mean(axis=0))
    assert np.array_equal(a["net_prob"], (each["net_cross"] != 0).mean(axis=0))
    # the generator and one chunk: sample_smoothed's draws
    one = batch.line_statistics(db, tl, nsamples, seed=4, chunk=16, quantiles=(0.25, 0.5), **kw)
    assert np.array_equal(one["cross_prob"], (direct["ncross"] > 0).mean(axis=0))
    assert np.array_equal(one["approach_prob"], (direct["min_dist"] <= 30.0).mean(axis=0))
    good = one["min_dist_count"] > 0
    assert good.all() and np.allclose(one["min_dist_mean"], direct["min_dist"].mean(axis=0), rtol=1e-13)
    assert one["min_dist_quantiles"].shape == (2, 3, hb.B)
    assert np.allclose(one["min_dist_quantiles"], np.quantile(direct["min_dist"], (0.25, 0.5), axis=0), rtol=1e-13, atol=1e-15)
    assert not one["sample_status"].any() and not one["line_status"].any() and not one["track_status"].any()
    assert "min_dist_quantiles" not in a
    with pytest.raises(ValueError, match=rf"{nsamples} x 3 x {hb.B} doubles per quantity, {8 * nsamples * 3 * hb.B} bytes, above max_bytes = 100"):
        batch.line_statistics(db, tl, nsamples, quantiles=(0.5,), max_bytes=100)
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.line_statistics(db, tl, 0)
    viahb = batch.line_statistics(hb, tl, 3, seed=9, chunk=3, **kw)
    viadb = batch.line_statistics(db, tl, 3, seed=9, chunk=3, **kw)
    assert all(np.array_equal(_bits(viahb[k]), _bits(viadb[k])) for k in viadb)
    with pytest.raises(ValueError, match="fewer than 2 vertices"):
        db.line_metrics(db.sm_mean, [[(0.0, 0.0)]])
    with pytest.raises(ValueError, match="at most 180"):
        db.line_metrics(db.sm_mean, [[(0.0, 0.0), (80.0, 0.0), (160.0, 0.0), (200.0, 0.0)]])


@pytest.mark.gpu
def test_line_approach_of_the_drop_in_filter():
    """UnscentedKalmanFilter.line_approach on the committed ship 01203823 with two lines: for that ship, what the batch calls
    give (DeviceBatch.line_metrics on its smoothed track, line_chainage, line_statistics with the filter's seed and one chunk)."""
    from conftest import GOLDEN, load_cases
    from track_estimators import batch
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter
    from track_estimators.ship_track import ShipTrack

    assert os.path.exists(os.path.join(GOLDEN, "ship_01203823.csv"))
    c = load_cases("ukf_ship_01203823.npz")[0]
    st = ShipTrack()
    st.lon, st.lat, st.dts = c["z"][0].copy(), c["z"][1].copy(), c["dts"].copy()
    st.sog, st.cog, st.sog_rate, st.cog_rate, st.z = c["sog"].copy(), c["cog"].copy(), c["sog_rate"].copy(), c["cog_rate"].copy(), c["z"].copy()
    ukf = UnscentedKalmanFilter(H=c["H"], Q=c["Q"], R=c["R"], P=c["P0"], x0=st.z[:, 0].reshape(-1, 1).copy(),
                                non_linear_process=geodetic_dynamics)
    ukf.inject_noise = False
    gate = [[(0.0, 0.0), (0.0, 1.0)]]
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.line_approach(gate)
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    sm = db.sm_mean.cpu().numpy()
    k = hb.Nmax // 4 + int(np.argmax(np.hypot(*np.diff(sm[hb.Nmax // 4: 3 * hb.Nmax // 4, :2, 0], axis=0).T)))  # a step that moves
    mid, way = 0.5 * (sm[k, :2, 0] + sm[k + 1, :2, 0]), sm[k + 1, :2, 0] - sm[k, :2, 0]
    normal = np.array([-way[1], way[0]]) / np.hypot(*way)
    lines = [np.stack([mid - 0.2 * normal, mid + 0.2 * normal]), np.stack([sm[0, :2, 0] + (3.0, 1.0), sm[0, :2, 0] + (3.5, 1.5), sm[0, :2, 0] + (4.0, 1.0)])]
    tl = batch.track_lines(lines)
    want = db.line_metrics(db.sm_mean, tl, model="wgs84")
    chain = batch.line_chainage(tl, want["min_seg"], want["min_frac"], model="wgs84").cpu().numpy()
    want = _host(want)
    got = ukf.line_approach(lines, model="wgs84")
    assert set(got) == set(PER_LINE) | {"chainage"}
    for name in PER_LINE:
        assert got[name].shape == (2,) and np.array_equal(_bits(got[name]), _bits(want[name][0, :, 0])), name
    assert np.array_equal(_bits(got["chainage"]), _bits(chain[0, :, 0]))
    assert got["ncross"][0] == 1 and got["ncross"][1] == 0 and got["min_dist"][0] <= 1e-9 and got["min_dist"][1] > 50.0
    n = 5
    stats = batch.line_statistics(hb, tl, n, seed=3, chunk=n, within_km=25.0, model="wgs84")
    vis = ukf.line_approach(lines, nsamples=n, within_km=25.0, model="wgs84", random_state=3)
    for name in ("cross_prob", "net_prob", "first_cross_mean", "min_dist_mean", "approach_prob") + tuple(p + "_smoothed" for p in PER_LINE):
        assert vis[name].shape == (2,) and np.array_equal(_bits(vis[name]), _bits(stats[name][:, 0])), name
    assert vis["cross_prob"][1] == 0.0 and vis["approach_prob"][1] == 0.0 and 0.0 < vis["cross_prob"][0] <= 1.0
    with pytest.raises(ValueError, match="nsamples must be >= 0"):
        ukf.line_approach(lines, nsamples=-1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
