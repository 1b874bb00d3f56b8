"""Values of a space-time gridded field at track positions and times (include/ste.h: ste_field_f64, ste_field_values_f64;
DESIGN.md, "Fields"): declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against hand
answers, nearest mode against the raster's row_value, the continuation of the accumulators and the conditions of the two fleet
fields that the device comparison rests on (CPU); on the GPU the hand cases and both fleets against the restatement bit for
bit, independence of the surroundings, a linear field against the positions call, the Python front ends on a real run, and
the refusals on the device build."""
import ctypes as C
import os
import re

import field_cases as fc
import numpy as np
import path_metrics_cases as pmc
import position_cases as pc
import pytest
import raster_cases as rc
import track_sampling_cases as tsc
from conftest import GOLDEN, ROOT, load_cases

FIELDS = ["nstates", "flags", "states", "nqueries", "qtrack", "qtime", "t0", "knots", "nx", "ny", "nt", "reserved", "lon0", "lat0",
          "dlon", "dlat", "lon_ref", "time0", "dtime", "min_cover", "values", "vanchor", "value", "cover", "status", "count",
          "moments", "vmin", "vmax"]
OUTPUTS = FIELDS[22:]
PLAIN = OUTPUTS[:3]  # the outputs that need no anchor
ACC = OUTPUTS[3:]


def _u64(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.float64)).view(np.uint64)


def _same_bits(a, b, what, cols_a=slice(None), cols_b=slice(None), keys=OUTPUTS):
    for k in keys:
        x, y = np.asarray(a[k])[..., cols_a], np.asarray(b[k])[..., cols_b]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(_u64(x), _u64(y)), (what, k, np.argwhere(_u64(x) != _u64(y))[:5].tolist())


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_point():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_field_values_f64\(const ste_ukf_batch_f64\* b, const ste_field_f64\* f, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_field_f64 {"): hdr.index("} ste_field_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double|void)\s*\*?\s*([\w\s,]+);", body):
        fields += [n.strip() for n in decl.split(",")]
    assert fields == [f[0] for f in binding.SteFieldF64._fields_] == FIELDS
    # the layout of the C struct by hand: no hidden padding anywhere
    offsets = {"nstates": 0, "flags": 4, "states": 8, "nqueries": 16, "qtrack": 24, "qtime": 32, "t0": 40, "knots": 48, "nx": 56,
               "ny": 60, "nt": 64, "reserved": 68, "lon0": 72, "lat0": 80, "dlon": 88, "dlat": 96, "lon_ref": 104, "time0": 112,
               "dtime": 120, "min_cover": 128, "values": 136, "vanchor": 144, "value": 152, "cover": 160, "status": 168,
               "count": 176, "moments": 184, "vmin": 192, "vmax": 200}
    assert {f: getattr(binding.SteFieldF64, f).offset for f in FIELDS} == offsets
    sizes = {f: getattr(binding.SteFieldF64, f).size for f in FIELDS}
    assert sum(sizes.values()) == C.sizeof(binding.SteFieldF64) == 208
    assert re.search(r"\} ste_field_f64;\s*/\* 208 bytes \*/", hdr)
    assert "ste_field_values_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_field_values_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264 and C.sizeof(binding.StePositionsF64) == 136  # unchanged
    assert re.search(r"#define STE_FIELD_MAX_SLABS 65536", hdr) and binding.STE_FIELD_MAX_SLABS == 65536
    assert int(re.search(r"#define STE_FLD_NEAREST 0x(\d+)u", hdr).group(1), 16) == binding.STE_FLD_NEAREST == 2
    assert int(re.search(r"#define STE_FLD_VALUES_F32 0x(\d+)u", hdr).group(1), 16) == binding.STE_FLD_VALUES_F32 == 4
    assert int(re.search(r"#define STE_FLD_TIME_OUTSIDE 0x(\d+)", hdr).group(1), 16) == binding.STE_FLD_TIME_OUTSIDE == fc.TIME_OUTSIDE == 8
    # the flags share a word with the grid's and the status with the positions': no bit twice
    assert len({binding.STE_GRID_PERIODIC_LON, binding.STE_FLD_NEAREST, binding.STE_FLD_VALUES_F32}) == 3
    assert binding.STE_FLD_TIME_OUTSIDE & (binding.STE_POS_BAD_INDEX | binding.STE_POS_BAD_TIME | binding.STE_POS_OUTSIDE) == 0
    comment = hdr[hdr.index("FIELDS:"): hdr.index("#define STE_FIELD_MAX_SLABS")]
    for word in ("Knots.", "Locate.", "Time,", "Space.", "Value.", "Nearest.", "Moments.", "BROKEN", "wrap180", "CELL CENTRES",
                 "never reads b->dt", "no extrapolation in time", "STE_FLD_TIME_OUTSIDE", "ON THE GRID", "OFF THE GRID",
                 "constant continuation", "modulo nx", "c = 4 e + 2 b + a", "(wt_e * wy_b) * wx_a", "den >= min_cover",
                 "+-inf are values", "row_value", "min(floor(gt + 0.5), nt - 1)", "START FROM THE STORED VALUES",
                 "without transcendentals"):
        assert word in comment, word
    assert "ste_field_values_f64" in hdr[: hdr.index("#ifndef STE_H")]  # the list at the top of the file
    version = hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert "(ste_field_values_f64)" in version and "(ste_ukf_noise_moments_f64, ste_ukf_noise_mstep_f64)" in version


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The pointers below are not memory: nothing may be launched, with a GPU or without one."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    pointers = [f for f in FIELDS if getattr(binding.SteFieldF64, f).size == 8 and f not in
                ("nqueries", "lon0", "lat0", "dlon", "dlat", "lon_ref", "time0", "dtime", "min_cover")]
    assert pointers == ["states", "qtrack", "qtime", "t0", "knots", "values", "vanchor"] + OUTPUTS

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.nsteps = 0x2000  # dt stays NULL: the call never reads it
        return s

    def good_field():
        f = binding.SteFieldF64()
        f.nstates, f.flags, f.nqueries = 3, 0, 5
        for k, name in enumerate(pointers):
            setattr(f, name, 0x4000 + 0x1000 * k)
        f.nx, f.ny, f.nt, f.reserved = 8, 4, 3, 0
        f.lon0, f.lat0, f.dlon, f.dlat, f.lon_ref = 10.0, -20.0, 0.5, 0.25, 12.0
        f.time0, f.dtime, f.min_cover = -6.0, 6.0, 0.5
        return f

    def refused(reason, **fields):
        s, f = good_batch(), good_field()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(f, name) else f, name, value)
        rc_ = lib.ste_field_values_f64(ref(s), ref(f), None)
        msg = lib.ste_last_error().decode()
        assert rc_ == -1 and reason in msg and "ste_field_values_f64" in msg, (fields, rc_, msg)

    for s, f, reason in ((None, good_field(), "batch pointer is NULL"), (good_batch(), None, "field arguments (f) are NULL")):
        assert lib.ste_field_values_f64(ref(s), ref(f), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_field_values_f64" in msg
    # those of the positions call that apply
    for name in ("states", "qtrack", "qtime", "knots", "values"):
        refused(f"f->{name} is required", **{name: None})
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1, (1 << 26) + 1, 1 << 40):
        refused("between 1 and STE_POSITIONS_MAX_QUERIES", nqueries=n)
    for fl in (8, 16, 0x80000000, 0x7 | 0x100):
        refused("unknown bits", flags=fl)
    refused("reserved must be 0", reserved=1)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
    # the grid's
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-2), dict(nx=1 << 14, ny=(1 << 12) + 1)):
        refused("nx * ny <= STE_GRID_MAX_CELLS", **kw)
    for name in ("lon0", "lat0", "lon_ref"):
        for v in (np.nan, np.inf):
            refused("must be finite", **{name: v})
    for name in ("dlon", "dlat"):
        for v in (np.nan, np.inf, 0.0, -1.0, 9e-7):
            refused("finite and >= 1e-6", **{name: v})
    refused("nx * dlon == 360 exactly", flags=1)
    refused("nx * dlon == 360 exactly", flags=1, nx=719, dlon=0.5)
    refused("within lon_ref +- 360", flags=1, nx=720, dlon=0.5, lon0=-180.0, lon_ref=181.0)
    refused("within lon_ref +- 90", lon_ref=101.0)
    refused("within lon_ref +- 90", nx=400, lon_ref=100.0)
    # the time axis and the cover
    for n in (0, -1, 65537):
        refused("between 1 and STE_FIELD_MAX_SLABS", nt=n)
    for v in (np.nan, np.inf, -np.inf):
        refused("time0 must be finite", time0=v)
    for v in (np.nan, np.inf, 0.0, -6.0):
        refused("dtime must be finite and > 0", dtime=v)
    for v in (np.nan, -0.25, 1.5, np.inf):
        refused("min_cover must lie in [0, 1]", min_cover=v)
    refused("vanchor is required", vanchor=None)
    for name in ACC:
        refused("vanchor is required", vanchor=None, **{k: None for k in ACC if k != name})
    refused("no output asked for", **{name: None for name in OUTPUTS})
    # a static field takes any dtime, and with no accumulator vanchor may be NULL: the refusal that then comes first is another
    refused("no output asked for", nt=1, dtime=np.nan, vanchor=None, **{name: None for name in OUTPUTS})


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_hand_answers():
    """A 4 x 3 grid of unit cells, three slabs, v = 100 j + 10 iy + ix (field_cases.HAND_ANSWERS): a knot on a node, the
    mid-point of four nodes between two slabs (30.5), a node hit half-way between slabs, the border half cells in a row and in
    a corner (constant continuation), off the grid (NaN, cover 0), both ends of the time axis and time outside it on either
    side, a query after the track and a bad index; one NaN corner of four (the other three renormalised, and NaN under
    min_cover = 0.8), all corners NaN; the column pair (nx - 1, 0) of a periodic grid; nt == 1, where time is never
    outside."""
    h, pos = fc.hand_batch(), fc.hand_positions()
    full = fc.field_values(pos, h["qtime"], fc.hand_field(), vanchor=np.zeros(len(h["qtime"])))
    fc.check_hand_answers(full, "restatement")
    assert full["count"].T.tolist() == [[1, 0, 0]] * 5 + [[0, 0, 1], [0, 0, 0], [1, 0, 0], [1, 0, 0]] + [[0, 0, 0]] * 3
    assert full["moments"][0, :5].tolist() == [0.0, 30.5, 61.0, 122.0, 153.0] and full["moments"][1, 1] == 30.5 * 30.5
    assert full["vmin"][1] == full["vmax"][1] == 30.5 and np.isnan(full["vmin"][5:7]).all()
    q = h["names"].index("mid-point of four nodes")
    one = fc.field_values(pos, h["qtime"], fc.hand_field("one nan"), vanchor=np.zeros(len(h["qtime"])))
    w0, w1 = 0.75 * 0.5 * 0.5, 0.25 * 0.5 * 0.5
    num = ((w0 * 0.0 + w0 * 1.0) + w0 * 10.0 + w1 * 100.0) + w1 * 101.0 + w1 * 110.0
    assert one["value"][0, q] == num / 0.75 and one["cover"][0, q] == 0.75 and one["count"][:, q].tolist() == [1, 0, 0]
    q0 = h["names"].index("first slab")
    assert one["value"][0, q0] == 2.75 / 0.75 and one["cover"][0, q0] == 0.75
    strict = fc.field_values(pos, h["qtime"], fc.hand_field("one nan"), min_cover=0.8, vanchor=np.zeros(len(h["qtime"])))
    assert np.isnan(strict["value"][0, q]) and strict["cover"][0, q] == 0.75 and strict["count"][:, q].tolist() == [0, 1, 0]
    assert np.isnan(one["value"][0, h["names"].index("node hit between slabs")])  # the node itself is the only corner
    none = fc.field_values(pos, h["qtime"], fc.hand_field("all nan"), vanchor=np.zeros(len(h["qtime"])))
    assert np.isnan(none["value"][0, q]) and none["cover"][0, q] == 0.0 and none["count"][:, q].tolist() == [0, 1, 0]
    # a periodic grid of four columns of 90 degrees, nodes at -135, -45, 45, 135: on the antimeridian the columns are 3 and 0
    per = (-180.0, 0.0, 90.0, 10.0, 4, 1, True, 0.0)
    vals = np.array([[[1.0, 2.0, 4.0, 8.0]]])
    for lon in (180.0, -180.0, 540.0):
        v, c, where, info = fc.sample_value(lon, 5.0, 0, 0, 0.0, per, vals)
        assert (v, c, where, info["cols"]) == (0.5 * 8.0 + 0.5 * 1.0, 1.0, fc.ON_GRID, (3, 0))
    v, c, where, info = fc.sample_value(157.5, 5.0, 0, 0, 0.0, per, vals)  # a quarter of the way from node 3 to node 0
    assert (v, info["cols"]) == (0.75 * 8.0 + 0.25 * 1.0, (3, 0))
    assert fc.sample_value(0.0, 10.0, 0, 0, 0.0, per, vals)[1:3] == (0.0, fc.OFF_GRID)  # rows do not wrap
    assert fc.sample_value(np.nan, 5.0, 0, 0, 0.0, per, vals)[2] == fc.NOWHERE
    assert fc.sample_value(np.inf, 5.0, 0, 0, 0.0, per, vals, nearest=True)[2] == fc.NOWHERE
    # +-inf are values
    assert fc.sample_value(-90.0, 5.0, 0, 0, 0.0, per, np.array([[[np.inf, 2.0, 4.0, 8.0]]]))[0] == np.inf
    # nt == 1: a static field, at any time the track is located at
    static = dict(grid=fc.HAND_GRID, values=fc.hand_values()[1:2], time0=1e9, dtime=np.nan)
    st = fc.field_values(pos, h["qtime"], static)
    assert (st["status"] & fc.TIME_OUTSIDE == 0).all() and st["value"][0, :5].tolist() == [100.0, 105.5, 111.0, 122.0, 103.0]
    assert fc.time_axis(3.0, 3, 0.0, 2.0) == (True, 1, 2, 0.5) and fc.time_axis(4.0, 3, 0.0, 2.0) == (True, 2, 2, 0.0)
    assert fc.time_axis(3.0, 3, 0.0, 2.0, nearest=True)[1] == 2 and fc.time_axis(2.9, 3, 0.0, 2.0, nearest=True)[1] == 1
    assert not fc.time_axis(np.nextafter(4.0, 5.0), 3, 0.0, 2.0)[0] and not fc.time_axis(-1e-300, 3, 0.0, 2.0)[0]


def test_nearest_mode_is_the_rasters_row_value():
    """At knot queries a sample is a row of the track, and STE_FLD_NEAREST on a static field reads the cell the raster's
    row_value reads: the two restatements agree bit for bit on every knot hit of the fleet, on both grids."""
    w, pos = pc.fleet(), pc.fleet_reference()
    hits = np.flatnonzero(pos["located"] & ~pos["interior"])
    assert len(hits) >= 400
    for name in ("global", "strip"):
        f = fc.fleet_field(name)
        static = dict(f, values=f["values"][:1])
        got = fc.field_values(pos, w["qtime"], static, nearest=True)
        on = 0
        for q in hits:
            t, j = w["qtrack"][q], pos["step"][q]
            want = [rc.row_value(w["states"][s, j, 0, t], w["states"][s, j, 1, t], f["grid"], static["values"][0]) for s in range(pc.FLEET_S)]
            assert np.array_equal(_u64(got["value"][:, q]), _u64(want)), (name, q)
            on += int(np.isfinite(want).sum())
        assert on >= 100, (name, on)
    # and in time the nearest slab, the later of two at the half
    moving = fc.fleet_reference("global", nearest=True)
    f = fc.fleet_field("global")
    located = np.flatnonzero(pos["located"] & (moving["status"] == 0))
    slabs = np.minimum(np.floor((w["qtime"][located] - f["time0"]) / f["dtime"] + 0.5), 4).astype(int)
    assert set(slabs.tolist()) == {0, 1, 2, 3, 4}
    for q, j in zip(located[:200], slabs[:200]):
        one = fc.field_values({k: v[..., q:q + 1] for k, v in pos.items() if k != "knots"}, w["qtime"][q:q + 1],
                              dict(f, values=f["values"][j:j + 1]), nearest=True)
        assert np.array_equal(_u64(one["value"][:, 0]), _u64(moving["value"][:, q]))


def test_accumulators_continue_bit_for_bit():
    """S = 5 in one call equals 2 + 3 on the same accumulators, in the restatement."""
    w, pos = pc.fleet(), pc.fleet_reference()
    for name in ("global", "strip"):
        ref, f, va = fc.fleet_reference(name), fc.fleet_field(name), fc.fleet_vanchor(name)
        part = lambda sl: {k: (v[sl] if k in pc.PER_SAMPLE else v) for k, v in pos.items()}  # noqa: E731
        first = fc.field_values(part(slice(0, 2)), w["qtime"], f, vanchor=va)
        both = fc.field_values(part(slice(2, 5)), w["qtime"], f, vanchor=va, acc=first)
        _same_bits(both, ref, f"2 + 3 samples against 5, {name}", keys=ACC)
        assert not np.array_equal(_u64(first["moments"]), _u64(ref["moments"]))
        assert np.array_equal(_u64(both["value"]), _u64(ref["value"][2:]))


def test_conditions_of_the_fleet_fields():
    """The restatement alone on the two fleet fields: what the device comparison assumes of them, so that it cannot pass on an
    empty category."""
    w, pos = pc.fleet(), pc.fleet_reference()
    S, Q = pc.FLEET_S, len(w["qtrack"])
    assert (S, pc.FLEET_N, pc.FLEET_B, Q) == (5, 9, 70, 754)
    g = fc.fleet_reference("global")
    f = fc.fleet_field("global")
    assert f["values"].shape == (5, 360, 720) and fc.fleet_field("strip")["values"].shape == (3, 15, 4)
    outside = g["status"] == fc.TIME_OUTSIDE
    info = g["info"]
    full = sum(1 for i in info.values() if i["nvalid"] == 8)
    some = sum(1 for i in info.values() if 0 < i["nvalid"] < i["ncorner"])
    none = sum(1 for i in info.values() if i["nvalid"] == 0)
    last_col = sum(1 for i in info.values() if i["cols"][0] == 719)
    cells = {}
    for (s, q), i in info.items():
        cells.setdefault(q, set()).add((i["cols"], i["rows"]))
    spread = sum(1 for c in cells.values() if len(c) > 1)
    print(f"global: {int(outside.sum())} time-outside queries; of {len(info)} (sample, query) values {full} with all eight corners "
          f"valid, {some} with some, {none} with none, {last_col} in column nx - 1; {spread} queries whose samples fall in "
          f"different cells")
    assert outside.sum() >= 50 and full >= 300 and some >= 300 and none >= 50 and last_col >= 100 and spread >= 30
    assert set(np.unique(g["status"]).tolist()) == {0, 1, 2, 4, 8}
    assert np.isnan(g["value"][:, outside]).all() and np.isnan(g["cover"][:, outside]).all() and not g["count"][:, outside].any()
    assert (g["where"][:, pos["located"] & ~outside] != fc.OFF_GRID).all()  # a periodic grid pole to pole: nothing is off it
    assert (g["where"] == fc.NOWHERE)[:, pos["located"] & ~outside].sum() >= 1  # the broken step
    assert (g["count"][0] >= 2).sum() >= 300 and (g["count"][1] > 0).sum() >= 30 and not g["count"][2].any()
    covers = g["cover"][np.isfinite(g["cover"])]
    assert ((covers > 0.0) & (covers < 1.0)).sum() >= 300 and (covers <= 1.0 + 2.0 ** -50).all()
    live = g["count"][0] > 0
    assert (g["vmin"][live] <= g["vmax"][live]).all() and np.isnan(g["vmin"][~live]).all() and np.isnan(g["vmax"][~live]).all()
    s = fc.fleet_reference("strip")
    info = s["info"]
    off = int((s["where"] == fc.OFF_GRID).sum())
    bcol = sum(1 for i in info.values() if i["cols"][0] == i["cols"][1])
    brow = sum(1 for i in info.values() if i["rows"][0] == i["rows"][1])
    counted = (s["where"] == fc.ON_GRID).any(axis=0) & (s["where"] == fc.OFF_GRID).any(axis=0)
    print(f"strip: {off} (sample, query) off the grid, {bcol} in a border column, {brow} in a border row, {int(counted.sum())} "
          f"queries with samples both on and off")
    assert off >= 500 and bcol >= 30 and brow >= 30 and counted.sum() >= 1
    assert s["count"][2].sum() == off and (s["cover"][s["where"] == fc.OFF_GRID] == 0.0).all()
    n = fc.fleet_reference("global", nearest=True)
    assert set(np.unique(n["cover"][np.isfinite(n["cover"])]).tolist()) == {0.0, 1.0}
    assert np.array_equal(n["status"], g["status"])


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _track_field(db, f, dtype=None):
    from track_estimators import batch

    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = f["grid"]
    grid = batch.TrackGrid(lon0=lon0, lat0=lat0, dlon=dlon, dlat=dlat, nx=nx, ny=ny, periodic=periodic, lon_ref=lon_ref)
    values = np.array(f["values"], dtype=dtype)  # a copy: the shared fields are read-only
    return batch.track_field(grid, values, time0=f["time0"], dtime=f["dtime"], device=db.device)


_SHAPES = {"status": ("int32", lambda S, Q: (Q,)), "count": ("int32", lambda S, Q: (3, Q)), "moments": ("float64", lambda S, Q: (2, Q)),
           "vmin": ("float64", lambda S, Q: (Q,)), "vmax": ("float64", lambda S, Q: (Q,))}


def _abi_call(db, states, tf, qtrack, qtime, t0, want=PLAIN, vanchor=None, accumulate=None, nearest=False, min_cover=0.0,
              batch_struct=None, knots=None):
    """ste_field_values_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor and a TrackField; ``want``: the
    outputs asked for (the others are NULL); the knots are those of ``db.track_knots()``; -> dict of NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    s = binding.SteUkfBatchF64.from_buffer_copy(db.struct if batch_struct is None else batch_struct)
    s.dt = None  # the call never reads it
    S, Q = int(states.shape[0]), len(qtrack)
    kn = db.track_knots() if knots is None else knots
    assert kn.stride() == (int(s.track_stride or s.B), 1)
    keep = [_dev(db, np.asarray(qtrack, dtype=np.int32)), _dev(db, np.asarray(qtime, dtype=np.float64))]
    f = binding.SteFieldF64()
    g = tf.grid
    f.nstates, f.states, f.nqueries, f.qtrack, f.qtime, f.knots = S, states.data_ptr(), Q, keep[0].data_ptr(), keep[1].data_ptr(), kn.data_ptr()
    f.flags = ((binding.STE_GRID_PERIODIC_LON if g.periodic else 0) | (binding.STE_FLD_NEAREST if nearest else 0)
               | (binding.STE_FLD_VALUES_F32 if tf.values.dtype == torch.float32 else 0))
    if t0 is not None:
        keep.append(_dev(db, np.asarray(t0, dtype=np.float64)))
        f.t0 = keep[-1].data_ptr()
    f.nx, f.ny, f.nt, f.lon0, f.lat0, f.dlon, f.dlat, f.lon_ref = g.nx, g.ny, tf.nt, g.lon0, g.lat0, g.dlon, g.dlat, g.lon_ref
    f.time0, f.dtime, f.min_cover, f.values = tf.time0, tf.dtime, min_cover, tf.values.data_ptr()
    out = {}
    for k in want:
        dtype, shape = _SHAPES.get(k, ("float64", lambda S, Q: (S, Q)))
        fill = float("nan") if k in ("vmin", "vmax") else (-7 if k in PLAIN else 0)
        out[k] = torch.full(shape(S, Q), fill, dtype=getattr(torch, dtype), device=db.device)
        if accumulate is not None and k in accumulate:
            out[k].copy_(_dev(db, accumulate[k]))
        setattr(f, k, out[k].data_ptr())
    if vanchor is not None:
        keep.append(_dev(db, np.asarray(vanchor, dtype=np.float64)))
        f.vanchor = keep[-1].data_ptr()
    binding.check(db.lib.ste_field_values_f64(C.byref(s), C.byref(f), db._stream(None)), "ste_field_values_f64")
    torch.cuda.synchronize()
    return _host(out)


@pytest.mark.gpu
def test_hand_cases_on_the_device():
    """The hand-made tracks and fields through the C ABI: the known answers, and every output equal to the restatement bit for
    bit, NaN patterns included: the full field, one NaN corner with and without min_cover, all corners NaN, nearest mode and
    a static field; track_knots equals the restatement's knots."""
    from track_estimators import batch

    h, pos = fc.hand_batch(), fc.hand_positions()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    states = _dev(db, h["states"])
    va = np.linspace(-1.0, 1.0, len(h["qtime"]))
    kn = db.track_knots()
    assert tuple(kn.shape) == (5, 2) and np.array_equal(_u64(kn.cpu().numpy()), _u64(pos["knots"]))
    got = _abi_call(db, states, _track_field(db, fc.hand_field()), h["qtrack"], h["qtime"], h["t0"], want=OUTPUTS, vanchor=va)
    fc.check_hand_answers(got, "device")
    static = dict(grid=fc.HAND_GRID, values=fc.hand_values()[1:2], time0=1e9, dtime=np.nan)
    for f, kw in ((fc.hand_field(), {}), (fc.hand_field("one nan"), {}), (fc.hand_field("one nan"), dict(min_cover=0.8)),
                  (fc.hand_field("all nan"), {}), (fc.hand_field("one nan"), dict(nearest=True)), (static, {}),
                  (static, dict(nearest=True))):
        got = _abi_call(db, states, _track_field(db, f), h["qtrack"], h["qtime"], h["t0"], want=OUTPUTS, vanchor=va, **kw)
        _same_bits(got, fc.field_values(pos, h["qtime"], f, vanchor=va, **kw), f"hand cases {kw}")


def _fleet_batch():
    from track_estimators import batch

    w = pc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["global", "strip"])
def test_fleet_against_the_restatement(name):
    """S = 5, Nmax = 9, B = 70 ragged, Q = 754 on the periodic global field (720 x 360 x 5) and on the strip astride the
    antimeridian (4 x 15 x 3): value, cover, status, count, moments, vmin and vmax equal the restatement bit for bit, trilinear
    and nearest, through the front end (which sorts the queries and undoes it) and through the C ABI on the list as it is; NaN
    in the rows past nsteps changes nothing."""
    w, db, full = _fleet_batch()
    tf, va = _track_field(db, fc.fleet_field(name)), fc.fleet_vanchor(name)
    Q = len(w["qtrack"])
    for nearest in (False, True):
        ref = fc.fleet_reference(name, nearest)
        out = db.field_at(full, tf, w["qtrack"], w["qtime"], t0=w["t0"], nearest=nearest, vanchor=va)
        assert set(out) == set(OUTPUTS) | {"knots"} and tuple(out["knots"].shape) == (pc.FLEET_N + 1, pc.FLEET_B)
        got = _host(out)
        assert got["value"].shape == (pc.FLEET_S, Q) and got["status"].shape == (Q,) and got["count"].shape == (3, Q)
        _same_bits(got, ref, f"{name}, nearest={nearest}, front end")
        raw = _abi_call(db, full, tf, w["qtrack"], w["qtime"], w["t0"], want=OUTPUTS, vanchor=va, nearest=nearest)
        _same_bits(raw, ref, f"{name}, nearest={nearest}, C ABI, unsorted")
    strict = fc.field_values(pc.fleet_reference(), w["qtime"], fc.fleet_field(name), min_cover=0.6, vanchor=va)
    assert not np.array_equal(np.isnan(strict["value"]), np.isnan(fc.fleet_reference(name)["value"]))
    got = _host(db.field_at(full, tf, w["qtrack"], w["qtime"], t0=w["t0"], min_cover=0.6, vanchor=va))
    _same_bits(got, strict, f"{name}, min_cover = 0.6")
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.field_at(_dev(db, poisoned), tf, w["qtrack"], w["qtime"], t0=w["t0"], vanchor=va))
    _same_bits(again, fc.fleet_reference(name), "rows past nsteps were read")


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit on the global field: the query list reversed and shuffled; S = 1 slices against S = 5; each output alone
    and two subsets; the window [3, 70) in place and as a copy with re-based qtrack; t0 NULL against zeros; one query alone;
    the accumulators in 2 + 3 against 5; Q = 64 and 65, and Q = 16 383 and 16 384 on either side of the mapping's threshold;
    a float field against the same values as doubles, trilinear and nearest."""
    w, db, full = _fleet_batch()
    qtrack, qtime, t0, va = w["qtrack"], w["qtime"], w["t0"], fc.fleet_vanchor("global")
    Q, S = len(qtrack), pc.FLEET_S
    tf = _track_field(db, fc.fleet_field("global"))
    whole = _abi_call(db, full, tf, qtrack, qtime, t0, want=OUTPUTS, vanchor=va)
    _same_bits(whole, fc.fleet_reference("global"), "the base of the comparisons")
    for name, perm in (("reversed", np.arange(Q)[::-1]), ("shuffled", np.random.default_rng(3).permutation(Q))):
        got = _abi_call(db, full, tf, qtrack[perm], qtime[perm], t0, want=OUTPUTS, vanchor=va[perm])
        _same_bits(got, whole, name, cols_b=perm)
    for s in range(S):
        one = _abi_call(db, full[s:s + 1].contiguous(), tf, qtrack, qtime, t0)
        _same_bits(one, {k: (v[s:s + 1] if k in ("value", "cover") else v) for k, v in whole.items()}, f"sample {s} alone", keys=PLAIN)
    for want in [(k,) for k in OUTPUTS] + [("value", "status"), ("cover", "count"), ("moments", "vmax"), ("value", "vmin", "count")]:
        got = _abi_call(db, full, tf, qtrack, qtime, t0, want=want, vanchor=va)
        _same_bits(got, whole, f"outputs {want}", keys=want)
    # the window [3, 70): in place on the fleet's rows (track_stride = 70) and as a batch of its own
    lo, hi = pc.FLEET_WINDOW
    inside = (qtrack >= lo) & (qtrack < hi)
    assert inside.sum() > 600
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == pc.FLEET_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _host(win.field_at(view, tf, qtrack[inside] - lo, qtime[inside], t0=t0[lo:hi], vanchor=va[inside]))
        _same_bits(got, whole, f"window, copied={copied}", cols_b=inside)
    raw = _abi_call(win, full[..., lo:hi], tf, qtrack[inside] - lo, qtime[inside], t0[lo:hi], want=OUTPUTS, vanchor=va[inside])
    _same_bits(raw, whole, "window in place through the C ABI", cols_b=inside)
    zeros = _abi_call(db, full, tf, qtrack, qtime, np.zeros(pc.FLEET_B))
    null = _abi_call(db, full, tf, qtrack, qtime, None)
    _same_bits(null, zeros, "t0 NULL against zeros", keys=PLAIN)
    _same_bits(_host(db.field_at(full, tf, qtrack, qtime)), zeros, "t0=None through the front end", keys=PLAIN)
    assert not np.array_equal(zeros["status"], whole["status"])
    ref = fc.fleet_reference("global")
    k = int(np.flatnonzero(pc.fleet_reference()["interior"] & (ref["count"][0] == S))[0])
    alone = _abi_call(db, full, tf, qtrack[k:k + 1], qtime[k:k + 1], t0, want=OUTPUTS, vanchor=va[k:k + 1])
    _same_bits(alone, whole, "one query alone", cols_b=slice(k, k + 1))
    # the accumulators of 5 samples as 2 + 3, through the C ABI and through the front end
    part = _abi_call(db, full[:2].contiguous(), tf, qtrack, qtime, t0, want=ACC, vanchor=va)
    assert not np.array_equal(_u64(part["moments"]), _u64(whole["moments"]))
    both = _abi_call(db, full[2:].contiguous(), tf, qtrack, qtime, t0, want=ACC, vanchor=va, accumulate=part)
    _same_bits(both, whole, "accumulators in 2 + 3 against 5", keys=ACC)
    a = db.field_at(full[:2], tf, qtrack, qtime, t0=t0, vanchor=va)
    acc = tuple(a[k] for k in ACC)
    b = db.field_at(full[2:], tf, qtrack, qtime, t0=t0, vanchor=va, accumulate=acc, knots=a["knots"], per_sample=False)
    assert all(b[k] is a[k] for k in ACC) and "value" not in b
    _same_bits(_host(b), whole, "accumulate= through the front end", keys=ACC)
    for n in (64, 65):  # a full wave, and one lane more
        got = _abi_call(db, full, tf, qtrack[:n], qtime[:n], t0, want=OUTPUTS, vanchor=va[:n])
        _same_bits(got, whole, f"Q = {n}", cols_b=slice(0, n))
    # from 16 384 queries on a lane walks all samples itself instead of one per grid row (without accumulators)
    reps = (1 << 14) // Q + 1
    for n in ((1 << 14) - 1, 1 << 14):
        got = _abi_call(db, full, tf, np.tile(qtrack, reps)[:n], np.tile(qtime, reps)[:n], t0)
        _same_bits(got, {k: np.tile(whole[k], reps)[..., :n] for k in PLAIN}, f"Q = {n}", keys=PLAIN)
    # a float field: the same bits as its values widened to doubles
    f32 = fc.fleet_field("global")["values"].astype(np.float32)
    wide = dict(fc.fleet_field("global"), values=f32.astype(np.float64))
    tf32 = _track_field(db, dict(wide, values=f32))
    assert tf32.values.dtype == db.torch.float32 and tf.values.dtype == db.torch.float64
    for nearest in (False, True):
        a32 = _abi_call(db, full, tf32, qtrack, qtime, t0, want=OUTPUTS, vanchor=va, nearest=nearest)
        a64 = _abi_call(db, full, _track_field(db, wide), qtrack, qtime, t0, want=OUTPUTS, vanchor=va, nearest=nearest)
        _same_bits(a32, a64, f"float field, nearest={nearest}")
        _same_bits(a32, fc.field_values(pc.fleet_reference(), qtime, wide, nearest=nearest, vanchor=va), "float field, restatement")
    assert not np.array_equal(_u64(a64["value"]), _u64(fc.fleet_reference("global", True)["value"]))
    with pytest.raises(ValueError, match="field must be a TrackField"):
        db.field_at(full, fc.fleet_field("global"), qtrack, qtime)
    with pytest.raises(ValueError, match=r"min_cover must lie in \[0, 1\]"):
        db.field_at(full, tf, qtrack, qtime, min_cover=1.5)
    with pytest.raises(ValueError, match="vanchor must have shape"):
        db.field_at(full, tf, qtrack, qtime, vanchor=va[:-1])
    with pytest.raises(ValueError, match="accumulate must be"):
        db.field_at(full, tf, qtrack, qtime, vanchor=va, accumulate=acc[::-1])
    with pytest.raises(ValueError, match="give the vanchor"):
        db.field_at(full, tf, qtrack, qtime, accumulate=acc)
    with pytest.raises(ValueError, match="knots must be"):
        db.field_at(full, tf, qtrack, qtime, knots=full[0, :, 0, :3])
    with pytest.raises(ValueError, match=r"qtrack must have shape \(Q,\)"):
        db.field_at(full, tf, qtrack[None], qtime)


LIN_A, LIN_B, LIN_C, LIN_D = 1.0, 0.25, 0.5, 0.125


@pytest.mark.gpu
def test_linear_field_against_the_positions_call():
    """A field that is linear in lon, lat and time with dyadic coefficients on the global grid's dyadic node coordinates has
    exact node values, and trilinear interpolation reproduces a linear function: on the queries whose samples all lie inside
    the node hull (off the periodic seam) value = a + b x + c lat + d tq with x, lat from positions_at, within
    2^-45 max|values|: about 128 roundings of 2^-52 for at most eight products, seven additions and a division, and the
    cancellation of weights that sum to 1 only to rounding.  The accumulators equal the sums formed from the per-sample value
    in order, bit for bit.  Measured on an MI355X: 308 queries, worst 4.3e-14 against the bound 2.7e-12."""
    w, db, full = _fleet_batch()
    lon0, lat0, dlon, dlat, nx, ny, periodic, lon_ref = fc.GLOBAL_GRID
    nt, time0, dtime = 5, -36.0, 18.0
    j, iy, ix = np.meshgrid(np.arange(nt), np.arange(ny), np.arange(nx), indexing="ij")
    values = LIN_A + LIN_B * (lon0 + (ix + 0.5) * dlon) + LIN_C * (lat0 + (iy + 0.5) * dlat) + LIN_D * (time0 + j * dtime)
    tf = _track_field(db, dict(grid=fc.GLOBAL_GRID, values=values, time0=time0, dtime=dtime))
    po = _host(db.positions_at(full, w["qtrack"], w["qtime"], t0=w["t0"]))
    va = np.round(np.nan_to_num(LIN_A + LIN_B * po["lon"][0] + LIN_C * po["lat"][0]), 1)
    got = _host(db.field_at(full, tf, w["qtrack"], w["qtime"], t0=w["t0"], vanchor=va))
    x, lat, tq = po["lon"], po["lat"], w["qtime"]
    hull = (np.isfinite(x) & (x >= lon0 + 0.5 * dlon) & (x <= lon0 + (nx - 0.5) * dlon) & (lat >= lat0 + 0.5 * dlat)
            & (lat <= lat0 + (ny - 0.5) * dlat)).all(axis=0) & (tq >= time0) & (tq <= time0 + (nt - 1) * dtime)
    assert hull.sum() >= 150 and (got["status"][hull] == 0).all()
    want = LIN_A + LIN_B * x[:, hull] + LIN_C * lat[:, hull] + LIN_D * tq[hull]
    worst = float(np.abs(got["value"][:, hull] - want).max())
    bound = 2.0 ** -45 * float(np.abs(values).max())
    print(f"linear field: {int(hull.sum())} queries inside the node hull, worst |value - (a + b x + c lat + d tq)| = {worst:.3e} "
          f"(bound {bound:.3e} = 2^-45 max|values|), worst |cover - 1| = {float(np.abs(got['cover'][:, hull] - 1.0).max()):.3e}")
    assert worst <= bound
    # the accumulators from the per-sample values, in order
    Q = len(tq)
    count, mom = np.zeros((3, Q), dtype=np.int32), np.zeros((2, Q))
    vmin, vmax = np.full(Q, np.nan), np.full(Q, np.nan)
    with np.errstate(all="ignore"):
        for s in range(pc.FLEET_S):
            v = got["value"][s]
            d = v - va
            ok = np.isfinite(v) & np.isfinite(d)
            count[0] += ok
            mom[0] = np.where(ok, mom[0] + d, mom[0])
            mom[1] = np.where(ok, mom[1] + d * d, mom[1])
            vmin = np.where(ok & ~(vmin <= v), v, vmin)
            vmax = np.where(ok & ~(vmax >= v), v, vmax)
    _same_bits(got, dict(count=count[0], moments=mom, vmin=vmin, vmax=vmax), "accumulators from the values",
               keys=("moments", "vmin", "vmax"))
    assert np.array_equal(got["count"][0], count[0]) and not got["count"][1].any() and not got["count"][2].any()


def _run_field(device):
    """A smooth global field of 1 degree and 4 slabs that covers the eight tracks of track_sampling_cases, with a block of no
    data, as float32."""
    from track_estimators import batch

    grid = batch.track_grid(-180.0, -90.0, 1.0, 1.0, 360, 180)
    assert grid.periodic and grid.lon_ref == 0.0
    j, iy, ix = np.meshgrid(np.arange(4), np.arange(180), np.arange(360), indexing="ij")
    values = (10.0 + 5.0 * np.sin(ix * (np.pi / 180.0)) + 0.1 * iy + 0.5 * j).astype(np.float32)
    values[:, 100:104, :] = np.nan
    return batch.track_field(grid, values, time0=-1.0, dtime=6.0, device=device), grid, values


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    """field_at on sm_mean and on the sampler's output of a real run against the restatement, bit for bit; field_statistics
    with one chunk equals the accumulators of sample_smoothed(nsamples, seed) finished by hand; with chunks of 16 it equals
    ONE field_at call on the same 40 draws; a HostBatch is uploaded and run first; no (S, Q) array comes back."""
    from track_estimators import batch

    hb = tsc.host_batch(np.arange(8), [12, 11, 12, 7, 12, 12, 3, 12])
    db = batch.DeviceBatch(hb)
    db.run()
    torch = db.torch
    tf, grid, values = _run_field(db.device)
    f = dict(grid=(grid.lon0, grid.lat0, grid.dlon, grid.dlat, grid.nx, grid.ny, grid.periodic, grid.lon_ref), values=values,
             time0=-1.0, dtime=6.0)
    rng = np.random.default_rng(5)
    T = pc.knot_times(hb.nsteps, hb.dt)
    t0 = np.round(rng.uniform(-1.0, 1.0, 8), 1)
    qtrack = np.concatenate([np.repeat(np.arange(8), 6), [0, 3, 6, 8]]).astype(np.int32)
    span = np.array([T[hb.nsteps[t], t] for t in range(8)])
    qtime = np.concatenate([t0[qtrack[:48]] + rng.uniform(0.0, 1.0, 48) * span[qtrack[:48]], [t0[0], t0[3] + span[3], t0[6] + span[6] + 1.0, 0.0]])
    sm = db.sm_mean.cpu().numpy()[None]
    got = _host(db.field_at(db.sm_mean, tf, qtrack, qtime, t0=t0))
    pos = pc.positions(sm, hb.nsteps, hb.dt, qtrack, qtime, t0)
    _same_bits(got, fc.field_values(pos, qtime, f), "smoothed tracks", keys=PLAIN)
    assert got["status"][-4:].tolist() == [0, 0, pc.OUTSIDE, pc.BAD_INDEX] and np.isfinite(got["value"][0, :48]).sum() >= 24
    nsamples = 6
    samples = db.sample_smoothed(nsamples, seed=4)
    va = np.nan_to_num(got["value"][0])
    direct = _host(db.field_at(samples, tf, torch.from_numpy(qtrack.astype(np.int64)).to(db.device), qtime, t0=t0, vanchor=va))
    spos = pc.positions(samples.cpu().numpy(), hb.nsteps, hb.dt, qtrack, qtime, t0)
    _same_bits(direct, fc.field_values(spos, qtime, f, vanchor=va), "sampled tracks")

    def finish(r, ns):
        n = r["count"][0].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            md = r["moments"][0] / n
            var = (r["moments"][1] - r["moments"][0] * md) / np.where(n >= 2, n - 1.0, np.nan)
        return {"anchor": got["value"][0], "mean": va + md, "std": np.sqrt(np.maximum(var, 0.0)), "min": r["vmin"], "max": r["vmax"],
                "n": r["count"][0], "p_nodata": r["count"][1] / float(ns), "p_off": r["count"][2] / float(ns), "status": got["status"]}

    one = batch.field_statistics(db, tf, qtrack, qtime, nsamples, seed=4, chunk=16, t0=t0)  # one chunk: sample_smoothed's draws
    assert set(one) == {"anchor", "mean", "std", "min", "max", "n", "p_nodata", "p_off", "status", "sample_status"}
    for k, v in finish(direct, nsamples).items():
        assert one[k].shape == (52,) and one[k].dtype == v.dtype and np.array_equal(_u64(one[k]), _u64(v)), k
    assert one["n"].dtype == np.int32 and one["n"][-2:].tolist() == [0, 0] and (one["n"] + 6 * one["p_nodata"] <= 6).all()
    assert np.isfinite(one["std"][one["n"] >= 2]).all() and np.isnan(one["std"][one["n"] < 2]).all()
    assert one["sample_status"].shape == (8,) and not one["sample_status"].any()
    with np.errstate(invalid="ignore"):
        assert ((one["min"] <= one["mean"] + 1e-9) & (one["mean"] <= one["max"] + 1e-9))[one["n"] > 0].all()
    # chunks of 16 on 40 samples: the same draws laid end to end and given to one call
    gen = torch.Generator(device=db.device)
    gen.manual_seed(9)
    buf = torch.empty((16, tsc.NMAX + 1, 4, 8), dtype=torch.float64, device=db.device)
    drawn = []
    for n in (16, 16, 8):
        buf[:n].normal_(generator=gen)
        drawn.append(db.sample_smoothed(n, draws=buf[:n]).clone())
    at_once = _host(db.field_at(torch.cat(drawn), tf, qtrack, qtime, t0=t0, vanchor=va, per_sample=False))
    chunked = batch.field_statistics(db, tf, qtrack, qtime, 40, seed=9, chunk=16, t0=t0)
    for k, v in finish(at_once, 40).items():
        assert np.array_equal(_u64(chunked[k]), _u64(v)), k
    assert chunked["n"].max() == 40 and not np.array_equal(_u64(chunked["std"]), _u64(one["std"]))
    a = batch.field_statistics(hb, tf, qtrack, qtime, 3, seed=9, chunk=3, t0=t0)
    b = batch.field_statistics(db, tf, qtrack, qtime, 3, seed=9, chunk=3, t0=t0)
    assert all(np.array_equal(_u64(a[k]), _u64(b[k])) for k in b)
    near = batch.field_statistics(db, tf, qtrack, qtime, 3, seed=9, chunk=3, t0=t0, nearest=True)
    assert set(np.unique(near["anchor"][np.isfinite(near["anchor"])]).tolist()) <= set(np.unique(values[np.isfinite(values)]).astype(np.float64).tolist())
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.field_statistics(db, tf, qtrack, qtime, 0)
    # track_field: what it takes and what it refuses
    assert tf.values.dtype == torch.float32 and tf.nt == 4
    flat = batch.track_field(grid, values[0].astype(np.float64), device=db.device)
    assert flat.nt == 1 and flat.values.dtype == torch.float64 and tuple(flat.values.shape) == (1, 180, 360)
    assert batch.track_field(grid, np.ones((180, 360), dtype=np.int16), device=db.device).values.dtype == torch.float64
    assert batch.track_field(grid, tf.values).values is tf.values
    with pytest.raises(ValueError, match=r"must have shape \(ny, nx\)"):
        batch.track_field(grid, values[:, :, :-1], device=db.device)
    with pytest.raises(ValueError, match="dtime must be finite and > 0"):
        batch.track_field(grid, values, dtime=0.0, device=db.device)
    with pytest.raises(ValueError, match="time0 must be finite"):
        batch.track_field(grid, values, time0=np.nan, device=db.device)
    with pytest.raises(ValueError, match="grid must be a TrackGrid"):
        batch.track_field(f["grid"], values, device=db.device)


@pytest.mark.gpu
def test_dropin_field_at():
    """UnscentedKalmanFilter.field_at() on the ship_01203823 golden run: with n_samples = 0 it is field_at(sm_mean) of the
    batch run() packed; with n_samples the dict of field_statistics."""
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
    N = len(c["dt"])
    tf, _, _ = _run_field("cuda:0")
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.field_at(tf, [0.0])
    ukf.run(nsteps=N, dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    T = pc.knot_times(hb.nsteps, hb.dt)[:, 0]
    times = np.concatenate([T[:6], 0.5 * (T[:5] + T[1:6]), [-1.0, T[-1] + 1.0]])
    at = ukf.field_at(tf, times)
    assert at.shape == (13,) and at.dtype == np.float64 and np.isnan(at[-2:]).all()
    want = db.field_at(db.sm_mean, tf, np.zeros(13, dtype=np.int32), times)["value"][0].cpu().numpy()
    assert np.array_equal(_u64(at), _u64(want))
    r = ukf.field_at(tf, times[:4], n_samples=8, random_state=2)
    s = batch.field_statistics(hb, tf, np.zeros(4, dtype=np.int32), times[:4], 8, seed=2, chunk=8)
    assert set(r) == set(s) - {"sample_status"} and all(np.array_equal(_u64(r[k]), _u64(s[k])) for k in r)
    assert np.array_equal(_u64(r["anchor"]), _u64(at[:4]))
    with pytest.raises(ValueError, match="n_samples must be >= 0"):
        ukf.field_at(tf, [0.0], -1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
