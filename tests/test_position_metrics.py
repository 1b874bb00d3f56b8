"""Positions of tracks on the device at query times (include/ste.h: ste_positions_f64, ste_track_positions_f64; DESIGN.md,
"Positions"): declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers, scan
against bisection, the continuation of the moments, the conditions of the fleet that the device comparison rests on and the
ellipse finishing against a closed form (CPU); on the GPU the hand-made tracks and the fleet against the restatement bit for
bit, independence of the surroundings, the statistics of sampled tracks against the smoother's covariance, the Python front
ends on a real run, and the refusals on the device build."""
import ctypes as C
import os
import re

import numpy as np
import path_metrics_cases as pmc
import position_cases as pc
import pytest
import track_sampling_cases as tsc
from conftest import GOLDEN, ROOT, load_cases

FIELDS = ["nstates", "flags", "states", "nqueries", "qtrack", "qtime", "t0", "knots", "anchor", "lon", "lat", "speed", "heading",
          "step", "frac", "status", "count", "moments"]
OUTPUTS = FIELDS[9:]
PLAIN = OUTPUTS[:7]  # the outputs that need no anchor
STAT_S, STAT_SEED = 4096, 20241  # the host draws of test_track_sampling.py::test_statistics
VAR_BOUND = 5.0 * np.sqrt(2.0 / (STAT_S - 1))


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
    proto = r"int ste_track_positions_f64\(const ste_ukf_batch_f64\* b, const ste_positions_f64\* po, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_positions_f64 {"): hdr.index("} ste_positions_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.StePositionsF64._fields_] == FIELDS
    # the layout of the C struct by hand: two 32-bit integers share a word, every pointer and the int64 take one
    offsets = {"nstates": 0, "flags": 4}
    offsets.update({name: 8 * (k + 1) for k, name in enumerate(FIELDS[2:])})
    assert {f: getattr(binding.StePositionsF64, f).offset for f in FIELDS} == offsets
    assert offsets["knots"] == 48 and offsets["lon"] == 64 and offsets["step"] == 96 and offsets["moments"] == 128
    assert C.sizeof(binding.StePositionsF64) == 136
    assert "ste_track_positions_f64" in binding.SYMBOLS
    assert hasattr(binding.load(), "ste_track_positions_f64")
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the position arguments travel beside the batch
    assert re.search(r"#define STE_POSITIONS_MAX_QUERIES \(1 << 26\)", hdr) and binding.STE_POSITIONS_MAX_QUERIES == 1 << 26
    assert int(re.search(r"#define STE_POS_REUSE_KNOTS 0x(\d+)u", hdr).group(1), 16) == binding.STE_POS_REUSE_KNOTS == 1
    assert int(re.search(r"#define STE_POS_BAD_INDEX 0x(\d+)", hdr).group(1), 16) == binding.STE_POS_BAD_INDEX == pc.BAD_INDEX == 1
    assert int(re.search(r"#define STE_POS_BAD_TIME +0x(\d+)", hdr).group(1), 16) == binding.STE_POS_BAD_TIME == pc.BAD_TIME == 2
    assert int(re.search(r"#define STE_POS_OUTSIDE +0x(\d+)", hdr).group(1), 16) == binding.STE_POS_OUTSIDE == pc.OUTSIDE == 4
    comment = hdr[hdr.index("POSITIONS:"): hdr.index("#define STE_POSITIONS_MAX_QUERIES")]
    for word in ("Knots.", "Bad index.", "Bad time.", "Locate", "Knot hit", "Interior.", "Not located.", "Moments.", "BROKEN",
                 "wrap180", "clamp01", "never extrapolates", "START FROM THE STORED VALUES", "bisection", "T_{k+1} - T_k"):
        assert word in comment, word
    assert "ste_track_positions_f64" in hdr[: hdr.index("#ifndef STE_H")]  # the list at the top of the file


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

    def good_pos():
        p = binding.StePositionsF64()
        p.nstates, p.flags, p.states, p.nqueries = 3, 0, 0x3000, 5
        for k, name in enumerate(FIELDS[4:]):
            setattr(p, name, 0x4000 + 0x1000 * k)
        return p

    def refused(reason, **fields):
        s, p = good_batch(), good_pos()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(p, name) else p, name, value)
        rc = lib.ste_track_positions_f64(ref(s), ref(p), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_track_positions_f64" in msg, (fields, rc, msg)

    for s, p, reason in ((None, good_pos(), "batch pointer is NULL"), (good_batch(), None, "position arguments (po) are NULL")):
        assert lib.ste_track_positions_f64(ref(s), ref(p), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_track_positions_f64" in msg
    for name in ("states", "qtrack", "qtime", "knots"):
        refused(f"po->{name} is required", **{name: None})
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1, (1 << 26) + 1, 1 << 40):
        refused("between 1 and STE_POSITIONS_MAX_QUERIES", nqueries=n)
    for f in (2, 3, 0x80000000):
        refused("unknown bits", flags=f)
    refused("dt is required without STE_POS_REUSE_KNOTS", dt=None)
    refused("go together", count=None)
    refused("go together", moments=None)
    refused("po->anchor is required", anchor=None)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
    # with the flag dt may be NULL: the refusal that then comes first is another one
    refused("no output asked for", dt=None, flags=1, **{name: None for name in OUTPUTS})


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_hand_answers():
    """Eight hand-made tracks, 35 named queries (position_cases.HAND_ANSWERS): a query at t0, at every knot and at the last one
    return rows; mid-step on the equator (lon 0.5, speed 11, heading 350 -> 10 through 0); a step across the antimeridian with
    one end stored wrapped (-180, inside [-180, 180)); two dt = 0 steps in a row (the smallest row wins); nsteps = 0 at t0 and
    off it; before and after the track; a NaN and a negative dt and a NaN t0; a NaN and an infinite query time; indices -1 and
    B; a NaN latitude that breaks two steps while the knots beside it answer.  Scan and bisection agree."""
    h = pc.hand_batch()
    args = (h["states"], h["nsteps"], h["dt"], h["qtrack"], h["qtime"], h["t0"])
    r = pc.positions(*args)
    pc.check_hand_answers(r, "restatement")
    _same_bits(pc.positions(*args, method="bisect"), r, "bisection on the hand-made tracks", keys=PLAIN)
    assert np.isnan(r["knots"][0, [4, 5]]).all() and not np.isnan(r["knots"][0, [0, 1, 2, 3, 6, 7]]).any()
    assert r["knots"][:, 2].tolist() == [0.0, 1.0, 1.0, 1.0, 2.0] and np.isnan(r["knots"][3:, 1]).all()


def test_conditions_of_the_fleet():
    """The restatement alone on the fleet: what the device comparison assumes of it.  Scan equals bisection on every query;
    at least 150 interior and 400 knot-hit queries; every status bit; a NaN from a broken step among the interior queries; at
    least 100 queries within a degree of the antimeridian, on either side; steps of zero hours; Q = full waves plus a partial
    one; nsteps 0 and 1 present."""
    w, ref = pc.fleet(), pc.fleet_reference()
    S, N, B, Q = pc.FLEET_S, pc.FLEET_N, pc.FLEET_B, len(w["qtrack"])
    assert w["states"].shape == (S, N + 1, 4, B) and w["dt"].shape == (N, B) and ref["lon"].shape == (S, Q)
    assert set(w["nsteps"].tolist()) == set(range(N + 1))
    assert Q > 64 and Q % 64 != 0
    bis = pc.positions(w["states"], w["nsteps"], w["dt"], w["qtrack"], w["qtime"], w["t0"], method="bisect")
    _same_bits(bis, ref, "bisection on the fleet", keys=PLAIN)
    located, interior, status = ref["located"], ref["interior"], ref["status"]
    hits = located & ~interior
    near = np.abs(np.abs(ref["lon"][0]) - 180.0) < 1.0
    broken = np.isnan(ref["lat"][:, interior]).sum()
    print(f"fleet: Q = {Q}, {int(located.sum())} located ({int(hits.sum())} knot hits, {int(interior.sum())} interior), "
          f"{int((status == pc.OUTSIDE).sum())} outside, {int((status == pc.BAD_TIME).sum())} bad time, "
          f"{int((status == pc.BAD_INDEX).sum())} bad index, {int(broken)} (sample, query) NaN from a broken step, "
          f"{int(near.sum())} within a degree of the antimeridian, {int((w['dt'] == 0.0).sum())} steps of zero hours")
    assert interior.sum() >= 150 and hits.sum() >= 400
    assert all((status == bit).any() for bit in (pc.BAD_INDEX, pc.BAD_TIME, pc.OUTSIDE)) and set(status.tolist()) <= {0, 1, 2, 4}
    assert broken >= 1
    assert near.sum() >= 100 and (ref["lon"][0][near] > 0).any() and (ref["lon"][0][near] < 0).any()
    assert (w["dt"] == 0.0).any() and (np.abs(w["states"][:, :, 0]) > 180.0).any()
    assert (ref["step"][~located] == -1).all() and np.isnan(ref["frac"][~located]).all() and (ref["frac"][hits] == 0.0).all()
    assert ((ref["frac"][interior] > 0.0) & (ref["frac"][interior] < 1.0)).all()
    lon = ref["lon"][np.isfinite(ref["lon"])]
    assert (lon >= -180.0).all() and (lon < 180.0).all()
    assert np.isnan(ref["lon"][:, ~located]).all() and (ref["count"][~located] == 0).all() and not ref["moments"][:, ~located].any()
    assert (ref["count"][located] >= S - 1).all() and (ref["count"] == S - 1).any()
    # a query at knot j returns row j of every sample
    for q in np.flatnonzero(hits):
        t, j = w["qtrack"][q], ref["step"][q]
        assert np.array_equal(_u64(ref["lat"][:, q]), _u64(w["states"][:, j, 1, t])) and np.array_equal(_u64(ref["speed"][:, q]), _u64(w["states"][:, j, 2, t]))


def test_moments_continue_bit_for_bit():
    """S = 5 in one call equals 2 + 3 on the same accumulators, in the restatement."""
    w, ref = pc.fleet(), pc.fleet_reference()
    args = (w["nsteps"], w["dt"], w["qtrack"], w["qtime"], w["t0"])
    first = pc.positions(w["states"][:2], *args, anchor=pc.fleet_anchor())
    both = pc.positions(w["states"][2:], *args, anchor=pc.fleet_anchor(), count=first["count"], moments=first["moments"])
    _same_bits(both, ref, "2 + 3 samples against 5", keys=("count", "moments"))
    assert not np.array_equal(_u64(first["moments"]), _u64(ref["moments"]))


def test_ellipse_finishing_against_a_closed_form():
    """batch.position_ellipse on moments built from a known covariance: points at +-a along an axis 30 degrees clockwise from
    north and +-b across it, on the equator (cos = 1), have covariance diag(2 a^2, 2 b^2) / 3 in that frame (n = 4, ddof 1);
    the ellipse has those axes and that orientation.  At 60 N a degree of longitude is half as many km.  count < 2 gives NaN."""
    from track_estimators import batch

    kd = 6378.137 * np.pi / 180.0
    assert batch.KM_PER_DEG == kd
    a, b, bearing = 0.3, 0.1, np.radians(30.0)
    major, minor = np.array([np.sin(bearing), np.cos(bearing)]), np.array([np.cos(bearing), -np.sin(bearing)])  # (east, north)
    pts = np.array([a * major, -a * major, b * minor, -b * minor]) + np.array([0.01, -0.02])  # degrees, with a mean offset

    def moments(p):
        dx, dy = p[:, 0], p[:, 1]
        return np.array([dx.sum(), dy.sum(), (dx * dx).sum(), (dx * dy).sum(), (dy * dy).sum()])

    m = np.stack([moments(pts), moments(pts), moments(pts[:1]), np.zeros(5)], axis=1)
    count = np.array([4, 4, 1, 0], dtype=np.int32)
    lat = np.array([0.0, 60.0, 0.0, 0.0])
    prob = 0.95
    r = batch.position_ellipse(count, m, lat, prob)
    scale = np.sqrt(-2.0 * np.log(1.0 - prob))
    assert scale == pytest.approx(2.4477468306808166, rel=1e-15)
    close = dict(rel=1e-12, abs=1e-12)
    assert r["mean_east_km"][0] == pytest.approx(0.01 * kd, **close) and r["mean_north_km"][0] == pytest.approx(-0.02 * kd, **close)
    assert r["semi_major_km"][0] == pytest.approx(scale * kd * a * np.sqrt(2.0 / 3.0), **close)
    assert r["semi_minor_km"][0] == pytest.approx(scale * kd * b * np.sqrt(2.0 / 3.0), **close)
    assert r["orientation_deg"][0] == pytest.approx(30.0, abs=1e-9)
    cov = np.cov((pts * kd).T, ddof=1)
    assert np.allclose(r["cov_km"][0], cov, rtol=1e-12, atol=1e-12) and r["cov_km"].shape == (4, 2, 2)
    # 60 N: east shrinks by cos(60 deg) = 1 / 2
    half = np.cov((pts * np.array([kd * np.cos(np.radians(60.0)), kd])).T, ddof=1)
    assert np.allclose(r["cov_km"][1], half, rtol=1e-12, atol=1e-12)
    lam = np.linalg.eigvalsh(half)
    assert r["semi_major_km"][1] == pytest.approx(scale * np.sqrt(lam[1]), **close)
    assert r["semi_minor_km"][1] == pytest.approx(scale * np.sqrt(lam[0]), **close)
    assert 0.0 < r["orientation_deg"][1] < 30.0  # squeezed towards north
    assert r["mean_east_km"][2] == pytest.approx((a * major[0] + 0.01) * kd, **close)
    for k in ("cov_km", "semi_major_km", "semi_minor_km", "orientation_deg"):
        assert np.isnan(r[k][2:]).all(), k
    assert np.isnan(r["mean_east_km"][3]) and np.isnan(r["mean_north_km"][3])
    # a circle has no orientation to get wrong; an axis along east is 90 degrees
    circ = batch.position_ellipse(np.array([4]), moments(np.array([[a, 0], [-a, 0], [0, b], [0, -b]]))[:, None], np.array([0.0]))
    assert circ["orientation_deg"][0] == pytest.approx(90.0, abs=1e-9)
    with pytest.raises(ValueError, match="prob must lie strictly between 0 and 1"):
        batch.position_ellipse(count, m, lat, 1.0)


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


_DTYPES = {"step": "int32", "status": "int32", "count": "int32"}


def _abi_call(db, states, qtrack, qtime, t0, want=PLAIN, anchor=None, accumulate=None, knots=None, batch_struct=None):
    """ste_track_positions_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor; ``want``: the outputs asked for (the
    others are NULL); ``knots``: a device tensor to reuse (STE_POS_REUSE_KNOTS); -> dict of NumPy arrays, and the knots tensor."""
    from track_estimators._hip import binding

    torch = db.torch
    s = db.struct if batch_struct is None else batch_struct
    S, Q = int(states.shape[0]), len(qtrack)
    N, ld = int(s.Nmax), int(s.track_stride or s.B)
    keep = [_dev(db, np.asarray(qtrack, dtype=np.int32)), _dev(db, np.asarray(qtime, dtype=np.float64))]
    po = binding.StePositionsF64()
    po.nstates, po.flags, po.states, po.nqueries = S, 0 if knots is None else binding.STE_POS_REUSE_KNOTS, states.data_ptr(), Q
    po.qtrack, po.qtime = keep[0].data_ptr(), keep[1].data_ptr()
    if t0 is not None:
        keep.append(_dev(db, np.asarray(t0, dtype=np.float64)))
        po.t0 = keep[-1].data_ptr()
    kn = torch.full((N + 1, ld), -7.0, dtype=torch.float64, device=db.device) if knots is None else knots
    po.knots = kn.data_ptr()
    out = {}
    for k in want:
        shape = (5, Q) if k == "moments" else ((Q,) if k in ("step", "frac", "status", "count") else (S, Q))
        out[k] = torch.zeros(shape, dtype=getattr(torch, _DTYPES.get(k, "float64")), device=db.device)
        if accumulate is not None and k in accumulate:
            out[k].copy_(_dev(db, accumulate[k]))
        setattr(po, k, out[k].data_ptr())
    if anchor is not None:
        keep.append(_dev(db, np.asarray(anchor, dtype=np.float64)))
        po.anchor = keep[-1].data_ptr()
    binding.check(db.lib.ste_track_positions_f64(C.byref(s), C.byref(po), db._stream(None)), "ste_track_positions_f64")
    torch.cuda.synchronize()
    return _host(out), kn


@pytest.mark.gpu
def test_hand_made_tracks_on_the_device():
    """The eight hand-made tracks through the C ABI: the known answers, and every output equal to the restatement bit for
    bit, NaN patterns included; the knots workspace holds the sums up to nsteps and is left alone past it."""
    from track_estimators import batch

    h = pc.hand_batch()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    plain = pc.positions(h["states"][:1], h["nsteps"], h["dt"], h["qtrack"], h["qtime"], h["t0"])
    anchor = np.round(np.nan_to_num(np.stack([plain["lon"][0], plain["lat"][0]])), 2)  # near sample 0, 0 where it has no position
    got, kn = _abi_call(db, _dev(db, h["states"]), h["qtrack"], h["qtime"], h["t0"], want=OUTPUTS, anchor=anchor)
    pc.check_hand_answers(got, "device")
    ref = pc.positions(h["states"], h["nsteps"], h["dt"], h["qtrack"], h["qtime"], h["t0"], anchor=anchor)
    _same_bits(got, ref, "hand-made tracks")
    kn = kn.cpu().numpy()
    live = np.arange(pc.HAND_N + 1)[:, None] <= h["nsteps"][None, :]
    assert np.array_equal(_u64(kn[live]), _u64(ref["knots"][live])) and (kn[~live] == -7.0).all()


def _fleet_batch():
    from track_estimators import batch

    w = pc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
def test_fleet_against_the_restatement():
    """S = 5, Nmax = 9, B = 70 ragged, Q = 754 (eleven waves and 50 lanes), half the ships astride the antimeridian: lon, lat,
    speed, heading, step, frac, status, count and moments equal the restatement bit for bit, through the front end (which
    sorts the queries and undoes it) and through the C ABI on the list as it is; a query at knot j returns row j of every
    sample; NaN in the rows past nsteps changes nothing."""
    w, db, full = _fleet_batch()
    ref = pc.fleet_reference()
    anchor = pc.fleet_anchor()
    out = db.positions_at(full, w["qtrack"], w["qtime"], t0=w["t0"], velocity=True, anchor=anchor)
    assert set(out) == set(OUTPUTS) | {"knots"} and tuple(out["knots"].shape) == (pc.FLEET_N + 1, pc.FLEET_B)
    got = _host(out)
    Q = len(w["qtrack"])
    assert got["lon"].shape == (pc.FLEET_S, Q) and got["status"].shape == (Q,) and got["moments"].shape == (5, Q)
    _same_bits(got, ref, "fleet, front end")
    raw, kn = _abi_call(db, full, w["qtrack"], w["qtime"], w["t0"], want=OUTPUTS, anchor=anchor)
    _same_bits(raw, ref, "fleet, C ABI, unsorted")
    live = np.arange(pc.FLEET_N + 1)[:, None] <= w["nsteps"][None, :]
    assert np.array_equal(_u64(kn.cpu().numpy()[live]), _u64(ref["knots"][live]))
    assert np.array_equal(_u64(got["knots"][live]), _u64(ref["knots"][live]))
    hits = ref["located"] & ~ref["interior"]
    for q in np.flatnonzero(hits):
        t, j = w["qtrack"][q], got["step"][q]
        assert np.array_equal(_u64(got["lat"][:, q]), _u64(w["states"][:, j, 1, t])), q
        assert np.array_equal(_u64(got["speed"][:, q]), _u64(w["states"][:, j, 2, t])), q
    poisoned = w["states"].copy()
    for b, ns in enumerate(w["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _host(db.positions_at(_dev(db, poisoned), w["qtrack"], w["qtime"], t0=w["t0"], velocity=True, anchor=anchor))
    _same_bits(again, got, "rows past nsteps were read")


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit: the query list reversed and shuffled; S = 1 slices against S = 5; each output alone and two subsets; the
    window [3, 70) in place and as a copy with re-based qtrack; t0 NULL against zeros; one query alone; STE_POS_REUSE_KNOTS
    against a fresh call (with dt NULL); moments in 2 + 3 against 5; Q = 64 and Q = 65."""
    w, db, full = _fleet_batch()
    qtrack, qtime, t0, anchor = w["qtrack"], w["qtime"], w["t0"], pc.fleet_anchor()
    Q, S = len(qtrack), pc.FLEET_S
    whole, knots = _abi_call(db, full, qtrack, qtime, t0, want=OUTPUTS, anchor=anchor)
    _same_bits(whole, pc.fleet_reference(), "the base of the comparisons")
    for name, perm in (("reversed", np.arange(Q)[::-1]), ("shuffled", np.random.default_rng(3).permutation(Q))):
        got, _ = _abi_call(db, full, qtrack[perm], qtime[perm], t0, want=OUTPUTS, anchor=anchor[:, perm])
        _same_bits(got, whole, name, cols_b=perm)
    for s in range(S):
        one, _ = _abi_call(db, full[s:s + 1].contiguous(), qtrack, qtime, t0)
        _same_bits(one, {k: (v[s:s + 1] if k in pc.PER_SAMPLE else v) for k, v in whole.items()}, f"sample {s} alone", keys=PLAIN)
    for want in [(k,) for k in PLAIN] + [("lon", "lat"), ("heading", "status"), ("count", "moments"), ("lat", "count", "moments")]:
        got, _ = _abi_call(db, full, qtrack, qtime, t0, want=want, anchor=anchor)
        _same_bits(got, whole, f"outputs {want}", keys=want)
    # the window [3, 70): in place on the fleet's rows (track_stride = 70) and as a batch of its own
    lo, hi = pc.FLEET_WINDOW
    inside = (qtrack >= lo) & (qtrack < hi)
    assert inside.sum() > 600
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == pc.FLEET_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _host(win.positions_at(view, qtrack[inside] - lo, qtime[inside], t0=t0[lo:hi], velocity=True, anchor=anchor[:, inside]))
        _same_bits(got, whole, f"window, copied={copied}", cols_b=inside)
        live = np.arange(pc.FLEET_N + 1)[:, None] <= w["nsteps"][None, lo:hi]
        assert np.array_equal(_u64(got["knots"][live]), _u64(knots.cpu().numpy()[:, lo:hi][live]))
    zeros, _ = _abi_call(db, full, qtrack, qtime, np.zeros(pc.FLEET_B))
    null, _ = _abi_call(db, full, qtrack, qtime, None)
    _same_bits(null, zeros, "t0 NULL against zeros", keys=PLAIN)
    _same_bits(_host(db.positions_at(full, qtrack, qtime, velocity=True)), zeros, "t0=None through the front end", keys=PLAIN)
    assert not np.array_equal(zeros["status"], whole["status"])
    k = int(np.flatnonzero(pc.fleet_reference()["interior"])[0])
    alone, _ = _abi_call(db, full, qtrack[k:k + 1], qtime[k:k + 1], t0, want=OUTPUTS, anchor=anchor[:, k:k + 1])
    _same_bits(alone, whole, "one query alone", cols_b=slice(k, k + 1))
    # the knots of the first call, read instead of summed: dt may then be NULL
    from track_estimators._hip import binding

    bare = binding.SteUkfBatchF64.from_buffer_copy(db.struct)
    bare.dt = None
    again, _ = _abi_call(db, full, qtrack, qtime, t0, want=OUTPUTS, anchor=anchor, knots=knots, batch_struct=bare)
    _same_bits(again, whole, "STE_POS_REUSE_KNOTS against a fresh call")
    first = db.positions_at(full, qtrack, qtime, t0=t0, velocity=True)
    reuse = _host(db.positions_at(full, qtrack, qtime, t0=t0, velocity=True, knots=first["knots"]))
    _same_bits(reuse, whole, "knots= through the front end", keys=PLAIN)
    # the moments of 5 samples as 2 + 3 on the same accumulators, through the C ABI and through the front end
    part, _ = _abi_call(db, full[:2].contiguous(), qtrack, qtime, t0, want=("count", "moments"), anchor=anchor)
    assert not np.array_equal(_u64(part["moments"]), _u64(whole["moments"]))
    both, _ = _abi_call(db, full[2:].contiguous(), qtrack, qtime, t0, want=("count", "moments"), anchor=anchor, accumulate=part)
    _same_bits(both, whole, "moments in 2 + 3 against 5", keys=("count", "moments"))
    a = db.positions_at(full[:2], qtrack, qtime, t0=t0, anchor=anchor)
    b = db.positions_at(full[2:], qtrack, qtime, t0=t0, anchor=anchor, accumulate=(a["count"], a["moments"]), knots=a["knots"])
    assert b["count"] is a["count"] and b["moments"] is a["moments"]
    _same_bits(_host(b), whole, "accumulate= through the front end", keys=("count", "moments"))
    _same_bits(_host(b), {k: v[2:] for k, v in whole.items() if k in ("lon", "lat")}, "its positions", keys=("lon", "lat"))
    for n in (64, 65):  # a full wave, and one lane more
        got, _ = _abi_call(db, full, qtrack[:n], qtime[:n], t0, want=OUTPUTS, anchor=anchor[:, :n])
        _same_bits(got, whole, f"Q = {n}", cols_b=slice(0, n))
    # from 16 384 queries on a lane walks all samples itself instead of one per grid row: the list repeated up to one query
    # below and up to that length, without moments (with them the lane always walks the samples)
    reps = (1 << 14) // Q + 1
    for n in ((1 << 14) - 1, 1 << 14):
        got, _ = _abi_call(db, full, np.tile(qtrack, reps)[:n], np.tile(qtime, reps)[:n], t0)
        tiled = {k: np.tile(whole[k], reps)[..., :n] for k in PLAIN}
        _same_bits(got, tiled, f"Q = {n}", keys=PLAIN)
    with pytest.raises(ValueError, match=r"qtrack must have shape \(Q,\)"):
        db.positions_at(full, qtrack[None], qtime)
    with pytest.raises(ValueError, match="integer array or tensor"):
        db.positions_at(full, qtrack.astype(np.float64), qtime)
    with pytest.raises(ValueError, match="qtime must have shape"):
        db.positions_at(full, qtrack, qtime[:-1])
    with pytest.raises(ValueError, match="anchor must have shape"):
        db.positions_at(full, qtrack, qtime, anchor=anchor.T)
    with pytest.raises(ValueError, match="accumulate must be"):
        db.positions_at(full, qtrack, qtime, anchor=anchor, accumulate=(a["moments"], a["count"]))
    with pytest.raises(ValueError, match="give the anchor"):
        db.positions_at(full, qtrack, qtime, accumulate=(a["count"], a["moments"]))
    with pytest.raises(ValueError, match="knots must be"):
        db.positions_at(full, qtrack, qtime, knots=full[0, :, 0, :3])
    with pytest.raises(ValueError, match="t0 must be None, a scalar or have shape"):
        db.positions_at(full, qtrack, qtime, t0=np.zeros(3))
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.positions_at(full[:, :, :3], qtrack, qtime)


@pytest.mark.gpu
def test_statistics():
    """The eight tracks of track_sampling_cases with the STAT_S = 4096 host draws of test_track_sampling.py::test_statistics,
    queried at every knot (104 queries), the moments continued over four calls of 1024 samples: cov_km of
    batch.position_ellipse against the lon / lat block of the smoother's covariance in the same scales (Kd cos(anchor lat) and
    Kd).  |var_S / var - 1| <= 5 sqrt(2 / (S - 1)) = 0.110 on both diagonals and the mean offsets within 5 standard errors
    sqrt(var / S): the 5-sigma bounds of the two estimators.  Measured on an MI355X: 0.055 and 2.3 standard errors."""
    from track_estimators import batch

    hb = tsc.host_batch(np.arange(8))
    db = batch.DeviceBatch(hb)
    db.run()
    N = tsc.NMAX
    T = pc.knot_times(hb.nsteps, hb.dt)
    qtrack = np.repeat(np.arange(8, dtype=np.int32), N + 1)
    qtime = T.T.reshape(-1).copy()
    sm = db.positions_at(db.sm_mean, qtrack, qtime)
    assert np.array_equal(sm["step"].cpu().numpy(), np.tile(np.arange(N + 1), 8)) and not sm["status"].any().item()
    anchor = db.torch.stack([sm["lon"][0], sm["lat"][0]])
    draws = np.random.default_rng(STAT_SEED).standard_normal((STAT_S, N + 1, 4, 8))
    acc, chunk = None, 1024
    for i in range(0, STAT_S, chunk):
        samples = db.sample_smoothed(chunk, draws=_dev(db, draws[i:i + chunk]))
        r = db.positions_at(samples, qtrack, qtime, anchor=anchor, accumulate=acc, knots=sm["knots"])
        acc = (r["count"], r["moments"])
    assert not db.sample_status.cpu().numpy().any()
    count = acc[0].cpu().numpy()
    assert (count == STAT_S).all()
    lat = anchor[1].cpu().numpy()
    e = batch.position_ellipse(count, acc[1].cpu().numpy(), lat)
    cov = db.download(("covs_smoothed",))["covs_smoothed"].reshape(8, N + 1, 4, 4)[:, :, :2, :2].reshape(-1, 2, 2)
    ke, kn = batch.KM_PER_DEG * np.cos(np.radians(lat)), batch.KM_PER_DEG
    var_e, var_n = cov[:, 0, 0] * ke * ke, cov[:, 1, 1] * kn * kn
    ratio = max(np.abs(e["cov_km"][:, 0, 0] / var_e - 1.0).max(), np.abs(e["cov_km"][:, 1, 1] / var_n - 1.0).max())
    mean = max((np.abs(e["mean_east_km"]) / np.sqrt(var_e / STAT_S)).max(), (np.abs(e["mean_north_km"]) / np.sqrt(var_n / STAT_S)).max())
    corr = np.abs(e["cov_km"][:, 0, 1] - cov[:, 0, 1] * ke * kn) / np.sqrt(var_e * var_n)
    print(f"positions at the knots, S = {STAT_S}: worst |var_S / var - 1| = {ratio:.4f} (bound {VAR_BOUND:.3f}), worst mean offset "
          f"{mean:.3f} standard errors (bound 5), worst covariance deviation {corr.max():.4f} of sqrt(var_e var_n)")
    assert ratio <= VAR_BOUND and mean <= 5.0
    assert (e["semi_major_km"] >= e["semi_minor_km"]).all() and (e["semi_minor_km"] > 0.0).all()
    assert ((e["orientation_deg"] >= 0.0) & (e["orientation_deg"] < 180.0)).all()


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    """positions_at on sm_mean and on the sampler's output of a real run against the restatement, bit for bit;
    position_statistics with one chunk equals the moments of sample_smoothed(nsamples, seed) fed in by hand; other chunks
    draw other samples after the first chunk; a HostBatch is uploaded and run first."""
    from track_estimators import batch

    hb = tsc.host_batch(np.arange(8), [12, 11, 12, 7, 12, 12, 3, 12])
    db = batch.DeviceBatch(hb)
    db.run()
    rng = np.random.default_rng(5)
    T = pc.knot_times(hb.nsteps, hb.dt)
    t0 = np.round(rng.uniform(-5.0, 5.0, 8), 1)
    qtrack = np.concatenate([np.repeat(np.arange(8), 6), [0, 3, 6, 8]]).astype(np.int32)
    span = np.array([T[hb.nsteps[t], t] for t in range(8)])
    qtime = np.concatenate([t0[qtrack[:48]] + rng.uniform(0.0, 1.0, 48) * span[qtrack[:48]], [t0[0], t0[3] + span[3], t0[6] + span[6] + 1.0, 0.0]])
    sm = db.sm_mean.cpu().numpy()[None]
    got = _host(db.positions_at(db.sm_mean, qtrack, qtime, t0=t0, velocity=True))
    ref = pc.positions(sm, hb.nsteps, hb.dt, qtrack, qtime, t0)
    _same_bits(got, ref, "smoothed tracks", keys=PLAIN)
    assert got["status"][-4:].tolist() == [0, 0, pc.OUTSIDE, pc.BAD_INDEX] and got["step"][-4:].tolist() == [0, 7, -1, -1]
    nsamples = 6
    samples = db.sample_smoothed(nsamples, seed=4)
    anchor = np.stack([got["lon"][0], got["lat"][0]])
    direct = _host(db.positions_at(samples, db.torch.from_numpy(qtrack.astype(np.int64)).to(db.device), qtime, t0=t0, velocity=True, anchor=anchor))
    _same_bits(direct, pc.positions(samples.cpu().numpy(), hb.nsteps, hb.dt, qtrack, qtime, t0, anchor=anchor), "sampled tracks")
    by_hand = batch.position_ellipse(direct["count"], direct["moments"], anchor[1])
    one = batch.position_statistics(db, qtrack, qtime, nsamples, seed=4, chunk=16, t0=t0)  # one chunk: sample_smoothed's draws
    for k in ("lon", "lat", "speed", "heading"):
        assert np.array_equal(_u64(one[k]), _u64(got[k][0])), k
    for k in ("step", "frac", "status"):
        assert one[k].dtype == got[k].dtype and np.array_equal(_u64(one[k]), _u64(got[k])), k
    assert one["count"].dtype == np.int32 and np.array_equal(one["count"], direct["count"])
    assert one["count"][:-2].tolist() == [nsamples] * 50 and one["count"][-2:].tolist() == [0, 0]
    for k, v in by_hand.items():
        assert one[k].shape == v.shape and np.array_equal(_u64(one[k]), _u64(v)), k
    assert one["cov_km"].shape == (52, 2, 2) and np.isnan(one["cov_km"][-2:]).all() and np.isfinite(one["cov_km"][:-2]).all()
    assert one["sample_status"].shape == (8,) and not one["sample_status"].any()
    two = batch.position_statistics(db, qtrack, qtime, nsamples, seed=4, chunk=2, t0=t0)  # chunks of 2: other draws after the first
    assert set(two) == set(one) and all(two[k].shape == one[k].shape and two[k].dtype == one[k].dtype for k in two)
    assert np.array_equal(two["count"], one["count"]) and np.array_equal(_u64(two["lon"]), _u64(one["lon"]))
    assert not np.array_equal(_u64(two["cov_km"][:50]), _u64(one["cov_km"][:50]))
    a = batch.position_statistics(hb, qtrack, qtime, 3, seed=9, chunk=3, t0=t0)
    b = batch.position_statistics(db, qtrack, qtime, 3, seed=9, chunk=3, t0=t0)
    assert all(np.array_equal(_u64(a[k]), _u64(b[k])) for k in b)
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.position_statistics(db, qtrack, qtime, 0)
    with pytest.raises(ValueError, match="prob must lie strictly between 0 and 1"):
        batch.position_statistics(db, qtrack, qtime, 2, prob=0.0)


@pytest.mark.gpu
def test_dropin_position_at():
    """UnscentedKalmanFilter.position_at() on the ship_01203823 golden run: at the step times it returns the smoothed rows
    (longitude through wrap180, heading through % 360), half-way through a step the mid-point, outside the track NaN; with
    n_samples the ellipse of position_statistics."""
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
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.position_at([0.0])
    N = len(c["dt"])
    ukf.run(nsteps=N, dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    rows = db.sm_mean.cpu().numpy()[:, :, 0]  # (N+1, 4)
    T = pc.knot_times(hb.nsteps, hb.dt)[:, 0]
    at = ukf.position_at(T)
    assert at.shape == (N + 1, 4) and at.dtype == np.float64
    want = np.stack([tsc.wrap180(rows[:, 0]), rows[:, 1], rows[:, 2], rows[:, 3] % 360.0], axis=1)
    assert np.array_equal(_u64(at), _u64(want))
    golden = c["means_smoothed"].reshape(N + 1, 4)  # and those are the golden run's, to the bound of test_api_dropin.py
    assert float(np.max(np.abs(rows - golden) / np.maximum(np.abs(golden), 1e-12))) < 1e-6
    k = int(np.argmax(hb.dt[:, 0] > 0.0))
    mid = ukf.position_at(0.5 * (T[k] + T[k + 1]))
    assert mid.shape == (1, 4) and mid[0, 1] == pytest.approx(0.5 * (rows[k, 1] + rows[k + 1, 1]), rel=1e-12)
    assert np.isnan(ukf.position_at([-1.0, T[-1] + 1.0])).all()
    r = ukf.position_at(T[:4], n_samples=8, random_state=2)
    assert np.array_equal(_u64(r["position"]), _u64(at[:4])) and r["count"].tolist() == [8] * 4
    assert r["cov_km"].shape == (4, 2, 2) and (r["semi_major_km"] >= r["semi_minor_km"]).all() and (r["semi_minor_km"] > 0.0).all()
    s = batch.position_statistics(hb, np.zeros(4, dtype=np.int32), T[:4], 8, seed=2, chunk=8)
    assert np.array_equal(_u64(r["cov_km"]), _u64(s["cov_km"]))
    with pytest.raises(ValueError, match="n_samples must be >= 0"):
        ukf.position_at([0.0], -1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
