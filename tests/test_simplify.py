"""Simplification of tracks on the device within a tolerance (include/ste.h: ste_simplify_f64, ste_track_simplify_f64; DESIGN.md,
"Simplification"): declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against hand answers, its
properties on the walk fleet and the conditions the device comparison rests on (CPU); on the GPU the hand-made ships, the walk
fleet, the unbalanced ship, the workspace path, independence of the surroundings, truncation and the identity, all BIT FOR BIT
against the restatement, the Python front ends on a real run, and the refusals on the device build."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import simplify_cases as sc
from conftest import ROOT

FIELDS = ["nstates", "flags", "cap", "reserved", "states", "tolerance", "tolerance_all", "lon_scale", "lon_scale_all", "work",
          "work_bytes", "keep", "nkeep", "worst_sq", "status", "rows", "out_states", "out_dt"]
PLAIN = ("keep", "nkeep", "worst_sq", "status")
COMPACT = ("rows", "out_states", "out_dt")
OUTPUTS = PLAIN + COMPACT
MODES = (False, True)  # shape


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for proto in (r"int ste_track_simplify_f64\(const ste_ukf_batch_f64\* b, const ste_simplify_f64\* sf, void\* stream\);",
                  r"size_t ste_track_simplify_workspace\(int32_t Nmax, int32_t nstates, int32_t B\);",
                  r"int ste_track_simplify_lds_rows\(void\);"):
        assert re.search("^" + proto, hdr, flags=re.M), proto
    body = hdr[hdr.index("typedef struct ste_simplify_f64 {"): hdr.index("} ste_simplify_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|uint8_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteSimplifyF64._fields_] == FIELDS
    # the layout of the C struct by hand: four 32-bit words, then every pointer, double and int64 takes one 8-byte word
    offsets = {"nstates": 0, "flags": 4, "cap": 8, "reserved": 12}
    offsets.update({name: 16 + 8 * k for k, name in enumerate(FIELDS[4:])})
    assert {f: getattr(binding.SteSimplifyF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteSimplifyF64) == 128 and re.search(r"} ste_simplify_f64;\s*/\* 128 bytes \*/", hdr)
    lib = binding.load()
    for name in ("ste_track_simplify_f64", "ste_track_simplify_workspace", "ste_track_simplify_lds_rows"):
        assert name in binding.SYMBOLS and hasattr(lib, name)
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340 == lib.ste_version()
    assert "(ste_track_simplify_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert " *   ste_track_simplify_f64 " in hdr[: hdr.index("Conventions")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the arguments travel beside the batch
    assert int(re.search(r"#define STE_SIMPLIFY_SHAPE 0x(\d+)u", hdr).group(1), 16) == binding.STE_SIMPLIFY_SHAPE == 1
    for name, value in (("BAD_TIME", sc.BAD_TIME), ("BAD_LIMIT", sc.BAD_LIMIT), ("BROKEN", sc.BROKEN), ("TRUNCATED", sc.TRUNCATED)):
        found = int(re.search(rf"#define STE_SIMPLIFY_{name} 0x(\d+)", hdr).group(1), 16)
        assert found == getattr(binding, "STE_SIMPLIFY_" + name) == value, name
    assert (sc.BAD_TIME, sc.BAD_LIMIT, sc.BROKEN, sc.TRUNCATED) == (1, 2, 4, 8)
    comment = hdr[hdr.index("SIMPLIFICATION:"): hdr.index("#define STE_SIMPLIFY_SHAPE")]
    for word in ("Clock.", "Unwrapped longitude.", "Metric.", "Deviation", "Rule.", "Compaction.", "Work.", "BROKEN", "SMALLEST",
                 "without contraction", "bit for bit", "STARTING FROM THE FIRST TERM", "Refused with STE_EINVAL"):
        assert word in comment, word
    rows = lib.ste_track_simplify_lds_rows()
    assert rows >= 64 and rows * 25 + 256 <= 65536
    assert lib.ste_track_simplify_workspace(rows - 1, 16, 100) == 0
    assert lib.ste_track_simplify_workspace(rows, 1, 1) == 64 * (rows + 1) * 32
    assert lib.ste_track_simplify_workspace(rows, 16, 10000) == 1024 * (rows + 1) * 32


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The device pointers below are not memory: nothing may be launched, with a GPU or without one."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    big = lib.ste_track_simplify_lds_rows()

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.dt, s.nsteps = 0x1000, 0x2000
        return s

    def good_args():
        e = binding.SteSimplifyF64()
        e.nstates, e.flags, e.cap, e.reserved, e.states = 3, 0, 5, 0, 0x3000
        e.tolerance, e.tolerance_all, e.lon_scale, e.lon_scale_all = 0x4000, float("nan"), 0x5000, float("nan")
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x6000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_args()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc = lib.ste_track_simplify_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_track_simplify_f64" in msg, (fields, rc, msg)

    for s, e, reason in ((None, good_args(), "batch pointer is NULL"), (good_batch(), None, "simplification arguments (sf) are NULL")):
        assert lib.ste_track_simplify_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_track_simplify_f64" in msg
    refused("sf->states is required", states=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for f in (2, 3, 0x80000000):
        refused("sf->flags must be 0 or STE_SIMPLIFY_SHAPE", flags=f)
    refused("reserved must be 0", reserved=1)
    for v in (float("nan"), float("inf"), -0.5):
        refused("tolerance_all must be finite and >= 0", tolerance=None, tolerance_all=v)
        refused("lon_scale_all must be finite and >= 0", lon_scale=None, lon_scale_all=v)
    for c in (-1, 14, 1 << 30):
        refused("cap must be between 1 and Nmax + 1", cap=c)
    none = {name: None for name in COMPACT}
    for name in COMPACT:  # one compaction output is enough
        refused("need sf->cap", cap=0, **{k: v for k, v in none.items() if k != name})
    refused("batch's dt is required", dt=None)
    refused("batch's dt is required", dt=None, flags=binding.STE_SIMPLIFY_SHAPE)  # out_dt is given
    refused("batch's dt is required", dt=None, flags=binding.STE_SIMPLIFY_SHAPE, rows=None, out_states=None)
    refused("no output asked for", dt=None, flags=binding.STE_SIMPLIFY_SHAPE, **{name: None for name in OUTPUTS})  # dt not read
    refused("no output asked for", **{name: None for name in OUTPUTS})
    refused("sf->work is required", Nmax=big, work=None)
    refused("sf->work is required", Nmax=big, work=0x9000, work_bytes=lib.ste_track_simplify_workspace(big, 3, 8) - 1)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("limited to 2^31 - 257", Nmax=2 ** 31 - 200)
    refused("track_stride", track_stride=7)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def _hand_restatement(shape, cap=7):
    h = sc.hand_batch()
    return sc.simplify(h["states"], h["nsteps"], h["dt"], h["tol"], 1.0, shape, cap)


def test_restatement_against_hand_answers():
    """Eleven hand-made ships on the equator with scale 1 (simplify_cases.HAND_SHIPS names them)."""
    h = sc.hand_batch()
    col = {name: t for t, name in enumerate(sc.HAND_SHIPS)}
    for shape in MODES:
        got = _hand_restatement(shape)
        sc.check_hand_answers(got, f"restatement, shape={shape}", shape)
        t = col["corner"]
        X, Y, T, status = sc.staged(h["states"][0, :, 0, t], h["states"][0, :, 1, t], h["dt"][:, t], shape)
        assert status == 0 and sc.deviations(X, Y, T, 1.0, 0, 6, shape)[2] == 4.5  # row 3
        t = col["tie"]
        X, Y, T, _ = sc.staged(h["states"][0, :5, 0, t], h["states"][0, :5, 1, t], h["dt"][:4, t], shape)
        assert sc.deviations(X, Y, T, 1.0, 0, 4, shape).tolist() == [1.0, 0.0, 1.0]  # rows 1 and 3 tie: the first wins
        t = col["antimeridian"]
        assert (np.abs(np.diff(h["states"][0, :, 0, t])) > 300.0).sum() == 1  # the stored longitudes do jump
        # the identity of a bad track carries every row, its own dt and all four components
        t = col["neg_dt"]
        if not shape:
            assert got["rows"][0, :, t].tolist() == list(range(7)) and np.array_equal(got["out_dt"][0, :, t], h["dt"][:, t])
            assert np.array_equal(got["out_states"][0, :, :, t], h["states"][0, :, :, t])
        t = col["pace"]
        assert got["out_dt"][0, :2, t].tolist() == ([3.0, 9.0] if not shape else [12.0, sc.SENTINEL])


@pytest.mark.parametrize("shape", MODES)
def test_restatement_properties_on_the_walk_fleet(shape):
    """Every dropped row is within the tolerance of the chord between its surviving neighbours, recomputed by the formula;
    tolerance 0 keeps every row; the order in which ranges are taken changes nothing; and what the device comparison assumes of
    the fleet: all the strip-edge lengths, several ships across the antimeridian, and at each tolerance at least a quarter of
    the tracks keeping strictly between 2 and ns + 1 rows."""
    w = sc.walk()
    assert w["states"].shape == (3, 200, 4, 24)
    assert {0, 1, 2, 62, 63, 64, 65, 127, 128, 129, 199} <= set(w["nsteps"].tolist())
    for t in sc.WALK_ANTIMERIDIAN:
        ns = int(w["nsteps"][t])
        assert (np.abs(np.diff(w["states"][0, :ns + 1, 0, t])) > 300.0).any(), t
    rng = np.random.default_rng(3)
    for tol_km in sc.WALK_TOL_KM:
        ref = sc.walk_reference(tol_km, shape)
        tol = sc.walk_tolerance(tol_km)
        assert not ref["status"].any()
        between = 0
        for s in range(sc.WALK_S):
            for t, ns in enumerate(w["nsteps"]):
                args = (w["states"][s, :ns + 1, 0, t], w["states"][s, :ns + 1, 1, t], w["dt"][:ns, t], w["scale"][t], tol[t], shape)
                keep = ref["keep"][s, :ns + 1, t]
                worst = sc.dropped_rows_within_tolerance(*args, keep)
                assert worst == ref["worst_sq"][s, t] and keep[0] == 1 and keep[ns] == 1
                assert (ref["keep"][s, ns + 1:, t] == sc.SENTINEL_B).all() and ref["nkeep"][s, t] == keep.sum()
                if tol_km == 0.0:
                    assert keep.all(), (s, t)
                between += 2 < keep.sum() < ns + 1
                if s == 0:
                    for order in ("fifo", "random"):
                        other = sc.simplify_track(*args, order=order, rng=rng)
                        assert np.array_equal(other[0], keep) and other[1] == ref["worst_sq"][s, t], (t, order)
        print(f"walk fleet, shape={shape}, {tol_km} km: {between} of {sc.WALK_S * sc.WALK_B} tracks keep some rows; kept fraction "
              f"{ref['nkeep'].sum() / (sc.WALK_S * (w['nsteps'] + 1).sum()):.3f}")
        if tol_km > 0.0:
            assert between >= sc.WALK_S * sc.WALK_B / 4, (tol_km, between)
    assert not np.array_equal(sc.walk_reference(1.0, shape)["keep"], sc.walk_reference(10.0, shape)["keep"])
    assert not np.array_equal(sc.walk_reference(1.0, False)["keep"], sc.walk_reference(1.0, True)["keep"])


@pytest.mark.parametrize("shape", MODES)
def test_unbalanced_ship_is_unbalanced(shape):
    """x_k = k, y_k = (-1)^k (n - k) / n at tolerance 0: a depth-first traversal that pushes both parts gets at least 64 levels
    deep on 160 rows, where a balanced recursion has 8."""
    u = sc.unbalanced()
    assert u["states"].shape[1] == sc.UNBALANCED_ROWS >= 130
    keep, worst, status, depth = sc.simplify_track(u["states"][0, :, 0, 0], u["states"][0, :, 1, 0], u["dt"][:, 0], 1.0, 0.0, shape)
    print(f"unbalanced ship, shape={shape}: depth {depth}, kept {int(keep.sum())} of {len(keep)}")
    assert status == 0 and depth >= 64 and keep.sum() > 130


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _abi_call(states, nsteps, dt, tol, scale, shape, cap=None, want=None, work=True):
    """ste_track_simplify_f64 through ctypes on contiguous device copies, a batch struct that carries B, Nmax, nsteps and dt
    alone; ``tol`` and ``scale``: a scalar (the *_all field) or (B,); ``want``: the outputs asked for (the others are NULL),
    each pre-filled with its sentinel; ``work``: allocate the workspace the sizes need.  -> (rc, dict of NumPy arrays)."""
    import torch
    from track_estimators._hip import binding

    lib = binding.require_gpu()
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    S, rows, _, B = states.shape
    N = rows - 1
    keep = [up(states), up(np.asarray(nsteps, dtype=np.int32))]
    b = binding.SteUkfBatchF64()
    b.B, b.Nmax, b.n, b.nsteps = B, N, 4, keep[1].data_ptr()
    if dt is not None:
        keep.append(up(np.asarray(dt, dtype=np.float64)))
        b.dt = keep[-1].data_ptr()
    sf = binding.SteSimplifyF64()
    sf.nstates, sf.flags, sf.states = S, (binding.STE_SIMPLIFY_SHAPE if shape else 0), keep[0].data_ptr()
    for name, v in (("tolerance", tol), ("lon_scale", scale)):
        if np.ndim(v) == 0:
            setattr(sf, name + "_all", float(v))
        else:
            keep.append(up(np.asarray(v, dtype=np.float64)))
            setattr(sf, name, keep[-1].data_ptr())
    need = lib.ste_track_simplify_workspace(N, S, B)
    if need and work:
        keep.append(torch.empty((need // 8,), dtype=torch.float64, device=dev))
        sf.work, sf.work_bytes = keep[-1].data_ptr(), need
    if want is None:
        want = PLAIN + (COMPACT if cap is not None else ())
    if cap is not None:
        sf.cap = cap
    shapes = {"keep": ((S, rows, B), torch.uint8, sc.SENTINEL_B), "nkeep": ((S, B), torch.int32, sc.SENTINEL_I),
              "worst_sq": ((S, B), torch.float64, sc.SENTINEL), "status": ((S, B), torch.int32, sc.SENTINEL_I),
              "rows": ((S, cap or 1, B), torch.int32, sc.SENTINEL_I), "out_states": ((S, cap or 1, 4, B), torch.float64, sc.SENTINEL),
              "out_dt": ((S, (cap or 1) - 1, B), torch.float64, sc.SENTINEL)}
    out = {}
    for k in want:
        shp, dtype, fill = shapes[k]
        out[k] = torch.full(shp, fill, dtype=dtype, device=dev)
        setattr(sf, k, out[k].data_ptr() if out[k].numel() else 0x10)  # an array of no entries: any pointer that is not NULL
    rc = lib.ste_track_simplify_f64(C.byref(b), C.byref(sf), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, ref, what, keys=None):
    """Bit for bit, sentinels included: integers equal, doubles with equal bits."""
    for k in (got if keys is None else keys):
        g, r = got[k], ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        same = _bits(g) == _bits(r)
        assert same.all(), (what, k, int((~same).sum()), np.argwhere(~same)[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MODES)
def test_hand_made_ships_on_the_device(shape):
    h = sc.hand_batch()
    rc, got = _abi_call(h["states"], h["nsteps"], h["dt"], h["tol"], 1.0, shape, cap=7)
    assert rc == 0
    sc.check_hand_answers(got, f"device, shape={shape}", shape)
    _same(got, _hand_restatement(shape), f"hand-made ships, shape={shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MODES)
def test_walk_fleet_against_the_restatement(shape):
    """S = 3, Nmax = 199, 24 ships whose lengths are the strip edges of the 64-lane scan and of the compaction, per-track
    tolerances (0, about 1 km and about 10 km) and scales: every output bit for bit."""
    w = sc.walk()
    for tol_km in sc.WALK_TOL_KM:
        rc, got = _abi_call(w["states"], w["nsteps"], w["dt"], sc.walk_tolerance(tol_km), w["scale"], shape, cap=sc.WALK_N + 1)
        assert rc == 0
        _same(got, sc.walk_reference(tol_km, shape), f"walk fleet, shape={shape}, {tol_km} km")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MODES)
def test_unbalanced_ship_on_the_device(shape):
    """Splits that take one row off an end each time: a kernel whose stack grew with the unbalance would go wrong here."""
    u = sc.unbalanced()
    rc, got = _abi_call(u["states"], u["nsteps"], u["dt"], 0.0, 1.0, shape, cap=sc.UNBALANCED_ROWS)
    assert rc == 0
    _same(got, sc.simplify(u["states"], u["nsteps"], u["dt"], 0.0, 1.0, shape, sc.UNBALANCED_ROWS), f"unbalanced ship, shape={shape}")


@pytest.mark.gpu
def test_long_track_goes_through_the_workspace():
    """One track of ste_track_simplify_lds_rows() + 70 rows: refused without the workspace, equal to the restatement with it."""
    from track_estimators._hip import binding

    lib = binding.load()
    rows = lib.ste_track_simplify_lds_rows() + 70
    lt = sc.long_track(rows)
    tol = 0.5 / sc.KM_PER_DEG
    rc, _ = _abi_call(lt["states"], lt["nsteps"], lt["dt"], tol, 0.98, False, cap=rows, work=False)
    assert rc == -1 and "sf->work is required" in lib.ste_last_error().decode()
    for shape in MODES:
        ref = sc.simplify(lt["states"], lt["nsteps"], lt["dt"], tol, 0.98, shape, rows)
        assert 10 < ref["nkeep"][0, 0] < rows // 4 and ref["status"][0, 0] == 0
        rc, got = _abi_call(lt["states"], lt["nsteps"], lt["dt"], tol, 0.98, shape, cap=rows)
        assert rc == 0
        _same(got, ref, f"long track, shape={shape}")


def _walk_db():
    import path_metrics_cases as pmc
    from track_estimators import batch

    w = sc.walk()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, db.torch.from_numpy(w["states"]).to(db.device)


def _front(db, states, tol_km_per_track, scale, shape, **kw):
    out = db.simplify_tracks(states, tol_km_per_track, shape=shape, lon_scale=scale, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MODES)
def test_same_bits_whatever_the_surroundings(shape):
    """Bit for bit: each sample alone against S = 3; the window WALK_WINDOW in place on the fleet's rows (track_stride) and as
    a contiguous copy; each output alone and subsets against all outputs; a scalar tolerance against the same value per track."""
    w, db, full = _walk_db()
    tol_km = w["factor"] * 1.0
    ref = sc.walk_reference(1.0, shape)
    m = int(ref["nkeep"].max())
    whole = _front(db, full, tol_km, w["scale"], shape)
    assert whole["states"].shape == (sc.WALK_S, m, 4, sc.WALK_B) and whole["dt"].shape == (sc.WALK_S, m - 1, sc.WALK_B)
    assert np.array_equal(whole["keep"], np.where(ref["keep"] == sc.SENTINEL_B, 0, ref["keep"]))
    _same(whole, ref, "front end", ("nkeep", "status"))
    live = ref["rows"][:, :m] >= 0
    assert np.array_equal(whole["rows"][live], ref["rows"][:, :m][live]) and (whole["rows"][~live] == -1).all()
    assert np.array_equal(_bits(whole["states"].transpose(0, 1, 3, 2)[live]), _bits(ref["out_states"][:, :m].transpose(0, 1, 3, 2)[live]))
    assert np.array_equal(_bits(whole["dt"][live[:, 1:]]), _bits(ref["out_dt"][:, :m - 1][live[:, 1:]]))
    assert np.array_equal(_bits(whole["worst_km"]), _bits(np.sqrt(ref["worst_sq"]) * sc.KM_PER_DEG))
    keys = ("keep", "nkeep", "worst_km", "status", "rows", "states", "dt")

    def cut(out, n):  # narrowed to n rows, as a call on fewer tracks narrows
        return {**out, "rows": out["rows"][:, :n], "states": out["states"][:, :n], "dt": out["dt"][:, :n - 1]}

    for s in range(sc.WALK_S):
        one = _front(db, full[s], tol_km, w["scale"], shape)
        n = one["rows"].shape[1]
        _same(one, {k: v[s:s + 1] for k, v in cut(whole, n).items() if k in keys}, f"sample {s} alone", keys)
    lo, hi = sc.WALK_WINDOW
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == sc.WALK_B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = _front(win, view, tol_km[lo:hi], w["scale"][lo:hi], shape)
        n = got["rows"].shape[1]
        _same(got, {k: v[..., lo:hi] for k, v in cut(whole, n).items() if k in keys}, f"window, copied={copied}", keys)
    tol = sc.walk_tolerance(1.0)
    for want in [(k,) for k in OUTPUTS] + [("keep", "out_dt"), ("nkeep", "rows", "status"), ("worst_sq", "out_states")]:
        rc, got = _abi_call(w["states"], w["nsteps"], w["dt"], tol, w["scale"], shape, cap=sc.WALK_N + 1, want=want)
        assert rc == 0
        _same(got, ref, f"outputs {want}", want)
    if shape:  # no clock is read when no out_dt is asked for
        rc, got = _abi_call(w["states"], w["nsteps"], None, tol, w["scale"], True, cap=sc.WALK_N + 1, want=PLAIN + ("rows", "out_states"))
        assert rc == 0
        _same(got, ref, "shape without dt")
    flat = _front(db, full, float(tol_km[5]), float(w["scale"][5]), shape)
    each = _front(db, full, np.full(sc.WALK_B, tol_km[5]), np.full(sc.WALK_B, w["scale"][5]), shape)
    assert "lon_scale" not in flat and np.array_equal(each.pop("lon_scale"), np.full(sc.WALK_B, w["scale"][5]))
    _same(flat, each, "a scalar tolerance against one per track")
    _same({k: flat[k][..., 5:6] for k in ("keep", "nkeep", "worst_km", "status")}, {k: whole[k][..., 5:6] for k in whole},
          "track 5 under its own tolerance")
    with pytest.raises(ValueError, match="tolerance_km must be a scalar or have shape"):
        db.simplify_tracks(full, np.zeros(3))
    with pytest.raises(ValueError, match="lon_scale must be 'track'"):
        db.simplify_tracks(full, 1.0, lon_scale="mercator")
    with pytest.raises(ValueError, match="max_rows must be None or between 1 and"):
        db.simplify_tracks(full, 1.0, max_rows=0)


@pytest.mark.gpu
def test_truncation():
    """cap below nkeep: the first cap kept rows, STE_SIMPLIFY_TRUNCATED and the true nkeep; through the front end as max_rows."""
    w, db, full = _walk_db()
    cap = 9
    ref = sc.walk_reference(1.0, False, cap)
    cut = ref["nkeep"] > cap
    assert cut.any() and not cut.all() and (ref["nkeep"] == cap).sum() >= 0
    assert np.array_equal((ref["status"] & sc.TRUNCATED) != 0, cut) and np.array_equal(ref["nkeep"], sc.walk_reference(1.0, False)["nkeep"])
    rc, got = _abi_call(w["states"], w["nsteps"], w["dt"], sc.walk_tolerance(1.0), w["scale"], False, cap=cap)
    assert rc == 0
    _same(got, ref, "truncated")
    front = _front(db, full, w["factor"] * 1.0, w["scale"], False, max_rows=cap)
    assert front["rows"].shape == (sc.WALK_S, cap, sc.WALK_B)
    assert np.array_equal(front["rows"], np.where(ref["rows"] == sc.SENTINEL_I, -1, ref["rows"]))
    _same(front, ref, "front end, truncated", ("nkeep", "status"))


@pytest.mark.gpu
def test_identity_reproduces_the_batch():
    """Tolerance 0 on the walk, compacted: rows 0 .. ns of states and dt bit for bit, and ste_path_metrics_f64 on that block,
    through a batch struct that carries B, Nmax = cap - 1, nsteps = nkeep - 1 and dt = out_dt alone, returns the dist bits of
    the original."""
    from track_estimators._hip import binding

    w, db, full = _walk_db()
    torch = db.torch
    out = db.simplify_tracks(full, 0.0, lon_scale=torch.from_numpy(w["scale"]))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["states"].shape == w["states"].shape and got["dt"].shape == (sc.WALK_S,) + w["dt"].shape
    assert not got["status"].any() and (got["worst_km"] == 0.0).all()
    for t, ns in enumerate(w["nsteps"]):
        assert (got["nkeep"][:, t] == ns + 1).all() and (got["rows"][:, :ns + 1, t] == np.arange(ns + 1)).all()
        assert np.array_equal(_bits(got["states"][:, :ns + 1, :, t]), _bits(w["states"][:, :ns + 1, :, t])), t
        assert np.array_equal(_bits(got["dt"][:, :ns, t]), _bits(np.broadcast_to(w["dt"][:ns, t], (sc.WALK_S, ns)))), t
    want = db.path_metrics(full)["distance"].cpu().numpy()
    block, ns = out["states"].contiguous(), (out["nkeep"][0] - 1).contiguous()
    dist = torch.full((sc.WALK_S, sc.WALK_B), sc.SENTINEL, dtype=torch.float64, device=db.device)
    for s in range(sc.WALK_S):  # out_dt is per sample: one call per sample, each on its own dt
        b = binding.SteUkfBatchF64()
        b.B, b.Nmax, b.n = sc.WALK_B, block.shape[1] - 1, 4
        dts = out["dt"][s].contiguous()
        b.nsteps, b.dt = ns.data_ptr(), dts.data_ptr()
        pm = binding.StePathF64()
        pm.nstates, pm.model, pm.states, pm.line_axis = 1, binding.STE_PREP_SPHERE, block[s].data_ptr(), -1
        pm.dist = dist[s].data_ptr()
        binding.check(db.lib.ste_path_metrics_f64(C.byref(b), C.byref(pm), db._stream(None)), "ste_path_metrics_f64")
        torch.cuda.synchronize()
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want))


def _real_batch():
    """Four synthetic tracks of 20 steps through the filter and the smoother; track 3 is short."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(4, nobs=11, seed0=100)
    hb = batch.pack_uniform(sb, 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 20, 13], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    return hb, db


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MODES)
def test_front_ends_on_a_real_run(shape):
    """simplify_tracks on sm_mean of a real run: the guarantee recomputed in NumPy from the download, worst_km <= tolerance,
    lon_scale="track" against the NumPy cosine rule (cos is the one transcendental here, and it is torch's on the device
    against NumPy's: each is within an ulp of the true cosine, so they may differ by 2 ulp of a value below 1, 2^-52), and
    batch.simplified_tracks returning exactly the kept rows of the full download."""
    from track_estimators import batch

    hb, db = _real_batch()
    down = db.download(("means_smoothed", "means"))
    for which, mean_t, mean in (("smoothed", db.sm_mean, down["means_smoothed"]), ("filtered", db.fwd_mean, down["means"])):
        spans = [float(np.ptp(mean[t, :ns + 1, 1]) * sc.KM_PER_DEG) for t, ns in enumerate(hb.nsteps)]
        tol_km = 0.05 * max(spans)
        out = {k: v.cpu().numpy() for k, v in db.simplify_tracks(mean_t, tol_km, shape=shape).items()}
        rule = np.array([np.cos(np.radians(np.abs(mean[t, :ns + 1, 1]).min())) for t, ns in enumerate(hb.nsteps)])
        assert np.abs(out["lon_scale"] - rule).max() <= 2.0 ** -52, np.abs(out["lon_scale"] - rule).max()
        assert not out["status"].any() and (out["worst_km"] <= tol_km).all()
        ref = sc.simplify(mean.transpose(1, 2, 0)[None], hb.nsteps, hb.dt, tol_km / sc.KM_PER_DEG, out["lon_scale"], shape)
        assert np.array_equal(out["keep"], np.where(ref["keep"] == sc.SENTINEL_B, 0, ref["keep"])) and np.array_equal(out["nkeep"], ref["nkeep"])
        assert (out["nkeep"][0] < hb.nsteps + 1).any()
        for t, ns in enumerate(hb.nsteps):
            worst = sc.dropped_rows_within_tolerance(mean[t, :ns + 1, 0], mean[t, :ns + 1, 1], hb.dt[:ns, t], out["lon_scale"][t],
                                                     tol_km / sc.KM_PER_DEG, shape, out["keep"][0, :ns + 1, t])
            assert np.sqrt(worst) * sc.KM_PER_DEG == out["worst_km"][0, t]
        ships = batch.simplified_tracks(db, tol_km, which=which, shape=shape)
        assert len(ships) == hb.B and len(ships.curves()) == hb.B
        for t, ship in enumerate(ships):
            r = np.flatnonzero(out["keep"][0, :, t])
            assert ship["rows"].tolist() == r.tolist() and ship["status"] == 0 and ship["worst_km"] == out["worst_km"][0, t]
            for c, name in enumerate(("lon", "lat", "speed", "heading")):
                assert np.array_equal(_bits(ship[name]), _bits(mean[t, r, c])), (t, name)
            assert np.array_equal(ship["time"], np.concatenate([[0.0], np.cumsum(hb.dt[:, t])])[r])
            assert ship.curve().shape == (len(r), 2) and np.array_equal(ships.curves()[t], ship.curve())
    viahb = batch.simplified_tracks(hb, tol_km, shape=shape)
    ships = batch.simplified_tracks(db, tol_km, shape=shape)
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for a, b in zip(viahb, ships) for k in ("rows", "lon", "lat", "speed", "heading", "time"))
    with pytest.raises(ValueError, match="which must be 'smoothed' or 'filtered'"):
        batch.simplified_tracks(db, 1.0, which="raw")


@pytest.mark.gpu
def test_simplified_track_of_the_drop_in_filter():
    """UnscentedKalmanFilter.simplified_track on the committed ship 01203823: the kept rows of the full download of that ship."""
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
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.simplified_track(1.0)
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    mean = db.download(("means_smoothed",))["means_smoothed"][0]
    tol_km = 0.05 * float(np.ptp(mean[:, 1])) * sc.KM_PER_DEG  # a twentieth of the track's extent in latitude
    for shape in MODES:
        got = ukf.simplified_track(tol_km, shape=shape)
        keep = db.simplify_tracks(db.sm_mean, tol_km, shape=shape, compact=False)["keep"][0, :, 0].cpu().numpy()
        r = np.flatnonzero(keep)
        assert got["rows"].tolist() == r.tolist() and 2 <= len(r) < hb.Nmax + 1 and got["worst_km"] <= tol_km and got["status"] == 0
        for col, name in enumerate(("lon", "lat", "speed", "heading")):
            assert np.array_equal(_bits(got[name]), _bits(mean[r, col])), name
        assert len(got.curves()) == 1 and got.curves()[0].shape == (len(r), 2)
        print(f"ship 01203823, shape={shape}: {len(r)} of {hb.Nmax + 1} rows within {tol_km:.2f} km")


@pytest.mark.gpu
def test_refusals_before_any_launch():
    _abi_refusals()
