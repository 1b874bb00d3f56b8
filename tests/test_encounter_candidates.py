"""Candidate pairs for encounters, found on the device (include/ste.h: CANDIDATES, ste_candidates_f64,
ste_encounter_candidates_mask_f64 / _list_f64; DESIGN.md, "Candidates"): declaration and layout of the C ABI, the refusals, the
NumPy restatement against hand answers, the guarantee (every pair the encounter restatement brings within R is listed, whatever
the windows) and the point of the feature (ocean voyages: a tenth of the cap list or less) on the CPU; on the GPU the hand-made
ships, boxes and lists against the restatement at the tile and word edges, independence of the surroundings bit for bit, the
Python front ends on a real run, and the refusals on the device build.

Tolerances.  Window occupancy, ranges, emptiness and status are functions of in-order sums, one division and a floor: exact.
h has no trigonometry: bit for bit.  A box corner is a product of two sines / cosines of the same radians on both sides, the
device held to 1.5 ulp per function and libm to 1: (1.5 + 1.5 + 0.5) + (1 + 1 + 0.5) = 6 ulp of 1 =
1.4e-15 absolute.  A pair-window test is grazing when |g2 - c^2| <= 1e-9 c^2, six orders above that; every fleet below is shown
on the CPU to have none, and then the device list, wfirst and nwin must equal the restatement's exactly."""
import ctypes as C
import os
import re

import candidate_cases as cc
import encounter_cases as enc
import numpy as np
import path_metrics_cases as pmc
import pytest
from conftest import ROOT

FIELDS = ["states", "t0", "track_margin_km", "reach_km", "time0", "window_h", "nwindows", "flags", "reserved", "reserved_pad",
          "workspace", "workspace_bytes", "track_status", "row_offset", "npairs", "pairs", "wfirst", "nwin"]
CALLS = ("ste_encounter_candidates_mask_f64", "ste_encounter_candidates_list_f64")
_CACHE = {}


def _restated(name, w, reach, W, time0, NW, t0="own", margin=None):
    """cc.candidates, computed once per case and never changed."""
    key = (name, reach, W, time0, NW, t0 if isinstance(t0, str) else "given", margin is not None)
    if key not in _CACHE:
        clock = w["t0"] if isinstance(t0, str) else t0
        _CACHE[key] = cc.candidates(w["states"][0], w["nsteps"], w["dt"], reach, W, time0, NW, clock, margin)
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for call in CALLS:
        assert re.search(r"^int " + call + r"\(const ste_ukf_batch_f64\* b, const ste_candidates_f64\* c, void\* stream\);", hdr,
                         flags=re.M), call
        assert call in binding.SYMBOLS and hasattr(binding.load(), call)
    assert re.search(r"^size_t ste_encounter_candidates_workspace\(int32_t B, int32_t nwindows\);", hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_candidates_f64 {"): hdr.index("} ste_candidates_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|uint64_t|double|void)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteCandidatesF64._fields_] == FIELDS
    offsets = {"states": 0, "t0": 8, "track_margin_km": 16, "reach_km": 24, "time0": 32, "window_h": 40, "nwindows": 48,
               "flags": 52, "reserved": 56, "reserved_pad": 60}
    offsets.update({name: 64 + 8 * k for k, name in enumerate(FIELDS[10:])})
    assert {f: getattr(binding.SteCandidatesF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteCandidatesF64) == 128
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the candidate arguments travel beside the batch
    assert int(re.search(r"#define STE_CANDIDATES_MAX_WINDOWS (\d+)", hdr).group(1)) == binding.STE_CANDIDATES_MAX_WINDOWS == 4096
    assert float(re.search(r"#define STE_CANDIDATES_MAX_REACH_KM ([\d.]+)", hdr).group(1)) == binding.STE_CANDIDATES_MAX_REACH_KM
    assert binding.STE_CANDIDATES_MAX_REACH_KM / cc.EARTH_KM < np.pi  # theta stays a bound below the half circle
    assert re.search(r"#define STE_CANDIDATES_MAX_TRACKS \(1 << 20\)", hdr) and binding.STE_CANDIDATES_MAX_TRACKS == 1 << 20
    for name, bit in (("BAD_TIME", cc.BAD_TIME), ("CLIPPED", cc.CLIPPED), ("EMPTY", cc.EMPTY), ("BAD_MARGIN", cc.BAD_MARGIN)):
        assert int(re.search(r"#define STE_CAND_" + name + r" +0x(\d+)", hdr).group(1), 16) == getattr(binding, "STE_CAND_" + name) == bit
    comment = hdr[hdr.index("CANDIDATES:"): hdr.index("#define STE_CANDIDATES_MAX_WINDOWS")]
    for word in ("Clock.", "Windows.", "Sound steps.", "Boxes.", "Near.", "Output.", "GUARANTEE.", "Determinism.", "BAD CLOCK",
                 "BROKEN", "EMPTY", "NEAR", "monotone", "1e-7", "wrap180", "row_offset", "No atomics"):
        assert word in comment, word
    assert "ste_encounter_candidates_mask_f64" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    lib = binding.load()
    size = lib.ste_encounter_candidates_workspace
    assert size(130, 65) == 8 * (7 * 65 * 130 + 130 * 3) + 12 * 130 and size(64, 1) == 8 * (7 * 64 + 64) + 12 * 64
    assert size(0, 4) == 0 and size(5, 0) == 0 and size(-1, 3) == 0


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

    def good_cand():
        c = binding.SteCandidatesF64()
        c.states, c.t0, c.track_margin_km = 0x3000, 0x4000, 0x5000
        c.reach_km, c.time0, c.window_h, c.nwindows, c.flags, c.reserved = 30.0, -5.0, 6.0, 7, 0, 0
        c.workspace, c.workspace_bytes, c.track_status = 0x10000, lib.ste_encounter_candidates_workspace(8, 7), 0x6000
        c.row_offset, c.npairs, c.pairs, c.wfirst, c.nwin = 0x7000, 5, 0x8000, 0x9000, 0xa000
        return c

    def refused(reason, calls=CALLS, **fields):
        for call in calls:
            s, c = good_batch(), good_cand()
            for name, value in fields.items():
                setattr(s if hasattr(s, name) and not hasattr(c, name) else c, name, value)
            rc = getattr(lib, call)(ref(s), ref(c), None)
            msg = lib.ste_last_error().decode()
            assert rc == -1 and reason in msg and call in msg, (call, fields, rc, msg)

    for call in CALLS:
        for s, c, reason in ((None, good_cand(), "batch pointer is NULL"), (good_batch(), None, "candidate arguments (c) are NULL")):
            assert getattr(lib, call)(ref(s), ref(c), None) == -1
            msg = lib.ste_last_error().decode()
            assert reason in msg and call in msg
    refused("c->states is required", states=None)
    refused("batch's dt is required", dt=None)
    for v in (0.0, -6.0, float("nan"), float("inf")):
        refused("window_h must be finite and > 0", window_h=v)
    for v in (float("nan"), float("inf"), -float("inf")):
        refused("time0 must be finite", time0=v)
    for n in (0, -1, 4097):
        refused("between 1 and STE_CANDIDATES_MAX_WINDOWS", nwindows=n)
    for r in (float("nan"), float("inf"), -1e-300, -5.0, 20000.000000000004, 1e9):
        refused("reach_km must be finite and between 0 and STE_CANDIDATES_MAX_REACH_KM", reach_km=r)
    for f in (1, 0x80000000):
        refused("c->flags must be 0", flags=f)
        refused("c->reserved must be 0", reserved=f)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("STE_CANDIDATES_MAX_TRACKS", B=(1 << 20) + 1, workspace_bytes=1 << 62)
    refused("Nmax >= 0", Nmax=-1)
    refused("track_stride", track_stride=7)
    refused("c->workspace is required", workspace=None)
    refused("aligned to 8 bytes", workspace=0x10004)
    refused("workspace_bytes is below", workspace_bytes=lib.ste_encounter_candidates_workspace(8, 7) - 1)
    refused("workspace_bytes is below", nwindows=8)
    refused("c->track_status is required", calls=CALLS[:1], track_status=None)
    refused("c->row_offset is required", calls=CALLS[1:], row_offset=None)
    refused("c->pairs is required", calls=CALLS[1:], pairs=None)
    for n in (0, -1, (1 << 26) + 1):
        refused("between 1 and STE_ENCOUNTER_MAX_PAIRS", calls=CALLS[1:], npairs=n)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_hand_answers():
    """Seventeen hand-made ships (candidate_cases.hand_batch): a lane sailed a day apart, a pair astride the antimeridian, one
    across the pole, a step of ten windows, a track that ends exactly on a window boundary, tracks before time0 and after the
    last window, nsteps 0 and 1, a NaN latitude in mid-track, a NaN dt inside nsteps (the track ends there) and one past it, a NaN t0 and a
    negative margin.  The list at W = 6 h is the one worked out by hand; the lane pair is in the cap list and in the list of one
    window, and not in the windowed one; no pair-window grazes."""
    import torch
    from track_estimators import batch

    h = cc.hand_batch()
    r = _restated("hand", h, cc.HAND_REACH, cc.HAND_W, 0.0, cc.HAND_NW)
    cc.check_hand_answers(r, "restatement")
    assert r["ngrazing"] == 0 and r["ntests"] > 100
    assert cc.clock_windows(h["nsteps"][:8], h["dt"][:, :8], h["t0"][:8], cc.HAND_W) == (0.0, cc.HAND_NW)
    one = _restated("hand", h, cc.HAND_REACH, cc.HAND_W, 0.0, 1)
    keys1 = set(map(tuple, one["pairs"].tolist()))
    assert (0, 1) in keys1 and (1, 8) in keys1 and set(cc.HAND_PAIRS) <= keys1 and one["ngrazing"] == 0
    assert (one["nwin"] == 1).all() and (one["wfirst"] == 0).all()
    assert one["status"].tolist() == [cc.HAND_STATUS.get(t, 0) | (0 if t in (10, 15) else cc.CLIPPED) for t in range(cc.HAND_B)]
    with np.errstate(invalid="ignore"):
        cap = batch.candidate_pairs(torch.from_numpy(h["states"][0].copy()), torch.from_numpy(h["nsteps"]),
                                    torch.from_numpy(np.nan_to_num(h["dt"], nan=2.0)), cc.HAND_REACH, t0=torch.from_numpy(h["t0"]))
    assert [0, 1] in cap.tolist()
    m = _restated("hand", h, cc.HAND_REACH, cc.HAND_W, 0.0, cc.HAND_NW, margin=h["margin"])  # ship 16 leaves, nothing else moves
    assert m["status"][16] == cc.BAD_MARGIN and m["pairs"].tolist() == [list(p) for p in cc.HAND_PAIRS if 16 not in p]
    big = h["margin"].copy()
    big[16], big[1] = 0.0, 300.0  # 300 km for ship 1 alone reaches ship 0, 267 km ahead of it
    assert [0, 1] in cc.candidates(h["states"][0], h["nsteps"], h["dt"], cc.HAND_REACH, cc.HAND_W, 0.0, cc.HAND_NW, h["t0"], big)["pairs"].tolist()


def _met(w, R):
    """The pairs i < j (all of them are tried) that the encounter restatement brings within R in sample 0."""
    B = w["states"].shape[3]
    every = np.array([(i, j) for i in range(B) for j in range(i + 1, B)], dtype=np.int32)
    ref = enc.encounter_metrics(w["states"][:1], w["nsteps"], w["dt"], every, R, w["t0"])
    return every[ref["nwithin"][0] > 0]


def test_guarantee_every_encounter_is_listed():
    """On the meeting fleet (all 2 415 pairs) and on encounter_cases' hand batch (all 120): every pair with nwithin > 0 at
    R = 30 km is in the restated list for reach 30.3 km (the 0.2 % of the planar metric, and more), at W = 0.25, 1, 4 and 100 h
    over the fleet's own clock range, and in the list of one window that starts below every clock."""
    for name, w, least in (("meeting fleet", enc.fleet(), 400), ("hand batch", enc.hand_batch(), 5)):
        B = w["states"].shape[3]
        met = _met(w, 30.0)
        assert len(met) >= least, (name, len(met))
        t0 = np.where(np.isfinite(w["t0"]), w["t0"], 0.0)
        for W in (0.25, 1.0, 4.0, 100.0):
            time0, NW = cc.clock_windows(w["nsteps"], np.nan_to_num(w["dt"], nan=1.0), t0, W)
            r = _restated(name, w, 30.3, W, time0, NW)
            missed = ~np.isin(cc.pair_keys(met, B), cc.pair_keys(r["pairs"], B))
            print(f"{name}, W = {W} h: {NW} windows, {len(r['pairs'])} candidates for {len(met)} encounters of {B * (B - 1) // 2} pairs")
            assert not missed.any(), (name, W, met[missed].tolist())
            assert len(r["pairs"]) < B * (B - 1) // 2
        r = _restated(name, w, 30.3, 1000.0, -500.0, 1)
        assert np.isin(cc.pair_keys(met, B), cc.pair_keys(r["pairs"], B)).all() and not (r["status"] & cc.CLIPPED).any()


def test_voyages_are_pruned_to_a_tenth_of_the_cap_list():
    """The point of the feature: 300 ships that cross oceans, 200 steps each.  The restated list at W = 24 h is a subset of
    batch.candidate_pairs' list and at most a tenth of it."""
    import torch
    from track_estimators import batch

    w = cc.voyage_fleet(300, 200)
    B = 300
    cap = batch.candidate_pairs(torch.from_numpy(w["states"][0].copy()), torch.from_numpy(w["nsteps"]), torch.from_numpy(w["dt"]),
                                30.0, t0=torch.from_numpy(w["t0"])).numpy()
    time0, NW = cc.clock_windows(w["nsteps"], w["dt"], w["t0"], 24.0)
    r = _restated("voyage", w, 30.0, 24.0, time0, NW)
    print(f"voyage fleet: {len(cap)} cap pairs, {len(r['pairs'])} windowed pairs in {NW} windows, of {B * (B - 1) // 2}")
    assert np.isin(cc.pair_keys(r["pairs"], B), cc.pair_keys(cap, B)).all()
    assert 0 < 10 * len(r["pairs"]) <= len(cap)
    assert r["ngrazing"] == 0


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _batch(w):
    from track_estimators import batch

    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return db, _dev(db, w["states"])


def _abi_call(db, states, reach, W, time0, NW, t0=None, margin=None, details=True, batch_struct=None, stream=None):
    """The two calls through ctypes on a contiguous (1, N+1, 4, B) device tensor, the prefix between them by torch -> dict of
    NumPy arrays: pairs, wfirst, nwin (details), status, and the workspace's box (NW, 7, B), wlo, whi, count."""
    from track_estimators._hip import binding

    torch = db.torch
    s = db.struct if batch_struct is None else batch_struct
    B = int(s.B)
    keep = [None if v is None else _dev(db, np.asarray(v, dtype=np.float64)) for v in (t0, margin)]
    c = binding.SteCandidatesF64()
    c.states, c.reach_km, c.time0, c.window_h, c.nwindows = states.data_ptr(), reach, time0, W, NW
    c.t0, c.track_margin_km = (None if v is None else v.data_ptr() for v in keep)
    nbytes = db.lib.ste_encounter_candidates_workspace(B, NW)
    nwords = (B + 63) // 64
    assert nbytes == 8 * (7 * NW * B + B * nwords) + 12 * B
    work = torch.full(((nbytes + 7) // 8 + 1,), -1, dtype=torch.int64, device=db.device)
    status = torch.full((B,), -1, dtype=torch.int32, device=db.device)
    c.workspace, c.workspace_bytes, c.track_status = work.data_ptr(), nbytes, status.data_ptr()
    st = db._stream(stream)
    binding.check(db.lib.ste_encounter_candidates_mask_f64(C.byref(s), C.byref(c), st), CALLS[0])
    at = 2 * (7 * NW * B + B * nwords)
    ints = work.view(torch.int32)
    count = ints[at + 2 * B: at + 3 * B]
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        P = int(ends[-1])
        out = dict(pairs=torch.empty((P, 2), dtype=torch.int32, device=db.device))
        if details:
            out.update(wfirst=torch.empty((P,), dtype=torch.int32, device=db.device), nwin=torch.empty((P,), dtype=torch.int32, device=db.device))
        if P:
            offsets = ends - count
            c.row_offset, c.npairs, c.pairs = offsets.data_ptr(), P, out["pairs"].data_ptr()
            if details:
                c.wfirst, c.nwin = out["wfirst"].data_ptr(), out["nwin"].data_ptr()
            binding.check(db.lib.ste_encounter_candidates_list_f64(C.byref(s), C.byref(c), st), CALLS[1])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["status"] = status.cpu().numpy()
    got["box"] = work[: 7 * NW * B].view(torch.float64).reshape(NW, 7, B).cpu().numpy()
    got["wlo"], got["whi"], got["count"] = (ints[at + k * B: at + (k + 1) * B].cpu().numpy() for k in range(3))
    assert int(work[-1]) == -1  # the word past the workspace
    return got


def _compare(got, ref, what, details=True):
    """The device against the restatement: status and window ranges exact; inside a track's range, emptiness exact, h bit for
    bit and corners within CORNER_ATOL; the list, wfirst and nwin equal (the restatement has no grazing pair-window)."""
    assert ref["ngrazing"] == 0, (what, "the case has a grazing pair-window", ref["ngrazing"])
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], ref["status"]), (what, "status", got["status"], ref["status"])
    assert np.array_equal(got["wlo"], ref["wlo"]) and np.array_equal(got["whi"], ref["whi"]), (what, "window ranges")
    NW, _, B = ref["box"].shape
    w = np.arange(NW)[:, None]
    live = (w >= ref["wlo"][None, :]) & (w <= ref["whi"][None, :])  # (NW, B): what the box kernel writes
    g, r = got["box"].transpose(0, 2, 1)[live], ref["box"].transpose(0, 2, 1)[live]  # (n, 7)
    assert np.array_equal(np.isinf(g), np.isinf(r)), (what, "emptiness")
    assert np.array_equal(g[:, 6].view(np.uint64), r[:, 6].view(np.uint64)), (what, "h")
    fin = np.isfinite(r)
    worst = float(np.abs(g[fin] - r[fin]).max()) if fin.any() else 0.0
    print(f"{what}: {int(live.sum())} boxes, corners deviate by at most {worst:.3g} (bound {cc.CORNER_ATOL:g}); "
          f"{len(ref['pairs'])} pairs of {ref['ntests']} pair-window tests")
    assert worst <= cc.CORNER_ATOL, (what, worst)
    assert got["pairs"].dtype == np.int32 and got["pairs"].shape == ref["pairs"].shape and np.array_equal(got["pairs"], ref["pairs"]), (what, "pairs")
    assert np.array_equal(got["count"], np.bincount(ref["pairs"][:, 0], minlength=B)), (what, "row counts")
    if details:
        assert np.array_equal(got["wfirst"], ref["wfirst"]) and np.array_equal(got["nwin"], ref["nwin"]), (what, "wfirst / nwin")


@pytest.mark.gpu
def test_hand_made_ships_on_the_device():
    """The seventeen hand-made ships through the C ABI: the answers worked out by hand, and boxes, ranges, status and lists
    against the restatement at W = 6 h, in one window, and with the margins (ship 16's is negative)."""
    h = cc.hand_batch()
    db, full = _batch(h)
    args = (cc.HAND_REACH, cc.HAND_W, 0.0)
    got = _abi_call(db, full, *args, cc.HAND_NW, h["t0"])
    cc.check_hand_answers(got, "device")
    _compare(got, _restated("hand", h, *args, cc.HAND_NW), "hand-made ships, W = 6 h")
    one = _abi_call(db, full, *args, 1, h["t0"])
    _compare(one, _restated("hand", h, *args, 1), "hand-made ships, one window")
    assert [0, 1] in one["pairs"].tolist() and [0, 1] not in got["pairs"].tolist()
    assert (got["pairs"][:, 0] < got["pairs"][:, 1]).all() and (one["pairs"][:, 0] < one["pairs"][:, 1]).all()
    m = _abi_call(db, full, *args, cc.HAND_NW, h["t0"], margin=h["margin"])
    _compare(m, _restated("hand", h, *args, cc.HAND_NW, margin=h["margin"]), "hand-made ships, margins")
    assert m["status"][16] == cc.BAD_MARGIN and not (m["pairs"] == 16).any()
    poisoned = h["states"].copy()
    for b, ns in enumerate(h["nsteps"]):
        poisoned[:, ns + 1:, :, b] = np.nan
    again = _abi_call(db, _dev(db, poisoned), *args, cc.HAND_NW, h["t0"])
    for k in ("pairs", "wfirst", "nwin", "status", "wlo", "whi"):
        assert np.array_equal(got[k], again[k]), (k, "rows past nsteps were read")


@pytest.mark.gpu
@pytest.mark.parametrize("B,NW", [(1, 1), (63, 2), (64, 65), (65, 1), (129, 2), (130, 65)])
def test_tile_and_word_edges(B, NW):
    """The meeting fleet's generator widened to B ships, NW windows over [0, 12) h (the last knots, up to 11.6 h, are inside;
    the ships without steps are EMPTY): B = 1, one tile short by a lane, full, over by a lane, two tiles and a lane, and two
    lanes; NW = 1, 2 and 65."""
    w = cc.wide_fleet(B)
    db, full = _batch(w)
    W = 12.0 / NW
    ref = _restated(("wide", B), w, 30.3, W, 0.0, NW)
    got = _abi_call(db, full, 30.3, W, 0.0, NW, w["t0"])
    _compare(got, ref, f"B = {B}, NW = {NW}")
    assert B < 63 or len(ref["pairs"]) > B


@pytest.mark.gpu
def test_full_rows_empty_rows_and_no_pairs():
    """66 ships of which 65 lie together: rows 0 .. 63 hold every later ship of the 65, rows 64 and 65 nothing (the tile's
    early way out, every lane having its answer, leaves nwin to the list kernel).  Three ships far apart at reach 0: P = 0,
    the front end returns a (0, 2) tensor and the list kernel is not asked."""
    d = cc.dense_batch()
    db, full = _batch(d)
    ref = _restated("dense", d, 30.0, 1.0, 0.0, 3)
    got = _abi_call(db, full, 30.0, 1.0, 0.0, 3, d["t0"])
    _compare(got, ref, "dense batch")
    assert got["count"].tolist() == [64 - i for i in range(64)] + [0, 0] and len(got["pairs"]) == 2080
    assert (got["nwin"] == 3).all() and (got["wfirst"] == 0).all()
    far = dict(states=d["states"][..., [0, 65, 1]].copy(), nsteps=d["nsteps"][:3], dt=d["dt"][:, :3], t0=d["t0"][:3])
    far["states"][0, :, 0, 2] += 90.0
    fdb, ffull = _batch(far)
    none = _abi_call(fdb, ffull, 0.0, 1.0, 0.0, 4, far["t0"])
    assert none["pairs"].shape == (0, 2) and none["count"].tolist() == [0, 0, 0] and not none["status"].any()
    out = fdb.encounter_candidates(0.0, 1.0, states=ffull, t0=far["t0"], details=True)
    assert tuple(out["pairs"].shape) == (0, 2) and out["pairs"].dtype == fdb.torch.int32 and tuple(out["wfirst"].shape) == (0,)
    assert (out["time0"], out["window_h"], out["nwindows"]) == (0.0, 1.0, 4)  # the last knot, at 3 h, opens window 3


@pytest.mark.gpu
def test_same_list_whatever_the_surroundings():
    """Bit-equal lists: the fleet window [3, 70) read in place and as a batch of its own against the whole fleet's pairs inside
    it, re-based; t0 NULL against zeros; nsteps NULL against full; details on and off; two calls in a row; a non-default
    stream; and the front ends: the method against the ABI, batch.encounter_candidates with window_h against the method and
    without it against batch.candidate_pairs."""
    import torch
    from track_estimators import batch

    w = cc.wide_fleet(130)
    db, full = _batch(w)
    B, reach, W, NW = 130, 30.3, 1.5, 8
    whole = _abi_call(db, full, reach, W, 0.0, NW, w["t0"])
    _compare(whole, _restated(("wide", 130), w, reach, W, 0.0, NW), "fleet of 130")
    again = _abi_call(db, full, reach, W, 0.0, NW, w["t0"])
    for k in ("pairs", "wfirst", "nwin", "status", "count"):
        assert np.array_equal(whole[k], again[k]), ("two calls in a row", k)
    assert np.array_equal(_abi_call(db, full, reach, W, 0.0, NW, w["t0"], details=False)["pairs"], whole["pairs"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert np.array_equal(_abi_call(db, full, reach, W, 0.0, NW, w["t0"], stream=side)["pairs"], whole["pairs"])
    # the method: explicit windows, then its own (the clock range of the fleet, found on the device)
    out = db.encounter_candidates(reach, W, states=full, t0=w["t0"], time0=0.0, nwindows=NW, details=True)
    for k in ("pairs", "wfirst", "nwin"):
        assert out[k].dtype == torch.int32 and np.array_equal(out[k].cpu().numpy(), whole[k]), ("method", k)
    assert np.array_equal(out["track_status"].cpu().numpy(), whole["status"])
    assert torch.equal(db.encounter_candidates(reach, W, states=full[0], t0=w["t0"], time0=0.0, nwindows=NW, stream=side), out["pairs"])
    auto = db.encounter_candidates(reach, W, states=full, t0=w["t0"], details=True)
    time0, nw = cc.clock_windows(w["nsteps"], w["dt"], w["t0"], W)
    assert (auto["time0"], auto["nwindows"]) == (time0, nw) and not (auto["track_status"].cpu().numpy() & cc.CLIPPED).any()
    assert np.array_equal(auto["pairs"].cpu().numpy(), _restated(("wide", 130), w, reach, W, time0, nw)["pairs"])
    # the window [3, 70): in place on the fleet's rows, and as a contiguous copy
    lo, hi = enc.FLEET_WINDOW
    inside = ((whole["pairs"] >= lo) & (whole["pairs"] < hi)).all(axis=1)
    assert inside.sum() > 100
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == B
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        got = win.encounter_candidates(reach, W, states=view, t0=w["t0"][lo:hi], time0=0.0, nwindows=NW, details=True)
        assert np.array_equal(got["pairs"].cpu().numpy(), whole["pairs"][inside] - lo), ("window", copied)
        assert np.array_equal(got["nwin"].cpu().numpy(), whole["nwin"][inside]) and np.array_equal(got["wfirst"].cpu().numpy(), whole["wfirst"][inside])
        assert np.array_equal(got["track_status"].cpu().numpy(), whole["status"][lo:hi])
    # t0 NULL against zeros, nsteps NULL against full
    zeros = _abi_call(db, full, reach, W, 0.0, NW, np.zeros(B))
    null = _abi_call(db, full, reach, W, 0.0, NW, None)
    for k in ("pairs", "wfirst", "nwin", "status", "wlo", "whi"):
        assert np.array_equal(zeros[k], null[k]), ("t0 NULL against zeros", k)
    assert np.array_equal(db.encounter_candidates(reach, W, states=full, time0=0.0, nwindows=NW).cpu().numpy(), null["pairs"])
    assert not np.array_equal(zeros["wlo"], whole["wlo"])
    fullsteps = dict(w, nsteps=np.full(B, enc.FLEET_N, dtype=np.int32))
    fdb, ffull = _batch(fullsteps)
    given = _abi_call(fdb, ffull, reach, W, 0.0, NW, w["t0"])
    from track_estimators._hip import binding
    s = binding.SteUkfBatchF64.from_buffer_copy(fdb.struct)
    s.nsteps = None
    absent = _abi_call(fdb, ffull, reach, W, 0.0, NW, w["t0"], batch_struct=s)
    for k in ("pairs", "wfirst", "nwin", "status", "wlo", "whi"):
        assert np.array_equal(given[k], absent[k]), ("nsteps NULL against full", k)
    assert len(given["pairs"]) > len(whole["pairs"])
    # the refusals of the front end
    with pytest.raises(ValueError, match="takes one state set"):
        db.encounter_candidates(reach, W, states=torch.cat([full, full]))
    with pytest.raises(ValueError, match="window_h must be finite and > 0"):
        db.encounter_candidates(reach, 0.0, states=full)
    with pytest.raises(ValueError, match="reach_km must be finite"):
        db.encounter_candidates(-1.0, W, states=full)
    with pytest.raises(ValueError, match=r"above STE_CANDIDATES_MAX_WINDOWS = 4096: window_h >= 0\.00234"):  # 9.616 h / 4095
        db.encounter_candidates(reach, 1e-3, states=full, t0=w["t0"])
    with pytest.raises(ValueError, match="track_margin_km must be None, a scalar or have shape"):
        db.encounter_candidates(reach, W, states=full, track_margin_km=np.zeros(3))
    with pytest.raises(ValueError, match="needs states, sm_mean or fwd_mean"):
        db.encounter_candidates(reach, W)


@pytest.mark.gpu
def test_through_the_front_ends_on_a_real_run():
    """A filtered and smoothed fleet of 40 synthetic ships in pairs of near copies: batch.encounter_candidates with window_h
    equals the method and without it is batch.candidate_pairs; encounter_metrics on the windowed list gives, for every pair it
    shares with the cap list, the same bits in all eight outputs, and the same set of pairs with nwithin > 0;
    position_spread_km feeds track_margin_km and the list with margins contains the one without; encounter_statistics runs on
    the list."""
    import dataclasses

    import torch
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(40, nobs=11, seed0=300)
    arrays = {f.name: getattr(sb, f.name).copy() for f in dataclasses.fields(sb)}
    for a in arrays.values():  # ship 2k + 1 is ship 2k again, a few km to the north
        a[1::2] = a[0::2]
    arrays["lat"][1::2] += 0.03
    arrays["z"][1::2, 1] += 0.03
    hb = batch.pack_uniform(synthetic.SyntheticBatch(**arrays), 2, H, Q, R, P0)
    db = batch.DeviceBatch(hb)
    db.run()
    B, radius, margin, W = hb.B, 30.0, 0.3, 4.0
    t0 = np.where(np.arange(B) % 4 < 2, 0.0, 0.5)
    method = db.encounter_candidates(radius + margin, W, t0=t0, details=True)
    front = batch.encounter_candidates(db, radius, margin, t0=t0, window_h=W)
    assert torch.equal(front, method["pairs"]) and front.dtype == torch.int32 and front.device == db.device
    cap = batch.encounter_candidates(db, radius, margin, t0=t0)
    nsteps, dt = db.t["nsteps"][:B], db.t["dt"][:, :B]
    assert torch.equal(cap, batch.candidate_pairs(db.sm_mean, nsteps, dt, radius, margin, t0))
    with pytest.raises(ValueError, match="give window_h as well"):
        batch.encounter_candidates(db, radius, margin, track_margin_km=1.0)
    sm = db.sm_mean.cpu().numpy()[None]
    time0, nw = method["time0"], method["nwindows"]
    ref = cc.candidates(sm[0], hb.nsteps, hb.dt, radius + margin, W, time0, nw, t0)
    assert ref["ngrazing"] == 0 and np.array_equal(method["pairs"].cpu().numpy(), ref["pairs"])
    assert np.array_equal(method["nwin"].cpu().numpy(), ref["nwin"]) and np.array_equal(method["wfirst"].cpu().numpy(), ref["wfirst"])
    wp, cp = method["pairs"].cpu().numpy(), cap.cpu().numpy()
    assert len(wp) >= 20 and all([2 * k, 2 * k + 1] in wp.tolist() for k in range(20))
    a = {k: v.cpu().numpy() for k, v in db.encounter_metrics(db.sm_mean, method["pairs"], radius, t0=t0).items()}
    b = {k: v.cpu().numpy() for k, v in db.encounter_metrics(db.sm_mean, cap, radius, t0=t0).items()}
    ka, kb = cc.pair_keys(wp, B), cc.pair_keys(cp, B)
    shared_a, shared_b = np.isin(ka, kb), np.isin(kb, ka)
    assert shared_a.sum() >= 20 and np.array_equal(ka[shared_a], kb[shared_b])
    for k in a:
        x, y = a[k][..., shared_a].astype(np.float64), b[k][..., shared_b].astype(np.float64)
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), k
    met_a, met_b = set(ka[a["nwithin"][0] > 0].tolist()), set(kb[b["nwithin"][0] > 0].tolist())
    assert met_a == met_b and len(met_a) >= 20
    spread = batch.position_spread_km(db)
    assert spread.shape == (B,) and spread.dtype == torch.float64 and spread.device == db.device
    sp = spread.cpu().numpy()
    cov = db.sm_cov.cpu().numpy()
    kd = cc.EARTH_KM * np.pi / 180.0
    worst = np.zeros(B)
    for t in range(B):
        for k in range(int(hb.nsteps[t]) + 1):
            kx = kd * np.cos(np.radians(sm[0, k, 1, t]))
            m = np.array([[cov[k, 0, t] * kx * kx, cov[k, 1, t] * kx * kd], [cov[k, 1, t] * kx * kd, cov[k, 4, t] * kd * kd]])
            worst[t] = max(worst[t], np.linalg.eigvalsh(m)[-1])
    assert db.packed_cov and np.allclose(sp, 3.0 * np.sqrt(worst), rtol=1e-9, atol=0.0) and (sp > 0.0).all()
    assert np.allclose(batch.position_spread_km(db, nsigma=1.0).cpu().numpy() * 3.0, sp, rtol=1e-14)
    wide = db.encounter_candidates(radius + margin, W, t0=t0, track_margin_km=spread, time0=time0, nwindows=nw)
    assert np.isin(ka, cc.pair_keys(wide.cpu().numpy(), B)).all() and len(wide) >= len(wp)
    assert torch.equal(wide, batch.encounter_candidates(db, radius, margin, t0=t0, window_h=W, track_margin_km=spread))
    stats = batch.encounter_statistics(db, wide, radius, 4, seed=2, chunk=4, t0=t0)
    assert stats["encounter_prob"].shape == (len(wide),) and not stats["status"].any()
    assert (stats["encounter_prob"][np.isin(cc.pair_keys(wide.cpu().numpy(), B), list(met_a))] > 0.0).any()


@pytest.mark.gpu
def test_refusals_before_any_launch():
    """The refusals on the device build: nothing is launched, and the status array of a refused call is untouched."""
    from track_estimators._hip import binding

    _abi_refusals()
    h = cc.hand_batch()
    db, full = _batch(h)
    torch = db.torch
    status = torch.full((cc.HAND_B,), -7, dtype=torch.int32, device=db.device)
    work = torch.zeros((db.lib.ste_encounter_candidates_workspace(cc.HAND_B, 4) // 8 + 1,), dtype=torch.int64, device=db.device)
    c = binding.SteCandidatesF64()
    c.states, c.reach_km, c.time0, c.window_h, c.nwindows = full.data_ptr(), 30.0, 0.0, -1.0, 4
    c.workspace, c.workspace_bytes, c.track_status = work.data_ptr(), 8 * work.numel(), status.data_ptr()
    assert db.lib.ste_encounter_candidates_mask_f64(C.byref(db.struct), C.byref(c), db._stream(None)) == -1
    torch.cuda.synchronize()
    assert (status == -7).all() and not work.any()
