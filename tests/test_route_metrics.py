"""Pairs of tracks on the device as curves (include/ste.h: ste_route_f64, ste_route_metrics_f64; DESIGN.md, "Routes"):
declaration and layout of the C ABI, the refusals of the call, the NumPy restatement against a brute force over every monotone
coupling and against hand answers, the near ties of the edge fleet, and the pruning of route_candidates (CPU); on the GPU the
hand-made curves for both leg functions, the edge fleet against the restatement with and without band and reversal, one pair
that leaves the LDS, independence of the surroundings bit for bit, the Python front ends on a real run, and the refusals on
the device build."""
import ctypes as C
import os
import re

import numpy as np
import path_metrics_cases as pmc
import pytest
import route_cases as rc
from conftest import ROOT

FIELDS = ["nstates", "model", "states", "npairs", "pairs", "band", "flags", "work", "work_bytes", "frechet", "frechet_at", "dtw",
          "dtw_len", "status"]
OUTPUTS = FIELDS[9:]
INT32 = ("frechet_at", "dtw_len", "status")
MAX_TIE_SHARE = 0.02
WITHIN_KM = 20.0  # route_candidates: twice the spacing of the edge fleet's longer ships


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bits(a):
    return _u64(np.asarray(a).astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_struct_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    proto = r"int ste_route_metrics_f64\(const ste_ukf_batch_f64\* b, const ste_route_f64\* ro, void\* stream\);"
    assert re.search("^" + proto, hdr, flags=re.M)
    assert re.search(r"^size_t ste_route_workspace\(int32_t Nmax, int32_t nstates, int64_t npairs\);", hdr, flags=re.M)
    assert re.search(r"^int ste_route_lds_cols\(void\);", hdr, flags=re.M)
    body = hdr[hdr.index("typedef struct ste_route_f64 {"): hdr.index("} ste_route_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteRouteF64._fields_] == FIELDS
    # the layout of the C struct by hand: nstates and model share a word, band and flags one, every other field takes one
    offsets = {"nstates": 0, "model": 4, "states": 8, "npairs": 16, "pairs": 24, "band": 32, "flags": 36, "work": 40, "work_bytes": 48}
    offsets.update({name: 56 + 8 * k for k, name in enumerate(OUTPUTS)})
    assert {f: getattr(binding.SteRouteF64, f).offset for f in FIELDS} == offsets
    assert C.sizeof(binding.SteRouteF64) == 96 and re.search(r"} ste_route_f64;\s*/\* 96 bytes \*/", hdr)
    for name in ("ste_route_metrics_f64", "ste_route_workspace", "ste_route_lds_cols"):
        assert name in binding.SYMBOLS
    lib = binding.load()
    assert hasattr(lib, "ste_route_metrics_f64") and 64 <= lib.ste_route_lds_cols() <= 2048
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert "(ste_route_metrics_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert "pairs of tracks on the device as curves" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the route arguments travel beside the batch
    assert re.search(r"#define STE_ROUTE_MAX_PAIRS \(1 << 26\)", hdr) and binding.STE_ROUTE_MAX_PAIRS == 1 << 26
    assert int(re.search(r"#define STE_ROUTE_REVERSE_J 0x(\d+)u", hdr).group(1), 16) == binding.STE_ROUTE_REVERSE_J == 1
    for name, value in (("BAD_INDEX", rc.BAD_INDEX), ("NO_PATH", rc.NO_PATH), ("NOT_FINITE", rc.NOT_FINITE)):
        assert int(re.search(r"#define STE_ROUTE_%s\s+0x(\d+)" % name, hdr).group(1), 16) == getattr(binding, "STE_ROUTE_" + name) == value
    assert (rc.BAD_INDEX, rc.NO_PATH, rc.NOT_FINITE) == (1, 2, 4)
    comment = hdr[hdr.index("ROUTES:"): hdr.index("#define STE_ROUTE_MAX_PAIRS")]
    for word in ("Curves.", "Point.", "Cell.", "Cost (DTW only).", "Band.", "Predecessor", "Frechet table.", "DTW tables.", "Bits.",
                 "Outputs", "Status.", "Work.", "ADMISSIBLE", "STE_ROUTE_REVERSE_J", "STE_ROUTE_NOT_FINITE", "STE_ROUTE_BAD_INDEX",
                 "STE_ROUTE_NO_PATH", "strictly smaller", "without contraction", "squared chord", "asin(h)", "row-major recurrence",
                 "(-1, -1)", "ste_route_lds_cols()", "Refused with STE_EINVAL"):
        assert word in comment, word


def _abi_refusals():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name in the message; a launch that failed would
    return STE_ELAUNCH (-2).  The pointers below are not memory: nothing may be launched, with a GPU or without one."""
    from track_estimators._hip import binding

    lib = binding.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    lds = lib.ste_route_lds_cols()

    def good_batch():
        s = binding.SteUkfBatchF64()
        s.B, s.Nmax, s.n = 8, 12, 4
        s.nsteps = 0x2000  # no dt: the call needs none
        return s

    def good_route():
        e = binding.SteRouteF64()
        e.nstates, e.model, e.states, e.npairs, e.pairs = 3, binding.STE_PREP_WGS84, 0x3000, 5, 0x4000
        e.band, e.flags, e.work, e.work_bytes = 2, binding.STE_ROUTE_REVERSE_J, None, 0
        for k, name in enumerate(OUTPUTS):
            setattr(e, name, 0x6000 + 0x1000 * k)
        return e

    def refused(reason, **fields):
        s, e = good_batch(), good_route()
        for name, value in fields.items():
            setattr(s if hasattr(s, name) and not hasattr(e, name) else e, name, value)
        rc_ = lib.ste_route_metrics_f64(ref(s), ref(e), None)
        msg = lib.ste_last_error().decode()
        assert rc_ == -1 and reason in msg and "ste_route_metrics_f64" in msg, (fields, rc_, msg)

    for s, e, reason in ((None, good_route(), "batch pointer is NULL"), (good_batch(), None, "route arguments (ro) are NULL")):
        assert lib.ste_route_metrics_f64(ref(s), ref(e), None) == -1
        msg = lib.ste_last_error().decode()
        assert reason in msg and "ste_route_metrics_f64" in msg
    refused("ro->states is required", states=None)
    refused("ro->pairs is required", pairs=None)
    for n in (0, -3):
        refused("nstates must be >= 1", nstates=n)
    refused("limited to 65535", nstates=65536)
    for n in (0, -1, (1 << 26) + 1, 1 << 40):
        refused("between 1 and STE_ROUTE_MAX_PAIRS", npairs=n)
    for m in (-1, 2, 7):
        refused("STE_PREP_SPHERE or STE_PREP_WGS84 when frechet is asked for", model=m)
    for b in (-1, -(2 ** 31)):
        refused("band must be >= 0", band=b)
    for f in (2, 3, 0x80000000):
        refused("flags must be 0 or STE_ROUTE_REVERSE_J", flags=f)
    refused("no output asked for", **{name: None for name in OUTPUTS})
    need = lib.ste_route_workspace(lds + 5, 3, 5)
    assert need > 0
    refused("ro->work is required", Nmax=lds + 5)
    refused("ro->work is required", Nmax=lds + 5, work=0x9000, work_bytes=need - 1)
    refused("ro->work is required", Nmax=lds + 5, work=None, work_bytes=need)
    for b in (0, -4):
        refused("B must be > 0", B=b)
    refused("Nmax >= 0", Nmax=-1)
    refused("Nmax is limited", Nmax=2 ** 31 - 1)
    refused("track_stride", track_stride=7)
    # the scratch: 0 while the columns fit the LDS, monotone in each argument
    ws = lib.ste_route_workspace
    assert ws(lds - 1, 16, 1000) == 0 and ws(lds, 1, 1) > 0 and ws(-1, 1, 1) == 0 and ws(lds, 0, 1) == 0 and ws(lds, 1, 0) == 0
    sizes = [lds - 2, lds - 1, lds, lds + 1, 2 * lds, 100 * lds]
    counts = [1, 2, 7, 100, 5000, 65535]
    npairs = [1, 3, 100, 4000, 1 << 20, 1 << 26]
    for n in sizes:
        for k in counts:
            vals = [ws(n, k, p) for p in npairs]
            assert vals == sorted(vals), ("npairs", n, k, vals)
    for n in sizes:
        for p in npairs:
            vals = [ws(n, k, p) for k in counts]
            assert vals == sorted(vals), ("nstates", n, p, vals)
    for k in counts:
        for p in npairs:
            vals = [ws(n, k, p) for n in sizes]
            assert vals == sorted(vals), ("Nmax", k, p, vals)


def test_abi_refusals_without_a_gpu():
    _abi_refusals()


def test_restatement_against_every_monotone_coupling():
    """All n, m <= 5 on random points, without a band and with band 1 and 2: F and D of the restatement are those of the best
    of the couplings taken one by one, bit for bit (min and max do not round, and a coupling's sum is taken in the order of the
    recurrence); `at` is the one cell whose q is F and L the length of the one cheapest coupling, where they are unique."""
    rng = np.random.default_rng(5)
    checked = {"F": 0, "at": 0, "L": 0, "no_path": 0}
    for n in range(1, 6):
        for m in range(1, 6):
            for band in (0, 1, 2):
                for rep in range(3):
                    ci = np.array([30.0, 40.0]) + rng.normal(0.0, 0.5, (n, 2))
                    cj = np.array([30.0, 40.0]) + rng.normal(0.0, 0.5, (m, 2))
                    states = np.full((1, 5, 4, 2), np.nan)
                    states[0, :n, :2, 0], states[0, :m, :2, 1] = ci, cj
                    got = rc.route_metrics(states, [n - 1, m - 1], [(0, 1)], band)
                    if band > 0 and abs(n - m) > band:
                        assert got["status"][0, 0] == rc.NO_PATH and not rc.couplings(n, m, band)
                        checked["no_path"] += 1
                        continue
                    bf = rc.brute_force(ci, cj, band)
                    assert got["status"][0, 0] == 0
                    assert _u64(got["F"][0, 0]) == _u64(np.float64(bf["F"])), (n, m, band)
                    assert _u64(got["dtw"][0, 0]) == _u64(np.float64(bf["D"])), (n, m, band)
                    checked["F"] += 1
                    if bf["at"] is not None:
                        assert tuple(got["frechet_at"][0, 0]) == bf["at"], (n, m, band)
                        checked["at"] += 1
                    if bf["L"] is not None:
                        assert got["dtw_len"][0, 0] == bf["L"], (n, m, band)
                        checked["L"] += 1
                    want = pmc.leg_km("sphere", *ci[got["frechet_at"][0, 0, 0]], *cj[got["frechet_at"][0, 0, 1]])
                    assert got["frechet"][0, 0] == want
    print("brute force:", checked)
    assert checked["F"] > 150 and checked["at"] > 150 and checked["L"] > 150 and checked["no_path"] > 20
    # the couplings themselves: Delannoy numbers, and a band that leaves the diagonal alone
    assert [len(rc.couplings(k, k)) for k in (1, 2, 3, 4, 5)] == [1, 3, 13, 63, 321]
    assert len(rc.couplings(4, 4, 3)) == 63 and len(rc.couplings(3, 5, 1)) == 0 and len(rc.couplings(1, 4)) == 1


def _hand_restated(model="sphere"):
    h = rc.hand_batch()
    return [rc.route_metrics(h["states"], h["nsteps"], h["pairs"], band, reverse, model)
            for band, reverse in ((0, False), (0, True), (2, False))]


def test_restatement_against_hand_answers():
    """Identical tracks and a track against itself give 0, dtw 0 and as many cells as points; a track against its reverse with
    the flag gives 0; two parallels a degree apart give one degree of meridian; a single point against six gives the largest
    distance, the sum and six cells; a detour's Frechet distance exceeds both directed Hausdorff distances tenfold; a NaN row,
    indices outside the batch and lengths further apart than the band give NaN, (-1, -1) and 0 with their status bit."""
    for model in ("sphere", "wgs84"):
        rc.check_hand_answers(*_hand_restated(model), f"restatement, {model}", model)


def test_a_narrower_band_never_lowers_the_tables():
    w = rc.fleet()
    keep = np.abs(w["nsteps"][w["pairs"][:, 0]].astype(int) - w["nsteps"][w["pairs"][:, 1]]) <= 3
    pairs = w["pairs"][keep][:40]
    assert len(pairs) >= 30
    last = None
    for band in (0, 100, 40, 12, 3):
        res = rc.route_metrics(w["states"][:1], w["nsteps"], pairs, band, leg=False)
        assert not res["status"].any()
        if last is not None:
            assert (res["F"] >= last["F"]).all() and (res["dtw"] >= last["dtw"]).all(), band
        last = res
    wide = rc.route_metrics(w["states"][:1], w["nsteps"], pairs, 0, leg=False)
    assert (last["dtw"] > wide["dtw"]).any()  # the band bites


def test_near_ties_of_the_edge_fleet():
    """The share of (sample, pair) whose frechet_at or dtw_len changes when every q and cost is scaled by 1 +- 1e-13 is a
    condition of the device comparison: at most 2 % (on this fleet the restatement leaves out none)."""
    w = rc.fleet()
    assert w["states"].shape == (rc.FLEET_S, rc.FLEET_N + 1, 4, rc.FLEET_B) and w["pairs"].shape == (rc.FLEET_P, 2)
    assert sorted(set(w["nsteps"].tolist())) == list(rc.FLEET_NSTEPS)
    assert ((w["pairs"] // len(rc.FLEET_NSTEPS))[:, 0] == (w["pairs"] // len(rc.FLEET_NSTEPS))[:, 1]).all()
    for band, reverse in ((0, False), (rc.FLEET_BAND, True)):
        ref = rc.fleet_reference(band, reverse)
        share = (ref["at_tie"] | ref["len_tie"]).mean()
        print(f"band {band}, reverse {reverse}: near ties {int((ref['at_tie'] | ref['len_tie']).sum())} of {ref['at_tie'].size}; "
              f"status counts {np.bincount(ref['status'].ravel()).tolist()}")
        assert share <= MAX_TIE_SHARE, (band, reverse, share)
        assert (ref["status"] == 0).sum() > 0.4 * ref["status"].size
        if band:
            assert (ref["status"] == rc.NO_PATH).any()
        else:
            assert not ref["status"].any()


def test_route_candidates_prune_nothing_that_is_within():
    """route_endpoint_pairs on CPU tensors: no pair (i < j) whose restated Frechet distance is <= within_km is pruned, with and
    without the reverse flag, and something is pruned."""
    import torch
    from track_estimators import batch

    w = rc.fleet()
    B = rc.FLEET_B
    mean = np.nan_to_num(w["states"][0])
    ij = np.array([(i, j) for i in range(B) for j in range(i + 1, B) if i // 12 == j // 12 or (i + j) % 7 == 0], dtype=np.int32)
    backwards = mean.copy()  # the odd ships stored from their last row to their first
    for t in range(1, B, 2):
        backwards[:w["nsteps"][t] + 1, :, t] = mean[w["nsteps"][t]::-1, :, t]
    for reverse, within in ((False, WITHIN_KM), (True, WITHIN_KM)):
        if reverse:
            mean = backwards
            ij = ij[(ij[:, 0] % 2 == 0) & (ij[:, 1] % 2 == 1)]
        ref = rc.route_metrics(mean[None], w["nsteps"], ij, 0, reverse)
        close = {tuple(p) for p in ij[ref["frechet"][0] <= within].tolist()}
        cand = batch.route_endpoint_pairs(torch.from_numpy(mean), torch.from_numpy(w["nsteps"]), within, reverse=reverse)
        assert cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[1] == 2
        c = [tuple(p) for p in cand.numpy().tolist()]
        assert c == sorted(c) and all(i < j for i, j in c)
        assert close <= set(c), (reverse, sorted(close - set(c))[:5])
        print(f"reverse {reverse}: {len(close)} of {len(ij)} restated pairs within {within} km, {len(c)} candidates of {B * (B - 1) // 2}")
        assert len(close) >= 3 and len(c) < B * (B - 1) // 2 // 4, (reverse, len(close), len(c))
        assert torch.equal(cand, batch.route_endpoint_pairs(torch.from_numpy(mean), torch.from_numpy(w["nsteps"]), within,
                                                            reverse=reverse, chunk=7))
        wider = batch.route_endpoint_pairs(torch.from_numpy(mean), torch.from_numpy(w["nsteps"]), within, margin_km=50.0, reverse=reverse)
        assert set(c) <= {tuple(p) for p in wider.numpy().tolist()} and len(wider) >= len(c)
    poisoned = np.nan_to_num(w["states"][0])
    poisoned[0, 1, 3] = np.nan
    cand = batch.route_endpoint_pairs(torch.from_numpy(poisoned), torch.from_numpy(w["nsteps"]), 1e5).numpy()
    assert len(cand) == (B - 1) * (B - 2) // 2 and not (cand == 3).any()


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
def _dev(db, a):
    return db.torch.from_numpy(np.ascontiguousarray(a)).to(db.device)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _abi_call(db, states, pairs, band=0, reverse=False, model="sphere", want=OUTPUTS, work_factor=1):
    """ste_route_metrics_f64 through ctypes on a contiguous (S, N+1, 4, B) device tensor; ``want``: the outputs asked for (the
    others are NULL); ``work_factor``: the scratch is that many times what ste_route_workspace asks for.  -> NumPy arrays."""
    from track_estimators._hip import binding

    torch = db.torch
    S, P = int(states.shape[0]), len(pairs)
    pr = _dev(db, np.asarray(pairs, dtype=np.int32))
    ro = binding.SteRouteF64()
    ro.nstates, ro.model, ro.states = S, {"sphere": binding.STE_PREP_SPHERE, "wgs84": binding.STE_PREP_WGS84}[model], states.data_ptr()
    ro.npairs, ro.pairs, ro.band, ro.flags = P, pr.data_ptr(), band, binding.STE_ROUTE_REVERSE_J if reverse else 0
    need = int(db.lib.ste_route_workspace(int(db.struct.Nmax), S, P)) * work_factor
    work = torch.full((max(need, 8) // 8,), float("nan"), dtype=torch.float64, device=db.device)
    ro.work, ro.work_bytes = work.data_ptr(), need
    out = {}
    for k in want:
        shape = (S, P, 2) if k == "frechet_at" else (S, P)
        out[k] = torch.empty(shape, dtype=torch.int32 if k in INT32 else torch.float64, device=db.device)
        setattr(ro, k, out[k].data_ptr())
    binding.check(db.lib.ste_route_metrics_f64(C.byref(db.struct), C.byref(ro), db._stream(None)), "ste_route_metrics_f64")
    torch.cuda.synchronize()
    return _host(out)


def _compare(got, ref, what, at_tie=None, len_tie=None, values_only=False):
    """The device against the restatement: status equal, NaN patterns identical, frechet within pmc.DIST_RTOL / DIST_ATOL and
    frechet_at equal outside the near ties of `at`, dtw within pmc.DIST_RTOL plus 1e-9 km per cell of the path, dtw_len equal
    outside the near ties of the length.  ``values_only``: for curves made of exact ties (equal points, parallels), whose
    frechet_at and dtw_len the hand answers cover: status, frechet and dtw alone.  Returns the largest deviations as fractions
    of their tolerances."""
    shape = ref["status"].shape
    at_tie = np.zeros(shape, dtype=bool) if at_tie is None else at_tie
    len_tie = np.zeros(shape, dtype=bool) if len_tie is None else len_tie
    if values_only:
        at_tie, len_tie = np.zeros(shape, dtype=bool), np.ones(shape, dtype=bool)
    assert values_only or (at_tie | len_tie).mean() <= MAX_TIE_SHARE, (what, "near ties", float((at_tie | len_tie).mean()))
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], ref["status"]), (what, "status")
    good = ref["status"] == 0
    assert got["frechet_at"].dtype == np.int32 and got["frechet_at"].shape == shape + (2,)
    same_at = (got["frechet_at"] == ref["frechet_at"]).all(axis=-1)
    assert values_only or same_at[~at_tie].all(), (what, "frechet_at", np.argwhere(~same_at & ~at_tie)[:5].tolist())
    assert (got["frechet_at"][~good] == -1).all() and np.isnan(got["frechet"][~good]).all()
    use = good if values_only else good & same_at
    err = np.abs(got["frechet"] - ref["frechet"])
    tol = pmc.DIST_ATOL + pmc.DIST_RTOL * np.abs(ref["frechet"])
    worst = {"frechet": float((err[use] / tol[use]).max()) if use.any() else 0.0}
    print(f"{what}: frechet deviates by at most {worst['frechet']:.3g} of its tolerance ({int(use.sum())} values, "
          f"{int((~same_at).sum())} other cells on near ties)")
    assert not np.isnan(got["frechet"][good]).any() and worst["frechet"] <= 1.0, (what, "frechet", worst)
    if "dtw" in got:
        assert got["dtw_len"].dtype == np.int32
        assert np.array_equal(got["dtw_len"][~len_tie], ref["dtw_len"][~len_tie]), (what, "dtw_len")
        assert (got["dtw_len"][~good] == 0).all() and np.isnan(got["dtw"][~good]).all() and not np.isnan(got["dtw"][good]).any()
        err = np.abs(got["dtw"] - ref["dtw"])
        tol = pmc.DIST_RTOL * np.abs(ref["dtw"]) + rc.DTW_ATOL_PER_CELL * ref["dtw_len"]
        # a pair against itself: every cost on the diagonal is exactly 0 on either side, and tol is 0 there only if len were 0
        worst["dtw"] = float((err[good] / tol[good]).max()) if good.any() else 0.0
        worst["dtw_km_per_cell"] = float((err[good] / ref["dtw_len"][good]).max()) if good.any() else 0.0
        print(f"{what}: dtw deviates by at most {worst['dtw']:.3g} of its tolerance, {worst['dtw_km_per_cell']:.3g} km per cell")
        assert worst["dtw"] <= 1.0, (what, "dtw", worst)
    return worst


def _hand_db():
    from track_estimators import batch

    h = rc.hand_batch()
    db = batch.DeviceBatch(pmc.bare_batch(h["nsteps"], h["dt"]), histories=False)
    return h, db, _dev(db, h["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sphere", "wgs84"])
def test_hand_made_curves_on_the_device(model):
    """The hand-made curves through DeviceBatch.route_metrics: the known answers, and the restatement, for either model."""
    h, db, full = _hand_db()
    got = [_host(db.route_metrics(full, h["pairs"], dtw=True, band=band, reverse=reverse, model=model))
           for band, reverse in ((0, False), (0, True), (2, False))]
    rc.check_hand_answers(*got, f"device, {model}", model)
    for g, r, name in zip(got, _hand_restated(model), ("plain", "reversed", "band 2")):
        assert set(g) == set(OUTPUTS)
        # the hand curves are full of exact ties (equal points, parallels), which a last bit of cos decides: the values
        _compare(g, r, f"hand-made curves, {name}, {model}", values_only=True)


def _fleet_db():
    from track_estimators import batch

    w = rc.fleet()
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    return w, db, _dev(db, w["states"])


@pytest.mark.gpu
@pytest.mark.parametrize("band,reverse", [(0, False), (0, True), (rc.FLEET_BAND, False), (rc.FLEET_BAND, True)])
def test_edge_fleet_against_the_restatement(band, reverse):
    """Nmax = 130, S = 3, 48 ships of the lengths 0, 1, 2, 62 .. 66, 127 .. 130 on four base routes, 160 pairs, with and
    without the band of 70 and the reverse flag, on the sphere; the run without either also on WGS84.  frechet within 1e-10
    relative, dtw within 1e-10 relative plus 1e-9 km per cell, frechet_at and dtw_len equal outside the near ties, status
    equal; a band never lowers dtw.  Measured on an MI355X: no (sample, pair) is a near tie and frechet_at, dtw_len and status
    are equal in all 480 of every run; as fractions of their tolerances frechet deviates by at most 4.8e-6 on the sphere and
    9.0e-4 on WGS84, dtw by at most 8.0e-5 (4.2e-13 km per cell of the path)."""
    w, db, full = _fleet_db()
    ref = rc.fleet_reference(band, reverse)
    got = _host(db.route_metrics(full, w["pairs"], dtw=True, band=band, reverse=reverse))
    assert got["frechet"].shape == (rc.FLEET_S, rc.FLEET_P) and got["frechet_at"].shape == (rc.FLEET_S, rc.FLEET_P, 2)
    _compare(got, ref, f"edge fleet, band {band}, reverse {reverse}", ref["at_tie"], ref["len_tie"])
    if band:
        free = _host(db.route_metrics(full, w["pairs"], dtw=True, reverse=reverse))
        good = got["status"] == 0
        assert (got["dtw"][good] >= free["dtw"][good]).all()
        assert (got["frechet"][good] >= free["frechet"][good] * (1.0 - pmc.DIST_RTOL) - pmc.DIST_ATOL).all()
    elif not reverse:
        wgs = _host(db.route_metrics(full, w["pairs"], dtw=True, model="wgs84"))
        rw = rc.fleet_reference(band, reverse, "wgs84")
        worst = _compare(wgs, rw, "edge fleet, wgs84", ref["at_tie"], ref["len_tie"])
        for k in ("frechet_at", "dtw", "dtw_len", "status"):
            assert np.array_equal(_bits(wgs[k]), _bits(got[k])), ("the model touches frechet alone", k)
        assert worst["frechet"] <= 1.0


@pytest.mark.gpu
def test_one_long_pair_leaves_the_lds():
    """ns_i = ns_j + 3 = ste_route_lds_cols() + 70, band 96, S = 1: the boundary row goes through `work`.  Against the
    restatement, and with `work` twice the required size the same bits."""
    from track_estimators import batch
    from track_estimators._hip import binding

    lds = binding.load().ste_route_lds_cols()
    w = rc.long_pair(lds)
    assert w["nsteps"].tolist() == [lds + 70, lds + 67]
    db = batch.DeviceBatch(pmc.bare_batch(w["nsteps"], w["dt"]), histories=False)
    assert db.lib.ste_route_workspace(int(db.struct.Nmax), 1, 1) > 0
    full = _dev(db, w["states"])
    ref = rc.route_metrics(w["states"], w["nsteps"], w["pairs"], 96)
    at_tie, len_tie = rc.near_ties(w["states"], w["nsteps"], w["pairs"], 96, ref=ref)
    got = _host(db.route_metrics(full, w["pairs"], dtw=True, band=96))
    assert not ref["status"].any() and ref["dtw_len"][0, 0] >= lds + 71
    if not (at_tie | len_tie).any():
        _compare(got, ref, "long pair, band 96")
    else:  # a single pair: a near tie leaves the value comparisons that do not depend on it
        assert np.array_equal(got["status"], ref["status"])
        assert abs(got["dtw"][0, 0] - ref["dtw"][0, 0]) <= pmc.DIST_RTOL * ref["dtw"][0, 0] + rc.DTW_ATOL_PER_CELL * ref["dtw_len"][0, 0]
    once = _abi_call(db, full, w["pairs"], band=96)
    twice = _abi_call(db, full, w["pairs"], band=96, work_factor=2)
    for k in OUTPUTS:
        assert np.array_equal(_bits(once[k]), _bits(got[k])) and np.array_equal(_bits(twice[k]), _bits(got[k])), k
    # the swapped pair sweeps ns_j + 1 > lds columns too, with the other track along the lanes
    swapped = _host(db.route_metrics(full, w["pairs"][:, ::-1].copy(), dtw=True, band=96))
    assert np.array_equal(_bits(swapped["dtw"]), _bits(got["dtw"]))


def _same_bits(a, b, what, cols_a=slice(None), cols_b=slice(None), keys=OUTPUTS):
    for k in keys:
        x, y = (a[k][:, cols_a], b[k][:, cols_b])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), (what, k)


@pytest.mark.gpu
def test_same_bits_whatever_the_surroundings():
    """Bit for bit: the pair list permuted; S = 1 slices against S = 3; the window [5, 41) with re-based indices and
    track_stride > B, in place on the fleet's rows and as a contiguous copy; every output alone and frechet without dtw; one
    pair alone; the swapped pair (j, i): dtw always, frechet wherever frechet_at is the transposed cell."""
    w, db, full = _fleet_db()
    pairs, P = w["pairs"], rc.FLEET_P
    kw = dict(dtw=True, band=rc.FLEET_BAND)
    whole = _host(db.route_metrics(full, pairs, **kw))
    for name, perm in (("reversed", np.arange(P)[::-1]), ("shuffled", np.random.default_rng(3).permutation(P))):
        _same_bits(_host(db.route_metrics(full, pairs[perm], **kw)), whole, name, cols_b=perm)
    for s in range(rc.FLEET_S):
        one = _host(db.route_metrics(full[s], pairs, **kw))
        _same_bits(one, {k: v[s:s + 1] for k, v in whole.items()}, f"sample {s} alone")
    for want in [(k,) for k in OUTPUTS] + [("frechet", "frechet_at", "status"), ("dtw", "status")]:
        _same_bits(_abi_call(db, full, pairs, band=rc.FLEET_BAND, want=want), whole, f"outputs {want}", keys=want)
    nodtw = _host(db.route_metrics(full, pairs, band=rc.FLEET_BAND))
    assert set(nodtw) == {"frechet", "frechet_at", "status"}
    _same_bits(nodtw, whole, "frechet without dtw", keys=tuple(nodtw))
    lo, hi = rc.FLEET_WINDOW
    inside = ((pairs >= lo) & (pairs < hi)).all(axis=1)
    assert inside.sum() > 60
    win = db.window(lo, hi)
    assert int(win.struct.track_stride) == rc.FLEET_B > hi - lo
    for copied in (False, True):
        view = full[..., lo:hi].contiguous() if copied else full[..., lo:hi]
        _same_bits(_host(win.route_metrics(view, pairs[inside] - lo, **kw)), whole, f"window, copied={copied}", cols_b=inside)
    k = int(np.argmax(whole["status"][0] == 0))
    _same_bits(_host(db.route_metrics(full, pairs[k:k + 1], **kw)), whole, "one pair alone", cols_b=slice(k, k + 1))
    # the swapped pair
    for band in (0, rc.FLEET_BAND):
        fwd = whole if band else _host(db.route_metrics(full, pairs, dtw=True))
        swp = _host(db.route_metrics(full, pairs[:, ::-1].copy(), dtw=True, band=band))
        assert np.array_equal(fwd["status"], swp["status"])
        assert np.array_equal(_bits(fwd["dtw"]), _bits(swp["dtw"])), band
        transposed = (fwd["frechet_at"] == swp["frechet_at"][..., ::-1]).all(axis=-1)
        ref = rc.fleet_reference(band, False)
        assert transposed[~ref["at_tie"]].all(), band
        assert np.array_equal(_bits(fwd["frechet"][transposed]), _bits(swp["frechet"][transposed])), band
    with pytest.raises(ValueError, match=r"pairs must have shape \(P, 2\)"):
        db.route_metrics(full, pairs.T)
    with pytest.raises(ValueError, match="integer array or tensor"):
        db.route_metrics(full, pairs.astype(np.float64))
    with pytest.raises(ValueError, match="band must be >= 0"):
        db.route_metrics(full, pairs, band=-1)
    with pytest.raises(ValueError, match="model must be one of"):
        db.route_metrics(full, pairs, model="plane")
    with pytest.raises(ValueError, match="states must be a float64 tensor of shape"):
        db.route_metrics(full[:, :, :3], pairs)


def _real_batch():
    """Four synthetic tracks of 20 steps through the filter and the smoother: track 1 is a copy of track 0, track 2 is track 0
    moved 60 degrees east, track 3 is another ship and short."""
    import dataclasses

    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    sb = synthetic.make_batch(4, nobs=11, seed0=100)
    arrays = {f.name: getattr(sb, f.name).copy() for f in dataclasses.fields(sb)}
    for a in arrays.values():
        a[1] = a[0]
        a[2] = a[0]
    arrays["lon"][2] += 60.0
    arrays["z"][2, 0] += 60.0
    hb = batch.pack_uniform(synthetic.SyntheticBatch(**arrays), 2, H, Q, R, P0)
    assert hb.Nmax == 20
    hb = dataclasses.replace(hb, nsteps=np.array([20, 20, 20, 13], dtype=np.int32))
    db = batch.DeviceBatch(hb)
    db.run()
    return hb, db


@pytest.mark.gpu
def test_through_the_sampler_and_the_front_ends():
    """route_metrics on sm_mean and on the sampler's output of a real run against the restatement; route_statistics:
    frechet_smoothed is route_metrics on sm_mean bit for bit, prob_within lies in [0, 1], grows with within_km and with one
    chunk is sample_smoothed + route_metrics; two copies of one track follow one route with probability 1 at any distance the
    posterior allows and ships 60 degrees apart with probability 0; curve_distance of a smoothed track against itself is 0 and
    equals route_metrics on the same rows; route_candidates keeps the copies and drops the far ship."""
    from track_estimators import batch

    hb, db = _real_batch()
    pairs = np.array([(0, 1), (0, 2), (0, 3), (3, 1), (2, 2)], dtype=np.int32)
    sm = db.sm_mean.cpu().numpy()[None]
    got = _host(db.route_metrics(db.sm_mean, pairs, dtw=True))
    ref = rc.route_metrics(sm, hb.nsteps, pairs)
    _compare(got, ref, "smoothed tracks", *rc.near_ties(sm, hb.nsteps, pairs, ref=ref))
    assert got["frechet"][0, 0] < 1e-6 and got["frechet"][0, 4] == 0.0 and got["frechet"][0, 1] > 3000.0
    nsamples = 6
    samples = db.sample_smoothed(nsamples, seed=4)
    direct = _host(db.route_metrics(samples, pairs, dtw=True))
    sh = samples.cpu().numpy()
    sref = rc.route_metrics(sh, hb.nsteps, pairs)
    at_tie, len_tie = rc.near_ties(sh, hb.nsteps, pairs, ref=sref)
    _compare(direct, sref, "sampled tracks", at_tie, len_tie)
    last = None
    for within in (5.0, 50.0, 500.0, 5000.0):
        one = batch.route_statistics(db, pairs, within, nsamples, seed=4, chunk=16, dtw=True, quantiles=(0.25, 0.5))
        assert np.array_equal(_bits(one["frechet_smoothed"]), _bits(got["frechet"][0]))
        assert np.array_equal(one["frechet_at_smoothed"], got["frechet_at"][0]) and np.array_equal(one["status"], got["status"][0])
        assert np.array_equal(_bits(one["dtw_smoothed"]), _bits(got["dtw"][0]))
        assert ((one["prob_within"] >= 0.0) & (one["prob_within"] <= 1.0)).all()
        assert np.array_equal(one["prob_within"], (direct["frechet"] <= within).mean(axis=0)), within  # one chunk: sample_smoothed's draws
        if last is not None:
            assert (one["prob_within"] >= last).all()
        last = one["prob_within"]
        assert not one["nbad"].any() and not one["sample_status"].any() and one["sample_status"].shape == (hb.B,)
        assert np.allclose(one["frechet_mean"], direct["frechet"].mean(axis=0), rtol=1e-13)
        assert np.allclose(one["dtw_per_cell_mean"], (direct["dtw"] / direct["dtw_len"]).mean(axis=0), rtol=1e-13)
        assert np.allclose(one["frechet_quantiles"], np.quantile(direct["frechet"], (0.25, 0.5), axis=0), rtol=1e-13, atol=1e-15)
    assert last[1] == 0.0 and last[4] == 1.0 and last[0] == 1.0  # 60 degrees apart; a sample against itself; copies, 5000 km
    two = batch.route_statistics(db, pairs, 50.0, nsamples, seed=4, chunk=2)
    assert "dtw_smoothed" not in two and "frechet_quantiles" not in two and two["prob_within"][4] == 1.0
    a = batch.route_statistics(hb, pairs, 50.0, 3, seed=9, chunk=3)
    b = batch.route_statistics(db, pairs, 50.0, 3, seed=9, chunk=3)
    assert set(a) == set(b) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in b)
    with pytest.raises(ValueError, match="nsamples and chunk must be >= 1"):
        batch.route_statistics(db, pairs, 50.0, 0)
    # curves that are no tracks of a batch
    t0, t1, t3 = sm[0, :, :2, 0], sm[0, :, :2, 1], sm[0, :14, :2, 3]
    own = batch.curve_distance([t0, t0, t3], [t0, t3, t1], dtw=True)
    assert own["frechet"][0] == 0.0 and own["dtw"][0] == 0.0 and own["dtw_len"][0] == 21 and not own["status"].any()
    for k in OUTPUTS:
        assert np.array_equal(_bits(own[k][1]), _bits(got[k][0, 2])), k   # (0, 3) of the batch
        assert np.array_equal(_bits(own[k][2]), _bits(got[k][0, 3])), k   # (3, 1) of the batch
    back = batch.curve_distance(t0, t0[::-1].copy(), reverse=True, model="wgs84")
    assert back["frechet"][0] == 0.0 and set(back) == {"frechet", "frechet_at", "status"}
    with pytest.raises(ValueError, match="equally long, non-empty lists"):
        batch.curve_distance([t0], [t0, t3])
    with pytest.raises(ValueError, match=r"\(n, 2\) array"):
        batch.curve_distance([t0[:, :1]], [t0])
    cand = batch.route_candidates(db, 100.0, margin_km=100.0)
    assert cand.dtype == db.torch.int32 and cand.device == db.device
    c = [tuple(p) for p in cand.cpu().numpy().tolist()]
    assert (0, 1) in c and all(2 not in p for p in c) and c == sorted(c)


@pytest.mark.gpu
def test_route_distance_of_the_drop_in_filter():
    """UnscentedKalmanFilter.route_distance on the committed ship 01203823 against its own observations: what curve_distance
    gives on the same arrays; with nsamples = 0 the zero-draw sample; with samples those of sample_smoothed."""
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
    obs = np.ascontiguousarray(c["z"][:2].T)
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.route_distance(obs)
    ukf.run(nsteps=len(c["dt"]), dt=c["dt"], ship_track=st)
    hb = ukf._sample_hb
    db = batch.DeviceBatch(hb)
    db.run()
    torch = db.torch
    sm = db.sm_mean[:, :2, 0].cpu().numpy()
    for kw in (dict(), dict(dtw=True, model="wgs84"), dict(reverse=True)):
        want = batch.curve_distance([sm], [obs], **kw)
        got = ukf.route_distance(obs, **kw)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(_bits(np.asarray(got[k])), _bits(want[k][0])), (kw, k)
    got = ukf.route_distance(obs, dtw=True)
    assert isinstance(got["frechet"], float) and isinstance(got["dtw_len"], int) and got["status"] == 0
    assert 0.0 < got["frechet"] < np.inf and got["dtw_len"] >= max(len(sm), len(obs))
    zero = db.sample_smoothed(1, draws=torch.zeros((1, hb.Nmax + 1, 4, hb.B), dtype=torch.float64, device=db.device))
    zd = batch.curve_distance([zero[0, :, :2, 0].cpu().numpy()], [obs], dtw=True)
    for k in zd:
        assert np.array_equal(_bits(np.asarray(got[k])), _bits(zd[k][0])), k
    n = 4
    vis = ukf.route_distance(obs, nsamples=n, dtw=True, random_state=3)
    samples = ukf.sample_smoothed(n, 3)
    want = batch.curve_distance([np.ascontiguousarray(t[:, :2]) for t in samples], [obs] * n, dtw=True)
    for k in want:
        assert vis[k].shape == want[k].shape and vis[k].shape[0] == n and np.array_equal(_bits(vis[k]), _bits(want[k])), k
    assert not np.array_equal(vis["frechet"], np.full(n, got["frechet"]))
    with pytest.raises(ValueError, match="nsamples must be >= 0"):
        ukf.route_distance(obs, nsamples=-1)


@pytest.mark.gpu
def test_refusals_before_any_launch():
    """The refusals again on the device build: -1, never a launch error, and the device stays usable."""
    _abi_refusals()
    h, db, full = _hand_db()
    got = _host(db.route_metrics(full, h["pairs"][:1]))
    assert got["frechet"][0, 0] == 0.0
