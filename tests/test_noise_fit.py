"""The measurement noise R fitted to the data by EM on the device (include/ste.h: ste_ukf_noise_moments_f64,
ste_ukf_noise_mstep_f64; DESIGN.md, "Noise fit"): declarations, layouts and refusals of the two calls, the refusals of the
front end, the restated group sum against math.fsum and the EM on the pinned oracle against the generator of the mixed fleet
(CPU); on the GPU both kernels against their restatements bit for bit, the fit on the mixed fleet against the grid's answers,
parity with the oracle EM, the bit-identity of the fitted batch with a shared launch, and the drop-in class."""
import ctypes as C
import dataclasses
import math
import os
import re
import types

import noise_fit_cases as nfc
import numpy as np
import pytest
import track_sampling_cases as tsc
from conftest import ROOT
from test_ukf_loglik import LIK_RTOL, _batch
from test_ukf_track_noise import ORACLE_BEST_SHARED, ORACLE_SUM_OF_MAXIMA, mixed_fleet

MOMENT_FIELDS = ["moments", "count", "vsum", "track_status", "flags", "reserved"]
MSTEP_FIELDS = ["ntracks", "ngroups", "nmembers", "structure", "ld", "moments", "count", "group_offsets", "group_members",
                "R_group", "n_group", "group_status", "R_tracks", "reserved"]
R_RTOL = 1e-6  # the project's history parity bound (tests/test_hip_parity.py MEAN_TOL), which the issue sets for R too
EVEN_R, ODD_R = (0.00125, 0.005), (0.02, 0.08)  # brackets of a factor 2 (4 for the odd tracks' upper end) about 0.05^2 and 0.2^2


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_header_declares_structs_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for proto in (r"int ste_ukf_noise_moments_f64\(const ste_ukf_batch_f64\* b, const ste_noise_moments_f64\* nm, void\* stream\);",
                  r"int ste_ukf_noise_mstep_f64\(const ste_noise_mstep_f64\* ms, void\* stream\);"):
        assert re.search("^" + proto, hdr, flags=re.M), proto
    for cname, mirror, fields, size in (("ste_noise_moments_f64", binding.SteNoiseMomentsF64, MOMENT_FIELDS, 40),
                                        ("ste_noise_mstep_f64", binding.SteNoiseMstepF64, MSTEP_FIELDS, 96)):
        body = hdr[hdr.index("typedef struct %s {" % cname): hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        found = re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double)\s*\*?\s*(\w+)\s*;", body)
        assert found == [f[0] for f in mirror._fields_] == fields, cname
        assert C.sizeof(mirror) == size and re.search(r"} %s;\s*/\* %d bytes \*/" % (cname, size), hdr), cname
    # by hand: four pointers, two words | four words, one int64, eight pointers, one int64
    assert [getattr(binding.SteNoiseMomentsF64, f).offset for f in MOMENT_FIELDS] == [0, 8, 16, 24, 32, 36]
    assert [getattr(binding.SteNoiseMstepF64, f).offset for f in MSTEP_FIELDS] == [0, 4, 8, 12] + [16 + 8 * k for k in range(10)]
    for name in ("ste_ukf_noise_moments_f64", "ste_ukf_noise_mstep_f64"):
        assert name in binding.SYMBOLS and hasattr(binding.load(), name)
        assert "(ste_ukf_noise_moments_f64, ste_ukf_noise_mstep_f64)" in hdr[hdr.index("#define STE_VERSION"): hdr.index("/* error codes */")]
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: both structs travel beside the batch
    for name, value in (("STE_NOISE_TRACK_NAN", nfc.TRACK_NAN), ("STE_NOISE_TRACK_NOT_FINITE", nfc.TRACK_NOT_FINITE),
                        ("STE_NOISE_GROUP_EMPTY", nfc.GROUP_EMPTY), ("STE_NOISE_GROUP_BAD_VARIANCE", nfc.GROUP_BAD_VARIANCE),
                        ("STE_NOISE_GROUP_BAD_MEMBER", nfc.GROUP_BAD_MEMBER)):
        assert int(re.search(r"#define %s 0x(\d+)" % name, hdr).group(1), 16) == getattr(binding, name) == value, name
    for name, value in nfc.STRUCTURES.items():
        cname = "STE_NOISE_FIT_" + name.upper()
        assert int(re.search(r"#define %s (\d+)" % cname, hdr).group(1)) == getattr(binding, cname) == value


def _good_moments(binding, keep):
    s = _batch(binding, keep)
    s.sm_mean = s.sm_cov = 0x6000
    return s, binding.SteNoiseMomentsF64(0x7000, 0x8000, 0x9000, 0xA000, 0, 0)


def test_moments_refusals_before_any_launch():
    """Every refusal of the header returns STE_EINVAL (-1) with the call's name; a launch on a machine without a GPU would
    return STE_ELAUNCH (-2).  The device pointers are not memory: nothing may be launched."""
    from track_estimators._hip import binding

    lib, keep = binding.load(), []
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731

    def refused(reason, with_batch=True, with_nm=True, **fields):  # nm_<field>: a field of the moment arguments
        s, nm = _good_moments(binding, keep)
        for name, value in fields.items():
            if name.startswith("nm_"):
                setattr(nm, name[3:], value)
            else:
                setattr(s, name, value)
        rc = lib.ste_ukf_noise_moments_f64(ref(s) if with_batch else None, ref(nm) if with_nm else None, None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_ukf_noise_moments_f64" in msg, (fields, rc, msg)

    refused("batch pointer is NULL", with_batch=False)
    refused("(nm) are NULL", with_nm=False)
    refused("nm->moments and nm->count are required", nm_moments=None)
    refused("nm->moments and nm->count are required", nm_count=None)
    for name in ("sm_mean", "sm_cov"):
        refused("sm_mean and sm_cov are required", **{name: None})
    for name in ("z", "upd_idx"):
        refused("z and upd_idx are required", **{name: None})
    refused("H is required", H=None)
    refused("STE_FLAG_ROBUST is refused", flags=binding.STE_FLAG_ROBUST)
    refused("recorded noise is refused", noise_upd=0xB000)
    for b, e in ((64, 0), (0, 128), (64, 256)):
        refused("time slices are refused", step_begin=b, step_end=e)
    refused("must be 0", nm_reserved=1)
    refused("must be 0", nm_flags=1)
    refused("B must be > 0", B=0)
    refused("track_stride must be 0 or >= B", track_stride=4)
    # accepted shapes stop at the launch, not before it: a whole-pass step range, a window's stride
    s, nm = _good_moments(binding, keep)
    s.step_end, s.track_stride = s.Nmax, 16
    if lib.ste_device_count() == 0:
        assert lib.ste_ukf_noise_moments_f64(C.byref(s), C.byref(nm), None) == -2


def test_mstep_refusals_before_any_launch():
    from track_estimators._hip import binding

    lib = binding.load()

    def good():
        return binding.SteNoiseMstepF64(8, 2, 8, binding.STE_NOISE_FIT_SCALAR, 0, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000,
                                        0x7000, 0x8000, 0)

    def refused(reason, **fields):
        ms = good()
        for name, value in fields.items():
            setattr(ms, name, value)
        rc = lib.ste_ukf_noise_mstep_f64(C.byref(ms), None)
        msg = lib.ste_last_error().decode()
        assert rc == -1 and reason in msg and "ste_ukf_noise_mstep_f64" in msg, (fields, rc, msg)

    assert lib.ste_ukf_noise_mstep_f64(None, None) == -1 and "(ms) are NULL" in lib.ste_last_error().decode()
    for name in ("moments", "count"):
        refused("ms->moments and ms->count are required", **{name: None})
    for name in ("R_group", "n_group", "group_status", "R_tracks"):
        refused("are required", **{name: None})
    refused("come together", group_offsets=None)
    refused("come together", group_members=None)
    refused("ngroups must equal ntracks", group_offsets=None, group_members=None)
    refused("ms->structure must be", structure=3)
    refused("ms->reserved must be 0", reserved=1)
    refused("ntracks and ngroups must be > 0", ntracks=0)
    refused("ntracks and ngroups must be > 0", ngroups=0)
    refused("ntracks and ngroups must be > 0", nmembers=-1)
    refused("ld must be 0 or >= ntracks", ld=4)


def test_fit_refuses_before_touching_the_device():
    from track_estimators import batch

    hb = tsc.host_batch(np.arange(4))
    with pytest.raises(ValueError, match="robust batch"):
        batch.fit_measurement_noise(dataclasses.replace(hb, robust=True))
    with pytest.raises(ValueError, match="recorded noise"):
        batch.fit_measurement_noise(dataclasses.replace(hb, noise_upd=np.zeros((hb.Nmax + 1, 4, hb.B))))
    with pytest.raises(ValueError, match="lanes=4"):
        batch.fit_measurement_noise(dataclasses.replace(hb, lanes=4))
    with pytest.raises(ValueError, match=r"one label per track, \(4,\)"):
        batch.fit_measurement_noise(hb, groups=np.arange(5))
    with pytest.raises(ValueError, match="one label per track"):
        batch.fit_measurement_noise(hb, groups=np.zeros(4))  # floats are not labels
    with pytest.raises(ValueError, match="structure must be one of"):
        batch.fit_measurement_noise(hb, structure="full")
    with pytest.raises(ValueError, match="leading 2 x 2 block"):
        batch.fit_measurement_noise(dataclasses.replace(hb, R=np.diag([0.25, 0.25, 0.01, 0.0])))


def test_groups_follow_the_callers_track_order():
    from track_estimators import batch

    hb = dataclasses.replace(tsc.host_batch(np.arange(4)), order=np.array([2, 0, 3, 1]))  # slot -> caller's track
    slots, labels = batch._noise_fit_groups(hb, np.array([7, 7, 9, 3]))
    assert labels.tolist() == [3, 7, 9] and slots.tolist() == [2, 1, 0, 1]
    slots, labels = batch._noise_fit_groups(hb, "track")
    assert slots.tolist() == [2, 0, 3, 1] and labels.tolist() == [0, 1, 2, 3]
    slots, labels = batch._noise_fit_groups(hb, None)
    assert slots.tolist() == [0, 0, 0, 0] and len(labels) == 1


def test_restated_group_sum_equals_fsum():
    """The lane-strided partial sums and the shuffle tree add every member exactly once: against math.fsum (the exact sum,
    rounded once) to 1e-12 relative, for the group sizes at which a lane holds 0, 1, 2 or 3 members."""
    rng = np.random.default_rng(5)
    for size in (0, 1, 63, 64, 65, 130):
        x = rng.uniform(0.5, 2.0, size) * 10.0 ** rng.integers(-3, 3, size)
        got, want = float(nfc.wave_sum(x)), math.fsum(x)
        assert abs(got - want) <= 1e-12 * abs(want), (size, got, want)


def test_oracle_em_separates_the_two_populations_of_the_mixed_fleet():
    """EM on the pinned oracle, two groups (even / odd tracks), scalar structure, 6 iterations from the shipped R = 0.25: the
    best iterate beats the best shared grid candidate, and the two fitted variances bracket the generator's 0.05^2 and 0.2^2."""
    from track_estimators import synthetic

    H, Q, R0, P0 = synthetic.example_matrices()
    groups = [list(range(0, 16, 2)), list(range(1, 16, 2))]
    R, ll, _ = nfc.oracle_em(mixed_fleet(), 4, H, Q, R0, P0, groups, "scalar", 6)
    fleet = ll.sum(axis=1)
    best = int(np.argmax(fleet))
    print("oracle EM, fleet loglik by iteration:", np.round(fleet, 2), "r:", R[best, :, 0, 0])
    assert fleet[best] > ORACLE_BEST_SHARED[1]
    assert EVEN_R[0] <= R[best, 0, 0, 0] <= EVEN_R[1] and ODD_R[0] <= R[best, 1, 0, 0] <= ODD_R[1]


# ----------------------------------------------------------------------------------------------------------------
# GPU: the moments kernel
# ----------------------------------------------------------------------------------------------------------------
GENERAL_H = np.array([[1.0, 0.1, 0.0, 0.0], [0.2, 1.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.01], [0.0, 0.0, 0.0, 1.0]])


def _ragged(B):
    """The eight tracks repeated, every length from Nmax down to 0: among them nsteps = 0 and nsteps = 1, whose only update
    is the initial one (2 substeps: the first update after a step follows step 1)."""
    return np.arange(B) % 8, (tsc.NMAX - (np.arange(B) * 5) % (tsc.NMAX + 1)).astype(np.int32)


def _smoothed(hb, **kw):
    from track_estimators import batch

    db = batch.DeviceBatch(dataclasses.replace(hb, lanes=1), **kw)
    db.run()
    return db


def _check_moments(db, got=None):
    """measurement_moments() of ``db`` against the restatement on the device's own downloaded rows, bit for bit."""
    got = db.measurement_moments() if got is None else got
    lo, hi = db.lo, db.lo + db.ntracks
    host = lambda t: t.cpu().numpy()  # noqa: E731
    mom, cnt, vsum, tst = nfc.restate_moments(db.hb.H, db.hb.nsteps[lo:hi], host(db.t["upd_idx"])[:, lo:hi], host(db.t["z"])[..., lo:hi],
                                              host(db.sm_mean), host(db.sm_cov), host(db.status))
    out = {k: host(v) for k, v in got.items()}
    assert np.array_equal(_u64(out["moments"]), _u64(mom))
    assert np.array_equal(_u64(out["vsum"]), _u64(vsum))
    assert np.array_equal(out["count"], cnt) and np.array_equal(out["track_status"], tst)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "full"])
@pytest.mark.parametrize("general_h", [False, True], ids=["H-diag", "H-general"])
def test_moments_match_the_restatement(packed, general_h):
    """The eight tracks with a ragged copy of them, packed and full covariances, the reference's H and a non-diagonal one."""
    idx = np.arange(16) % 8
    nsteps = np.concatenate([np.full(8, tsc.NMAX), [12, 11, 9, 7, 5, 3, 1, 0]]).astype(np.int32)
    hb = tsc.host_batch(idx, nsteps)
    if general_h:
        hb = dataclasses.replace(hb, H=GENERAL_H.copy())
    out = _check_moments(_smoothed(hb, packed_cov=packed))
    updates = nsteps // tsc.SUBSTEPS
    assert out["count"].tolist() == updates.tolist() and not out["track_status"].any()
    assert out["count"][14] == 0 and out["count"][15] == 0  # the initial update alone; no step at all
    assert np.all(out["moments"][0, :14] > 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [65, 129])
def test_moments_with_a_wave_edge_inside_the_batch(B):
    idx, nsteps = _ragged(B)
    out = _check_moments(_smoothed(tsc.host_batch(idx, nsteps)))
    assert out["count"].tolist() == (nsteps // tsc.SUBSTEPS).tolist()


@pytest.mark.gpu
def test_moments_of_a_window_equal_those_of_a_batch_of_its_own():
    idx, nsteps = _ragged(129)
    fleet = _smoothed(tsc.host_batch(idx, nsteps))
    win = _check_moments(fleet.window(3, 70))
    own = _check_moments(_smoothed(tsc.host_batch(idx[3:70], nsteps[3:70])))
    for k in ("moments", "vsum", "count", "track_status"):
        assert np.array_equal(_u64(win[k]) if win[k].dtype == np.float64 else win[k],
                              _u64(own[k]) if own[k].dtype == np.float64 else own[k]), k


@pytest.mark.gpu
def test_a_nan_observation_empties_its_track_and_no_other():
    idx = np.arange(70) % 8
    hb = tsc.host_batch(idx)
    clean = _check_moments(_smoothed(hb))
    z = hb.z.copy()
    z[3, 0, 37] = np.nan  # observation 3 of slot 37: its longitude
    bad = _check_moments(_smoothed(dataclasses.replace(hb, z=z)))
    assert bad["count"][37] == 0 and bad["track_status"][37] != 0 and not bad["moments"][:, 37].any() and not bad["vsum"][:, 37].any()
    others = np.arange(70) != 37
    assert not bad["track_status"][others].any()
    for k in ("moments", "vsum"):
        assert np.array_equal(_u64(bad[k][:, others]), _u64(clean[k][:, others]))
    assert np.array_equal(bad["count"][others], clean["count"][others])


# ----------------------------------------------------------------------------------------------------------------
# GPU: the M-step kernel
# ----------------------------------------------------------------------------------------------------------------
GROUP_SIZES = (1, 63, 64, 65, 130, 0, 2)  # the last group's tracks carry zero moments: a variance of 0


def _mstep_case():
    rng = np.random.default_rng(11)
    B = sum(GROUP_SIZES) + 5  # five tracks in no group, without updates: as groups of their own they are empty ones
    count = rng.integers(1, 26, B).astype(np.int32)
    mom = rng.normal(0.0, 1.0, (10, B)) * 1e-3
    mom[[0, 4]] = rng.uniform(0.5, 2.0, (2, B)) * 10.0 ** rng.integers(-4, 0, (2, B))
    mom *= count
    perm = rng.permutation(B)
    members, outside = perm[: sum(GROUP_SIZES)].astype(np.int32), perm[sum(GROUP_SIZES):]
    offsets = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int32)
    zero = members[offsets[-2]:]
    mom[:, zero], count[zero] = 0.0, 3
    mom[:, outside], count[outside] = 0.0, 0
    R_tracks = rng.uniform(0.1, 0.2, (10, B))
    return mom, count, offsets, members, R_tracks


def _device_mstep(mom, count, offsets, members, structure, R_tracks):
    import torch
    from track_estimators._hip import binding

    lib = binding.require_gpu()
    dev = torch.device("cuda:0")
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    B = mom.shape[1]
    G = B if offsets is None else len(offsets) - 1
    m, c, o, me, Rt = up(mom), up(count), up(offsets), up(members), up(R_tracks)
    Rg = torch.full((10, G), -1.0, dtype=torch.float64, device=dev)
    ng = torch.full((G,), -1, dtype=torch.int32, device=dev)
    gs = torch.full((G,), -1, dtype=torch.int32, device=dev)
    ms = binding.SteNoiseMstepF64(B, G, 0 if members is None else len(members), nfc.STRUCTURES[structure], 0, ptr(m), ptr(c),
                                  ptr(o), ptr(me), ptr(Rg), ptr(ng), ptr(gs), ptr(Rt), 0)
    binding.check(lib.ste_ukf_noise_mstep_f64(C.byref(ms), None), "ste_ukf_noise_mstep_f64")
    torch.cuda.synchronize()
    return Rg.cpu().numpy(), ng.cpu().numpy(), gs.cpu().numpy(), Rt.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("structure", list(nfc.STRUCTURES))
@pytest.mark.parametrize("grouped", [True, False], ids=["groups", "null-groups"])
def test_mstep_matches_the_restatement(structure, grouped):
    """Group sizes 1, 63, 64, 65, 130, an empty group and one whose variance is 0 in one call (or every track its own group):
    R_group, n_group, group_status and R_tracks bit for bit, and twice the same bits."""
    mom, count, offsets, members, R_tracks = _mstep_case()
    if not grouped:
        offsets = members = None
    want = nfc.restate_mstep(mom, count, offsets, members, structure, R_tracks)
    got = _device_mstep(mom, count, offsets, members, structure, R_tracks)
    again = _device_mstep(mom, count, offsets, members, structure, R_tracks)
    for w, g, a, name in zip(want, got, again, ("R_group", "n_group", "group_status", "R_tracks")):
        same = (lambda x, y: np.array_equal(_u64(x), _u64(y))) if w.dtype == np.float64 else np.array_equal
        assert same(w, g), name
        assert same(g, a), name
    Rg, ng, gs, Rt = got
    if grouped:
        assert gs.tolist() == [0, 0, 0, 0, 0, nfc.GROUP_EMPTY | nfc.GROUP_BAD_VARIANCE, nfc.GROUP_BAD_VARIANCE]
        kept = np.concatenate([members[offsets[-2]:], np.setdiff1d(np.arange(mom.shape[1]), members)])
        assert np.array_equal(_u64(Rt[:, kept]), _u64(R_tracks[:, kept]))  # a variance of 0, and tracks in no group: old bits
        assert np.all(np.delete(Rt[:, members[: offsets[-3]]], (0, 1, 4), axis=0) == 0.0)
    else:
        assert np.array_equal(gs != 0, (count == 0) | (mom[0] == 0.0))


# ----------------------------------------------------------------------------------------------------------------
# GPU: the fit
# ----------------------------------------------------------------------------------------------------------------
_FITS = {}


def _mixed_hb():
    from track_estimators import batch, synthetic

    H, Q, R, P0 = synthetic.example_matrices()
    return batch.pack_uniform(mixed_fleet(), 4, H, Q, R, P0)


def _mixed_fit(groups):
    """The three fits of the mixed fleet (16 tracks x 100 steps, scalar structure), each computed once."""
    from track_estimators import batch

    if groups not in _FITS:
        arg = {"one": None, "track": "track", "two": np.arange(16) % 2}[groups]
        _FITS[groups] = batch.fit_measurement_noise(_mixed_hb(), groups=arg, structure="scalar")
    return _FITS[groups]


@pytest.mark.gpu
@pytest.mark.parametrize("groups", ["one", "track", "two"])
def test_fit_on_the_mixed_fleet(groups):
    fit = _mixed_fit(groups)
    G = {"one": 1, "track": 16, "two": 2}[groups]
    best = fit.loglik[fit.best_iter, np.arange(G)]
    print(f"{groups}: iterations {fit.loglik.shape[0] - 1}, fleet loglik by iterate {np.round(fit.loglik.sum(axis=1), 2)}, "
          f"best {best.sum():.3f}, r {fit.R[:, 0, 0]}")
    assert fit.loglik.shape[1] == G and fit.R.shape == (G, 4, 4) and len(fit.excluded) == 0
    assert np.all(best >= fit.loglik[0]) and np.array_equal(best, fit.loglik.max(axis=0))
    assert np.all(fit.nobs == 25 * np.bincount(fit.groups, minlength=G))
    if groups == "one":
        assert best[0] > ORACLE_BEST_SHARED[1]
    elif groups == "track":
        assert best.sum() > ORACLE_SUM_OF_MAXIMA
    else:
        assert EVEN_R[0] <= fit.R[0, 0, 0] <= EVEN_R[1] and ODD_R[0] <= fit.R[1, 0, 0] <= ODD_R[1]
    # the batch holds the fitted triangles, and they are confined to the leading block
    Rt = fit.host_batch.R_tracks
    assert np.array_equal(Rt, fit.device_batch.t["R_tracks"].cpu().numpy())
    assert np.array_equal(Rt[0], fit.R[fit.groups, 0, 0]) and not np.delete(Rt, (0, 4), axis=0).any()


@pytest.mark.gpu
def test_fit_matches_the_oracle_em():
    """The eight small tracks, two groups, 4 iterations: every iterate's R within 1e-6 relative of the oracle EM's and the
    log-likelihood trace within LIK_RTOL of the sum of |l_u|."""
    from track_estimators import batch, synthetic

    H, Q, R0, P0 = synthetic.example_matrices()
    fit = batch.fit_measurement_noise(tsc.host_batch(np.arange(8)), groups=np.arange(8) % 2, structure="block2", max_iter=4, rtol=0.0)
    R, ll, ab = nfc.oracle_em(tsc.synthetic_batch(), tsc.SUBSTEPS, H, Q, R0, P0, [[0, 2, 4, 6], [1, 3, 5, 7]], "block2", 4)
    assert fit.R_trace.shape == R.shape == (5, 2, 4, 4) and fit.loglik.shape == ll.shape
    r_err = float(np.max(np.abs(fit.R_trace - R) / np.max(np.abs(R), axis=(-1, -2), keepdims=True)))
    l_err = float(np.max(np.abs(fit.loglik - ll) / ab))
    print(f"device fit against the oracle EM: R to {r_err:.2e}, loglik to {l_err:.2e} of sum |l_u|")
    assert r_err < R_RTOL and l_err < LIK_RTOL


@pytest.mark.gpu
def test_fitted_batch_is_bit_identical_to_a_shared_launch_and_runs_as_a_fleet():
    """After a one-group fit the batch's histories are those of run_batch on the plain batch with the fitted R as the shared
    one (the per-track-noise property), and NoiseFit.host_batch goes through run_fleet as it is."""
    from track_estimators import batch

    fit = _mixed_fit("one")
    mine = fit.device_batch.download()
    shared = batch.run_batch(dataclasses.replace(_mixed_hb(), R=fit.R[0], lanes=1))
    fleet = batch.run_fleet(fit.host_batch)
    for name in ("means", "covs", "means_smoothed", "covs_smoothed"):
        assert np.array_equal(_u64(mine[name]), _u64(shared[name])), name
        assert np.array_equal(_u64(mine[name]), _u64(fleet[name])), name
    assert not shared["status"].any() and not fleet["status"].any()


@pytest.mark.gpu
def test_dropin_fit_equals_the_batch_call():
    from track_estimators import batch, synthetic
    from track_estimators.kalman_filters.non_linear_process import geodetic_dynamics
    from track_estimators.kalman_filters.unscented import UnscentedKalmanFilter

    sb = tsc.synthetic_batch()
    H, Q, R, P0 = synthetic.example_matrices()
    trk = types.SimpleNamespace(z=sb.z[0], dts=sb.dts[0], sog=sb.sog[0], cog=sb.cog[0], sog_rate=sb.sog_rate[0].copy(),
                                cog_rate=sb.cog_rate[0].copy())
    ukf = UnscentedKalmanFilter(H=H, Q=Q, R=R, P=P0, x0=sb.z[0][:, 0], non_linear_process=geodetic_dynamics)
    with pytest.raises(RuntimeError, match="run\\(\\) first"):
        ukf.fit_measurement_noise()
    dt = np.repeat(sb.dts[0] / tsc.SUBSTEPS, tsc.SUBSTEPS)
    ukf.run(len(dt), dt, trk)
    Rf, trace = ukf.fit_measurement_noise(structure="diag2", max_iter=5)
    hb = batch.pack_tracks([trk], [dt], [sb.z[0][:, 0]], H, Q, R, P0)
    fit = batch.fit_measurement_noise(hb, structure="diag2", max_iter=5)
    assert Rf.shape == (4, 4) and np.array_equal(_u64(Rf), _u64(fit.R[0])) and np.array_equal(_u64(trace), _u64(fit.loglik[:, 0]))
    assert trace.max() > trace[0] and np.array_equal(ukf.R, R)
