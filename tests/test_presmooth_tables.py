"""The host tables of the pre-smoothing filters (batch.box_filter, batch.savgol_filter_table) and the ABI's argument checks,
without a GPU.

The tables are exact rationals rounded once; scipy's own weights come from a floating-point least-squares solve and differ
from them by its rounding (3.9e-14 at worst on the machine where the bound below was set, and that varies with the LAPACK
build, hence 1e-12).  The restatement of the filter form is tests/presmooth_cases.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from conftest import GOLDEN

import presmooth_cases as pc
from track_estimators import batch

SAVGOL = [(20, 4), (4, 2), (5, 2), (7, 3), (6, 3)]
EINVAL = -1  # STE_EINVAL of include/ste.h


@pytest.mark.parametrize("w,p", SAVGOL)
def test_savgol_table_is_scipys_operator(w, p):
    from scipy.signal import savgol_filter

    f = batch.savgol_filter_table(w, p)
    assert (f.window, f.nedge, f.left) == (w, w // 2, w // 2 if w % 2 else w // 2 - 1)
    assert f.taps.shape == (w,) and f.edge.shape == (w // 2, w)
    for n in (w, w + 1, 34, 2 * w + 3):
        ref = savgol_filter(np.eye(n), w, p, axis=0)  # column j = the filter applied to unit vector j
        diff = float(np.max(np.abs(pc.dense_operator(f, n) - ref)))
        print(f"savgol ({w},{p}) n={n}: max |table - scipy| = {diff:.2e}")
        assert diff <= 1e-12, (w, p, n, diff)


@pytest.mark.parametrize("w", [2, 4, 5, 9])
def test_box_filter_is_np_convolve_same(w):
    f = batch.box_filter(w)
    assert (f.window, f.left, f.nedge) == (w, w // 2, 0) and np.array_equal(f.taps, np.full(w, 1.0 / w))
    rng = np.random.default_rng(w)
    for n in (w, w + 1, 31):
        y = rng.normal(0, 10, n)
        ref = np.convolve(y, np.ones(w) / w, "same")
        assert np.max(np.abs(pc.apply(f, y) - ref)) <= w * 2.0 ** -52 * np.max(np.abs(y))
        assert np.max(np.abs(pc.dense_operator(f, n) @ y - ref)) <= w * 2.0 ** -52 * np.max(np.abs(y))


def test_box_filter_on_the_reference_cli_fixture():
    g = np.load(os.path.join(GOLDEN, "cli_smooth.npz"))
    f = batch.box_filter(int(g["box"]))
    for raw, want in ((g["raw_sog"], g["sog"]), (g["raw_cog"], g["cog"])):
        assert np.max(np.abs(pc.apply(f, raw) - want)) <= 5 * 2.0 ** -52 * np.max(np.abs(raw))
    y = np.arange(7.0) ** 2  # the even window: make_golden.smooth_case, smooth(arange(7) ** 2, 4)
    assert np.max(np.abs(pc.apply(batch.box_filter(4), y) - g["smooth_even"])) <= 4 * 2.0 ** -52 * np.max(np.abs(y))


def test_savgol_tables_on_the_reference_example_fixture():
    g = np.load(os.path.join(GOLDEN, "savgol_example.npz"))
    for (w, p), raw, want in (((20, 4), g["raw_sog"], g["sog"]), ((4, 2), g["raw_cog"], g["cog"])):
        diff = float(np.max(np.abs(pc.apply(batch.savgol_filter_table(w, p), raw) - want)))
        print(f"savgol ({w},{p}) on the example: max |diff| = {diff:.2e}, relative {diff / np.max(np.abs(raw)):.2e}")
        assert diff <= 1e-10 * np.max(np.abs(raw))


@pytest.mark.parametrize("w,p", SAVGOL + [(128, 8), (3, 0), (9, 8)])
def test_savgol_weights_sum_to_one(w, p):
    f = batch.savgol_filter_table(w, p)
    for row in [f.taps] + list(f.edge):
        assert abs(math.fsum(row) - 1.0) <= 4 * 2.0 ** -52  # a fit of any order reproduces a constant


def test_limits_raise():
    for w in (1, 0, -3, 129, 2.0, True):
        with pytest.raises(ValueError):
            batch.box_filter(w)
        with pytest.raises(ValueError):
            batch.savgol_filter_table(w, 1)
    for w, p in ((5, 5), (5, -1), (20, 9), (4, 1.0), (2, 2)):
        with pytest.raises(ValueError):
            batch.savgol_filter_table(w, p)
    batch.box_filter(2), batch.box_filter(128), batch.savgol_filter_table(2, 1), batch.savgol_filter_table(128, 8)


def test_fir_struct_matches_header():
    import re

    from conftest import ROOT
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    body = hdr[hdr.index("typedef struct ste_fir_f64 {"): hdr.index("} ste_fir_f64;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:const\s+)?(?:int32_t|double)\s*\*?\s*(\w+)\s*;", body)
    assert fields == [f[0] for f in binding.SteFirF64._fields_]
    assert C.sizeof(binding.SteFirF64) == 4 * 4 + 2 * 8


def test_bad_descriptors_are_refused_without_a_launch():
    """STE_EINVAL with the argument named in ste_last_error(), before anything touches a device (the pointers are never
    dereferenced: argument errors come first)."""
    from track_estimators._hip import binding

    lib = binding.load()
    pb = binding.StePrepBatchF64()
    pb.B, pb.Tmax, pb.model = 4, 8, binding.STE_PREP_SPHERE
    nbytes = 4 * 8 * 8
    for i, name in enumerate(("lon", "lat", "gap", "sog", "cog", "sog_rate", "cog_rate")):
        setattr(pb, name, 0x100000 + i * nbytes)
    pb.z = 0x200000
    ws = (0x300000, 0x300000 + nbytes)

    def fir(**kw):
        f = binding.SteFirF64()
        f.window, f.left, f.nedge, f.circular, f.taps, f.edge = 5, 2, 2, 0, 0x400000, 0x500000
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def refused(fs, fc, raw_sog, raw_cog, *words):
        rc = lib.ste_track_prep_smooth_f64(C.byref(pb), C.byref(fs) if fs else None, C.byref(fc) if fc else None, raw_sog, raw_cog,
                                           None)
        msg = lib.ste_last_error()
        assert rc == EINVAL, (rc, words)
        assert all(w in msg for w in words), (msg, words)

    refused(fir(), None, None, ws[1], b"raw_sog")
    refused(fir(), None, ws[0], None, b"raw_cog")
    refused(fir(), None, ws[0], ws[0], b"alias")
    refused(fir(), None, ws[0], ws[0] + 8, b"alias")  # overlapping, not equal
    refused(fir(), None, pb.sog, ws[1], b"alias")
    refused(fir(), None, ws[0], pb.cog_rate, b"alias")
    refused(fir(), None, ws[0], pb.z + 3 * nbytes, b"alias")
    for name in ("lon", "lat", "gap"):  # the inputs the later kernels still read
        refused(fir(), None, ws[0], getattr(pb, name) + 8, b"alias")
    nobs_at = 0x600000
    pb.nobs = nobs_at
    refused(fir(), None, nobs_at - nbytes + 8, ws[1], b"alias")
    pb.nobs = None
    for name in ("sog", "cog"):  # the call's own outputs: ste_track_prep_f64 below only sees the workspace in their place
        was = getattr(pb, name)
        setattr(pb, name, None)
        refused(fir(), None, *ws, name.encode(), b"required")
        refused(None, None, *ws, name.encode(), b"required")
        setattr(pb, name, was)
    for B, T in ((0, 8), (-1, 8), (4, 0)):
        pb.B, pb.Tmax = B, T
        refused(fir(), None, *ws, b"B must be")
    pb.B, pb.Tmax = 4, 8
    for bad in (1, 0, 129, -4):
        refused(fir(window=bad), None, *ws, b"fir_sog", b"window")
        refused(None, fir(window=bad), *ws, b"fir_cog", b"window")
    for bad in (-1, 5):
        refused(fir(left=bad), None, *ws, b"fir_sog", b"left")
    for bad in (-1, 3):
        refused(None, fir(nedge=bad), *ws, b"fir_cog", b"nedge")
    refused(fir(taps=None), None, *ws, b"fir_sog", b"taps")
    refused(None, fir(edge=None), *ws, b"fir_cog", b"edge")
    refused(None, fir(circular=2), *ws, b"fir_cog", b"circular")
    assert lib.ste_track_prep_smooth_f64(None, None, None, ws[0], ws[1], None) == EINVAL
    pb.model = 7  # what ste_track_prep_f64 refuses is refused here
    refused(fir(nedge=0, edge=None), None, *ws, b"model")


def test_front_end_refuses_short_tracks_and_circular_without_filter(monkeypatch):
    """Both are host checks that come before the device is asked for; require_gpu is stubbed so that they run anywhere."""
    from track_estimators._hip import binding

    monkeypatch.setattr(binding, "require_gpu", lambda: None)
    lons, lats, gaps = [np.arange(9.0), np.arange(4.0)], [np.arange(9.0), np.arange(4.0)], [np.ones(8), np.ones(3)]
    with pytest.raises(ValueError, match="track 1"):
        batch.prepare_observations(lons, lats, gaps, model="sphere", smooth_sog=batch.box_filter(5))
    with pytest.raises(ValueError, match="track 1"):
        batch.prepare_observations(lons, lats, gaps, model="sphere", smooth_cog=batch.savgol_filter_table(5, 2))
    with pytest.raises(ValueError, match="cog_circular"):
        batch.prepare_observations(lons, lats, gaps, model="sphere", smooth_sog=batch.box_filter(3), cog_circular=True)
