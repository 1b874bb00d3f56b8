"""CPU-side checks of the lag-one additions to the C ABI (include/ste.h: ste_lag_one_f64, ste_position_cov_f64): the ctypes
mirrors have the header's fields in the header's order and the documented sizes, and the entry points are declared, bound and
exported."""
import ctypes as C
import os
import re

from conftest import ROOT


def _fields(hdr, cname):
    body = hdr[hdr.index("typedef struct %s {" % cname): hdr.index("} %s;" % cname)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(?:const\s+)?(?:int32_t|uint32_t|int64_t|double|size_t|void)\s*\*?\s*(\w+)\s*;", body)


def test_structs_and_entry_points():
    from track_estimators._hip import binding

    hdr = open(os.path.join(ROOT, "include", "ste.h")).read()
    for proto in (r"int ste_urtss_lag_one_f64\(const ste_ukf_batch_f64\* b, const ste_ukf_noise_f64\* nz, "
                  r"const ste_lag_one_f64\* lg, void\* stream\);",
                  r"int ste_track_position_cov_f64\(const ste_ukf_batch_f64\* b, const ste_position_cov_f64\* pc, void\* stream\);"):
        assert re.search("^" + proto, hdr, flags=re.M), proto
    assert _fields(hdr, "ste_lag_one_f64") == [f[0] for f in binding.SteLagOneF64._fields_] == ["lag1", "status", "flags", "reserved"]
    assert _fields(hdr, "ste_position_cov_f64") == [f[0] for f in binding.StePositionCovF64._fields_] == [
        "flags", "reserved", "nqueries", "qtrack", "qtime", "t0", "knots", "cov", "lag1", "pcov", "step", "frac", "status"]
    assert C.sizeof(binding.SteLagOneF64) == 24 and "} ste_lag_one_f64;     /* 24 bytes */" in hdr
    assert C.sizeof(binding.StePositionCovF64) == 96 and "} ste_position_cov_f64;     /* 96 bytes */" in hdr
    assert C.sizeof(binding.SteUkfBatchF64) == 264  # unchanged: the new arguments travel beside the batch
    assert int(re.search(r"#define STE_VERSION (\d+)", hdr).group(1)) == 340  # an unnumbered addition
    for name, value in (("STE_LAG1_POSITION", 0x1), ("STE_PCOV_FULL", 0x1), ("STE_PCOV_LAG1_POSITION", 0x2)):
        assert int(re.search(r"#define %s (0x[0-9a-f]+)u" % name, hdr).group(1), 16) == getattr(binding, name) == value
    lib = binding.load()
    for name in ("ste_urtss_lag_one_f64", "ste_track_position_cov_f64"):
        assert name in binding.SYMBOLS and hasattr(lib, name)
    # the ordering against a two-kernel smoother on another stream is the caller's, and the header says so
    assert "never beside it" in hdr[hdr.index("LAG-ONE COVARIANCE"): hdr.index("typedef struct ste_lag_one_f64 {")]
