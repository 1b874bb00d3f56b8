"""The two helpers of the metric front end that lay per-track outputs and inputs out in a window's columns
(``track_estimators.batch``: ``track_outputs``, ``track_input``), on CPU tensors: width 5, column 2, two tracks."""
import ctypes as C
import math
import types

import pytest

WIDTH, COL, B = 5, 2, 2
LEADING = [(), (2,), (2, 3)]
DTYPES = ["float64", "int64", "int32", "uint8"]


class _Call(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p)]


def _fills(dtype):
    return {"float64": (None, 0, float("nan")), "uint8": (None, 0)}.get(dtype, (None, 0, -1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("leading", LEADING, ids=str)
def test_outputs_lie_in_the_windows_columns(leading, dtype, monkeypatch):
    import torch

    from track_estimators import batch

    made = []
    for fn in ("empty", "zeros", "full"):
        monkeypatch.setattr(torch, fn, lambda *a, _fn=getattr(torch, fn), _name=fn, **k: made.append(_name) or _fn(*a, **k))
    dt = getattr(torch, dtype)
    for fill in _fills(dtype):
        call = _Call()
        del made[:]
        out = batch.track_outputs(call, WIDTH, COL, B, [("a", leading, dt, fill), ("b", (), torch.float64, None)], torch.device("cpu"))
        # the allocator is the one the fill names: an empty is not filled, a fill is not left empty
        assert made == [{None: "empty", 0: "zeros"}.get(fill, "full"), "empty"], (fill, made)
        assert list(out) == ["a", "b"]
        view = out["a"]
        wide = view._base
        assert tuple(wide.shape) == leading + (WIDTH,) and wide.is_contiguous() and wide.dtype == dt
        assert tuple(view.shape) == leading + (B,) and view.stride() == wide.stride() and view.storage_offset() == COL
        assert view.untyped_storage().data_ptr() == wide.untyped_storage().data_ptr()
        assert call.a == wide.data_ptr() + wide.element_size() * COL == view.data_ptr()
        assert call.b == out["b"]._base.data_ptr() + 8 * COL
        if fill is not None:  # the whole row, the neighbours' columns included
            assert bool(torch.isnan(wide).all()) if isinstance(fill, float) and math.isnan(fill) else bool((wide == fill).all())
        view.fill_(1)  # what the kernel writes lands in the wide tensor's columns [COL, COL + B) and nowhere else
        assert bool((wide[..., COL:COL + B] == 1).all())
        if fill == 0:
            assert int(wide.sum()) == B * math.prod(leading)


def test_column_pointer_counts_in_elements():
    import torch

    from track_estimators import batch

    for dtype, size in (("float64", 8), ("int64", 8), ("int32", 4), ("uint8", 1)):
        ten = torch.zeros((3, WIDTH), dtype=getattr(torch, dtype))
        assert batch.column_pointer(ten, COL) == ten.data_ptr() + size * COL == ten[0, COL:].data_ptr()


def test_input_of_none_a_scalar_and_one_value_per_track():
    import numpy as np
    import torch

    from track_estimators import batch

    cpu = torch.device("cpu")
    keep = []
    assert batch.track_input(None, B, WIDTH, COL, keep, cpu, "x") is None
    assert batch.track_input(None, B, WIDTH, COL, keep, cpu, "x", scalar=True) == (None, None)
    # the scalar form, where the kernel takes a scalar beside the pointer (speed_metrics' threshold, simplify's limits)
    for value in (2.5, np.float64(2.5), np.asarray(2.5), torch.tensor(2.5), 2):
        ptr, scalar = batch.track_input(value, B, WIDTH, COL, keep, cpu, "x", scalar=True)
        assert ptr is None and isinstance(scalar, float) and scalar == float(value)
    assert keep == []
    # a scalar where the kernel takes a pointer alone (a clock, a line's value): the row holds it in this batch's columns
    ptr = batch.track_input(2.5, B, WIDTH, COL, keep, cpu, "x")
    assert len(keep) == 1 and ptr == keep[0].data_ptr() + 8 * COL
    assert keep[0].dtype == torch.float64 and keep[0].tolist() == [0.0, 0.0, 2.5, 2.5, 0.0]
    # one value per track, from a list, an integer array, a float32 tensor
    for value in ([1.5, -2.0], np.array([3, 4]), torch.tensor([0.5, 0.25], dtype=torch.float32)):
        for scalar in (False, True):
            del keep[:]
            got = batch.track_input(value, B, WIDTH, COL, keep, cpu, "x", scalar=scalar)
            ptr = got[0] if scalar else got
            assert not scalar or got[1] is None
            (row,) = keep
            assert tuple(row.shape) == (WIDTH,) and row.dtype == torch.float64 and ptr == row.data_ptr() + 8 * COL
            assert row.tolist() == [0.0, 0.0, float(value[0]), float(value[1]), 0.0]


def test_a_wrong_shape_raises_each_callers_own_text():
    import torch

    from track_estimators import batch

    cpu = torch.device("cpu")
    me = types.SimpleNamespace(ntracks=B, device=cpu, torch=torch)  # what the two thin callers read of a batch
    bad = [1.0, 2.0, 3.0]
    texts = {
        "t0 must be None, a scalar or have shape (2,), got (3,)":
            lambda keep: batch.DeviceBatch._track_clock(me, bad, WIDTH, COL, keep),
        "track_margin_km must be None, a scalar or have shape (2,), got (3,)":
            lambda keep: batch.DeviceBatch._track_clock(me, bad, WIDTH, COL, keep, name="track_margin_km"),
        "tolerance_km must be a scalar or have shape (2,), got (3,)":
            lambda keep: batch.DeviceBatch._track_limit(me, bad, "tolerance_km", WIDTH, COL, keep),
        "lon_scale must be a scalar or have shape (2,), got (1, 2)":
            lambda keep: batch.DeviceBatch._track_limit(me, [[1.0, 2.0]], "lon_scale", WIDTH, COL, keep),
        # the two that call the placer themselves (path_metrics, speed_metrics) pass these beginnings
        "line_value must be a scalar or have shape (2,), got (3,)":
            lambda keep: batch.track_input(bad, B, WIDTH, COL, keep, cpu, f"line_value must be a scalar or have shape ({B},)"),
        "threshold must be None, a scalar or have shape (2,), got (3,)":
            lambda keep: batch.track_input(bad, B, WIDTH, COL, keep, cpu, f"threshold must be None, a scalar or have shape ({B},)",
                                           scalar=True),
    }
    for text, call in texts.items():
        keep = []
        with pytest.raises(ValueError) as err:
            call(keep)
        assert str(err.value) == text and keep == []
    # and the callers' results in their own forms
    keep = []
    assert batch.DeviceBatch._track_clock(me, None, WIDTH, COL, keep) is None
    assert batch.DeviceBatch._track_limit(me, 0.5, "tolerance_km", WIDTH, COL, keep) == (None, 0.5) and keep == []
    ptr, beside = batch.DeviceBatch._track_limit(me, [0.5, 0.75], "tolerance_km", WIDTH, COL, keep)
    assert beside == 0.0 and ptr == keep[0].data_ptr() + 8 * COL and keep[0].tolist() == [0.0, 0.0, 0.5, 0.75, 0.0]
