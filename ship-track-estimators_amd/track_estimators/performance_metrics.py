"""Row-by-row comparison of two arrays, under the reference package's import path (``track_estimators.performance_metrics``):
``abs_diff`` is the elementwise absolute difference, ``cum_abs_diff`` its cumulative sum and ``rmse`` the root of the mean
squared difference.  The operands are broadcast to one shape; shapes that do not broadcast raise ``ValueError``.

These compare numbers as they are given -- degrees against degrees, one track at a time, on the host.  The error of tracks
that stay on the device against truth positions, in km, split along and across the true course and scored against the track's
covariance, is ``DeviceBatch.track_errors`` (``track_estimators.batch``; DESIGN.md, "Errors").
"""
import numpy as np

__all__ = ["rmse", "cum_abs_diff", "abs_diff"]


def _pair(x, xref):
    x, xref = np.asarray(x, dtype=np.float64), np.asarray(xref, dtype=np.float64)
    try:
        return np.broadcast_arrays(x, xref)
    except ValueError:
        raise ValueError(f"x and xref must broadcast to one shape, got {x.shape} and {xref.shape}") from None


def abs_diff(x, xref) -> np.ndarray:
    """|x - xref|, element by element."""
    x, xref = _pair(x, xref)
    return np.abs(x - xref)


def cum_abs_diff(x, xref) -> np.ndarray:
    """The cumulative sum of ``abs_diff`` over the flattened elements, in order."""
    return np.cumsum(abs_diff(x, xref))


def rmse(x, xref) -> float:
    """The root of the mean of (x - xref) squared over all elements."""
    x, xref = _pair(x, xref)
    d = x - xref
    return float(np.sqrt(np.mean(d * d)))
