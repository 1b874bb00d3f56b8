"""NumPy restatement of the filter form of ``struct ste_fir_f64`` (include/ste.h, "Pre-smoothing"), shared by
tests/test_presmooth_tables.py (CPU) and tests/test_presmooth.py (GPU).  A filter is anything with ``window``, ``left``,
``nedge``, ``taps`` (w,) and ``edge`` (h, w): what ``batch.box_filter`` and ``batch.savgol_filter_table`` return.

  row_weights(f, n)        per output row, the samples it reads inside [0, n) and their weights
  dense_operator(f, n)     the n x n matrix A with out = A @ y (finite y only: a dense product multiplies every sample by a 0)
  apply(f, y)              the filter over the window alone, so that a non-finite sample reaches exactly the rows that read it
  abs_sum(f, y)            sum_k |c_k y_k| per row: the scale of the dot-product rounding bound
  apply_circular(f, y)     the circular variant: wrapped differences from the row's own value, result in [0, 360)
  abs_sum_circular(f, y)   sum_k |c_k d_k| per row
"""
import numpy as np


def row_weights(f, n):
    """[(sample indices, weights)] for rows 0..n-1.  Interior row i reads y[i - left + k] against taps[k]; samples outside
    [0, n) count as zero and are left out here.  With h = nedge > 0, row i < h is edge[i] over y[0..w) and row n - 1 - r
    (r < h) is edge[r] reversed over y[n - w..n); that needs n >= w."""
    w, h = int(f.window), int(f.nedge)
    taps, edge = np.asarray(f.taps, float), np.asarray(f.edge, float).reshape(h, w)
    if h > 0 and n < w:
        raise ValueError("edge rows need n >= window")
    rows = []
    for i in range(n):
        if i < h:
            j, c = np.arange(w), edge[i]
        elif i >= n - h:
            j, c = np.arange(n - w, n), edge[n - 1 - i][::-1]
        else:
            j, c = i - int(f.left) + np.arange(w), taps
        ok = (j >= 0) & (j < n)
        rows.append((j[ok], c[ok]))
    return rows


def dense_operator(f, n):
    A = np.zeros((n, n))
    for i, (j, c) in enumerate(row_weights(f, n)):
        A[i, j] = c
    return A


def apply(f, y):
    y = np.asarray(y, float)
    with np.errstate(all="ignore"):
        return np.array([np.sum(c * y[j]) for j, c in row_weights(f, len(y))])


def abs_sum(f, y):
    y = np.asarray(y, float)
    return np.array([np.sum(np.abs(c * y[j])) for j, c in row_weights(f, len(y))])


def wrap_diff(delta):
    return delta - 360.0 * np.rint(delta / 360.0)


def apply_circular(f, y):
    """out[i] = (y[i] + sum_k c_k d_k) mod 360 with d_k = wrap_diff(y[j] - y[i]); a sample outside [0, n) has d = 0."""
    y = np.asarray(y, float)
    with np.errstate(all="ignore"):
        return np.array([np.mod(y[i] + np.sum(c * wrap_diff(y[j] - y[i])), 360.0) for i, (j, c) in enumerate(row_weights(f, len(y)))])


def abs_sum_circular(f, y):
    y = np.asarray(y, float)
    return np.array([np.sum(np.abs(c * wrap_diff(y[j] - y[i]))) for i, (j, c) in enumerate(row_weights(f, len(y)))])


def rates(v, gaps):
    """Backward difference over gap[i-1], 0 at i = 0 (ship_track.py:242-246, :296-300)."""
    v, gaps = np.asarray(v, float), np.asarray(gaps, float)
    with np.errstate(all="ignore"):
        return np.concatenate([[0.0], (v[1:] - v[:-1]) / gaps])
