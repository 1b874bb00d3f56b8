"""ctypes binding of the math probe (csrc/ste_probe.hip) for the tests.

The ``ste_probe_*`` entry points expose the ``__device__`` functions of csrc/ste_math.h element-wise.  They are test hooks,
not ABI: include/ste.h does not declare them and ``binding.SYMBOLS`` does not list them (tests/test_abi.py keeps those two
sets equal), so they are bound here.  The op numbers mirror the enums of ste_probe.hip.
"""
import ctypes as C

import numpy as np

# ste_probe_scalar_f64
FLOORED_MOD360, WRAP180, RSQRT_FAST, DIV_POS, DIV_EARTH_RADIUS, RCP_REFINED = 0, 1, 2, 3, 4, 5
SINCOS_KERNEL, SINCOS_FAST, SINCOS_DELTA, ATAN_SMALL, ATAN2_FAST, ASIN_SMALL = 6, 7, 8, 9, 10, 11
SINCOS_FAST3_LIT, SINCOS_FAST3_REG, SINCOS_DELTA3_LIT, SINCOS_DELTA3_REG = 12, 13, 14, 15
ATAN_SMALL3_LIT, ATAN_SMALL3_REG, ASIN_SMALL3_LIT, ASIN_SMALL3_REG = 16, 17, 18, 19
GEO_FINISH, GEO_FINISH1, GEO_FINISH2, GEO_FINISH3_REG = 20, 21, 22, 23
SCALAR_OPS = 24
# ste_probe_mat4_f64
JACOBI_EIG4, JACOBI_EIG4_WARM, SYM_SQRT4_COLD, SYM_SQRT4_WARM, SYM_PINV4, SYM_PINV4_BLOCK2, LDL_RIGHT_SOLVE4 = range(7)
MAT4_OPS = 7

_dp = C.c_void_p
_bound = None


def load():
    """The library with the two probe symbols bound (AttributeError if the probe was not linked in)."""
    global _bound
    from track_estimators._hip import binding

    lib = binding.load()
    if _bound is None:
        lib.ste_probe_scalar_f64.restype = C.c_int
        lib.ste_probe_scalar_f64.argtypes = [C.c_int32, C.c_int64, _dp, _dp, _dp, _dp, _dp, C.c_void_p]
        lib.ste_probe_mat4_f64.restype = C.c_int
        lib.ste_probe_mat4_f64.argtypes = [C.c_int32, C.c_int64, _dp, _dp, _dp, _dp, C.c_double, _dp, C.c_void_p]
        _bound = lib
    return lib


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


GUARD = -7.25  # guard element behind every output array


def run_scalar(op, in0, in1=None):
    """One launch of a scalar op over ``in0`` ([count], or [8][count] for the GEO_* ops).  Returns (out0, out1, flag); an
    output the op does not write keeps its NaN fill.  Every output has a guard element behind it, checked here."""
    import torch
    from track_estimators._hip import binding

    lib = load()
    in0 = np.asarray(in0, dtype=np.float64)
    count = in0.shape[-1]
    a = _up(in0)
    b = _up(np.zeros(count) if in1 is None else in1)
    o0 = torch.full((count + 1,), float("nan"), dtype=torch.float64, device="cuda:0")
    o1 = torch.full((count + 1,), float("nan"), dtype=torch.float64, device="cuda:0")
    fl = torch.full((count + 1,), -9, dtype=torch.int32, device="cuda:0")
    o0[count] = o1[count] = GUARD
    binding.check(lib.ste_probe_scalar_f64(op, count, a.data_ptr(), b.data_ptr(), o0.data_ptr(), o1.data_ptr(),
                                           fl.data_ptr(), None), "ste_probe_scalar_f64")
    torch.cuda.synchronize()
    o0, o1, fl = o0.cpu().numpy(), o1.cpu().numpy(), fl.cpu().numpy()
    assert o0[count] == GUARD and o1[count] == GUARD and fl[count] == -9, "probe wrote past its arrays"
    return o0[:count], o1[:count], fl[:count]


def run_mat4(op, A, V=None, scale=1.0):
    """One launch of a matrix op over A (count, 4, 4) and V (count, 4, 4; identity when None).  Returns
    (V (count, 4, 4), w (count, 4), out (count, 4, 4), status (count,))."""
    import torch
    from track_estimators._hip import binding

    lib = load()
    A = np.asarray(A, dtype=np.float64)
    count = A.shape[0]
    V = np.broadcast_to(np.eye(4), (count, 4, 4)) if V is None else np.asarray(V, dtype=np.float64)
    a = _up(A.reshape(count, 16).T)
    v = _up(V.reshape(count, 16).T)
    w = torch.full((4 * count + 1,), GUARD, dtype=torch.float64, device="cuda:0")
    o = torch.full((16 * count + 1,), GUARD, dtype=torch.float64, device="cuda:0")
    st = torch.full((count + 1,), -9, dtype=torch.int32, device="cuda:0")
    binding.check(lib.ste_probe_mat4_f64(op, count, a.data_ptr(), v.data_ptr(), w.data_ptr(), o.data_ptr(),
                                         C.c_double(scale), st.data_ptr(), None), "ste_probe_mat4_f64")
    torch.cuda.synchronize()
    w, o, st, v = w.cpu().numpy(), o.cpu().numpy(), st.cpu().numpy(), v.cpu().numpy()
    assert w[-1] == GUARD and o[-1] == GUARD and st[-1] == -9, "probe wrote past its arrays"
    return (v.T.reshape(count, 4, 4).copy(), w[:-1].reshape(4, count).T.copy(), o[:-1].reshape(16, count).T.reshape(count, 4, 4).copy(),
            st[:-1].copy())
