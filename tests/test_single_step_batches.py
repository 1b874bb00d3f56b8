"""The one-step entry points ("one step, many filters") at count > 1.  Needs a real MI355X: run with ``pytest -m gpu``.

ste_ukf_predict_f64, ste_ukf_update_f64, ste_ukf_robust_terms_f64, ste_sigma_points_f64, ste_sigma_points_generic_f64 and
ste_geodetic_dynamics_f64 are documented for ``count`` independent elements, but the drop-in classes only ever call them with
count = 1: their [component][count] indexing, the per-element noise and status arrays and the tail of the grid had never
run.  Here they run at counts 1, 63, 64, 65 and 130 (under, on and over a wave; a tail of 2 lanes in a third wave) on a
batch whose elements all differ, with and without noise and status, with guarded output arrays, against the 50-digit
restatement of one UKF step (oracle/mp_reference.py).

Bound: 4 x (the float64 oracle's error against the same restatement on the same inputs) + 8 * 2^-52, in the project's
metrics (means element-wise relative, covariances per matrix); tests/test_mp_reference.py checks the oracle side on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

import single_step_cases as ss

pytestmark = pytest.mark.gpu

SENTINEL = -77
GUARD = -7.25


def _lib():
    from track_estimators._hip import binding

    return binding.require_gpu(), binding


def _up(a, count=None):
    """(count, ...) host array -> device [components][count], the first ``count`` elements"""
    import torch

    a = np.asarray(a, dtype=np.float64)
    a = a[:count] if count is not None else a
    return torch.from_numpy(np.ascontiguousarray(a.reshape(a.shape[0], -1).T)).to("cuda:0")


def _out(comps, count):
    import torch

    t = torch.full((comps * count + 1,), float("nan"), dtype=torch.float64, device="cuda:0")
    t[-1] = GUARD
    return t


def _status(count, want):
    import torch

    return torch.full((count + 1,), SENTINEL, dtype=torch.int32, device="cuda:0") if want else None


def _down(t, comps, count):
    import torch

    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert a[-1] == GUARD, "wrote past the end of an output array"
    return a[:-1].reshape(comps, count).T.copy()


def _down_status(st, count):
    if st is None:
        return None
    a = st.cpu().numpy()
    assert a[-1] == SENTINEL, "wrote past the end of status"
    return a[:count].copy()


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_predict(count, noise, status, P=None):
    lib, binding = _lib()
    b = ss.batch()
    x, Pd, dt, sr, cr = _up(b.x, count), _up(b.P if P is None else P, count), _up(b.dt, count), _up(b.sr, count), _up(b.cr, count)
    nz = _up(b.noise, count) if noise else None
    xo, Po, st = _out(4, count), _out(16, count), _status(count, status)
    binding.check(lib.ste_ukf_predict_f64(count, x.data_ptr(), Pd.data_ptr(), dt.data_ptr(), sr.data_ptr(), cr.data_ptr(), _ptr(nz),
                                          b.Q.ctypes.data, C.c_double(b.fan_scale), C.c_double(b.w0), C.c_double(b.wi),
                                          xo.data_ptr(), Po.data_ptr(), _ptr(st), None), "ste_ukf_predict_f64")
    return _down(xo, 4, count), _down(Po, 16, count).reshape(count, 4, 4), _down_status(st, count)


def run_update(route, count, noise, status, x=None, P=None, z=None):
    """noise=False passes NULL and the rounded sum z + noise as the observation: the same update, one array fewer"""
    lib, binding = _lib()
    b = ss.batch()
    zz = b.z[route] if z is None else z
    xd, Pd = _up(b.x if x is None else x, count), _up(b.P if P is None else P, count)
    zd = _up(zz if noise else zz + b.noise[:len(zz)], count)
    nz = _up(b.noise, count) if noise else None
    xo, Po, st = _out(4, count), _out(16, count), _status(count, status)
    binding.check(lib.ste_ukf_update_f64(count, xd.data_ptr(), Pd.data_ptr(), zd.data_ptr(), _ptr(nz), b.H[route].ctypes.data,
                                         b.R[route].ctypes.data, xo.data_ptr(), Po.data_ptr(), _ptr(st), None), "ste_ukf_update_f64")
    return _down(xo, 4, count), _down(Po, 16, count).reshape(count, 4, 4), _down_status(st, count)


@pytest.mark.parametrize("count", ss.COUNTS)
@pytest.mark.parametrize("noise,status", [(False, False), (True, True), (True, False), (False, True)],
                         ids=["plain", "noise+status", "noise", "status"])
def test_predict_batches(count, noise, status):
    x, P, st = run_predict(count, noise, status)
    rx, rP = ss.predict_reference(noise)
    o = ss.oracle_errors("block")
    key = "predict+noise" if noise else "predict"
    em, ec = ss.mean_err(x, rx[:count]), ss.cov_err(P, rP[:count])
    print(f"\n[single step] predict count={count} noise={noise}: mean {em:.3e} (oracle {o[key + ' mean']:.3e}), cov {ec:.3e} "
          f"(oracle {o[key + ' cov']:.3e})")
    assert em <= ss.bound(o[key + " mean"]) and ec <= ss.bound(o[key + " cov"])
    if status:
        assert (st == 0).all(), st


@pytest.mark.parametrize("route", ["block", "dense"])
@pytest.mark.parametrize("count", ss.COUNTS)
@pytest.mark.parametrize("noise,status", [(False, False), (True, True)], ids=["plain", "noise+status"])
def test_update_batches(route, count, noise, status):
    """H = diag(1, 1, 0, 0) with a block R takes the closed-form 2 x 2 pseudo-inverse, a dense H and R the 4 x 4 route."""
    x, P, st = run_update(route, count, noise, status)
    rx, rP, _, _ = ss.update_reference(route)
    o = ss.oracle_errors(route)
    em, ec = ss.mean_err(x, rx[:count]), ss.cov_err(P, rP[:count])
    print(f"\n[single step] update {route} count={count} noise={noise}: mean {em:.3e} (oracle {o['update mean']:.3e}), cov {ec:.3e} "
          f"(oracle {o['update cov']:.3e})")
    assert em <= ss.bound(o["update mean"]) and ec <= ss.bound(o["update cov"])
    if status:
        assert (st == 0).all(), st


def run_robust(route, count, P=None):
    lib, binding = _lib()
    b = ss.batch()
    x, Pd, z = _up(b.x, count), _up(b.P if P is None else P, count), _up(b.z[route], count)
    g, d = _out(1, count), _out(1, count)
    binding.check(lib.ste_ukf_robust_terms_f64(count, x.data_ptr(), Pd.data_ptr(), z.data_ptr(), b.H[route].ctypes.data,
                                               b.R[route].ctypes.data, g.data_ptr(), d.data_ptr(), None), "ste_ukf_robust_terms_f64")
    return _down(g, 1, count)[:, 0], _down(d, 1, count)[:, 0]


@pytest.mark.parametrize("route", ["block", "dense"])
@pytest.mark.parametrize("count", ss.COUNTS)
def test_robust_terms_batches(route, count):
    g, d = run_robust(route, count)
    _, _, rg, rd = ss.update_reference(route)
    o = ss.oracle_errors(route)
    eg, ed = ss.mean_err(g, rg[:count]), ss.mean_err(d, rd[:count])
    print(f"\n[single step] robust terms {route} count={count}: gamma {eg:.3e} (oracle {o['gamma']:.3e}), denom {ed:.3e} "
          f"(oracle {o['denom']:.3e})")
    assert eg <= ss.bound(o["gamma"]) and ed <= ss.bound(o["denom"])


@pytest.mark.parametrize("route", ["block", "dense"])
def test_robust_terms_one_nan_element_is_alone(route):
    """The robust terms have no status array, so what there is to hold is that the other elements come out bit for bit
    unchanged.  (The element itself reports gamma = denom = 0: every eigenvalue of its S is NaN, and the pseudo-inverse
    keeps none of them.  The update that follows such a criterion spreads the NaN and sets STE_STATUS_NAN, see above.)"""
    b = ss.batch()
    bad = 70
    Pn = b.P.copy()
    Pn[bad, 0, 1] = Pn[bad, 1, 0] = np.nan
    clean, dirty = run_robust(route, 130), run_robust(route, 130, P=Pn)
    others = np.arange(130) != bad
    for k in (0, 1):
        assert np.array_equal(clean[k][others], dirty[k][others])


@pytest.mark.parametrize("which", ["predict", "update block", "update dense"])
def test_one_nan_element_is_flagged_and_alone(which):
    """One element of a 130-element batch gets a NaN in P: its status carries STE_STATUS_NAN, and every other element comes out
    bit for bit as from the same batch without it (a lane's arithmetic does not depend on its wave-mates' data)."""
    b = ss.batch()
    bad = 70
    Pn = b.P.copy()
    Pn[bad, 1, 2] = Pn[bad, 2, 1] = np.nan
    if which == "predict":
        clean, dirty = run_predict(130, True, True), run_predict(130, True, True, P=Pn)
    else:
        route = which.split()[1]
        clean, dirty = run_update(route, 130, True, True), run_update(route, 130, True, True, P=Pn)
    others = np.arange(130) != bad
    assert (dirty[2][bad] & 0x1) and (dirty[2][others] == 0).all() and (clean[2] == 0).all()
    for k in (0, 1):
        assert np.array_equal(clean[k][others], dirty[k][others])
        # the update spreads the NaN over its outputs; the predict's eigen-solve can swallow one that sits off the diagonal
        # (a rotation with a NaN pivot is skipped), which is why ste_ukf_predict_f64 also looks at its inputs
        assert which == "predict" or np.isnan(dirty[k][bad]).any()


def test_update_of_a_heading_just_below_zero():
    """x[3] = -1e-20 with P = 0: the gain is zero, the state passes through, and the heading is NumPy's -1e-20 % 360 = 360.0
    (a + 360 rounds to 360.0).  floored_mod360 used to return -1e-20 here."""
    b = ss.batch()
    x = b.x[:3].copy()
    x[1, 3] = -1e-20
    x, P, st = run_update("block", 3, True, True, x=x, P=np.zeros((3, 4, 4)), z=b.z["block"][:3])
    assert x[1, 3] == 360.0 == float(np.mod(-1e-20, 360.0))
    assert np.array_equal(x[[0, 2]], b.x[[0, 2]]) and (P == 0).all() and (st == 0).all()


@pytest.mark.parametrize("count", ss.COUNTS)
def test_geodetic_dynamics_batches(count):
    lib, binding = _lib()
    b = ss.batch()
    x, dt, sr, cr = _up(b.x, count), _up(b.dt, count), _up(b.sr, count), _up(b.cr, count)
    out = _out(4, count)
    binding.check(lib.ste_geodetic_dynamics_f64(count, x.data_ptr(), dt.data_ptr(), sr.data_ptr(), cr.data_ptr(), out.data_ptr(), None),
                  "ste_geodetic_dynamics_f64")
    got = _down(out, 4, count)
    o = ss.oracle_errors("block")
    e = ss.mean_err(got, ss.geodetic_reference()[:count])
    print(f"\n[single step] geodetic count={count}: {e:.3e} (oracle {o['geodetic']:.3e})")
    assert e <= ss.bound(o["geodetic"])


@pytest.mark.parametrize("count", ss.COUNTS)
def test_sigma_points_batches(count):
    lib, binding = _lib()
    b = ss.batch()
    x, P = _up(b.x, count), _up(b.P, count)
    out = _out(36, count)
    binding.check(lib.ste_sigma_points_f64(count, x.data_ptr(), P.data_ptr(), C.c_double(b.fan_scale), out.data_ptr(), None),
                  "ste_sigma_points_f64")
    got = _down(out, 36, count).reshape(count, 9, 4)
    o = ss.oracle_errors("block")
    e = ss.cov_err(got, ss.sigma4_reference()[:count])
    print(f"\n[single step] sigma fan count={count}: {e:.3e} (oracle {o['sigma fan']:.3e})")
    assert e <= ss.bound(o["sigma fan"])


@pytest.mark.parametrize("n", [1, 2, 4, 7, 16])
@pytest.mark.parametrize("count", ss.COUNTS)
def test_sigma_points_generic_batches(n, count):
    """The general-dimension fan.  Against the 50-digit fan on every element for n <= 4 and, for n = 7 and 16 (whose 50-digit
    eigen-decompositions cost 20 to 150 ms each), on the elements either side of the wave boundaries -- the lanes a wrong
    stride or a missed tail shows on; the kernel runs the same code on every lane.  Every element is also held to the float64
    oracle at 1e-9 per fan, which a misplaced element (an O(1) error) cannot pass."""
    lib, binding = _lib()
    b = ss.batch()
    xs, Ps = b.gen[n]
    x, P = _up(xs, count), _up(Ps, count)
    m = 2 * n + 1
    out = _out(m * n, count)
    binding.check(lib.ste_sigma_points_generic_f64(n, count, x.data_ptr(), P.data_ptr(), C.c_double(b.gen_scale), out.data_ptr(), None),
                  "ste_sigma_points_generic_f64")
    got = _down(out, m * n, count).reshape(count, m, n)
    ref = ss.sigma_reference(n)
    o = ss.oracle_errors("block")["sigma n=%d" % n]
    rows = [i for i in ref if i < count]
    e = max(ss.cov_err(got[i][None], ref[i][None]) for i in rows)
    print(f"\n[single step] generic fan n={n} count={count}: {e:.3e} over {len(rows)} elements (oracle {o:.3e})")
    assert e <= ss.bound(o)
    every = max(ss.cov_err(got[i][None], ss.oracle_sigma(xs[i], Ps[i], b.gen_scale)[None]) for i in range(count))
    assert every <= 1e-9
