"""The device against an extended-precision solve (oracle/exact_kriging.py) with a bar per case:

    |dz|       <= C u (cond_1(A) + M) max|v|
    |dsigma^2| <= C u (cond_1(A) + M) max|b|      (u = 2^-53; max|b| = the largest variogram value on the point's right-hand side)

each capped at the absolute bar of the float64 parity tests (1e-8 / 1e-6, scaled by max(1, max|z|) / max(1, max|sigma^2|)).  The
float64 parity tests compare against a float64 oracle, so their bars must cover the errors of both sides; this one is held to the
device's own.  A defect that moves results by 1e-9 (a wrong polynomial coefficient of exp_neg_lean, a station just inside the
spherical range dropped by k_sp_cand, a gamma off by 1e-9 relative in k_rhs) fails here and passes the parity bars.

The case matrix (tests/_error_cases.py): the dense path across the 16- and 128-wide tiles, launch chunks and the factor /
symmetric / tri options; values, sills and coordinates far from order 1 through the dense, range-aware and moving-window paths;
stations just inside the spherical range, points with none, geographic problems across the antimeridian and at the poles; the
moving window's four solvers, each asserted through timing()["mw_kernel"] -- windows on both sides of every LDL^T class of
mw_chol_class (k_mw_chol); of the six pivoting classes of dispatch_mw_solve (k_mw_solve: nb = K + 1 <= 16, 32, 48, 64, 96, 128), of
its hand-off to k_mw_solve_big at K = 127 | 128 and of that kernel's 256-thread row strides at nb = 256 | 257; on the 64-wide panel
edges of k_mw_chol_blocked (K = 64 | 65, 128 | 129, 320 | 321, 384 | 385), with a single panel, a mostly padded last panel and the
shift of the unbounded models; 3-D and geographic station set-ups through each; custom variograms (the K x K table gtab) through
the class API into both pivoting solvers; the exact-hit rule; every execute fixture of tests/golden.  The CPU side (tests/test_exact_reference.py) checks the exact reference against mpmath and shows that the float64
oracle meets the same bar on every case."""
import collections

import numpy as np
import pytest

from tests import _error_cases as ec
from tests import _fixtures as fx

pytestmark = pytest.mark.gpu

_WORST = collections.defaultdict(list)  # group -> [(ratio z, ratio ss, cond, how many times tighter than today's bar, name)]


def _run_handle(c):
    from pykrige_amd import _lib

    st = c["st"]
    h = _lib.Handle(0)
    for k, v in c["opts"].items():
        h.set_option(k, v)
    h.set_problem(ndim=st.ndim, xs=st.coords_adj[:, 0], ys=st.coords_adj[:, 1], zs=st.coords_adj[:, 2] if st.ndim == 3 else None,
                  values=st.values, model_id=_lib.MODEL_IDS[st.model], params=st.params, exact_values=st.exact_values,
                  regional_linear=st.regional_linear, wells=st.wells_adj, geographic=st.geographic)
    p = c["pts"]
    h.set_points(p[:, 0], p[:, 1], p[:, 2] if st.ndim == 3 else None)
    if c["k"] is None:
        h.factor()
        h.predict()
    else:
        h.predict_moving_window(c["k"])
    z, ss = h.get_results()
    t = h.timing()
    z, ss = np.array(z), np.array(ss)
    h.close()
    return z, ss, t


def _run_golden(c):
    g = fx.load(c["golden"])
    m = fx.amd_model_from(c["golden"], g)
    kw = {"specified_drift_arrays": [g["spec_grid"]]} if "spec_grid" in g else {}
    z, ss = m.execute("grid", *fx.grid_args(g), backend="vectorized", **kw)
    return np.ma.getdata(z).ravel()[c["sel"]], np.ma.getdata(ss).ravel()[c["sel"]], m.last_timing


def _check(c, z, ss):
    rz, rs, r, (bz, bs) = ec.ratios(c, z, ss)
    today = min(1e-8 * max(1.0, float(np.abs(r.z).max())) / float(bz.max()),
                1e-6 * max(1.0, float(np.abs(r.ss).max())) / float(bs.max()))
    _WORST[c["group"]].append((rz, rs, float(r.cond.max()), today, c["name"]))
    assert rz <= 1.0 and rs <= 1.0, "%s/%s: |dz| / bar = %.3g, |dss| / bar = %.3g (cond_1 %.3g, C = %g)" % (
        c["group"], c["name"], rz, rs, float(r.cond.max()), ec.C_BAR)


@pytest.mark.parametrize("cid", ec.ids())
def test_device_within_the_extended_precision_bar(cid):
    """Regression notes: no case has failed on the device.  First MI355X run at C = 8: worst err / bar 0.52 (sigma^2, dense linear
    model, N = 257, one point, chunk 128), i.e. an error of 4.1 u (cond_1 + M) max|b|; every other group below 0.4.
    First run of the groups of the pivoting and blocked moving-window solvers (same bar): every case ran the solver it names and none
    was redone with pivoting; worst err / bar of mw_piv 0.077 (sigma^2; z 0.029: hole_k2, cond_1 15.7 -- the 3 x 3 system, where the
    bar is 8 u (15.7 + 3)); of mw_blocked 0.005 (sigma^2; z 0.001: class1_k8_spherical); of the
    custom variograms through the class API 0.001.  No kernel defect found."""
    c = ec.case(cid)
    if c["group"] == "golden":
        z, ss, t = _run_golden(c)
    else:
        z, ss, t = _run_handle(c)
    if c["sparse"] is not None:
        assert t["sparse"] == c["sparse"], t  # the range-aware path was (not) taken, as the case intends
    if c.get("mw_kernel") is not None:
        assert t["mw_kernel"] == c["mw_kernel"], t  # the solver the case is meant for (2 or 3 in place of 1 or 4: redone with pivoting)
    _check(c, z, ss)


@pytest.mark.parametrize("k", sorted(ec.CUSTOM_KS))
def test_custom_variogram_within_the_extended_precision_bar(k):
    """A custom variogram -- the reference's exponential model written out as a Python callable -- through OrdinaryKriging.execute
    with n_closest_points: its K x K table gtab enters k_mw_solve (K = 31 | 32, the nb <= 32 class limit) and k_mw_solve_big
    (K = 130).  Held to the exact reference of the NAMED model on the object's own adjusted coordinates, same bar."""
    import pykrige_amd as pa

    c, v, p = ec.custom_problem(k)
    m = pa.OrdinaryKriging(c[:, 0], c[:, 1], v, variogram_model="custom", variogram_parameters=list(ec.USER["exponential"]),
                           variogram_function=ec.custom_exponential)
    z, ss = m.execute("points", p[:, 0], p[:, 1], backend="loop", n_closest_points=k)
    assert m.last_timing["mw_kernel"] == ec.CUSTOM_KS[k], m.last_timing
    _check(ec.custom_state(k, m.X_ADJUSTED, m.Y_ADJUSTED), np.ma.getdata(z).ravel(), np.ma.getdata(ss).ravel())


def test_zz_worst_ratio_per_group():
    """Prints each group's worst err / bar, the cond_1 of that case, and how many times tighter the effective bar was than the
    float64 parity tests' (the median over the group's cases)."""
    if not _WORST:
        pytest.skip("runs after the cases")
    print("\nextended-precision bars, C = %g (u = 2^-53):" % ec.C_BAR)
    for g, rows in _WORST.items():
        wz = max(rows, key=lambda r: r[0])
        ws = max(rows, key=lambda r: r[1])
        print("  %-10s %3d cases  worst z %.3f (%s, cond %.2e)  worst ss %.3f (%s, cond %.2e)  bar tighter than today's: median %.1e, min %.1e"
              % (g, len(rows), wz[0], wz[4], wz[2], ws[1], ws[4], ws[2], float(np.median([r[3] for r in rows])),
                 min(r[3] for r in rows)))
    worst = max(max(r[0], r[1]) for rows in _WORST.values() for r in rows)
    print("  overall worst err / bar: %.3f" % worst)
    assert worst <= 1.0
