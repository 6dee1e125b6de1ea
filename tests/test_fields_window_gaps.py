"""execute_fields_window() on the device: value fields with missing stations through the moving window (mik_predict_window_gaps).

Every case of tests/_fwg_cases.py is held, over all points of all fields, to the bar of the moving-window kernels -- C u (cond_1 + k + 1)
max|v| on z and C u (cond_1 + k + 1) max|b| on sigma^2 with cond_1 of each point's local system, C = 8 -- against the brute-force
extended-precision reference on the state restricted to the field's stations, and asserts the solver that ran.  The bit-for-bit checks tie a
plane to the moving window of the problem of its valid stations alone, the fields of a pattern to the one-field call, a pattern without a gap
to execute_fields(..., n_closest_points=k), and show that the call and the existing ones leave each other's results alone."""
import numpy as np
import pytest

from pykrige_amd import _lib
from tests import _cv_cases as cv
from tests import _fwg_cases as fw
from tests._error_cases import C_BAR
from tests.test_fields_gaps_host import adjusted

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(fw.CASES))
def test_every_point_of_every_field_is_within_the_bar_of_its_local_system(name):
    d, k, kernel = fw.case(name)
    refs = fw.reference(name)
    z, ss = fw.call(d, k)
    nf, npt = d.valid.shape[1], d.pts.shape[0]
    assert z.shape == (nf, npt) and ss.shape == (nf, npt) and z.dtype == np.float64 and ss.dtype == np.float64
    assert type(z) is np.ndarray and type(ss) is np.ndarray
    worst = []
    for f, ref in enumerate(refs):
        rz, rs = cv.ratios(ref, z[f], ss[f], C_BAR)
        print("%s field %d: N %d (%d valid) k %d  mw_kernel %d  worst cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (
            name, f, d.st.n, int(d.valid[:, f].sum()), k, d.obj.last_timing["mw_kernel"], float(ref.cond.max()), rz, rs))
        worst.append((rz, rs))
    assert d.obj.last_timing["mw_kernel"] == kernel, (name, d.obj.last_timing["mw_kernel"])
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(ss))  # no ignored value (NaN) reached a result
    for f, (rz, rs) in enumerate(worst):
        assert rz <= 1.0 and rs <= 1.0, (name, f, rz, rs)


def test_exactly_k_valid_stations_pass_and_one_fewer_is_refused():
    d, k, _ = fw.case("exponential_n12_k8")
    assert int(d.valid[:, 0].sum()) == k
    valid = d.valid.copy()
    valid[np.flatnonzero(valid[:, 0])[0], 0] = False  # five missing
    with pytest.raises(ValueError, match="field 0"):
        fw.call(d, k, valid=valid)
    h = d.obj._get_handle()  # ... and by the library itself
    h.set_fields(np.nan_to_num(d.values).T)
    try:
        with pytest.raises(ValueError, match="mik_predict_window_gaps: field 0 has 7 valid"):
            h.predict_window_gaps(k, valid.T)
    finally:
        h.set_fields(None)


def test_a_coincident_partner_answers_and_a_missing_station_does_not():
    d, k, _ = fw.case("pair_exact_k8")
    ref = fw.reference("pair_exact_k8")[0]
    a, b = fw.cw.PAIR
    assert np.array_equal(d.st.coords_adj[a], d.st.coords_adj[b]) and d.valid[a, 0] and not d.valid[b, 0]
    z, ss = fw.call(d, k)
    bz, bs = fw.ek.bars(ref, C_BAR)
    npt = d.pts.shape[0]
    at_pair = [i for i in range(npt - 6, npt) if np.array_equal(d.pts[i], d.st.coords_orig[a])]
    assert len(at_pair) == 3  # the query on the valid partner and the two on the missing one
    for i in at_pair:
        assert abs(float(ref.z[i]) - d.st.values[a]) <= 1e-15 and abs(float(ref.ss[i])) <= 1e-15
        assert abs(z[0, i] - d.st.values[a]) <= bz[i] and abs(ss[0, i]) <= bs[i], (i, z[0, i], ss[0, i])
    i5 = npt - 3  # the query on missing station 5: not that station's value, and a positive variance
    assert d.on_missing[0] == 5 and np.array_equal(d.pts[i5], d.st.coords_orig[5])
    assert abs(z[0, i5] - d.st.values[5]) > 1e-3 and ss[0, i5] > 1e-3
    assert abs(z[0, i5] - float(ref.z[i5])) <= bz[i5]


def test_style_grid_on_23_by_17_axes():
    d, k, _ = fw.case("exponential_n300_k10")
    gx, gy = np.linspace(0.0, 1.0, 23), np.linspace(0.0, 1.0, 17)
    z, ss = fw.call(d, k, style="grid", axes=[gx, gy])
    assert z.shape == (3, 17, 23) and ss.shape == (3, 17, 23)
    mx, my = np.meshgrid(gx, gy)
    zp, sp = fw.call(d, k, axes=[mx.ravel(), my.ravel()])
    assert np.array_equal(z.reshape(3, -1), zp) and np.array_equal(ss.reshape(3, -1), sp)


def _handles(d, f, k):
    """Plane f at handle level and the handle of field f's valid stations alone, same adjusted coordinates, station order and points:
    ((z, sigma^2) of plane f, (z, sigma^2) of the subset handle)."""
    obj, st = d.obj, d.st
    ca, pa_ = np.array(obj._coords_adj, dtype=np.float64), adjusted(st, d.pts)
    nd = obj._ndim
    keep = d.valid[:, f]
    kw = dict(ndim=nd, model_id=_lib.MODEL_IDS[obj.variogram_model], params=obj.variogram_model_parameters, eps=obj.eps,
              exact_values=obj.exact_values)
    pts = (pa_[:, 0], pa_[:, 1], pa_[:, 2] if nd == 3 else None)
    h, g = _lib.Handle(), _lib.Handle()
    try:
        h.set_problem(xs=ca[:, 0], ys=ca[:, 1], zs=ca[:, 2] if nd == 3 else None, values=st.values, **kw)
        h.set_points(*pts)
        h.set_fields(d.values.T)
        z, ss = h.predict_window_gaps(k, d.valid.T)
        g.set_problem(xs=ca[keep, 0], ys=ca[keep, 1], zs=ca[keep, 2] if nd == 3 else None, values=d.values[keep, f], **kw)
        g.set_points(*pts)
        g.predict_moving_window(k)
        zg, sg = g.get_results()
        return (z[f], ss[f]), (np.array(zg), np.array(sg))
    finally:
        h.close()
        g.close()


@pytest.mark.parametrize("name,f", [("exponential_n300_k10", 1), ("exponential_n300_k10", 2), ("hole_effect_n200_k20", 0),
                                    ("hole_effect_n200_k20", 1), ("ok3d_exponential_aniso_n400_k24", 0)])
def test_plane_f_is_bit_for_bit_the_moving_window_of_its_valid_stations_alone(name, f):
    d, k, _ = fw.case(name)
    assert not d.valid[:, f].all()
    (z, ss), (zg, sg) = _handles(d, f, k)
    assert np.array_equal(z, zg) and np.array_equal(ss, sg), (name, f, float(np.abs(z - zg).max()), float(np.abs(ss - sg).max()))


def test_nine_fields_in_three_patterns_cross_the_row_groups():
    d, k, _ = fw.case("exponential_n300_k10")  # class {4, 4}: G - 2 = 2 value rows per pass
    rng = np.random.default_rng(7)
    pat = np.array([0, 1, 2, 1, 1, 0, 2, 1, 1])  # 2, 5 and 2 fields: an odd pattern crosses the groups of two
    valid = d.valid[:, pat]
    v = rng.standard_normal((d.st.n, 9))
    v[~valid] = np.nan
    z, ss = fw.call(d, k, values=v, valid=valid)
    assert z.shape == (9, d.pts.shape[0])
    for f in range(9):
        z1, s1 = fw.call(d, k, values=v[:, f], valid=valid[:, f])
        assert z1.shape == (1, d.pts.shape[0]) and np.array_equal(z1[0], z[f]) and np.array_equal(s1[0], ss[f]), f
        assert np.array_equal(ss[f], ss[pat[f]]), f  # the fields of a pattern share their sigma^2 bits (fields 0, 1, 2 open the patterns)
    assert not np.array_equal(ss[0], ss[1]) and not np.array_equal(ss[1], ss[2])
    order = rng.permutation(9)
    zo, so = fw.call(d, k, values=v[:, order], valid=valid[:, order])
    assert np.array_equal(zo, z[order]) and np.array_equal(so, ss[order])
    # the solvers that take one field per launch: the pivoting Gauss-Jordan
    dh, kh, _ = fw.case("hole_effect_n200_k20")
    vh = rng.standard_normal((dh.st.n, 3))
    mh = dh.valid[:, [0, 1, 0]]
    vh[~mh] = np.nan
    zh, sh = fw.call(dh, kh, values=vh, valid=mh)
    assert np.array_equal(sh[0], sh[2])
    for f in range(3):
        z1, s1 = fw.call(dh, kh, values=vh[:, f], valid=mh[:, f])
        assert np.array_equal(z1[0], zh[f]) and np.array_equal(s1[0], sh[f]), f


@pytest.mark.parametrize("name", ["exponential_n300_k10", "ok3d_exponential_aniso_n400_k24", "exponential_n300_k257"])
def test_patterns_without_a_gap_are_execute_fields_with_a_window(name):
    d, k, _ = fw.case(name)
    v = np.random.default_rng(8).standard_normal((d.st.n, 3))
    axes = [d.pts[:, i] for i in range(d.st.ndim)]
    zf, s0 = d.obj.execute_fields("points", *axes, v, backend="loop", n_closest_points=k)
    for valid in (None, np.ones(v.shape, dtype=bool)):
        z, ss = fw.call(d, k, values=v, valid=valid)
        assert np.array_equal(z, zf)
        for f in range(3):
            assert np.array_equal(ss[f], s0), f


def test_the_other_calls_and_this_one_leave_each_other_alone():
    d, k, _ = fw.case("exponential_n300_k10")
    obj = d.obj
    gx, gy = np.linspace(0.0, 1.0, 23), np.linspace(0.0, 1.0, 17)
    px, py = np.random.default_rng(9).random((2, 500))
    vg = np.nan_to_num(d.values)

    def others():
        return (obj.execute("grid", gx, gy), obj.execute("points", px, py, n_closest_points=10, backend="loop"), obj.cross_validate(),
                obj.execute_fields("points", px, py, vg, valid=d.valid))

    before = others()
    w0 = fw.call(d, k)
    after = others()
    for (a0, a1), (b0, b1) in zip(before, after):
        assert np.array_equal(np.asarray(a0), np.asarray(b0)) and np.array_equal(np.asarray(a1), np.asarray(b1))
    w1 = fw.call(d, k)
    assert np.array_equal(w0[0], w1[0]) and np.array_equal(w0[1], w1[1])
    # straight after a dense execute (factor resident), a windowed execute (no factor) and the global gaps call
    for leave in (lambda: obj.execute("grid", gx, gy), lambda: obj.execute("points", px, py, n_closest_points=10, backend="loop"),
                  lambda: obj.execute_fields("points", px, py, vg, valid=d.valid)):
        leave()
        w = fw.call(d, k)
        assert np.array_equal(w0[0], w[0]) and np.array_equal(w0[1], w[1])


def test_refusals_of_the_library_come_before_any_launch():
    d, k, _ = fw.case("exponential_n300_k10")
    obj, st = d.obj, d.st
    ca = np.array(obj._coords_adj, dtype=np.float64)
    h = _lib.Handle()
    try:
        h.set_problem(ndim=2, xs=ca[:, 0], ys=ca[:, 1], zs=None, values=st.values, model_id=_lib.MODEL_IDS[obj.variogram_model],
                      params=obj.variogram_model_parameters, eps=obj.eps, exact_values=obj.exact_values)
        h.set_points(d.pts[:, 0], d.pts[:, 1])
        z, ss = h.predict_window_gaps(k)  # no fields: the problem's values, nf = 1
        h.predict_moving_window(k)
        z0, s0 = h.get_results()
        assert z.shape == (1, d.pts.shape[0]) and np.array_equal(z[0], z0) and np.array_equal(ss[0], s0)
        for bad in (1, st.n + 1):
            with pytest.raises(ValueError, match="n_closest_points"):
                h.predict_window_gaps(bad)
        h.set_option("mw_lds_cap", 512)  # K + 256 > 512 from K = 257 on
        with pytest.raises(ValueError, match="beyond the neighbour search in LDS"):
            h.predict_window_gaps(257)
        h.set_option("mw_lds_cap", 8192)
        h.set_fields(np.zeros((2, st.n)))
        h.set_field_gaps(np.array([[True] * (st.n - 1) + [False], [True] * st.n]))
        with pytest.raises(ValueError, match="mik_set_field_gaps"):
            h.predict_window_gaps(k)
        with pytest.raises(ValueError, match="gaps"):  # the old refusal stays
            h.predict_moving_window(k)
    finally:
        h.close()
    with pytest.raises(NotImplementedError, match="not built"):  # and so does execute_fields'
        obj.execute_fields("points", d.pts[:, 0], d.pts[:, 1], np.nan_to_num(d.values), backend="loop", n_closest_points=k, valid=d.valid)
