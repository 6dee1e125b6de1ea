"""cross_validate_window() on the device: station i kriged from its k nearest OTHER stations (mik_cross_validate_window).

Every case of tests/_cvw_cases.py is held, over all N stations, to the bar of the moving-window kernels -- C u (cond_1 + k + 1) max|v| on z
and C u (cond_1 + k + 1) max|b| on sigma^2 with cond_1 of each station's local system, C = 8 -- against the brute-force extended-precision
reference, and asserts the solver that ran.  The bit-for-bit checks tie the call to the moving window of the problem without station i, the
fields to the one-field call, and show that the call and the existing ones leave each other's results alone."""
import numpy as np
import pytest

from pykrige_amd import _lib
from tests import _cv_cases as cv
from tests import _cvw_cases as cw
from tests._error_cases import C_BAR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(cw.CASES))
def test_every_station_is_within_the_bar_of_its_local_system(name):
    obj, st, k, kernel = cw.case(name)
    ref = cw.reference(name)
    zhat, ss = obj.cross_validate_window(k)
    assert zhat.shape == (st.n,) and ss.shape == (st.n,) and zhat.dtype == np.float64 and ss.dtype == np.float64
    rz, rs = cv.ratios(ref, zhat, ss, C_BAR)
    print("%s: N %d k %d  mw_kernel %d  worst cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (
        name, st.n, k, obj.last_timing["mw_kernel"], float(ref.cond.max()), rz, rs))
    assert obj.last_timing["mw_kernel"] == kernel, (name, obj.last_timing["mw_kernel"])
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)


@pytest.mark.parametrize("name", ["pair_exact_k8", "pair_inexact_k8"])
def test_a_coincident_station_stays_in_the_window(name):
    """The reference decides what the two stations of the pair return; with exact_values it is the partner's value and sigma^2 = 0 -- which a
    search that left the query out by distance 0 could not give (it would drop the partner too)."""
    obj, st, k, _ = cw.case(name)
    ref = cw.reference(name)
    a, b = cw.PAIR
    assert np.array_equal(st.coords_adj[a], st.coords_adj[b]) and st.values[a] != st.values[b]
    zhat, ss = obj.cross_validate_window(k)
    bz, bs = cw.ek.bars(ref, C_BAR)
    for i, j in ((a, b), (b, a)):
        if st.exact_values:
            assert abs(float(ref.z[i]) - st.values[j]) <= 1e-15 and abs(float(ref.ss[i])) <= 1e-15, (i, ref.z[i], ref.ss[i])
        assert abs(zhat[i] - float(ref.z[i])) <= bz[i] and abs(ss[i] - float(ref.ss[i])) <= bs[i], (i, zhat[i], ss[i])
    if st.exact_values:
        assert abs(zhat[a] - st.values[b]) <= bz[a] and abs(zhat[b] - st.values[a]) <= bz[b]
    else:
        assert abs(float(ref.z[a]) - st.values[b]) > 1e-3  # without exact_values the nugget keeps the answer off the partner's value


def _handle_without(obj, i, k):
    """The handle-level moving window of the problem without station i, at station i's adjusted coordinates: (z, sigma^2)."""
    ca = np.array(obj._coords_adj, dtype=np.float64)
    keep = np.delete(np.arange(ca.shape[0]), i)
    nd = obj._ndim
    h = _lib.Handle()
    try:
        h.set_problem(ndim=nd, xs=ca[keep, 0], ys=ca[keep, 1], zs=ca[keep, 2] if nd == 3 else None, values=np.asarray(obj._values())[keep],
                      model_id=_lib.MODEL_IDS[obj.variogram_model], params=obj.variogram_model_parameters, eps=obj.eps,
                      exact_values=obj.exact_values)
        h.set_points(ca[i:i + 1, 0], ca[i:i + 1, 1], ca[i:i + 1, 2] if nd == 3 else None)
        h.predict_moving_window(k)
        z, ss = h.get_results()
        return float(z[0]), float(ss[0])
    finally:
        h.close()


@pytest.mark.parametrize("name", ["exponential_n300_k10", "ok3d_exponential_aniso_n400_k24"])
def test_entry_i_is_bit_for_bit_the_moving_window_without_station_i(name):
    obj, st, k, _ = cw.case(name)
    zhat, ss = obj.cross_validate_window(k)
    for i in (0, 1, st.n // 3, st.n // 2 + 1, st.n - 1):
        z1, s1 = _handle_without(obj, i, k)
        assert zhat[i] == z1 and ss[i] == s1, (name, i, zhat[i], z1, ss[i], s1)


def test_nine_fields_cross_the_row_groups_with_the_bits_of_the_one_field_call():
    obj, st, k, _ = cw.case("exponential_n300_k10")  # class {4, 4}: G - 2 = 2 value rows per pass
    rng = np.random.default_rng(5)
    v = np.concatenate([st.values[:, None], rng.standard_normal((st.n, 8))], axis=1)
    z0, s0 = obj.cross_validate_window(k)
    zf, sf = obj.cross_validate_window(k, values=v)
    assert zf.shape == (9, st.n) and sf.shape == (st.n,)
    assert np.array_equal(sf, s0) and np.array_equal(zf[0], z0)
    for f in range(9):
        z1, s1 = obj.cross_validate_window(k, values=v[:, f])
        assert z1.shape == (st.n,) and np.array_equal(z1, zf[f]) and np.array_equal(s1, s0), f
    # the solvers that take one field per launch: the pivoting Gauss-Jordan
    objh, sth, kh, _ = cw.case("hole_effect_n200_k20")
    vh = np.concatenate([sth.values[:, None], rng.standard_normal((sth.n, 2))], axis=1)
    zh0, sh0 = objh.cross_validate_window(kh)
    zhf, shf = objh.cross_validate_window(kh, values=vh)
    assert np.array_equal(zhf[0], zh0) and np.array_equal(shf, sh0)
    assert np.array_equal(objh.cross_validate_window(kh, values=vh[:, 2])[0], zhf[2])


def test_the_other_calls_and_the_windowed_form_leave_each_other_alone():
    obj, st, k, _ = cw.case("exponential_n300_k10")
    gx, gy = np.linspace(0.0, 1.0, 23), np.linspace(0.0, 1.0, 17)
    px, py = np.random.default_rng(9).random((2, 500))

    def others():
        return (obj.execute("grid", gx, gy), obj.execute("points", px, py, n_closest_points=10, backend="loop"), obj.cross_validate())

    before = others()
    w0 = obj.cross_validate_window(k)
    after = others()
    for (a0, a1), (b0, b1) in zip(before, after):
        assert np.array_equal(np.asarray(a0), np.asarray(b0)) and np.array_equal(np.asarray(a1), np.asarray(b1))
    w1 = obj.cross_validate_window(k)
    assert np.array_equal(w0[0], w1[0]) and np.array_equal(w0[1], w1[1])
    # straight after a dense execute (factor resident) and straight after a windowed execute (no factor)
    obj.execute("grid", gx, gy)
    w2 = obj.cross_validate_window(k)
    obj.execute("points", px, py, n_closest_points=10, backend="loop")
    w3 = obj.cross_validate_window(k)
    for w in (w2, w3):
        assert np.array_equal(w0[0], w[0]) and np.array_equal(w0[1], w[1])


def test_handle_level_results_and_points_of_an_earlier_predict_stay():
    obj, st, k, _ = cw.case("exponential_n300_k10")
    ca = np.array(obj._coords_adj, dtype=np.float64)
    px, py = np.random.default_rng(10).random((2, 700))
    kw = dict(ndim=2, xs=ca[:, 0], ys=ca[:, 1], zs=None, values=st.values, model_id=_lib.MODEL_IDS[obj.variogram_model],
              params=obj.variogram_model_parameters, eps=obj.eps, exact_values=obj.exact_values)
    h, g = _lib.Handle(), _lib.Handle()
    try:
        for x in (h, g):
            x.set_problem(**kw)
            x.set_points(px, py)
            x.predict_moving_window(k)
        z0, s0 = (np.array(a) for a in g.get_results())
        zw, sw = h.cross_validate_window(k)
        assert h.timing()["mw_kernel"] == 1
        z1, s1 = h.get_results()  # the earlier predict's, not the cross-validation's
        assert np.array_equal(z1, z0) and np.array_equal(s1, s0)
        zo, so = obj.cross_validate_window(k)
        assert zw.shape == (1, st.n) and np.array_equal(zw[0], zo) and np.array_equal(sw, so)
        # the resident points are still there: a dense predict needs no new set_points
        for x in (g, h):
            x.factor()
            x.predict()
        zd, sd = h.get_results()
        zg, sg = g.get_results()
        assert zd.shape == (700,) and np.array_equal(zd, zg) and np.array_equal(sd, sg)
    finally:
        h.close()
        g.close()


def test_window_limits_on_the_device():
    obj, st, _, _ = cw.case("exponential_n12_k11")
    with pytest.raises(ValueError, match="other stations"):
        obj.cross_validate_window(12)
    h = obj._get_handle()
    obj._set_problem(h)
    with pytest.raises(ValueError, match="OTHER stations"):
        h.cross_validate_window(12)  # k = N
    with pytest.raises(ValueError, match="at least two"):
        h.cross_validate_window(1)
    zhat, ss = h.cross_validate_window(11)
    assert zhat.shape == (1, 12) and np.all(np.isfinite(zhat)) and np.all(np.isfinite(ss))
    # a window beyond the neighbour search in LDS is refused, and the message names the global form
    big, _ = cw.station_set("ok2d_exponential_n300")
    hb = _lib.Handle()
    try:
        ca = np.array(big._coords_adj, dtype=np.float64)
        hb.set_problem(ndim=2, xs=ca[:, 0], ys=ca[:, 1], zs=None, values=np.asarray(big._values()), model_id=_lib.MODEL_IDS[big.variogram_model],
                       params=big.variogram_model_parameters, eps=big.eps, exact_values=big.exact_values)
        hb.set_option("mw_lds_cap", 512)  # K + 256 > 512 from K = 257 on
        with pytest.raises(ValueError, match="mik_cross_validate"):
            hb.cross_validate_window(257)
        hb.set_fields(np.zeros((2, 300)))
        hb.set_field_gaps(np.array([[True] * 299 + [False], [True] * 300]))
        with pytest.raises(ValueError, match="gaps"):
            hb.cross_validate_window(10)
    finally:
        hb.close()
