"""cross_validate on the device (include/mikrige.h: mik_cross_validate): leave-one-out kriging of every station from all other
stations, out of the resident inverse (the global form; the windowed form is not built and raises).

The reference is brute force in extended precision (tests/_cv_cases.py): station i kriged from the state without station i.  Bars:
C u (cond_1(A) + M) max|v| on z and C u (cond_1(A) + M) max|b| on sigma^2 with C = tests/_error_cases.C_BAR and A the full kriging
matrix."""
import numpy as np
import pytest

from tests import _cv_cases as cv

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------------------------------- global form
@pytest.mark.parametrize("name", sorted(cv.GLOBAL))
def test_global_form_against_brute_force(name):
    """Each case prints cond_1 of the full matrix and its worst err / bar on z and sigma^2 before it asserts (run with -s)."""
    m, st = cv.global_case(name)
    ref = cv.global_reference(name)
    if "spherical" in name:  # the factor must hold the stations in Hilbert-curve order: the results have to be un-permuted
        m.execute("points", st.coords_orig[:3, 0], st.coords_orig[:3, 1])
        assert m.last_timing["sparse"] == 1 and m.last_timing["stations_sorted"] == 1, m.last_timing
    zhat, ss = m.cross_validate()
    assert type(zhat) is np.ndarray and type(ss) is np.ndarray and zhat.dtype == ss.dtype == np.float64
    assert zhat.shape == ss.shape == (st.n,)
    rz, rs = cv.ratios(ref, zhat, ss)
    print("%s: cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (name, float(ref.cond[0]), rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)
    if "values_1e3" in name:
        assert float(np.abs(st.values).max()) > 500.0
    # the object's own values given explicitly: the same bits
    z1, s1 = m.cross_validate(st.values)
    assert _bits(z1, zhat) and _bits(s1, ss)


def _nine_fields(st):
    rng = np.random.default_rng(5)
    v = rng.standard_normal((st.n, 9))  # crosses MIK_FB = 8
    v[:, 0] = st.values
    return v


@pytest.mark.parametrize("name", ["ok2d_exponential_n67", "ok2d_spherical_n130_values_1e3", "uk3d_functional_n40"])
def test_global_fields_are_the_one_field_results_bit_for_bit(name):
    m, st = cv.global_case(name)
    v = _nine_fields(st)
    zf, ss = m.cross_validate(v)
    assert zf.shape == (9, st.n) and ss.shape == (st.n,) and type(zf) is np.ndarray
    z0, s0 = m.cross_validate()
    assert _bits(zf[0], z0) and _bits(ss, s0)
    for f in range(9):
        z1, s1 = m.cross_validate(v[:, f])
        assert z1.shape == (st.n,)
        assert _bits(zf[f], z1), f
        assert _bits(ss, s1), f
    z2, _ = m.cross_validate(v[:, :1])
    assert z2.shape == (1, st.n) and _bits(z2[0], z0)


# ------------------------------------------------------------------------------------------------------------- untouched paths
def test_execute_is_bit_identical_before_and_after_cross_validate():
    import pykrige_amd as pa

    rng = np.random.default_rng(1501)
    c = rng.random((150, 2))
    m = pa.OrdinaryKriging(c[:, 0], c[:, 1], cv._field(c), variogram_model="spherical", variogram_parameters=[1.0, 0.4, 0.02])
    gx, gy = np.linspace(0, 1, 23), np.linspace(0, 1, 19)
    px, py = rng.random(300), rng.random(300)

    def both():
        zg, sg = m.execute("grid", gx, gy)
        zp, sp = m.execute("points", px, py, n_closest_points=10, backend="loop")
        return [np.array(np.ma.getdata(a)) for a in (zg, sg, zp, sp)]

    before = both()
    z1, s1 = m.cross_validate()
    z3, s3 = m.cross_validate(rng.standard_normal((150, 3)))
    after = both()
    for a, b in zip(before, after):
        assert _bits(a, b)
    # and the other way round: cross_validate is not moved by the executes between its calls
    z1b, s1b = m.cross_validate()
    assert _bits(z1, z1b) and _bits(s1, s1b) and _bits(s1, s3)


def test_resident_points_and_results_survive_a_cross_validate_on_the_handle():
    """mik_cross_validate between mik_predict and mik_get_results, factoring by itself: the earlier results come back, and a second predict
    on the same resident points needs no mik_set_points."""
    from pykrige_amd import _lib

    m, st = cv.global_case("ok2d_exponential_n67")
    rng = np.random.default_rng(1601)
    p = rng.random((500, 2))
    k = 17
    h = _lib.Handle(0)
    try:
        h.set_problem(ndim=2, xs=st.coords_adj[:, 0], ys=st.coords_adj[:, 1], zs=None, values=st.values, model_id=_lib.MODEL_IDS[st.model],
                      params=st.params)
        h.set_points(p[:, 0], p[:, 1])
        h.predict_moving_window(k)
        z0, s0 = [np.array(a) for a in h.get_results()]
        h.predict_moving_window(k)
        zg, sg = h.cross_validate(0)  # factors by itself
        z1, s1 = [np.array(a) for a in h.get_results()]
        assert _bits(z0, z1) and _bits(s0, s1)
        h.predict()  # the factor the call left, the points set before
        zd, sd = [np.array(a) for a in h.get_results()]
        h.predict()
        zg2, sg2 = h.cross_validate(0)  # the resident factor
        zd2, sd2 = [np.array(a) for a in h.get_results()]
        assert zd.shape == (500,) and _bits(zd, zd2) and _bits(sd, sd2) and _bits(zg, zg2) and _bits(sg, sg2)
        zm, sm = m.cross_validate()
        assert _bits(zg[0], zm) and _bits(sg, sm)
        with pytest.raises(ValueError, match="global form"):
            h.cross_validate(k)  # the windowed form is not built: an error, no fall-back
    finally:
        h.close()


def test_windowed_form_is_an_error():
    m, st = cv.global_case("ok2d_exponential_n67")
    with pytest.raises(NotImplementedError, match="n_closest_points"):
        m.cross_validate(n_closest_points=10, backend="loop")
