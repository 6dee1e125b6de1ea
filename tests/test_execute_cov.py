"""execute_cov on the device: the kriging error covariance between prediction points from the one resident inverse (mik_k_cov.h).

The reference is brute force in extended precision (tests/test_execute_cov_host.py: reference, cached per session): the right-hand sides
of ek.right_hand_sides solved by ek.refined_solve, d_pq from the same float64 distance functions, gamma* = 0 where d_pq <= ko.EPS.  The
bar of entry (p, q) is C_BAR u (cond_1(A) + M) max(bscale_p, bscale_q), capped at 1e-6 max(1, max|cov|).

Worst |err| / bar at P = 300 on an MI355X (the assertion is <= 1): geographic_ok_n50 0.023, ok2d_exponential_n67 0.031,
ok2d_spherical_n130_values_1e3 0.014, ok3d_gaussian_aniso_n40 0.015, uk2d_regional_linear_n67 0.023, uk3d_functional_n40 0.031; the
largest error of an entry is 4.3e-14.  Tile edges P = 1, 2, 127, 128, 129: 0.0023, 0.0056, 0.022, 0.022, 0.022."""
import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import _lib
from tests import _cv_cases as cv
from tests import test_execute_cov_host as ch

pytestmark = pytest.mark.gpu

EDGE = "ok2d_exponential_n67"


def _bits(a, b):
    a, b = np.ascontiguousarray(np.asarray(a), dtype=np.float64), np.ascontiguousarray(np.asarray(b), dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cols(pts):
    return tuple(np.ascontiguousarray(pts[:, k]) for k in range(pts.shape[1]))


# ------------------------------------------------------------------------------------------------------------- against brute force
@pytest.mark.parametrize("name", sorted(cv.GLOBAL))
def test_every_entry_is_inside_the_bar(name):
    """P = 300 (three point blocks; M = 131 of the spherical case gives Mp = 256, two station blocks), two points on one station, one
    on another, two pairs of coincident points.  Also: exact symmetry, the diagonal and z are execute()'s bits, the rows of the
    on-station points are zero to the bar, and the matrix is positive semidefinite to the bar."""
    m, st = cv.global_case(name)
    p = _cols(ch.points(name))
    z, cov = m.execute_cov("points", *p)
    # (a range-aware predict keeps its path, hence execute()'s bits; the panel of all right-hand sides is a dense pass of its own)
    assert m.last_timing["sparse"] == ("spherical" in name) and m.last_timing["contract_launches"] == 1
    assert isinstance(cov, np.ndarray) and not isinstance(cov, np.ma.MaskedArray)
    assert cov.shape == (ch.P_FULL, ch.P_FULL) and cov.dtype == np.float64 and cov.flags["C_CONTIGUOUS"]
    ratio, err = ch.worst_ratio(name, cov)
    print("%s: worst err / bar %.3g, max err %.3g" % (name, ratio, err))
    assert ratio <= 1.0, (name, ratio, err)
    assert np.array_equal(cov, cov.T)
    z0, s0 = m.execute("points", *p)
    assert type(z) is type(z0) and z.shape == z0.shape and _bits(z, z0)
    assert np.array_equal(np.diag(cov), np.asarray(s0))
    _, bar = ch.reference(name)
    assert st.exact_values
    for q in ch.ON_STATION:
        assert np.all(np.abs(cov[q]) <= bar[q]), q
    assert np.linalg.eigvalsh(cov).min() >= -ch.P_FULL * bar.max()


@pytest.mark.parametrize("npt", [1, 2, 127, 128, 129])
def test_tile_edges(npt):
    m, _ = cv.global_case(EDGE)
    p = tuple(c[:npt] for c in _cols(ch.points(EDGE)))
    z, cov = m.execute_cov("points", *p)
    assert cov.shape == (npt, npt) and z.shape == (npt,)
    ratio, err = ch.worst_ratio(EDGE, cov, npt)
    print("P = %d: worst err / bar %.3g, max err %.3g" % (npt, ratio, err))
    assert ratio <= 1.0, (npt, ratio, err)
    z0, s0 = m.execute("points", *p)
    assert np.array_equal(cov, cov.T) and np.array_equal(np.diag(cov), np.asarray(s0)) and _bits(z, z0)


# ------------------------------------------------------------------------------------------------------------- bits
def test_three_launches_give_the_bits_of_one():
    m, _ = cv.global_case(EDGE)
    p = _cols(ch.points(EDGE))
    z1, c1 = m.execute_cov("points", *p)
    assert m.last_timing["contract_launches"] == 1
    h = m._get_handle()
    h.set_option("chunk", 128)
    try:
        z3, c3 = m.execute_cov("points", *p)
        assert m.last_timing["contract_launches"] == 3
    finally:
        h.set_option("chunk", 131072)
    assert _bits(z3, z1) and _bits(c3, c1)


@pytest.mark.parametrize("name", ["ok2d_exponential_n67", "uk2d_regional_linear_n67", "ok3d_gaussian_aniso_n40", "geographic_ok_n50"])
def test_grid_is_points_on_the_meshgrid(name):
    m, st = cv.global_case(name)
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    axes = [np.linspace(lo[k], hi[k], n) for k, n in zip(range(st.ndim), (13, 11, 2))]
    zg, cg = m.execute_cov("grid", *axes)
    shape = tuple(a.size for a in reversed(axes))
    assert zg.shape == shape and cg.shape == (zg.size, zg.size)
    if st.ndim == 2:
        gx, gy = np.meshgrid(axes[0], axes[1])
        flat = (gx.ravel(), gy.ravel())
    else:
        gz, gy, gx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        flat = (gx.ravel(), gy.ravel(), gz.ravel())
    zp, cp = m.execute_cov("points", *flat)
    assert _bits(np.asarray(zg).ravel(), zp) and _bits(cg, cp)
    z0, s0 = m.execute("grid", *axes)
    assert type(zg) is type(z0) and _bits(zg, z0) and np.array_equal(np.diag(cg), np.asarray(s0).ravel())


def test_execute_and_execute_fields_keep_their_bits_after_execute_cov():
    m, st = cv.global_case(EDGE)
    p = _cols(ch.points(EDGE)[:130])
    rng = np.random.default_rng(7)
    values = st.values[:, None] * (1.0 + 0.25 * np.arange(3)) + 0.1 * rng.standard_normal((st.n, 3))
    valid = np.ones(values.shape, dtype=bool)
    valid[[3, 11, 40], 1] = valid[[3, 20], 2] = False
    z0, s0 = [np.array(a) for a in m.execute("points", *p)]
    f0, g0 = [np.array(a) for a in m.execute_fields("points", *p, values, valid=valid)]
    m.execute_cov("points", *p)
    z1, s1 = [np.array(a) for a in m.execute("points", *p)]
    f1, g1 = [np.array(a) for a in m.execute_fields("points", *p, values, valid=valid)]
    assert _bits(z0, z1) and _bits(s0, s1) and _bits(f0, f1) and _bits(g0, g1)


# ------------------------------------------------------------------------------------------------------------- refusals
def _resident(h, n=30, npt=10, **kw):
    rng = np.random.default_rng(3)
    x, y, v = rng.random(n), rng.random(n), rng.random(n)
    h.set_problem(2, x, y, None, v, _lib.MODEL_IDS["exponential"], [1.0, 0.5, 0.02], **kw)
    h.set_points(rng.random(npt), rng.random(npt))


def test_the_library_refuses_what_is_not_built():
    h = _lib.Handle(0)
    with pytest.raises(RuntimeError, match="set the problem first"):
        h.predict_cov()
    _resident(h, pseudo_inv=1)
    with pytest.raises(ValueError, match="pseudo_inv"):
        h.predict_cov()
    _resident(h)
    rng = np.random.default_rng(4)
    h.set_points(rng.random(10), rng.random(10), mask=np.arange(10) % 3 == 0)
    with pytest.raises(ValueError, match="masked"):
        h.predict_cov()
    h.set_points(np.zeros(0), np.zeros(0))
    with pytest.raises(ValueError, match="no points"):
        h.predict_cov()
    h.set_custom_variogram(lambda d: 0.1 + d)
    try:
        rng = np.random.default_rng(3)
        h.set_problem(2, rng.random(30), rng.random(30), None, rng.random(30), _lib.MODEL_IDS["custom"], [0.0, 0.0, 0.0])
        h.set_points(rng.random(10), rng.random(10))
        with pytest.raises(ValueError, match="custom variogram"):
            h.predict_cov()
    finally:
        h.set_custom_variogram(None)
    # the refusals leave the handle usable: the same handle computes a covariance, and factors by itself (no factor() above)
    _resident(h)
    cov = h.predict_cov()
    z, ss = h.get_results()
    assert cov.shape == (10, 10) and np.array_equal(cov, cov.T) and np.array_equal(np.diag(cov), ss) and np.all(np.isfinite(z))
    h.close()


def test_an_oversized_point_list_is_refused_with_nothing_launched():
    """400 000 points: C alone would be 1.28 TB.  The refusal names the largest number of points that fits, and that number is right: the
    library's own check (cov_out = NULL: nothing is launched) passes that many resident points and refuses one more."""
    h = _lib.Handle(0)
    npt = 400000
    _resident(h, npt=npt)
    with pytest.raises(ValueError, match=r"quarter of device memory; the largest number of points that fits is (\d+)") as e:
        h.predict_cov()
    z = np.empty(npt)
    with pytest.raises(RuntimeError, match="predict first"):  # nothing ran
        _lib.check(h._lib.mik_get_results(h._h, _lib._ptr(z), _lib._ptr(z)))
    fit = int(str(e.value).rsplit(" ", 1)[1])
    assert fit % 128 == 0 and 0 < fit < npt
    for n, rc in ((fit, _lib.MIK_OK), (fit + 1, _lib.MIK_EINVAL)):
        h.set_points(np.zeros(n), np.zeros(n))
        assert h._lib.mik_predict_cov(h._h, None) == rc, n
    h.close()


def test_a_device_group_is_refused():
    h = _lib.Handle(0)
    h.set_devices(2, alias=True)
    _resident(h)
    with pytest.raises(ValueError, match="device group"):
        h.predict_cov()
    m = pa.OrdinaryKriging(np.array([0.0, 1.0, 0.3]), np.array([0.0, 0.2, 0.9]), np.array([1.0, 2.0, 3.0]), variogram_model="linear",
                           variogram_parameters=[1.0, 0.1])
    m._handle = h
    try:
        with pytest.raises(ValueError, match="device group of 2"):
            m.execute_cov("points", np.array([0.5]), np.array([0.5]))
    finally:
        m._handle = None
        h.close()
