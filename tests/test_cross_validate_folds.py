"""cross_validate(folds=...) on the device (include/mikrige.h: mik_cross_validate_folds): k-fold and leave-group-out kriging of every
fold from the stations outside it, out of the resident inverse.

The reference is brute force in extended precision (tests/test_cross_validate_folds_host.py): the fold's stations kriged from the state
without the fold.  Bars as tests/test_cross_validate.py: C u (cond_1(A) + M) max|v| on z and C u (cond_1(A) + M) max|b| on sigma^2 with
C = tests/_error_cases.C_BAR and A the full kriging matrix."""
import numpy as np
import pytest

from tests import _cv_cases as cv
from tests import test_cross_validate_folds_host as fh

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name,folding", fh.FOLDINGS)
def test_folds_against_brute_force(name, folding):
    """Each case prints cond_1 of the full matrix and its worst err / bar on z and sigma^2 before it asserts (run with -s)."""
    m, st = cv.global_case(name)
    ref = fh.fold_reference(name, folding)
    lab = fh.labels_of(st.n, folding)
    if "spherical" in name:  # the factor must hold the stations in Hilbert-curve order: lists and results go through sort_perm
        m.execute("points", st.coords_orig[:3, 0], st.coords_orig[:3, 1])
        assert m.last_timing["sparse"] == 1 and m.last_timing["stations_sorted"] == 1, m.last_timing
    zhat, ss = m.cross_validate(folds=5 if folding == "contiguous5" else lab)
    assert type(zhat) is np.ndarray and type(ss) is np.ndarray and zhat.dtype == ss.dtype == np.float64
    assert zhat.shape == ss.shape == (st.n,)
    rz, rs = cv.ratios(ref, zhat, ss)
    print("%s %s: cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (name, folding, float(ref.cond[0]), rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (name, folding, rz, rs)
    z1, s1 = m.cross_validate(st.values, folds=lab)  # the object's own values given explicitly, the folds as labels: the same bits
    assert _bits(z1, zhat) and _bits(s1, ss)


@pytest.mark.parametrize("which", ["small", "limit", "panels"])
def test_size_class_edges_against_brute_force(which):
    """Ordinary kriging, 2-D exponential, N = 300; one fold each of the sizes of fh.edge_sizes() and the remaining stations as one more:
    1, 2, 63, 64, 65 (+ 105) | LDS limit - 1, limit, limit + 1 (+ the rest) | 200, four panels (+ 100)."""
    m, st = fh.edge_case()
    lab = fh.edge_labels(which)
    sizes = np.bincount(lab)
    assert tuple(sizes[:-1]) == fh.edge_sizes()[which] and sizes.sum() == 300
    ref = fh.edge_reference(which)
    zi, si = fh.identity_folds(st, lab)
    iz, is_ = cv.ratios(ref, zi, si)
    print("%s (CPU identity): cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (which, float(ref.cond[0]), iz, is_))
    assert iz <= 0.5 and is_ <= 0.5, (which, iz, is_)
    zhat, ss = m.cross_validate(folds=lab)
    for f, s in enumerate(sizes):  # the figures per fold size, before the assertion
        sel = lab == f
        bz, bs = (b[sel] for b in cv.ek.bars(ref, cv.ec.C_BAR))
        print("  fold of %3d: |dz| / bar %.3g  |dss| / bar %.3g" % (s, float((np.abs(zhat[sel] - ref.z[sel].astype(np.float64)) / bz).max()),
                                                                   float((np.abs(ss[sel] - ref.ss[sel].astype(np.float64)) / bs).max())))
    rz, rs = cv.ratios(ref, zhat, ss)
    print("%s: |dz| / bar %.3g  |dss| / bar %.3g" % (which, rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (which, rz, rs)


@pytest.mark.parametrize("name", ["ok2d_exponential_n67", "ok2d_spherical_n130_values_1e3", "uk2d_regional_linear_n67"])
def test_leave_one_out_through_the_fold_path(name):
    m, st = cv.global_case(name)
    ref = cv.global_reference(name)
    z0, s0 = m.cross_validate()
    zn, sn = m.cross_validate(folds=st.n)
    zl, sl = m.cross_validate(folds=np.arange(st.n)[::-1].copy())
    assert _bits(zn, zl) and _bits(sn, sl)
    r0, rn = cv.ratios(ref, z0, s0), cv.ratios(ref, zn, sn)
    print("%s: folds=None %.3g %.3g   folds=N %.3g %.3g" % ((name,) + r0 + rn))
    assert max(r0) <= 1.0 and max(rn) <= 1.0, (name, r0, rn)


def test_results_do_not_depend_on_the_labels():
    m, st = fh.edge_case()
    rng = np.random.default_rng(21)
    lab = rng.integers(0, 4, st.n)
    lab[:120] = 0  # one blocked fold among the LDS ones
    z0, s0 = m.cross_validate(folds=lab)
    assert np.isfinite(z0).all() and np.isfinite(s0).all()
    for relabel in (np.array([3, 0, 2, 1]), np.array([-50, 7, 1 << 40, 8])):  # permuted; arbitrary values (another order, too)
        z1, s1 = m.cross_validate(folds=relabel[lab])
        assert _bits(z0, z1) and _bits(s0, s1)
    z2, s2 = m.cross_validate(folds=lab.astype(np.uint8))
    assert _bits(z0, z2) and _bits(s0, s2)
    for k in (2, 7):
        zk, sk = m.cross_validate(folds=k)
        zl, sl = m.cross_validate(folds=fh.contiguous(st.n, k) * 3 - 1)
        assert _bits(zk, zl) and _bits(sk, sl)


@pytest.mark.parametrize("name,folding", [("ok2d_exponential_n67", "contiguous5"), ("ok2d_spherical_n130_values_1e3", "leaves3"),
                                          ("uk3d_functional_n40", "random3")])
def test_fields_are_the_one_field_results_bit_for_bit(name, folding):
    m, st = cv.global_case(name)
    lab = fh.labels_of(st.n, folding)
    rng = np.random.default_rng(5)
    v = rng.standard_normal((st.n, 9))  # crosses MIK_FB = 8
    v[:, 0] = st.values
    zf, ss = m.cross_validate(v, folds=lab)
    assert zf.shape == (9, st.n) and ss.shape == (st.n,) and type(zf) is np.ndarray
    z0, s0 = m.cross_validate(folds=lab)
    assert _bits(zf[0], z0) and _bits(ss, s0)
    for f in range(9):
        z1, s1 = m.cross_validate(v[:, f], folds=lab)
        assert z1.shape == (st.n,)
        assert _bits(zf[f], z1), f
        assert _bits(ss, s1), f
    z2, _ = m.cross_validate(v[:, :1], folds=lab)
    assert z2.shape == (1, st.n) and _bits(z2[0], z0)


def test_execute_is_bit_identical_before_and_after_fold_calls():
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
    z1, s1 = m.cross_validate(folds=5)
    z3, s3 = m.cross_validate(rng.standard_normal((150, 3)), folds=5)
    z0, s0 = m.cross_validate()
    after = both()
    for a, b in zip(before, after):
        assert _bits(a, b)
    z1b, s1b = m.cross_validate(folds=5)
    z0b, s0b = m.cross_validate()
    assert _bits(z1, z1b) and _bits(s1, s1b) and _bits(s1, s3) and _bits(z0, z0b) and _bits(s0, s0b)


def test_resident_points_and_results_survive_a_fold_call_on_the_handle():
    """mik_cross_validate_folds between mik_predict and mik_get_results, factoring by itself: the earlier results come back, and a second
    predict on the same resident points needs no mik_set_points."""
    from pykrige_amd import _lib

    m, st = cv.global_case("ok2d_exponential_n67")
    rng = np.random.default_rng(1601)
    p = rng.random((500, 2))
    k = 17
    lab = fh.contiguous(st.n, 5)
    h = _lib.Handle(0)
    try:
        h.set_problem(ndim=2, xs=st.coords_adj[:, 0], ys=st.coords_adj[:, 1], zs=None, values=st.values, model_id=_lib.MODEL_IDS[st.model],
                      params=st.params)
        h.set_points(p[:, 0], p[:, 1])
        h.predict_moving_window(k)
        z0, s0 = [np.array(a) for a in h.get_results()]
        h.predict_moving_window(k)
        zg, sg = h.cross_validate_folds(lab, 5)  # factors by itself
        z1, s1 = [np.array(a) for a in h.get_results()]
        assert _bits(z0, z1) and _bits(s0, s1)
        h.predict()  # the factor the call left, the points set before
        zd, sd = [np.array(a) for a in h.get_results()]
        h.predict()
        zg2, sg2 = h.cross_validate_folds(lab, 5)  # the resident factor
        zd2, sd2 = [np.array(a) for a in h.get_results()]
        assert zd.shape == (500,) and _bits(zd, zd2) and _bits(sd, sd2) and _bits(zg, zg2) and _bits(sg, sg2)
        zm, sm = m.cross_validate(folds=5)
        assert _bits(zg[0], zm) and _bits(sg, sm)
        with pytest.raises(ValueError, match="fold index"):
            h.cross_validate_folds(lab, 4)  # an index outside [0, nfolds): an error, nothing computed
        with pytest.raises(ValueError, match="every station"):
            h.cross_validate_folds(np.zeros(st.n, dtype=np.int32), 2)
    finally:
        h.close()


def test_windowed_form_with_folds_is_an_error():
    m, st = cv.global_case("ok2d_exponential_n67")
    with pytest.raises(NotImplementedError, match="n_closest_points"):
        m.cross_validate(n_closest_points=10, backend="loop", folds=5)
