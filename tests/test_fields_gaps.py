"""execute_fields(valid=...) on the device: fields with missing stations kriged from the one resident inverse (mik_k_gaps.h).

References are brute force (tests/test_fields_gaps_host.py: the points kriged from the state without the missing stations, in extended
precision, cached per session); the bar is the cross-validation bar (tests/_cv_cases.ratios, C_BAR, cond and order of the full matrix)."""
import numpy as np
import pytest

from tests import _cv_cases as cv
from tests import test_fields_gaps_host as gh

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a, b = np.ascontiguousarray(np.asarray(a), dtype=np.float64), np.ascontiguousarray(np.asarray(b), dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cols(pts):
    return tuple(np.ascontiguousarray(pts[:, k]) for k in range(pts.shape[1]))


# ------------------------------------------------------------------------------------------------------------- against brute force
def test_edge_sizes_against_brute_force():
    """0, 1, 2, 15, 16, 17, 63, 64, 65, 95, 96, 97 and 200 missing stations of 300 in one call of 13 fields, 130 points."""
    m, st, values, valid, pts = gh.edge_gap_case()
    z, ss = m.execute_fields("points", *_cols(pts), values, valid=valid)
    assert z.shape == ss.shape == (len(gh.EDGE_GAPS), 130) and isinstance(z, np.ma.MaskedArray) and isinstance(ss, np.ma.MaskedArray)
    assert m.last_timing["sparse"] == 0
    rz, rs = gh.worst_ratios(gh.edge_gap_reference(), np.asarray(z), np.asarray(ss))
    assert rz <= 1.0 and rs <= 1.0, (rz, rs)
    assert _bits(np.asarray(z)[:, 129], np.asarray(z)[:, 77]) and _bits(np.asarray(ss)[:, 129], np.asarray(ss)[:, 77])  # the repeated point


@pytest.mark.parametrize("name", sorted(cv.GLOBAL))
def test_classes_against_brute_force(name):
    m, st, values, valid, pts = gh.class_gap_case(name)
    z, ss = m.execute_fields("points", *_cols(pts), values, valid=valid)
    assert z.shape == ss.shape == (3, 40)
    rz, rs = gh.worst_ratios(gh.class_gap_reference(name), np.asarray(z), np.asarray(ss))
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)
    if "spherical" in name:  # gaps take the dense path; the next call without them is range-aware again
        assert m.last_timing["sparse"] == 0
        m.execute_fields("points", *_cols(pts), values)
        assert m.last_timing["sparse"] == 1


# ------------------------------------------------------------------------------------------------------------- bits
def _bits_case():
    m, st, values, valid, pts = gh.edge_gap_case()
    # fields 3 and 7 (15 and 64 missing), a field without gaps, field 3's pattern again on other values, field 12 (200 missing)
    v = np.stack([values[:, 3], values[:, 7], values[:, 0], values[:, 5], values[:, 12]], axis=1)
    ok = np.stack([valid[:, 3], valid[:, 7], valid[:, 0], valid[:, 3], valid[:, 12]], axis=1)
    return m, v, ok, _cols(pts)


def test_planes_are_the_one_field_results_bit_for_bit():
    m, v, ok, p = _bits_case()
    z, ss = [np.asarray(a) for a in m.execute_fields("points", *p, v, valid=ok)]
    for f in range(v.shape[1]):
        z1, s1 = [np.asarray(a) for a in m.execute_fields("points", *p, v[:, f], valid=ok[:, f])]
        assert z1.shape == s1.shape == (1, 130)
        assert _bits(z1[0], z[f]) and _bits(s1[0], ss[f]), f
    assert _bits(ss[0], ss[3]) and not _bits(ss[0], ss[1])  # one pattern, one sigma^2 plane
    # the field without gaps: z and sigma^2 of execute_fields without valid (which kriges it as field 2 of the same five)
    zp, sp = [np.asarray(a) for a in m.execute_fields("points", *p, np.where(ok, v, 0.0))]
    assert _bits(z[2], zp[2]) and _bits(ss[2], sp)


def test_valid_all_true_is_the_call_without_valid():
    m, v, ok, p = _bits_case()
    zp, sp = [np.asarray(a) for a in m.execute_fields("points", *p, v)]
    z, ss = [np.asarray(a) for a in m.execute_fields("points", *p, v, valid=np.ones(v.shape, dtype=bool))]
    assert _bits(z, zp) and ss.shape == z.shape
    for f in range(v.shape[1]):
        assert _bits(ss[f], sp)


def test_ignored_entries_change_no_bit():
    m, v, ok, p = _bits_case()
    z, ss = [np.asarray(a) for a in m.execute_fields("points", *p, v, valid=ok)]
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(ss))
    for fill in (np.nan, 0.0, 1e300, np.inf):
        z2, s2 = [np.asarray(a) for a in m.execute_fields("points", *p, np.where(ok, v, fill), valid=ok)]
        assert _bits(z2, z) and _bits(s2, ss), fill


def test_several_launches_give_the_bits_of_one():
    m, v, ok, _ = _bits_case()
    gx, gy = np.linspace(0.0, 1.0, 61), np.linspace(0.0, 1.0, 47)
    z, ss = [np.asarray(a) for a in m.execute_fields("grid", gx, gy, v, valid=ok)]
    assert m.last_timing["contract_launches"] == 1
    h = m._get_handle()
    h.set_option("chunk", 1024)
    try:
        z3, s3 = [np.asarray(a) for a in m.execute_fields("grid", gx, gy, v, valid=ok)]
        assert m.last_timing["contract_launches"] >= 3
    finally:
        h.set_option("chunk", 131072)
    assert z.shape == ss.shape == (5, 47, 61) and _bits(z3, z) and _bits(s3, ss)


# ------------------------------------------------------------------------------------------------------------- styles, afterwards
def test_grid_and_masked_styles():
    m, v, ok, _ = _bits_case()
    gx, gy = np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 7)
    zg, sg = m.execute_fields("grid", gx, gy, v, valid=ok)
    assert zg.shape == sg.shape == (5, 7, 9) and isinstance(zg, np.ma.MaskedArray) and isinstance(sg, np.ma.MaskedArray)
    assert not np.ma.getmaskarray(zg).any() and not np.ma.getmaskarray(sg).any()
    zl, sl = m.execute_fields("grid", gx, gy, v, backend="loop", valid=ok)
    assert not isinstance(zl, np.ma.MaskedArray) and not isinstance(sl, np.ma.MaskedArray) and _bits(zl, zg.data) and _bits(sl, sg.data)
    mask = np.zeros((7, 9), dtype=bool)
    mask[2, 3:6] = mask[5, 0] = mask[6, 8] = True
    zm, sm = m.execute_fields("masked", gx, gy, v, mask=mask, valid=ok)
    assert zm.shape == sm.shape == (5, 7, 9) and isinstance(zm, np.ma.MaskedArray) and isinstance(sm, np.ma.MaskedArray)
    for f in range(5):
        assert np.array_equal(np.ma.getmaskarray(zm[f]), mask) and np.array_equal(np.ma.getmaskarray(sm[f]), mask)
        assert np.all(zm.data[f][mask] == 0.0) and np.all(sm.data[f][mask] == 0.0)
        assert _bits(zm.data[f][~mask], zg.data[f][~mask]) and _bits(sm.data[f][~mask], sg.data[f][~mask])


def test_execute_and_cross_validate_keep_their_bits_after_a_call_with_gaps():
    m, v, ok, p = _bits_case()
    z0, s0 = [np.array(a) for a in m.execute("points", *p)]
    c0, d0 = m.cross_validate(folds=5)
    m.execute_fields("points", *p, v, valid=ok)
    z1, s1 = [np.array(a) for a in m.execute("points", *p)]
    c1, d1 = m.cross_validate(folds=5)
    assert _bits(z0, z1) and _bits(s0, s1) and _bits(c0, c1) and _bits(d0, d1)


def test_the_library_refuses_gaps_where_they_are_not_built():
    m, v, ok, p = _bits_case()
    m.execute("points", *p)  # problem, factor and points are resident
    h = m._get_handle()
    h.set_fields(v.T)
    try:
        none = ok.copy()
        none[:, 1] = False
        with pytest.raises(Exception, match="no valid station"):
            h.set_field_gaps(none.T)
        h.set_field_gaps(ok.T)
        with pytest.raises(Exception, match="gaps"):
            h.predict_moving_window(8)
        h.set_field_gaps(None)
        h.predict()  # gaps cleared: the plain fields path
        assert _bits(h.get_field_sigmasq()[1], h.get_results()[1])
    finally:
        h.set_fields(None)
