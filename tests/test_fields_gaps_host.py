"""execute_fields(valid=...) without a GPU: the two entry points exist in the built library, every argument error is raised before a
handle is touched, valid=None keeps the old behaviour, and the identity the device evaluates -- for the missing stations S of a field,
with B the inverse of the full kriging matrix, b(p) the right-hand side of point p, v0 the field with zeros at S and c0 = B[:, :n] v0:
L L^T = B_SS, W = L^-1 B[S, :], g = L^-1 c0_S, c~ = c0 - W^T g (c~_S = 0), z_R(p) = c~ . b(p), sigma^2_R(p) = sigma^2(p) + |W b(p)|^2
-- agrees with brute force (the points kriged from the state without S, in extended precision) at the bar the device is held to.

Also the home of what tests/test_fields_gaps.py (GPU) shares with this file: the cases, their cached brute-force references and the
NumPy restatement of the identity."""
import functools
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg

import pykrige_amd as pa
from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _cv_cases as cv
from tests import test_cross_validate_folds_host as fh

CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)
EDGE_GAPS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 95, 96, 97, 200)  # around a 16-row group, a 64-column panel, the LDS limit; four panels
CLASS_GAPS = (0, 3, 5)


# ------------------------------------------------------------------------------------------------------------- cases
def adjusted(st, pts):
    """Points as the device sees them: the object's anisotropy adjustment about the object's centre."""
    pts = np.asarray(pts, dtype=np.float64)
    return pts if st.geographic else ko.adjust_for_anisotropy(pts, st.center, st.scaling, st.angle)


def full_cond(st):
    a = ko.kriging_matrix(st)
    return float(np.abs(a).sum(axis=0).max() * np.abs(scipy.linalg.inv(a)).sum(axis=0).max()), a.shape[0]


def reference(st, values, valid, pts):
    """Brute force per field: exact_points on the state without the field's missing stations (same centre, same adjusted coordinates).
    cond / order are the FULL matrix's (the identity reads the inverse of that matrix).  Returns one ExactResult per field."""
    cond, order = full_cond(st)
    pa_ = adjusted(st, pts)
    out = []
    for f in range(values.shape[1]):
        s = np.flatnonzero(~valid[:, f])
        sub = cv.without(st, s)
        sub.values = np.delete(values[:, f], s)
        r = ek.exact_points(sub, pa_)
        npt = pa_.shape[0]
        out.append(ek.ExactResult(z=r.z, ss=r.ss, cond=np.full(npt, cond), order=np.full(npt, order),
                                  vscale=np.full(npt, float(np.abs(sub.values).max())), bscale=r.bscale))
    return out


def identity_gaps(st, values, valid, pts):
    """The NumPy restatement of the device's path, (z, sigma^2) of shape (F, npt)."""
    n = st.n
    bm = np.linalg.inv(ko.kriging_matrix(st))
    b = ko.rhs(st, adjusted(st, pts))  # (npt, M)
    ss_all = -np.einsum("ti,ti->t", b, b @ bm.T)
    z, ss = [], []
    for f in range(values.shape[1]):
        s = np.flatnonzero(~valid[:, f])
        v0 = np.where(valid[:, f], values[:, f], 0.0)
        c0 = bm[:, :n] @ v0
        if s.size == 0:
            z.append(b @ c0)
            ss.append(ss_all)
            continue
        low = np.linalg.cholesky(bm[np.ix_(s, s)])
        w = scipy.linalg.solve_triangular(low, bm[s, :], lower=True)
        g = scipy.linalg.solve_triangular(low, c0[s], lower=True)
        ct = c0 - w.T @ g
        ct[s] = 0.0
        z.append(b @ ct)
        ss.append(ss_all + ((w @ b.T) ** 2).sum(axis=0))
    return np.array(z), np.array(ss)


def scattered_valid(n, counts, seed):
    """(n, F) valid with counts[f] missing stations in field f, nested prefixes of one permutation: the stations are scattered over the
    station order, perm[0] is missing in every field with a gap and perm[-1] in none."""
    perm = np.random.default_rng(seed).permutation(n)
    valid = np.ones((n, len(counts)), dtype=bool)
    for f, m in enumerate(counts):
        valid[perm[:m], f] = False
    return valid, perm


def field_values(st, nf, seed):
    rng = np.random.default_rng(seed)
    scale = float(np.abs(st.values).max())
    return st.values[:, None] * (1.0 + 0.25 * np.arange(nf)) + 0.1 * scale * rng.standard_normal((st.n, nf))


@functools.lru_cache(maxsize=None)
def edge_gap_case():
    """The 300-station case of the fold tests, 13 fields, 130 points (crosses a 128-point block): a point on a missing station, one on a
    present station, that one repeated."""
    m, st = fh.edge_case()
    valid, perm = scattered_valid(st.n, EDGE_GAPS, 21)
    values = field_values(st, len(EDGE_GAPS), 22)
    pts = np.random.default_rng(23).random((130, 2))
    pts[5] = st.coords_orig[perm[0]]
    pts[77] = st.coords_orig[perm[-1]]
    pts[129] = pts[77]
    return m, st, values, valid, pts


@functools.lru_cache(maxsize=None)
def edge_gap_reference():
    _, st, values, valid, pts = edge_gap_case()
    return reference(st, values, valid, pts)


@functools.lru_cache(maxsize=None)
def class_gap_case(name):
    """A GLOBAL case of the cross-validation tests with F = 3 (0, 3 and 5 missing stations) and 40 points inside the stations' box."""
    m, st = cv.global_case(name)
    valid, perm = scattered_valid(st.n, CLASS_GAPS, 31)
    values = field_values(st, len(CLASS_GAPS), 32)
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    pts = lo + (hi - lo) * np.random.default_rng(33).random((40, st.ndim))
    pts[3] = st.coords_orig[perm[0]]
    pts[17] = st.coords_orig[perm[-1]]
    return m, st, values, valid, pts


@functools.lru_cache(maxsize=None)
def class_gap_reference(name):
    _, st, values, valid, pts = class_gap_case(name)
    return reference(st, values, valid, pts)


def worst_ratios(refs, z, ss):
    """(max |dz| / bar, max |dss| / bar) over the fields, each field printed."""
    wz = ws = 0.0
    for f, ref in enumerate(refs):
        rz, rs = cv.ratios(ref, z[f], ss[f])
        print("field %d: cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (f, float(ref.cond[0]), rz, rs))
        wz, ws = max(wz, rz), max(ws, rs)
    return wz, ws


# ------------------------------------------------------------------------------------------------------------- tests
def test_library_exports_the_gap_entry_points_at_abi_9():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert lib.mik_abi_version() == 9 and _lib.ABI_VERSION == 9
    for name in ("mik_set_field_gaps", "mik_get_field_sigmasq"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(getattr(_lib.Handle, "set_field_gaps", None)) and callable(getattr(_lib.Handle, "get_field_sigmasq", None))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert {"mik_set_field_gaps", "mik_get_field_sigmasq"} <= have


@pytest.mark.parametrize("missing", ["mik_set_field_gaps", "mik_get_field_sigmasq"])
def test_a_library_without_the_symbols_is_answered_as_stale(monkeypatch, missing):
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == missing:
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export %s.*rebuild" % missing):
        _lib.load()


def _objects(n=20, **extra):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1], **extra)
    for cls, coords in ((pa.OrdinaryKriging, (x, y)), (pa.UniversalKriging, (x, y)), (pa.OrdinaryKriging3D, (x, y, z)),
                        (pa.UniversalKriging3D, (x, y, z))):
        yield cls, fh._no_device(cls(*coords, v, **kw)), tuple(np.array([0.5, 0.25]) for _ in coords)


def test_valid_argument_errors_raise_before_any_device_call():
    n = 20
    rng = np.random.default_rng(1)
    vals = rng.random((n, 3))
    good = np.ones((n, 3), dtype=bool)
    good[2, 1] = good[7, 1] = good[7, 2] = False
    for cls, obj, pts in _objects(n):
        def call(values, valid, **kw):
            return obj.execute_fields("points", *pts, values, valid=valid, **kw)

        for bad in (good.astype(np.uint8), good.astype(np.float64), good.astype(np.int64), good.astype(int).tolist(), "valid", 1):  # not boolean
            with pytest.raises(ValueError, match="valid must be a boolean"):
                call(vals, bad)
        for bad in (good[:-1], good[:, :2], good.T, good[:, 0], good[:, :1], good[None], np.ones((0,), dtype=bool)):  # shape
            with pytest.raises(ValueError, match="valid has shape"):
                call(vals, bad)
        with pytest.raises(ValueError, match="valid has shape"):  # 1-D values take a 1-D valid
            call(vals[:, 0], good[:, :1])
        for poison in (np.nan, np.inf, -np.inf):  # a True entry on a non-finite value
            v = vals.copy()
            v[4, 0] = poison
            with pytest.raises(ValueError, match="non-finite entries where valid is True"):
                call(v, good)
        none = good.copy()
        none[:, 2] = False
        with pytest.raises(ValueError, match="field 2 has no valid station"):
            call(vals, none)
        with pytest.raises(ValueError, match="no valid station"):
            call(vals[:, 0], np.zeros(n, dtype=bool))
        # the existing checks come first: style, backend, the values' own shape
        with pytest.raises(ValueError, match="style"):
            obj.execute_fields("cloud", *pts, vals, valid=good.astype(np.uint8))
        with pytest.raises(ValueError, match="rows"):
            call(np.zeros((n + 1, 3)), good)
        # non-finite values under a False entry are fine as far as the host checks go: the next stop is the device
        v = vals.copy()
        v[2, 1], v[7, 1], v[7, 2] = np.nan, np.inf, -np.inf
        with pytest.raises(AssertionError, match="device was touched"):
            call(v, good)
    for cls, obj, pts in _objects(n, pseudo_inv=True):
        with pytest.raises(ValueError, match="pseudo_inv"):
            obj.execute_fields("points", *pts, vals, valid=good)
        with pytest.raises(ValueError, match="valid must be a boolean"):  # a bad valid before pseudo_inv
            obj.execute_fields("points", *pts, vals, valid=good.astype(np.int8))
    for cls, obj, pts in _objects(n):
        if cls in (pa.OrdinaryKriging, pa.OrdinaryKriging3D):  # the classes with a moving window
            with pytest.raises(NotImplementedError, match="n_closest_points"):
                obj.execute_fields("points", *pts, vals, backend="loop", n_closest_points=5, valid=good)
        else:
            with pytest.raises(TypeError):
                obj.execute_fields("points", *pts, vals, n_closest_points=5, valid=good)

        class Group:
            n_devices = 4

        obj._handle = Group()
        try:
            with pytest.raises(ValueError, match="device group of 4"):
                obj.execute_fields("points", *pts, vals, valid=good)
        finally:
            obj._handle = None


def test_valid_is_the_last_keyword_and_none_keeps_the_old_errors():
    import inspect

    v = np.random.default_rng(2).random((20, 2))
    v[3, 1] = np.nan
    for cls, obj, pts in _objects(20):
        params = list(inspect.signature(cls.execute_fields).parameters)
        assert params[-1] == "valid" and inspect.signature(cls.execute_fields).parameters["valid"].default is None
        for kw in ({}, {"valid": None}):
            with pytest.raises(ValueError, match="^values holds non-finite entries$"):
                obj.execute_fields("points", *pts, v, **kw)
        for s in ("valid", "sigma^2_R(p) = sigma^2(p) + |W b(p)|^2", "NotImplementedError", "device group"):
            assert s in cls.execute_fields.__doc__, (cls.__name__, s)


@pytest.mark.parametrize("name", sorted(cv.GLOBAL))
def test_gap_identity_agrees_with_brute_force_at_the_bar(name):
    _, st, values, valid, pts = class_gap_case(name)
    z, ss = identity_gaps(st, values, valid, pts)
    rz, rs = worst_ratios(class_gap_reference(name), z, ss)
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)


def test_gap_identity_at_the_edge_sizes_agrees_with_brute_force_at_the_bar():
    _, st, values, valid, pts = edge_gap_case()
    z, ss = identity_gaps(st, values, valid, pts)
    rz, rs = worst_ratios(edge_gap_reference(), z, ss)
    assert rz <= 1.0 and rs <= 1.0, (rz, rs)
