"""cross_validate(folds=...) without a GPU: the entry point exists in the built library, every argument error is raised before a handle
is touched, folds=K is scikit-learn's KFold(K), and the identity the device evaluates -- for a fold S, with B the inverse of the full
kriging matrix and c = B[:, :n] v:  zhat_S = v_S - B_SS^-1 c_S,  sigma^2_S = diag(B_SS^-1)  -- agrees with brute force (the fold kriged
from the state without it, in extended precision) within half the bar the device is held to.

Also the home of what tests/test_cross_validate_folds.py (GPU) shares with this file: the foldings, their cached brute-force
references and the NumPy restatement of the identity."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg

import pykrige_amd as pa
from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _cv_cases as cv

CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)
ORDINARY = ("ok2d_exponential_n67", "ok2d_spherical_n130_values_1e3", "ok3d_gaussian_aniso_n40")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- foldings
def contiguous(n, k):
    """KFold(k) without shuffle as labels: the first n % k folds have n // k + 1 stations."""
    lab = np.empty(n, dtype=np.int64)
    for f, s in enumerate(np.array_split(np.arange(n), k)):
        lab[s] = f
    return lab


def labels_of(n, folding):
    if folding == "contiguous5":
        return contiguous(n, 5)
    if folding == "random3":
        return np.random.default_rng(7).integers(0, 3, n)
    if folding == "leaves3":  # one fold that leaves only three stations (ordinary kriging only: three stations do not carry a regional drift)
        return np.array([0] * (n - 3) + [1] * 3, dtype=np.int64)
    raise KeyError(folding)


FOLDINGS = [(name, f) for name in sorted(cv.GLOBAL) for f in ("contiguous5", "random3")] + [(name, "leaves3") for name in ORDINARY]


def _reference(st, labels):
    """Brute force: exact_points on the state without the fold, at the fold's stations.  cond / order are the FULL matrix's."""
    n = st.n
    z, ss, bscale = np.zeros(n, dtype=ek.LD), np.zeros(n, dtype=ek.LD), np.zeros(n)
    for g in np.unique(labels):
        s = np.flatnonzero(labels == g)
        r = ek.exact_points(cv.without(st, s), st.coords_adj[s])
        z[s], ss[s], bscale[s] = r.z, r.ss, r.bscale
    a = ko.kriging_matrix(st)
    cond = float(np.abs(a).sum(axis=0).max() * np.abs(scipy.linalg.inv(a)).sum(axis=0).max())
    return ek.ExactResult(z=z, ss=ss, cond=np.full(n, cond), order=np.full(n, a.shape[0]),
                          vscale=np.full(n, float(np.abs(st.values).max())), bscale=bscale)


@functools.lru_cache(maxsize=None)
def fold_reference(name, folding):
    _, st = cv.global_case(name)
    return _reference(st, labels_of(st.n, folding))


def identity_folds(st, labels, values=None):
    """The NumPy restatement of the device's fold path: B = inv(A), c = B[:, :n] v and per fold G = B[S, S] = L L^T, W = L^-1,
    zhat_S = v_S - W^T (W c_S), sigma^2_S = column sums of W^2."""
    n = st.n
    v = st.values if values is None else values
    b = np.linalg.inv(ko.kriging_matrix(st))
    c = b[:n, :n] @ v
    z, ss = np.empty(n), np.empty(n)
    for g in np.unique(labels):
        s = np.flatnonzero(labels == g)
        w = scipy.linalg.solve_triangular(np.linalg.cholesky(b[np.ix_(s, s)]), np.eye(s.size), lower=True)
        z[s] = v[s] - w.T @ (w @ c[s])
        ss[s] = (w * w).sum(axis=0)
    return z, ss


# the size-class edges of the device (tests/test_cross_validate_folds.py): ordinary kriging, 2-D exponential, N = 300
@functools.lru_cache(maxsize=None)
def edge_case():
    rng = np.random.default_rng(1201)
    c = rng.random((300, 2))
    m = pa.OrdinaryKriging(c[:, 0], c[:, 1], cv._field(c), variogram_model="exponential", variogram_parameters=[1.0, 0.5, 0.02])
    return m, cv.state_of(m)


def edge_sizes():
    """Fold sizes of the three edge foldings; in each the remaining stations form one further fold.  1 and 2; 63, 64, 65 (one panel of the
    blocked class and its neighbours, here still in LDS); the LDS limit - 1, the limit and the limit + 1 (the first blocked fold, two
    panels); 200 (four panels); the remainders 105 and 100 (two panels)."""
    from pykrige_amd import _lib

    lim = _lib.CV_FOLDS_LDS
    return {"small": (1, 2, 63, 64, 65), "limit": (lim - 1, lim, lim + 1), "panels": (200,)}


def edge_labels(which):
    sizes = edge_sizes()[which]
    perm = np.random.default_rng(11).permutation(300)  # the folds are scattered over the station order
    lab = np.full(300, len(sizes), dtype=np.int64)
    o = 0
    for f, s in enumerate(sizes):
        lab[perm[o:o + s]] = f
        o += s
    assert o < 300
    return lab


@functools.lru_cache(maxsize=None)
def edge_reference(which):
    return _reference(edge_case()[1], edge_labels(which))


# ------------------------------------------------------------------------------------------------------------- tests
def test_library_exports_mik_cross_validate_folds_at_abi_9():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert lib.mik_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert hasattr(lib, "mik_cross_validate_folds") and "mik_cross_validate_folds" in _lib.SIGNATURES
    assert callable(getattr(_lib.Handle, "cross_validate_folds", None))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_cross_validate_folds" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    # the LDS limit the tests cross is the kernel header's
    src = open(os.path.join(ROOT, "pykrige_amd", "csrc", "mik_k_cvfolds.h")).read()
    assert int(re.search(r"#define MIK_CVF_LDS (\d+)", src).group(1)) == _lib.CV_FOLDS_LDS


def test_a_library_without_the_symbol_is_answered_as_stale(monkeypatch):
    """A library from before the entry point also reports ABI 9: the loader must end in its rebuild message, not in an AttributeError."""
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == "mik_cross_validate_folds":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mik_cross_validate_folds.*rebuild"):
        _lib.load()


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def test_fold_argument_errors_raise_before_any_device_call():
    rng = np.random.default_rng(0)
    n = 20
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1])
    good = np.arange(n) % 4
    for cls, coords in ((pa.OrdinaryKriging, (x, y)), (pa.UniversalKriging, (x, y)), (pa.OrdinaryKriging3D, (x, y, z)),
                        (pa.UniversalKriging3D, (x, y, z))):
        obj = _no_device(cls(*coords, v, **kw))
        for bad in (2.0, np.float64(3), "5", True, good.astype(np.float64), good.astype(bool), [0.5] * n,  # not integers
                    good[:-1], np.zeros(n + 1, dtype=np.int64), good.reshape(4, 5), good[:, None], np.zeros((0,), dtype=np.int32),  # shape
                    1, 0, -3, n + 1, np.int64(n + 1), np.int32(1),  # K out of range
                    np.zeros(n, dtype=np.int64), np.full(n, -7)):  # fewer than two distinct labels
            with pytest.raises(ValueError, match="folds"):
                obj.cross_validate(folds=bad)
        # the existing checks come first: backend, then values
        with pytest.raises(ValueError, match="backend|not supported"):
            obj.cross_validate(backend="cuda", folds=2.0)
        with pytest.raises(ValueError, match="rows"):
            obj.cross_validate(np.zeros(n + 1), folds=2.0)
        # a bad folds before the windowed form's NotImplementedError and before pseudo_inv
        with pytest.raises(ValueError, match="folds"):
            _no_device(cls(*coords, v, pseudo_inv=True, **kw)).cross_validate(folds=1)
        with pytest.raises(ValueError, match="pseudo_inv"):
            _no_device(cls(*coords, v, pseudo_inv=True, **kw)).cross_validate(folds=good)
        with pytest.raises(ValueError, match="pseudo_inv"):
            _no_device(cls(*coords, v, pseudo_inv=True, **kw)).cross_validate(None, None, "vectorized", 4)  # folds is the fourth argument
    for cls, coords in ((pa.OrdinaryKriging, (x, y)), (pa.OrdinaryKriging3D, (x, y, z))):  # the classes with a moving window
        obj = _no_device(cls(*coords, v, **kw))
        with pytest.raises(ValueError, match="folds"):
            obj.cross_validate(n_closest_points=5, backend="loop", folds=1)
        for ok_folds in (5, np.int64(n), good, list(good), good - 100):
            with pytest.raises(NotImplementedError, match="n_closest_points"):
                obj.cross_validate(n_closest_points=5, backend="loop", folds=ok_folds)
            with pytest.raises(NotImplementedError, match="n_closest_points"):  # pseudo_inv comes after the windowed form
                _no_device(cls(*coords, v, pseudo_inv=True, **kw)).cross_validate(n_closest_points=5, backend="loop", folds=ok_folds)


def test_the_docstring_states_the_fold_formulas_and_keeps_the_leave_one_out_wording():
    for cls in CLASSES:
        doc = cls.cross_validate.__doc__
        for s in ("1 / B_ii", "NotImplementedError", "folds=None", "B_SS^-1 = A_SS - A_SR A_RR^-1 A_RS", "zhat_S = v_S - B_SS^-1 c_S",
                  "sigmasq_S = diag(B_SS^-1)", "KFold", "NaN"):
            assert s in doc, (cls.__name__, s)


@pytest.mark.parametrize("n,k", [(67, 5), (10, 10)])
def test_integer_folds_are_scikit_learns_kfold(n, k):
    from sklearn.model_selection import KFold

    rng = np.random.default_rng(3)
    m = pa.OrdinaryKriging(rng.random(n), rng.random(n), rng.random(n), variogram_model="linear", variogram_parameters=[1.0, 0.1])
    for kk in (k, np.int64(k), np.int32(k)):
        lab, nfolds = m._fold_labels(kk)
        assert nfolds == k and lab.dtype == np.int32 and lab.shape == (n,)
        for f, (_, test) in enumerate(KFold(k).split(np.zeros((n, 1)))):
            assert np.array_equal(np.flatnonzero(lab == f), test), f
    assert np.array_equal(lab, contiguous(n, k))
    # labels: compacted in ascending order of the label values, whatever they are
    raw = np.array([40, -3, 40, 7, -3] * (n // 5) + [7] * (n % 5))
    lab, nfolds = m._fold_labels(raw)
    assert nfolds == 3 and np.array_equal(lab, np.searchsorted([-3, 7, 40], raw)) and lab.dtype == np.int32


@pytest.mark.parametrize("name,folding", FOLDINGS)
def test_fold_identity_agrees_with_brute_force_within_half_the_bar(name, folding):
    """Measured here (float64 NumPy inverse and Cholesky) at C = 8: worst err / bar 0.0043 on z and 0.0041 on sigma^2 over the six cases
    with 5 contiguous folds and 3 random groups; at most 0.036 with the fold that leaves three stations (ordinary kriging)."""
    _, st = cv.global_case(name)
    ref = fold_reference(name, folding)
    z, ss = identity_folds(st, labels_of(st.n, folding))
    rz, rs = cv.ratios(ref, z, ss)
    print("%s %s: cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (name, folding, float(ref.cond[0]), rz, rs))
    assert rz <= 0.5 and rs <= 0.5, (name, folding, rz, rs)
