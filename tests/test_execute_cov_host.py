"""execute_cov without a GPU: the method exists on the four classes with the signature and the docstring the users read, every argument
error is raised before a handle is touched, mik_predict_cov is declared and exported, and the algebra the device evaluates -- B = A^-1
symmetrised, Y = b B, C = -gamma* - b Y^T with gamma*(d) = 0 for d <= eps -- stays inside the bar the device is held to, against the
extended-precision brute force.

Also the home of what tests/test_execute_cov.py (GPU) shares with this file: the points of a case, the cached brute-force reference and its
bar.  The bar of entry (p, q) is C_BAR u (cond_1(A) + M) max(max|b(p)|, max|b(q)|), capped at 1e-6 max(1, max|cov|): the project's sigma^2
bar (tests/_error_cases.C_BAR, the cap of ek.bars) with the larger of the two right-hand sides the entry is bilinear in."""
import functools
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _cv_cases as cv
from tests import _error_cases as ec
from tests.test_fields_gaps_host import adjusted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)
P_FULL = 300  # three blocks of 128 points: off-diagonal and mirrored tiles
ON_STATION = (0, 1, 2)  # points 0 and 1 sit on one station, point 2 on another
COINCIDENT = ((3, 4), (5, 299))  # pairs of equal points, inside one block and across blocks


# ------------------------------------------------------------------------------------------------------------- cases and references
@functools.lru_cache(maxsize=None)
def points(name):
    """P_FULL points in the bounding box of the stations of the GLOBAL case `name`, in the caller's (unadjusted) coordinates."""
    _, st = cv.global_case(name)
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    pts = lo + (hi - lo) * np.random.default_rng(4100 + sorted(cv.GLOBAL).index(name)).random((P_FULL, st.ndim))
    pts[0] = pts[1] = st.coords_orig[7]
    pts[2] = st.coords_orig[st.n - 1]
    for a, b in COINCIDENT:
        pts[b] = pts[a]
    return pts


def point_pair_distances(st, pa_):
    """(P, P) float64 distances between the adjusted points, by the functions the right-hand sides take theirs from."""
    if st.geographic:
        return ko.great_circle_distance(pa_[:, 0][:, None], pa_[:, 1][:, None], pa_[:, 0], pa_[:, 1])
    from scipy.spatial.distance import cdist

    rev = slice(None, None, -1) if st.ndim == 3 else slice(None)
    return cdist(pa_[:, rev], pa_[:, rev], "euclidean")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(cov longdouble (P, P), bar float64 (P, P)): -gamma*(d_pq) - b(p) . x(q) with A x(q) = b(q) refined in extended precision."""
    _, st = cv.global_case(name)
    pa_ = adjusted(st, points(name))
    a = ek.assemble(st, ek.station_distances(st))
    b = ek.right_hand_sides(st, pa_, ek.point_distances(st, pa_))
    x, cond = ek.refined_solve(a, b.T.copy())
    d = point_pair_distances(st, pa_)
    gam = ek.variogram_ld(st.model, st.params, d)
    gam[d <= ko.EPS] = 0
    cov = -gam - b @ x
    bscale = np.abs(b[:, :st.n]).max(axis=1).astype(np.float64)
    bar = ec.C_BAR * ek.U_F64 * (cond + a.shape[0]) * np.maximum(bscale[:, None], bscale[None, :])
    return cov, np.minimum(bar, 1e-6 * max(1.0, float(np.abs(cov).max())))


def worst_ratio(name, cov, npt=P_FULL):
    """max |cov - reference| / bar over the leading npt x npt corner, and the largest error."""
    ref, bar = reference(name)
    err = np.abs(np.asarray(cov, dtype=np.float64).astype(ek.LD) - ref[:npt, :npt]).astype(np.float64)
    return float((err / bar[:npt, :npt]).max()), float(err.max())


def restatement(name):
    """The device's stages in float64 NumPy."""
    _, st = cv.global_case(name)
    pa_ = adjusted(st, points(name))
    binv = np.linalg.inv(ko.kriging_matrix(st))
    binv = 0.5 * (binv + binv.T)
    b = ko.rhs(st, pa_)
    d = point_pair_distances(st, pa_)
    c = -np.where(d <= ko.EPS, 0.0, ko.variogram(st.model, st.params, d))  # stage 0
    y = b @ binv  # stage 1
    return c - b @ y.T  # stage 2


# ------------------------------------------------------------------------------------------------------------- the interface
def test_the_four_classes_have_execute_cov_with_the_documented_signature():
    for cls in CLASSES:
        names = list(inspect.signature(cls.execute_cov).parameters)
        coords = ["xpoints", "ypoints"] + (["zpoints"] if cls._ndim == 3 else [])
        assert names == ["self", "style"] + coords + ["backend", "specified_drift_arrays"], (cls, names)
        sig = inspect.signature(cls.execute_cov)
        assert sig.parameters["backend"].default == "vectorized" and sig.parameters["specified_drift_arrays"].default is None
        assert "n_closest_points" not in names
        doc = " ".join(cls.execute_cov.__doc__.split())
        for phrase in ("-gamma*(d_pq) - b(p)^T A^-1 b(q)", "gamma*(d) = 0 if d <= eps", "great-circle", "exact_values=True", "'masked'",
                       "'custom'", "NotImplementedError", "pseudo_inv=True", "device group", "largest ``P`` that fits",
                       "n_closest_points", "C-contiguous float64"):
            assert phrase in doc, (cls.__name__, phrase)


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def _objects(n=20, **kw):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    base = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1])
    base.update(kw)
    for cls in CLASSES:
        coords = (x, y, z) if cls._ndim == 3 else (x, y)
        yield cls, _no_device(cls(*coords, v, **base)), tuple(np.array([0.5, 0.25]) for _ in coords)


def test_argument_errors_raise_before_any_device_call():
    for cls, obj, pts in _objects():
        with pytest.raises(ValueError, match="masked"):
            obj.execute_cov("masked", *pts)
        with pytest.raises(ValueError, match="style argument"):
            obj.execute_cov("lattice", *pts)
        with pytest.raises(ValueError, match="backend"):
            obj.execute_cov("points", *pts, backend="cuda")
        with pytest.raises(ValueError, match="same dimensions"):
            obj.execute_cov("points", np.zeros(3), *[np.zeros(2) for _ in pts[1:]])
        with pytest.raises(ValueError, match="no points"):
            obj.execute_cov("points", *[np.zeros(0) for _ in pts])
        with pytest.raises(TypeError):
            obj.execute_cov("points", *pts, n_closest_points=4)
        if cls in (pa.OrdinaryKriging, pa.OrdinaryKriging3D):
            with pytest.raises(ValueError, match="specified_drift_arrays"):
                obj.execute_cov("points", *pts, specified_drift_arrays=[np.zeros(2)])
    for cls, obj, pts in _objects(pseudo_inv=True):
        with pytest.raises(ValueError, match="pseudo_inv"):
            obj.execute_cov("points", *pts)
    for cls, obj, pts in _objects(variogram_model="custom", variogram_parameters=[1.0, 0.1], variogram_function=lambda p, d: p[0] * d + p[1]):
        with pytest.raises(NotImplementedError, match="custom"):
            obj.execute_cov("points", *pts)


def test_specified_drift_errors_of_the_universal_classes_raise_before_any_device_call():
    rng = np.random.default_rng(2)
    n = 20
    x, y, v = rng.random(n), rng.random(n), rng.random(n)
    uk = _no_device(pa.UniversalKriging(x, y, v, variogram_model="linear", variogram_parameters=[1.0, 0.1], drift_terms=["specified"],
                                        specified_drift=[rng.random(n)]))
    pts = (np.array([0.5, 0.25]), np.array([0.5, 0.25]))
    with pytest.raises(ValueError, match="Must provide drift values"):
        uk.execute_cov("points", *pts)
    with pytest.raises(TypeError, match="encapsulated in a list"):
        uk.execute_cov("points", *pts, specified_drift_arrays=np.zeros(2))
    with pytest.raises(ValueError, match="do not match"):
        uk.execute_cov("points", *pts, specified_drift_arrays=[np.zeros(3)])


def test_a_device_group_is_refused_before_the_device_is_touched():
    class Group:
        n_devices = 2

    for cls, obj, pts in _objects():
        obj._handle = Group()
        try:
            with pytest.raises(ValueError, match="device group of 2"):
                obj.execute_cov("points", *pts)
        finally:
            obj._handle = None


# ------------------------------------------------------------------------------------------------------------- the library
def test_library_declares_and_exports_mik_predict_cov_at_abi_9():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert lib.mik_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert hasattr(lib, "mik_predict_cov") and "mik_predict_cov" in _lib.SIGNATURES
    assert callable(getattr(_lib.Handle, "predict_cov", None))
    header = open(os.path.join(ROOT, "include", "mikrige.h")).read()
    assert "int  mik_predict_cov(mik_handle *h, double *cov_out" in header
    assert "mik_predict_cov" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_predict_cov" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_a_library_without_the_symbol_is_answered_as_stale(monkeypatch):
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == "mik_predict_cov":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mik_predict_cov.*rebuild"):
        _lib.load()


# ------------------------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("name", sorted(cv.GLOBAL))
def test_the_float64_restatement_of_the_stages_is_inside_the_bar(name):
    cov = restatement(name)
    ratio, err = worst_ratio(name, cov)
    print("%s: worst err / bar %.3g, max err %.3g" % (name, ratio, err))
    assert ratio <= 1.0, (name, ratio, err)
    ref, bar = reference(name)
    r64 = ref.astype(np.float64)
    r64 = 0.5 * (r64 + r64.T)
    assert np.linalg.eigvalsh(r64).min() >= -P_FULL * bar.max()  # the reference is positive semidefinite
    _, st = cv.global_case(name)
    assert st.exact_values
    for p in ON_STATION:  # a point on a station is predicted without error
        assert np.all(np.abs(r64[p]) <= bar[p])
    for a, b in COINCIDENT:
        assert np.all(np.abs(r64[a] - r64[b]) <= 2 * bar[a])
