"""cross_validate without a GPU: the entry point exists in the built library, every argument error is raised before a handle is
touched, and the identity the device's global form evaluates -- zhat_i = v_i - c_i / B_ii, sigma^2_i = 1 / B_ii with B the inverse of
the full kriging matrix and c = B[:, :n] v -- agrees with brute force (station i kriged from the state without it, in extended
precision) on every global case of tests/test_cross_validate.py, within half the bar the device is held to."""
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from tests import _cv_cases as cv

CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)


def test_library_exports_mik_cross_validate_at_abi_9():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert lib.mik_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert hasattr(lib, "mik_cross_validate") and "mik_cross_validate" in _lib.SIGNATURES
    assert callable(getattr(_lib.Handle, "cross_validate", None))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_cross_validate" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_the_four_classes_have_cross_validate():
    for cls in CLASSES:
        assert callable(getattr(cls, "cross_validate", None)), cls.__name__
        assert "1 / B_ii" in cls.cross_validate.__doc__ and "NotImplementedError" in cls.cross_validate.__doc__


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def test_argument_errors_raise_before_any_device_call():
    rng = np.random.default_rng(0)
    n = 20
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1])
    ok = _no_device(pa.OrdinaryKriging(x, y, v, **kw))
    for bad, what in ((np.zeros((19, 2)), "rows"), (np.zeros(21), "rows"), (np.zeros((20, 0)), "F = 0"), (np.zeros((20, 2, 1)), "dimensions")):
        with pytest.raises(ValueError, match=what):
            ok.cross_validate(bad)
        with pytest.raises(ValueError, match=what):
            ok.cross_validate(bad, n_closest_points=5, backend="loop")
    for nonfinite in (np.nan, np.inf, -np.inf):
        bad = np.zeros((n, 2))
        bad[3, 1] = nonfinite
        with pytest.raises(ValueError, match="non-finite"):
            ok.cross_validate(bad)
    with pytest.raises(ValueError, match="backend"):
        ok.cross_validate(backend="cuda")
    with pytest.raises(ValueError, match="at least two"):
        ok.cross_validate(n_closest_points=1, backend="loop")
    with pytest.raises(ValueError, match="moving window is not supported"):  # ok.py:982-986: 'vectorized' has no moving window
        ok.cross_validate(n_closest_points=5)
    # the windowed form is not built: once the backend rules and the values have passed it is an error, never another path
    for k, backend in ((5, "loop"), (n, "loop"), (n + 5, "C")):
        with pytest.raises(NotImplementedError, match="n_closest_points"):
            ok.cross_validate(np.zeros((n, 3)), n_closest_points=k, backend=backend)
    ok3 = _no_device(pa.OrdinaryKriging3D(x, y, z, v, **kw))
    with pytest.raises(ValueError, match="not supported"):
        ok3.cross_validate(n_closest_points=5, backend="C")  # ok3d.py: no C backend
    with pytest.raises(ValueError, match="moving window is not supported"):
        ok3.cross_validate(n_closest_points=5, backend="vectorized")
    with pytest.raises(NotImplementedError, match="n_closest_points"):
        ok3.cross_validate(n_closest_points=5, backend="loop")
    # the universal-kriging classes have no moving window, whatever the backend
    uk = _no_device(pa.UniversalKriging(x, y, v, drift_terms=["regional_linear"], **kw))
    uk3 = _no_device(pa.UniversalKriging3D(x, y, z, v, drift_terms=["regional_linear"], **kw))
    for obj in (uk, uk3):
        for backend in ("vectorized", "loop", "hip"):
            with pytest.raises(ValueError, match="moving window is not supported"):
                obj.cross_validate(n_closest_points=5, backend=backend)
        with pytest.raises(ValueError, match="rows"):
            obj.cross_validate(np.zeros(n + 1))
    # the identity needs a regular matrix
    for cls, coords in ((pa.OrdinaryKriging, (x, y)), (pa.UniversalKriging, (x, y)), (pa.OrdinaryKriging3D, (x, y, z)),
                        (pa.UniversalKriging3D, (x, y, z))):
        with pytest.raises(ValueError, match="pseudo_inv"):
            _no_device(cls(*coords, v, pseudo_inv=True, **kw)).cross_validate()


@pytest.mark.parametrize("name", sorted(cv.GLOBAL))
def test_identity_agrees_with_brute_force_within_half_the_bar(name):
    """Measured here (float64 NumPy inverse): worst err / bar 0.0042 on z and 0.0014 on sigma^2 over the six cases at C = 8
    (cond_1 from 3e2 to 2.5e3)."""
    _, st = cv.global_case(name)
    ref = cv.global_reference(name)
    z, ss = cv.identity(st)
    rz, rs = cv.ratios(ref, z, ss)
    print("%s: cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (name, float(ref.cond[0]), rz, rs))
    assert rz <= 0.5 and rs <= 0.5, (name, rz, rs)
