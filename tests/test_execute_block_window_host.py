"""execute_block_window without a GPU: the method exists on the four classes with the signature and the docstring the users read, every
refusal is raised before a handle is touched, mik_predict_block_window is declared and exported at ABI 9, and the algebra the device
evaluates -- the window chosen by the block's centre, bbar = the node-ordered mean of the nodes' right-hand sides over that window, an LU
solve of the local system, sigma^2 = -lam . bbar - mu - gbar -- stays inside the bars the device is held to, against the extended-precision
brute force, for every case the GPU tests run (tests/_mwblock_cases.py): the cases and their bars are satisfiable and tie-free."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from tests import _mwblock_cases as mb
from tests import test_execute_cov_host as ch

ROOT = ch.ROOT
CLASSES = ch.CLASSES
ORDINARY = (pa.OrdinaryKriging, pa.OrdinaryKriging3D)


# ------------------------------------------------------------------------------------------------------------- the interface
def test_the_four_classes_have_execute_block_window_with_the_documented_signature():
    for cls in CLASSES:
        sig = inspect.signature(cls.execute_block_window)
        coords = ["xpoints", "ypoints"] + (["zpoints"] if cls._ndim == 3 else [])
        assert list(sig.parameters) == ["self", "style"] + coords + ["block_size", "n_closest_points", "n_disc", "backend"], (cls, list(sig.parameters))
        assert sig.parameters["n_disc"].default == 4 and sig.parameters["backend"].default == "loop"
        assert sig.parameters["block_size"].default is inspect.Parameter.empty
        assert sig.parameters["n_closest_points"].default is inspect.Parameter.empty
        doc = " ".join(cls.execute_block_window.__doc__.split())
        for phrase in ("chosen by the centre", "(squared distance, station index)", "bbar_j = (sum_u g(|p + T u - s_j|)) / nd",
                       "g(d) = 0 if exact_values and d <= eps, else -gamma(d)", "bbar_k = 1", "sigma^2_V = -lam . bbar - mu - gbar",
                       "ARITHMETIC MEAN", "``n_disc=1`` is ``execute(style, ..., n_closest_points=k)`` bit for bit", "nd = prod(n_disc) <= 512",
                       "'masked'", "'geographic'", "device group", "'custom'", "NotImplementedError", "n_closest_points > N",
                       "Singular matrix", "``last_timing`` is set"):
            assert phrase in doc, (cls.__name__, phrase)
        # execute_block keeps its signature and now points here
        bdoc = " ".join(cls.execute_block.__doc__.split())
        assert "n_closest_points" in bdoc and "execute_block_window()" in bdoc and "There is no ``n_closest_points``" not in bdoc
        assert "n_closest_points" not in inspect.signature(cls.execute_block).parameters


def test_every_refusal_is_raised_before_any_device_call():
    for cls, obj, pts in ch._objects():
        if cls not in ORDINARY:
            continue
        with pytest.raises(ValueError, match="masked"):
            obj.execute_block_window("masked", *pts, 0.1, 4)
        with pytest.raises(ValueError, match="style argument"):
            obj.execute_block_window("lattice", *pts, 0.1, 4)
        with pytest.raises(ValueError, match="backend"):
            obj.execute_block_window("points", *pts, 0.1, 4, backend="cuda")
        with pytest.raises(ValueError, match="moving window"):  # a backend of execute() that the reference has no window for
            obj.execute_block_window("points", *pts, 0.1, 4, backend="vectorized")
        with pytest.raises(TypeError):  # n_closest_points has no default
            obj.execute_block_window("points", *pts, 0.1)
        with pytest.raises(ValueError, match="needs n_closest_points"):
            obj.execute_block_window("points", *pts, 0.1, None)
        for bad in (1, 0, -3):
            with pytest.raises(ValueError, match="at least two"):
                obj.execute_block_window("points", *pts, 0.1, bad)
        with pytest.raises(ValueError, match="exceeds the number of stations"):
            obj.execute_block_window("points", *pts, 0.1, 21)  # N = 20
        for bad in (0.0, -1.0, float("nan"), float("inf"), (0.1,) * (cls._ndim + 1), (0.1,) * (cls._ndim - 1), (0.1,) * (cls._ndim - 1) + (0.0,),
                    "wide"):
            with pytest.raises(ValueError, match="block_size"):
                obj.execute_block_window("points", *pts, bad, 4)
        for bad in (0, -2, 2.5, (2,) * (cls._ndim + 1), (2,) * (cls._ndim - 1) + (0,), None):
            with pytest.raises(ValueError, match="n_disc"):
                obj.execute_block_window("points", *pts, 0.1, 4, n_disc=bad)
        too_many = (23, 23) if cls._ndim == 2 else (9, 8, 8)  # 529 and 576 nodes
        with pytest.raises(ValueError, match="at most 512"):
            obj.execute_block_window("points", *pts, 0.1, 4, n_disc=too_many)
        with pytest.raises(ValueError, match="same dimensions"):
            obj.execute_block_window("points", np.zeros(3), *[np.zeros(2) for _ in pts[1:]], 0.1, 4)
    for cls, obj, pts in ch._objects(variogram_model="custom", variogram_parameters=[1.0, 0.1], variogram_function=lambda p, d: p[0] * d + p[1]):
        if cls in ORDINARY:
            with pytest.raises(NotImplementedError, match="custom"):
                obj.execute_block_window("points", *pts, 0.1, 4)
    rng = np.random.default_rng(5)
    lon, lat, v = rng.uniform(0, 30, 20), rng.uniform(30, 60, 20), rng.random(20)
    geo = ch._no_device(pa.OrdinaryKriging(lon, lat, v, variogram_model="linear", variogram_parameters=[1.0, 0.1],
                                           coordinates_type="geographic"))
    with pytest.raises(ValueError, match="geographic"):
        geo.execute_block_window("points", np.array([10.0]), np.array([40.0]), 0.5, 4)


def test_the_universal_classes_have_no_moving_window():
    for cls, obj, pts in ch._objects():
        if cls in ORDINARY:
            continue
        for backend in ("loop", "vectorized"):
            with pytest.raises(ValueError, match="moving window"):
                obj.execute_block_window("points", *pts, 0.1, 4, backend=backend)
        with pytest.raises(ValueError, match="moving window"):
            obj.execute_block_window("grid", *pts, 0.1, 4, n_disc=2)


def test_a_device_group_is_refused_before_the_device_is_touched():
    class Group:
        n_devices = 2

    for cls, obj, pts in ch._objects():
        if cls not in ORDINARY:
            continue
        obj._handle = Group()
        try:
            with pytest.raises(ValueError, match="device group of 2"):
                obj.execute_block_window("points", *pts, 0.1, 4)
        finally:
            obj._handle = None


# ------------------------------------------------------------------------------------------------------------- the library
def test_library_declares_and_exports_mik_predict_block_window_at_abi_9():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert lib.mik_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert hasattr(lib, "mik_predict_block_window") and "mik_predict_block_window" in _lib.SIGNATURES
    assert callable(getattr(_lib.Handle, "predict_block_window", None))
    header = open(os.path.join(ROOT, "include", "mikrige.h")).read()
    assert "#define MIK_ABI_VERSION 9" in " ".join(header.split())
    assert ("int  mik_predict_block_window(mik_handle *h, const double *offsets /* nd x ndim, ADJUSTED */, int nd, int n_closest_points);"
            in header)
    assert "mik_predict_block_window" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_predict_block_window" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_a_library_without_the_symbol_is_answered_as_stale(monkeypatch):
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == "mik_predict_block_window":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mik_predict_block_window.*rebuild"):
        _lib.load()


# ------------------------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("name", sorted(mb.CASES))
def test_the_float64_restatement_of_the_stages_is_inside_the_bars(name):
    _, st, k, _, ctr, bsize, n_disc = mb.case(name)
    assert mb.tie_free(st, mb.adjusted(st, ctr), (k,))
    ref = mb.reference(name)
    rz, rs = mb.worst_ratios(ref, *mb.restatement(st, k, ctr, bsize, n_disc))
    print("%s: k %d  worst cond_1 %.3g  err / bar z %.3g sigma^2 %.3g" % (name, k, float(ref.cond.max()), rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)
    assert st.exact_values
    if name == mb.INEXACT:
        _, st2 = mb.inexact_twin(mb.CASES[name][0])
        ref2 = mb.reference(name, exact=False)
        rz, rs = mb.worst_ratios(ref2, *mb.restatement(st2, k, ctr, bsize, n_disc))
        print("%s, exact_values=False: err / bar z %.3g sigma^2 %.3g" % (name, rz, rs))
        assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)
        # the centre node of a station-centred block is an exact hit: the two references differ there
        on = list(mb.ON_STATION)
        assert np.all(np.abs(ref.z[on] - ref2.z[on]) > 0)


def test_k_equal_n_is_the_global_block_kriging():
    _, st, k, ctr, bsize, n_disc, gref = mb.k_is_n()
    rz, rs = mb.worst_ratios(gref, *mb.restatement(st, k, ctr, bsize, n_disc))
    print("k = N = %d: err / bar z %.3g sigma^2 %.3g against the global reference" % (k, rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (rz, rs)
    # and the window reference is the global one, to the bars
    wref = mb.window_reference(st, k, ctr, bsize, n_disc)
    rz, rs = mb.worst_ratios(gref, wref.z.astype(np.float64), wref.ss.astype(np.float64))
    assert rz <= 1.0 and rs <= 1.0, (rz, rs)


def test_n_disc_one_is_the_point_problem_and_blocks_lower_the_variance():
    from oracle import exact_kriging as ek

    name = "exponential_n300_k10_3x3"
    _, st, k, _, ctr, bsize, _ = mb.case(name)
    pt = ek.exact_moving_window(st, mb.adjusted(st, ctr), k)
    one = mb.window_reference(st, k, ctr, bsize, (1, 1))
    assert np.all(np.abs(one.z - pt.z) <= 1e-17) and np.all(np.abs(one.ss - pt.ss) <= 1e-17)
    ref = mb.reference(name)
    off = [q for q in range(len(ctr)) if q not in mb.ON_STATION]
    assert np.all(ref.ss[off] < pt.ss[off])
