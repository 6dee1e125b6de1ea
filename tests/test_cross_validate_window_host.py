"""cross_validate_window() without a GPU: the entry point exists in the built library, the loader answers a library without it as stale,
every argument error is raised before a handle is touched, the docstring states the semantics, cross_validate(n_closest_points=...) is what
it was, and the reference helper of tests/_cvw_cases.py is the definition it stands for."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from oracle import exact_kriging as ek
from tests import _cv_cases as cv
from tests import _cvw_cases as cw

CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_mik_cross_validate_window():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert hasattr(lib, "mik_cross_validate_window")
    assert _lib.SIGNATURES["mik_cross_validate_window"] == _lib.SIGNATURES["mik_cross_validate"]  # mik_cross_validate's shape
    assert callable(getattr(_lib.Handle, "cross_validate_window", None))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_cross_validate_window" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "mikrige.h")).read()
    assert re.search(r"int\s+mik_cross_validate_window\(mik_handle \*h, int n_closest_points, double \*zhat_out[^,]*, double \*ss_out[^)]*\);", header)


def test_a_library_without_the_symbol_is_answered_as_stale(monkeypatch):
    """The symbol came without a version step: a library from before it reports the same ABI version and must end in the rebuild message."""
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == "mik_cross_validate_window":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mik_cross_validate_window.*rebuild"):
        _lib.load()


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def _objects(n=20, **extra):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1], **extra)
    return [(cls, _no_device(cls(*((x, y, z) if "3D" in cls.__name__ else (x, y)), v, **kw))) for cls in CLASSES]


def test_argument_order_and_errors_on_all_four_classes():
    n = 20
    for cls, obj in _objects(n):
        universal = "Universal" in cls.__name__
        # 1. the backend rules of a moving window, n_closest_points <= 1 first
        for k in (1, 0, -2):
            with pytest.raises(ValueError, match="at least two"):
                obj.cross_validate_window(k)
        with pytest.raises(ValueError, match="not supported"):
            obj.cross_validate_window(5, backend="cuda")
        with pytest.raises(ValueError, match="not supported"):
            obj.cross_validate_window(5, None, "vectorized")  # (n_closest_points, values, backend): no window on the vectorized backend
        if universal:  # no moving window at all: the default backend raises, before the values are looked at
            with pytest.raises(ValueError, match="for a moving window is not supported"):
                obj.cross_validate_window(5)
            with pytest.raises(ValueError, match="for a moving window is not supported"):
                obj.cross_validate_window(5, np.zeros(n + 1))
            continue
        # 2. the values
        with pytest.raises(ValueError, match="rows"):
            obj.cross_validate_window(5, np.zeros(n + 1))
        with pytest.raises(ValueError, match="rows"):
            obj.cross_validate_window(n, values=np.zeros(n + 1))  # before the window limit
        with pytest.raises(ValueError, match="non-finite"):
            obj.cross_validate_window(5, values=np.full(n, np.nan))
        with pytest.raises(ValueError, match="F = 0"):
            obj.cross_validate_window(5, values=np.zeros((n, 0)))
        with pytest.raises(ValueError, match="at least two"):
            obj.cross_validate_window(1, values=np.zeros(n + 1))  # the backend rules before the values
        # 3. the window against the N - 1 other stations
        for k in (n, n + 5):
            with pytest.raises(ValueError, match=r"other stations \(N - 1 = %d\)" % (n - 1)):
                obj.cross_validate_window(k)
        with pytest.raises(ValueError, match="n_closest_points"):
            obj.cross_validate_window(None)
        # everything passed: the next thing is the device
        for k, be in ((n - 1, "loop"), (2, "loop"), (5, "hip")) + (((5, "C"),) if cls is pa.OrdinaryKriging else ()):
            with pytest.raises(AssertionError, match="device was touched"):
                obj.cross_validate_window(k, backend=be)
    # pseudo_inv plays no part, as in execute() with a window
    for cls, obj in _objects(n, pseudo_inv=True):
        if "Universal" not in cls.__name__:
            with pytest.raises(AssertionError, match="device was touched"):
                obj.cross_validate_window(5)


def test_the_docstring_names_the_semantics():
    for cls in CLASSES:
        doc = cls.cross_validate_window.__doc__
        for s in ("k nearest OTHER stations", "other N - 1 stations", "n_closest_points=k", "by its index, never by its distance", "coincident",
                  "its value is then the answer", "``sigmasq`` is 0", "not fitted again", "``pseudo_inv`` plays no part", "(F, N)", "N - 1",
                  "global form", "last_timing", "custom"):
            assert s in doc, (cls.__name__, s)
        assert "cross_validate_window(n_closest_points)" in cls.cross_validate.__doc__


def test_cross_validate_with_a_window_still_raises_not_implemented():
    for cls, obj in _objects():
        if "Universal" in cls.__name__:
            with pytest.raises(ValueError, match="moving window"):
                obj.cross_validate(n_closest_points=5, backend="loop")
        else:
            with pytest.raises(NotImplementedError, match="n_closest_points"):
                obj.cross_validate(n_closest_points=5, backend="loop")


def test_the_kernels_leave_the_query_out_by_index():
    """The two neighbour searches carry the compile-time SELF and compare station indices, and KnnArgs ends with the self list (the offsets of
    the fields before it stay where execute()'s kernels read them)."""
    src = open(os.path.join(ROOT, "pykrige_amd", "csrc", "mik_k_mw.h")).read()
    assert "template <int NDIM, int KMAX, bool SELF>" in src and "template <int NDIM, bool SELF>" in src
    args = src[src.index("struct KnnArgs {"):]
    args = args[:args.index("};")]
    members = [ln.split("//")[0].strip() for ln in args.splitlines()[1:] if ln.split("//")[0].strip()]
    assert members[-1] == "const int* self;" and members[-2] == "int* todo_count;", members[-3:]
    assert "(!SELF || st != me)" in src and "(!SELF || id[u] != me)" in src


def test_the_reference_helper_is_the_definition():
    """reference() cuts the local systems out of ONE long-double matrix of all stations; entry i must be exact_moving_window on the state
    without station i, to the last bit of the extended type (all 12 stations at k = N - 1, five of the coincident-pair set)."""
    for name, which in (("exponential_n12_k11", range(12)), ("pair_exact_k8", (0, 17, 59, 60, 61))):
        _, st, k, _ = cw.case(name)
        ref = cw.reference(name)
        for i in which:
            r = ek.exact_moving_window(cv.without(st, i), st.coords_adj[i:i + 1], k)
            assert r.z[0] == ref.z[i] and r.ss[0] == ref.ss[i] and r.cond[0] == ref.cond[i], (name, i)
            assert r.vscale[0] == ref.vscale[i] and r.bscale[0] == ref.bscale[i] and ref.order[i] == k + 1


def test_station_sets_have_no_tie_at_their_windows_and_the_pair_is_isolated():
    for sname in ("ok2d_exponential_n12", "pair_exact", "pair_inexact", "geographic_ok_n200"):
        _, st = cw.station_set(sname)
        assert cw.no_ties(st, cw.SETS[sname][2])
    _, st = cw.station_set("pair_exact")
    a, b = cw.PAIR
    for i in range(st.n):  # no third station's window holds one of the pair; each of the pair holds the other
        _, idx = ek.neighbours(cv.without(st, i), st.coords_adj[i:i + 1], 8)
        idx = idx[0] + (idx[0] >= i)
        if i in (a, b):
            assert (b if i == a else a) in idx and i not in idx
        else:
            assert a not in idx and b not in idx
