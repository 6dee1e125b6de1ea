"""execute_fields_window() without a GPU: the entry point is declared, exported and in the ctypes table, every refusal is raised with its
type before a handle is touched, the universal classes raise as for any moving window, the two old refusals are what they were, and the
reference and the seeds of tests/_fwg_cases.py are what that file says."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from oracle import exact_kriging as ek
from tests import _fwg_cases as fw
from tests.test_fields_gaps_host import adjusted

CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_declares_and_exports_mik_predict_window_gaps():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    C = _lib.C
    assert hasattr(lib, "mik_predict_window_gaps")
    assert _lib.SIGNATURES["mik_predict_window_gaps"] == (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), _lib._dp, _lib._dp])
    assert callable(getattr(_lib.Handle, "predict_window_gaps", None))
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_predict_window_gaps" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "mikrige.h")).read()
    assert re.search(r"int\s+mik_predict_window_gaps\(mik_handle \*h, int n_closest_points, const uint8_t \*valid /\*[^*]*\*/,\s*double \*z_out /\*[^*]*\*/, "
                     r"double \*ss_out /\*[^*]*\*/\);", header)
    assert "mik_predict_window_gaps" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_a_library_without_the_symbol_is_answered_as_stale(monkeypatch):
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == "mik_predict_window_gaps":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mik_predict_window_gaps.*rebuild"):
        _lib.load()


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def _objects(n=20, **extra):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    kw = dict(dict(variogram_model="linear", variogram_parameters=[1.0, 0.1]), **extra)
    return [(cls, _no_device(cls(*((x, y, z) if "3D" in cls.__name__ else (x, y)), v, **kw))) for cls in CLASSES]


def _call(cls, obj, style, values, k, **kw):
    p = np.array([0.2, 0.4])
    axes = (p, p, p) if "3D" in cls.__name__ else (p, p)
    return obj.execute_fields_window(style, *axes, values, k, **kw)


def test_every_refusal_is_raised_with_its_type_before_the_device_is_touched():
    n = 20
    v = np.zeros((n, 3))
    for cls, obj in _objects(n):
        with pytest.raises(ValueError, match="masked"):
            _call(cls, obj, "masked", v, 5)
        with pytest.raises(ValueError, match="style argument"):
            _call(cls, obj, "mesh", v, 5)
        with pytest.raises(ValueError, match="needs n_closest_points"):
            _call(cls, obj, "points", v, None)
        for k in (1, 0, -3):
            with pytest.raises(ValueError, match="at least two"):
                _call(cls, obj, "points", v, k)
        with pytest.raises(ValueError, match="not supported"):
            _call(cls, obj, "points", v, 5, backend="cuda")
        with pytest.raises(ValueError, match="not supported"):
            _call(cls, obj, "points", v, 5, backend="vectorized")  # as the existing window calls treat it
        if "Universal" in cls.__name__:  # no moving window at all, exactly as execute_block_window raises there
            with pytest.raises(ValueError, match="for a moving window is not supported") as e1:
                _call(cls, obj, "points", v, 5)
            p = np.array([0.2, 0.4])
            with pytest.raises(ValueError, match="for a moving window is not supported") as e2:
                obj.execute_block_window("points", *((p, p, p) if "3D" in cls.__name__ else (p, p)), 0.1, 5)
            assert str(e1.value) == str(e2.value)
            continue
        # the values and valid: _field_values / _field_gaps
        with pytest.raises(ValueError, match="rows"):
            _call(cls, obj, "points", np.zeros(n + 1), 5)
        with pytest.raises(ValueError, match="non-finite"):
            _call(cls, obj, "points", np.full(n, np.nan), 5)
        with pytest.raises(ValueError, match="boolean"):
            _call(cls, obj, "points", v, 5, valid=np.ones((n, 3), dtype=np.int8))
        with pytest.raises(ValueError, match="valid has shape"):
            _call(cls, obj, "points", v, 5, valid=np.ones((n, 2), dtype=bool))
        with pytest.raises(ValueError, match="valid has shape"):
            _call(cls, obj, "points", np.zeros(n), 5, valid=np.ones((n, 1), dtype=bool))
        m = np.ones((n, 3), dtype=bool)
        m[4, 1] = False
        bad = v.copy()
        bad[6, 2] = np.inf
        with pytest.raises(ValueError, match="non-finite entries where valid is True"):
            _call(cls, obj, "points", bad, 5, valid=m)
        # fewer than k valid stations: the first such field is named; without valid the bound is N
        m[:, 2] = False
        m[:4, 2] = True
        m[:, 1] = False
        with pytest.raises(ValueError, match="field 1 has 0 valid stations, fewer than n_closest_points = 5"):
            _call(cls, obj, "points", v, 5, valid=m)
        m[:, 1] = True
        with pytest.raises(ValueError, match="field 2 has 4 valid stations"):
            _call(cls, obj, "points", v, 5, valid=m)
        with pytest.raises(ValueError, match="field 0 has %d valid stations" % n):
            _call(cls, obj, "points", v, n + 1)
        # everything passed (ignored entries may be NaN or inf): the next thing is the device
        ok = v.copy()
        ok[~m] = np.nan
        for kw in (dict(valid=m), dict(), dict(valid=None, backend="loop")) + ((dict(backend="C"),) if cls is pa.OrdinaryKriging else ()):
            with pytest.raises(AssertionError, match="device was touched"):
                _call(cls, obj, "grid", ok if "valid" in kw and kw["valid"] is not None else v, 4, **kw)
    # a custom variogram: NotImplementedError; pseudo_inv plays no part
    for cls, obj in _objects(n, variogram_model="custom", variogram_parameters=[1.0], variogram_function=lambda p, d: p[0] * d):
        if "Universal" not in cls.__name__:
            with pytest.raises(NotImplementedError, match="custom"):
                _call(cls, obj, "points", v, 5)
    for cls, obj in _objects(n, pseudo_inv=True):
        if "Universal" not in cls.__name__:
            with pytest.raises(AssertionError, match="device was touched"):
                _call(cls, obj, "points", v, 5)


def test_a_handle_that_spans_a_device_group_is_refused():
    class Group:
        n_devices = 2

    for cls, obj in _objects():
        if "Universal" in cls.__name__:
            continue
        obj._handle = Group()
        with pytest.raises(ValueError, match="device group of 2 devices"):
            _call(cls, obj, "points", np.zeros(20), 5)
        obj._handle = None


def test_execute_fields_with_window_and_valid_still_raises_not_implemented():
    n = 20
    for cls, obj in _objects(n):
        if "Universal" in cls.__name__:
            continue
        p = np.array([0.2, 0.4])
        axes = (p, p, p) if "3D" in cls.__name__ else (p, p)
        with pytest.raises(NotImplementedError, match="the moving window with gaps"):
            obj.execute_fields("points", *axes, np.zeros(n), backend="loop", n_closest_points=5, valid=np.ones(n, dtype=bool))
    src = open(os.path.join(ROOT, "pykrige_amd", "csrc", "mikrige.hip")).read()
    assert 'if (h->gaps_any) return fail(MIK_EINVAL, "mik_predict_moving_window: fields with gaps' in src  # (on the device: tests/test_fields_window_gaps.py)


def test_the_docstring_names_the_semantics():
    for cls in CLASSES:
        doc = cls.execute_fields_window.__doc__
        for s in ("valid[:, f]", "(F,) + shape", "bit for bit", "share the bits", "No factor is needed", "buffers of its own", "NotImplementedError",
                  "naming the first such field", "7936", "device group", "station index"):
            assert s in doc, (cls.__name__, s)


def test_the_masked_search_is_a_compile_time_form_of_the_two_search_kernels():
    """The mask rides on NDIM (dimension + MIK_MW_LIVE), the flag sits beside orig in KnnArgs, and a dead station is dropped where a
    candidate is taken -- in the lane kernel (whose masked form the header keeps, the library does not instantiate) through the negative id
    staged in LDS."""
    src = open(os.path.join(ROOT, "pykrige_amd", "csrc", "mik_k_mw.h")).read()
    args = src[src.index("struct KnnArgs {"):]
    args = args[:args.index("};")]
    members = [ln.split("//")[0].strip() for ln in args.splitlines()[1:] if ln.split("//")[0].strip()]
    assert members[members.index("const int* orig;") + 1] == "const unsigned char* live;"
    assert src.count("constexpr bool LIVE = (NDIM & MIK_MW_LIVE) != 0;") == 2
    assert "sid[l] = (LIVE && !a.live[j]) ? -1 : a.orig[j];" in src and "(!LIVE || st >= 0)" in src and "(!LIVE || lv[u])" in src
    host = open(os.path.join(ROOT, "pykrige_amd", "csrc", "mik_mw.hip")).read()
    assert "k_mw_knn<2 + MIK_MW_LIVE, false>" in host and "k_mw_knn<3 + MIK_MW_LIVE, false>" in host
    assert "MIK_MW_LIVE, true>" not in host and "MIK_MW_LIVE, 16, true>" not in host  # no form with both exclusions
    # the masked lane forms are not in the library (its size bar): a masked job runs without the lane pass
    assert "k_mw_knn_lane<2 + MIK_MW_LIVE" not in host and "k_mw_knn_lane<3 + MIK_MW_LIVE" not in host and "J.lane && !J.live;" in host
    assert "if (J.self || J.live) return fail(MIK_EINVAL" in host  # the list scan in HBM gets no masked form


def test_every_station_set_finds_a_tie_free_seed_within_twenty_draws():
    for sname, spec in fw.SETS.items():
        d = fw.station_set(sname)  # raises if 20 draws were not enough
        assert fw.tie_free(d.st, d.valid, adjusted(d.st, d.pts), spec[2])
        assert np.isnan(d.values[~d.valid]).all() and np.isfinite(d.values[d.valid]).all()
        assert d.pts.shape[0] == fw.N_RANDOM + 6
        gap = next(f for f in range(d.valid.shape[1]) if not d.valid[:, f].all())
        assert all(d.valid[i, gap] for i in d.on_valid) and not any(d.valid[i, gap] for i in d.on_missing)
        assert np.array_equal(adjusted(d.st, d.pts[-6:]), d.st.coords_adj[list(d.on_valid + d.on_missing)])  # exactly on the stations
    d = fw.station_set("ok2d_exponential_n300")
    assert d.valid[:, 0].all() and 30 <= int((~d.valid[:, 2]).sum()) <= 50  # the disc empties a neighbourhood
    assert int(fw.station_set("ok2d_exponential_n12").valid[:, 0].sum()) == 8


def test_the_reference_on_a_subset_state_does_not_depend_on_the_order_of_the_fields():
    d, k, _ = fw.case("exponential_n12_k8")
    pa_ = adjusted(d.st, d.pts[:25])
    rng = np.random.default_rng(3)
    valid = np.stack([d.valid[:, 0], np.ones(d.st.n, dtype=bool), d.valid[:, 0]], axis=1)
    values = rng.standard_normal((d.st.n, 3))

    def refs(order):
        return [ek.exact_moving_window(fw.subset(d.st, valid[:, f], values[:, f]), pa_, k) for f in order]

    a, b = refs([0, 1, 2]), refs([2, 0, 1])
    for f, g in ((0, 1), (1, 2), (2, 0)):
        assert np.array_equal(a[f].z, b[g].z) and np.array_equal(a[f].ss, b[g].ss) and np.array_equal(a[f].cond, b[g].cond)
    assert np.array_equal(a[0].ss, a[2].ss) and not np.array_equal(a[0].ss, a[1].ss)  # one pattern, one sigma^2
    sub = fw.subset(d.st, valid[:, 0], values[:, 0])
    assert sub.n == 8 and np.array_equal(sub.coords_adj, d.st.coords_adj[valid[:, 0]]) and np.array_equal(sub.values, values[valid[:, 0], 0])
