"""vecchia_grad.VecchiaGradPlan / neg_log_likelihood_vecchia_grad / fit_variogram_vecchia_grad without a GPU: the build yields a
seventh library from a second list while build.LIBRARIES keeps its six records, include/mikvgrad.h declares what libmikvgrad.so exports
and the ctypes mirror agrees, the exported kernels are the three k_vec_* and the two k_vgrad_* families and the six other libraries hold
nothing of the seventh, every refusal comes with its reason before anything is loaded, the long-double reference of
tests/_vgrad_cases.py agrees with central differences of the long-double Vecchia objective, a float64 NumPy restatement of the device
algorithm is inside the bar the device is held to on every GPU case, ``nll_grad_from_gram`` is the derivative of ``nll_from_gram``, and
the quasi-Newton search runs on that restatement."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import likelihood as lk
from pykrige_amd import vecchia as vc
from pykrige_amd import vecchia_grad as vgd
from tests import _vecchia_cases as vcs
from tests import _vgrad_cases as vg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------- the library
def _declared():
    text = open(os.path.join(ROOT, "include", "mikvgrad.h")).read()
    verbatim = " ".join(text.split()).replace(" * ", " ")
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return verbatim, text, sorted(set(re.findall(r"\b(mvg_[a-z_0-9]+)\s*\(", text)))


def test_the_build_yields_a_seventh_library_and_the_table_keeps_its_six_records():
    from pykrige_amd import build

    build.build_library()
    assert len(build.LIBRARIES) == 6 and [os.path.basename(lib.out) for lib in build.EXTRA_LIBRARIES] == ["libmikvgrad.so"]
    lib = build.EXTRA_LIBRARIES[0]
    assert os.path.exists(build.OUT_VGRAD) and build.OUT_VGRAD == lib.out == vgd.LIB_PATH and build.API_VGRAD == lib.api
    assert build.API_VGRAD == os.path.join(ROOT, "include", "mikvgrad.h") and lib.units is build.UNITS_VGRAD and lib.tail == ["-Wl,-s"]
    assert build.UNITS_VGRAD == {"mik_vgrad": ("mik_vgrad.hip", ["mik_k_vgrad.h", "mik_k_vecchia.h"])} and lib.common == []
    csrc = os.path.join(ROOT, "pykrige_amd", "csrc")
    assert build.vgrad_deps("mik_vgrad") == lib.deps("mik_vgrad") == [os.path.join(csrc, f) for f in (
        "mik_vgrad.hip", "mik_k_vgrad.h", "mik_k_vecchia.h")] + [build.API_VGRAD]
    assert "libmikvgrad.so" in build.__doc__ and "EXTRA_LIBRARIES" in build.__doc__
    assert not any("vgrad" in os.path.basename(d) for six in build.LIBRARIES for d in six.sources())
    assert build.up_to_date()
    plain = lambda flags: [c for c in flags if c not in build.COMPRESS and not c.startswith("-I")]
    assert plain(open(os.path.join(build.OBJ, "mik_vgrad.flags")).read().split()) == plain(build.FLAGS)
    old = os.path.getmtime(build.OUT_VGRAD)  # up_to_date() sees the seventh library: a library older than its header is stale
    try:
        os.utime(build.OUT_VGRAD, (1.0, 1.0))
        assert not build.up_to_date()
    finally:
        os.utime(build.OUT_VGRAD, (old, old))
    assert build.up_to_date()
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "vecchia_grad.load()" in text and "OUT_VGRAD" in text
    assert subprocess.run(["git", "check-ignore", "-q", build.OUT_VGRAD], cwd=ROOT).returncode in (0, 128)
    hip, hdr = open(os.path.join(csrc, "mik_vgrad.hip")).read(), open(os.path.join(csrc, "mik_k_vgrad.h")).read()
    # no code of the other libraries but the sixth's kernel header; no atomics, no inline assembly
    assert re.findall(r'#include "([^"]+)"', hdr) == ["mik_k_vecchia.h"]
    assert re.findall(r'#include "([^"]+)"', hip) == ["mik_k_vgrad.h", "../../include/mikvgrad.h"]
    for text in (hip, hdr):
        for word in ("atomic", "asm"):
            assert word not in text.replace("no atomic", ""), word
    assert '#include "mik_k_vecchia.h"' in hdr and "namespace mvg" in hdr and hdr.count("#pragma clang fp contract(off)") >= 3
    assert "static_assert" in hdr and "static_assert" in hip and "163840" in hdr and "163840" in hip


def test_the_header_declares_what_the_library_exports_and_the_ctypes_mirror_agrees():
    from pykrige_amd import build

    build.build_library()
    verbatim, text, names = _declared()
    assert names == sorted(vgd.SIGNATURES) == ["mvg_abi_version", "mvg_last_error", "mvg_plan_create", "mvg_plan_destroy", "mvg_plan_grad",
                                               "mvg_plan_neighbours"]
    for phrase in ("bit for bit mvc_plan_gram's", "beta = S^-1 s, u = [-beta ; 1], d_p = sigma - s^T beta", "r_p(w) = u^T [w_c ; w_p]",
                   "t = D u", "d_k d_p = u^T t", "d_k r_p(w) = -(S^-1 w_c)^T t_c = -(L^-1 w_c)^T (L^-1 t_c)",
                   "dlogdet[k] = sum_p d_k d_p / d_p",
                   "dG[k][a][b] = sum_p [ (d_k r_p(a) r_p(b) + r_p(a) d_k r_p(b)) / d_p - r_p(a) r_p(b) d_k d_p / d_p^2 ]",
                   "((dr_a r_b) + (r_a dr_b)) / d - ((r_a r_b) dd) / (d d)", "exactly symmetric", "A position with k_p = 0",
                   "beyond the range every derivative is exactly 0", "c_p = 1, c_r = 0 and c_g = 0", "MVG_ENOTPD",
                   "1-based station index of the earliest such position", "writes none of its results",
                   "fixed order that depends on n only", "there are no atomics", "depends only on columns a and b",
                   "a quarter of the device's memory", "ceil(n / 1024) 8 9 821 + 65536 8 8 41 bytes"  # (the reader drops the comment's " * ")
                   ,
                   "(3 + ng) (m_cols + 1) doubles", "no partial sum sees the cut", "MIK_VGRAD_SLAB"):
        assert phrase in verbatim, phrase
    lib = vgd.load()
    assert lib.mvg_abi_version() == vgd.ABI_VERSION == int(re.search(r"#define MVG_ABI_VERSION (\d+)", text).group(1)) == 1
    for macro, value in (("MVG_MAXNB", vc.MAXNB), ("MVG_MAXCOLS", lk.MAXCOLS), ("MVG_MAXGEOM", lk.MAXGEOM), ("MVG_SLAB", 65536),
                         ("MVG_EINVAL", "(-1)"), ("MVG_ENOTPD", "(-2)"), ("MVG_EHIP", "(-3)"), ("MVG_GAUSSIAN", 0), ("MVG_EXPONENTIAL", 1),
                         ("MVG_SPHERICAL", 2), ("MVG_HOLE_EFFECT", 3)):
        assert re.search(r"#define %s %s(?=\s)" % (macro, re.escape(str(value))), text), macro
    assert (vgd.MVG_EINVAL, vgd.MVG_ENOTPD, vgd.MVG_EHIP) == (-1, -2, -3)
    ctype = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "const double *": vgd._dp,
             "double *": vgd._dp, "int32_t *": vgd._i32p, "const int32_t *": vgd._i32p, "mvg_plan *": vgd._plan_p,
             "const mvg_plan *": vgd._plan_p, "mvg_plan **": ctypes.POINTER(vgd._plan_p)}
    flat = " ".join(text.split())
    for name, res in (("mvg_plan_create", "int"), ("mvg_plan_neighbours", "int"), ("mvg_plan_grad", "int"), ("mvg_plan_destroy", "void")):
        args = re.search(r"%s %s\((.*?)\);" % (res, name), flat).group(1).split(",")
        want = [ctype[re.match(r"\s*((?:const )?\w+ \*+|\w+)", a).group(1)] for a in args]
        assert vgd.SIGNATURES[name] == (ctypes.c_int if res == "int" else None, want), name
    assert len(vgd.SIGNATURES["mvg_plan_grad"][1]) == 15 and vgd.SIGNATURES["mvg_plan_create"] == vc.SIGNATURES["mvc_plan_create"]
    if shutil.which("nm"):
        from pykrige_amd import build

        out = subprocess.run(["nm", "-D", "-C", build.OUT_VGRAD], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert {e for e in exported if e.startswith("mvg_")} == set(names)
        kernels = sorted({m.group(1) for m in re.finditer(r"__device_stub__([A-Za-z_0-9]+)[<(]", out)})
        assert kernels == ["k_vec_knn", "k_vec_reduce", "k_vec_solve", "k_vgrad_reduce", "k_vgrad_solve"], kernels
        for other in (lib.out for lib in build.LIBRARIES):  # nothing of the seventh in the six others
            sym = subprocess.run(["nm", "-D", "-C", other], capture_output=True, text=True, check=True).stdout
            assert "mvg_" not in sym and "k_vgrad" not in sym, other
        for word in ("mkv_", "mkv3_", "mlk_", "mlg_", "mvc_", "k_vario", "k_lik", "k_grad", "mik_"):  # nor the reverse
            assert word not in out, word


def test_every_refusal_of_the_library_comes_with_its_reason_and_writes_nothing():
    lib = vgd.load()
    p = lambda a: a.ctypes.data_as(vgd._dp)
    c, o = np.array([0.0, 1.0, 2.0, 0.0, 1.0, 0.5]), np.array([2, 0, 1], dtype=np.int32)
    handle = vgd._plan_p(7)

    def create(n=3, ndim=2, coords=c, order=o, m=2):
        return lib.mvg_plan_create(0, n, ndim, p(coords), order.ctypes.data_as(vgd._i32p), m, ctypes.byref(handle))

    for kw, reason in ((dict(n=1), b"two stations"), (dict(ndim=4), b"ndim"), (dict(ndim=1), b"ndim"), (dict(m=0), b"MVG_MAXNB"),
                       (dict(m=65), b"MVG_MAXNB"), (dict(n=2 ** 31), b"fits no device"),
                       (dict(coords=np.array([0.0, np.nan, 2.0, 0.0, 1.0, 0.5])), b"coordinates must be finite"),
                       (dict(coords=np.array([0.0, 1.0, 2.0, 0.0, np.inf, 0.5])), b"coordinates must be finite"),
                       (dict(order=np.array([0, 1, 1], dtype=np.int32)), b"permutation"), (dict(order=np.array([0, 1, 3], dtype=np.int32)), b"permutation"),
                       (dict(order=np.array([-1, 1, 2], dtype=np.int32)), b"permutation")):
        handle.value = 7
        assert create(**kw) == vgd.MVG_EINVAL and reason in lib.mvg_last_error(), (kw, lib.mvg_last_error())
        assert not handle.value  # no plan
    assert lib.mvg_plan_create(0, 3, 2, None, o.ctypes.data_as(vgd._i32p), 2, ctypes.byref(handle)) == vgd.MVG_EINVAL
    assert b"NULL argument" in lib.mvg_last_error()
    # mvg_plan_grad checks what it can before it looks at the plan: these refusals need neither a plan nor a GPU
    w, g, dl, dg, e = np.ones(3), np.full(4, 7.0), np.full(8, 7.0), np.full(32, 7.0), np.zeros(12)
    logdet, info = ctypes.c_double(7.0), ctypes.c_int32(5)

    def grad(model=1, psill=1.0, rng=0.5, nugget=0.1, m_cols=1, coords=c, ng=2, dcoords=e, dlogdet=dl):
        return lib.mvg_plan_grad(None, None if coords is None else p(coords), ng, None if dcoords is None else p(dcoords), model, psill, rng,
                                 nugget, p(w), m_cols, ctypes.byref(logdet), p(g), None if dlogdet is None else p(dlogdet), p(dg),
                                 ctypes.byref(info))

    for kw, reason in ((dict(coords=None), b"NULL argument"), (dict(dlogdet=None), b"NULL argument"), (dict(m_cols=0), b"MVG_MAXCOLS"),
                       (dict(m_cols=41), b"MVG_MAXCOLS"), (dict(ng=-1), b"MVG_MAXGEOM"), (dict(ng=6), b"MVG_MAXGEOM"),
                       (dict(dcoords=None), b"NULL only when ng = 0"), (dict(model=4), b"model"), (dict(model=-1), b"model"),
                       (dict(psill=0.0), b"psill > 0"), (dict(rng=-1.0), b"range > 0"), (dict(nugget=-0.5), b"nugget >= 0"),
                       (dict(psill=float("inf")), b"finite"), (dict(rng=float("nan")), b"finite"), ({}, b"NULL plan"),
                       (dict(ng=0, dcoords=None), b"NULL plan")):
        assert grad(**kw) == vgd.MVG_EINVAL and reason in lib.mvg_last_error(), (kw, lib.mvg_last_error())
    assert logdet.value == 7.0 and np.all(g == 7.0) and np.all(dl == 7.0) and np.all(dg == 7.0)  # a refused call writes no result
    assert lib.mvg_plan_neighbours(None, None) == vgd.MVG_EINVAL and b"NULL argument" in lib.mvg_last_error()
    lib.mvg_plan_destroy(None)  # harmless


def test_a_missing_or_stale_library_is_answered_as_the_others_are(monkeypatch):
    monkeypatch.setattr(vgd, "_lib", None)
    monkeypatch.setattr(vgd, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    with pytest.raises(ImportError, match=r"is missing -- build it with `python -m pykrige_amd.build`"):
        vgd.load()
    monkeypatch.undo()
    real = vgd.load()

    class Old:
        def __getattr__(self, name):
            if name == "mvg_plan_grad":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(vgd, "_lib", None)
    monkeypatch.setattr(vgd.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mvg_plan_grad.*rebuild"):
        vgd.load()


def test_the_module_loads_through_open_library(monkeypatch):
    from pykrige_amd import _dl

    calls = []
    monkeypatch.setattr(_dl, "open_library", lambda *a: calls.append(a) or "the library")
    monkeypatch.setattr(vgd, "_lib", None)
    monkeypatch.setattr(vgd, "LIB_PATH", "/somewhere/else.so")
    assert vgd.load() == "the library" and vgd.load() == "the library" and len(calls) == 1
    assert calls[0] == ("/somewhere/else.so", "mvg", vgd.ABI_VERSION, vgd.SIGNATURES)


# ------------------------------------------------------------------------------------------------------------- the interface
def test_signatures_and_docstrings():
    sig = inspect.signature(vgd.VecchiaGradPlan.__init__).parameters
    assert list(sig) == ["self", "coords", "m", "order", "seed"] and (sig["m"].default, sig["order"].default, sig["seed"].default) == (30, "random", 0)
    assert list(inspect.signature(vgd.VecchiaGradPlan.grad).parameters) == ["self", "coords", "dcoords", "model", "parameters", "W"]
    assert list(inspect.signature(lk.nll_grad_from_gram).parameters) == ["n", "logdet", "G", "dlogdet", "dG", "nfields", "reml", "logdet_xtx"]
    doc = " ".join(vgd.fit_variogram_vecchia_grad.__doc__.split())
    for phrase in ("L-BFGS-B", "one plan built in the start metric", "at most 5000 stations", "Nelder-Mead", "MLFit", "does not raise"):
        assert phrase in doc, phrase
    doc = " ".join(vgd.neg_log_likelihood_vecchia_grad.__doc__.split())
    for phrase in ("m=30, order=\"random\", seed=0, plan=None", "bit for bit", "GRAD_NAMES_2D", "angles per degree", "``inf``", "NaN",
                   "no CPU fallback"):
        assert phrase in doc, phrase
    # the sixth library's entry points stay as they are
    assert "There is no gradient method" in " ".join(vc.fit_variogram_vecchia.__doc__.split())
    for cls in (pa.OrdinaryKriging, pa.OrdinaryKriging3D):
        sig = inspect.signature(cls.neg_log_likelihood_vecchia_grad)
        assert list(sig.parameters) == ["self", "variogram_parameters", "m", "order", "seed", "plan", "reml", "anisotropy"]
        sig = inspect.signature(cls.fit_variogram_vecchia_grad)
        assert list(sig.parameters) == ["self", "m", "order", "seed", "start", "fit_anisotropy", "reml", "bounds", "anisotropy"]
        for fn in (cls.neg_log_likelihood_vecchia_grad, cls.fit_variogram_vecchia_grad):
            doc = " ".join(fn.__doc__.split())
            for phrase in ("regional_linear", "NotImplementedError", "geographic", "device group", "'custom'"):
                assert phrase in doc, (cls.__name__, fn.__name__, phrase)
    assert "vecchia_grad" in pa.__all__ and pa.vecchia_grad is vgd


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    for mod in (vgd, vc):
        monkeypatch.setattr(mod, "_lib", None)
        monkeypatch.setattr(mod, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
        monkeypatch.setattr(mod, "load", boom)
    monkeypatch.setattr(vgd.C, "CDLL", boom)
    monkeypatch.setattr(lk, "load", boom)
    monkeypatch.setattr(lk, "load_grad", boom)


def test_every_refusal_is_raised_before_the_library_is_loaded(no_library):
    rng = np.random.default_rng(0)
    X, v = rng.random((20, 2)), rng.standard_normal(20)
    x, y, z = X[:, 0], X[:, 1], rng.random(20)
    for kw, match in ((dict(coords=X[:, :1]), r"shape \(N, 2\) or \(N, 3\)"), (dict(coords=X[:1]), "two stations"), (dict(m=0), "MVC_MAXNB"),
                      (dict(m=65), "MVC_MAXNB"), (dict(order="maxmin"), "'random', 'coordinate' or a permutation"),
                      (dict(order=np.arange(19)), "permutation"),
                      (dict(coords=np.where(np.arange(40).reshape(20, 2) == 3, np.inf, X)), "coordinates must be finite")):
        with pytest.raises(ValueError, match=match):
            vgd.VecchiaGradPlan(**{"coords": X, **kw})
    plan = vgd.VecchiaGradPlan.__new__(vgd.VecchiaGradPlan)  # a plan without a handle: grad checks its arguments first
    plan._handle, plan.n, plan.ndim, plan.m = None, 20, 2, 5
    par, D = [1.0, 0.5, 0.1], np.zeros((2, 20, 2))
    for args, match in (((X[:10], D, "exponential", par, v), "plan's shape"), ((X, D, "linear", par, v), "unbounded"),
                        ((X, D, "exponential", [0.0, 0.5, 0.1], v), "psill > 0"), ((X, D, "exponential", par, np.zeros((20, 41))), "MVG_MAXCOLS"),
                        ((X, np.zeros((6, 20, 2)), "exponential", par, v), "MVG_MAXGEOM"), ((X, np.zeros((2, 20, 3)), "exponential", par, v), "dcoords"),
                        ((X, np.full((2, 20, 2), np.nan), "exponential", par, v), "dcoords must be finite"),
                        ((X, D, "exponential", par, v), "the plan is closed")):
        with pytest.raises(ValueError, match=match):
            plan.grad(*args)
    full = [1.1, 0.5, 0.1]
    for fn, tail in ((vgd.neg_log_likelihood_vecchia_grad, (full,)), (vgd.fit_variogram_vecchia_grad, ())):
        for args, kw, exc, match in (
                ((x, y, v, "linear") + tail, {}, ValueError, "unbounded"), ((x, y, v, "custom") + tail, {}, NotImplementedError, "custom"),
                ((x, y, v, "cubic") + tail, {}, ValueError, "must be one of"),
                ((x, y, np.where(np.arange(20) == 2, np.inf, v), "exponential") + tail, {}, ValueError, "values must be finite"),
                ((x, y[:-1], v, "exponential") + tail, {}, ValueError, "same length"),
                ((x, y, np.zeros((20, 33)), "exponential") + tail, {}, ValueError, "F <= 32"),
                ((x, y, v, "exponential") + tail, dict(drift=np.ones((20, 1))), ValueError, "rank-deficient"),
                ((x, y, v, "exponential") + tail, dict(drift="quadratic"), ValueError, "regional_linear"),
                ((x, y, v, "exponential") + tail, dict(anisotropy_scaling_z=2.0), ValueError, "3-D classes"),
                ((x, y, z, v, "exponential") + tail, dict(anisotropy_scaling=2.0), ValueError, "2-D classes"),
                ((x, y, v, "exponential") + tail, dict(m=0), ValueError, "MVC_MAXNB"), ((x, y, v, "exponential") + tail, dict(m=65), ValueError, "MVC_MAXNB"),
                ((x, y, v, "exponential") + tail, dict(order="maxmin"), ValueError, "'random', 'coordinate'"),
                ((x, y, v, "exponential") + tail, dict(seed=-1), ValueError, "seed"),
                ((x, y, v, "exponential") + tail, dict(nlags=6), TypeError, "unexpected argument"),
                ((x, y, v, "exponential") + tail, dict(method="l-bfgs-b"), TypeError, "unexpected argument"),
                ((x, y, v), {}, TypeError, "variogram_model is required")):
            with pytest.raises(exc, match=match):
                fn(*args, **kw)
    with pytest.raises(ValueError, match="plan must be a VecchiaGradPlan"):
        vgd.neg_log_likelihood_vecchia_grad(x, y, v, "exponential", full, plan=object())
    with pytest.raises(ValueError, match="constant"):
        vgd.fit_variogram_vecchia_grad(x, y, np.ones(20), "exponential")
    with pytest.raises(ValueError, match="bounds"):
        vgd.fit_variogram_vecchia_grad(x, y, v, "exponential", start=full, bounds={"sill": (0.1, 1.0)})
    kw = dict(variogram_model="exponential", variogram_parameters=full)
    calls = (lambda o: o.neg_log_likelihood_vecchia_grad(), lambda o: o.fit_variogram_vecchia_grad())

    class Group:
        n_devices = 2

    for obj in (pa.OrdinaryKriging(x, y, v, **kw), pa.OrdinaryKriging3D(x, y, z, v, **kw)):
        for call in calls:
            obj._handle = Group()
            try:
                with pytest.raises(ValueError, match="device group of 2"):
                    call(obj)
            finally:
                obj._handle = None
        with pytest.raises(TypeError, match="unexpected argument"):
            obj.neg_log_likelihood_vecchia_grad(nlags=6)
        with pytest.raises(ValueError, match="MVC_MAXNB"):
            obj.fit_variogram_vecchia_grad(m=100)
    for call in calls:
        with pytest.raises(ValueError, match="geographic"):
            call(pa.OrdinaryKriging(360.0 * x, 90.0 * y, v, coordinates_type="geographic", **kw))
        with pytest.raises(ValueError, match="unbounded"):
            call(pa.OrdinaryKriging(x, y, v, variogram_model="linear", variogram_parameters=[1.0, 0.1]))


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", sorted(vg.HOST_CASES))
def test_the_reference_agrees_with_central_differences_of_the_long_double_objective(name):
    """Every entry of the reference's dlogdet and dG against central differences (h = 1e-5) of ``_vecchia_cases.brute_force`` on the
    same order and neighbour lists, relative to the bar's magnitudes, at the 1e-6 of the dense gradient's host test."""
    case = vg.HOST_CASES[name]
    ref = vg.reference(name)
    dl, dG = vg.central_differences(name)
    wl, wg = float(np.max(np.abs(dl - ref[2]) / ref[7])), float(np.max(np.abs(dG - ref[3]) / ref[8]))
    print("%s: worst |central difference - reference| / scale: dlogdet %.3g, dG %.3g" % (name, wl, wg))
    assert ref[2].shape == (3 + case["ng"],) and ref[3].shape == (3 + case["ng"], case["cols"], case["cols"]) and wl <= 1e-6 and wg <= 1e-6
    # logdet and G of the reference are the Vecchia brute force's
    adj, dco, W, order, nbr = vg.problem(name)
    logdet, G = vcs.brute_force(adj, order, nbr, case["model"], case["par"], W)
    assert abs(ref[0] - logdet) <= 1e-15 * case["n"] * abs(logdet) and np.all(np.abs(ref[1] - G) <= 1e-15 * case["n"] * np.abs(G).max())


@pytest.mark.parametrize("name", sorted(vg.CASES))
def test_the_float64_restatement_is_within_the_bar(name):
    """The CPU proof that the bar is reachable: k_vgrad_solve and k_vgrad_reduce in float64 NumPy against the long-double brute force."""
    case = vg.CASES[name]
    adj, dco, W, order, nbr = vg.problem(name)
    got = vg.float64_grad(adj, dco, order, nbr, case["model"], case["par"], W)
    fl, fg = vg.worst(got, name)
    print("%-16s worst kappa_2 %8.3g  |dlogdet - ref| / bar %8.3g  |dG - ref| / bar %8.3g" % (name, vg.reference(name)[6], fl, fg))
    assert vg.reference(name)[6] <= 1e5 and fl <= 1.0 and fg <= 1.0
    assert all(np.array_equal(got[3][k], got[3][k].T) for k in range(3 + case["ng"]))
    logdet6, G6 = vcs.float64_gram(adj, order, nbr, case["model"], case["par"], W)
    assert abs(got[0] - logdet6) <= 1e-12 * abs(logdet6) and np.allclose(got[1], G6, rtol=1e-11, atol=0)


def test_a_coincident_pair_and_a_short_range_keep_the_rules_of_the_header():
    name = "g129_pair"
    adj, dco, W, order, nbr = vg.problem(name)
    k, j = vg.CASES[name]["repeat"]
    assert np.array_equal(adj[k], adj[j]) and (nbr[k][0] == j or nbr[j][0] == k)
    cp, cr, cg = vg._factors("exponential", [1.0, 0.5, 0.1], np.zeros(1), LD)
    assert cp[0] == 1 and cr[0] == 0 and cg[0] == 0
    cp, cr, cg = vg._factors("spherical", [1.0, 0.03, 0.1], np.array([0.03, 0.030000001]), np.float64)
    assert cp[1] == 0 and cr[1] == 0 and cg[1] == 0 and abs(cp[0]) < 1e-15


def test_the_reference_answers_a_matrix_that_is_not_positive_definite():
    from tests import _lik_cases as lc

    case, _ = lc.NOT_PD["notpd_n200"]
    X, W = lc.inputs(case)
    order = np.arange(case["n"], dtype=np.int32)
    nbr = vcs.neighbours_ref(X, order, 5)
    assert vg.pieces(X, np.zeros((2,) + X.shape), order, nbr, case["model"], case["par"], W) == (None, 151)
    assert vg.float64_grad(X, np.zeros((0,) + X.shape), order, nbr, case["model"], case["par"], W) == (None, 151)


# ------------------------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("reml", [False, True])
def test_nll_grad_from_gram_is_the_derivative_of_nll_from_gram(reml):
    """On a random symmetric positive definite G(e) = G + e dG_k with logdet(e) = logdet + e dlogdet_k: the gradient against central
    differences in e of the objective's formula in long double, which agrees with ``nll_from_gram`` itself at e = 0."""
    rng = np.random.default_rng(31)
    F, p, n, K = 3, 2, 50, 4
    A = rng.standard_normal((F + p, 12))
    G = A @ A.T
    dG = rng.standard_normal((K, F + p, F + p))
    dG = dG + dG.transpose(0, 2, 1)
    logdet, dlogdet, xtx = 3.7, rng.standard_normal(K), 1.3

    def objective(Gl, ld):
        Gi = np.linalg.inv(Gl[F:, F:].astype(np.float64)).astype(LD)
        Gi = Gi @ (LD(2) * np.eye(p, dtype=LD) - Gl[F:, F:] @ Gi)  # one Newton step: the inverse in long double
        lgx = np.log(Gl[F, F] * Gl[F + 1, F + 1] - Gl[F, F + 1] * Gl[F + 1, F])
        log_two_pi = np.log(LD(8) * np.arctan(LD(1)))
        q = np.array([Gl[f, f] - Gl[F:, f] @ (Gi @ Gl[F:, f]) for f in range(F)])
        return LD(0.5) * ((n - p) * log_two_pi - LD(xtx) + ld + lgx + q) if reml else LD(0.5) * (n * log_two_pi + ld + q)

    nll, grad = lk.nll_grad_from_gram(n, logdet, G, dlogdet, dG, F, reml, xtx)
    assert np.array_equal(nll, lk.nll_from_gram(n, logdet, G, F, reml, xtx)) and grad.shape == (F, K)
    assert np.all(np.abs(objective(G.astype(LD), LD(logdet)) - nll) <= 1e-13 * np.abs(nll))
    h = LD(1e-6)
    for k in range(K):
        up, dn = objective(G.astype(LD) + h * dG[k].astype(LD), LD(logdet) + h * LD(dlogdet[k])), objective(G.astype(LD) - h * dG[k].astype(LD), LD(logdet) - h * LD(dlogdet[k]))
        cd = (up - dn) / (2 * h)
        assert np.all(np.abs(cd - grad[:, k]) <= 1e-8 * (1.0 + np.abs(grad[:, k]))), (k, cd, grad[:, k])
    # a field's row does not depend on the fields beside it
    for f in range(F):
        keep = [f] + list(range(F, F + p))
        one = lk.nll_grad_from_gram(n, logdet, G[np.ix_(keep, keep)], dlogdet, dG[:, keep][:, :, keep], 1, reml, xtx)
        assert one[0][0] == nll[f] and np.array_equal(one[1][0], grad[f])
    bad = lk.nll_grad_from_gram(n, math.inf, np.full_like(G, np.nan), np.full(K, np.nan), np.full_like(dG, np.nan), F, reml, xtx)
    assert np.all(bad[0] == np.inf) and np.all(np.isnan(bad[1])) and bad[1].shape == (F, K)


# ------------------------------------------------------------------------------------------------------------- the search
def _field(n=60):
    from tests import _lik_cases as lc

    rng = np.random.default_rng(77)
    raw = rng.random((n, 2)) * [4.0, 3.0]
    Cm = lc.covariance_ld(lk._adjust(raw, [2.0], [30.0]), "exponential", [0.95, 1.2, 0.05]).astype(np.float64)
    return raw[:, 0], raw[:, 1], 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)


@pytest.fixture
def stand_in(monkeypatch, no_library):
    """The two plans replaced by the float64 restatements of tests/_vecchia_cases.py and tests/_vgrad_cases.py; loading a library fails
    the test."""
    plans = []

    class Plan(vg.StandInGradPlan):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            plans.append(self)

    monkeypatch.setattr(vgd, "VecchiaGradPlan", Plan)
    monkeypatch.setattr(vc, "VecchiaPlan", vcs.StandInPlan)
    return plans


def test_the_fit_on_a_stand_in_is_never_worse_than_its_start_and_needs_fewer_evaluations(stand_in):
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    at_start, g0 = vgd.neg_log_likelihood_vecchia_grad(x, y, v, "exponential", start, m=10)
    assert at_start == vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=10) and g0.shape == (5,)
    fit = vgd.fit_variogram_vecchia_grad(x, y, v, "exponential", m=10, start=start, fit_anisotropy=True)
    print(fit, fit.message)
    assert isinstance(fit, lk.MLFit) and math.isfinite(fit.nll) and fit.nll <= at_start and fit.nll < at_start - 0.1  # it moved
    assert len(stand_in) == 2 and fit.n_evaluations == stand_in[1].calls and set(fit.anisotropy) == set(lk._ANIS2)  # one plan, one search
    simplex = vc.fit_variogram_vecchia(x, y, v, "exponential", m=10, start=start, fit_anisotropy=True)
    print(simplex, simplex.message)
    assert fit.n_evaluations < simplex.n_evaluations and fit.nll <= simplex.nll + 1e-3 * abs(simplex.nll)
    # the gradient in natural units against differences of the value on the same stand-in
    for k, h in enumerate((1e-6, 1e-6, 1e-6)):
        up, dn = list(start), list(start)
        # psill with the nugget held moves the FULL sill; the nugget with psill held moves both
        up[0], dn[0] = start[0] + (h if k != 1 else 0.0), start[0] - (h if k != 1 else 0.0)
        up[k], dn[k] = (up[k] + h, dn[k] - h) if k else (up[k], dn[k])
        cd = (vc.neg_log_likelihood_vecchia(x, y, v, "exponential", up, m=10) - vc.neg_log_likelihood_vecchia(x, y, v, "exponential", dn, m=10)) / (2 * h)
        assert abs(cd - g0[k]) <= 1e-5 * (1.0 + abs(g0[k])), (k, cd, g0[k])
    ok = pa.OrdinaryKriging(x, y, v, variogram_model="exponential", variogram_parameters=start)
    assert ok.fit_variogram_vecchia_grad(m=10, fit_anisotropy=True).nll == fit.nll
    nll_c, grad_c = ok.neg_log_likelihood_vecchia_grad(m=10)
    assert nll_c == at_start and np.array_equal(grad_c, g0)


def test_a_trial_that_is_not_positive_definite_does_not_raise(stand_in, monkeypatch):
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    at_start = vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=10)
    seen = [0]
    real = vg.StandInGradPlan.grad

    def sometimes_inf(self, coords, dcoords, model, parameters, W):
        seen[0] += 1
        if seen[0] in (3, 4, 9):
            mc, K = np.shape(W)[1], 3 + (0 if dcoords is None else len(dcoords))
            return math.inf, np.full((mc, mc), np.nan), np.full(K, np.nan), np.full((K, mc, mc), np.nan)
        return real(self, coords, dcoords, model, parameters, W)

    monkeypatch.setattr(vg.StandInGradPlan, "grad", sometimes_inf)
    fit = vgd.fit_variogram_vecchia_grad(x, y, v, "exponential", m=10, start=start)
    print(fit, fit.message)
    assert seen[0] >= 9 and math.isfinite(fit.nll) and fit.nll <= at_start
