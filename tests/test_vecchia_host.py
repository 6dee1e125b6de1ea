"""vecchia.VecchiaPlan / neg_log_likelihood_vecchia / fit_variogram_vecchia without a GPU: include/mikvecchia.h declares what
libmikvecchia.so exports and the ctypes mirror agrees, the exported kernels are the three k_vec_* families and the five other libraries
hold nothing of the sixth, the sixth library is a unit of its own, every refusal comes with its reason before anything is loaded, the
long-double reference of tests/_vecchia_cases.py is the exact likelihood for m >= N - 1, a float64 NumPy restatement of the local
elimination is inside the bar the device is held to, and the search runs on that restatement."""
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
from tests import _lik_cases as lc
from tests import _vecchia_cases as vcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------- the library
def _declared():
    text = open(os.path.join(ROOT, "include", "mikvecchia.h")).read()
    verbatim = " ".join(text.split()).replace(" * ", " ")
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return verbatim, text, sorted(set(re.findall(r"\b(mvc_[a-z_0-9]+)\s*\(", text)))


def test_the_header_declares_what_the_library_exports_and_the_ctypes_mirror_agrees():
    from pykrige_amd import build

    build.build_library()
    assert os.path.exists(build.OUT_VECCHIA) and build.OUT_VECCHIA == vc.LIB_PATH and build.API_VECCHIA.endswith("mikvecchia.h")
    verbatim, text, names = _declared()
    assert names == sorted(vc.SIGNATURES) == ["mvc_abi_version", "mvc_last_error", "mvc_plan_create", "mvc_plan_destroy", "mvc_plan_gram",
                                              "mvc_plan_neighbours"]
    for phrase in ("k_p = min(m, p)", "d2 = dx*dx + dy*dy in 2-D and (dx*dx + dy*dy) + dz*dz in 3-D", "Ties go to the smaller position",
                   "ascending by (d2, position)", "C_ii = psill + nugget", "also at d = 0", "The last pivot squared is the conditional variance d_p",
                   "r_p(w) = w_p - s^T S^-1 w_c", "logdet = sum_p log d_p", "G_ab = sum_p r_p(a) r_p(b) / d_p", "exactly symmetric",
                   "MVC_ENOTPD", "1-based station index of the earliest such position", "writes neither result",
                   "fixed order that depends on n only", "depends only on its two columns", "equals the exact likelihood for m >= n - 1",
                   "a quarter of the device's memory", "(ndim + m_cols) n 8 bytes"):
        assert phrase in verbatim, phrase
    lib = vc.load()
    assert lib.mvc_abi_version() == vc.ABI_VERSION == int(re.search(r"#define MVC_ABI_VERSION (\d+)", text).group(1)) == 1
    for macro, value in (("MVC_MAXNB", vc.MAXNB), ("MVC_MAXCOLS", lk.MAXCOLS), ("MVC_EINVAL", "(-1)"), ("MVC_ENOTPD", "(-2)"),
                         ("MVC_EHIP", "(-3)"), ("MVC_GAUSSIAN", 0), ("MVC_EXPONENTIAL", 1), ("MVC_SPHERICAL", 2), ("MVC_HOLE_EFFECT", 3)):
        assert re.search(r"#define %s %s(?=\s)" % (macro, re.escape(str(value))), text), macro
    assert (vc.MVC_EINVAL, vc.MVC_ENOTPD, vc.MVC_EHIP) == (-1, -2, -3) and vc.MAXNB == 64
    ctype = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "const double *": vc._dp,
             "double *": vc._dp, "int32_t *": vc._i32p, "const int32_t *": vc._i32p, "mvc_plan *": vc._plan_p, "const mvc_plan *": vc._plan_p,
             "mvc_plan **": ctypes.POINTER(vc._plan_p)}
    flat = " ".join(text.split())
    for name, res in (("mvc_plan_create", "int"), ("mvc_plan_neighbours", "int"), ("mvc_plan_gram", "int"), ("mvc_plan_destroy", "void")):
        args = re.search(r"%s %s\((.*?)\);" % (res, name), flat).group(1).split(",")
        want = [ctype[re.match(r"\s*((?:const )?\w+ \*+|\w+)", a).group(1)] for a in args]
        assert vc.SIGNATURES[name] == (ctypes.c_int if res == "int" else None, want), name
    assert len(vc.SIGNATURES["mvc_plan_gram"][1]) == 11 and len(vc.SIGNATURES["mvc_plan_create"][1]) == 7
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "-C", build.OUT_VECCHIA], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert {e for e in exported if e.startswith("mvc_")} == set(names)
        kernels = sorted({m.group(1) for m in re.finditer(r"__device_stub__([A-Za-z_0-9]+)[<(]", out)})
        assert kernels == ["k_vec_knn", "k_vec_reduce", "k_vec_solve"], kernels
        for other in (build.OUT, build.OUT_VARIO, build.OUT_VARIO3, build.OUT_LIK, build.OUT_GRAD):  # nothing of the sixth in the five others
            sym = subprocess.run(["nm", "-D", "-C", other], capture_output=True, text=True, check=True).stdout
            assert "mvc_" not in sym and "k_vec_" not in sym, other
        for word in ("mkv_", "mkv3_", "mlk_", "mlg_", "k_vario", "k_lik", "k_grad", "mik_"):  # nor the reverse
            assert word not in out, word


def test_every_refusal_of_the_library_comes_with_its_reason_and_writes_nothing():
    lib = vc.load()
    p = lambda a: a.ctypes.data_as(vc._dp)
    c, o = np.array([0.0, 1.0, 2.0, 0.0, 1.0, 0.5]), np.array([2, 0, 1], dtype=np.int32)
    handle = vc._plan_p(7)

    def create(n=3, ndim=2, coords=c, order=o, m=2):
        return lib.mvc_plan_create(0, n, ndim, p(coords), order.ctypes.data_as(vc._i32p), m, ctypes.byref(handle))

    for kw, reason in ((dict(n=1), b"two stations"), (dict(ndim=4), b"ndim"), (dict(ndim=1), b"ndim"), (dict(m=0), b"MVC_MAXNB"),
                       (dict(m=65), b"MVC_MAXNB"), (dict(n=2 ** 31), b"fits no device"),
                       (dict(coords=np.array([0.0, np.nan, 2.0, 0.0, 1.0, 0.5])), b"coordinates must be finite"),
                       (dict(coords=np.array([0.0, 1.0, 2.0, 0.0, np.inf, 0.5])), b"coordinates must be finite"),
                       (dict(order=np.array([0, 1, 1], dtype=np.int32)), b"permutation"), (dict(order=np.array([0, 1, 3], dtype=np.int32)), b"permutation"),
                       (dict(order=np.array([-1, 1, 2], dtype=np.int32)), b"permutation")):
        handle.value = 7
        assert create(**kw) == vc.MVC_EINVAL and reason in lib.mvc_last_error(), (kw, lib.mvc_last_error())
        assert not handle.value  # no plan
    assert lib.mvc_plan_create(0, 3, 2, None, o.ctypes.data_as(vc._i32p), 2, ctypes.byref(handle)) == vc.MVC_EINVAL
    assert b"NULL argument" in lib.mvc_last_error()
    # mvc_plan_gram checks what it can before it looks at the plan: these refusals need neither a plan nor a GPU
    w, g = np.ones(3), np.full(4, 7.0)
    logdet, info = ctypes.c_double(7.0), ctypes.c_int32(5)

    def gram(model=1, psill=1.0, rng=0.5, nugget=0.1, m_cols=1, coords=c):
        return lib.mvc_plan_gram(None, None if coords is None else p(coords), model, psill, rng, nugget, p(w), m_cols, ctypes.byref(logdet),
                                 p(g), ctypes.byref(info))

    for kw, reason in ((dict(coords=None), b"NULL argument"), (dict(m_cols=0), b"MVC_MAXCOLS"), (dict(m_cols=41), b"MVC_MAXCOLS"),
                       (dict(model=4), b"model"), (dict(model=-1), b"model"), (dict(psill=0.0), b"psill > 0"), (dict(rng=-1.0), b"range > 0"),
                       (dict(nugget=-0.5), b"nugget >= 0"), (dict(psill=float("inf")), b"finite"), (dict(rng=float("nan")), b"finite"),
                       ({}, b"NULL plan")):
        assert gram(**kw) == vc.MVC_EINVAL and reason in lib.mvc_last_error(), (kw, lib.mvc_last_error())
    assert logdet.value == 7.0 and np.all(g == 7.0)  # a refused call writes no result
    assert lib.mvc_plan_neighbours(None, None) == vc.MVC_EINVAL and b"NULL argument" in lib.mvc_last_error()
    lib.mvc_plan_destroy(None)  # harmless


def test_a_missing_or_stale_library_is_answered_as_the_others_are(monkeypatch):
    monkeypatch.setattr(vc, "_lib", None)
    monkeypatch.setattr(vc, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    with pytest.raises(ImportError, match=r"is missing -- build it with `python -m pykrige_amd.build`"):
        vc.load()
    monkeypatch.undo()
    real = vc.load()

    class Old:
        def __getattr__(self, name):
            if name == "mvc_plan_gram":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(vc, "_lib", None)
    monkeypatch.setattr(vc.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mvc_plan_gram.*rebuild"):
        vc.load()


def test_the_sixth_library_is_a_unit_of_its_own():
    from pykrige_amd import build

    assert list(build.UNITS_VECCHIA) == ["mik_vecchia"] and build.UNITS_VECCHIA["mik_vecchia"] == ("mik_vecchia.hip", ["mik_k_vecchia.h"])
    assert len(build.UNITS) == 10 and "mik_vecchia" not in build.UNITS
    assert build.UNITS_LIK["mik_lik"] == ("mik_lik.hip", ["mik_k_lik.h"]) and list(build.UNITS_GRAD) == ["mik_grad"]
    others = build.all_sources() + build.lik_deps("mik_lik") + build.grad_deps("mik_grad") + build.vario_deps("mik_vario") + build.vario3_deps(
        "mik_vario3")
    assert not any("vecchia" in os.path.basename(d) for d in others)
    assert build.OUT_VECCHIA.endswith("libmikvecchia.so") and "libmikvecchia.so" in build.__doc__
    csrc = os.path.join(ROOT, "pykrige_amd", "csrc")
    hip, hdr = open(os.path.join(csrc, "mik_vecchia.hip")).read(), open(os.path.join(csrc, "mik_k_vecchia.h")).read()
    for text in (hip, hdr):  # no code of the other libraries; no options, no environment, no atomics, no inline assembly
        for word in ('"mik_k_lik', '"mik_k_grad', '"mik_k_vario', '"mik_dev.h"', '"mik_host.h"', "mikvario", "mikrige.h", "miklik.h", "mikgrad.h",
                     "getenv", "strcmp", "atomic", "asm"):
            assert word not in text.replace("no atomic", ""), word
    assert "namespace mvc" in hdr and "#pragma clang fp contract(off)" in hdr and hdr.count("#pragma clang fp contract(off)") >= 4
    assert "static_assert" in hdr and "static_assert" in hip and "163840" in hdr and "163840" in hip
    build.build_library()
    assert build.up_to_date()
    plain = lambda flags: [c for c in flags if c not in build.COMPRESS and not c.startswith("-I")]
    assert plain(open(os.path.join(build.OBJ, "mik_vecchia.flags")).read().split()) == plain(build.FLAGS)
    deps = build.vecchia_deps("mik_vecchia")
    assert deps == [os.path.join(csrc, "mik_vecchia.hip"), os.path.join(csrc, "mik_k_vecchia.h"), build.API_VECCHIA]
    old = os.path.getmtime(build.OUT_VECCHIA)  # up_to_date() sees the sixth library: a library older than its header is stale
    try:
        os.utime(build.OUT_VECCHIA, (1.0, 1.0))
        assert not build.up_to_date()
    finally:
        os.utime(build.OUT_VECCHIA, (old, old))
    assert build.up_to_date()
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_library" in text and "vecchia.load()" in text and "OUT_VECCHIA" in text
    ignored = subprocess.run(["git", "check-ignore", "-q", build.OUT_VECCHIA], cwd=ROOT).returncode
    assert ignored in (0, 128)  # ignored like its siblings (128: not a git checkout)


# ------------------------------------------------------------------------------------------------------------- the interface
def test_signatures_and_docstrings():
    assert list(inspect.signature(vc.VecchiaPlan.__init__).parameters) == ["self", "coords", "m", "order", "seed"]
    sig = inspect.signature(vc.VecchiaPlan.__init__).parameters
    assert (sig["m"].default, sig["order"].default, sig["seed"].default) == (30, "random", 0)
    assert list(inspect.signature(vc.VecchiaPlan.gram).parameters) == ["self", "coords", "model", "parameters", "W"]
    assert list(inspect.signature(vc.neg_log_likelihood_vecchia).parameters)[:2] == ["x", "y"]
    assert list(inspect.signature(vc.fit_variogram_vecchia).parameters)[:2] == ["x", "y"]
    doc = " ".join(vc.fit_variogram_vecchia.__doc__.split())
    for phrase in ("Nelder-Mead", "One plan, built in the start metric", "at most 5000 stations", "There is no gradient method", "MLFit",
                   "does not raise"):
        assert phrase in doc, phrase
    doc = " ".join(vc.neg_log_likelihood_vecchia.__doc__.split())
    for phrase in ("m=30, order=\"random\", seed=0, plan=None", "bit for bit", "exact likelihood", "``inf``", "no CPU fallback"):
        assert phrase in doc, phrase
    assert vc.nll_from_gram is lk.nll_from_gram and vc.MLFit is lk.MLFit and vc._split is lk._split and vc._trend is lk._trend
    for cls in (pa.OrdinaryKriging, pa.OrdinaryKriging3D):
        sig = inspect.signature(cls.neg_log_likelihood_vecchia)
        assert list(sig.parameters) == ["self", "variogram_parameters", "m", "order", "seed", "plan", "reml", "anisotropy"]
        sig = inspect.signature(cls.fit_variogram_vecchia)
        assert list(sig.parameters) == ["self", "m", "order", "seed", "start", "fit_anisotropy", "reml", "bounds", "anisotropy"]
        for fn in (cls.neg_log_likelihood_vecchia, cls.fit_variogram_vecchia):
            doc = " ".join(fn.__doc__.split())
            for phrase in ("regional_linear", "NotImplementedError", "geographic", "device group", "'custom'"):
                assert phrase in doc, (cls.__name__, fn.__name__, phrase)
    assert "vecchia" in pa.__all__ and pa.vecchia is vc


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(vc, "_lib", None)
    monkeypatch.setattr(vc, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    monkeypatch.setattr(vc, "load", boom)
    monkeypatch.setattr(vc.C, "CDLL", boom)
    monkeypatch.setattr(lk, "load", boom)


def test_every_refusal_is_raised_before_the_library_is_loaded(no_library):
    rng = np.random.default_rng(0)
    X, v = rng.random((20, 2)), rng.standard_normal(20)
    x, y, z = X[:, 0], X[:, 1], rng.random(20)
    for kw, match in ((dict(coords=X[:, :1]), r"shape \(N, 2\) or \(N, 3\)"), (dict(coords=X[:1]), "two stations"), (dict(m=0), "MVC_MAXNB"),
                      (dict(m=65), "MVC_MAXNB"), (dict(m=2.5), "MVC_MAXNB"), (dict(order="maxmin"), "'random', 'coordinate' or a permutation"),
                      (dict(order=np.arange(19)), "permutation"), (dict(order=np.zeros(20, dtype=int)), "permutation"),
                      (dict(order=np.arange(20.0)), "permutation"),
                      (dict(coords=np.where(np.arange(40).reshape(20, 2) == 3, np.inf, X)), "coordinates must be finite")):
        with pytest.raises(ValueError, match=match):
            vc.VecchiaPlan(**{"coords": X, **kw})
    full = [1.1, 0.5, 0.1]
    for fn, tail in ((vc.neg_log_likelihood_vecchia, (full,)), (vc.fit_variogram_vecchia, ())):
        for args, kw, exc, match in (
                ((x, y, v, "linear") + tail, {}, ValueError, "unbounded"), ((x, y, v, "power") + tail, {}, ValueError, "unbounded"),
                ((x, y, v, "custom") + tail, {}, NotImplementedError, "custom"), ((x, y, v, "cubic") + tail, {}, ValueError, "must be one of"),
                ((x, y, np.where(np.arange(20) == 2, np.inf, v), "exponential") + tail, {}, ValueError, "values must be finite"),
                ((np.where(np.arange(20) == 2, np.nan, x), y, v, "exponential") + tail, {}, ValueError, "coordinates must be finite"),
                ((x, y[:-1], v, "exponential") + tail, {}, ValueError, "same length"),
                ((x, y, np.zeros((20, 33)), "exponential") + tail, {}, ValueError, "F <= 32"),
                ((x[:1], y[:1], v[:1], "exponential") + tail, {}, ValueError, "two stations"),
                ((x, y, v, "exponential") + tail, dict(drift=np.ones((20, 1))), ValueError, "rank-deficient"),
                ((x, y, v, "exponential") + tail, dict(drift=rng.random((20, 8))), ValueError, "at most 8 trend columns"),
                ((x, y, v, "exponential") + tail, dict(drift="quadratic"), ValueError, "regional_linear"),
                ((x, y, v, "exponential") + tail, dict(anisotropy_scaling_z=2.0), ValueError, "3-D classes"),
                ((x, y, z, v, "exponential") + tail, dict(anisotropy_scaling=2.0), ValueError, "2-D classes"),
                ((x, y, v, "exponential") + tail, dict(anisotropy_scaling=0.0), ValueError, "scaling must be positive"),
                ((x, y, v, "exponential") + tail, dict(m=0), ValueError, "MVC_MAXNB"), ((x, y, v, "exponential") + tail, dict(m=65), ValueError, "MVC_MAXNB"),
                ((x, y, v, "exponential") + tail, dict(order="maxmin"), ValueError, "'random', 'coordinate'"),
                ((x, y, v, "exponential") + tail, dict(order=np.arange(5)), ValueError, "permutation"),
                ((x, y, v, "exponential") + tail, dict(seed=-1), ValueError, "seed"),
                ((x, y, v, "exponential") + tail, dict(nlags=6), TypeError, "unexpected argument"),
                ((x, y, v, "exponential") + tail, dict(method="l-bfgs-b"), TypeError, "unexpected argument"),
                ((x, y, v), {}, TypeError, "variogram_model is required")):
            with pytest.raises(exc, match=match):
                fn(*args, **kw)
    for par, match in (([0.1, 0.5, 0.1], "partial sill > 0"), (None, "must be given")):
        with pytest.raises(ValueError, match=match):
            vc.neg_log_likelihood_vecchia(x, y, v, "exponential", par)
    with pytest.raises(ValueError, match="plan must be a VecchiaPlan"):
        vc.neg_log_likelihood_vecchia(x, y, v, "exponential", full, plan=object())
    with pytest.raises(ValueError, match="constant"):
        vc.fit_variogram_vecchia(x, y, np.ones(20), "exponential")
    for bounds in ({"sill": (0.1, 1.0)}, {"range": (1.0, 0.5)}, [(0, 1)]):
        with pytest.raises(ValueError, match="bounds"):
            vc.fit_variogram_vecchia(x, y, v, "exponential", start=full, bounds=bounds)
    kw = dict(variogram_model="exponential", variogram_parameters=full)
    calls = (lambda o: o.neg_log_likelihood_vecchia(), lambda o: o.fit_variogram_vecchia())

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
            obj.neg_log_likelihood_vecchia(nlags=6)
        with pytest.raises(ValueError, match="MVC_MAXNB"):
            obj.fit_variogram_vecchia(m=100)
    for call in calls:
        with pytest.raises(ValueError, match="geographic"):
            call(pa.OrdinaryKriging(360.0 * x, 90.0 * y, v, coordinates_type="geographic", **kw))
        with pytest.raises(ValueError, match="unbounded"):
            call(pa.OrdinaryKriging(x, y, v, variogram_model="linear", variogram_parameters=[1.0, 0.1]))
        with pytest.raises(ValueError, match="unbounded"):
            call(pa.OrdinaryKriging3D(x, y, z, v, variogram_model="power", variogram_parameters=[1.0, 1.5, 0.1]))
        with pytest.raises(NotImplementedError, match="custom"):
            call(pa.OrdinaryKriging(x, y, v, variogram_model="custom", variogram_parameters=[1.0], variogram_function=lambda p, d: p[0] * d))


# ------------------------------------------------------------------------------------------------------------- the reference
def test_neighbours_ref_on_a_lattice_gives_the_hand_checked_lists():
    """5 x 5 unit lattice, station s = 5 row + column at (column, row), identity order.  Station 12 = (2, 2): its predecessors 0 .. 11 at
    d2 = 1 are 7 and 11 (7 first: the smaller position), at d2 = 2 are 6 and 8, at d2 = 4 are 2 and 10.  Station 24 = (4, 4): d2 = 1 are
    19 and 23, d2 = 2 is 18, d2 = 4 are 14 and 22, d2 = 5 are 13 and 17.  Reversed order for station 12: its predecessors are 24 .. 13;
    d2 = 1 are 17 (position 7) and 13 (position 11), d2 = 2 are 18 (position 6) and 16 (position 8), d2 = 4 are 22 and 14."""
    X = np.array([[c, r] for r in range(5) for c in range(5)], dtype=np.float64)
    nb = vcs.neighbours_ref(X, np.arange(25), 6)
    assert nb[12].tolist() == [7, 11, 6, 8, 2, 10] and nb[24].tolist() == [19, 23, 18, 14, 22, 13]
    assert nb[0].tolist() == [-1] * 6 and nb[2].tolist() == [1, 0, -1, -1, -1, -1]
    nb = vcs.neighbours_ref(X, np.arange(24, -1, -1), 6)
    assert nb[12].tolist() == [17, 13, 18, 16, 22, 14] and nb[24].tolist() == [-1] * 6


@pytest.mark.parametrize("name,kind", [("n63_sph3d_m7", "random"), ("n63_sph3d_m7", "reversed"), ("n65_gau_m17", "random"),
                                       ("n65_gau_m17", "identity")])
def test_with_every_predecessor_as_neighbour_the_reference_is_the_exact_likelihood(name, kind):
    """m >= N - 1, any order: log det and G equal ``_lik_cases.brute_force`` -- two long-double eliminations of the same matrix in a
    different order, held to 1e-15 N relative."""
    case = lc.CASES[name]
    X, W = lc.inputs(case)
    n = case["n"]
    order = vcs.order_of(n, kind)
    nbr = vcs.neighbours_ref(X, order, n - 1)
    assert np.all(np.sort(nbr[order[n - 1]]) == np.sort(order[:n - 1]))
    logdet, G = vcs.brute_force(X, order, nbr, case["model"], case["par"], W)
    ref_logdet, ref_G = lc.brute_force(X, case["model"], case["par"], W)
    el, eg = lc.errors(logdet, G, ref_logdet, ref_G)
    print("%s %s: logdet %.6f relative error %.3g, G error %.3g" % (name, kind, float(logdet), el / abs(float(ref_logdet)), eg))
    assert el <= 1e-15 * n * abs(float(ref_logdet)) and eg <= 1e-15 * n


@pytest.mark.parametrize("name,m", vcs.DEVICE + [("big", vcs.BIG_M)])
def test_the_float64_restatement_is_within_the_bar(name, m):
    """The CPU proof that the bar is reachable: the elimination of k_vec_solve in float64 NumPy against the long-double brute force."""
    case = vcs.case_of(name)
    X, W = vcs.inputs(name)
    order, nbr, ref_logdet, ref_G, kappa, bar = vcs.reference(name, m)
    assert kappa <= lc.KAPPA_MAX
    logdet, G = vcs.float64_gram(X, order, nbr, case["model"], case["par"], W)
    el, eg = vcs.errors(logdet, G, ref_logdet, ref_G)
    print("%-16s m %2d kappa_2 %9.3g bar %9.3g logdet error %9.3g G error %9.3g worst/bar %8.3g" % (name, m, kappa, bar, el, eg, max(el, eg) / bar))
    assert el <= bar and eg <= bar


def test_the_reference_answers_a_matrix_that_is_not_positive_definite():
    for name, kind, station in (("notpd_n2", "identity", 2), ("notpd_n2", "reversed", 1), ("notpd_n200", "identity", 151),
                                ("notpd_n200", "reversed", 1)):
        case, _ = lc.NOT_PD[name]
        X, W = lc.inputs(case)
        order = vcs.order_of(case["n"], kind)
        nbr = vcs.neighbours_ref(X, order, 5)
        k, j = case["repeat"]
        later, earlier = (k, j) if kind == "identity" else (j, k)
        assert nbr[later][0] == earlier and later + 1 == station
        assert vcs.brute_force(X, order, nbr, case["model"], case["par"], W) == (None, station)
        assert vcs.float64_gram(X, order, nbr, case["model"], case["par"], W) == (None, station)


# ------------------------------------------------------------------------------------------------------------- the search
def _field(n=60):
    rng = np.random.default_rng(77)
    raw = rng.random((n, 2)) * [4.0, 3.0]
    Cm = lc.covariance_ld(lk._adjust(raw, [2.0], [30.0]), "exponential", [0.95, 1.2, 0.05]).astype(np.float64)
    return raw[:, 0], raw[:, 1], 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)


@pytest.fixture
def stand_in(monkeypatch, no_library):
    """``VecchiaPlan`` replaced by ``_vecchia_cases.StandInPlan`` -- the float64 restatement behind ``gram``; the real constructor
    needs a device.  Loading the library fails the test."""
    plans = []

    class Plan(vcs.StandInPlan):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            plans.append(self)

    monkeypatch.setattr(vc, "VecchiaPlan", Plan)
    return plans


def test_the_fit_on_a_stand_in_is_never_worse_than_its_start(stand_in):
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    at_start = vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=10)
    fit = vc.fit_variogram_vecchia(x, y, v, "exponential", m=10, start=start, fit_anisotropy=True)
    print(fit, fit.message)
    assert isinstance(fit, lk.MLFit) and math.isfinite(fit.nll) and fit.nll <= at_start and fit.nll < at_start - 0.1  # it moved
    assert len(stand_in) == 2 and fit.n_evaluations == stand_in[1].calls and set(fit.anisotropy) == set(lk._ANIS2)  # one plan, one search
    lo, hi = 1e-6 * np.var(v), 100.0 * np.var(v)
    sill, rng_, nugget = fit.variogram_parameters
    assert lo <= sill - nugget <= hi and 0.0 <= nugget <= hi and 0.05 <= fit.anisotropy["anisotropy_scaling"] <= 20.0
    # with every predecessor as a neighbour the objective is likelihood.neg_log_likelihood on the dense restatement
    from tests import _grad_cases as gc

    exact = vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=59)
    logdet, G = gc.standin_gram(lk._adjust(np.column_stack([x, y]), [1.0], [0.0]), "exponential", [1.3, 0.6, 0.2], np.column_stack([v, np.ones(60)]))
    dense = float(lk.nll_from_gram(60, logdet, G, 1, True, lk._pieces(np.ones((60, 1))))[0])
    assert abs(exact - dense) <= 1e-9 * abs(dense)
    # the start from a subsample: no start given
    fit0 = vc.fit_variogram_vecchia(x, y, v, "exponential", m=10)
    assert math.isfinite(fit0.nll) and fit0.anisotropy == dict(anisotropy_scaling=1.0, anisotropy_angle=0.0)
    ok = pa.OrdinaryKriging(x, y, v, variogram_model="exponential", variogram_parameters=start)
    assert ok.fit_variogram_vecchia(m=10, fit_anisotropy=True).nll == fit.nll
    assert ok.neg_log_likelihood_vecchia(m=10) == at_start


def test_a_trial_that_is_not_positive_definite_does_not_raise(stand_in, monkeypatch):
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    at_start = vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=10)
    seen = [0]
    real = vcs.StandInPlan.gram

    def sometimes_inf(self, coords, model, parameters, W):
        seen[0] += 1
        if seen[0] in (3, 4, 9):
            mc = np.shape(W)[1]
            return math.inf, np.full((mc, mc), np.nan)
        return real(self, coords, model, parameters, W)

    monkeypatch.setattr(vcs.StandInPlan, "gram", sometimes_inf)
    fit = vc.fit_variogram_vecchia(x, y, v, "exponential", m=10, start=start)
    print(fit, fit.message)
    assert seen[0] >= 9 and math.isfinite(fit.nll) and fit.nll <= at_start
