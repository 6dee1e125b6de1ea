"""likelihood.gram / neg_log_likelihood / fit_variogram_ml without a GPU: the module and the four classes carry the signatures and
docstrings the users read, every refusal is raised before ctypes loads anything, include/miklik.h declares what libmiklik.so exports and
the ctypes mirror agrees with it, the exported kernels are the four k_lik_* families, the other three libraries hold nothing of the
fourth, every case keeps its condition number, and a float64 NumPy restatement of the blocked elimination agrees with the long-double
brute force inside the bar the device is held to (tests/_lik_cases.py)."""
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
from tests import _lik_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the interface
def test_signatures_and_docstrings():
    assert list(inspect.signature(lk.gram).parameters) == ["coords", "model", "parameters", "W"]
    assert list(inspect.signature(lk.neg_log_likelihood).parameters)[:2] == ["x", "y"]
    assert list(inspect.signature(lk.fit_variogram_ml).parameters)[:2] == ["x", "y"]
    doc = " ".join(lk.gram.__doc__.split())
    for phrase in ("[psill, range, nugget]", "C_ii = psill + nugget", "C_ij = (psill + nugget) - gamma(d_ij)", "also at d = 0",
                   "exactly symmetric", "bit for bit", "1 <= m <= 40", "``inf``", "no CPU fallback"):
        assert phrase in doc, phrase
    doc = " ".join(lk.neg_log_likelihood.__doc__.split())
    for phrase in ("x, y[, z], values, variogram_model, variogram_parameters", "anisotropy_scaling=1.0", "anisotropy_angle_z", "F <= 32",
                   "FULL sill", "p = 1 + q <= 8", "1/2 [N log 2 pi + log det C + Q_f]",
                   "1/2 [(N - p) log 2 pi - log det(X^T X) + log det C + log det G_xx + Q_f]", "``inf``", "NotImplementedError",
                   "rank-deficient"):
        assert phrase in doc, phrase
    doc = " ".join(lk.fit_variogram_ml.__doc__.split())
    for phrase in ("Nelder-Mead", "derivative-free", "One device call per evaluation", "log(nugget + floor)", "fit_anisotropy",
                   "independent replicates", "least-squares fit", "n_evaluations", "success"):
        assert phrase in doc, phrase
    for cls in (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D):
        sig = inspect.signature(cls.neg_log_likelihood)
        assert list(sig.parameters) == ["self", "variogram_parameters", "reml", "anisotropy"]
        assert sig.parameters["variogram_parameters"].default is None and sig.parameters["reml"].default is True
        sig = inspect.signature(cls.fit_variogram_ml)
        assert list(sig.parameters) == ["self", "start", "fit_anisotropy", "reml", "bounds", "anisotropy"]
        assert sig.parameters["fit_anisotropy"].default is False and sig.parameters["start"].default is None
        for fn in (cls.neg_log_likelihood, cls.fit_variogram_ml):
            doc = " ".join(fn.__doc__.split())
            for phrase in ("regional_linear", "NotImplementedError", "geographic", "device group", "'custom'"):
                assert phrase in doc, (cls.__name__, fn.__name__, phrase)
    assert "likelihood" in pa.__all__ and pa.likelihood is lk
    assert (lk.MAXCOLS, lk.MAXFIELDS, lk.MAXTREND) == (40, 32, 8)


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(lk, "_lib", None)
    monkeypatch.setattr(lk, "load", boom)
    monkeypatch.setattr(lk.C, "CDLL", boom)


def test_every_refusal_is_raised_before_anything_is_loaded(no_library):
    rng = np.random.default_rng(0)
    X, v = rng.random((20, 2)), rng.standard_normal(20)
    x, y, z = X[:, 0], X[:, 1], rng.random(20)
    ok = [1.0, 0.5, 0.1]
    for args, match in (((X[:, :1], "exponential", ok, v), r"shape \(N, 2\) or \(N, 3\)"), ((X[:1], "exponential", ok, v[:1]), "two stations"),
                        ((X, "exponential", [0.0, 0.5, 0.1], v), "psill > 0"), ((X, "exponential", [1.0, 0.0, 0.1], v), "range > 0"),
                        ((X, "exponential", [1.0, 0.5, -0.1], v), "nugget >= 0"), ((X, "exponential", [1.0, 0.5], v), "three numbers"),
                        ((X, "exponential", [1.0, np.nan, 0.1], v), "finite"), ((X, "exponential", ok, v[:-1]), r"shape \(N,\) or \(N, m\)"),
                        ((X, "exponential", ok, np.zeros((20, 41))), "MLK_MAXCOLS"), ((X, "linear", ok, v), "unbounded"),
                        ((X, "power", ok, v), "unbounded"), ((X, "cubic", ok, v), "must be one of"),
                        ((np.where(np.arange(40).reshape(20, 2) == 3, np.inf, X), "exponential", ok, v), "coordinates must be finite"),
                        ((X, "exponential", ok, np.where(np.arange(20) == 3, np.nan, v)), "W must be finite")):
        with pytest.raises(ValueError, match=match):
            lk.gram(*args)
    with pytest.raises(NotImplementedError, match="custom"):
        lk.gram(X, "custom", ok, v)
    full = [1.1, 0.5, 0.1]
    for fn, tail in ((lk.neg_log_likelihood, (full,)), (lk.fit_variogram_ml, ())):
        for args, kw, exc, match in (
                ((x, y, v, "linear") + tail, {}, ValueError, "unbounded"), ((x, y, v, "power") + tail, {}, ValueError, "unbounded"),
                ((x, y, v, "custom") + tail, {}, NotImplementedError, "custom"),
                ((x, y, np.where(np.arange(20) == 2, np.inf, v), "exponential") + tail, {}, ValueError, "values must be finite"),
                ((np.where(np.arange(20) == 2, np.nan, x), y, v, "exponential") + tail, {}, ValueError, "coordinates must be finite"),
                ((x, y[:-1], v, "exponential") + tail, {}, ValueError, "same length"),
                ((x, y, np.zeros((20, 33)), "exponential") + tail, {}, ValueError, "F <= 32"),
                ((x, y, v, "exponential") + tail, dict(drift=np.ones((20, 1))), ValueError, "rank-deficient"),
                ((x, y, v, "exponential") + tail, dict(drift=np.column_stack([x, 2.0 * x])), ValueError, "rank-deficient"),
                ((x, y, v, "exponential") + tail, dict(drift=rng.random((20, 8))), ValueError, "at most 8 trend columns"),
                ((x, y, v, "exponential") + tail, dict(drift=np.where(np.arange(20) == 1, np.nan, x)), ValueError, "drift must be finite"),
                ((x, y, v, "exponential") + tail, dict(drift=x[:-1]), ValueError, r"shape \(N, q\)"),
                ((x, y, v, "exponential") + tail, dict(anisotropy_scaling_z=2.0), ValueError, "3-D classes"),
                ((x, y, z, v, "exponential") + tail, dict(anisotropy_scaling=2.0), ValueError, "2-D classes"),
                ((x, y, v, "exponential") + tail, dict(anisotropy_scaling=0.0), ValueError, "scaling must be positive"),
                ((x, y, v, "exponential") + tail, dict(anisotropy_angle=float("nan")), ValueError, "must be finite"),
                ((x, y, v, "exponential") + tail, dict(nlags=6), TypeError, "unexpected argument")):
            with pytest.raises(exc, match=match):
                fn(*args, **kw)
    for par, match in (([0.1, 0.5, 0.1], "partial sill > 0"), ({"sill": 1.0, "range": -1.0, "nugget": 0.0}, "range > 0"), (None, "must be given")):
        with pytest.raises(ValueError, match=match):
            lk.neg_log_likelihood(x, y, v, "exponential", par)
    with pytest.raises(ValueError, match="constant"):
        lk.fit_variogram_ml(x, y, np.ones(20), "exponential")
    for bounds in ({"sill": (0.1, 1.0)}, {"range": (1.0, 0.5)}, {"psill": (0.0, 1.0)}, [(0, 1)]):
        with pytest.raises(ValueError, match="bounds"):
            lk.fit_variogram_ml(x, y, v, "exponential", start=full, bounds=bounds)


def test_the_classes_refuse_before_anything_is_loaded(no_library):
    rng = np.random.default_rng(1)
    x, y, z, v = rng.random(20), rng.random(20), rng.random(20), rng.standard_normal(20)
    kw = dict(variogram_model="exponential", variogram_parameters=[1.1, 0.5, 0.1])
    calls = (lambda o: o.neg_log_likelihood(), lambda o: o.fit_variogram_ml())
    two = [pa.OrdinaryKriging(x, y, v, **kw), pa.UniversalKriging(x, y, v, drift_terms=["regional_linear"], **kw)]
    three = [pa.OrdinaryKriging3D(x, y, z, v, **kw), pa.UniversalKriging3D(x, y, z, v, drift_terms=["regional_linear"], **kw)]

    class Group:
        n_devices = 2

    for obj in two + three:
        obj._handle = Group()
        try:
            for call in calls:
                with pytest.raises(ValueError, match="device group of 2"):
                    call(obj)
        finally:
            obj._handle = None
        with pytest.raises(TypeError, match="unexpected argument"):
            obj.neg_log_likelihood(nlags=6)
    for obj in two:
        with pytest.raises(TypeError, match="anisotropy_scaling, anisotropy_angle"):
            obj.neg_log_likelihood(anisotropy_scaling_y=2.0)
    for obj in three:
        with pytest.raises(TypeError, match="anisotropy_scaling_y"):
            obj.fit_variogram_ml(anisotropy_scaling=2.0)
    geo = pa.OrdinaryKriging(360.0 * x, 90.0 * y, v, coordinates_type="geographic", **kw)
    for model, par, exc in (("linear", [1.0, 0.1], ValueError), ("power", [1.0, 1.5, 0.1], ValueError)):
        obj = pa.OrdinaryKriging(x, y, v, variogram_model=model, variogram_parameters=par)
        for call in calls:
            with pytest.raises(exc, match="unbounded"):
                call(obj)
    custom = pa.OrdinaryKriging(x, y, v, variogram_model="custom", variogram_parameters=[1.0], variogram_function=lambda p, d: p[0] * d)
    others = [pa.UniversalKriging(x, y, v, drift_terms=["regional_linear", "specified"], specified_drift=[x * y], **kw),
              pa.UniversalKriging(x, y, v, drift_terms=["functional"], functional_drift=[lambda a, b: a * b], **kw),
              pa.UniversalKriging(x, y, v, drift_terms=["point_log"], point_drift=[[0.5, 0.5, 1.0]], **kw),
              pa.UniversalKriging3D(x, y, z, v, drift_terms=["specified"], specified_drift=[x * z], **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="geographic"):
            call(geo)
        with pytest.raises(NotImplementedError, match="custom"):
            call(custom)
        for obj in others:
            with pytest.raises(NotImplementedError, match="regional_linear is the only drift term"):
                call(obj)


# ------------------------------------------------------------------------------------------------------------- the libraries
def _declared():
    text = open(os.path.join(ROOT, "include", "miklik.h")).read()
    verbatim = " ".join(text.split())
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return verbatim, text, sorted(set(re.findall(r"\b(mlk_[a-z_0-9]+)\s*\(", text)))


def test_the_header_declares_what_the_library_exports_and_the_ctypes_mirror_agrees():
    from pykrige_amd import build

    build.build_library()
    assert os.path.exists(build.OUT_LIK) and build.OUT_LIK == lk.LIB_PATH and build.API_LIK.endswith("miklik.h")
    verbatim, text, names = _declared()
    assert names == sorted(lk.SIGNATURES) == ["mlk_abi_version", "mlk_gram", "mlk_last_error"]
    for phrase in ("C_ii = psill + nugget.", "For i != j, C_ij = (psill + nugget) - gamma(d_ij).", "d_ij is the Euclidean distance",
                   "gamma is the model formula of core.variogram_value", "library exp", "applied at d = 0 too", "C_ij = psill",
                   "logdet = 2 sum_i log L_ii", "G = W^T C^-1 W", "both halves written", "<= 0 or not finite", "MLK_ENOTPD",
                   "launches nothing further"):
        assert phrase in verbatim.replace(" * ", " "), phrase
    lib = lk.load()
    assert lib.mlk_abi_version() == lk.ABI_VERSION == int(re.search(r"#define MLK_ABI_VERSION (\d+)", text).group(1)) == 1
    for macro, value in (("MLK_MAXCOLS", lk.MAXCOLS), ("MLK_EINVAL", "(-1)"), ("MLK_ENOTPD", "(-2)"), ("MLK_EHIP", "(-3)"),
                         ("MLK_GAUSSIAN", 0), ("MLK_EXPONENTIAL", 1), ("MLK_SPHERICAL", 2), ("MLK_HOLE_EFFECT", 3)):
        assert re.search(r"#define %s %s(?=\s)" % (macro, re.escape(str(value))), text), macro
    assert lk.MODEL_IDS == {"gaussian": 0, "exponential": 1, "spherical": 2, "hole-effect": 3}
    assert (lk.MLK_EINVAL, lk.MLK_ENOTPD, lk.MLK_EHIP) == (-1, -2, -3)
    ctype = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
             "const double *": lk._dp, "double *": lk._dp, "int32_t *": lk._i32p}
    flat = " ".join(text.split())
    args = re.search(r"int mlk_gram\((.*?)\);", flat).group(1).split(",")
    want = [ctype[re.match(r"\s*((?:const )?\w+ \*|\w+)", a).group(1)] for a in args]
    assert lk.SIGNATURES["mlk_gram"] == (ctypes.c_int, want) and len(want) == 13
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "-C", build.OUT_LIK], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert {e for e in exported if e.startswith("mlk_")} == set(names)
        kernels = sorted({m.group(1) for m in re.finditer(r"__device_stub__([A-Za-z_0-9]+)\(", out)})
        assert kernels == ["k_lik_assemble", "k_lik_potrf", "k_lik_syrk", "k_lik_trsm"], kernels
        for other in (build.OUT, build.OUT_VARIO, build.OUT_VARIO3):  # nothing of the fourth library is linked into the three others
            sym = subprocess.run(["nm", "-D", "-C", other], capture_output=True, text=True, check=True).stdout
            assert "mlk_" not in sym and "k_lik" not in sym, other
        assert "mkv_" not in out and "mkv3_" not in out and "k_vario" not in out and "mik_" not in out  # nor the reverse
    # calls that are refused launch nothing and need no GPU: the library's own checks answer MLK_EINVAL with a reason
    c, w, g = np.zeros(6), np.ones(3), np.zeros(1)
    p = lambda a: a.ctypes.data_as(lk._dp)
    logdet, info = ctypes.c_double(7.0), ctypes.c_int32(5)

    def call(n=3, ndim=2, coords=c, model=1, psill=1.0, rng=0.5, nugget=0.1, W=w, m=1):
        return lib.mlk_gram(0, n, ndim, p(coords), model, psill, rng, nugget, p(W), m, ctypes.byref(logdet), p(g), ctypes.byref(info))

    for kw, reason in ((dict(n=1), b"two stations"), (dict(ndim=4), b"ndim"), (dict(m=0), b"MLK_MAXCOLS"), (dict(m=41), b"MLK_MAXCOLS"),
                       (dict(model=4), b"model"), (dict(model=-1), b"model"), (dict(psill=0.0), b"psill > 0"), (dict(rng=-1.0), b"range > 0"),
                       (dict(nugget=-0.5), b"nugget >= 0"), (dict(psill=float("inf")), b"finite"),
                       (dict(coords=np.array([0.0, np.nan, 1.0, 0.0, 1.0, 2.0])), b"coordinates must be finite"),
                       (dict(W=np.array([1.0, np.inf, 0.0])), b"W must be finite"), (dict(n=2 ** 31), b"fits no device")):
        if kw.get("n", 0) > 3:  # (refused before a single element is read)
            kw = dict(kw, coords=c, W=w)
        assert call(**kw) == lk.MLK_EINVAL and reason in lib.mlk_last_error(), (kw, lib.mlk_last_error())
    assert logdet.value == 7.0  # a refused call writes no result


def test_a_missing_or_stale_library_is_answered_as_the_others_are(monkeypatch):
    monkeypatch.setattr(lk, "_lib", None)
    monkeypatch.setattr(lk, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    with pytest.raises(ImportError, match=r"is missing -- build it with `python -m pykrige_amd.build`"):
        lk.load()
    monkeypatch.undo()
    real = lk.load()

    class Old:
        def __getattr__(self, name):
            if name == "mlk_gram":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(lk, "_lib", None)
    monkeypatch.setattr(lk.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mlk_gram.*rebuild"):
        lk.load()

    class Older:
        def __getattr__(self, name):
            raise AttributeError(name)

    monkeypatch.setattr(lk.C, "CDLL", lambda path: Older())
    with pytest.raises(ImportError, match="has no mlk_abi_version.*rebuild"):
        lk.load()


def test_the_fourth_library_is_a_unit_of_its_own():
    from pykrige_amd import build

    assert list(build.UNITS_LIK) == ["mik_lik"] and build.UNITS_LIK["mik_lik"] == ("mik_lik.hip", ["mik_k_lik.h"])
    assert list(build.UNITS_VARIO3) == ["mik_vario3"] and list(build.UNITS_VARIO) == ["mik_vario"] and len(build.UNITS) == 10
    assert "mik_lik" not in build.UNITS and not any("lik" in os.path.basename(d) for d in build.all_sources())
    assert build.OUT_LIK.endswith("libmiklik.so") and "libmiklik.so" in build.__doc__
    csrc = os.path.join(ROOT, "pykrige_amd", "csrc")
    hip, hdr = open(os.path.join(csrc, "mik_lik.hip")).read(), open(os.path.join(csrc, "mik_k_lik.h")).read()
    for text in (hip, hdr):  # self-contained; no options, no environment, no atomics, no inline assembly
        for word in ('"mik_k_vario', '"mik_dev.h"', '"mik_k_cov.h"', '"mik_host.h"', "mikvario", "mikrige.h", "getenv", "strcmp", "atomic", "asm"):
            assert word not in text.replace("no atomic", ""), word
    assert "namespace mlk" in hdr and "#pragma clang fp contract(off)" in hdr and "static_assert" in hdr and "static_assert" in hip
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in hdr and "163840" in hdr
    build.build_library()
    assert build.up_to_date()
    plain = lambda flags: [c for c in flags if c not in build.COMPRESS and not c.startswith("-I")]
    assert plain(open(os.path.join(build.OBJ, "mik_lik.flags")).read().split()) == plain(build.FLAGS)
    # a change of the fourth library's header makes the whole stale, as the others' do
    assert os.path.join(csrc, "mik_k_lik.h") in build.lik_deps("mik_lik") and build.API_LIK in build.lik_deps("mik_lik")


def test_graft_entry_builds_through_build_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_library" in text


# ------------------------------------------------------------------------------------------------------------- the definitions
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_every_case_keeps_its_condition(name):
    logdet, G, kappa, bar = lc.reference(name)
    print("%s: kappa_2 %.3g bar %.3g" % (name, kappa, bar))
    assert logdet is not None, "%s is not positive definite on the CPU reference (pivot of column %s)" % (name, G)
    assert kappa <= lc.KAPPA_MAX and bar <= 2.5e-8, (name, kappa, bar)
    case = lc.CASES[name]
    X, _ = lc.inputs(case)
    Cm = lc.covariance_ld(X, case["model"], case["par"])
    assert np.all(np.diag(Cm) == np.longdouble(case["par"][0]) + np.longdouble(case["par"][2]))
    if case["model"] == "spherical":
        assert np.count_nonzero(Cm == 0) > 0  # a range shorter than the domain: exact zeros
    if "repeat" in case:
        k, j = case["repeat"]
        assert abs(float(Cm[k, j]) - case["par"][0]) <= 2 * lc.U * (case["par"][0] + case["par"][2])  # a coincident pair: C_ij = psill


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_the_float64_restatement_of_the_blocked_elimination_agrees_with_the_brute_force(name):
    case = lc.CASES[name]
    X, W = lc.inputs(case)
    ref_logdet, ref_G, kappa, bar = lc.reference(name)
    logdet, G = lc.blocked_float64(X, case["model"], case["par"], W)
    el, eg = lc.errors(logdet, G, ref_logdet, ref_G)
    print("%s: bar %.3g logdet error %.3g G error %.3g" % (name, bar, el, eg))
    assert el <= bar and eg <= bar, (name, el, eg, bar)
    if case["n"] > 2:  # (at N = 2 the bar is 2.5 units in the last place of a result that takes half a dozen roundings)
        assert 10 * max(el, eg) <= bar, "within a factor of ten of the bar: a finding to explain"


@pytest.mark.parametrize("name", sorted(lc.NOT_PD))
def test_the_not_positive_definite_inputs_fail_at_their_column_in_any_arithmetic(name):
    case, column = lc.NOT_PD[name]
    X, W = lc.inputs(case)
    assert lc.brute_force(X, case["model"], case["par"], W) == (None, column)
    for nb in (64, 32, 7):
        assert lc.blocked_float64(X, case["model"], case["par"], W, nb=nb) == (None, column)


def test_nll_from_gram_is_the_formula_and_works_field_by_field():
    rng = np.random.default_rng(3)
    n, F, p = 50, 3, 2
    A = rng.standard_normal((n, n))
    Cm = A @ A.T + n * np.eye(n)
    V, X = rng.standard_normal((n, F)), np.column_stack([np.ones(n), rng.random(n)])
    W = np.hstack([V, X])
    G = W.T @ np.linalg.solve(Cm, W)
    G = 0.5 * (G + G.T)
    logdet = float(np.linalg.slogdet(Cm)[1])
    lx = float(np.linalg.slogdet(X.T @ X)[1])
    assert abs(lk._pieces(X) - lx) <= 1e-12
    for reml in (False, True):
        got = lk.nll_from_gram(n, logdet, G, F, reml, lx)
        for f in range(F):
            beta = np.linalg.solve(G[F:, F:], G[F:, f])
            q = G[f, f] - G[F:, f] @ beta
            want = 0.5 * (n * math.log(2 * math.pi) + logdet + q) if not reml else \
                0.5 * ((n - p) * math.log(2 * math.pi) - lx + logdet + float(np.linalg.slogdet(G[F:, F:])[1]) + q)
            assert abs(got[f] - want) <= 1e-10 * abs(want)
            keep = [f] + list(range(F, F + p))  # the one-field call sees the same entries: the same bits
            assert lk.nll_from_gram(n, logdet, G[np.ix_(keep, keep)], 1, reml, lx)[0] == got[f]
    assert np.all(np.isinf(lk.nll_from_gram(n, math.inf, np.full((F + p, F + p), np.nan), F, True, lx)))
