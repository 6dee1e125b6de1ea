"""likelihood.neg_log_likelihood_grad / gram_grad / fit_variogram_ml(method='l-bfgs-b') without a GPU: the long-double reference gradient
of tests/_grad_cases.py is right (central differences of the long-double objective, the trend rebuilt at every step), the host's
derivatives of the adjusted coordinates are those of core.adjust_for_anisotropy, include/mikgrad.h declares what libmikgrad.so exports and
the ctypes mirror agrees, the fifth library is a unit of its own and the four others hold nothing of it, every refusal is raised before
anything is loaded, and the optimiser logic runs on a float64 NumPy stand-in for the one device call."""
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
from pykrige_amd import core
from pykrige_amd import likelihood as lk
from tests import _grad_cases as gc
from tests import _lik_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", sorted(gc.HOST_CASES))
def test_the_reference_gradient_is_the_derivative_of_the_long_double_objective(name):
    """Central differences with step 1e-5 (relative; degrees for angles) agree with the reference within 1e-6 of the bar's factor
    1/2 |P|_F |D_k|_F + |a_f|^2 |D_k|_F.  With drift='regional_linear' the differences rebuild the trend from the moved coordinates and
    the reference holds it: the invariance of the objective under X -> X A."""
    case = gc.HOST_CASES[name]
    grad, bar, kappa = gc.reference(name)
    assert kappa <= gc.KAPPA_MAX
    scale = bar / (case["n"] * gc.U * kappa)
    cd = gc.central_differences(case)
    worst = float(np.max(np.abs(cd - grad) / scale))
    print("%s: kappa_2 %.3g, worst |central difference - reference| / scale %.3g" % (name, kappa, worst))
    assert grad.shape == (case["F"], 3 + (2 if case["ndim"] == 2 else 5)) and worst <= 1e-6, (name, worst)
    adj, dco, V, X = gc.problem(case)
    d = lc.distances(adj)
    if "repeat" in case:
        k, j = case["repeat"]
        assert d[k, j] == 0.0
        Ds = gc.derivative_matrices(adj, dco, case["model"], case["par"])
        assert Ds[0][k, j] == 1 and Ds[1][k, j] == 0 and all(D[k, j] == 0 for D in Ds[2:])  # C_ij = psill stays
    if case["model"] == "spherical":
        beyond = d > case["par"][1]
        assert beyond.any()
        for D in gc.derivative_matrices(adj, dco, case["model"], case["par"]):
            assert np.all(D[beyond] == 0)  # exactly


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_every_device_case_keeps_its_condition(name):
    grad, bar, kappa = gc.reference(name)
    print("%s: kappa_2 %.3g" % (name, kappa))
    assert kappa <= gc.KAPPA_MAX and np.all(np.isfinite(grad.astype(np.float64))) and np.all(bar > 0)


def test_the_float64_stand_in_is_within_the_bar():
    for name in ("n63_sph3d_f1", "n65_gau_f9_p3", "n129_pair_f7_ml"):
        case = gc.CASES[name]
        adj, dco, V, X = gc.problem(case)
        grad, bar, _ = gc.reference(name)
        logdet, G, g64, info = gc.standin_gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])
        assert info == 0 and np.all(np.abs(g64 - grad) <= bar), name


@pytest.mark.parametrize("ndim", [2, 3])
def test_the_hosts_dcoords_are_the_derivatives_of_adjust_for_anisotropy(ndim):
    """Central differences with h = 1e-4: the truncation is h^2 / 6 times a third derivative of at most |x| (zero for a scaling), the
    rounding 4 u |x| / 2h = 5e-12 |x|: held to 1e-10 |x|."""
    rng = np.random.default_rng(5)
    raw = rng.random((30, ndim)) * 3.0
    sc, an = ([1.7], [25.0]) if ndim == 2 else ([1.4, 0.6], [10.0, -20.0, 35.0])
    D = lk.anisotropy_derivatives(raw, sc, an)
    assert D.shape == (len(sc) + len(an), 30, ndim)
    theta, h = sc + an, 1e-4
    for k in range(len(theta)):
        up, dn = list(theta), list(theta)
        up[k] += h
        dn[k] -= h
        cd = (gc.adjusted(raw, up[:len(sc)], up[len(sc):]) - gc.adjusted(raw, dn[:len(sc)], dn[len(sc):])) / (up[k] - dn[k])
        assert np.max(np.abs(cd - D[k])) <= 1e-10 * np.abs(raw).max(), k
    rot, stretch = core.anisotropy_matrices(ndim, sc, an)  # the scaling rows are rows of the rotation itself
    center = np.array([(raw[:, c].max() + raw[:, c].min()) / 2.0 for c in range(ndim)])
    assert np.allclose(D[0][:, 1], (raw - center) @ rot[1], rtol=0, atol=1e-14) and np.all(D[0][:, 0] == 0)


# ------------------------------------------------------------------------------------------------------------- the interface
def test_signatures_and_docstrings():
    assert list(inspect.signature(lk.neg_log_likelihood_grad).parameters)[:2] == ["x", "y"]
    assert list(inspect.signature(lk.gram_grad).parameters) == ["coords", "dcoords", "model", "parameters", "V", "X", "reml"]
    assert lk.GRAD_NAMES_2D == ("psill", "range", "nugget", "anisotropy_scaling", "anisotropy_angle")
    assert lk.GRAD_NAMES_3D == ("psill", "range", "nugget") + lk._ANIS3 and lk.MAXGEOM == 5
    doc = " ".join(lk.neg_log_likelihood_grad.__doc__.split())
    for phrase in ("bit for bit", "(F, 3 + ng)", "PARTIAL sill", "angles per degree", "regional_linear", "column space", "is exact",
                   "X -> X A", "``inf``", "NaN", "no CPU fallback"):
        assert phrase in doc, phrase
    doc = " ".join(lk.fit_variogram_ml.__doc__.split())
    for phrase in ("method='nelder-mead'", "method='l-bfgs-b'", "jac=True", "chain rule", "does not raise", "``message`` says so",
                   "device calls of both kinds"):
        assert phrase in doc, phrase
    for cls in (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D):
        sig = inspect.signature(cls.neg_log_likelihood_grad)
        assert list(sig.parameters) == ["self", "variogram_parameters", "reml", "anisotropy"]
        assert sig.parameters["variogram_parameters"].default is None and sig.parameters["reml"].default is True
        doc = " ".join(cls.neg_log_likelihood_grad.__doc__.split())
        for phrase in ("bit for bit", "regional_linear", "NotImplementedError", "geographic", "device group", "'custom'", "per degree"):
            assert phrase in doc, (cls.__name__, phrase)
        assert "method='l-bfgs-b'" in cls.fit_variogram_ml.__doc__


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a library was loaded before the arguments were checked")

    monkeypatch.setattr(lk, "_lib", None)
    monkeypatch.setattr(lk, "_lib_grad", None)
    monkeypatch.setattr(lk, "load", boom)
    monkeypatch.setattr(lk, "load_grad", boom)
    monkeypatch.setattr(lk.C, "CDLL", boom)


def test_every_refusal_is_raised_before_anything_is_loaded(no_library):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(20), rng.random(20), rng.random(20), rng.standard_normal(20)
    full = [1.1, 0.5, 0.1]
    for args, kw, exc, match in (
            ((x, y, v, "linear", full), {}, ValueError, "unbounded"), ((x, y, v, "power", full), {}, ValueError, "unbounded"),
            ((x, y, v, "custom", full), {}, NotImplementedError, "custom"), ((x, y, v, "cubic", full), {}, ValueError, "must be one of"),
            ((x, y, np.where(np.arange(20) == 2, np.inf, v), "exponential", full), {}, ValueError, "values must be finite"),
            ((np.where(np.arange(20) == 2, np.nan, x), y, v, "exponential", full), {}, ValueError, "coordinates must be finite"),
            ((x, y[:-1], v, "exponential", full), {}, ValueError, "same length"),
            ((x, y, np.zeros((20, 33)), "exponential", full), {}, ValueError, "F <= 32"),
            ((x[:1], y[:1], v[:1], "exponential", full), {}, ValueError, "two stations"),
            ((x, y, v, "exponential", full), dict(drift=np.ones((20, 1))), ValueError, "rank-deficient"),
            ((x, y, v, "exponential", full), dict(drift=rng.random((20, 8))), ValueError, "at most 8 trend columns"),
            ((x, y, v, "exponential", full), dict(drift="quadratic"), ValueError, "regional_linear"),
            ((x, y, v, "exponential", full), dict(anisotropy_scaling_z=2.0), ValueError, "3-D classes"),
            ((x, y, z, v, "exponential", full), dict(anisotropy_scaling=2.0), ValueError, "2-D classes"),
            ((x, y, v, "exponential", full), dict(anisotropy_scaling=0.0), ValueError, "scaling must be positive"),
            ((x, y, v, "exponential", full), dict(anisotropy_angle=float("nan")), ValueError, "must be finite"),
            ((x, y, v, "exponential", [0.1, 0.5, 0.1]), {}, ValueError, "partial sill > 0"),
            ((x, y, v, "exponential", None), {}, ValueError, "must be given"),
            ((x, y, v, "exponential", full), dict(nlags=6), TypeError, "unexpected argument"),
            ((x, y, v), {}, TypeError, "variogram_model is required")):
        with pytest.raises(exc, match=match):
            lk.neg_log_likelihood_grad(*args, **kw)
    for method in ("bfgs", "newton", 3):
        with pytest.raises(ValueError, match="method must be one of 'nelder-mead', 'l-bfgs-b'"):
            lk.fit_variogram_ml(x, y, v, "exponential", start=full, method=method)
    with pytest.raises(ValueError, match="constant"):
        lk.fit_variogram_ml(x, y, np.ones(20), "exponential", method="l-bfgs-b")
    kw = dict(variogram_model="exponential", variogram_parameters=full)
    objs = [pa.OrdinaryKriging(x, y, v, **kw), pa.UniversalKriging3D(x, y, z, v, drift_terms=["regional_linear"], **kw)]

    class Group:
        n_devices = 2

    for obj in objs:
        obj._handle = Group()
        try:
            with pytest.raises(ValueError, match="device group of 2"):
                obj.neg_log_likelihood_grad()
        finally:
            obj._handle = None
        with pytest.raises(TypeError, match="unexpected argument"):
            obj.neg_log_likelihood_grad(nlags=6)
        with pytest.raises(ValueError, match="method must be one of"):
            obj.fit_variogram_ml(method="simplex")
    with pytest.raises(ValueError, match="geographic"):
        pa.OrdinaryKriging(360.0 * x, 90.0 * y, v, coordinates_type="geographic", **kw).neg_log_likelihood_grad()
    with pytest.raises(ValueError, match="unbounded"):
        pa.OrdinaryKriging(x, y, v, variogram_model="linear", variogram_parameters=[1.0, 0.1]).neg_log_likelihood_grad()
    with pytest.raises(NotImplementedError, match="regional_linear is the only drift term"):
        pa.UniversalKriging(x, y, v, drift_terms=["point_log"], point_drift=[[0.5, 0.5, 1.0]], **kw).neg_log_likelihood_grad()


# ------------------------------------------------------------------------------------------------------------- the library
def _declared():
    text = open(os.path.join(ROOT, "include", "mikgrad.h")).read()
    verbatim = " ".join(text.split()).replace(" * ", " ")
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return verbatim, text, sorted(set(re.findall(r"\b(mlg_[a-z_0-9]+)\s*\(", text)))


def test_the_header_declares_what_the_library_exports_and_the_ctypes_mirror_agrees():
    from pykrige_amd import build

    build.build_library()
    assert os.path.exists(build.OUT_GRAD) and build.OUT_GRAD == lk.LIB_PATH_GRAD and build.API_GRAD.endswith("mikgrad.h")
    verbatim, text, names = _declared()
    assert names == sorted(lk.SIGNATURES_GRAD) == ["mlg_abi_version", "mlg_grad", "mlg_last_error"]
    for phrase in ("grad[f][k] = 1/2 S_k - 1/2 T_kf", "M = P under REML (reml = 1) and M = Q under ML (reml = 0)", "X is held fixed",
                   "mlk_gram's bit for bit", "c_p = 1 - f(d)", "c_r = -psill df/drange", "c_g = -psill f'(d) / d, defined as 0 where d = 0",
                   "dC / dnugget = I: the diagonal only", "keep C_ij = psill", "beyond the range every derivative is exactly 0",
                   "f'(range) = 0", "MLG_ENOTPD", "launches nothing further", "(2n + 48)^2", "[[C, ., .], [W^T, 0, .], [I, 0, 0]]"):
        assert phrase in verbatim, phrase
    lib = lk.load_grad()
    assert lib.mlg_abi_version() == lk.ABI_VERSION_GRAD == int(re.search(r"#define MLG_ABI_VERSION (\d+)", text).group(1)) == 1
    for macro, value in (("MLG_MAXFIELDS", lk.MAXFIELDS), ("MLG_MAXTREND", lk.MAXTREND), ("MLG_MAXGEOM", lk.MAXGEOM), ("MLG_EINVAL", "(-1)"),
                         ("MLG_ENOTPD", "(-2)"), ("MLG_EHIP", "(-3)"), ("MLG_GAUSSIAN", 0), ("MLG_EXPONENTIAL", 1), ("MLG_SPHERICAL", 2),
                         ("MLG_HOLE_EFFECT", 3)):
        assert re.search(r"#define %s %s(?=\s)" % (macro, re.escape(str(value))), text), macro
    assert (lk.MLG_EINVAL, lk.MLG_ENOTPD, lk.MLG_EHIP) == (-1, -2, -3)
    ctype = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
             "const double *": lk._dp, "double *": lk._dp, "int32_t *": lk._i32p}
    flat = " ".join(text.split())
    args = re.search(r"int mlg_grad\((.*?)\);", flat).group(1).split(",")
    want = [ctype[re.match(r"\s*((?:const )?\w+ \*|\w+)", a).group(1)] for a in args]
    assert lk.SIGNATURES_GRAD["mlg_grad"] == (ctypes.c_int, want) and len(want) == 19
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "-C", build.OUT_GRAD], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert {e for e in exported if e.startswith("mlg_")} == set(names)
        assert not {e for e in exported if e.startswith("mlk_")}  # the fourth library's kernels, not its C ABI
        kernels = sorted({m.group(1) for m in re.finditer(r"__device_stub__([A-Za-z_0-9]+)\(", out)})
        assert kernels == ["k_grad_pairs", "k_grad_seed", "k_lik_assemble", "k_lik_potrf", "k_lik_syrk", "k_lik_trsm"], kernels
        for other in (build.OUT, build.OUT_VARIO, build.OUT_VARIO3, build.OUT_LIK):  # nothing of the fifth library in the four others
            sym = subprocess.run(["nm", "-D", "-C", other], capture_output=True, text=True, check=True).stdout
            assert "mlg_" not in sym and "k_grad" not in sym, other
        assert "mkv_" not in out and "mkv3_" not in out and "k_vario" not in out and "mik_" not in out  # nor the reverse
    # calls that are refused launch nothing and need no GPU: the library's own checks answer MLG_EINVAL with a reason
    c, e, vv, xx = np.zeros(6), np.zeros(12), np.ones(3), np.ones(3)
    g, gr = np.full(4, 7.0), np.full(5, 7.0)
    p = lambda a: a.ctypes.data_as(lk._dp)
    logdet, info = ctypes.c_double(7.0), ctypes.c_int32(5)

    def call(n=3, ndim=2, coords=c, ng=2, dcoords=e, model=1, psill=1.0, rng=0.5, nugget=0.1, V=vv, F=1, X=xx, pp=1, reml=1):
        return lib.mlg_grad(0, n, ndim, p(coords), ng, None if dcoords is None else p(dcoords), model, psill, rng, nugget, p(V), F, p(X), pp,
                            reml, ctypes.byref(logdet), p(g), p(gr), ctypes.byref(info))

    for kw, reason in ((dict(n=1), b"two stations"), (dict(ndim=4), b"ndim"), (dict(ng=-1), b"MLG_MAXGEOM"), (dict(ng=6), b"MLG_MAXGEOM"),
                       (dict(dcoords=None), b"NULL dcoords"), (dict(F=0), b"MLG_MAXFIELDS"), (dict(F=33), b"MLG_MAXFIELDS"),
                       (dict(pp=0), b"MLG_MAXTREND"), (dict(pp=9), b"MLG_MAXTREND"), (dict(reml=2), b"reml"), (dict(model=4), b"model"),
                       (dict(model=-1), b"model"), (dict(psill=0.0), b"psill > 0"), (dict(rng=-1.0), b"range > 0"),
                       (dict(nugget=-0.5), b"nugget >= 0"), (dict(psill=float("inf")), b"finite"),
                       (dict(coords=np.array([0.0, np.nan, 1.0, 0.0, 1.0, 2.0])), b"coordinates must be finite"),
                       (dict(dcoords=np.where(np.arange(12) == 7, np.inf, e)), b"dcoords must be finite"),
                       (dict(V=np.array([1.0, np.inf, 0.0])), b"V must be finite"), (dict(X=np.array([1.0, np.nan, 0.0])), b"X must be finite"),
                       (dict(n=2 ** 30), b"fits no device")):
        assert call(**kw) == lk.MLG_EINVAL and reason in lib.mlg_last_error(), (kw, lib.mlg_last_error())
    assert logdet.value == 7.0 and np.all(g == 7.0) and np.all(gr == 7.0)  # a refused call writes no result


def test_a_missing_or_stale_library_is_answered_as_the_others_are(monkeypatch):
    monkeypatch.setattr(lk, "_lib_grad", None)
    monkeypatch.setattr(lk, "LIB_PATH_GRAD", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    with pytest.raises(ImportError, match=r"is missing -- build it with `python -m pykrige_amd.build`"):
        lk.load_grad()
    monkeypatch.undo()
    real = lk.load_grad()

    class Old:
        def __getattr__(self, name):
            if name == "mlg_grad":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(lk, "_lib_grad", None)
    monkeypatch.setattr(lk.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mlg_grad.*rebuild"):
        lk.load_grad()


def test_the_fifth_library_is_a_unit_of_its_own():
    from pykrige_amd import build

    assert list(build.UNITS_GRAD) == ["mik_grad"] and build.UNITS_GRAD["mik_grad"] == ("mik_grad.hip", ["mik_k_grad.h", "mik_k_lik.h"])
    assert build.UNITS_LIK["mik_lik"] == ("mik_lik.hip", ["mik_k_lik.h"]) and len(build.UNITS) == 10 and "mik_grad" not in build.UNITS
    assert not any("grad" in os.path.basename(d) for d in build.all_sources() + build.lik_deps("mik_lik"))
    assert build.OUT_GRAD.endswith("libmikgrad.so") and "libmikgrad.so" in build.__doc__
    assert not any("lik" in name for name in ("mikgrad.h", "mik_grad.hip", "mik_k_grad.h", "libmikgrad.so"))
    csrc = os.path.join(ROOT, "pykrige_amd", "csrc")
    hip, hdr = open(os.path.join(csrc, "mik_grad.hip")).read(), open(os.path.join(csrc, "mik_k_grad.h")).read()
    for text in (hip, hdr):  # no code of the other three libraries; no options, no environment, no atomics, no inline assembly
        for word in ('"mik_k_vario', '"mik_dev.h"', '"mik_k_cov.h"', '"mik_host.h"', "mikvario", "mikrige.h", "miklik.h", "getenv", "strcmp",
                     "atomic", "asm"):
            assert word not in text.replace("no atomic", ""), word
    assert '#include "mik_k_lik.h"' in hdr and "namespace mlg" in hdr and "#pragma clang fp contract(off)" in hdr
    assert "static_assert" in hdr and "static_assert" in hip and "163840" in hdr and "163840" in hip
    build.build_library()
    assert build.up_to_date()
    plain = lambda flags: [c for c in flags if c not in build.COMPRESS and not c.startswith("-I")]
    assert plain(open(os.path.join(build.OBJ, "mik_grad.flags")).read().split()) == plain(build.FLAGS)
    deps = build.grad_deps("mik_grad")
    assert os.path.join(csrc, "mik_k_grad.h") in deps and os.path.join(csrc, "mik_k_lik.h") in deps and build.API_GRAD in deps
    # up_to_date() sees the fifth library: a library older than its header is stale
    old = os.path.getmtime(build.OUT_GRAD)
    try:
        os.utime(build.OUT_GRAD, (1.0, 1.0))
        assert not build.up_to_date()
    finally:
        os.utime(build.OUT_GRAD, (old, old))
    assert build.up_to_date()
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "build_library" in text and "load_grad" in text


# ------------------------------------------------------------------------------------------------------------- the optimiser
def _field(n=60):
    rng = np.random.default_rng(77)
    raw = rng.random((n, 2)) * [4.0, 3.0]
    adj = gc.adjusted(raw, [2.0], [30.0])
    Cm = lc.covariance_ld(adj, "exponential", [0.95, 1.2, 0.05]).astype(np.float64)
    return raw[:, 0], raw[:, 1], 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)


@pytest.fixture
def stand_in(monkeypatch):
    """The two device calls replaced by float64 NumPy; loading either library fails the test.  Returns the call counters."""
    calls = {"gram": 0, "gram_grad": 0}

    def boom(*a, **k):
        raise AssertionError("a library was loaded")

    def gram(*a):
        calls["gram"] += 1
        return gc.standin_gram(*a)

    def gram_grad(*a):
        calls["gram_grad"] += 1
        return gc.standin_gram_grad(*a)

    monkeypatch.setattr(lk, "load", boom)
    monkeypatch.setattr(lk, "load_grad", boom)
    monkeypatch.setattr(lk, "gram", gram)
    monkeypatch.setattr(lk, "gram_grad", gram_grad)
    return calls


def test_the_quasi_newton_fit_on_a_stand_in_is_never_worse_than_its_start(stand_in):
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    at_start = lk.neg_log_likelihood(x, y, v, "exponential", start)
    before = dict(stand_in)
    fit = lk.fit_variogram_ml(x, y, v, "exponential", start=start, fit_anisotropy=True, method="l-bfgs-b")
    spent = stand_in["gram"] - before["gram"] + stand_in["gram_grad"] - before["gram_grad"]
    print(fit, fit.message)
    assert math.isfinite(fit.nll) and fit.nll <= at_start and fit.nll < at_start - 0.1  # it moved
    assert fit.n_evaluations == spent and stand_in["gram_grad"] > 0 and set(fit.anisotropy) == set(lk._ANIS2)
    nm = lk.fit_variogram_ml(x, y, v, "exponential", start=start, fit_anisotropy=True)
    print(nm, nm.message)
    assert fit.nll <= nm.nll + 1e-4 and fit.n_evaluations < nm.n_evaluations
    # the nll it reports is the objective at what it reports
    again = lk.neg_log_likelihood(x, y, v, "exponential", fit.variogram_parameters, **fit.anisotropy)
    assert abs(again - fit.nll) <= 1e-9 * abs(fit.nll)
    # a fixed anisotropy: three parameters, no geometry derivatives asked for
    fit3 = lk.fit_variogram_ml(x, y, v, "exponential", start=start, method="L-BFGS-B", anisotropy_scaling=2.0, anisotropy_angle=30.0)
    assert fit3.anisotropy == dict(anisotropy_scaling=2.0, anisotropy_angle=30.0)
    assert fit3.nll <= lk.neg_log_likelihood(x, y, v, "exponential", start, anisotropy_scaling=2.0, anisotropy_angle=30.0)


def test_a_trial_that_is_not_positive_definite_does_not_raise(stand_in, monkeypatch):
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    at_start = lk.neg_log_likelihood(x, y, v, "exponential", start)
    seen = [0]

    def sometimes_inf(coords, dcoords, model, parameters, V, X, reml):
        seen[0] += 1
        if seen[0] in (2, 3, 7):  # trials of the line search answered as not positive definite
            F, m, ng = V.shape[1], V.shape[1] + X.shape[1], len(dcoords)
            return math.inf, np.full((m, m), np.nan), np.full((F, 3 + ng), np.nan), 1
        return gc.standin_gram_grad(coords, dcoords, model, parameters, V, X, reml)

    monkeypatch.setattr(lk, "gram_grad", sometimes_inf)
    fit = lk.fit_variogram_ml(x, y, v, "exponential", start=start, fit_anisotropy=True, method="l-bfgs-b")
    print(fit, fit.message)
    assert seen[0] >= 7 and math.isfinite(fit.nll) and fit.nll <= at_start

    def always_inf_after_the_first(coords, dcoords, model, parameters, V, X, reml):
        seen[0] += 1
        if seen[0] > 1:
            F, m, ng = V.shape[1], V.shape[1] + X.shape[1], len(dcoords)
            return math.inf, np.full((m, m), np.nan), np.full((F, 3 + ng), np.nan), 1
        return gc.standin_gram_grad(coords, dcoords, model, parameters, V, X, reml)

    seen[0] = 0
    monkeypatch.setattr(lk, "gram_grad", always_inf_after_the_first)
    fit = lk.fit_variogram_ml(x, y, v, "exponential", start=start, method="l-bfgs-b")
    print(fit, fit.message)
    assert math.isfinite(fit.nll) and fit.nll <= at_start
    assert "Nelder-Mead" in fit.message and "could not continue" in fit.message  # the line search gave up; the simplex finished


def test_the_default_method_takes_the_old_path_and_never_touches_the_new_library(stand_in, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the default method called the gradient path")

    monkeypatch.setattr(lk, "gram_grad", boom)
    monkeypatch.setattr(lk, "anisotropy_derivatives", boom)
    x, y, v = _field()
    start = [1.5, 0.6, 0.2]
    fit = lk.fit_variogram_ml(x, y, v, "exponential", start=start)
    same = lk.fit_variogram_ml(x, y, v, "exponential", start=start, method="nelder-mead")
    assert fit.n_evaluations == same.n_evaluations and fit.nll == same.nll and fit.variogram_parameters == same.variogram_parameters
    assert stand_in["gram"] == fit.n_evaluations + same.n_evaluations
    ok = pa.OrdinaryKriging(x, y, v, variogram_model="exponential", variogram_parameters=start)
    assert ok.fit_variogram_ml().nll == fit.nll
