"""likelihood.gram / neg_log_likelihood / fit_variogram_ml on the GPU against the long-double brute force of tests/_lik_cases.py.

The bar (derived there): every entry of G within N 2^-52 kappa_2(C) of the reference relative to sqrt(G_aa G_bb), logdet within the same
number absolutely.  The shapes are the smallest at which the blocking of mik_k_lik.h can go wrong -- N = 2, 63, 64, 65, 127, 129 around
the 64-column block and the 128-row update tile, N = 200, 333, 700 with several block columns and update tiles, m = 1, 7, 16, 17, 40 around
the 16-row padding of W^T, and the whole tiles N = 128, 192, 256 | 257, 512 | 513 with m = 24 | 25, 32 | 33 -- in 2-D and 3-D, each model,
one coincident pair with a nugget, and three inputs that are not positive definite.  Every figure is printed before it is asserted;
profiles/likelihood_parity.txt and profiles/fit_edges_parity.txt hold them."""
import ctypes
import functools
import math

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import core
from pykrige_amd import likelihood as lk
from tests import _lik_cases as lc

pytestmark = pytest.mark.gpu
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def device(name):
    """(logdet, G) of CASES[name] from the device, once; do not write into it."""
    case = lc.CASES[name]
    X, W = lc.inputs(case)
    return lk.gram(X, case["model"], case["par"], W)


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_gram_is_within_the_bar_symmetric_and_reproducible(name):
    case = lc.CASES[name]
    ref_logdet, ref_G, kappa, bar = lc.reference(name)
    logdet, G = device(name)
    el, eg = lc.errors(logdet, G, ref_logdet, ref_G)
    (lc.record if name in lc.EDGES else print)("gram      %-16s N %4d m %2d kappa_2 %9.3g bar %9.3g logdet error %9.3g G error %9.3g worst/bar %8.3g"
                                               % (name, case["n"], case["m"], kappa, bar, el, eg, max(el, eg) / bar))
    assert G.shape == (case["m"], case["m"]) and np.array_equal(G, G.T)
    assert el <= bar and eg <= bar, (name, el, eg, bar)
    X, W = lc.inputs(case)
    again_logdet, again_G = lk.gram(X, case["model"], case["par"], W)
    assert again_logdet == logdet and np.array_equal(again_G.view(np.int64), G.view(np.int64))  # the same bits


@pytest.mark.parametrize("name", ["n129_exp3d_m40", "n333_sph_m7"])
def test_an_entry_of_g_does_not_depend_on_the_columns_beside_it(name):
    case = lc.CASES[name]
    X, W = lc.inputs(case)
    logdet, G = device(name)
    for cols in ([0], [2, 0], [case["m"] - 1, 1, 3]):
        ld1, G1 = lk.gram(X, case["model"], case["par"], W[:, cols])
        assert ld1 == logdet and np.array_equal(G1.view(np.int64), np.ascontiguousarray(G[np.ix_(cols, cols)]).view(np.int64)), cols


@pytest.mark.parametrize("name", sorted(lc.NOT_PD))
def test_a_matrix_that_is_not_positive_definite_is_answered_and_harms_nothing(name):
    case, column = lc.NOT_PD[name]
    X, W = lc.inputs(case)
    logdet, G = lk.gram(X, case["model"], case["par"], W)
    assert logdet == math.inf and G.shape == (case["m"],) * 2 and np.all(np.isnan(G))
    lib = lk.load()
    ct, wt = np.ascontiguousarray(X.T), np.ascontiguousarray(W.T)
    out, ld, info = np.full((case["m"],) * 2, 7.0), ctypes.c_double(7.0), ctypes.c_int32(-5)
    rc = lib.mlk_gram(0, case["n"], case["ndim"], ct.ctypes.data_as(lk._dp), lk.MODEL_IDS[case["model"]], *case["par"],
                      wt.ctypes.data_as(lk._dp), case["m"], ctypes.byref(ld), out.ctypes.data_as(lk._dp), ctypes.byref(info))
    print("%s: rc %d info %d (reference: column %d)" % (name, rc, info.value, column))
    assert rc == lk.MLK_ENOTPD and info.value == column and b"not positive definite" in lib.mlk_last_error()
    assert ld.value == 7.0 and np.all(out == 7.0)  # never a partial result
    v = W[:, 0]
    assert lk.neg_log_likelihood(*X.T, v, case["model"], [case["par"][0] + case["par"][2], case["par"][1], case["par"][2]]) == math.inf
    # a following valid call is unaffected
    good = "n200_exp_m1"
    first = device(good)
    Xg, Wg = lc.inputs(lc.CASES[good])
    again = lk.gram(Xg, lc.CASES[good]["model"], lc.CASES[good]["par"], Wg)
    assert again[0] == first[0] and np.array_equal(again[1], first[1])


def test_forty_one_columns_are_refused_and_harm_nothing():
    """MLK_MAXCOLS = 40 is a case; 41 is refused by ``gram`` with a ValueError, and the valid call that follows returns the bits it
    returned before."""
    good = "n129_exp3d_m40"
    case = lc.CASES[good]
    X, W = lc.inputs(case)
    first = device(good)
    with pytest.raises(ValueError, match="MLK_MAXCOLS"):
        lk.gram(X, case["model"], case["par"], np.hstack([W, W[:, :1]]))
    lib = lk.load()  # the library's own refusal, past the Python check
    ct, wt = np.ascontiguousarray(X.T), np.ascontiguousarray(np.hstack([W, W[:, :1]]).T)
    out, ld, info = np.full((41, 41), 7.0), ctypes.c_double(7.0), ctypes.c_int32(-5)
    rc = lib.mlk_gram(0, case["n"], case["ndim"], ct.ctypes.data_as(lk._dp), lk.MODEL_IDS[case["model"]], *case["par"],
                      wt.ctypes.data_as(lk._dp), 41, ctypes.byref(ld), out.ctypes.data_as(lk._dp), ctypes.byref(info))
    assert rc == lk.MLK_EINVAL and b"MLK_MAXCOLS" in lib.mlk_last_error() and ld.value == 7.0 and np.all(out == 7.0)
    again = lk.gram(X, case["model"], case["par"], W)
    assert again[0] == first[0] and np.array_equal(again[1].view(np.int64), first[1].view(np.int64))


# ------------------------------------------------------------------------------------------------------------- the likelihood
def _problem(n, ndim, seed, nf=1):
    rng = np.random.default_rng(seed)
    raw = rng.random((n, ndim)) * ([3.0, 2.0, 1.0][:ndim])
    v = np.sin(2.0 * raw[:, 0])[:, None] + 0.5 * raw[:, 1][:, None] + 0.4 * rng.standard_normal((n, nf))
    return raw, v


def _reference_nll(raw, v, model, full, scaling, angle, drift, reml):
    """The formulas of neg_log_likelihood on the long-double pieces, and the tolerance the device's pieces allow.

    G = D R D with D = diag(sqrt(G_aa)): every entry of R is off by at most `bar`.  Q_f / G_ff = 1 - r^T R_xx^-1 r moves by at most
    bar (1 + s)^2 with s = |R_xx^-1 r|_1; log det G_xx = sum log G_aa + log det R_xx by at most bar (p + t), t = sum |R_xx^-1|; logdet by
    bar.  Half of their sum, and 16 roundings of the float64 evaluation of a number of size |nll|."""
    n = len(raw)
    center = [(raw[:, c].max() + raw[:, c].min()) / 2.0 for c in range(raw.shape[1])]
    adj = core.adjust_for_anisotropy(raw, center, scaling, angle)
    par = [full[0] - full[2], full[1], full[2]]
    X = np.ones((n, 1)) if drift is None else np.hstack([np.ones((n, 1)), adj if isinstance(drift, str) else drift])
    F, p = v.shape[1], X.shape[1]
    logdet, G = lc.brute_force(adj, model, par, np.hstack([v, X]))
    kappa = float(np.linalg.cond(lc.covariance_ld(adj, model, par).astype(np.float64), 2))
    assert kappa <= lc.KAPPA_MAX
    bar = n * lc.U * kappa
    Xl = X.astype(LD)
    G64 = G.astype(np.float64)
    ldx = LD(np.linalg.slogdet((Xl.T @ Xl).astype(np.float64))[1])
    d = np.sqrt(np.diag(G64))
    R = G64 / d[:, None] / d[None, :]
    Rinv = np.linalg.inv(R[F:, F:])
    out, tol = np.zeros(F), np.zeros(F)
    lgx = LD(np.linalg.slogdet(G64[F:, F:])[1])
    for f in range(F):
        beta = np.linalg.solve(G64[F:, F:], G64[F:, f])
        q = G[f, f] - LD(G64[F:, f] @ beta)
        s = np.abs(Rinv @ R[F:, f]).sum()
        if reml:
            val = LD(0.5) * ((n - p) * LD(math.log(2 * math.pi)) - ldx + logdet + lgx + q)
            wobble = bar * (1.0 + float(G64[f, f]) * (1.0 + s) ** 2 + p + np.abs(Rinv).sum())
        else:
            val = LD(0.5) * (n * LD(math.log(2 * math.pi)) + logdet + q)
            wobble = bar * (1.0 + float(G64[f, f]) * (1.0 + s) ** 2)
        out[f], tol[f] = float(val), 0.5 * wobble + 16 * lc.U * abs(float(val))
    return out, tol


@pytest.mark.parametrize("ndim,drift", [(2, None), (2, "array"), (3, None), (3, "regional_linear")])
def test_neg_log_likelihood_is_the_formula_on_the_long_double_pieces(ndim, drift):
    raw, v = _problem(200, ndim, 11 + ndim, nf=3)
    full = [1.2, 0.9, 0.1]
    anis = dict(anisotropy_scaling=1.7, anisotropy_angle=25.0) if ndim == 2 else dict(
        anisotropy_scaling_y=1.4, anisotropy_scaling_z=0.6, anisotropy_angle_x=10.0, anisotropy_angle_y=-20.0, anisotropy_angle_z=35.0)
    sc, an = list(anis.values())[:ndim - 1], list(anis.values())[ndim - 1:]
    if drift == "array":
        drift = np.column_stack([raw[:, 0], raw[:, 0] * raw[:, 1]])
    for reml in (False, True):
        got = lk.neg_log_likelihood(*raw.T, v, "exponential", full, drift=drift, reml=reml, **anis)
        want, tol = _reference_nll(raw, v, "exponential", full, sc, an, drift, reml)
        print("ndim %d reml %s: nll %s error %s tolerance %s" % (ndim, reml, got, np.abs(got - want), tol))
        assert got.shape == (3,) and np.all(np.abs(got - want) <= tol), (got, want, tol)
        for f in range(3):  # column f of an (N, F) call equals the one-field call bit for bit
            one = lk.neg_log_likelihood(*raw.T, v[:, f], "exponential", full, drift=drift, reml=reml, **anis)
            assert isinstance(one, float) and one == got[f]
        as_dict = lk.neg_log_likelihood(*raw.T, v, "exponential", {"sill": 1.2, "range": 0.9, "nugget": 0.1}, drift=drift, reml=reml, **anis)
        assert np.array_equal(as_dict, got)


def test_the_ml_likelihood_is_scipys_logpdf_at_the_gls_mean():
    from scipy.stats import multivariate_normal

    raw, v = _problem(65, 2, 5)
    v = v[:, 0]
    full = [0.9, 1.1, 0.15]
    par = [full[0] - full[2], full[1], full[2]]
    Cm = lc.covariance_ld(raw, "spherical", par).astype(np.float64)
    for drift in (None, raw[:, :1]):
        X = np.ones((65, 1)) if drift is None else np.hstack([np.ones((65, 1)), drift])
        beta = np.linalg.solve(X.T @ np.linalg.solve(Cm, X), X.T @ np.linalg.solve(Cm, v))
        want = -multivariate_normal.logpdf(v, mean=X @ beta, cov=Cm)
        got = lk.neg_log_likelihood(raw[:, 0], raw[:, 1], v, "spherical", full, drift=drift, reml=False)
        print("logpdf %.15g device %.15g" % (want, got))
        assert abs(got - want) <= 1e-10 * abs(want)  # (scipy's own route is an eigendecomposition in float64)


def test_the_methods_are_the_module_functions_on_the_objects_stations():
    raw, v = _problem(129, 3, 21)
    v = v[:, 0]
    x, y, z = raw.T
    kw = dict(variogram_model="gaussian", variogram_parameters=[1.0, 1.5, 0.2])
    a2, a3 = dict(anisotropy_scaling=2.0, anisotropy_angle=40.0), dict(anisotropy_scaling_y=1.5, anisotropy_scaling_z=0.5, anisotropy_angle_x=15.0)
    ok = pa.OrdinaryKriging(x, y, v, **kw, **a2)
    assert ok.neg_log_likelihood() == lk.neg_log_likelihood(x, y, v, "gaussian", [1.0, 1.5, 0.2], **a2)
    assert ok.neg_log_likelihood(reml=False, anisotropy_angle=10.0) == lk.neg_log_likelihood(
        x, y, v, "gaussian", [1.0, 1.5, 0.2], reml=False, anisotropy_scaling=2.0, anisotropy_angle=10.0)
    assert ok.neg_log_likelihood([0.8, 1.0, 0.1]) == lk.neg_log_likelihood(x, y, v, "gaussian", [0.8, 1.0, 0.1], **a2)
    uk = pa.UniversalKriging(x, y, v, drift_terms=["regional_linear"], **kw, **a2)
    assert uk.neg_log_likelihood() == lk.neg_log_likelihood(x, y, v, "gaussian", [1.0, 1.5, 0.2], drift=uk._coords_adj, **a2)
    assert uk.neg_log_likelihood() != ok.neg_log_likelihood()
    assert pa.UniversalKriging(x, y, v, **kw, **a2).neg_log_likelihood() == ok.neg_log_likelihood()  # no drift term: a constant mean
    ok3 = pa.OrdinaryKriging3D(x, y, z, v, **kw, **a3)
    assert ok3.neg_log_likelihood() == lk.neg_log_likelihood(x, y, z, v, "gaussian", [1.0, 1.5, 0.2], **a3)
    uk3 = pa.UniversalKriging3D(x, y, z, v, drift_terms=["regional_linear"], **kw, **a3)
    assert uk3.neg_log_likelihood() == lk.neg_log_likelihood(x, y, z, v, "gaussian", [1.0, 1.5, 0.2], drift=uk3._coords_adj, **a3)
    fit = ok3.fit_variogram_ml()
    print(fit)
    assert fit.nll <= ok3.neg_log_likelihood() and set(fit.anisotropy) == set(lk._ANIS3) and fit.anisotropy["anisotropy_scaling_y"] == 1.5


def test_the_fit_is_a_minimiser_and_its_result_kriges():
    """A field simulated on the host from a known exponential model with a 2 : 1 anisotropy at 30 degrees, N = 400, by a Cholesky factor
    with a fixed seed.  The fit's nll is no greater than at the truth and at the start: properties of a minimiser.  No closeness of the
    estimates to the truth is asserted -- that is statistics, not a property of the code."""
    rng = np.random.default_rng(2024)
    n = 400
    raw = rng.random((n, 2)) * [4.0, 3.0]
    truth, anis = [1.0, 1.2, 0.05], dict(anisotropy_scaling=2.0, anisotropy_angle=30.0)
    center = [(raw[:, c].max() + raw[:, c].min()) / 2.0 for c in range(2)]
    adj = core.adjust_for_anisotropy(raw, center, [2.0], [30.0])
    Cm = lc.covariance_ld(adj, "exponential", [truth[0] - truth[2], truth[1], truth[2]]).astype(np.float64)
    v = 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)
    x, y = raw.T
    at_truth = lk.neg_log_likelihood(x, y, v, "exponential", truth, **anis)
    fit = lk.fit_variogram_ml(x, y, v, "exponential", fit_anisotropy=True)
    ok0 = pa.OrdinaryKriging(x, y, v, variogram_model="exponential")  # the start: the constructor's least-squares fit, isotropic
    at_start = ok0.neg_log_likelihood()
    print("nll at the truth %.6f, at the start %.6f, at the fit %.6f after %d evaluations: %r" % (at_truth, at_start, fit.nll, fit.n_evaluations, fit))
    assert fit.nll <= at_truth and fit.nll <= at_start
    assert fit.success and fit.n_evaluations > 10 and len(fit.variogram_parameters) == 3
    # (the list form carries the full sill: the partial sill comes back within a rounding, and the nll within the bar of kappa_2 <= 1e5)
    assert abs(fit.nll - lk.neg_log_likelihood(x, y, v, "exponential", fit.variogram_parameters, **fit.anisotropy)) <= n * lc.U * lc.KAPPA_MAX
    ok = pa.OrdinaryKriging(x, y, v, variogram_model=fit.variogram_model, variogram_parameters=fit.variogram_parameters, **fit.anisotropy)
    zz, ss = ok.execute("grid", np.linspace(0.5, 3.5, 5), np.linspace(0.5, 2.5, 4))
    assert zz.shape == (4, 5) and np.all(np.isfinite(zz)) and np.all(ss >= 0.0)
    # replicates of one variogram: the objective is the sum over the fields
    v2 = np.column_stack([v, 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)])
    fit2 = lk.fit_variogram_ml(x, y, v2, "exponential", start=truth, **anis)
    both = lk.neg_log_likelihood(x, y, v2, "exponential", truth, **anis)
    print("two replicates: nll at the truth %.6f, at the fit %.6f after %d evaluations" % (both.sum(), fit2.nll, fit2.n_evaluations))
    assert fit2.nll <= both.sum() and fit2.anisotropy == anis
