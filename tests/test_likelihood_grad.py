"""likelihood.gram_grad / neg_log_likelihood_grad / fit_variogram_ml(method='l-bfgs-b') on the GPU against the long-double reference of
tests/_grad_cases.py.

The bar (derived there): entry (f, k) of the gradient within N 2^-52 kappa_2(C) (1/2 |P|_F |D_k|_F + |a_f|^2 |D_k|_F) of the reference.
The cases sit at the edges of the 64-column blocks (N = 2, 63, 64, 65, 129), of the rule that identity row i joins the elimination at
block column i / 64 (N = 129, 200, 333: two to six block columns), of the 64 x 64 pair tiles of k_grad_pairs (N = 128, 192 | 193,
256 | 257) and of the eight-field chunks (F = 1, 7, 8, 9, 32), in 2-D and 3-D,
each model, ML and REML, one coincident pair with a nugget, exact zeros beyond a spherical range, and the three inputs of
tests/_lik_cases.py that are not positive definite.  logdet, G and nll are held to ``gram`` / ``neg_log_likelihood`` bit for bit.
Every figure is printed before it is asserted; profiles/likelihood_grad_parity.txt holds them."""
import ctypes
import functools
import math

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import likelihood as lk
from tests import _grad_cases as gc
from tests import _lik_cases as lc

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@functools.lru_cache(maxsize=None)
def device(name):
    """(logdet, G, grad, info) of CASES[name] from the device, once; do not write into it."""
    case = gc.CASES[name]
    adj, dco, V, X = gc.problem(case)
    return lk.gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_the_gradient_is_within_its_bar_and_the_pieces_are_grams_bit_for_bit(name):
    case = gc.CASES[name]
    ref, bar, kappa = gc.reference(name)
    adj, dco, V, X = gc.problem(case)
    logdet, G, grad, info = device(name)
    ng = 2 if case["ndim"] == 2 else 5
    assert info == 0 and grad.shape == (case["F"], 3 + ng) and np.all(np.isfinite(grad))
    frac = np.abs(grad.astype(gc.LD) - ref) / bar
    (lc.record if name in gc.EDGES else print)("gram_grad %-18s N %3d F %2d p %d %s kappa_2 %8.3g  worst / bar per parameter: %s  max |grad| %.3g  worst/bar %8.3g"
                                               % (name, case["n"], case["F"], X.shape[1], "REML" if case["reml"] else "ML  ", kappa,
                                                  " ".join("%8.2e" % float(t) for t in frac.max(axis=0)), float(np.abs(grad).max()), float(frac.max())))
    assert np.all(frac <= 1.0), (name, float(frac.max()))
    # logdet and G are mlk_gram's bits
    logdet4, G4 = lk.gram(adj, case["model"], case["par"], np.hstack([V, X]))
    assert logdet == logdet4 and np.array_equal(bits(G), bits(G4)) and np.array_equal(G, G.T)
    # two calls return the same bits
    again = lk.gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])
    assert again[0] == logdet and np.array_equal(bits(again[1]), bits(G)) and np.array_equal(bits(again[2]), bits(grad))
    # field f of the (N, F) call is the one-field call
    for f in sorted({0, case["F"] // 2, case["F"] - 1}):
        one = lk.gram_grad(adj, dco, case["model"], case["par"], V[:, [f]], X, case["reml"])
        assert one[0] == logdet and np.array_equal(bits(one[2][0]), bits(grad[f])), (name, f)
        assert one[1][0, 0] == G[f, f]


def test_fewer_geometry_parameters_leave_the_others_alone():
    """ng = 0 and ng = 1 of the C call: the first three derivatives do not depend on the geometry sets beside them."""
    name = "n65_gau_f9_p3"
    case = gc.CASES[name]
    adj, dco, V, X = gc.problem(case)
    logdet, G, grad, _ = device(name)
    for keep in (0, 1):
        got = lk.gram_grad(adj, dco[:keep], case["model"], case["par"], V, X, case["reml"])
        assert got[2].shape == (case["F"], 3 + keep) and np.array_equal(bits(got[2]), bits(grad[:, :3 + keep]))


def test_forty_one_columns_are_refused_and_harm_nothing():
    """F + p = 40 is a case (n129_exp3d_f32_p8); F + p = 41 is refused by ``gram_grad`` with a ValueError on either side -- 33 fields, or
    9 trend columns -- and the valid call that follows returns the bits it returned before."""
    good = "n129_exp3d_f32_p8"
    case = gc.CASES[good]
    adj, dco, V, X = gc.problem(case)
    first = device(good)
    with pytest.raises(ValueError, match="MLG_MAXFIELDS"):
        lk.gram_grad(adj, dco, case["model"], case["par"], np.hstack([V, V[:, :1]]), X, case["reml"])
    with pytest.raises(ValueError, match="MLG_MAXTREND"):
        lk.gram_grad(adj, dco, case["model"], case["par"], V, np.hstack([X, V[:, :1]]), case["reml"])
    again = lk.gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])
    assert again[0] == first[0] and np.array_equal(bits(again[1]), bits(first[1])) and np.array_equal(bits(again[2]), bits(first[2]))


def _problem(n, ndim, seed, nf=1):
    rng = np.random.default_rng(seed)
    raw = rng.random((n, ndim)) * ([3.0, 2.0, 1.0][:ndim])
    v = np.sin(2.0 * raw[:, 0])[:, None] + 0.5 * raw[:, 1][:, None] + 0.4 * rng.standard_normal((n, nf))
    return raw, v


@pytest.mark.parametrize("ndim,drift", [(2, "array"), (3, "regional_linear")])
def test_nll_is_neg_log_likelihoods_bit_for_bit_and_the_gradient_is_in_natural_units(ndim, drift):
    raw, v = _problem(129, ndim, 11 + ndim, nf=3)
    full = [1.2, 0.9, 0.1]
    anis = dict(anisotropy_scaling=1.7, anisotropy_angle=25.0) if ndim == 2 else dict(
        anisotropy_scaling_y=1.4, anisotropy_scaling_z=0.6, anisotropy_angle_x=10.0, anisotropy_angle_y=-20.0, anisotropy_angle_z=35.0)
    sc, an = list(anis.values())[:ndim - 1], list(anis.values())[ndim - 1:]
    names = lk.GRAD_NAMES_2D if ndim == 2 else lk.GRAD_NAMES_3D
    if drift == "array":
        drift = np.column_stack([raw[:, 0], raw[:, 0] * raw[:, 1]])
    for reml in (False, True):
        nll, grad = lk.neg_log_likelihood_grad(*raw.T, v, "exponential", full, drift=drift, reml=reml, **anis)
        want = lk.neg_log_likelihood(*raw.T, v, "exponential", full, drift=drift, reml=reml, **anis)
        assert nll.shape == (3,) and grad.shape == (3, len(names)) and np.array_equal(bits(nll), bits(want))
        for f in range(3):
            one, g1 = lk.neg_log_likelihood_grad(*raw.T, v[:, f], "exponential", full, drift=drift, reml=reml, **anis)
            assert isinstance(one, float) and one == nll[f] and g1.shape == (len(names),) and np.array_equal(bits(g1), bits(grad[f]))
        # the long-double gradient of the same problem (the trend held, as the docstring says), and its bar
        adj = gc.adjusted(raw, sc, an)
        X = gc.trend(adj, drift)
        par = [full[0] - full[2], full[1], full[2]]
        ref, scale, kappa = gc.gradient_ld(adj, lk.anisotropy_derivatives(raw, sc, an), "exponential", par, v, X, reml)
        assert kappa <= gc.KAPPA_MAX
        frac = np.abs(grad.astype(gc.LD) - ref) / (len(raw) * gc.U * kappa * scale)
        print("ndim %d reml %s: worst / bar %s" % (ndim, reml, dict(zip(names, ["%.2e" % float(t) for t in frac.max(axis=0)]))))
        assert np.all(frac <= 1.0)


@pytest.mark.parametrize("name", sorted(lc.NOT_PD))
def test_a_matrix_that_is_not_positive_definite_is_answered_and_harms_nothing(name):
    case, column = lc.NOT_PD[name]
    X, W = lc.inputs(case)
    V, T = W[:, :1], np.ones((case["n"], 1))
    dco = lk.anisotropy_derivatives(X, [1.0], [0.0])
    logdet, G, grad, info = lk.gram_grad(X, dco, case["model"], case["par"], V, T, True)
    print("%s: info %d (reference: column %d)" % (name, info, column))
    assert logdet == math.inf and G.shape == (2, 2) and np.all(np.isnan(G)) and grad.shape == (1, 5) and np.all(np.isnan(grad))
    assert info == column
    lib = lk.load_grad()
    p = lambda a: a.ctypes.data_as(lk._dp)
    ct, et, vt, tt = (np.ascontiguousarray(a) for a in (X.T, dco.transpose(0, 2, 1), V.T, T.T))
    outG, outg, ld, inf_ = np.full((2, 2), 7.0), np.full((1, 5), 7.0), ctypes.c_double(7.0), ctypes.c_int32(-5)
    rc = lib.mlg_grad(0, case["n"], 2, p(ct), 2, p(et), lk.MODEL_IDS[case["model"]], *case["par"], p(vt), 1, p(tt), 1, 1, ctypes.byref(ld),
                      p(outG), p(outg), ctypes.byref(inf_))
    assert rc == lk.MLG_ENOTPD and inf_.value == column and b"not positive definite" in lib.mlg_last_error()
    assert ld.value == 7.0 and np.all(outG == 7.0) and np.all(outg == 7.0)  # never a partial result
    full = [case["par"][0] + case["par"][2], case["par"][1], case["par"][2]]
    nll, g = lk.neg_log_likelihood_grad(*X.T, V[:, 0], case["model"], full)
    assert nll == math.inf and g.shape == (5,) and np.all(np.isnan(g))
    # a following valid call is unaffected
    good = "n64_exp_f8"
    first = device(good)
    adj, dc2, V2, X2 = gc.problem(gc.CASES[good])
    again = lk.gram_grad(adj, dc2, gc.CASES[good]["model"], gc.CASES[good]["par"], V2, X2, gc.CASES[good]["reml"])
    assert again[0] == first[0] and np.array_equal(bits(again[2]), bits(first[2]))


def test_the_methods_are_the_module_functions_on_the_objects_stations():
    raw, v = _problem(129, 3, 21)
    v = v[:, 0]
    x, y, z = raw.T
    kw = dict(variogram_model="gaussian", variogram_parameters=[1.0, 1.5, 0.2])
    a2, a3 = dict(anisotropy_scaling=2.0, anisotropy_angle=40.0), dict(anisotropy_scaling_y=1.5, anisotropy_scaling_z=0.5, anisotropy_angle_x=15.0)

    def same(a, b):
        return a[0] == b[0] and np.array_equal(bits(a[1]), bits(b[1]))

    ok = pa.OrdinaryKriging(x, y, v, **kw, **a2)
    got = ok.neg_log_likelihood_grad()
    assert same(got, lk.neg_log_likelihood_grad(x, y, v, "gaussian", [1.0, 1.5, 0.2], **a2)) and got[0] == ok.neg_log_likelihood()
    assert same(ok.neg_log_likelihood_grad(reml=False, anisotropy_angle=10.0), lk.neg_log_likelihood_grad(
        x, y, v, "gaussian", [1.0, 1.5, 0.2], reml=False, anisotropy_scaling=2.0, anisotropy_angle=10.0))
    assert same(ok.neg_log_likelihood_grad([0.8, 1.0, 0.1]), lk.neg_log_likelihood_grad(x, y, v, "gaussian", [0.8, 1.0, 0.1], **a2))
    uk = pa.UniversalKriging(x, y, v, drift_terms=["regional_linear"], **kw, **a2)
    assert same(uk.neg_log_likelihood_grad(), lk.neg_log_likelihood_grad(x, y, v, "gaussian", [1.0, 1.5, 0.2], drift="regional_linear", **a2))
    assert uk.neg_log_likelihood_grad()[0] == uk.neg_log_likelihood()
    ok3 = pa.OrdinaryKriging3D(x, y, z, v, **kw, **a3)
    assert same(ok3.neg_log_likelihood_grad(), lk.neg_log_likelihood_grad(x, y, z, v, "gaussian", [1.0, 1.5, 0.2], **a3))
    uk3 = pa.UniversalKriging3D(x, y, z, v, drift_terms=["regional_linear"], **kw, **a3)
    got = uk3.neg_log_likelihood_grad()
    assert same(got, lk.neg_log_likelihood_grad(x, y, z, v, "gaussian", [1.0, 1.5, 0.2], drift="regional_linear", **a3))
    assert got[1].shape == (8,) and got[0] == uk3.neg_log_likelihood()
    fit = ok3.fit_variogram_ml(method="l-bfgs-b")
    print(fit, fit.message)
    assert fit.nll <= ok3.neg_log_likelihood() and set(fit.anisotropy) == set(lk._ANIS3) and fit.anisotropy["anisotropy_scaling_y"] == 1.5


def test_the_quasi_newton_fit_reaches_the_simplex_fit_in_fewer_evaluations():
    """N = 150, exponential, one field, fit_anisotropy=True, both methods from the same start: the default one, the least-squares fit of
    the binned variogram (the likelihood of a variogram with anisotropy has more than one local minimum; neither search is global, so
    the start is the one a user gets without asking).  Nelder-Mead stops at 1e-6 in the
    objective and 1e-3 in the parameters, so its own answer is only that good: l-bfgs-b must end with nll <= Nelder-Mead's + 1e-4, in
    fewer device calls."""
    rng = np.random.default_rng(2025)
    n = 150
    raw = rng.random((n, 2)) * [4.0, 3.0]
    adj = gc.adjusted(raw, [2.0], [30.0])
    Cm = lc.covariance_ld(adj, "exponential", [0.95, 1.2, 0.05]).astype(np.float64)
    v = 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)
    x, y = raw.T
    nm = lk.fit_variogram_ml(x, y, v, "exponential", fit_anisotropy=True)
    qn = lk.fit_variogram_ml(x, y, v, "exponential", fit_anisotropy=True, method="l-bfgs-b")
    at_start = pa.OrdinaryKriging(x, y, v, variogram_model="exponential").neg_log_likelihood()
    print("start %.6f\nnelder-mead %.6f after %d evaluations: %r\nl-bfgs-b    %.6f after %d evaluations: %r (%s)"
          % (at_start, nm.nll, nm.n_evaluations, nm, qn.nll, qn.n_evaluations, qn, qn.message))
    assert qn.nll <= at_start and nm.nll <= at_start
    assert qn.nll <= nm.nll + 1e-4
    assert qn.n_evaluations < nm.n_evaluations
    assert abs(qn.nll - lk.neg_log_likelihood(x, y, v, "exponential", qn.variogram_parameters, **qn.anisotropy)) <= n * lc.U * lc.KAPPA_MAX
