"""The fit libraries on the GPU held to the scaling laws of tests/_scaling_cases.py: ``likelihood.gram``, ``likelihood.gram_grad`` and
``VecchiaPlan.gram`` at three base problems (N = 65 gaussian 2-D, N = 129 spherical 3-D with its range inside the domain, N = 200
hole-effect at range 0.1) under factors 2^k, k = -20, -3, 7, 30, on psill and nugget (law 1), on the coordinates, dcoords and the range
(law 2) and on the columns (law 3) -- bit for bit, with no tolerance, wherever float64 keeps the law exactly; one case per library at the
magnitudes of projected coordinates held to the ordinary long-double bar; and ``neg_log_likelihood_grad`` in natural units under laws 1
and 2.

What is not bit for bit, and why (derived in tests/_scaling_cases.py, shown on the float64 restatements in
tests/test_fit_scaling_host.py): law 1 at the odd k = -3 and 7 -- sqrt(2 x) is not sqrt(2) sqrt(x), so the Cholesky factor of C times an
odd power of two is not the base factor times a constant; the float64 restatement's own G differs by about 2e-13 relative there.  Those
calls are held to the module's bar against the long-double reference scaled exactly.  A field's gradient under laws 1 and 3 is a sum of
two terms with different factors; a field of zeros isolates the trace term bit for bit and the rows are held to the prediction within
the roundings of the prediction.  Every figure is printed before it is asserted and appended to the file FIT_EDGES_PARITY_OUT names
(profiles/fit_edges_parity.txt), never by default."""
import functools
import math

import numpy as np
import pytest

from pykrige_amd import likelihood as lk
from tests import _grad_cases as gc
from tests import _lik_cases as lc
from tests import _scaling_cases as sc
from tests import _vecchia_cases as vcs

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAMES = sorted(sc.BASES)


@functools.lru_cache(maxsize=None)
def base_gram(name):
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    return lk.gram(X, case["model"], case["par"], W)


@functools.lru_cache(maxsize=None)
def base_gram_grad(name):
    case = sc.case_of(name)
    adj, dco, V, X = sc.grad_inputs(name)
    return lk.gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])


@pytest.mark.parametrize("law", sc.LAWS)
@pytest.mark.parametrize("name", NAMES)
def test_gram_keeps_the_law(name, law):
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    ref_logdet, ref_G, kappa, bar, _ = sc.dense_reference(name)
    worst = 0.0
    for k in sc.KS:
        Xs, par, Ws, _ = sc.apply_law(law, k, X, case["par"], W)
        worst = max(worst, sc.check_gram(name, law, k, base_gram(name), lk.gram(Xs, case["model"], par, Ws), ref_logdet, ref_G, bar))
    lc.record("scaling gram      %-8s law %d: exact at every exact k; worst err / bar at the odd k of law 1 %.3g" % (name, law, worst))


@pytest.mark.parametrize("law", sc.LAWS)
@pytest.mark.parametrize("name", NAMES)
def test_gram_grad_keeps_the_law(name, law):
    case = sc.case_of(name)
    adj, dco, V, X = sc.grad_inputs(name)
    F = V.shape[1]
    ref_logdet, ref_G, bar = sc.grad_gram_reference(name)
    logdet0, G0, grad0, info = base_gram_grad(name)
    assert info == 0 and np.all(G0[0] == 0.0)  # the field of zeros
    worst = 0.0
    for k in sc.KS:
        a, par, Ws, d = sc.apply_law(law, k, adj, case["par"], np.hstack([V, X]), dco)
        logdet1, G1, grad1, info = lk.gram_grad(a, d, case["model"], par, Ws[:, :F], Ws[:, F:], case["reml"])
        assert info == 0 and np.all(G1[0] == 0.0)
        worst = max(worst, sc.check_gram(name, law, k, (logdet0, G0[1:, 1:]), (logdet1, G1[1:, 1:]), ref_logdet, ref_G, bar))
        worst = max(worst, sc.check_grad(name, law, k, grad0, grad1, reference=sc.grad_reference(name)))
    lc.record("scaling gram_grad %-8s law %d: exact at every exact k; worst err / bar at the odd k of law 1 %.3g" % (name, law, worst))


@pytest.mark.parametrize("law", sc.LAWS)
@pytest.mark.parametrize("name", NAMES)
def test_vecchia_gram_keeps_the_law(name, law):
    from pykrige_amd import vecchia as vc

    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    worst = 0.0
    for m in case["vecchia_m"]:
        order, nbr, ref_logdet, ref_G, bar = sc.vecchia_reference(name, m)
        with vc.VecchiaPlan(X, m=m) as plan:
            assert np.array_equal(plan.neighbours, nbr)
            base = plan.gram(X, case["model"], case["par"], W)
            for k in sc.KS:
                Xs, par, Ws, _ = sc.apply_law(law, k, X, case["par"], W)
                on_base_plan = plan.gram(Xs, case["model"], par, Ws)  # the plan built on the base coordinates, called with the scaled ones
                worst = max(worst, sc.check_gram(name, law, k, base, on_base_plan, ref_logdet, ref_G, bar))
                if law == 2:
                    with vc.VecchiaPlan(Xs, m=m) as moved:
                        assert np.array_equal(moved.neighbours, nbr), (name, m, k)  # d2 times s^2 exactly: the same order and ties
                        own = moved.gram(Xs, case["model"], par, Ws)
                    assert own[0] == on_base_plan[0] and sc.same(own[1], on_base_plan[1])
    lc.record("scaling vecchia   %-8s law %d: exact at every exact k; worst err / bar at the odd k of law 1 %.3g" % (name, law, worst))


# ------------------------------------------------------------------------------------------------------------- the magnitudes
def test_the_magnitude_case_is_within_the_bar_through_gram_and_vecchia():
    """Coordinates 5e5 + 1e3 * unit, psill 2.5e3, nugget 1.5e2, range 4e2, columns of order 1e3 (kappa_2 about 1.2e3, asserted inside the
    cap on the CPU too): not powers of two, so the ordinary long-double bar."""
    from pykrige_amd import vecchia as vc

    name = "magnitude"
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    ref_logdet, ref_G, kappa, bar, _ = sc.dense_reference(name)
    assert kappa <= lc.KAPPA_MAX
    logdet, G = lk.gram(X, case["model"], case["par"], W)
    el, eg = lc.errors(logdet, G, ref_logdet, ref_G)
    lc.record("magnitude gram      N %d kappa_2 %9.4g bar %9.3g logdet error %9.3g G error %9.3g worst/bar %8.3g" % (case["n"], kappa, bar, el, eg, max(el, eg) / bar))
    assert el <= bar and eg <= bar and np.array_equal(G, G.T)
    m = case["vecchia_m"][0]
    order, nbr, v_logdet, v_G, _ = sc.vecchia_reference(name, m)
    with vc.VecchiaPlan(X, m=m) as plan:
        assert np.array_equal(plan.neighbours, nbr)
        logdet, G = plan.gram(X, case["model"], case["par"], W)
    el, eg = lc.errors(logdet, G, v_logdet, v_G)
    lc.record("magnitude vecchia   N %d m %d kappa_2 %9.4g bar %9.3g logdet error %9.3g G error %9.3g worst/bar %8.3g" % (case["n"], m, kappa, bar, el, eg, max(el, eg) / bar))
    assert el <= bar and eg <= bar and np.array_equal(G, G.T)


def test_the_magnitude_case_is_within_the_bar_through_gram_grad():
    name = "magnitude"
    case = sc.case_of(name)
    adj, dco, V, X = sc.grad_inputs(name)
    ref, piece_s, piece_t, kappa = sc.grad_reference(name)
    assert kappa <= lc.KAPPA_MAX
    logdet, G, grad, info = lk.gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])
    frac = np.abs(grad.astype(LD) - ref) / (case["n"] * lc.U * kappa * (piece_s[None, :] + piece_t))
    lc.record("magnitude gram_grad N %d kappa_2 %9.4g worst / bar per parameter: %s  worst/bar %8.3g"
              % (case["n"], kappa, " ".join("%8.2e" % float(t) for t in frac.max(axis=0)), float(frac.max())))
    assert info == 0 and np.all(frac <= 1.0)
    ref_logdet, ref_G, bar = sc.grad_gram_reference(name)
    el, eg = lc.errors(logdet, G[1:, 1:], ref_logdet, ref_G)
    assert el <= bar and eg <= bar


# ------------------------------------------------------------------------------------------------------------- the Python layer
def check_python_layer(reml, exact_calls=True, say=print):
    """``neg_log_likelihood_grad`` in natural units at N = 129 in the plane with anisotropy 1.7 at 25 degrees, three fields of which field
    0 is zeros, a constant trend (p = 1), under law 1 on the FULL sill and the nugget and law 2 on x, y and the range, with s = 2^7 (the
    issue's k) and s = 2^8 (its even neighbour, where law 1 is exact too).

    The objective is 1/2 [(N - p') log 2 pi - p'' + logdet + l_xx + Q_f] with p' = p'' = l_xx = 0 under ML and p' = p,
    p'' = log det(X^T X), l_xx = log det G_xx under REML.  Law 1: logdet moves by N k ln 2, G by 1 / s, so l_xx moves by -p k ln 2 and Q_f
    becomes Q_f / s.  For the field of zeros Q = 0: its nll moves by 1/2 N k ln 2 (ML) or 1/2 (N - p) k ln 2 (REML), which is asserted; a
    field with values also has its Q_f divided by s, so its nll is held to ``nll_from_gram`` of the base pieces moved exactly.  Law 2
    with a constant trend changes no bit of C, X or W: nll is unchanged bit for bit under ML and REML alike.  (With a regional-linear
    trend X^T X and G_xx both become D . D, D = diag(1, s, s), and the two log determinants cancel only to rounding: the constant trend is
    used.)  The gradient columns move as tests/_scaling_cases.py derives; the two angle columns stay per degree: factor 1 under law 2.
    A wrong chain-rule factor is off by a factor, not by an ulp.  At k = 7 law 1 is held to the bars (the square roots), at k = 8 to the
    few roundings of the prediction."""
    from tests.test_likelihood import _reference_nll

    n, model, full = 129, "exponential", [1.2, 0.9, 0.1]
    anis, scal, ang = dict(anisotropy_scaling=1.7, anisotropy_angle=25.0), [1.7], [25.0]
    rng = np.random.default_rng(13)
    raw = rng.random((n, 2)) * [3.0, 2.0]
    v = np.sin(2.0 * raw[:, 0])[:, None] + 0.5 * raw[:, 1][:, None] + 0.4 * rng.standard_normal((n, 2))
    V = np.hstack([np.zeros((n, 1)), v])
    x, y = raw.T
    p = 1
    close = sc.same if exact_calls else (lambda a, b: sc.ulps(a, b) <= 8)
    nll0, g0 = lk.neg_log_likelihood_grad(x, y, V, model, full, reml=reml, **anis)
    assert nll0.shape == (3,) and g0.shape == (3, 5) and np.all(np.isfinite(g0))
    adj = gc.adjusted(raw, scal, ang)
    par = [full[0] - full[2], full[1], full[2]]
    X = np.ones((n, 1))
    dco = lk.anisotropy_derivatives(raw, scal, ang)
    ref, scale, kappa = gc.gradient_ld(adj, dco, model, par, V, X, reml)
    assert kappa <= lc.KAPPA_MAX
    reference = (ref, scale[0].copy(), scale - scale[0][None, :], kappa)
    _, tol_ref = _reference_nll(raw, v, model, full, scal, ang, None, reml)  # what the bar of the pieces allows the nll of a field
    logdet0, G0 = lk.gram(adj, model, par, np.hstack([V, X]))
    for k in (7, 8):
        s = 2.0 ** k
        # law 2: x, y and the range
        nll2, g2 = lk.neg_log_likelihood_grad(x * s, y * s, V, model, [full[0], full[1] * s, full[2]], reml=reml, **anis)
        say("python layer reml %s k %d law 2: nll differs by %.3g ulp" % (reml, k, sc.ulps(nll2, nll0)))
        assert close(nll2, nll0)
        sc.check_grad("python", 2, k, g0, g2, exact_calls=exact_calls, say=say, n=n)
        # law 1: the full sill and the nugget
        nll1, g1 = lk.neg_log_likelihood_grad(x, y, V, model, [full[0] * s, full[1], full[2] * s], reml=reml, **anis)
        want = lk.nll_from_gram(n, logdet0 + n * k * math.log(2.0), G0 / s, 3, reml, lk._pieces(X))
        margin = 0.5 * 4 * n * lc.U * max(1.0, abs(logdet0), abs(logdet0 + n * k * math.log(2.0))) + 16 * lc.U * np.abs(want)
        if k % 2:
            margin = margin + 2.0 * float(np.max(tol_ref))  # two device results, each within what its bar allows
        shift = 0.5 * (n - (p if reml else 0)) * k * math.log(2.0)
        say("python layer reml %s k %d law 1: |nll' - prediction| %s margin %s; field of zeros moved by %.15g, 1/2 (N - p') k ln 2 = %.15g"
            % (reml, k, np.abs(nll1 - want), margin, nll1[0] - nll0[0], shift))
        assert np.all(np.abs(nll1 - want) <= margin)
        assert abs((nll1[0] - nll0[0]) - shift) <= margin[0] + 16 * lc.U * abs(nll0[0])
        sc.check_grad("python", 1, k, g0, g1, exact_calls=exact_calls, say=say, reference=reference, n=n)


@pytest.mark.parametrize("reml", [False, True])
def test_neg_log_likelihood_grad_in_natural_units_keeps_the_laws(reml):
    check_python_layer(reml, say=lc.record)
