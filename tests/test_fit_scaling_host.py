"""The scaling laws of tests/_scaling_cases.py without a GPU: they belong to the arithmetic, not to the device.  Each exact law is asserted
on the float64 NumPy restatements the project already has -- ``_lik_cases.blocked_float64``, ``_vecchia_cases.float64_gram`` behind
``StandInPlan``, ``_grad_cases.standin_gram_grad`` -- the logdet margin on the long-double references, and the inputs are shown to stay
far from overflow and from the subnormals (k = 30 on the cube of a spherical range, k = -20 on a psill).  Every base problem and the
magnitude case keep kappa_2 <= 1e5.  The Python layer's chain to natural units is run on the stand-ins."""
import numpy as np
import pytest

from pykrige_amd import likelihood as lk
from tests import _grad_cases as gc
from tests import _lik_cases as lc
from tests import _scaling_cases as sc
from tests import _vecchia_cases as vcs

LD = np.longdouble


@pytest.mark.parametrize("name", sorted(sc.BASES) + ["magnitude"])
def test_every_problem_keeps_its_condition_and_stays_inside_the_exponent_range(name):
    case = sc.case_of(name)
    logdet, G, kappa, bar, cmin = sc.dense_reference(name)
    print("%s: kappa_2 %.4g bar %.3g min nonzero |C_ij| %.3g" % (name, kappa, bar, cmin))
    assert logdet is not None and kappa <= lc.KAPPA_MAX
    grad, piece_s, piece_t, kappa_g = sc.grad_reference(name)
    print("%s (the gradient's adjusted coordinates): kappa_2 %.4g" % (name, kappa_g))
    assert kappa_g <= lc.KAPPA_MAX and np.all(np.isfinite(grad.astype(np.float64))) and np.all(piece_s > 0)
    if name == "magnitude":
        return
    X, W = sc.gram_inputs(name)
    if case["model"] == "spherical":
        assert np.count_nonzero(lc.covariance_ld(X, case["model"], case["par"]) == 0) > 0  # the range is inside the domain
    for k in sc.KS:  # the scaled matrices themselves: every nonzero entry far from the subnormals, everything finite
        for law in (1, 2):
            Xs, par, _, _ = sc.apply_law(law, k, X, case["par"], W)
            Cm = lc.covariance_ld(Xs, case["model"], par).astype(np.float64)
            assert np.all(np.isfinite(Cm)) and np.min(np.abs(Cm[Cm != 0])) > 1e-290, (name, law, k)
            if law == 1:
                assert sc.same(Cm / 2.0 ** k, lc.covariance_ld(X, case["model"], case["par"]).astype(np.float64))  # C times s exactly
            else:
                assert sc.same(Cm, lc.covariance_ld(X, case["model"], case["par"]).astype(np.float64))  # every bit of C
        r = case["par"][1] * 2.0 ** k
        assert 1e-290 < r * r * r * r < 1e290  # range^3 of the covariance, range^4 of its derivative


@pytest.mark.parametrize("law", sc.LAWS)
@pytest.mark.parametrize("name", sorted(sc.BASES))
def test_the_blocked_float64_restatement_keeps_the_laws(name, law):
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    ref_logdet, ref_G, _, bar, _ = sc.dense_reference(name)
    base = lc.blocked_float64(X, case["model"], case["par"], W)
    for k in sc.KS:
        Xs, par, Ws, _ = sc.apply_law(law, k, X, case["par"], W)
        sc.check_gram(name, law, k, base, lc.blocked_float64(Xs, case["model"], par, Ws), ref_logdet, ref_G, bar)


def test_an_odd_power_of_two_on_the_sill_is_not_exact_in_float64_either():
    """The reason law 1 falls back to the bar at k = -3 and 7: the restatement's own G times s differs from the base G there, by about
    2e-13 relative on gau65, and is exact at the even k."""
    case = sc.case_of("gau65")
    X, W = sc.gram_inputs("gau65")
    _, G0 = lc.blocked_float64(X, case["model"], case["par"], W)
    for k in sc.KS:
        _, par, _, _ = sc.apply_law(1, k, X, case["par"], W)
        _, G1 = lc.blocked_float64(X, case["model"], par, W)
        print("k %3d: G' * s differs from G by %.3g ulp" % (k, sc.ulps(G1 * 2.0 ** k, G0)))
        assert sc.same(G1 * 2.0 ** k, G0) == (k % 2 == 0)


@pytest.mark.parametrize("law", sc.LAWS)
@pytest.mark.parametrize("name", sorted(sc.BASES))
def test_the_float64_vecchia_restatement_keeps_the_laws(name, law):
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    for m in case["vecchia_m"]:
        order, nbr, ref_logdet, ref_G, bar = sc.vecchia_reference(name, m)
        plan = vcs.StandInPlan(X, m=m)
        assert np.array_equal(plan.neighbours, nbr)
        base = plan.gram(X, case["model"], case["par"], W)
        for k in sc.KS:
            Xs, par, Ws, _ = sc.apply_law(law, k, X, case["par"], W)
            sc.check_gram(name, law, k, base, plan.gram(Xs, case["model"], par, Ws), ref_logdet, ref_G, bar)  # the base plan, moved inputs
            if law == 2:
                assert np.array_equal(vcs.StandInPlan(Xs, m=m).neighbours, nbr)  # d2 times s^2 exactly: the same order, the same ties


@pytest.mark.parametrize("law", sc.LAWS)
@pytest.mark.parametrize("name", sorted(sc.BASES))
def test_the_float64_gradient_stand_in_keeps_the_laws(name, law):
    """``standin_gram_grad`` goes through ``np.linalg.cholesky``, ``inv`` and ``solve`` and through matrix products whose order of
    summation the BLAS may choose by size and alignment: they are not order-stable, so this restatement is held to 8 units in the last
    place where the device is held to the bit (and to the same bar at the odd k of law 1)."""
    case = sc.case_of(name)
    adj, dco, V, X = sc.grad_inputs(name)
    reference = sc.grad_reference(name)
    base = gc.standin_gram_grad(adj, dco, case["model"], case["par"], V, X, case["reml"])
    assert base[3] == 0
    for k in sc.KS:
        a, par, Ws, d = sc.apply_law(law, k, adj, case["par"], np.hstack([V, X]), dco)
        got = gc.standin_gram_grad(a, d, case["model"], par, Ws[:, :V.shape[1]], Ws[:, V.shape[1]:], case["reml"])
        assert got[3] == 0
        sc.check_grad(name, law, k, base[2], got[2], exact_calls=False, reference=reference)


@pytest.mark.parametrize("name", sorted(sc.BASES))
def test_the_long_double_logdet_moves_by_n_k_ln_2_within_the_margin(name):
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    ref_logdet, ref_G, _, _, _ = sc.dense_reference(name)
    n = case["n"]
    for k in sc.KS:
        _, par, _, _ = sc.apply_law(1, k, X, case["par"], W)
        logdet, G = lc.brute_force(X, case["model"], par, W[:, :1])
        d = float(abs(logdet - (ref_logdet + LD(n * k) * np.log(LD(2)))))
        margin = 4 * n * lc.U * max(1.0, abs(float(ref_logdet)), abs(float(logdet)))
        print("%s k %3d: long-double |logdet' - logdet - N k ln 2| %.3g, the float64 margin %.3g" % (name, k, d, margin))
        assert d <= margin / 1024  # (eleven more bits than float64)
        assert abs(float(G[0, 0] * LD(2.0 ** k) - ref_G[0, 0])) <= 1e-15 * n * abs(float(ref_G[0, 0]))


def test_the_magnitude_case_is_within_the_bar_on_the_restatements():
    """Coordinates 5e5 + 1e3 * unit, psill 2.5e3, nugget 1.5e2, range 4e2, columns of order 1e3: kappa_2 is printed (about 1.2e3) and is
    inside the cap; the three float64 restatements are inside the ordinary long-double bars."""
    name = "magnitude"
    case = sc.case_of(name)
    X, W = sc.gram_inputs(name)
    ref_logdet, ref_G, kappa, bar, _ = sc.dense_reference(name)
    assert kappa <= lc.KAPPA_MAX
    el, eg = lc.errors(*lc.blocked_float64(X, case["model"], case["par"], W), ref_logdet, ref_G)
    print("magnitude: kappa_2 %.4g bar %.3g; blocked float64 logdet error %.3g G error %.3g" % (kappa, bar, el, eg))
    assert el <= bar and eg <= bar
    order, nbr, v_logdet, v_G, _ = sc.vecchia_reference(name, case["vecchia_m"][0])
    el, eg = lc.errors(*vcs.float64_gram(X, order, nbr, case["model"], case["par"], W), v_logdet, v_G)
    print("magnitude: float64 vecchia logdet error %.3g G error %.3g" % (el, eg))
    assert el <= bar and eg <= bar
    adj, dco, V, Xt = sc.grad_inputs(name)
    ref, piece_s, piece_t, kappa_g = sc.grad_reference(name)
    g = gc.standin_gram_grad(adj, dco, case["model"], case["par"], V, Xt, case["reml"])[2]
    frac = np.abs(g.astype(LD) - ref) / (case["n"] * lc.U * kappa_g * (piece_s[None, :] + piece_t))
    print("magnitude: float64 gradient stand-in worst / bar %.3g (kappa_2 %.4g)" % (float(frac.max()), kappa_g))
    assert kappa_g <= lc.KAPPA_MAX and np.all(frac <= 1.0)


# ------------------------------------------------------------------------------------------------------------- the Python layer
@pytest.fixture
def stand_in(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a library was loaded")

    monkeypatch.setattr(lk, "load", boom)
    monkeypatch.setattr(lk, "load_grad", boom)
    monkeypatch.setattr(lk, "gram", gc.standin_gram)
    monkeypatch.setattr(lk, "gram_grad", gc.standin_gram_grad)


@pytest.mark.parametrize("reml", [False, True])
def test_neg_log_likelihood_grad_in_natural_units_keeps_the_laws_on_the_stand_in(stand_in, reml):
    from tests.test_fit_scaling import check_python_layer

    check_python_layer(reml, exact_calls=False)
