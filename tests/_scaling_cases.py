"""What tests/test_fit_scaling_host.py (CPU) and tests/test_fit_scaling.py (GPU) share: three base problems of the fit libraries, the
three scaling laws that float64 keeps exactly, and the checks that hold ``likelihood.gram``, ``likelihood.gram_grad`` and
``VecchiaPlan.gram`` -- or their float64 NumPy restatements -- to them.

A factor s = 2^k changes the exponent of a float64 and nothing else, as long as nothing overflows or turns subnormal.  So with s = 2^k:

 law 1  psill, nugget times s.  Every entry of C is times s exactly.  In exact arithmetic logdet moves by N k ln 2 and G = W^T C^-1 W is
        divided by s.  The elimination keeps that to the bit only where its square roots do: sqrt(4^j x) = 2^j sqrt(x) is exact, but
        sqrt(2 x) is not sqrt(2) sqrt(x) rounded, so a factor of C times an ODD power of two is not the base factor times a constant and
        every later rounding differs.  That is a rounding of the method, not of the device -- the float64 restatements show the same
        (tests/test_fit_scaling_host.py: at k = -3 and 7 the entries of G differ from the scaled base by about 2e-13 relative).  So for
        even k (-20, 30) ``G' * s`` must hold the bits of G, and for odd k (-3, 7) the scaled call is held to the module's bar against the
        long-double reference scaled exactly.  logdet is a sum of N logarithms each shifted by k ln 2: within 4 N 2^-52 max(1, |logdet|),
        |logdet| the larger of the base's and the scaled call's (the sum that is rounded is the scaled one).
 law 2  coordinates, dcoords and range times s.  Every d / range keeps its bits, hence every bit of C, logdet and G.
 law 3  W (V and X together) times s.  C is untouched; every product with a column of W is times s exactly: ``G' / s^2`` holds the bits
        of G and logdet is unchanged.

The gradient of include/mikgrad.h is grad[f][k] = 1/2 S_k - 1/2 T_kf with S_k = sum M D_k (the trace term) and T_kf = a_f^T D_k a_f (the
quadratic term), M = P or Q, a_f = P v_f.  P and Q go as 1 / s under law 1 and are unchanged under laws 2 and 3; a_f goes as 1 / s under
law 1 and as s under law 3; D_psill and D_nugget never move, D_range goes as s under law 1 (c_r has the factor psill) and as 1 / s under
law 2 (a derivative by a length), a geometry D goes as s under law 1 and is unchanged under law 2 (c_g as 1 / s^2, w_g as s^2).  The two
terms therefore scale by

            trace term S_k                         quadratic term T_kf
 law 1      psill, nugget 1/s; range, geometry 1   psill, nugget 1/s^2; range, geometry 1/s
 law 2      range 1/s; the others 1                range 1/s; the others 1
 law 3      1                                      s^2

Under law 1 a field y is not scaled, so the two terms of its gradient move by different factors: the columns are NOT the base columns
times one factor (that would need V times sqrt(s)).  Every problem here carries a field of zeros as field 0: its a_f is 0, its T is 0 and
its row is 1/2 S_k to the bit, which separates the terms.  Row 0 is held to its factor bit for bit; where a row's two factors agree (law 2)
every row is; otherwise row f is held to 1/2 S_k alpha_k - (1/2 S_k - grad[f][k]) beta_k within the few roundings of that expression.
"""
import functools

import numpy as np

from tests import _grad_cases as gc
from tests import _lik_cases as lc
from tests import _vecchia_cases as vcs

LD = np.longdouble
U = lc.U
KS = (-20, -3, 7, 30)
LAWS = (1, 2, 3)

# name -> the problem in the form of _lik_cases (m columns of W) and of _grad_cases (F fields, p trend columns, reml, anisotropy), and
# the neighbour bounds of the Vecchia plans.  gau65 is _lik_cases' n65_gau_m17 / _grad_cases' n65_gau_f9_p3; hole200 is _grad_cases'
# n200_hole_f1 (its adjusted coordinates serve all three libraries); sph129 is new: 129 stations in the unit cube with range 0.4, inside the domain, so C holds exact zeros.
BASES = {
    "gau65": dict(n=65, ndim=2, model="gaussian", par=[1.0, 0.2, 0.05], m=17, F=9, p=3, reml=True, vecchia_m=(10, 64), **gc.A2),
    "sph129": dict(n=129, ndim=3, model="spherical", par=[1.0, 0.4, 0.1], m=7, F=2, p=2, reml=True, vecchia_m=(10,), **gc.A3),
    "hole200": dict(n=200, ndim=2, model="hole-effect", par=[1.0, 0.1, 0.1], m=3, F=1, p=1, reml=True, vecchia_m=(10,), **gc.A2),
}
# one problem at the magnitudes of projected coordinates and of values of order 1e3, held to the ordinary bar: 5e5 is no power of two
MAGNITUDE = dict(n=129, ndim=2, model="exponential", par=[2.5e3, 4e2, 1.5e2], m=7, F=3, p=2, reml=True, vecchia_m=(10,), **gc.A2)


def case_of(name):
    return MAGNITUDE if name == "magnitude" else BASES[name]


def gram_inputs(name):
    """(coords, W) for ``likelihood.gram`` and ``VecchiaPlan.gram``: ``_lik_cases.inputs``; the magnitude case moved to
    5e5 + 1e3 * unit with columns of order 1e3."""
    X, W = lc.inputs(case_of(name))
    if name == "hole200":  # (hole-effect is positive definite at the stations of _grad_cases' n200_hole_f1, not at any 200 in the square)
        X = grad_inputs(name)[0]
    return (5e5 + 1e3 * X, 1e3 * W) if name == "magnitude" else (X, W)


def grad_inputs(name):
    """(adjusted coordinates, dcoords, V, X) for ``likelihood.gram_grad``: ``_grad_cases.problem`` with a field of zeros put first."""
    case = case_of(name)
    raw, V, drift = gc.inputs(case)
    if name == "magnitude":
        raw, V, drift = 5e5 + 1e3 * raw, 1e3 * V, (None if drift is None else 1e3 * drift)
    adj = gc.adjusted(raw, case["scaling"], case["angle"])
    V = np.hstack([np.zeros((case["n"], 1)), V])
    return adj, gc.lk.anisotropy_derivatives(raw, case["scaling"], case["angle"]), V, gc.trend(adj, drift)


def apply_law(law, k, coords, par, W, dcoords=None):
    """The inputs after the law: (coords, par, W, dcoords)."""
    s = 2.0 ** k
    if law == 1:
        return coords, [par[0] * s, par[1], par[2] * s], W, dcoords
    if law == 2:
        return coords * s, [par[0], par[1] * s, par[2]], W, (None if dcoords is None else dcoords * s)
    return coords, list(par), W * s, dcoords


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


def ulps(a, b):
    """max |a - b| in units of 2^-52 max(|a|, |b|), 0 where both are 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    big = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(big > 0, np.abs(a - b) / np.where(big > 0, big, 1.0), 0.0)) / U)


def exact_here(law, k):
    """Whether the law holds to the bit through an elimination with square roots: always, but for law 1 with an odd k."""
    return law != 1 or k % 2 == 0


# ------------------------------------------------------------------------------------------------------------- the references
@functools.lru_cache(maxsize=None)
def dense_reference(name):
    """(logdet, G, kappa_2, bar, min |C_ij| over the nonzero entries) of the dense problem in long double; do not write into it."""
    case = case_of(name)
    X, W = gram_inputs(name)
    logdet, G = lc.brute_force(X, case["model"], case["par"], W)
    Cm = lc.covariance_ld(X, case["model"], case["par"]).astype(np.float64)
    kappa = float(np.linalg.cond(Cm, 2))
    return logdet, G, kappa, case["n"] * U * kappa, float(np.min(np.abs(Cm[Cm != 0])))


@functools.lru_cache(maxsize=None)
def vecchia_reference(name, m):
    """(order, neighbours, logdet, G, bar) of the Vecchia problem in long double; the bar is the dense problem's."""
    case = case_of(name)
    X, W = gram_inputs(name)
    order = vcs.order_of(case["n"])
    nbr = vcs.neighbours_ref(X, order, m)
    logdet, G = vcs.brute_force(X, order, nbr, case["model"], case["par"], W)
    return order, nbr, logdet, G, dense_reference(name)[3]


@functools.lru_cache(maxsize=None)
def grad_gram_reference(name):
    """(logdet, G, bar) in long double of W = [V | X] of the gradient problem without its field of zeros (whose G_00 = 0 gives the
    relative error of an entry no scale)."""
    case = case_of(name)
    adj, dco, V, X = grad_inputs(name)
    logdet, G = lc.brute_force(adj, case["model"], case["par"], np.hstack([V[:, 1:], X]))
    return logdet, G, case["n"] * U * grad_reference(name)[3]


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """(grad, trace piece, quadratic piece, kappa_2) in long double: the reference gradient with the field of zeros first, and the two
    pieces 1/2 |P|_F |D_k|_F (per parameter) and |a_f|^2 |D_k|_F (per field and parameter) of the bar's factor in ``_grad_cases``."""
    case = case_of(name)
    adj, dco, V, X = grad_inputs(name)
    grad, scale, kappa = gc.gradient_ld(adj, dco, case["model"], case["par"], V, X, case["reml"])
    return grad, scale[0].copy(), scale - scale[0][None, :], kappa


# ------------------------------------------------------------------------------------------------------------- the checks
def check_gram(name, law, k, base, scaled, ref_logdet, ref_G, bar, exact_calls=True, say=print):
    """``base`` and ``scaled`` are (logdet, G) of the base inputs and of ``apply_law``'s.  Asserts the law's row for logdet and G; with
    ``exact_calls`` false (a restatement whose library calls promise no order) the bit-for-bit assertions become 8 units in the last
    place.  Returns the worst error / bar where the bar was used, else 0."""
    n, s = case_of(name)["n"], 2.0 ** k
    (ld0, G0), (ld1, G1) = base, scaled
    shift = n * k * np.log(2.0) if law == 1 else 0.0
    back = G1 * s if law == 1 else (G1 / s / s if law == 3 else G1)  # (a power of two: the multiplication rounds nothing)
    # (|logdet| is the larger of the two: at hole200 the base logdet is 0.84 and the scaled one -2772, whose own last place is 4.5e-13)
    dl, margin = abs(ld1 - (ld0 + shift)), 4 * n * U * max(1.0, abs(ld0), abs(ld1))
    say("%-8s law %d k %3d: |logdet' - logdet - shift| %.3g (margin %.3g), G back-scaled differs by %.3g ulp" % (name, law, k, dl, margin, ulps(back, G0)))
    assert np.all(np.isfinite(G1)) and np.isfinite(ld1)
    if law == 1:
        assert dl <= margin, (name, law, k, dl, margin)
    elif exact_calls:
        assert ld1 == ld0, (name, law, k, ld1, ld0)
    else:
        assert ulps(ld1, ld0) <= 8
    if exact_here(law, k):
        if exact_calls:
            assert same(back, G0), (name, law, k, ulps(back, G0))
        else:
            assert ulps(back, G0) <= 8, (name, law, k, ulps(back, G0))
        return 0.0
    el, eg = lc.errors(ld1 - shift, back, ref_logdet, ref_G)
    say("%-8s law %d k %3d (odd: the square roots are not scale-free) held to the bar %.3g: logdet error %.3g G error %.3g" % (name, law, k, bar, el, eg))
    assert el <= bar + margin and eg <= bar, (name, law, k, el, eg, bar)
    return max(el - margin, eg) / bar


def grad_factors(law, k, ncol):
    """(alpha, beta): the factors of the trace term and of the quadratic term per gradient column (psill, range, nugget, geometry ...)."""
    s = 2.0 ** k
    one = np.ones(ncol)
    if law == 1:
        a, b = one.copy(), one / s
        a[[0, 2]], b[[0, 2]] = 1.0 / s, 1.0 / s / s
        return a, b
    if law == 2:
        a = one.copy()
        a[1] = 1.0 / s
        return a, a.copy()
    return one, one * s * s


def check_grad(name, law, k, base, scaled, exact_calls=True, say=print, reference=None, n=None):
    """``base`` and ``scaled`` are the (F, 3 + ng) gradients with the field of zeros first.  Row 0 is the trace term: its factor bit for
    bit.  Where both factors agree every row is its factor bit for bit.  Otherwise row f is held to
    1/2 S alpha - (1/2 S - grad_f) beta within 4 2^-52 of the two terms' sizes and 2 2^-52 (|1/2 S| + |grad_f|) beta for the subtraction
    that recovers the quadratic term.  Law 1 with an odd k: held to the bar of ``_grad_cases`` with its two pieces scaled as the terms are,
    against the long-double gradient scaled exactly (``reference``: what ``grad_reference`` returns).  Returns the worst error / bar."""
    g0, g1 = np.asarray(base), np.asarray(scaled)
    alpha, beta = grad_factors(law, k, g0.shape[1])
    assert np.all(np.isfinite(g1))
    if not exact_here(law, k):
        ref, piece_s, piece_t, kappa = reference
        n = case_of(name)["n"] if n is None else n
        want = ref[0][None, :] * alpha.astype(LD) - (ref[0][None, :] - ref) * beta.astype(LD)
        bar = n * U * kappa * (piece_s[None, :] * alpha + piece_t * beta)
        frac = np.abs(g1.astype(LD) - want) / bar
        say("%-8s law %d k %3d (odd) gradient held to the bar: worst / bar per parameter %s" % (name, law, k, " ".join("%8.2e" % float(t) for t in frac.max(axis=0))))
        assert np.all(frac <= 1.0), (name, law, k, float(frac.max()))
        return float(frac.max())
    half_s = g0[0]
    close = (lambda a, b: same(a, b)) if exact_calls else (lambda a, b: ulps(a, b) <= 8)
    assert close(g1[0] / alpha, half_s), (name, law, k, "trace term", ulps(g1[0] / alpha, half_s))
    if np.array_equal(alpha, beta):
        assert close(g1 / alpha[None, :], g0), (name, law, k, ulps(g1 / alpha[None, :], g0))
        say("%-8s law %d k %3d gradient: every row its factor %s" % (name, law, k, "bit for bit" if exact_calls else "within 8 ulp"))
        return 0.0
    half_t = half_s[None, :] - g0
    want = half_s[None, :] * alpha - half_t * beta
    tol = (8 if not exact_calls else 1) * U * (4 * (np.abs(half_s)[None, :] * alpha + np.abs(half_t) * beta) + 2 * (np.abs(half_s)[None, :] + np.abs(g0)) * beta)
    err = np.abs(g1 - want)
    say("%-8s law %d k %3d gradient: trace row exact, worst |row - prediction| / tolerance %.3g" % (name, law, k, float(np.max(err[1:] / tol[1:])) if len(g0) > 1 else 0.0))
    assert np.all(err <= tol), (name, law, k, float(np.max(err / np.where(tol > 0, tol, 1.0))))
    return 0.0
