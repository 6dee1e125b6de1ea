"""What tests/test_likelihood_grad_host.py (CPU) and tests/test_likelihood_grad.py (GPU) share: the inputs of ``likelihood.gram_grad``,
the np.longdouble reference gradient they are compared with, its bar, the long-double objective whose central differences check the
reference, and a float64 NumPy stand-in for the one device call.

The reference builds C in long double from float64 distances (tests/_lik_cases.py), Q = C^-1 from an unblocked long-double Cholesky
factor and its inverse, P = Q - Q X (X^T Q X)^-1 X^T Q and a_f = P v_f, the derivative matrices D_k by the formulas of
include/mikgrad.h in long double from the float64 distances and differences, and
  grad[f][k] = 1/2 sum(M * D_k) - 1/2 a_f^T D_k a_f,  M = P (REML) or Q (ML).

The bar is derived, not tuned.  The elimination leaves Q with an error dQ, |dQ|_F <~ N u kappa_2(C) |Q|_F (the constant 1 the project
already uses for G); |tr(dQ D)| <= |dQ|_F |D|_F, and a = P y moves a^T D a by about 2 |a| |da| |D| with |da| <~ N u kappa |a|.  With
|P|_F <= |Q|_F standing for the matrix under the trace, parameter k and field f are held to
  N 2^-52 kappa_2(C) (1/2 |P|_F |D_k|_F + |a_f|^2 |D_k|_F).
Every case keeps kappa_2 <= 1e5, asserted on the CPU.
"""
import functools

import numpy as np

from pykrige_amd import core
from pykrige_amd import likelihood as lk
from tests import _lik_cases as lc

LD = np.longdouble
U = lc.U
KAPPA_MAX = lc.KAPPA_MAX

A2 = dict(scaling=[1.3], angle=[25.0])
A3 = dict(scaling=[1.4, 0.7], angle=[10.0, -20.0, 35.0])
# name -> n, ndim, model, [psill, range, nugget], F fields, p trend columns, reml, the anisotropy, and optionally repeat=(k, j).
# N = 2, 63, 64, 65, 129 straddle the 64-column block, the 64 x 64 pair tile and the 128-row update tile; 200 and 333 take several block
# columns, so that identity rows join the elimination at more than one of them; F = 1, 7, 8, 9, 32 straddle the eight-field chunks.
CASES = {
    "n2_exp_f1_ml": dict(n=2, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=1, p=1, reml=False, **A2),
    "n63_sph3d_f1": dict(n=63, ndim=3, model="spherical", par=[1.0, 0.4, 0.05], F=1, p=1, reml=True, **A3),  # 5 geometry parameters
    "n64_exp_f8": dict(n=64, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=8, p=1, reml=True, **A2),
    "n65_gau_f9_p3": dict(n=65, ndim=2, model="gaussian", par=[1.0, 0.2, 0.05], F=9, p=3, reml=True, **A2),
    "n129_pair_f7_ml": dict(n=129, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=7, p=1, reml=False, repeat=(128, 5), **A2),
    "n129_exp3d_f32_p8": dict(n=129, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], F=32, p=8, reml=True, **A3),
    "n200_hole_f1": dict(n=200, ndim=2, model="hole-effect", par=[1.0, 0.1, 0.1], F=1, p=1, reml=True, **A2),  # the short range
    "n333_sph_f7_p4": dict(n=333, ndim=2, model="spherical", par=[1.0, 0.4, 0.05], F=7, p=4, reml=True, **A2),  # exact zeros
    # whole 64 x 64 pair tiles and one row past them: N = 128 (two tiles a side), 192 | 193, 256 | 257, with F = 1 | 8 | 9 around the
    # eight-field chunk.  The reference inverts C in long double, so 257 is the last.  psill 1, nugget 0.1: kappa_2 <= 1.1 N / 0.1
    "n128_exp_f8": dict(n=128, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=8, p=1, reml=True, **A2),
    "n192_gau3d_f9_ml": dict(n=192, ndim=3, model="gaussian", par=[1.0, 0.2, 0.1], F=9, p=2, reml=False, **A3),
    "n193_sph_f1_p3": dict(n=193, ndim=2, model="spherical", par=[1.0, 0.4, 0.1], F=1, p=3, reml=True, **A2),
    "n256_hole_f9": dict(n=256, ndim=2, model="hole-effect", par=[1.0, 0.05, 0.1], F=9, p=1, reml=True, **A2),  # (range 0.05: see _lik_cases)
    "n257_exp3d_f8_p4": dict(n=257, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], F=8, p=4, reml=True, **A3),
}
# the cases above that close the gaps between the tile edges: their worst err / bar is what profiles/fit_edges_parity.txt records
EDGES = ("n128_exp_f8", "n192_gau3d_f9_ml", "n193_sph_f1_p3", "n256_hole_f9", "n257_exp3d_f8_p4")
# the small problems on which central differences of the long-double objective check the reference itself (CPU only)
HOST_CASES = {
    "h_exp2d_ml": dict(n=40, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=2, p=1, reml=False, **A2),
    "h_exp2d_reml": dict(n=40, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=2, p=3, reml=True, **A2),
    "h_gau3d_reml": dict(n=45, ndim=3, model="gaussian", par=[1.0, 0.2, 0.05], F=1, p=1, reml=True, **A3),
    "h_hole3d_ml": dict(n=30, ndim=3, model="hole-effect", par=[1.0, 0.1, 0.1], F=1, p=2, reml=False, **A3),
    "h_regional2d": dict(n=40, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=1, reml=True, drift="regional_linear", **A2),
    "h_regional3d_ml": dict(n=40, ndim=3, model="gaussian", par=[1.0, 0.25, 0.05], F=1, reml=False, drift="regional_linear", **A3),
    "h_pair": dict(n=33, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], F=1, p=1, reml=True, repeat=(32, 5), **A2),
    "h_sph_beyond": dict(n=50, ndim=2, model="spherical", par=[1.0, 0.4, 0.05], F=1, p=2, reml=True, **A2),
}


def inputs(case):
    """(raw (n, ndim), V (n, F), drift (n, p - 1) or None or 'regional_linear'): random stations in the unit square / cube, standard
    normal fields and trend columns."""
    rng = np.random.default_rng(9100 + 31 * case["n"] + case["F"])
    raw = rng.random((case["n"], case["ndim"]))
    V = rng.standard_normal((case["n"], case["F"]))
    if "repeat" in case:
        k, j = case["repeat"]
        raw[k] = raw[j]
    if "drift" in case:
        return raw, V, case["drift"]
    return raw, V, (rng.standard_normal((case["n"], case["p"] - 1)) if case["p"] > 1 else None)


def adjusted(raw, scaling, angle):
    center = [(float(np.amax(c)) + float(np.amin(c))) / 2.0 for c in raw.T]
    return core.adjust_for_anisotropy(raw, center, scaling, angle)


def trend(adj, drift):
    n = len(adj)
    if drift is None:
        return np.ones((n, 1))
    return np.hstack([np.ones((n, 1)), adj if isinstance(drift, str) else drift])


def problem(case):
    """(adjusted coordinates, dcoords (ng, n, ndim), V, X) of a case: the arguments of ``likelihood.gram_grad``."""
    raw, V, drift = inputs(case)
    adj = adjusted(raw, case["scaling"], case["angle"])
    return adj, lk.anisotropy_derivatives(raw, case["scaling"], case["angle"]), V, trend(adj, drift)


def derivative_matrices(adj, dco, model, par, dtype=LD):
    """[dC/dpsill, dC/drange, dC/dnugget, dC/dtheta_0 ...] by the formulas of include/mikgrad.h, evaluated in `dtype` from float64
    distances and float64 coordinate differences."""
    n, ndim = adj.shape
    d64 = lc.distances(adj)
    d = d64.astype(dtype)
    psill, r = dtype(par[0]), dtype(par[1])
    one, two, three = dtype(1), dtype(2), dtype(3)
    off = ~np.eye(n, dtype=bool)
    dd = np.where(d64 > 0.0, d, one)  # (divided by only where d > 0)
    if model == "gaussian":
        s = r * dtype(4) / dtype(7)
        E = np.exp(-(d * d) / (s * s))
        cp, cr, cg = E, psill * E * ((two * (d * d)) / ((s * s) * r)), -(psill * E * (two / (s * s)))
    elif model == "exponential":
        s = r / three
        E = np.exp(-d / s)
        cp, cr, cg = E, psill * E * (d / (s * r)), -((psill * E / s) / dd)
    elif model == "spherical":
        inside = d64 <= float(par[1])
        cp = np.where(inside, one - ((three * d) / (two * r) - (d * d * d) / (two * (r * r * r))), dtype(0))
        cr = np.where(inside, psill * ((three * d) / (two * (r * r)) - (three * (d * d * d)) / (two * (r * r * r * r))), dtype(0))
        cg = np.where(inside, -((psill * (three / (two * r) - (three * (d * d)) / (two * (r * r * r)))) / dd), dtype(0))
    else:
        q = d / (r / three)
        E = np.exp(-q)
        cp, cr, cg = (one - q) * E, psill * (((two - q) * E * q) / r), -((psill * ((two - q) * E / (r / three))) / dd)
    cg = np.where(d64 > 0.0, cg, dtype(0))
    eye = np.eye(n, dtype=dtype)
    out = [np.where(off, cp, one), np.where(off, cr, dtype(0)), eye]
    h = [(adj[:, c][:, None] - adj[:, c][None, :]).astype(dtype) for c in range(ndim)]
    for g in range(len(dco)):
        w = np.zeros((n, n), dtype=dtype)
        for c in range(ndim):
            w = w + h[c] * (dco[g][:, c][:, None] - dco[g][:, c][None, :]).astype(dtype)
        out.append(np.where(off, cg * w, dtype(0)))
    return out


def _cholesky_ld(A):
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        p = A[j, j] - np.dot(L[j, :j], L[j, :j])
        assert p > 0
        L[j, j] = np.sqrt(p)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _inverse_ld(A):
    """A^-1 of a symmetric positive definite matrix from its long-double Cholesky factor."""
    L = _cholesky_ld(A)
    n = len(A)
    Y = np.zeros((n, n), dtype=LD)  # L Y = I
    I = np.eye(n, dtype=LD)
    for i in range(n):
        Y[i] = (I[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y.T @ Y


def gradient_ld(adj, dco, model, par, V, X, reml):
    """(grad (F, 3 + ng), scale (F, 3 + ng), kappa_2): the long-double gradient, the bar's factor in parentheses
    1/2 |P|_F |D_k|_F + |a_f|^2 |D_k|_F, and the condition number of C."""
    Cm = lc.covariance_ld(adj, model, par)
    Q = _inverse_ld(Cm)
    Xl, Vl = X.astype(LD), V.astype(LD)
    QX = Q @ Xl
    P = Q - QX @ _inverse_ld(Xl.T @ QX) @ QX.T
    A = P @ Vl
    M = P if reml else Q
    Ds = derivative_matrices(adj, dco, model, par)
    F = V.shape[1]
    grad, scale = np.zeros((F, len(Ds)), dtype=LD), np.zeros((F, len(Ds)))
    pn = float(np.sqrt(np.sum(P * P)))
    for k, D in enumerate(Ds):
        tr = np.sum(M * D)
        dn = float(np.sqrt(np.sum(D * D)))
        for f in range(F):
            grad[f, k] = LD(0.5) * tr - LD(0.5) * (A[:, f] @ (D @ A[:, f]))
            scale[f, k] = 0.5 * pn * dn + float(A[:, f] @ A[:, f]) * dn
    kappa = float(np.linalg.cond(Cm.astype(np.float64), 2))
    return grad, scale, kappa


@functools.lru_cache(maxsize=None)
def reference(name):
    """(grad, bar, kappa_2) of CASES[name] (or HOST_CASES[name]), computed once and shared; do not write into it."""
    case = CASES.get(name) or HOST_CASES[name]
    adj, dco, V, X = problem(case)
    grad, scale, kappa = gradient_ld(adj, dco, case["model"], case["par"], V, X, case["reml"])
    return grad, case["n"] * U * kappa * scale, kappa


def objective_ld(raw, V, drift, model, par, scaling, angle, reml):
    """(F,) long double: the objective of ``likelihood.nll_from_gram`` on the long-double pieces, the trend rebuilt from the adjusted
    coordinates of THESE anisotropy values when drift is 'regional_linear'."""
    adj = adjusted(raw, scaling, angle)
    X = trend(adj, drift)
    n, F, p = len(raw), V.shape[1], X.shape[1]
    logdet, G = lc.brute_force(adj, model, par, np.hstack([V, X]))
    Xl = X.astype(LD)
    ldx = LD(2) * np.sum(np.log(np.diag(_cholesky_ld(Xl.T @ Xl))))
    Lx = _cholesky_ld(G[F:, F:])
    lgx = LD(2) * np.sum(np.log(np.diag(Lx)))
    Gi = _inverse_ld(G[F:, F:])
    log_two_pi = np.log(LD(8) * np.arctan(LD(1)))
    out = np.zeros(F, dtype=LD)
    for f in range(F):
        q = G[f, f] - G[F:, f] @ (Gi @ G[F:, f])
        out[f] = LD(0.5) * ((n - p) * log_two_pi - ldx + logdet + lgx + q) if reml else LD(0.5) * (n * log_two_pi + logdet + q)
    return out


def central_differences(case, h=1e-5):
    """(F, 3 + ng) long double: central differences of ``objective_ld`` with step h in each natural parameter -- relative for psill,
    range, nugget and the scalings, in degrees for the angles."""
    raw, V, drift = inputs(case)
    par, sc, an = list(case["par"]), list(case["scaling"]), list(case["angle"])
    theta = par + sc + an
    steps = [h * t for t in par] + [h * t for t in sc] + [h] * len(an)
    cols = []
    for k, st in enumerate(steps):
        vals = []
        for sign in (1.0, -1.0):
            t = list(theta)
            t[k] = t[k] + sign * st
            vals.append(objective_ld(raw, V, drift, case["model"], t[:3], t[3:3 + len(sc)], t[3 + len(sc):], case["reml"]))
        # the step that was taken, as float64 arithmetic took it
        cols.append((vals[0] - vals[1]) / (LD(theta[k] + st) - LD(theta[k] - st)))
    return np.array(cols).T


# ------------------------------------------------------------------------------------------------------------- a float64 stand-in
def standin_gram(coords, model, parameters, W):
    """``likelihood.gram`` in float64 NumPy."""
    Cm = lc.covariance_ld(np.asarray(coords, dtype=np.float64), model, parameters).astype(np.float64)
    W = np.asarray(W, dtype=np.float64)
    W = W[:, None] if W.ndim == 1 else W
    try:
        L = np.linalg.cholesky(Cm)
    except np.linalg.LinAlgError:
        return np.inf, np.full((W.shape[1],) * 2, np.nan)
    Y = np.linalg.solve(L, W)
    return 2.0 * float(np.sum(np.log(np.diag(L)))), Y.T @ Y


def standin_gram_grad(coords, dcoords, model, parameters, V, X, reml):
    """``likelihood.gram_grad`` in float64 NumPy: (logdet, G, grad, info)."""
    adj = np.asarray(coords, dtype=np.float64)
    V, X = np.asarray(V, dtype=np.float64), np.asarray(X, dtype=np.float64)
    F, m = V.shape[1], V.shape[1] + X.shape[1]
    dco = np.asarray(dcoords, dtype=np.float64).reshape(-1, len(adj), adj.shape[1])
    logdet, G = standin_gram(adj, model, parameters, np.hstack([V, X]))
    if not np.isfinite(logdet):
        return np.inf, np.full((m, m), np.nan), np.full((F, 3 + len(dco)), np.nan), 1
    Q = np.linalg.inv(lc.covariance_ld(adj, model, parameters).astype(np.float64))
    QX = Q @ X
    P = Q - QX @ np.linalg.solve(X.T @ QX, QX.T)
    A = P @ V
    M = P if reml else Q
    Ds = derivative_matrices(adj, dco, model, parameters, dtype=np.float64)
    grad = np.array([[0.5 * np.sum(M * D) - 0.5 * A[:, f] @ D @ A[:, f] for D in Ds] for f in range(F)])
    return logdet, G, grad, 0
