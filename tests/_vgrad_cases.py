"""What tests/test_vecchia_grad_host.py (CPU) and tests/test_vecchia_grad.py (GPU) share: the cases, the np.longdouble brute force of
include/mikvgrad.h's results from neighbour lists computed on the host, the bar, and a float64 NumPy restatement of k_vgrad_solve /
k_vgrad_reduce.

``pieces`` works every local system [neighbours in list order, the station itself] of Vecchia's approximation -- all positions with the
same number of neighbours at once, as a stack -- in the dtype it is given: the covariances of tests/_lik_cases.py and the derivative
matrices of include/mikgrad.h from float64 distances and differences, S = L L^T by an unblocked Cholesky, y = L^-1 s, beta = L^-T y,
d = sigma - y^T y, u = [-beta ; 1], r(w) = u^T [w_c ; w_p], t = D u, dd = u^T t and dr(w) = -(L^-1 w_c)^T (L^-1 t_c).  In long double
it is the reference; in float64, with the sums over the positions taken in the order of k_vgrad_reduce, it is the restatement.

The bar is the dense gradient's (tests/_grad_cases.py) applied per local system and summed over the positions.  There the elimination
leaves Q = C^-1 with |dQ|_F <~ N u kappa_2(C) |Q|_F, a trace tr(M D) moves by at most |dM|_F |D|_F and a form a^T D a, a = Q w, by
about |a| |da| |D|_F with |da| <~ N u kappa_2 |a| (the constant 1 the project uses throughout).  Here the local matrix Sigma_p has
k_p + 1 rows and its own kappa_2 (that of S is no larger: a principal submatrix), and the terms of a position are
  d_k d_p / d_p = tr((u u^T / d_p) D):          the matrix under the trace is u u^T / d_p, of Frobenius norm |u|^2 / d_p;
  the term of dG[k][a][b] = -a_a^T D a_b + a~_a^T D_cc a~_b, a_w = Sigma_p^-1 [w_c ; w_p], a~_w = S^-1 w_c
  (u u^T / d_p = Sigma_p^-1 - [[S^-1, 0], [0, 0]], differentiated).
So dlogdet[k] is held to sum_p (k_p + 1) 2^-52 kappa_2(Sigma_p) (|u|^2 / d_p) |D|_F and dG[k][a][b] to
sum_p (k_p + 1) 2^-52 kappa_2(Sigma_p) |D|_F (|a_a| |a_b| + |a~_a| |a~_b|), D the local block of D_k.  No margin is added.
"""
import functools

import numpy as np

from oracle.exact_kriging import variogram_ld
from pykrige_amd import likelihood as lk
from tests import _grad_cases as gc
from tests import _lik_cases as lc
from tests import _vecchia_cases as vcs

LD = np.longdouble
U = lc.U
RB = 1024  # mvc::RB: the positions of one partial sum

A2, A3 = gc.A2, gc.A3
# name -> n, ndim, model, [psill, range, nugget], m neighbours, cols of W, ng geometry parameters (0, or all of the dimension: 2 | 5),
# optionally repeat=(k, j): station k repeats station j.  m = 1, 16 | 17, 32 | 33, 64 straddle the size classes of k_vgrad_solve (16 / 32 /
# 64 lanes per station, 16 / 8 / 4 stations per workgroup: no n here is a multiple of its count but 2); cols = 1, 8, 9, 40 straddle the
# groups of eight; n = 1025 and 2049 cross the 1024-position blocks of the reduction and, with a slab of 1024, a slab edge.
CASES = {
    "g2_exp": dict(n=2, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=1, cols=1, ng=2),
    "g67_exp3d_m1": dict(n=67, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], m=1, cols=9, ng=5),
    "g70_gau_m16": dict(n=70, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=16, cols=8, ng=0),
    "g70_gau_m17": dict(n=70, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=17, cols=9, ng=2),
    "g75_sph3d_m32": dict(n=75, ndim=3, model="spherical", par=[1.0, 0.4, 0.1], m=32, cols=1, ng=5),
    "g75_hole_m33": dict(n=75, ndim=2, model="hole-effect", par=[1.0, 0.1, 0.1], m=33, cols=8, ng=2),
    "g90_exp_m64": dict(n=90, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=64, cols=40, ng=2),
    "g129_pair": dict(n=129, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=10, cols=2, ng=2, repeat=(128, 5)),
    "g200_sph_short": dict(n=200, ndim=2, model="spherical", par=[1.0, 0.03, 0.1], m=10, cols=2, ng=2),  # most neighbours beyond the range
    "g1025_gau": dict(n=1025, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=3, cols=1, ng=2),
    "g2049_sph": dict(n=2049, ndim=2, model="spherical", par=[1.0, 0.4, 0.1], m=3, cols=2, ng=0),
    "g60_exact": dict(n=60, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=59, cols=2, ng=2),  # m >= n - 1: the exact likelihood
}
SLAB_CASES = ("g1025_gau", "g2049_sph")
# the small problems on which central differences of the long-double Vecchia objective check the reference itself (CPU only)
HOST_CASES = {
    "h_exp2d": dict(n=40, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=6, cols=2, ng=2),
    "h_gau3d": dict(n=36, ndim=3, model="gaussian", par=[1.0, 0.25, 0.05], m=5, cols=2, ng=5),
    "h_hole": dict(n=40, ndim=2, model="hole-effect", par=[1.0, 0.1, 0.1], m=4, cols=1, ng=2),
    "h_sph": dict(n=50, ndim=2, model="spherical", par=[1.0, 0.4, 0.05], m=7, cols=2, ng=2),
}


def case_of(name):
    return CASES.get(name) or HOST_CASES[name]


def anisotropy(case):
    a = A2 if case["ndim"] == 2 else A3
    return list(a["scaling"]), list(a["angle"])


def inputs(name):
    """(raw (n, ndim), W (n, cols)): random stations in the unit square / cube, standard normal columns."""
    case = case_of(name)
    rng = np.random.default_rng(7300 + 13 * case["n"] + case["cols"] + 101 * case["m"])
    raw = rng.random((case["n"], case["ndim"]))
    W = rng.standard_normal((case["n"], case["cols"]))
    if "repeat" in case:
        k, j = case["repeat"]
        raw[k] = raw[j]
    return raw, W


def problem(name):
    """(adjusted coordinates, dcoords (ng, n, ndim), W, order, neighbours) of a case: the 'random' order with seed 0 and the lists of
    ``_vecchia_cases.neighbours_ref`` in the adjusted metric."""
    case = case_of(name)
    raw, W = inputs(name)
    sc, an = anisotropy(case)
    adj = gc.adjusted(raw, sc, an)
    dco = lk.anisotropy_derivatives(raw, sc, an)[:case["ng"]]
    order = vcs.order_of(case["n"])
    return adj, dco, W, order, vcs.neighbours_ref(adj, order, case["m"])


def _factors(model, par, d64, dtype):
    """c_p, c_r, c_g of include/mikgrad.h at the float64 distances d64, in dtype; c_g = 0 where d = 0."""
    d = d64.astype(dtype)
    psill, r = dtype(par[0]), dtype(par[1])
    one, two, three = dtype(1), dtype(2), dtype(3)
    dd = np.where(d64 > 0.0, d, one)
    if model == "gaussian":
        s = r * dtype(4) / dtype(7)
        E = np.exp(-(d * d) / (s * s))
        cp, cr, cg = E, psill * E * ((two * (d * d)) / ((s * s) * r)), -(psill * E * (two / (s * s))) + 0 * d
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
    return cp, cr, np.where(d64 > 0.0, cg, dtype(0))


def _lower_solve(L, B):
    """L^-1 B for stacks: L (P, k, k) lower triangular, B (P, k, c)."""
    Y = np.zeros_like(B)
    for i in range(L.shape[1]):
        Y[:, i] = (B[:, i] - np.einsum("pj,pjc->pc", L[:, i, :i], Y[:, :i])) / L[:, i, i][:, None]
    return Y


def _upper_solve(L, B):
    """L^-T B for stacks."""
    k = L.shape[1]
    Y = np.zeros_like(B)
    for i in range(k - 1, -1, -1):
        Y[:, i] = (B[:, i] - np.einsum("pj,pjc->pc", L[:, i + 1:, i], Y[:, i + 1:])) / L[:, i, i][:, None]
    return Y


def pieces(adj, dco, order, nbr, model, par, W, dtype=LD, norms=False):
    """Per position p (rows in position order): r (n, cols), d (n,), dr (n, K, cols), dd (n, K) with K = 3 + ng -- or (None, station) for
    the earliest position whose local system has a pivot <= 0.  With ``norms`` also the bar's factors: kp + 1, kappa_2(Sigma_p),
    |u|^2 / d, |D|_F (n, K), |a_w| (n, cols) and |a~_w| (n, cols)."""
    adj, W = np.asarray(adj, dtype=np.float64), np.asarray(W, dtype=np.float64)
    dco = np.asarray(dco, dtype=np.float64).reshape(-1, adj.shape[0], adj.shape[1])
    n, ndim = adj.shape
    mc, K = W.shape[1], 3 + len(dco)
    m = nbr.shape[1]
    r, d, dr, dd = np.zeros((n, mc), dtype), np.zeros(n, dtype), np.zeros((n, K, mc), dtype), np.zeros((n, K), dtype)
    nm = dict(size=np.zeros(n), kappa=np.zeros(n), uu=np.zeros(n), D=np.zeros((n, K)), a=np.zeros((n, mc)), at=np.zeros((n, mc)))
    sigma = dtype(par[0]) + dtype(par[2])
    kps = np.minimum(np.arange(n), m)
    bad = []
    for k in sorted(set(kps.tolist())):
        pos = np.nonzero(kps == k)[0]
        st = np.asarray(order)[pos]
        idx = np.concatenate([nbr[st][:, :k], st[:, None]], axis=1)  # (P, k + 1) local stations
        Xl = adj[idx]
        h = [Xl[:, :, None, c] - Xl[:, None, :, c] for c in range(ndim)]  # float64 differences
        d2 = h[0] * h[0] + h[1] * h[1]
        if ndim == 3:
            d2 = d2 + h[2] * h[2]
        d64 = np.sqrt(d2)
        eye = np.eye(k + 1, dtype=bool)[None]
        A = np.where(eye, sigma, (LD(par[0]) + LD(par[2]) - variogram_ld(model, par, d64)).astype(dtype))
        cp, cr, cg = _factors(model, par, d64, dtype)
        zero, one = dtype(0), dtype(1)
        Ds = [np.where(eye, one, cp), np.where(eye, zero, cr), np.where(eye, one, zero) + 0 * cp]
        for g in range(len(dco)):
            El = dco[g][idx]
            w = np.zeros(d64.shape, dtype)
            for c in range(ndim):
                w = w + h[c].astype(dtype) * (El[:, :, None, c] - El[:, None, :, c]).astype(dtype)
            Ds.append(np.where(eye, zero, cg * w))
        P = len(pos)
        L = np.zeros((P, k, k), dtype)
        for j in range(k):
            piv = A[:, j, j] - np.einsum("pi,pi->p", L[:, j, :j], L[:, j, :j])
            bad += [int(q) for q in pos[~(piv > 0)]]
            piv = np.where(piv > 0, piv, one)
            L[:, j, j] = np.sqrt(piv)
            L[:, j + 1:, j] = (A[:, j + 1:k, j] - np.einsum("pik,pk->pi", L[:, j + 1:, :j], L[:, j, :j])) / L[:, j, j][:, None]
        Wl = W[idx].astype(dtype)  # (P, k + 1, mc)
        y = _lower_solve(L, A[:, :k, k][:, :, None])
        beta = _upper_solve(L, y)[:, :, 0]
        dp = sigma - np.einsum("pi,pi->p", y[:, :, 0], y[:, :, 0])
        bad += [int(q) for q in pos[~(dp > 0)]]
        u = np.concatenate([-beta, np.ones((P, 1), dtype)], axis=1)
        z = _lower_solve(L, Wl[:, :k])
        r[pos], d[pos] = Wl[:, k] - np.einsum("pi,pic->pc", y[:, :, 0], z), dp
        T = np.stack([np.einsum("pij,pj->pi", D, u) for D in Ds], axis=2)  # (P, k + 1, K)
        dd[pos] = np.einsum("pi,pik->pk", u, T)
        dr[pos] = -np.einsum("pic,pik->pkc", z, _lower_solve(L, T[:, :k]))
        if norms:
            at = _upper_solve(L, z)  # S^-1 w_c
            ap = r[pos] / dp[:, None]
            ac = at - beta[:, :, None] * ap[:, None, :]
            f = lambda v: np.asarray(v, dtype=np.float64)
            nm["size"][pos] = k + 1
            nm["kappa"][pos] = np.linalg.cond(f(A), 2)
            nm["uu"][pos] = f(np.einsum("pi,pi->p", u, u) / dp)
            nm["D"][pos] = np.stack([np.sqrt(f(np.einsum("pij,pij->p", D, D))) for D in Ds], axis=1)
            nm["a"][pos] = np.sqrt(f(np.einsum("pic,pic->pc", ac, ac) + ap * ap))
            nm["at"][pos] = np.sqrt(f(np.einsum("pic,pic->pc", at, at)))
    if bad:
        return None, int(np.asarray(order)[min(bad)]) + 1
    return (r, d, dr, dd, nm) if norms else (r, d, dr, dd)


def _sum(x, two_phase):
    """The sum over the positions (axis 0): exact order is the reduction's -- sequential within blocks of RB, then the blocks in order."""
    if not two_phase:
        return np.sum(x, axis=0)
    parts = [np.cumsum(x[b:b + RB], axis=0)[-1] for b in range(0, len(x), RB)]
    return np.cumsum(np.array(parts), axis=0)[-1]


def totals(r, d, dr, dd, two_phase=False):
    """(logdet, G, dlogdet, dG) from the per-position rows, each term spelled as include/mikvgrad.h spells it."""
    logdet = _sum(np.log(d), two_phase)
    G = _sum(r[:, :, None] * r[:, None, :] / d[:, None, None], two_phase)
    dlogdet = _sum(dd / d[:, None], two_phase)
    ra, rb = r[:, None, :, None], r[:, None, None, :]
    da, db = dr[:, :, :, None], dr[:, :, None, :]
    dn = d[:, None, None, None]
    dG = _sum((da * rb + ra * db) / dn - ((ra * rb) * dd[:, :, None, None]) / (dn * dn), two_phase)
    return logdet, G, dlogdet, dG


@functools.lru_cache(maxsize=None)
def reference(name):
    """(logdet, G, dlogdet, dG, bar_dlogdet, bar_dG, worst kappa_2, scale_dlogdet, scale_dG) of a case in long double, computed once
    and shared; do not write into it.  The scales are the bars without (k_p + 1) 2^-52 kappa_2: the magnitudes the errors are relative
    to."""
    case = case_of(name)
    adj, dco, W, order, nbr = problem(name)
    r, d, dr, dd, nm = pieces(adj, dco, order, nbr, case["model"], case["par"], W, LD, norms=True)
    w = nm["size"] * U * nm["kappa"]
    bar_dlogdet = np.sum((w * nm["uu"])[:, None] * nm["D"], axis=0)
    pair = nm["a"][:, :, None] * nm["a"][:, None, :] + nm["at"][:, :, None] * nm["at"][:, None, :]
    bar_dG = np.einsum("p,pk,pab->kab", w, nm["D"], pair)
    scales = (np.sum(nm["uu"][:, None] * nm["D"], axis=0), np.einsum("pk,pab->kab", nm["D"], pair))
    return totals(r, d, dr, dd) + (bar_dlogdet, bar_dG, float(nm["kappa"].max())) + scales


def float64_grad(adj, dco, order, nbr, model, par, W):
    """k_vgrad_solve and k_vgrad_reduce restated in float64 NumPy: (logdet, G, dlogdet, dG), or (None, station)."""
    got = pieces(adj, dco, order, nbr, model, par, W, np.float64)
    if got[0] is None:
        return got
    return totals(*got, two_phase=True)


def worst(got, name):
    """The largest |entry - reference| / bar over dlogdet and over dG of (logdet, G, dlogdet, dG); an entry whose bar is 0 must be the
    reference exactly (the spherical model beyond its range) and counts as 0, or inf."""
    ref = reference(name)

    def frac(x, want, bar):
        err = np.abs(np.asarray(x, dtype=np.float64).astype(LD) - want).astype(np.float64)
        return float(np.max(np.where(bar > 0.0, err / np.where(bar > 0.0, bar, 1.0), np.where(err == 0.0, 0.0, np.inf))))

    return frac(got[2], ref[2], ref[4]), frac(got[3], ref[3], ref[5])


def central_differences(name, h=1e-5):
    """(dlogdet, dG) by central differences of ``_vecchia_cases.brute_force`` -- the long-double Vecchia logdet and G -- on the case's
    own order and neighbour lists, with step h in each natural parameter: relative for psill, range, nugget and the scalings, in degrees
    for the angles (the geometry parameters a case leaves out are not moved)."""
    case = case_of(name)
    raw, W = inputs(name)
    _, _, _, order, nbr = problem(name)
    sc, an = anisotropy(case)
    theta = list(case["par"]) + sc + an
    steps = [h * t for t in case["par"]] + [h * t for t in sc] + [h] * len(an)
    dl, dG = [], []
    for k in range(3 + case["ng"]):
        vals = []
        for sign in (1.0, -1.0):
            t = list(theta)
            t[k] = t[k] + sign * steps[k]
            adj = gc.adjusted(raw, t[3:3 + len(sc)], t[3 + len(sc):])
            vals.append(vcs.brute_force(adj, order, nbr, case["model"], t[:3], W))
        width = LD(theta[k] + steps[k]) - LD(theta[k] - steps[k])  # the step that was taken, as float64 arithmetic took it
        dl.append((vals[0][0] - vals[1][0]) / width)
        dG.append((vals[0][1] - vals[1][1]) / width)
    return np.array(dl), np.array(dG)


class StandInGradPlan:
    """``vecchia_grad.VecchiaGradPlan`` without a device: ``neighbours_ref`` and ``float64_grad``, with the conventions of the real one."""

    def __init__(self, coords, m=30, order="random", seed=0):
        X = np.asarray(coords, dtype=np.float64)
        self.n, self.ndim, self.m = X.shape[0], X.shape[1], int(m)
        self.order = vcs.order_of(self.n, "random", seed) if isinstance(order, str) else np.asarray(order, dtype=np.int32)
        self.neighbours = vcs.neighbours_ref(X, self.order, self.m)
        self.calls = 0

    def grad(self, coords, dcoords, model, parameters, W):
        self.calls += 1
        W = np.asarray(W, dtype=np.float64)
        W = W[:, None] if W.ndim == 1 else W
        dco = np.zeros((0, self.n, self.ndim)) if dcoords is None else dcoords
        got = float64_grad(coords, dco, self.order, self.neighbours, model, parameters, W)
        if got[0] is None:
            mc, K = W.shape[1], 3 + len(dco)
            return np.inf, np.full((mc, mc), np.nan), np.full(K, np.nan), np.full((K, mc, mc), np.nan)
        return float(got[0]), got[1], got[2], got[3]

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass
