"""What tests/test_vecchia_host.py (CPU) and tests/test_vecchia.py (GPU) share: the neighbour sets of include/mikvecchia.h restated in
NumPy, the np.longdouble brute force of Vecchia's log det and W^T C^-1 W, a float64 restatement of the local elimination of
mik_k_vecchia.h, and the cases.

Coordinates, W, models and parameters are those of tests/_lik_cases.py (``inputs`` on its ``CASES``), whose kappa_2(C) <= 1e5 is asserted
there.  The bar is that module's: every entry of G within N 2^-52 kappa_2(C) of the reference relative to sqrt(G_aa G_bb), logdet within
the same number absolutely, with C the full covariance matrix of the case.  Every local system is a principal submatrix of C, so its
condition number is no larger; no margin is added.

The not-positive-definite inputs are ``_lik_cases.NOT_PD``'s coincident pairs with psill = 1 and nugget = 0: the later of the two stations
has the earlier as its first neighbour (distance 0), so column 0 of its local system has pivot exactly 1 and L_j0 = C_j0; the station's
own row holds the same bits as the neighbour's, so after the first column it is exactly zero and stays zero, and the station's own pivot
is exactly 0 -- the argument of that module's docstring, applied to the local system."""
import functools

import numpy as np

from tests import _lik_cases as lc

LD = np.longdouble
U = lc.U

# (case of _lik_cases.CASES, m): m = 1, 15, 16, 17, 32, 33, 64 straddle the size classes of k_vec_solve (16 / 32 / 64 lanes per station);
# 40 columns are five groups of eight, 17 are 8 + 8 + 1; m >= N - 1 is the exact likelihood
DEVICE = [("n2_exp_m1", 1), ("n63_sph3d_m7", 64), ("n64_exp_m16", 15), ("n64_exp_m16", 16), ("n64_exp_m16", 17), ("n65_gau_m17", 32),
          ("n65_gau_m17", 33), ("n127_hole_m1", 8), ("n129_exp3d_m40", 30), ("n129_pair_m7", 10), ("n333_sph_m7", 20), ("n700_exp_m17", 30)]
# several reduction blocks (1024 positions each) and many workgroups.  kappa_2 <= N (psill + nugget) / nugget = 3.3e4 by Gershgorin
# (lambda_max <= N * 1.1) and the nugget (lambda_min >= 0.1); the bar uses the computed kappa_2
BIG = dict(n=3000, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=1)
BIG_M = 10
# Cases of this module alone (the dense reference of _lik_cases would not finish at these N), in that module's form; `m` is the number of
# W columns.  psill 1, nugget 0.1: kappa_2 <= 1.1 N / 0.1 <= 2.3e4 by Gershgorin; the bar uses the computed kappa_2.
#   v1023 .. v2049: k_vec_reduce sums RB = 1024 positions per partial -- one partial short of full, full, a second partial of one
#   position, two full partials, a third of one position; v1025_exp_c17: the same edge with the widest local systems and 8 + 8 + 1 columns.
#   w*: k_vec_solve packs SOLVE_WAVES * (64 / KPAD) = 4 * 64 / KPAD stations into a workgroup and mvc_plan_gram picks KPAD = 16 for
#   m <= 16, 32 for m <= 32 and 64 beyond (mik_vecchia.hip): 16, 8 and 4 stations.  N one below, at and one above each count, 9 columns.
EDGE = {
    "v1023_exp": dict(n=1023, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=1),
    "v1024_sph3d": dict(n=1024, ndim=3, model="spherical", par=[1.0, 0.4, 0.1], m=1),
    "v1025_gau": dict(n=1025, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=1),
    "v2048_exp3d": dict(n=2048, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], m=1),
    "v2049_sph": dict(n=2049, ndim=2, model="spherical", par=[1.0, 0.4, 0.1], m=1),
    "v1025_exp_c17": dict(n=1025, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=17),
    "w15_exp": dict(n=15, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=9),
    "w16_gau3d": dict(n=16, ndim=3, model="gaussian", par=[1.0, 0.2, 0.1], m=9),
    "w17_sph": dict(n=17, ndim=2, model="spherical", par=[1.0, 0.4, 0.1], m=9),
    "w7_exp3d": dict(n=7, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], m=9),
    "w8_sph": dict(n=8, ndim=2, model="spherical", par=[1.0, 0.4, 0.1], m=9),
    "w9_gau": dict(n=9, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=9),
    "w3_exp": dict(n=3, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=9),
    "w4_gau": dict(n=4, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=9),
    "w5_sph3d": dict(n=5, ndim=3, model="spherical", par=[1.0, 0.4, 0.1], m=9),
}
# (case, m) of the edges above, and of the dense edge cases of _lik_cases with 24 | 25 | 32 | 33 columns
EDGE_DEVICE = [("v1023_exp", 3), ("v1024_sph3d", 3), ("v1025_gau", 3), ("v2048_exp3d", 3), ("v2049_sph", 3), ("v1025_exp_c17", 64),
               ("w15_exp", 16), ("w16_gau3d", 16), ("w17_sph", 16), ("w7_exp3d", 32), ("w8_sph", 32), ("w9_gau", 32), ("w3_exp", 64),
               ("w4_gau", 64), ("w5_sph3d", 64), ("n128_gau_m24", 10), ("n192_sph3d_m25", 20), ("n256_hole_m32", 16), ("n257_exp3d_m33", 33)]
DEVICE = DEVICE + EDGE_DEVICE
# k_vec_knn stages candidates through LDS in tiles of TC = 256: a last tile that is one short of full, full, or holds one candidate
KNN_EDGE_SIZES = (255, 256, 257, 512, 513)
KNN_EDGE_M = (1, 16, 33, 64)


def case_of(name):
    return BIG if name == "big" else EDGE[name] if name in EDGE else lc.CASES[name]


def neighbours_ref(X, order, m):
    """(N, m) int32 station indices, row = station index, -1 beyond min(m, p): for the station at position p the predecessors with the
    smallest d2 = dx*dx + dy*dy (3-D: (dx*dx + dy*dy) + dz*dz) in float64, ascending by (d2, position)."""
    X = np.asarray(X, dtype=np.float64)
    order = np.asarray(order)
    n = len(X)
    P = X[order]  # by position
    out = np.full((n, m), -1, dtype=np.int32)
    for p in range(1, n):
        dx, dy = P[:p, 0] - P[p, 0], P[:p, 1] - P[p, 1]
        d2 = dx * dx + dy * dy
        if X.shape[1] == 3:
            dz = P[:p, 2] - P[p, 2]
            d2 = d2 + dz * dz
        pick = np.lexsort((np.arange(p), d2))[:m]
        out[order[p], :len(pick)] = order[pick]
    return out


def _local(X, order, nbr, p):
    s = int(order[p])
    row = nbr[s]
    idx = [int(t) for t in row[row >= 0]] + [s]
    return s, idx


def brute_force(X, order, nbr, model, par, W):
    """(logdet, G) of Vecchia's covariance in long double, or (None, 1-based station index) for the earliest position whose local system
    has a pivot <= 0.  The local matrices are ``_lik_cases.covariance_ld`` of the local stations [neighbours in list order, the station
    itself]; each is factored by an unblocked Cholesky and [w_c ; w_p] forward-substituted."""
    X = np.asarray(X, dtype=np.float64)
    Wl = np.asarray(W, dtype=np.float64).astype(LD)
    if Wl.ndim == 1:
        Wl = Wl[:, None]
    logdet, G = LD(0), np.zeros((Wl.shape[1],) * 2, dtype=LD)
    for p in range(len(X)):
        s, idx = _local(X, order, nbr, p)
        A = lc.covariance_ld(X[idx], model, par)
        k = len(idx)
        L = np.zeros((k, k), dtype=LD)
        for j in range(k):
            piv = A[j, j] - np.dot(L[j, :j], L[j, :j])
            if not piv > 0:
                return None, s + 1
            L[j, j] = np.sqrt(piv)
            if j + 1 < k:
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        Y = np.zeros((k, Wl.shape[1]), dtype=LD)
        Wc = Wl[idx]
        for i in range(k - 1):
            Y[i] = (Wc[i] - L[i, :i] @ Y[:i]) / L[i, i]
        r = Wc[k - 1] - L[k - 1, :k - 1] @ Y[:k - 1]  # the residual: the last place before its division
        d = L[k - 1, k - 1] ** 2
        logdet = logdet + np.log(d)
        G = G + np.outer(r, r) / d
    return logdet, G


def float64_gram(X, order, nbr, model, par, W):
    """The elimination of k_vec_solve restated in float64 NumPy: the neighbours' matrix S = L L^T left-looking, the station's own row
    y = L^-1 s, d = C_pp - y^T y, z = L^-1 w_c, r = w_p - y^T z; G and logdet summed in position order.  (logdet, G) or (None, station)."""
    X = np.asarray(X, dtype=np.float64)
    Wa = np.asarray(W, dtype=np.float64)
    if Wa.ndim == 1:
        Wa = Wa[:, None]
    logdet, G = 0.0, np.zeros((Wa.shape[1],) * 2)
    sill = float(par[0]) + float(par[2])
    for p in range(len(X)):
        s, idx = _local(X, order, nbr, p)
        A = lc.covariance_ld(X[idx], model, par).astype(np.float64)
        k = len(idx) - 1
        L = np.zeros((k, k))
        for j in range(k):
            col = A[j:k, j] - L[j:k, :j] @ L[j, :j]
            if not col[0] > 0.0 or not np.isfinite(col[0]):
                return None, s + 1
            L[j, j] = np.sqrt(col[0])
            L[j + 1:k, j] = col[1:] / L[j, j]
        y, Z = A[k, :k].copy(), Wa[idx[:k]].copy()
        for i in range(k):
            y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
            Z[i] = (Z[i] - L[i, :i] @ Z[:i]) / L[i, i]
        d = sill - float(y @ y)
        if not d > 0.0 or not np.isfinite(d):
            return None, s + 1
        r = Wa[s] - y @ Z
        logdet += float(np.log(d))
        G += np.outer(r, r) / d
    return logdet, G


def inputs(name):
    """(coords, W) of a case: ``_lik_cases.inputs``."""
    return lc.inputs(case_of(name))


@functools.lru_cache(maxsize=None)
def kappa(name):
    """kappa_2 of the full covariance matrix of the case (float64 eigenvalues of the symmetric C)."""
    case = case_of(name)
    X, _ = inputs(name)
    ev = np.linalg.eigvalsh(lc.covariance_ld(X, case["model"], case["par"]).astype(np.float64))
    return float(ev[-1] / ev[0])


def order_of(n, kind="random", seed=0):
    if kind == "random":
        return np.random.default_rng(seed).permutation(n).astype(np.int32)
    if kind == "reversed":
        return np.arange(n - 1, -1, -1, dtype=np.int32)
    return np.arange(n, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def reference(name, m):
    """(order, neighbours, logdet, G, kappa_2, bar) of a case in the 'random' order with seed 0, computed once and shared; do not write
    into it."""
    case = case_of(name)
    X, W = inputs(name)
    order = order_of(case["n"])
    nbr = neighbours_ref(X, order, m)
    logdet, G = brute_force(X, order, nbr, case["model"], case["par"], W)
    k = kappa(name)
    return order, nbr, logdet, G, k, case["n"] * U * k


errors = lc.errors


class StandInPlan:
    """``vecchia.VecchiaPlan`` without a device: ``neighbours_ref`` and ``float64_gram``, with the conventions of the real one."""

    def __init__(self, coords, m=30, order="random", seed=0):
        X = np.asarray(coords, dtype=np.float64)
        self.n, self.ndim, self.m = X.shape[0], X.shape[1], int(m)
        self.order = order_of(self.n, "random", seed) if isinstance(order, str) else np.asarray(order, dtype=np.int32)
        self.neighbours = neighbours_ref(X, self.order, self.m)
        self.calls = 0

    def gram(self, coords, model, parameters, W):
        self.calls += 1
        logdet, G = float64_gram(coords, self.order, self.neighbours, model, parameters, W)
        if logdet is None:
            mc = 1 if np.ndim(W) == 1 else np.shape(W)[1]
            return np.inf, np.full((mc, mc), np.nan)
        return logdet, G

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass
