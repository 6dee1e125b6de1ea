"""What tests/test_likelihood_host.py (CPU) and tests/test_likelihood.py (GPU) share: the inputs of ``likelihood.gram``, the
np.longdouble brute force they are compared with, the bar, and a float64 NumPy restatement of the blocked elimination of mik_k_lik.h.

The brute force builds C from float64 distances with ``oracle.exact_kriging.variogram_ld`` (C_ii = psill + nugget, C_ij = (psill +
nugget) - gamma(d_ij), the formula applied at d = 0 too), runs an unblocked long-double Cholesky and a forward substitution and returns
logdet = 2 sum log L_ii and G = W^T C^-1 W = Y^T Y with L Y = W.

The bar is derived, not tuned: a backward-stable Cholesky of an n x n matrix has a relative forward error bounded by a modest multiple
of n u kappa_2(C), so every entry of G is held to N 2^-52 kappa_2(C) relative to sqrt(G_aa G_bb), and logdet to the same number
absolutely.  kappa_2 is NumPy's (float64 SVD of C).  Every case must keep kappa_2 <= 1e5, asserted on the CPU: the bar never exceeds
about 2e-8.

The not-positive-definite inputs are exact by construction, not by luck of rounding: station k repeats station 0 with psill = 1 and
nugget = 0, so C_00 = 1, L_00 = 1 and L_j0 = C_j0 exactly; rows 0 and k of C hold the same bits, so after the first column row k of the
trailing matrix is C_kj - 1 * C_j0 = 0 exactly, it stays zero through every later update (0 * x = 0, and a sum of zeros), and the pivot
of column k is 0 -- in any blocking, in float64 and in long double alike.  The failing column is k + 1, counted from 1.
"""
import functools
import os

import numpy as np

from oracle.exact_kriging import variogram_ld

LD = np.longdouble
U = 2.0 ** -52
KAPPA_MAX = 1e5
NB = 64  # mlk::NB: the block column of mik_k_lik.h; the update tiles are 128 x 128

# name -> n, ndim, model, [psill, range, nugget], m, and optionally repeat=(k, j): station k repeats station j.
# N = 2, 63, 64, 65, 127, 129 straddle the 64-column block and the 128-row update tile; 200, 333, 700 take several block columns and
# more than one update tile per side; m = 1, 7, 16, 17, 40 straddle the 16-row padding of W^T (16 / 32 / 48 rows).
CASES = {
    "n2_exp_m1": dict(n=2, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=1),
    "n63_sph3d_m7": dict(n=63, ndim=3, model="spherical", par=[1.0, 0.4, 0.05], m=7),
    "n64_exp_m16": dict(n=64, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=16),
    "n65_gau_m17": dict(n=65, ndim=2, model="gaussian", par=[1.0, 0.2, 0.05], m=17),
    # (hole-effect is no valid covariance in the plane at a range that many stations share: with range 0.5 it is NOT_PD's third case;
    # at range 0.1, where a station has a few neighbours inside the first lobe, C is positive definite)
    "n127_hole_m1": dict(n=127, ndim=2, model="hole-effect", par=[1.0, 0.1, 0.1], m=1),
    "n129_exp3d_m40": dict(n=129, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], m=40),
    "n129_pair_m7": dict(n=129, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=7, repeat=(128, 5)),  # one coincident pair, with a nugget
    "n150_gau3d_m1": dict(n=150, ndim=3, model="gaussian", par=[1.0, 0.2, 0.05], m=1),
    "n200_exp_m1": dict(n=200, ndim=2, model="exponential", par=[1.0, 0.5, 0.1], m=1),
    "n333_sph_m7": dict(n=333, ndim=2, model="spherical", par=[1.0, 0.4, 0.05], m=7),  # range < domain: exact zeros in C
    "n700_exp_m17": dict(n=700, ndim=2, model="exponential", par=[1.0, 1.0, 0.01], m=17),
    # a whole number of tiles, and one row past it: N = 128 (one update tile, two block columns), 192 (three block columns), 256 | 257,
    # 512 | 513; m = 24 | 25 and 32 | 33 straddle the eight-column groups and the 16-row padding of W^T.  psill 1, nugget 0.1: by
    # Gershgorin kappa_2 <= 1.1 N / 0.1 for the three valid models; hole-effect at N = 256 needs range 0.05 to stay positive definite in
    # the plane (at range 0.1 the pivot of column 114 fails) and has kappa_2 = 8.4
    "n128_gau_m24": dict(n=128, ndim=2, model="gaussian", par=[1.0, 0.2, 0.1], m=24),
    "n192_sph3d_m25": dict(n=192, ndim=3, model="spherical", par=[1.0, 0.4, 0.1], m=25),
    "n256_hole_m32": dict(n=256, ndim=2, model="hole-effect", par=[1.0, 0.05, 0.1], m=32),
    "n257_exp3d_m33": dict(n=257, ndim=3, model="exponential", par=[1.0, 0.5, 0.1], m=33),
    "n512_sph_m1": dict(n=512, ndim=2, model="spherical", par=[1.0, 0.4, 0.1], m=1),
    "n513_gau3d_m7": dict(n=513, ndim=3, model="gaussian", par=[1.0, 0.2, 0.1], m=7),
}
# the cases above that close the gaps between the tile edges: their worst err / bar is what profiles/fit_edges_parity.txt records
EDGES = ("n128_gau_m24", "n192_sph3d_m25", "n256_hole_m32", "n257_exp3d_m33", "n512_sph_m1", "n513_gau3d_m7")
# not positive definite -- two coincident stations with zero nugget, and the hole-effect model: name -> case, and the 1-based column of the
# pivot that fails
NOT_PD = {
    "notpd_n2": (dict(n=2, ndim=2, model="exponential", par=[1.0, 0.5, 0.0], m=1, repeat=(1, 0)), 2),
    "notpd_n200": (dict(n=200, ndim=2, model="exponential", par=[1.0, 0.5, 0.0], m=7, repeat=(150, 0)), 151),
    # hole-effect at range 0.5: the leading 18 x 18 block has an eigenvalue of -0.05, the 17 x 17 one of +0.02 -- far from rounding
    "notpd_hole_n127": (dict(n=127, ndim=2, model="hole-effect", par=[1.0, 0.5, 0.1], m=1), 18),
}


def record(line):
    """Print a figure, and append it to the file the environment variable FIT_EDGES_PARITY_OUT names (never by default): how
    profiles/fit_edges_parity.txt is written."""
    print(line)
    path = os.environ.get("FIT_EDGES_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def inputs(case):
    """(coords (n, ndim), W (n, m)) of a case: random stations in the unit square / cube, standard normal columns."""
    rng = np.random.default_rng(4200 + 17 * case["n"] + case["m"])
    X = rng.random((case["n"], case["ndim"]))
    W = rng.standard_normal((case["n"], case["m"]))
    if "repeat" in case:
        k, j = case["repeat"]
        X[k] = X[j]
    return X, W


def distances(X):
    """float64 Euclidean distances, sqrt(dx*dx + dy*dy (+ dz*dz)) as include/miklik.h spells them."""
    d2 = np.zeros((len(X), len(X)))
    for c in range(X.shape[1]):
        diff = X[:, c][:, None] - X[:, c][None, :]
        d2 = d2 + diff * diff
    return np.sqrt(d2)


def covariance_ld(X, model, par):
    """C in long double from float64 distances."""
    sill = LD(par[0]) + LD(par[2])
    Cm = sill - variogram_ld(model, par, distances(X))
    Cm[np.diag_indices(len(X))] = sill
    return Cm


def brute_force(X, model, par, W):
    """(logdet, G) in long double, or None with the 1-based column if a pivot is <= 0."""
    A = covariance_ld(X, model, par)
    n = len(A)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        p = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not p > 0:
            return None, j + 1
        L[j, j] = np.sqrt(p)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.zeros(W.shape, dtype=LD)
    Wl = np.asarray(W, dtype=np.float64).astype(LD)
    for i in range(n):
        Y[i] = (Wl[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return LD(2) * np.sum(np.log(np.diag(L))), Y.T @ Y


@functools.lru_cache(maxsize=None)
def reference(name):
    """(logdet, G, kappa_2, bar) of CASES[name], computed once and shared; do not write into it."""
    case = CASES[name]
    X, W = inputs(case)
    logdet, G = brute_force(X, case["model"], case["par"], W)
    if logdet is None:
        return None, G, np.inf, np.inf
    kappa = float(np.linalg.cond(covariance_ld(X, case["model"], case["par"]).astype(np.float64), 2))
    return logdet, G, kappa, case["n"] * U * kappa


def errors(logdet, G, ref_logdet, ref_G):
    """(|logdet - ref|, max |G_ab - ref_ab| / sqrt(ref_aa ref_bb))."""
    s = np.sqrt(np.diag(ref_G))
    eg = np.abs(np.asarray(G, dtype=np.float64).astype(LD) - ref_G) / (s[:, None] * s[None, :])
    return float(abs(LD(logdet) - ref_logdet)), float(eg.max())


def blocked_float64(X, model, par, W, nb=NB):
    """The elimination of mik_k_lik.h restated in float64 NumPy: the lower triangle of [[C, .], [W^T, 0]], right-looking by block columns
    of nb -- an unblocked Cholesky of the diagonal block, the rows below it times L^-T by forward substitution, the trailing update --
    stopped after the first n columns.  (logdet, G), or (None, column)."""
    n, m = W.shape
    A = np.zeros((n + m, n + m))
    A[:n, :n] = covariance_ld(X, model, par).astype(np.float64)
    A[n:, :n] = W.T
    for k0 in range(0, n, nb):
        jb = min(nb, n - k0)
        S = A[k0:k0 + jb, k0:k0 + jb]
        for k in range(jb):
            if not S[k, k] > 0.0 or not np.isfinite(S[k, k]):
                return None, k0 + k + 1
            S[k, k] = np.sqrt(S[k, k])
            S[k + 1:, k] /= S[k, k]
            for j in range(k + 1, jb):
                S[j:, j] -= S[j:, k] * S[j, k]
        r0 = k0 + jb
        P = A[r0:, k0:r0]
        for j in range(jb):
            P[:, j] = (P[:, j] - P[:, :j] @ S[j, :j]) / S[j, j]
        A[r0:, r0:] -= P @ P.T
    return 2.0 * float(np.sum(np.log(np.diag(A)[:n]))), -A[n:, n:]
