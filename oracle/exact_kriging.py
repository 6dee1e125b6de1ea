"""Extended-precision kriging reference  --  TEST INFRASTRUCTURE, NOT PRODUCT.

The float64 oracle (kriging_oracle.py) inverts the kriging matrix and multiplies; the device evaluates a different algebra.  Each
carries an error of about cond(A) u of its own, so comparing the two needs bars loose enough for both.  This module computes, for
the same ``KrigingState``, the z and sigma^2 of the problem with an error far below float64 rounding, so the device can be held to
a bar of its own.

What defines the problem stays float64, exactly as the oracle computes it: adjusted coordinates, distances (cdist or
great_circle_distance), the exact-hit rule |bd| <= EPS, drift columns and the moving window's cKDTree neighbour sets.  Everything
after that is np.longdouble (x86 80-bit, u = 2^-64): the variogram values, the assembled A and B, and the solve -- a float64 LU
with iterative refinement whose residuals B - A X and accumulated X are longdouble.  The refined X is accurate to about
cond(A) u_longdouble, 2^11 times below cond(A) u_double; refinement that does not get there raises (never an unrefined answer).
Then z = X[:n] . v and sigma^2 = -X . b (ok.py:680-681) in longdouble.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np
import scipy.linalg

from oracle import kriging_oracle as ko

LD = np.longdouble
U_LD = float(np.finfo(LD).eps) / 2.0  # unit roundoff of the extended type
U_F64 = 2.0 ** -53
MAX_REFINE = 30


class RefinementError(ArithmeticError):
    """Iterative refinement did not converge: the system is too ill-conditioned for a float64 LU to steer it."""


@dataclass
class ExactResult:
    """z / sigma^2 (longdouble) per point and the scales a bar needs: cond_1 of the system that point is solved with, its
    order M, max|v| over the values it combines and max|b| = the largest variogram value on its right-hand side."""

    z: np.ndarray
    ss: np.ndarray
    cond: np.ndarray
    order: np.ndarray
    vscale: np.ndarray
    bscale: np.ndarray


def variogram_ld(model: str, m: Sequence[float], d: np.ndarray) -> np.ndarray:
    """variogram_models.py:25-81 in longdouble on float64 distances (the same formulas as ko.variogram)."""
    d = np.asarray(d, dtype=np.float64).astype(LD)
    p = [LD(float(v)) for v in m]
    if model == "linear":
        return p[0] * d + p[1]
    if model == "power":
        return p[0] * d ** p[1] + p[2]
    psill, rng, nugget = p[0], p[1], p[2]
    if model == "gaussian":
        return psill * (1 - np.exp(-(d * d) / (rng * 4 / 7) ** 2)) + nugget
    if model == "exponential":
        return psill * (1 - np.exp(-d / (rng / 3))) + nugget
    if model == "spherical":
        inside = psill * ((3 * d) / (2 * rng) - (d * d * d) / (2 * rng * rng * rng)) + nugget
        return np.where(d <= rng, inside, psill + nugget)
    if model == "hole-effect":
        q = d / (rng / 3)
        return psill * (1 - (1 - q) * np.exp(-q)) + nugget
    raise ValueError("unknown variogram model %r" % (model,))


# ---------------------------------------------------------------------------------------------- the float64 problem data
def station_distances(st: ko.KrigingState) -> np.ndarray:
    """(n, n) float64 station distances as ko.kriging_matrix computes them."""
    c = st.coords_adj
    if st.geographic:
        return ko.great_circle_distance(c[:, 0][:, None], c[:, 1][:, None], c[:, 0], c[:, 1])
    from scipy.spatial.distance import cdist

    return cdist(c, c, "euclidean")


def point_distances(st: ko.KrigingState, pts_adj: np.ndarray) -> np.ndarray:
    """(npt, n) float64 point-station distances as ko.rhs computes them (3-D: cdist on (z, y, x) columns)."""
    c = st.coords_adj
    if st.geographic:
        return ko.great_circle_distance(pts_adj[:, 0][:, None], pts_adj[:, 1][:, None], c[:, 0], c[:, 1])
    from scipy.spatial.distance import cdist

    rev = slice(None, None, -1) if st.ndim == 3 else slice(None)
    return cdist(pts_adj[:, rev], c[:, rev], "euclidean")


def assemble(st: ko.KrigingState, d_st: np.ndarray, gamma=None) -> np.ndarray:
    """The kriging matrix (ko.kriging_matrix's layout) in longdouble from float64 distances and float64 drift columns."""
    gamma = gamma or (lambda d: variogram_ld(st.model, st.params, d))
    n, p = st.n, st.n_drift
    a = np.zeros((n + p + 1, n + p + 1), dtype=LD)
    a[:n, :n] = -gamma(d_st)
    np.fill_diagonal(a, 0)
    if p:
        f = ko._drift_columns(st, st.coords_adj, st.specified_data).astype(LD)
        a[:n, n:n + p] = f
        a[n:n + p, :n] = f.T
    a[n + p, :n] = 1
    a[:n, n + p] = 1
    return a


def right_hand_sides(st: ko.KrigingState, pts_adj: np.ndarray, bd: np.ndarray, spec_pts=(), gamma=None) -> np.ndarray:
    """(npt, M) longdouble right-hand sides (ko.rhs's layout); the exact-hit rule is decided on the float64 distances."""
    gamma = gamma or (lambda d: variogram_ld(st.model, st.params, d))
    n, p = st.n, st.n_drift
    b = np.zeros((pts_adj.shape[0], n + p + 1), dtype=LD)
    b[:, :n] = -gamma(bd)
    if st.exact_values:
        b[:, :n][np.absolute(bd) <= ko.EPS] = 0
    if p:
        b[:, n:n + p] = ko._drift_columns(st, pts_adj, spec_pts).astype(LD)
    b[:, n + p] = 1
    return b


# ---------------------------------------------------------------------------------------------- the refined solve
def refined_solve(a: np.ndarray, b: np.ndarray):
    """X with a X = b (a: (M, M) longdouble, b: (M, r) longdouble) by a float64 LU and longdouble iterative refinement.
    Returns (X, cond_1(a)).  Each step contracts the error by about cond(a) u_double; it stops when the corrections reach the
    longdouble floor, max(1e-18, 16 cond(a) u_longdouble) of |X| per column, and raises RefinementError if they do not."""
    a64 = a.astype(np.float64)
    lu = scipy.linalg.lu_factor(a64, check_finite=True)
    inv = scipy.linalg.lu_solve(lu, np.eye(a.shape[0]))
    cond = float(np.abs(a64).sum(axis=0).max() * np.abs(inv).sum(axis=0).max())
    if not np.isfinite(cond) or cond * U_F64 > 0.5:
        raise RefinementError("cond_1 = %.3e: a float64 LU cannot steer the refinement" % cond)
    tol = max(1e-18, 16.0 * U_LD * cond)
    x = np.zeros(b.shape, dtype=LD)
    r = b.copy()
    for _ in range(MAX_REFINE):
        dx = scipy.linalg.lu_solve(lu, r.astype(np.float64))
        x += dx.astype(LD)
        r = b - a @ x
        xs = np.abs(x).max(axis=0).astype(np.float64)
        if np.all(np.abs(dx).max(axis=0) <= tol * np.maximum(xs, np.finfo(np.float64).tiny)):
            return x, cond
    raise RefinementError("refinement did not converge in %d steps (cond_1 = %.3e)" % (MAX_REFINE, cond))


def _reduce(st, x, b, values):
    n = values.shape[-1]
    z = np.einsum("...i,...i->...", x[..., :n], values.astype(LD))
    ss = -np.einsum("...i,...i->...", x, b)
    return z, ss


# ---------------------------------------------------------------------------------------------- public entry points
def exact_points(st: ko.KrigingState, pts_adj: np.ndarray, spec_pts: Sequence[np.ndarray] = ()) -> ExactResult:
    """z, sigma^2 at adjusted points (the one-system path: ok.py:650-683, uk.py:922-1009 and the 3-D forms)."""
    pts_adj = np.asarray(pts_adj, dtype=np.float64)
    a = assemble(st, station_distances(st))
    bd = point_distances(st, pts_adj)
    b = right_hand_sides(st, pts_adj, bd, [np.asarray(s, dtype=np.float64).ravel() for s in spec_pts])
    x, cond = refined_solve(a, b.T.copy())
    z, ss = _reduce(st, x.T, b, st.values)
    npt, n = pts_adj.shape[0], st.n
    return ExactResult(z=z, ss=ss, cond=np.full(npt, cond), order=np.full(npt, a.shape[0]),
                       vscale=np.full(npt, float(np.abs(st.values).max())),
                       bscale=np.abs(b[:, :n]).max(axis=1).astype(np.float64))


def neighbours(st: ko.KrigingState, pts_adj: np.ndarray, k: int):
    """(bd, idx): the moving window's cKDTree neighbour sets and their float64 distances, as ko.solve_points_moving_window
    forms them (ok.py:957-960, ok3d.py:901-904; geographic: the tree on unit vectors, great-circle distances)."""
    from scipy.spatial import cKDTree

    rev = slice(None, None, -1) if st.ndim == 3 else slice(None)
    if st.geographic:
        def unit(ll):
            lo, la = ll[:, 0] * np.pi / 180.0, ll[:, 1] * np.pi / 180.0
            return np.stack([np.cos(lo) * np.cos(la), np.sin(lo) * np.cos(la), np.sin(la)], 1)

        _, idx = cKDTree(unit(st.coords_adj)).query(unit(pts_adj), k=k, eps=0.0)
        bd = ko.great_circle_distance(pts_adj[:, 0][:, None], pts_adj[:, 1][:, None], st.coords_adj[idx, 0],
                                      st.coords_adj[idx, 1])
    else:
        bd, idx = cKDTree(st.coords_adj[:, rev]).query(pts_adj[:, rev], k=k, eps=0.0)
    return np.atleast_2d(bd), np.atleast_2d(idx)


def exact_moving_window(st: ko.KrigingState, pts_adj: np.ndarray, k: int) -> ExactResult:
    """Moving-window ordinary kriging: per point the (k+1) x (k+1) system cut out of the full matrix (ok.py:722-758)."""
    if st.n_drift:
        raise ValueError("moving window exists for ordinary kriging only")
    pts_adj = np.asarray(pts_adj, dtype=np.float64)
    bd_all, idx_all = neighbours(st, pts_adj, k)
    a_all = assemble(st, station_distances(st))
    npt = pts_adj.shape[0]
    out = ExactResult(z=np.zeros(npt, dtype=LD), ss=np.zeros(npt, dtype=LD), cond=np.zeros(npt), order=np.full(npt, k + 1),
                      vscale=np.zeros(npt), bscale=np.zeros(npt))
    for i in range(npt):
        sel = np.concatenate((idx_all[i], [a_all.shape[0] - 1]))
        a = a_all[sel[:, None], sel]
        b = np.zeros(k + 1, dtype=LD)
        b[:k] = -variogram_ld(st.model, st.params, bd_all[i])
        if st.exact_values:
            b[:k][np.absolute(bd_all[i]) <= ko.EPS] = 0
        b[k] = 1
        x, cond = refined_solve(a, b[:, None].copy())
        v = st.values[idx_all[i]]
        out.z[i], out.ss[i] = _reduce(st, x[:, 0], b, v)
        out.cond[i], out.vscale[i], out.bscale[i] = cond, float(np.abs(v).max()), float(np.abs(b[:k]).max())
    return out


def bars(res: ExactResult, c: float, z_cap=1e-8, ss_cap=1e-6):
    """Per-point bars C u (cond_1 + M) max|v| on z and C u (cond_1 + M) max|b| on sigma^2, each capped at the absolute bar the
    float64 parity tests use (scaled by max(1, max|z|) / max(1, max|sigma^2|)): never looser than those."""
    g = c * U_F64 * (res.cond + res.order)
    zc = z_cap * max(1.0, float(np.abs(res.z).max()))
    sc = ss_cap * max(1.0, float(np.abs(res.ss).max()))
    return np.minimum(g * res.vscale, zc), np.minimum(g * res.bscale, sc)
