"""Vecchia's likelihood of a variogram model with its analytic gradient on the GPU, and a quasi-Newton ML / REML fit on it.

ctypes binding of libmikvgrad.so (include/mikvgrad.h), a seventh library, loaded on first use.  NumPy + ctypes (+ scipy.optimize for the
fit).  There is no CPU fallback: a missing library or no visible GPU raises.  Every argument error is a ValueError (NotImplementedError
for a custom model) raised here, before the library is loaded.

``vecchia.VecchiaPlan.gram`` returns ``logdet`` and ``G = W^T C^-1 W`` of Vecchia's covariance; ``VecchiaGradPlan.grad`` returns the same
two -- the same bits -- and their derivatives with respect to psill, range, nugget and the geometry parameters, from the same N small
factorisations and a handful of further substitutions per station.  ``likelihood.nll_grad_from_gram`` takes them through the ML / REML
algebra, and ``fit_variogram_vecchia_grad`` minimises with L-BFGS-B what ``vecchia.fit_variogram_vecchia`` searches with Nelder-Mead.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _dl
from .likelihood import MODEL_IDS, MLFit, _Fit, _fit_lbfgsb, _gram_arguments, _ml_fit, _nll_arguments, _pieces  # noqa: F401
from .likelihood import GRAD_NAMES_2D, GRAD_NAMES_3D, MAXGEOM, anisotropy_derivatives, nll_from_gram, nll_grad_from_gram  # noqa: F401
from .vecchia import MAXNB, START_SUBSAMPLE, _FIT_NAMES, _PLAN_NAMES, _check_m, _order, _plan_arguments

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmikvgrad.so")

MVG_OK, MVG_EINVAL, MVG_ENOTPD, MVG_EHIP = 0, -1, -2, -3
ABI_VERSION = 1  # include/mikvgrad.h MVG_ABI_VERSION

_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_plan_p = C.c_void_p

# every entry point include/mikvgrad.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mvg_abi_version": (C.c_int, []),
    "mvg_last_error": (C.c_char_p, []),
    "mvg_plan_create": (C.c_int, [C.c_int, C.c_int64, C.c_int32, _dp, _i32p, C.c_int32, C.POINTER(_plan_p)]),
    "mvg_plan_neighbours": (C.c_int, [_plan_p, _i32p]),
    "mvg_plan_grad": (C.c_int, [_plan_p, _dp, C.c_int32, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, _dp, C.c_int32, _dp, _dp, _dp, _dp,
                                _i32p]),
    "mvg_plan_destroy": (None, [_plan_p]),
}

_lib = None


def load():
    """dlopen libmikvgrad.so and declare the signatures.  Raises ImportError if it has not been built or is stale."""
    global _lib
    if _lib is None:
        _lib = _dl.open_library(LIB_PATH, "mvg", ABI_VERSION, SIGNATURES)
    return _lib


def _raise(lib, rc):
    _dl.raise_for(lib, "mvg", "libmikvgrad", rc, MVG_EINVAL)


class VecchiaGradPlan:
    """``VecchiaGradPlan(coords, m=30, order="random", seed=0)``: the neighbour sets of Vecchia's approximation, found on the GPU once
    and kept there for every ``grad`` that follows.  The arguments, the attributes (``n``, ``m``, ``order``, ``neighbours``), the
    neighbour sets themselves and the context-manager behaviour are ``vecchia.VecchiaPlan``'s; the handle is one of libmikvgrad.so.
    Argument errors raise ValueError before the library is loaded; there is no CPU fallback."""

    def __init__(self, coords, m=30, order="random", seed=0):
        who = "VecchiaGradPlan"
        self._handle = None
        X = np.asarray(coords, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] not in (2, 3):
            raise ValueError("%s: coords must have shape (N, 2) or (N, 3), got %s" % (who, np.shape(coords)))
        if X.shape[0] < 2:
            raise ValueError("%s: need at least two stations" % who)
        if not np.all(np.isfinite(X)):
            raise ValueError("%s: station coordinates must be finite" % who)
        self.m = _check_m(who, m)
        self.n, self.ndim = int(X.shape[0]), int(X.shape[1])
        self.order = _order(who, order, X, seed)
        self._neighbours = None
        ct = np.ascontiguousarray(X.T)
        handle = _plan_p()
        lib = load()
        rc = lib.mvg_plan_create(_dl.device(), self.n, self.ndim, ct.ctypes.data_as(_dp), self.order.ctypes.data_as(_i32p), self.m,
                                 C.byref(handle))
        if rc != MVG_OK:
            _raise(lib, rc)
        self._handle = handle

    @property
    def neighbours(self):
        if self._neighbours is None:
            if self._handle is None:
                raise ValueError("VecchiaGradPlan: the plan is closed")
            out = np.empty((self.n, self.m), dtype=np.int32)
            lib = load()
            rc = lib.mvg_plan_neighbours(self._handle, out.ctypes.data_as(_i32p))
            if rc != MVG_OK:
                _raise(lib, rc)
            out.setflags(write=False)
            self._neighbours = out
        return self._neighbours

    def grad(self, coords, dcoords, model, parameters, W):
        """``logdet, G, dlogdet, dG = plan.grad(coords, dcoords, model, parameters, W)``: one call of ``mvg_plan_grad``.  coords, model,
        parameters and W are ``VecchiaPlan.gram``'s, and logdet and G are its results bit for bit.  dcoords: (ng, N, ndim), 0 <= ng <= 5
        (None for ng = 0), for each geometry parameter the derivative of the adjusted coordinates (``likelihood.anisotropy_derivatives``).
        dlogdet is (3 + ng,) and dG (3 + ng, m_cols, m_cols): the derivatives with respect to psill, range, nugget and the ng geometry
        parameters; every dG[k] is exactly symmetric, the results are the same bits from run to run, and dG[k][a][b] depends only on
        columns a and b.  If a local system is not positive definite in float64, logdet is ``inf`` and G, dlogdet and dG are NaN."""
        who = "VecchiaGradPlan.grad"
        _, _, psill, rng, nugget, mc, ct, wt = _gram_arguments(who, coords, model, parameters, W, "MVG_MAXCOLS", (self.n, self.ndim))
        D = np.zeros((0, self.n, self.ndim)) if dcoords is None else np.asarray(dcoords, dtype=np.float64)
        if D.ndim != 3 or D.shape[1:] != (self.n, self.ndim) or D.shape[0] > MAXGEOM:
            raise ValueError("%s: dcoords must have shape (ng, %d, %d) with 0 <= ng <= %d (MVG_MAXGEOM), got %s"
                             % (who, self.n, self.ndim, MAXGEOM, np.shape(dcoords)))
        if not np.all(np.isfinite(D)):
            raise ValueError("%s: dcoords must be finite" % who)
        if self._handle is None:
            raise ValueError("%s: the plan is closed" % who)
        ng = int(D.shape[0])
        dt = np.ascontiguousarray(D.transpose(0, 2, 1))
        G, dlogdet, dG = np.zeros((mc, mc)), np.zeros(3 + ng), np.zeros((3 + ng, mc, mc))
        logdet, info = C.c_double(0.0), C.c_int32(0)
        lib = load()
        rc = lib.mvg_plan_grad(self._handle, ct.ctypes.data_as(_dp), ng, dt.ctypes.data_as(_dp) if ng else None, MODEL_IDS[model], psill, rng,
                               nugget, wt.ctypes.data_as(_dp), mc, C.byref(logdet), G.ctypes.data_as(_dp), dlogdet.ctypes.data_as(_dp),
                               dG.ctypes.data_as(_dp), C.byref(info))
        if rc == MVG_ENOTPD:
            return math.inf, np.full((mc, mc), np.nan), np.full(3 + ng, np.nan), np.full((3 + ng, mc, mc), np.nan)
        if rc != MVG_OK:
            _raise(lib, rc)
        return float(logdet.value), G, dlogdet, dG

    def close(self):
        handle, self._handle = self._handle, None
        if handle is not None and _lib is not None:
            _lib.mvg_plan_destroy(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_plan(who, plan, n, ndim):
    if not isinstance(plan, VecchiaGradPlan):
        raise ValueError("%s: plan must be a VecchiaGradPlan, got %r" % (who, type(plan).__name__))
    if (plan.n, plan.ndim) != (n, ndim):
        raise ValueError("%s: the plan was built for (%d, %d) coordinates; these stations are (%d, %d)" % (who, plan.n, plan.ndim, n, ndim))


def neg_log_likelihood_vecchia_grad(x, y, *args, **kwargs):
    """``vecchia.neg_log_likelihood_vecchia`` and its analytic gradient, from one device call.

    ``nll, grad = neg_log_likelihood_vecchia_grad(x, y[, z], values, variogram_model, variogram_parameters, m=30, order="random", seed=0,
    plan=None, drift=None, reml=True, **anisotropy)``

    The arguments and refusals are ``neg_log_likelihood_vecchia``'s, with ``plan`` a ``VecchiaGradPlan``.  nll is what
    ``neg_log_likelihood_vecchia`` returns for the same plan arguments, bit for bit.  grad has the shapes, units and order of
    ``likelihood.neg_log_likelihood_grad``: (3 + ng,) for (N,) values and (F, 3 + ng) for (N, F) values, in natural units, in the order
    of ``GRAD_NAMES_2D`` / ``GRAD_NAMES_3D`` -- psill (the PARTIAL sill, the nugget held), range, nugget, then the constructor's
    anisotropy keywords (ng = 2 in the plane, 5 in space), angles per degree.  Field f of an (N, F) call is bit for bit the one-field
    call.  The neighbour sets are held: the gradient is that of the objective a search on one plan sees.  With
    drift='regional_linear' the gradient taken with the trend columns held is exact, as in ``neg_log_likelihood_grad``: the objective
    depends on X only through its column space.  A local system that is not positive definite in float64 gives ``inf`` and a gradient of
    NaN.  Every refusal is raised before the library is loaded; there is no CPU fallback."""
    who = "neg_log_likelihood_vecchia_grad"
    raw, n, ndim, v, many, model, par, scaling, angle, adj, X, reml, kw = _nll_arguments(who, (x, y) + args, kwargs, ("plan",) + _PLAN_NAMES)
    plan = kw.get("plan")
    dco = anisotropy_derivatives(raw, scaling, angle)
    if plan is not None:
        _check_plan(who, plan, n, ndim)
        pieces = plan.grad(adj, dco, model, par, np.hstack([v, X]))
    else:
        m, order, seed = _plan_arguments(who, kw)
        order = _order(who, order, adj, seed)
        with VecchiaGradPlan(adj, m=m, order=order) as own:
            pieces = own.grad(adj, dco, model, par, np.hstack([v, X]))
    out, grad = nll_grad_from_gram(n, *pieces, v.shape[1], reml, _pieces(X))
    return (out, grad) if many else (float(out[0]), grad[0])


def fit_variogram_vecchia_grad(x, y, *args, **kwargs):
    """Maximum-likelihood / REML fit of a bounded variogram model, and optionally of the anisotropy, under Vecchia's approximation, by a
    quasi-Newton search with the analytic gradient.

    ``fit = fit_variogram_vecchia_grad(x, y[, z], values, variogram_model, m=30, order="random", seed=0, start=None,
    fit_anisotropy=False, drift=None, reml=True, bounds=None, **anisotropy)``

    The arguments, the start (with start=None the least-squares fit on a seeded random subsample of at most 5000 stations), the search
    coordinates, the bounds and the rule of one plan built in the start metric are ``vecchia.fit_variogram_vecchia``'s.  The objective is
    minimised as ``likelihood.fit_variogram_ml(method='l-bfgs-b')`` minimises the exact one: ``scipy.optimize.minimize(method='L-BFGS-B',
    jac=True)`` on the value and the gradient of one ``VecchiaGradPlan.grad`` per evaluation, summed over the fields and taken to the
    search coordinates by the chain rule on the host; the start is a candidate too; a trial whose local systems are not positive definite
    does not raise -- the line search is told to back off; if L-BFGS-B cannot finish, the Nelder-Mead search continues from the best
    point seen and ``message`` says so.  Returns an ``MLFit``; ``nll`` is Vecchia's objective at the fit, summed over the fields, and
    ``n_evaluations`` counts the device calls of both kinds.  Argument errors are raised before the library is loaded."""
    from scipy.optimize import minimize

    who = "fit_variogram_vecchia_grad"
    fit = _Fit(who, (x, y) + args, kwargs, _FIT_NAMES, _PLAN_NAMES)
    m, order, seed = _plan_arguments(who, fit.kw)
    order = _order(who, order, fit.adj0, seed)
    fit.prepare(lambda: np.sort(np.random.default_rng(seed).permutation(fit.n)[:START_SUBSAMPLE]))
    with VecchiaGradPlan(fit.adj0, m=m, order=order) as plan:
        objective = fit.objective(lambda adj, par, W: plan.grad(adj, None, fit.model, par, W)[:2])
        nll0 = objective(fit.t0)  # the start is a candidate too: the result is never worse than it

        def value_and_gradient(t):
            """The objective and its gradient in the search coordinates: one device call."""
            par, sc, an, adj, Xt, pieces = fit.trial(t)
            dco = anisotropy_derivatives(fit.raw, sc, an) if fit.fit_anis else None
            F = fit.v.shape[1]
            nll, grad = nll_grad_from_gram(fit.n, *plan.grad(adj, dco, fit.model, par, np.hstack([fit.v, Xt])), F, fit.reml, pieces)
            # d/dlog psill, d/dlog range, d/dlog(nugget + floor), d/dlog scaling; the angles are searched in degrees
            chain = [par[0], par[1], par[2] + fit.floor] + ([float(s_) for s_ in sc] + [1.0] * len(an) if fit.fit_anis else [])
            return float(np.sum(nll)), np.sum(grad, axis=0) * np.array(chain)

        result = _fit_lbfgsb(minimize, objective, value_and_gradient, fit.t0, nll0, fit.box, fit.simplex)
    return _ml_fit(fit, *result)
