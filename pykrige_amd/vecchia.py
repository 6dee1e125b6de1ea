"""The Gaussian likelihood of a variogram model under Vecchia's approximation on the GPU: ML / REML fits past the N x N matrix.

ctypes binding of libmikvecchia.so (include/mikvecchia.h), a sixth library, loaded on first use.  NumPy + ctypes (+ scipy.optimize for the
fit).  There is no CPU fallback: a missing library or no visible GPU raises.  Every argument error is a ValueError (NotImplementedError
for a custom model) raised here, before the library is loaded.

Where ``likelihood.gram`` factors the N x N covariance matrix, a ``VecchiaPlan`` puts the stations in an order and conditions each on
its m nearest predecessors: p(v) ~ prod_i p(v_i | v_c(i)), the exact density of a Gaussian whose precision matrix is sparse.  One
evaluation is N Cholesky factorisations of size <= m + 1 and returns what ``likelihood.gram`` returns -- ``logdet`` and
``G = W^T C^-1 W`` -- so ``likelihood.nll_from_gram`` and with it the ML / REML algebra, the trend columns and the fields are reused as
they are.  For m >= N - 1 the result is the exact likelihood.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _dl
from .likelihood import MODEL_IDS, _Fit, _gram_arguments, _ml_fit, _nelder_mead, _nll_arguments, _pieces, nll_from_gram
from .likelihood import MLFit, _split, _trend  # noqa: F401 (the likelihood's own, importable from here as before)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmikvecchia.so")

MVC_OK, MVC_EINVAL, MVC_ENOTPD, MVC_EHIP = 0, -1, -2, -3
ABI_VERSION = 1  # include/mikvecchia.h MVC_ABI_VERSION
MAXNB = 64  # MVC_MAXNB
START_SUBSAMPLE = 5000  # stations of the least-squares start of fit_variogram_vecchia

_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_plan_p = C.c_void_p

# every entry point include/mikvecchia.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mvc_abi_version": (C.c_int, []),
    "mvc_last_error": (C.c_char_p, []),
    "mvc_plan_create": (C.c_int, [C.c_int, C.c_int64, C.c_int32, _dp, _i32p, C.c_int32, C.POINTER(_plan_p)]),
    "mvc_plan_neighbours": (C.c_int, [_plan_p, _i32p]),
    "mvc_plan_gram": (C.c_int, [_plan_p, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, _dp, C.c_int32, _dp, _dp, _i32p]),
    "mvc_plan_destroy": (None, [_plan_p]),
}

_lib = None


def load():
    """dlopen libmikvecchia.so and declare the signatures.  Raises ImportError if it has not been built or is stale."""
    global _lib
    if _lib is None:
        _lib = _dl.open_library(LIB_PATH, "mvc", ABI_VERSION, SIGNATURES)
    return _lib


def _raise(lib, rc):
    _dl.raise_for(lib, "mvc", "libmikvecchia", rc, MVC_EINVAL)


def _check_m(who, m):
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= MAXNB:
        raise ValueError("%s: m must be an integer in 1..%d (MVC_MAXNB), got %r" % (who, MAXNB, m))
    return int(m)


def _order(who, order, X, seed):
    """The permutation: position p holds station order[p]."""
    n = len(X)
    if isinstance(order, str):
        if order == "random":
            return np.random.default_rng(seed).permutation(n).astype(np.int32)
        if order == "coordinate":
            return np.argsort(X.sum(axis=1), kind="stable").astype(np.int32)
        raise ValueError("%s: order must be 'random', 'coordinate' or a permutation of 0 .. N - 1, got %r" % (who, order))
    o = np.asarray(order)
    if o.ndim != 1 or o.shape[0] != n or o.dtype.kind not in "iu" or not np.array_equal(np.sort(o), np.arange(n)):
        raise ValueError("%s: order must be 'random', 'coordinate' or a permutation of 0 .. N - 1 (N = %d)" % (who, n))
    return o.astype(np.int32)


class VecchiaPlan:
    """``VecchiaPlan(coords, m=30, order="random", seed=0)``: the neighbour sets of Vecchia's approximation, found on the GPU once and
    kept there for every ``gram`` that follows.

    coords: (N, 2) or (N, 3) anisotropy-adjusted Euclidean station coordinates, N >= 2.  m: the neighbour bound, 1 <= m <= 64.  order:
    'random' (``np.random.default_rng(seed).permutation(N)``), 'coordinate' (a stable argsort of the coordinate sum) or an explicit
    permutation; position p holds station ``order[p]``.  The station at position p is conditioned on its min(m, p) nearest predecessors
    by squared Euclidean distance, ties to the smaller position, listed ascending by (distance, position).

    Attributes: ``n``, ``m``, ``order`` ((N,) int32) and ``neighbours`` ((N, m) int32 station indices, row = station index, -1 beyond
    min(m, p); fetched from the device on first use).  A context manager; ``close()`` (and ``__del__``) destroy the handle.  Argument
    errors raise ValueError before the library is loaded; there is no CPU fallback."""

    def __init__(self, coords, m=30, order="random", seed=0):
        who = "VecchiaPlan"
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
        rc = lib.mvc_plan_create(_dl.device(), self.n, self.ndim, ct.ctypes.data_as(_dp), self.order.ctypes.data_as(_i32p), self.m,
                                 C.byref(handle))
        if rc != MVC_OK:
            _raise(lib, rc)
        self._handle = handle

    @property
    def neighbours(self):
        if self._neighbours is None:
            if self._handle is None:
                raise ValueError("VecchiaPlan: the plan is closed")
            out = np.empty((self.n, self.m), dtype=np.int32)
            lib = load()
            rc = lib.mvc_plan_neighbours(self._handle, out.ctypes.data_as(_i32p))
            if rc != MVC_OK:
                _raise(lib, rc)
            out.setflags(write=False)
            self._neighbours = out
        return self._neighbours

    def gram(self, coords, model, parameters, W):
        """``logdet, G = plan.gram(coords, model, parameters, W)``: log det C^ and W^T C^-1 W of Vecchia's covariance C^, one call of
        ``mvc_plan_gram``, with the conventions of ``likelihood.gram``: parameters is the internal [psill, range, nugget], W is (N,) or
        (N, m_cols) with 1 <= m_cols <= 40, G is exactly symmetric, both results are the same bits from run to run and an entry of G
        depends only on its two columns.  coords may differ from the plan's -- a search that moves the anisotropy: the neighbour sets
        stay those of the plan's metric.  If a local system is not positive definite in float64, logdet is ``inf`` and G is NaN."""
        who = "VecchiaPlan.gram"
        _, _, psill, rng, nugget, mc, ct, wt = _gram_arguments(who, coords, model, parameters, W, "MVC_MAXCOLS", (self.n, self.ndim))
        if self._handle is None:
            raise ValueError("%s: the plan is closed" % who)
        G = np.zeros((mc, mc))
        logdet, info = C.c_double(0.0), C.c_int32(0)
        lib = load()
        rc = lib.mvc_plan_gram(self._handle, ct.ctypes.data_as(_dp), MODEL_IDS[model], psill, rng, nugget, wt.ctypes.data_as(_dp), mc,
                               C.byref(logdet), G.ctypes.data_as(_dp), C.byref(info))
        if rc == MVC_ENOTPD:
            return math.inf, np.full((mc, mc), np.nan)
        if rc != MVC_OK:
            _raise(lib, rc)
        return float(logdet.value), G

    def close(self):
        handle, self._handle = self._handle, None
        if handle is not None and _lib is not None:
            _lib.mvc_plan_destroy(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _plan_arguments(who, kw):
    m = _check_m(who, kw.get("m", 30))
    order = kw.get("order", "random")
    if isinstance(order, str) and order not in ("random", "coordinate"):
        raise ValueError("%s: order must be 'random', 'coordinate' or a permutation of 0 .. N - 1, got %r" % (who, order))
    seed = kw.get("seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("%s: seed must be a non-negative integer, got %r" % (who, seed))
    return m, order, int(seed)


def _check_plan(who, plan, n, ndim):
    if not isinstance(plan, VecchiaPlan):
        raise ValueError("%s: plan must be a VecchiaPlan, got %r" % (who, type(plan).__name__))
    if (plan.n, plan.ndim) != (n, ndim):
        raise ValueError("%s: the plan was built for (%d, %d) coordinates; these stations are (%d, %d)" % (who, plan.n, plan.ndim, n, ndim))


_PLAN_NAMES = ("m", "order", "seed")


def neg_log_likelihood_vecchia(x, y, *args, **kwargs):
    """The negative Gaussian log-likelihood of the stations under a variogram model in Vecchia's approximation: N small Cholesky
    factorisations on the GPU in place of one of size N.

    ``neg_log_likelihood_vecchia(x, y[, z], values, variogram_model, variogram_parameters, m=30, order="random", seed=0, plan=None,
    drift=None, reml=True, **anisotropy)``

    The arguments, shapes, refusals and formulas are those of ``likelihood.neg_log_likelihood``, with log det C and W^T C^-1 W
    replaced by those of Vecchia's covariance (``VecchiaPlan.gram``).  m, order and seed are ``VecchiaPlan``'s; without ``plan`` one
    plan is built in the call's adjusted metric and dropped, with ``plan`` (a ``VecchiaPlan`` of the same stations) its neighbour
    sets are used and m, order and seed are ignored.  Returns a float for (N,) values or (F,) for (N, F) values; field f of an (N, F)
    call is bit for bit the one-field call on the same plan.  With m >= N - 1 the value is the exact likelihood.  A local system that
    is not positive definite in float64 gives ``inf``.  Every refusal is raised before the library is loaded; there is no CPU
    fallback."""
    who = "neg_log_likelihood_vecchia"
    _, n, ndim, v, many, model, par, _, _, adj, X, reml, kw = _nll_arguments(who, (x, y) + args, kwargs, ("plan",) + _PLAN_NAMES)
    plan = kw.get("plan")
    if plan is not None:
        _check_plan(who, plan, n, ndim)
        logdet, G = plan.gram(adj, model, par, np.hstack([v, X]))
    else:
        m, order, seed = _plan_arguments(who, kw)
        order = _order(who, order, adj, seed)
        with VecchiaPlan(adj, m=m, order=order) as own:
            logdet, G = own.gram(adj, model, par, np.hstack([v, X]))
    out = nll_from_gram(n, logdet, G, v.shape[1], reml, _pieces(X))
    return out if many else float(out[0])


_FIT_NAMES = ("variogram_model", "start", "fit_anisotropy", "drift", "reml", "bounds")


def fit_variogram_vecchia(x, y, *args, **kwargs):
    """Maximum-likelihood / REML fit of a bounded variogram model, and optionally of the anisotropy, under Vecchia's approximation.

    ``fit = fit_variogram_vecchia(x, y[, z], values, variogram_model, m=30, order="random", seed=0, start=None, fit_anisotropy=False,
    drift=None, reml=True, bounds=None, **anisotropy)``

    Minimises ``neg_log_likelihood_vecchia`` as ``likelihood.fit_variogram_ml`` minimises the exact objective: the same search
    coordinates (log psill, log range, log(nugget + floor), with fit_anisotropy the log scalings and the angles), the same bounds and
    floors, the same two-pass Nelder-Mead search with the same tolerances, and the start as a candidate.  One plan, built in the start
    metric, serves the whole search: the neighbour sets stay those of the start's anisotropy while the covariances follow the trial's.
    One device call per evaluation.  With start=None the least-squares start is fitted on a seeded random subsample of at most 5000
    stations (``np.random.default_rng(seed)``), not on the binned variogram of all pairs.  There is no gradient method: the objective has
    no analytic gradient in this library, and ``method`` is not an argument.  A trial whose local systems are not positive definite
    (``inf``) does not raise.  Returns an ``MLFit``; ``nll`` is Vecchia's objective at the fit, summed over the fields.  Argument errors
    are raised before the library is loaded."""
    from scipy.optimize import minimize

    who = "fit_variogram_vecchia"
    fit = _Fit(who, (x, y) + args, kwargs, _FIT_NAMES, _PLAN_NAMES)
    m, order, seed = _plan_arguments(who, fit.kw)
    order = _order(who, order, fit.adj0, seed)
    fit.prepare(lambda: np.sort(np.random.default_rng(seed).permutation(fit.n)[:START_SUBSAMPLE]))
    with VecchiaPlan(fit.adj0, m=m, order=order) as plan:
        objective = fit.objective(lambda adj, par, W: plan.gram(adj, fit.model, par, W))
        nll0 = objective(fit.t0)  # the start is a candidate too: the result is never worse than it
        result = _nelder_mead(minimize, objective, fit, nll0)
    return _ml_fit(fit, *result)
