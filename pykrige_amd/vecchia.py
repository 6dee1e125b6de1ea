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

from .likelihood import (MODEL_IDS, MLFit, _adjust, _anisotropy, _check_model, _fields, _internal_parameters, _pieces, _split, _trend,
                         nll_from_gram)
from .likelihood import _ANIS2, _ANIS3, MAXCOLS, NUGGET_FLOOR

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
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "pykrige_amd: %s is missing -- build it with `python -m pykrige_amd.build` "
            "(needs hipcc; there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    have = getattr(lib, "mvc_abi_version", None)
    version = None
    if have is not None:
        have.restype, have.argtypes = SIGNATURES["mvc_abi_version"]
        version = have()
    stale = "pykrige_amd: %s %%s, this package was written against ABI version %d -- rebuild it (`python -m pykrige_amd.build --force`)" % (
        LIB_PATH, ABI_VERSION)
    if version != ABI_VERSION:
        raise ImportError(stale % ("has no mvc_abi_version" if version is None else "has ABI version %d" % version))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(stale % ("does not export %s" % name)) from None
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _device():
    return int(os.environ.get("MIK_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def _raise(lib, rc):
    msg = (lib.mvc_last_error() or b"").decode("utf-8", "replace")
    if rc == MVC_EINVAL:
        raise ValueError(msg)
    raise RuntimeError("libmikvecchia: %s (code %d)" % (msg, rc))


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
        rc = lib.mvc_plan_create(_device(), self.n, self.ndim, ct.ctypes.data_as(_dp), self.order.ctypes.data_as(_i32p), self.m,
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
        _check_model(who, model)
        X = np.asarray(coords, dtype=np.float64)
        if X.shape != (self.n, self.ndim):
            raise ValueError("%s: coords must have the plan's shape (%d, %d), got %s" % (who, self.n, self.ndim, np.shape(coords)))
        try:
            psill, rng, nugget = (float(v) for v in parameters)
        except (TypeError, ValueError):
            raise ValueError("%s: parameters must be the three numbers [psill, range, nugget]" % who) from None
        if not (math.isfinite(psill) and math.isfinite(rng) and math.isfinite(nugget) and psill > 0.0 and rng > 0.0 and nugget >= 0.0):
            raise ValueError("%s: need finite psill > 0, range > 0 and nugget >= 0, got %r" % (who, [psill, rng, nugget]))
        Wa = np.asarray(W, dtype=np.float64)
        if Wa.ndim == 1:
            Wa = Wa[:, None]
        if Wa.ndim != 2 or Wa.shape[0] != self.n or not 1 <= Wa.shape[1] <= MAXCOLS:
            raise ValueError("%s: W must have shape (N,) or (N, m) with N = %d stations and 1 <= m <= %d columns (MVC_MAXCOLS), got %s"
                             % (who, self.n, MAXCOLS, np.shape(W)))
        if not np.all(np.isfinite(X)):
            raise ValueError("%s: station coordinates must be finite" % who)
        if not np.all(np.isfinite(Wa)):
            raise ValueError("%s: W must be finite" % who)
        if self._handle is None:
            raise ValueError("%s: the plan is closed" % who)
        mc = int(Wa.shape[1])
        ct, wt = np.ascontiguousarray(X.T), np.ascontiguousarray(Wa.T)
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


_NLL_NAMES = ("variogram_model", "variogram_parameters")
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
    raw, values, kw = _split(who, (x, y) + args, dict(kwargs), _NLL_NAMES)
    unknown = set(kw) - set(_NLL_NAMES) - set(_ANIS2) - set(_ANIS3) - {"drift", "reml", "plan"} - set(_PLAN_NAMES)
    if unknown:
        raise TypeError("%s: unexpected argument %s" % (who, ", ".join(sorted(unknown))))
    if "variogram_model" not in kw:
        raise TypeError("%s: variogram_model is required" % who)
    model = kw["variogram_model"]
    _check_model(who, model)
    n, ndim = raw.shape
    if n < 2:
        raise ValueError("%s: need at least two stations" % who)
    if not np.all(np.isfinite(raw)):
        raise ValueError("%s: station coordinates must be finite" % who)
    v, many = _fields(who, values, n)
    par = _internal_parameters(who, model, kw.get("variogram_parameters"))
    scaling, angle = _anisotropy(who, ndim, kw)
    adj = _adjust(raw, scaling, angle)
    X = _trend(who, kw.get("drift"), n, adj)
    reml = bool(kw.get("reml", True))
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
    raw, values, kw = _split(who, (x, y) + args, dict(kwargs), _FIT_NAMES)
    unknown = set(kw) - set(_FIT_NAMES) - set(_ANIS2) - set(_ANIS3) - set(_PLAN_NAMES)
    if unknown:
        raise TypeError("%s: unexpected argument %s" % (who, ", ".join(sorted(unknown))))
    if "variogram_model" not in kw:
        raise TypeError("%s: variogram_model is required" % who)
    model = kw["variogram_model"]
    _check_model(who, model)
    n, ndim = raw.shape
    if n < 2:
        raise ValueError("%s: need at least two stations" % who)
    if not np.all(np.isfinite(raw)):
        raise ValueError("%s: station coordinates must be finite" % who)
    v, _ = _fields(who, values, n)
    scaling0, angle0 = _anisotropy(who, ndim, kw)
    drift = kw.get("drift")
    adj0 = _adjust(raw, scaling0, angle0)
    X = _trend(who, drift, n, adj0)
    reml = bool(kw.get("reml", True))
    fit_anis = bool(kw.get("fit_anisotropy", False))
    m, order, seed = _plan_arguments(who, kw)
    order = _order(who, order, adj0, seed)
    var = float(np.var(v))
    if not var > 0.0:
        raise ValueError("%s: the values are constant; there is no variogram to fit" % who)
    diag = float(np.sqrt(np.sum((raw.max(axis=0) - raw.min(axis=0)) ** 2)))
    if not diag > 0.0:
        raise ValueError("%s: all stations coincide" % who)
    floor = NUGGET_FLOOR * var
    lim = {"psill": (1e-6 * var, 100.0 * var), "range": (1e-3 * diag, 10.0 * diag), "nugget": (0.0, 100.0 * var), "scaling": (0.05, 20.0)}
    given = kw.get("bounds")
    if given is not None:
        if not isinstance(given, dict) or set(given) - set(lim):
            raise ValueError("%s: bounds must be a dict with keys among 'psill', 'range', 'nugget', 'scaling'" % who)
        for k, (lo, hi) in given.items():
            lo, hi = float(lo), float(hi)
            if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi and (lo > 0.0 or (k == "nugget" and lo >= 0.0))):
                raise ValueError("%s: bounds[%r] must be (low, high) with 0 < low < high (nugget: 0 <= low)" % (who, k))
            lim[k] = (lo, hi)
    start = kw.get("start")
    if start is None:
        from . import variogram_fit

        pick = np.sort(np.random.default_rng(seed).permutation(n)[:START_SUBSAMPLE])
        _, _, par0 = variogram_fit.fit(adj0[pick], v[pick, 0], model, 6, False, "euclidean")
        par0 = [float(t) for t in par0]
    else:
        par0 = _internal_parameters(who, model, start)
    clip = lambda t, k: min(max(t, lim[k][0]), lim[k][1])
    par0 = [clip(par0[0], "psill"), clip(par0[1], "range"), clip(par0[2], "nugget")]
    pieces = _pieces(X)
    moving = isinstance(drift, str) and fit_anis  # the trend columns are the adjusted coordinates: they move with the anisotropy
    nscale = len(scaling0)

    def unpack(t):
        par = [math.exp(t[0]), math.exp(t[1]), max(math.exp(t[2]) - floor, 0.0)]
        if fit_anis:
            return par, [math.exp(s) for s in t[3:3 + nscale]], [float(a) for a in t[3 + nscale:]]
        return par, scaling0, angle0

    calls = [0]
    with VecchiaPlan(adj0, m=m, order=order) as plan:

        def objective(t):
            par, sc, an = unpack(t)
            calls[0] += 1
            adj = _adjust(raw, sc, an)
            Xt = np.hstack([np.ones((n, 1)), adj]) if moving else X
            logdet, G = plan.gram(adj, model, par, np.hstack([v, Xt]))
            return float(np.sum(nll_from_gram(n, logdet, G, v.shape[1], reml, _pieces(Xt) if moving else pieces)))

        t0 = [math.log(par0[0]), math.log(par0[1]), math.log(par0[2] + floor)]
        box = [tuple(math.log(b) for b in lim["psill"]), tuple(math.log(b) for b in lim["range"]),
               (math.log(lim["nugget"][0] + floor), math.log(lim["nugget"][1] + floor))]
        step = [0.4, 0.4, 0.6]
        if fit_anis:
            t0 += [math.log(clip(s, "scaling")) for s in scaling0] + list(angle0)
            box += [tuple(math.log(b) for b in lim["scaling"])] * nscale + [(None, None)] * len(angle0)
            step += [0.35] * nscale + [25.0] * len(angle0)
        t0 = np.array(t0)
        nll0 = objective(t0)  # the start is a candidate too: the result is never worse than it

        def simplex(c, scale):
            pts = [np.array(c)]
            for k, s in enumerate(step):
                q = np.array(c)
                q[k] += s * scale if box[k][1] is None or q[k] + s * scale <= box[k][1] else -s * scale
                pts.append(q)
            return np.array(pts)

        best_t, best = t0, nll0
        converged, message = False, ""
        for scale in (1.0, 0.5):  # the search, and one restart from its result
            res = minimize(objective, best_t, method="Nelder-Mead", bounds=box,
                           options=dict(initial_simplex=simplex(best_t, scale), xatol=1e-3, fatol=1e-6, maxfev=200 * len(t0)))
            converged, message = converged or bool(res.success), str(res.message)
            if res.fun < best:
                best_t, best = np.array(res.x), float(res.fun)
    par, sc, an = unpack(best_t)
    names = _ANIS2 if ndim == 2 else _ANIS3
    anis = dict(zip(names, list(sc) + list(an)))
    return MLFit(model, [par[0] + par[2], par[1], par[2]], anis, best, calls[0], bool(converged and math.isfinite(best)), message, reml)
