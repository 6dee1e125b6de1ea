"""The Gaussian likelihood of a variogram model on the GPU: maximum likelihood and restricted maximum likelihood (REML) fits of psill,
range, nugget and the anisotropy, binning-free.

ctypes binding of libmiklik.so (include/miklik.h), a fourth library beside libmikrige.so, libmikvario.so and libmikvario3.so, loaded on
first use.  NumPy + ctypes (+ scipy.optimize for the fit).  There is no CPU fallback: a missing library or no visible GPU raises.  Every
argument error is a ValueError (NotImplementedError for a custom model) raised here, before the library is loaded.

One evaluation is one device call: the N x N covariance matrix C of the stations is assembled, Cholesky-factored and thrown away;
``logdet = log det C`` and ``G = W^T C^-1 W`` for a handful of columns W come back.  With W = [V | X] (fields and trend columns) the small
algebra of the likelihood is NumPy's.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _dl, core

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmiklik.so")

MLK_OK, MLK_EINVAL, MLK_ENOTPD, MLK_EHIP = 0, -1, -2, -3
ABI_VERSION = 1  # include/miklik.h MLK_ABI_VERSION
MAXCOLS, MAXFIELDS, MAXTREND = 40, 32, 8  # MLK_MAXCOLS = MAXFIELDS + MAXTREND
MODEL_IDS = {"gaussian": 0, "exponential": 1, "spherical": 2, "hole-effect": 3}  # MLK_GAUSSIAN ...

_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)

# every entry point include/miklik.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mlk_abi_version": (C.c_int, []),
    "mlk_last_error": (C.c_char_p, []),
    "mlk_gram": (C.c_int, [C.c_int, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, _dp, C.c_int32, _dp, _dp,
                           _i32p]),
}

_lib = None


def load():
    """dlopen libmiklik.so and declare the signatures.  Raises ImportError if it has not been built or is stale."""
    global _lib
    if _lib is None:
        _lib = _dl.open_library(LIB_PATH, "mlk", ABI_VERSION, SIGNATURES)
    return _lib


def _check_model(who, model):
    if model == "custom" or callable(model) or hasattr(model, "pykrige_kwargs"):
        raise NotImplementedError("%s: variogram_model='custom' is evaluated on the host; the likelihood needs a covariance the device can "
                                  "evaluate" % who)
    if model in ("linear", "power"):
        raise ValueError("%s: the '%s' variogram is unbounded -- no covariance exists; use one of %s"
                         % (who, model, ", ".join(repr(k) for k in MODEL_IDS)))
    if model not in MODEL_IDS:
        raise ValueError("%s: variogram_model must be one of %s, got %r" % (who, ", ".join(repr(k) for k in MODEL_IDS), model))


def _gram_arguments(who, coords, model, parameters, W, macro, plan_shape=None):
    """The checks ``gram`` and ``VecchiaPlan.gram`` share -> n, ndim, psill, range, nugget, m and the transposed contiguous coordinates and
    columns.  ``macro`` is the library's name for the column bound; with ``plan_shape`` the coordinates must have that (N, ndim)."""
    _check_model(who, model)
    X = np.asarray(coords, dtype=np.float64)
    if plan_shape is not None:
        if X.shape != plan_shape:
            raise ValueError("%s: coords must have the plan's shape (%d, %d), got %s" % ((who,) + plan_shape + (np.shape(coords),)))
    elif X.ndim != 2 or X.shape[1] not in (2, 3):
        raise ValueError("%s: coords must have shape (N, 2) or (N, 3), got %s" % (who, np.shape(coords)))
    n, ndim = X.shape
    if n < 2:
        raise ValueError("%s: need at least two stations" % who)
    try:
        psill, rng, nugget = (float(v) for v in parameters)
    except (TypeError, ValueError):
        raise ValueError("%s: parameters must be the three numbers [psill, range, nugget]" % who) from None
    if not (math.isfinite(psill) and math.isfinite(rng) and math.isfinite(nugget) and psill > 0.0 and rng > 0.0 and nugget >= 0.0):
        raise ValueError("%s: need finite psill > 0, range > 0 and nugget >= 0, got %r" % (who, [psill, rng, nugget]))
    Wa = np.asarray(W, dtype=np.float64)
    if Wa.ndim == 1:
        Wa = Wa[:, None]
    if Wa.ndim != 2 or Wa.shape[0] != n or not 1 <= Wa.shape[1] <= MAXCOLS:
        raise ValueError("%s: W must have shape (N,) or (N, m) with N = %d stations and 1 <= m <= %d columns (%s), got %s"
                         % (who, n, MAXCOLS, macro, np.shape(W)))
    if not np.all(np.isfinite(X)):
        raise ValueError("%s: station coordinates must be finite" % who)
    if not np.all(np.isfinite(Wa)):
        raise ValueError("%s: W must be finite" % who)
    return n, ndim, psill, rng, nugget, int(Wa.shape[1]), np.ascontiguousarray(X.T), np.ascontiguousarray(Wa.T)


def gram(coords, model, parameters, W):
    """``logdet, G = gram(coords, model, parameters, W)``: log det C and W^T C^-1 W on the GPU, one call of ``mlk_gram``.

    coords: (N, 2) or (N, 3) anisotropy-adjusted Euclidean station coordinates, N >= 2.  model: 'gaussian', 'exponential', 'spherical' or
    'hole-effect'.  parameters: the internal list [psill, range, nugget] (partial sill), psill > 0, range > 0, nugget >= 0.  W: (N,) or
    (N, m) columns, 1 <= m <= 40.

    C_ii = psill + nugget and, for i != j, C_ij = (psill + nugget) - gamma(d_ij) with the model formula of ``core.variogram_value`` in
    float64 -- also at d = 0: two coincident distinct stations have C_ij = psill.  G is (m, m) and exactly symmetric.  Both results are
    reproducible bit for bit from run to run, and an entry of G does not depend on where its two columns stand in W.  If C is not
    positive definite in float64, logdet is ``inf`` and G is filled with NaN.  Argument errors raise ValueError before the library is
    loaded; there is no CPU fallback."""
    n, ndim, psill, rng, nugget, m, ct, wt = _gram_arguments("gram", coords, model, parameters, W, "MLK_MAXCOLS")
    G = np.zeros((m, m))
    logdet = C.c_double(0.0)
    info = C.c_int32(0)
    lib = load()
    rc = lib.mlk_gram(_dl.device(), n, ndim, ct.ctypes.data_as(_dp), MODEL_IDS[model], psill, rng, nugget, wt.ctypes.data_as(_dp), m,
                      C.byref(logdet), G.ctypes.data_as(_dp), C.byref(info))
    if rc == MLK_ENOTPD:
        return math.inf, np.full((m, m), np.nan)
    if rc != MLK_OK:
        _dl.raise_for(lib, "mlk", "libmiklik", rc, MLK_EINVAL)
    return float(logdet.value), G


# ------------------------------------------------------------------------------------------------------------- the likelihood
_ANIS2 = ("anisotropy_scaling", "anisotropy_angle")
_ANIS3 = ("anisotropy_scaling_y", "anisotropy_scaling_z", "anisotropy_angle_x", "anisotropy_angle_y", "anisotropy_angle_z")


def _split(who, args, kw, names):
    """(x, y[, z], values, *rest) -> raw (N, d) coordinates, the values and the remaining named arguments: the first string among the
    positional arguments is the variogram model, which tells 2-D from 3-D."""
    args = list(args)
    at = next((k for k, a in enumerate(args) if isinstance(a, str) or hasattr(a, "pykrige_kwargs")), len(args))
    if at < len(args):
        for name, a in zip(names, args[at:]):
            if name in kw:
                raise TypeError("%s: %s given twice" % (who, name))
            kw[name] = a
        if len(args) - at > len(names):
            raise TypeError("%s: too many positional arguments" % who)
        args = args[:at]
    if len(args) not in (3, 4):
        raise TypeError("%s: the leading arguments are x, y, values or x, y, z, values" % who)
    cols = [np.atleast_1d(np.squeeze(np.asarray(a, dtype=np.float64))) for a in args[:-1]]
    if any(c.ndim != 1 or c.shape != cols[0].shape for c in cols):
        raise ValueError("%s: x, y%s must be one-dimensional arrays of the same length" % (who, " and z" if len(cols) == 3 else ""))
    return np.vstack(cols).T, args[-1], kw


def _fields(who, values, n):
    v = np.asarray(values, dtype=np.float64)
    many = v.ndim == 2
    if v.ndim == 1:
        v = v[:, None]
    if v.ndim != 2 or v.shape[0] != n or not 1 <= v.shape[1] <= MAXFIELDS:
        raise ValueError("%s: values must have shape (N,) or (N, F) with N = %d stations and 1 <= F <= %d fields, got %s"
                         % (who, n, MAXFIELDS, np.shape(values)))
    if not np.all(np.isfinite(v)):
        raise ValueError("%s: values must be finite" % who)
    return v, many


def _anisotropy(who, ndim, kw):
    """The constructor's anisotropy arguments of this dimension -> (scaling list, angle list)."""
    own, other = (_ANIS2, _ANIS3) if ndim == 2 else (_ANIS3, _ANIS2)
    for name in other:
        if kw.get(name) is not None:
            raise ValueError("%s: %s is an argument of the %s classes; these are %d-D stations" % (who, name, "3-D" if ndim == 2 else "2-D",
                                                                                                   ndim))
    vals = [float(kw[name]) if kw.get(name) is not None else (1.0 if "scaling" in name else 0.0) for name in own]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("%s: the anisotropy arguments must be finite" % who)
    nscale = 1 if ndim == 2 else 2
    if not all(v > 0.0 for v in vals[:nscale]):
        raise ValueError("%s: an anisotropy scaling must be positive" % who)
    return vals[:nscale], vals[nscale:]


def _adjust(raw, scaling, angle):
    """core.adjust_for_anisotropy about the constructor's centre: the middle of the bounding box."""
    center = [(float(np.amax(c)) + float(np.amin(c))) / 2.0 for c in raw.T]
    return core.adjust_for_anisotropy(raw, center, scaling, angle)


def _trend(who, drift, n, adjusted):
    """X = [1 | drift]: (N, p), p = 1 + q <= 8, of full column rank.  drift='regional_linear': the adjusted coordinates, the trend of
    the universal classes' regional_linear term."""
    X = np.ones((n, 1))
    if isinstance(drift, str):
        if drift != "regional_linear":
            raise ValueError("%s: drift must be None, an (N, q) array or 'regional_linear', got %r" % (who, drift))
        X = np.hstack([X, adjusted])
    elif drift is not None:
        d = np.asarray(drift, dtype=np.float64)
        if d.ndim == 1:
            d = d[:, None]
        if d.ndim != 2 or d.shape[0] != n:
            raise ValueError("%s: drift must have shape (N, q) with N = %d stations, got %s" % (who, n, np.shape(drift)))
        if not np.all(np.isfinite(d)):
            raise ValueError("%s: drift must be finite" % who)
        X = np.hstack([X, d])
    p = X.shape[1]
    if p > MAXTREND:
        raise ValueError("%s: at most %d trend columns, the ones column included (p = 1 + q <= %d), got %d" % (who, MAXTREND, MAXTREND, p))
    if p > n or np.linalg.matrix_rank(X) < p:
        raise ValueError("%s: the trend matrix X = [1 | drift] is rank-deficient" % who)
    return X


def _pieces(X):
    """log det(X^T X), from the Cholesky factor of the p x p matrix."""
    return 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(X.T @ X)))))


def nll_from_gram(n, logdet, G, nfields, reml, logdet_xtx):
    """The negative log-likelihoods of nfields fields from ``logdet`` and ``G = W^T C^-1 W`` of W = [V | X]: with
    beta_f = G_xx^-1 G_xv[:, f] and Q_f = G_vv[f, f] - G_xv[:, f]^T beta_f,
    ML: 1/2 [N log 2 pi + logdet + Q_f];  REML: 1/2 [(N - p) log 2 pi - log det(X^T X) + logdet + log det G_xx + Q_f].
    Each field is worked on its own, so that a field's number does not depend on the fields beside it.  (F,) float64; inf where C or
    G_xx is not positive definite."""
    F = int(nfields)
    out = np.full(F, np.inf)
    if not math.isfinite(logdet) or not np.all(np.isfinite(G)):
        return out
    Gxx = G[F:, F:]
    p = Gxx.shape[0]
    try:
        Lx = np.linalg.cholesky(Gxx)
    except np.linalg.LinAlgError:
        return out
    logdet_gxx = 2.0 * float(np.sum(np.log(np.diag(Lx))))
    for f in range(F):
        g = np.ascontiguousarray(G[F:, f])
        y = np.zeros(p)  # forward substitution Lx y = g, one field at a time
        for i in range(p):
            y[i] = (g[i] - float(np.dot(Lx[i, :i], y[:i]))) / Lx[i, i]
        q = float(G[f, f]) - float(np.dot(y, y))
        if reml:
            out[f] = 0.5 * ((n - p) * math.log(2.0 * math.pi) - logdet_xtx + logdet + logdet_gxx + q)
        else:
            out[f] = 0.5 * (n * math.log(2.0 * math.pi) + logdet + q)
    return out


def nll_grad_from_gram(n, logdet, G, dlogdet, dG, nfields, reml, logdet_xtx):
    """``nll, grad = nll_grad_from_gram(n, logdet, G, dlogdet, dG, nfields, reml, logdet_xtx)``: the negative log-likelihoods of
    ``nll_from_gram`` -- its bits: it is called -- and their derivatives from ``dlogdet`` (K,) and ``dG`` (K, m, m), the derivatives of
    ``logdet`` and ``G`` with respect to K parameters of the covariance, X held fixed.  The chain rule through the ML / REML algebra in
    float64: with beta_f = G_xx^-1 G_xv[:, f],
    dQ_f = dG_vv[f, f] - 2 dG_xv[:, f]^T beta_f + beta_f^T dG_xx beta_f,
    ML: 1/2 [dlogdet + dQ_f];  REML: 1/2 [dlogdet + tr(G_xx^-1 dG_xx) + dQ_f].
    grad is (F, K); each field is worked on its own.  Where ``nll_from_gram`` gives inf -- C or G_xx not positive definite -- nll is inf
    and grad NaN."""
    F = int(nfields)
    nll = nll_from_gram(n, logdet, G, F, reml, logdet_xtx)
    dlogdet, dG = np.asarray(dlogdet, dtype=np.float64), np.asarray(dG, dtype=np.float64)
    K = dlogdet.shape[0]
    grad = np.full((F, K), np.nan)
    if not np.all(np.isfinite(nll)) or not (np.all(np.isfinite(dlogdet)) and np.all(np.isfinite(dG))):
        return np.full(F, np.inf), grad
    Li = np.linalg.inv(np.linalg.cholesky(G[F:, F:]))
    Gi = Li.T @ Li
    trace = [float(np.sum(Gi * dG[k][F:, F:])) if reml else 0.0 for k in range(K)]
    for f in range(F):
        beta = Gi @ np.ascontiguousarray(G[F:, f])
        for k in range(K):
            dq = float(dG[k][f, f]) - 2.0 * float(np.dot(np.ascontiguousarray(dG[k][F:, f]), beta)) + float(beta @ (dG[k][F:, F:] @ beta))
            grad[f, k] = 0.5 * (float(dlogdet[k]) + trace[k] + dq)
    return nll, grad


def _internal_parameters(who, model, variogram_parameters):
    if variogram_parameters is None:
        raise ValueError("%s: variogram_parameters must be given (a list [sill, range, nugget] or a dict)" % who)
    plist = core.make_variogram_parameter_list(model, variogram_parameters if type(variogram_parameters) in (list, dict)
                                               else list(variogram_parameters))
    psill, rng, nugget = (float(v) for v in plist)
    if not (math.isfinite(psill) and math.isfinite(rng) and math.isfinite(nugget) and psill > 0.0 and rng > 0.0 and nugget >= 0.0):
        raise ValueError("%s: need a finite partial sill > 0 (sill - nugget), range > 0 and nugget >= 0, got psill = %r, range = %r, "
                         "nugget = %r" % (who, psill, rng, nugget))
    return [psill, rng, nugget]


_NLL_NAMES = ("variogram_model", "variogram_parameters")


def _station_arguments(who, args, kwargs, names, accepted):
    """The leading checks of the likelihoods and the fits -> raw coordinates, n, ndim, the fields (N, F), whether they came as (N, F),
    the model and the named arguments.  ``names`` may be given by position after the values; ``accepted`` are the further keywords."""
    raw, values, kw = _split(who, args, dict(kwargs), names)
    unknown = set(kw) - set(names) - set(_ANIS2) - set(_ANIS3) - set(accepted)
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
    return raw, n, ndim, v, many, model, kw


def _nll_arguments(who, args, kwargs, extra=()):
    """The arguments of ``neg_log_likelihood`` and its kin, checked in their order -> raw coordinates, n, ndim, the fields, whether
    they came as (N, F), the model, the internal parameters, the anisotropy scaling and angle, the adjusted coordinates, the trend
    matrix X, reml and the named arguments (``extra``: the keywords accepted beside drift and reml)."""
    raw, n, ndim, v, many, model, kw = _station_arguments(who, args, kwargs, _NLL_NAMES, ("drift", "reml") + tuple(extra))
    par = _internal_parameters(who, model, kw.get("variogram_parameters"))
    scaling, angle = _anisotropy(who, ndim, kw)
    adj = _adjust(raw, scaling, angle)
    X = _trend(who, kw.get("drift"), n, adj)
    return raw, n, ndim, v, many, model, par, scaling, angle, adj, X, bool(kw.get("reml", True)), kw


def neg_log_likelihood(x, y, *args, **kwargs):
    """The negative Gaussian log-likelihood of the stations under a variogram model, one Cholesky factorisation on the GPU.

    ``neg_log_likelihood(x, y[, z], values, variogram_model, variogram_parameters, anisotropy_scaling=1.0, anisotropy_angle=0.0,
    drift=None, reml=True)`` -- for 3-D stations the anisotropy arguments are ``anisotropy_scaling_y, anisotropy_scaling_z,
    anisotropy_angle_x, anisotropy_angle_y, anisotropy_angle_z``, as in the constructors.

    Returns a float for (N,) values, or (F,) for (N, F) values with F <= 32: all F fields ride as columns of W through the one
    factorisation, and field f's number is bit for bit that of the one-field call.  variogram_parameters takes the forms of the
    constructors: a list [sill, range, nugget] with the FULL sill, or a dict.  The coordinates are adjusted on the host by
    ``core.adjust_for_anisotropy`` about the constructor's centre (the middle of the bounding box).  drift is None -- a constant mean,
    X = 1 -- or an (N, q) array whose columns follow the ones column, p = 1 + q <= 8, or 'regional_linear': the adjusted coordinates
    (the regional_linear term of the universal classes).

    With W = [V | X], G = W^T C^-1 W, beta_f = G_xx^-1 G_xv[:, f] and Q_f = G_vv[f, f] - G_xv[:, f]^T beta_f (the generalised
    least-squares residual sum of squares):
    ML (reml=False): 1/2 [N log 2 pi + log det C + Q_f];
    REML (reml=True): 1/2 [(N - p) log 2 pi - log det(X^T X) + log det C + log det G_xx + Q_f].
    A covariance matrix that is not positive definite in float64 gives ``inf``.  'linear' and 'power' (unbounded: no covariance exists)
    and non-finite input raise ValueError, a rank-deficient X raises ValueError, 'custom' raises NotImplementedError -- all before the
    library is loaded.  There is no CPU fallback."""
    raw, n, ndim, v, many, model, par, scaling, angle, adj, X, reml, kw = _nll_arguments("neg_log_likelihood", (x, y) + args, kwargs)
    logdet, G = gram(adj, model, par, np.hstack([v, X]))
    out = nll_from_gram(n, logdet, G, v.shape[1], reml, _pieces(X))
    return out if many else float(out[0])


class MLFit:
    """What ``fit_variogram_ml`` returns.  ``variogram_parameters`` is the constructor's list form [sill, range, nugget] (FULL sill) and
    ``anisotropy`` the constructor's anisotropy keywords, so ``OrdinaryKriging(x, y, v, variogram_model=fit.variogram_model,
    variogram_parameters=fit.variogram_parameters, **fit.anisotropy)`` kriges with the fit.  ``nll`` is the objective at the fit (summed
    over the fields of (N, F) values), ``n_evaluations`` the device calls spent, ``success`` and ``message`` the optimiser's."""

    def __init__(self, variogram_model, variogram_parameters, anisotropy, nll, n_evaluations, success, message, reml):
        self.variogram_model = variogram_model
        self.variogram_parameters = variogram_parameters
        self.anisotropy = anisotropy
        for k, val in anisotropy.items():
            setattr(self, k, val)
        self.nll = nll
        self.n_evaluations = n_evaluations
        self.success = success
        self.message = message
        self.reml = reml

    def __repr__(self):
        return "MLFit(variogram_model=%r, variogram_parameters=%r, anisotropy=%r, nll=%r, n_evaluations=%d, success=%r)" % (
            self.variogram_model, self.variogram_parameters, self.anisotropy, self.nll, self.n_evaluations, self.success)


_FIT_NAMES = ("variogram_model", "start", "fit_anisotropy", "drift", "reml", "bounds", "method")
FIT_METHODS = ("nelder-mead", "l-bfgs-b")
NUGGET_FLOOR = 1e-8  # times the variance of the values: the nugget is searched as log(nugget + floor), so that zero is a reachable bound


def fit_variogram_ml(x, y, *args, **kwargs):
    """Maximum-likelihood / REML fit of a bounded variogram model, and optionally of the anisotropy, to the stations -- binning-free.

    ``fit = fit_variogram_ml(x, y[, z], values, variogram_model, start=None, fit_anisotropy=False, drift=None, reml=True, bounds=None,
    **anisotropy)``

    Minimises ``neg_log_likelihood`` with ``scipy.optimize.minimize(method='Nelder-Mead')``: derivative-free, so a trial model whose
    matrix is not positive definite (``inf``) does no harm, and deterministic.  One device call per evaluation.  The search is over
    log psill, log range and log(nugget + floor), floor = 1e-8 var(values), so that nugget = 0 is reachable as a bound; with
    fit_anisotropy also over log scaling and the angle in degrees (2-D) or the two log scalings and the three angles (3-D).  After the
    first convergence the search is restarted once from its result with a fresh simplex.

    values: one field (N,), or (N, F) treated as F independent replicates of one variogram -- the objective is the sum over the fields.
    start: None -- the constructor's least-squares fit of the binned variogram (of the first field) -- or variogram parameters in the
    constructor's forms.  The anisotropy keywords of the constructor (``anisotropy_scaling``, ``anisotropy_angle``; 3-D:
    ``anisotropy_scaling_y`` ...) give the fixed anisotropy, or the start of its search.  bounds: a dict from 'psill', 'range', 'nugget',
    'scaling' to (low, high) in natural units, overriding the defaults (psill and nugget up to 100 var(values), range between 1e-3 and
    10 times the bounding box's diagonal, scaling in [0.05, 20]; angles are free).  drift and reml as in ``neg_log_likelihood``.

    Returns an ``MLFit``: ``variogram_parameters`` in the constructor's list form, the anisotropy values (``fit.anisotropy`` as
    keywords), ``nll``, ``n_evaluations``, ``success`` (either pass of the search met its tolerances: 1e-3 in the
    parameters, 1e-6 in the objective).  Argument errors are raised before the library is loaded.

    ``method='nelder-mead'`` (the default) is the search above.  ``method='l-bfgs-b'`` minimises the same objective over the same
    coordinates and bounds with ``scipy.optimize.minimize(method='L-BFGS-B', jac=True)`` and the analytic gradient of
    ``neg_log_likelihood_grad`` (libmikgrad.so; one device call returns the value and the gradient), summed over the fields and taken
    to the search coordinates by the chain rule on the host.  The start is a candidate here too.  A trial that is not positive definite
    does not raise: the line search is told to back off; if L-BFGS-B cannot finish, the Nelder-Mead search continues from the best point
    seen and ``message`` says so.  ``n_evaluations`` counts the device calls of both kinds."""
    from scipy.optimize import minimize

    who = "fit_variogram_ml"
    fit = _Fit(who, (x, y) + args, kwargs, _FIT_NAMES)
    method = fit.kw.get("method", "nelder-mead")
    if method is None:
        method = "nelder-mead"
    if not isinstance(method, str) or method.lower() not in FIT_METHODS:
        raise ValueError("%s: method must be one of %s, got %r" % (who, ", ".join(repr(k) for k in FIT_METHODS), method))
    raw, n, ndim, v, model, reml = fit.raw, fit.n, fit.ndim, fit.v, fit.model, fit.reml
    fit.prepare()
    objective = fit.objective(lambda adj, par, W: gram(adj, model, par, W))
    nll0 = objective(fit.t0)  # the start is a candidate too: the result is never worse than it

    def value_and_gradient(t):
        """The objective and its gradient in the search coordinates: one device call."""
        par, sc, an, adj, Xt, pieces = fit.trial(t)
        dco = anisotropy_derivatives(raw, sc, an) if fit.fit_anis else np.zeros((0, n, ndim))
        logdet, G, grad, _ = gram_grad(adj, dco, model, par, v, Xt, reml)
        f = float(np.sum(nll_from_gram(n, logdet, G, v.shape[1], reml, pieces)))
        g = np.sum(grad, axis=0)
        # d/dlog psill, d/dlog range, d/dlog(nugget + floor), d/dlog scaling; the angles are searched in degrees
        chain = [par[0], par[1], par[2] + fit.floor] + ([float(s_) for s_ in sc] + [1.0] * len(an) if fit.fit_anis else [])
        return f, g * np.array(chain)

    if method.lower() == "l-bfgs-b":
        return _ml_fit(fit, *_fit_lbfgsb(minimize, objective, value_and_gradient, fit.t0, nll0, fit.box, fit.simplex))
    return _ml_fit(fit, *_nelder_mead(minimize, objective, fit, nll0))


class _Fit:
    """What ``fit_variogram_ml`` and ``fit_variogram_vecchia`` share: the checked arguments (``__init__``), the search coordinates with
    their start, bounds and simplex (``prepare``) and the objective over them.  The coordinates are t = [log psill, log range,
    log(nugget + floor)], with fit_anisotropy followed by the log scalings and the angles in degrees."""

    def __init__(self, who, args, kwargs, names, accepted=()):
        self.who = who
        self.raw, self.n, self.ndim, self.v, _, self.model, self.kw = _station_arguments(who, args, kwargs, names, accepted)
        self.scaling0, self.angle0 = _anisotropy(who, self.ndim, self.kw)
        self.adj0 = _adjust(self.raw, self.scaling0, self.angle0)
        self.X = _trend(who, self.kw.get("drift"), self.n, self.adj0)
        self.reml = bool(self.kw.get("reml", True))
        self.fit_anis = bool(self.kw.get("fit_anisotropy", False))
        self.calls = 0  # the device calls spent

    def prepare(self, start_rows=None):
        """The bounds, the start and the simplex steps.  With start=None the start is the constructor's least-squares fit of the binned
        variogram of the first field, over all stations or over the rows ``start_rows()`` returns."""
        who, raw, v = self.who, self.raw, self.v
        var = float(np.var(v))
        if not var > 0.0:
            raise ValueError("%s: the values are constant; there is no variogram to fit" % who)
        diag = float(np.sqrt(np.sum((raw.max(axis=0) - raw.min(axis=0)) ** 2)))
        if not diag > 0.0:
            raise ValueError("%s: all stations coincide" % who)
        self.floor = floor = NUGGET_FLOOR * var
        lim = {"psill": (1e-6 * var, 100.0 * var), "range": (1e-3 * diag, 10.0 * diag), "nugget": (0.0, 100.0 * var), "scaling": (0.05, 20.0)}
        given = self.kw.get("bounds")
        if given is not None:
            if not isinstance(given, dict) or set(given) - set(lim):
                raise ValueError("%s: bounds must be a dict with keys among 'psill', 'range', 'nugget', 'scaling'" % who)
            for k, (lo, hi) in given.items():
                lo, hi = float(lo), float(hi)
                if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi and (lo > 0.0 or (k == "nugget" and lo >= 0.0))):
                    raise ValueError("%s: bounds[%r] must be (low, high) with 0 < low < high (nugget: 0 <= low)" % (who, k))
                lim[k] = (lo, hi)
        start = self.kw.get("start")
        if start is None:
            from . import variogram_fit

            rows = slice(None) if start_rows is None else start_rows()
            par0 = [float(t) for t in variogram_fit.fit(self.adj0[rows], v[rows, 0], self.model, 6, False, "euclidean")[2]]
        else:
            par0 = _internal_parameters(who, self.model, start)
        clip = lambda t, k: min(max(t, lim[k][0]), lim[k][1])
        par0 = [clip(par0[0], "psill"), clip(par0[1], "range"), clip(par0[2], "nugget")]
        self.pieces = _pieces(self.X)
        # with drift='regional_linear' the trend columns are the adjusted coordinates: they move with the anisotropy
        self.moving = isinstance(self.kw.get("drift"), str) and self.fit_anis
        t0 = [math.log(par0[0]), math.log(par0[1]), math.log(par0[2] + floor)]
        self.box = [tuple(math.log(b) for b in lim["psill"]), tuple(math.log(b) for b in lim["range"]),
                    (math.log(lim["nugget"][0] + floor), math.log(lim["nugget"][1] + floor))]
        self.step = [0.4, 0.4, 0.6]
        if self.fit_anis:
            nscale = len(self.scaling0)
            t0 += [math.log(clip(s, "scaling")) for s in self.scaling0] + list(self.angle0)
            self.box += [tuple(math.log(b) for b in lim["scaling"])] * nscale + [(None, None)] * len(self.angle0)
            self.step += [0.35] * nscale + [25.0] * len(self.angle0)
        self.t0 = np.array(t0)

    def unpack(self, t):
        """t -> the internal parameters [psill, range, nugget], the scaling list, the angle list."""
        par = [math.exp(t[0]), math.exp(t[1]), max(math.exp(t[2]) - self.floor, 0.0)]
        if self.fit_anis:
            nscale = len(self.scaling0)
            return par, [math.exp(s) for s in t[3:3 + nscale]], [float(a) for a in t[3 + nscale:]]
        return par, self.scaling0, self.angle0

    def trial(self, t):
        """One evaluation at t is counted -> parameters, scaling, angle, adjusted coordinates, trend matrix, log det(X^T X)."""
        par, sc, an = self.unpack(t)
        self.calls += 1
        adj = _adjust(self.raw, sc, an)
        if self.moving:
            Xt = np.hstack([np.ones((self.n, 1)), adj])
            return par, sc, an, adj, Xt, _pieces(Xt)
        return par, sc, an, adj, self.X, self.pieces

    def objective(self, gram_of):
        """The negative log-likelihood summed over the fields as a function of t; ``gram_of(adj, par, W)`` is the device call."""
        def objective(t):
            par, _, _, adj, Xt, pieces = self.trial(t)
            logdet, G = gram_of(adj, par, np.hstack([self.v, Xt]))
            return float(np.sum(nll_from_gram(self.n, logdet, G, self.v.shape[1], self.reml, pieces)))

        return objective

    def simplex(self, c, scale):
        pts = [np.array(c)]
        for k, s in enumerate(self.step):
            q = np.array(c)
            q[k] += s * scale if self.box[k][1] is None or q[k] + s * scale <= self.box[k][1] else -s * scale
            pts.append(q)
        return np.array(pts)


def _nelder_mead(minimize, objective, fit, nll0):
    """The derivative-free search from the start, and one restart from its result: (best t, best nll, converged, message)."""
    best_t, best = fit.t0, nll0
    converged, message = False, ""
    for scale in (1.0, 0.5):
        res = minimize(objective, best_t, method="Nelder-Mead", bounds=fit.box,
                       options=dict(initial_simplex=fit.simplex(best_t, scale), xatol=1e-3, fatol=1e-6, maxfev=200 * len(fit.t0)))
        converged, message = converged or bool(res.success), str(res.message)
        if res.fun < best:
            best_t, best = np.array(res.x), float(res.fun)
    return best_t, best, converged, message


def _ml_fit(fit, best_t, best, converged, message):
    par, sc, an = fit.unpack(best_t)
    anis = dict(zip(_ANIS2 if fit.ndim == 2 else _ANIS3, list(sc) + list(an)))
    return MLFit(fit.model, [par[0] + par[2], par[1], par[2]], anis, best, fit.calls, bool(converged and math.isfinite(best)), message,
                 fit.reml)


# ------------------------------------------------------------------------------------------------------------- the analytic gradient
# ctypes binding of libmikgrad.so (include/mikgrad.h), a fifth library, loaded on first use of neg_log_likelihood_grad or of
# fit_variogram_ml(method='l-bfgs-b'); everything above works without it.
LIB_PATH_GRAD = os.path.join(_HERE, "libmikgrad.so")
MLG_OK, MLG_EINVAL, MLG_ENOTPD, MLG_EHIP = 0, -1, -2, -3
ABI_VERSION_GRAD = 1  # include/mikgrad.h MLG_ABI_VERSION
MAXGEOM = 5  # MLG_MAXGEOM
GRAD_NAMES_2D = ("psill", "range", "nugget") + _ANIS2
GRAD_NAMES_3D = ("psill", "range", "nugget") + _ANIS3

# every entry point include/mikgrad.h declares: name -> (restype, argtypes)
SIGNATURES_GRAD = {
    "mlg_abi_version": (C.c_int, []),
    "mlg_last_error": (C.c_char_p, []),
    "mlg_grad": (C.c_int, [C.c_int, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, _dp, C.c_int32,
                           _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _i32p]),
}

_lib_grad = None


def load_grad():
    """dlopen libmikgrad.so and declare the signatures.  Raises ImportError if it has not been built or is stale."""
    global _lib_grad
    if _lib_grad is None:
        _lib_grad = _dl.open_library(LIB_PATH_GRAD, "mlg", ABI_VERSION_GRAD, SIGNATURES_GRAD)
    return _lib_grad


def gram_grad(coords, dcoords, model, parameters, V, X, reml):
    """``logdet, G, grad, info = gram_grad(coords, dcoords, model, parameters, V, X, reml)``: one call of ``mlg_grad``, the one device
    call of the gradient path.

    coords: (N, 2) or (N, 3) adjusted coordinates; dcoords: (ng, N, ndim), 0 <= ng <= 5, for each geometry parameter the derivative of
    the adjusted coordinates; parameters: the internal [psill, range, nugget]; V: (N, F) fields, 1 <= F <= 32; X: (N, p) trend columns,
    1 <= p <= 8.  logdet and G = W^T C^-1 W of W = [V | X] are ``gram``'s bit for bit; grad is (F, 3 + ng): for every field the
    derivatives of the ML (reml false) or REML objective of ``nll_from_gram`` with respect to psill, range, nugget and the ng geometry
    parameters, X held fixed.  If C (or X^T C^-1 X) is not positive definite in float64: logdet ``inf``, G and grad NaN, and info the
    1-based column of the failed pivot (0 otherwise).  The arguments are checked by the callers in this module; there is no CPU
    fallback."""
    Xc = np.ascontiguousarray(np.asarray(coords, dtype=np.float64))
    n, ndim = Xc.shape
    D = np.ascontiguousarray(np.asarray(dcoords, dtype=np.float64).reshape(-1, n, ndim).transpose(0, 2, 1))
    ng = int(D.shape[0])
    psill, rng, nugget = (float(t) for t in parameters)
    Va, Xa = np.asarray(V, dtype=np.float64), np.asarray(X, dtype=np.float64)
    F, p = int(Va.shape[1]), int(Xa.shape[1])
    ct, vt, xt = np.ascontiguousarray(Xc.T), np.ascontiguousarray(Va.T), np.ascontiguousarray(Xa.T)
    m = F + p
    G = np.zeros((m, m))
    grad = np.zeros((F, 3 + ng))
    logdet = C.c_double(0.0)
    info = C.c_int32(0)
    lib = load_grad()
    rc = lib.mlg_grad(_dl.device(), n, ndim, ct.ctypes.data_as(_dp), ng, D.ctypes.data_as(_dp) if ng else None, MODEL_IDS[model], psill, rng,
                      nugget, vt.ctypes.data_as(_dp), F, xt.ctypes.data_as(_dp), p, 1 if reml else 0, C.byref(logdet), G.ctypes.data_as(_dp),
                      grad.ctypes.data_as(_dp), C.byref(info))
    if rc == MLG_ENOTPD:
        return math.inf, np.full((m, m), np.nan), np.full((F, 3 + ng), np.nan), int(info.value)
    if rc != MLG_OK:
        _dl.raise_for(lib, "mlg", "libmikgrad", rc, MLG_EINVAL)
    return float(logdet.value), G, grad, 0


def anisotropy_derivatives(raw, scaling, angle):
    """(ng, N, ndim): for each anisotropy parameter -- 2-D: scaling, angle; 3-D: scaling_y, scaling_z, angle_x, angle_y, angle_z -- the
    derivative of ``core.adjust_for_anisotropy(raw, centre, scaling, angle)`` with respect to it, angles per degree: the derivative of
    ``stretch . rot`` (``core.anisotropy_matrices``) applied to the raw coordinates about the constructor's centre.  The centre cancels
    in every difference of two stations."""
    raw = np.asarray(raw, dtype=np.float64)
    ndim = raw.shape[1]
    center = np.array([(float(np.amax(c)) + float(np.amin(c))) / 2.0 for c in raw.T])
    Y = (raw - center[None, :]).T
    rot, stretch = core.anisotropy_matrices(ndim, scaling, angle)
    S = np.diag(stretch)
    k = -np.pi / 180.0  # the rotations are built from -angle in radians
    ang = np.asarray(angle, dtype=np.float64) * np.pi / 180
    if ndim == 2:
        c, s = np.cos(-ang[0]), np.sin(-ang[0])
        mats = [np.diag([0.0, 1.0]) @ rot, S @ (k * np.array([[-s, -c], [c, -s]]))]
    else:
        cx, sx = np.cos(-ang[0]), np.sin(-ang[0])
        cy, sy = np.cos(-ang[1]), np.sin(-ang[1])
        cz, sz = np.cos(-ang[2]), np.sin(-ang[2])
        rot_x = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
        rot_y = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
        rot_z = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
        d_x = k * np.array([[0.0, 0.0, 0.0], [0.0, -sx, -cx], [0.0, cx, -sx]])
        d_y = k * np.array([[-sy, 0.0, cy], [0.0, 0.0, 0.0], [-cy, 0.0, -sy]])
        d_z = k * np.array([[-sz, -cz, 0.0], [cz, -sz, 0.0], [0.0, 0.0, 0.0]])
        mats = [np.diag([0.0, 1.0, 0.0]) @ rot, np.diag([0.0, 0.0, 1.0]) @ rot, S @ rot_z @ rot_y @ d_x, S @ rot_z @ d_y @ rot_x,
                S @ d_z @ rot_y @ rot_x]
    return np.array([(M @ Y).T for M in mats])


def neg_log_likelihood_grad(x, y, *args, **kwargs):
    """The negative Gaussian log-likelihood of ``neg_log_likelihood`` and its analytic gradient, from one elimination on the GPU.

    ``nll, grad = neg_log_likelihood_grad(x, y[, z], values, variogram_model, variogram_parameters, anisotropy_scaling=1.0,
    anisotropy_angle=0.0, drift=None, reml=True)`` -- the arguments of ``neg_log_likelihood``.  nll is what ``neg_log_likelihood``
    returns, bit for bit.  grad has shape (3 + ng,) for (N,) values and (F, 3 + ng) for (N, F) values, in natural units and in the
    order of ``GRAD_NAMES_2D`` / ``GRAD_NAMES_3D``: psill (the PARTIAL sill, with the nugget held), range, nugget, then the
    constructor's anisotropy keywords (ng = 2 in the plane, 5 in space), angles per degree.  Row f of an (N, F) call is bit for bit the
    one-field call.

    d nll / d theta_k = 1/2 tr(M dC/dtheta_k) - 1/2 a^T (dC/dtheta_k) a with a = P y, P = Q - Q X (X^T Q X)^-1 X^T Q, Q = C^-1, and
    M = P under REML, Q under ML; the derivative matrices are defined in include/mikgrad.h.  The host forms the derivatives of the
    adjusted coordinates analytically (``anisotropy_derivatives``).  With drift='regional_linear' the trend columns move with the
    anisotropy, but the objective depends on X only through its column space (-log det X^T X + log det X^T Q X is invariant under
    X -> X A), and the column space of [1 | adjusted coordinates] is that of [1 | raw coordinates] for every anisotropy: the gradient
    taken with X held at the current adjusted coordinates is exact.

    A covariance matrix that is not positive definite in float64 gives ``inf`` and a gradient of NaN.  The refusals are
    ``neg_log_likelihood``'s, raised before the library is loaded.  There is no CPU fallback."""
    raw, n, ndim, v, many, model, par, scaling, angle, adj, X, reml, kw = _nll_arguments("neg_log_likelihood_grad", (x, y) + args, kwargs)
    logdet, G, grad, _ = gram_grad(adj, anisotropy_derivatives(raw, scaling, angle), model, par, v, X, reml)
    out = nll_from_gram(n, logdet, G, v.shape[1], reml, _pieces(X))
    return (out, grad) if many else (float(out[0]), grad[0])


def _fit_lbfgsb(minimize, objective, value_and_gradient, t0, nll0, box, simplex):
    """The quasi-Newton search of fit_variogram_ml(method='l-bfgs-b'): (best t, best nll, converged, message).  A trial whose matrix is
    not positive definite is answered with a finite value above everything seen and a zero gradient, so that the line search backs off;
    if L-BFGS-B still cannot finish, the Nelder-Mead search continues from the best point seen.

    The nugget is searched as log(nugget + floor): where the nugget is far below the partial sill that coordinate is a plateau -- its
    gradient is (nugget + floor) d nll / d nugget, next to nothing whatever the natural derivative says -- and a start with nugget = 0
    (the least-squares fit gives it often) sits on the bound.  So after a pass that ends with nugget < psill / 1000 and
    d nll / d nugget < 0, the search is run once more from its result with the nugget lifted to psill / 100; the best point seen wins."""
    best = [np.array(t0), float(nll0), None]
    worst = [float(nll0)]
    refused = set()  # the trials that were answered with the stand-in value

    def fun(t):
        f, g = value_and_gradient(t)
        if not (math.isfinite(f) and np.all(np.isfinite(g))):
            refused.add(tuple(float(c) for c in t))
            return worst[0] + 1e3 * (1.0 + abs(worst[0])), np.zeros(len(t))
        worst[0] = max(worst[0], f)
        if f < best[1] or best[2] is None:
            best[0], best[1], best[2] = np.array(t), min(f, best[1]), np.array(g)
        return f, g

    opts = dict(maxiter=200, maxfun=400, ftol=1e-10, gtol=1e-6)
    res = minimize(fun, np.array(t0), method="L-BFGS-B", jac=True, bounds=box, options=opts)
    lifted = float(np.log(1e-2 * math.exp(best[0][0]) + math.exp(box[2][0])))  # (exp of the lower bound of t[2] is nugget_low + floor)
    if best[2] is not None and best[2][2] < 0.0 and math.exp(best[0][2]) - math.exp(box[2][0]) < 1e-3 * math.exp(best[0][0]) \
            and box[2][0] < lifted < box[2][1]:
        t1 = np.array(best[0])
        t1[2] = lifted
        again = minimize(fun, t1, method="L-BFGS-B", jac=True, bounds=box, options=opts)
        if again.fun <= res.fun:
            res = again
    message = str(res.message.decode() if isinstance(res.message, bytes) else res.message)
    converged = bool(res.success) and tuple(float(c) for c in res.x) not in refused  # (a zero gradient there is no convergence)
    if not converged:
        res = minimize(objective, best[0], method="Nelder-Mead", bounds=box,
                       options=dict(initial_simplex=simplex(best[0], 0.5), xatol=1e-3, fatol=1e-6, maxfev=200 * len(t0)))
        message = "L-BFGS-B could not continue (%s); finished with the Nelder-Mead search from the best point: %s" % (message, res.message)
        converged = bool(res.success)
        if res.fun < best[1]:
            best[0], best[1] = np.array(res.x), float(res.fun)
    return best[0], best[1], converged, message
