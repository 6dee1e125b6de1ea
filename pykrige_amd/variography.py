"""Directional semivariograms and variogram maps on the GPU: the tools that find ``anisotropy_scaling`` and ``anisotropy_angle``.

ctypes binding of libmikvario.so (include/mikvario.h), a second library beside libmikrige.so, loaded on first use.  NumPy + ctypes only.
As in _lib there is no CPU fallback: a missing library or no visible GPU raises.  Every argument error is a ValueError raised here,
before the library is loaded.

For a pair i < j in the caller's station order: dx = x[j] - x[i], dy = y[j] - y[i], d = sqrt(dx*dx + dy*dy), g = 0.5 (v[i] - v[j])^2.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _dl

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmikvario.so")

MKV_OK, MKV_EINVAL, MKV_EHIP = 0, -1, -3
ABI_VERSION = 1  # include/mikvario.h MKV_ABI_VERSION
MAXLAGS, MAXDIRS, MAXCELLS = 64, 16, 4225  # MKV_MAXLAGS, MKV_MAXDIRS, MKV_MAXCELLS

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)

# every entry point include/mikvario.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mkv_abi_version": (C.c_int, []),
    "mkv_last_error": (C.c_char_p, []),
    "mkv_directional": (C.c_int, [C.c_int, C.c_int64, _dp, _dp, _dp, C.c_int32, _dp, C.c_int32, C.c_double, C.c_double, _dp, C.c_int32,
                                  _dp, _dp, _ip]),
    "mkv_map": (C.c_int, [C.c_int, C.c_int64, _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _dp, _ip]),
}

_lib = None


def load():
    """dlopen libmikvario.so and declare the signatures.  Raises ImportError if it has not been built or is stale."""
    global _lib
    if _lib is None:
        _lib = _dl.open_library(LIB_PATH, "mkv", ABI_VERSION, SIGNATURES)
    return _lib


def _check(lib, rc):
    if rc != MKV_OK:
        _dl.raise_for(lib, "mkv", "libmikvario", rc, MKV_EINVAL)


def direction_constants(azimuths, tolerance):
    """(cos theta, sin theta) per azimuth and tan(tolerance) as the library forms them: the C library's cos / sin / tan of
    degrees * (pi / 180), float64.  The device decides direction membership from exactly these numbers."""
    az = [float(a) for a in np.atleast_1d(np.asarray(azimuths, dtype=np.float64)).ravel()]
    rad = math.pi / 180.0
    return (np.array([math.cos(a * rad) for a in az]), np.array([math.sin(a * rad) for a in az]), math.tan(float(tolerance) * rad))


def _stations(who, x, y, values):
    """x, y (N,), values (N,) or (N, F) -> x, y, field-major values (F, N), whether values came as (N, F)."""
    x = np.ascontiguousarray(np.atleast_1d(np.squeeze(np.asarray(x, dtype=np.float64))))
    y = np.ascontiguousarray(np.atleast_1d(np.squeeze(np.asarray(y, dtype=np.float64))))
    v = np.asarray(values, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("%s: x and y must be one-dimensional arrays of the same length" % who)
    n = x.size
    if n < 2:
        raise ValueError("%s: need at least two stations" % who)
    if n >= 2 ** 31:
        raise ValueError("%s: the number of stations must be below 2^31" % who)
    many = v.ndim == 2
    if v.ndim == 1:
        v = v[:, None]
    if v.ndim != 2 or v.shape[0] != n or v.shape[1] < 1:
        raise ValueError("%s: values must have shape (N,) or (N, F) with N = %d stations and F >= 1 fields, got %s"
                         % (who, n, np.shape(values)))
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("%s: station coordinates must be finite" % who)
    if not np.all(np.isfinite(v)):
        raise ValueError("%s: values must be finite (krige fields with gaps through execute_fields(valid=...))" % who)
    return x, y, np.ascontiguousarray(v.T), many


def _mean(total, counts):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts > 0, total / np.maximum(counts, 1), np.nan)


def directional_variogram(x, y, values, azimuths, tolerance=22.5, nlags=6, maxlag=None, edges=None, bandwidth=None):
    """Experimental semivariograms by direction, all N (N - 1) / 2 pairs binned on the GPU.

    ``lags, semivariance, counts = directional_variogram(x, y, values, azimuths, tolerance=22.5, nlags=6, maxlag=None, edges=None,
    bandwidth=None)``

    x, y: (N,) station coordinates.  values: (N,) or (N, F) -- F fields on the same stations, as in ``execute_fields``; the pair
    geometry is evaluated once for every eight fields.  azimuths: A directions in degrees counter-clockwise from +x, the convention of
    ``anisotropy_angle``; directions are axial (theta and theta + 180 are the same).  A pair with separation (dx, dy) belongs to
    direction theta if ``across <= along * tan(tolerance)`` with ``along = |dx cos theta + dy sin theta|`` and ``across = |-dx sin theta
    + dy cos theta|`` (tolerance in degrees, in (0, 90]; 90 takes every pair: the omnidirectional variogram) and, if a bandwidth is
    given, ``across <= bandwidth``.  A pair may belong to several directions; coincident stations (d = 0) belong to all of them.

    Lag bin b holds the pairs with ``edges[b] <= d < edges[b + 1]``; pairs outside every bin are dropped.  edges (ascending, at most
    64 bins) overrides nlags and maxlag; without it ``edges = linspace(0, maxlag, nlags + 1)``, and maxlag=None is half the diagonal of
    the stations' bounding box.  At most 16 azimuths per call.

    Returns lags (A, nlags) -- the mean pair distance per bin --, semivariance (A, nlags), or (F, A, nlags) for (N, F) values -- the
    mean of 0.5 (v_i - v_j)^2 --, and counts (A, nlags), int64, which do not depend on the field.  Bins without a pair hold NaN.  Counts
    are exact; the means are float64 sums whose order may differ from run to run.  Argument errors raise ValueError before the library is
    loaded; there is no CPU fallback."""
    who = "directional_variogram"
    x, y, v, many = _stations(who, x, y, values)
    az = np.ascontiguousarray(np.atleast_1d(np.asarray(azimuths, dtype=np.float64)))
    if az.ndim != 1 or az.size < 1:
        raise ValueError("%s: azimuths must be a non-empty one-dimensional sequence of angles in degrees" % who)
    if az.size > MAXDIRS:
        raise ValueError("%s: at most %d azimuths per call (MKV_MAXDIRS), got %d" % (who, MAXDIRS, az.size))
    if not np.all(np.isfinite(az)):
        raise ValueError("%s: azimuths must be finite" % who)
    tol = float(tolerance)
    if not (0.0 < tol <= 90.0):
        raise ValueError("%s: tolerance must be in (0, 90] degrees, got %r" % (who, tolerance))
    bw = 0.0
    if bandwidth is not None:
        bw = float(bandwidth)
        if not (math.isfinite(bw) and bw > 0.0):
            raise ValueError("%s: bandwidth must be positive and finite (None: no bandwidth), got %r" % (who, bandwidth))
    if edges is None:
        if isinstance(nlags, bool) or int(nlags) != nlags or nlags < 1:
            raise ValueError("%s: nlags must be a positive integer, got %r" % (who, nlags))
        if nlags > MAXLAGS:
            raise ValueError("%s: at most %d lag bins (MKV_MAXLAGS), got %d" % (who, MAXLAGS, nlags))
        if maxlag is None:
            maxlag = 0.5 * math.hypot(float(x.max() - x.min()), float(y.max() - y.min()))
            if not maxlag > 0.0:
                raise ValueError("%s: all stations coincide; give maxlag or edges" % who)
        maxlag = float(maxlag)
        if not (math.isfinite(maxlag) and maxlag > 0.0):
            raise ValueError("%s: maxlag must be positive and finite, got %r" % (who, maxlag))
        e = np.linspace(0.0, maxlag, int(nlags) + 1)
    else:
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
        if e.ndim != 1 or e.size < 2:
            raise ValueError("%s: edges must be a one-dimensional sequence of at least two values" % who)
        if e.size - 1 > MAXLAGS:
            raise ValueError("%s: at most %d lag bins (MKV_MAXLAGS), got %d" % (who, MAXLAGS, e.size - 1))
        if not np.all(np.isfinite(e)):
            raise ValueError("%s: edges must be finite" % who)
    if not np.all(np.diff(e) > 0.0):
        raise ValueError("%s: edges must be ascending" % who)
    nb, na, nf, n = int(e.size - 1), int(az.size), int(v.shape[0]), int(x.size)
    lag_sum = np.zeros((na, nb))
    semi_sum = np.zeros((nf, na, nb))
    counts = np.zeros((na, nb), dtype=np.int64)
    lib = load()
    _check(lib, lib.mkv_directional(_dl.device(), n, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), v.ctypes.data_as(_dp), nf,
                                    az.ctypes.data_as(_dp), na, tol, bw, e.ctypes.data_as(_dp), nb,
                                    lag_sum.ctypes.data_as(_dp), semi_sum.ctypes.data_as(_dp), counts.ctypes.data_as(_ip)))
    semi = _mean(semi_sum, counts[None, :, :])
    return _mean(lag_sum, counts), (semi if many else semi[0]), counts


def variogram_map(x, y, values, nx, ny, dx, dy):
    """Variogram map: the semivariance over a grid of lag vectors, all pairs binned on the GPU.

    ``semivariance, counts = variogram_map(x, y, values, nx, ny, dx, dy)``

    The map has (2 ny + 1) x (2 nx + 1) cells of size dx x dy centred on lag zero, at most 4225 (65 x 65) cells.  A pair i < j with
    separation h = (x[j] - x[i], y[j] - y[i]) falls into cell ``[ny + floor(h_y / dy + 0.5), nx + floor(h_x / dx + 0.5)]`` and into the
    mirror cell of -h, and is dropped when outside the map: the map is exactly point-symmetric.  Coincident stations count twice in the
    centre cell.  values: (N,) or (N, F) as in ``directional_variogram``.

    Returns semivariance (2 ny + 1, 2 nx + 1), or (F, 2 ny + 1, 2 nx + 1) for (N, F) values -- the mean of 0.5 (v_i - v_j)^2, NaN in
    cells without a pair -- and counts (2 ny + 1, 2 nx + 1), int64.  Argument errors raise ValueError before the library is loaded."""
    who = "variogram_map"
    x, y, v, many = _stations(who, x, y, values)
    for name, k in (("nx", nx), ("ny", ny)):
        if isinstance(k, bool) or int(k) != k or k < 0:
            raise ValueError("%s: %s must be a non-negative integer, got %r" % (who, name, k))
    nx, ny = int(nx), int(ny)
    if (2 * nx + 1) * (2 * ny + 1) > MAXCELLS:
        raise ValueError("%s: (2 nx + 1)(2 ny + 1) = %d cells, at most %d (MKV_MAXCELLS: half the map is kept in the LDS of a workgroup)"
                         % (who, (2 * nx + 1) * (2 * ny + 1), MAXCELLS))
    dx, dy = float(dx), float(dy)
    if not (math.isfinite(dx) and math.isfinite(dy) and dx > 0.0 and dy > 0.0):
        raise ValueError("%s: dx and dy must be positive and finite" % who)
    nf, n = int(v.shape[0]), int(x.size)
    semi_sum = np.zeros((nf, 2 * ny + 1, 2 * nx + 1))
    counts = np.zeros((2 * ny + 1, 2 * nx + 1), dtype=np.int64)
    lib = load()
    _check(lib, lib.mkv_map(_dl.device(), n, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), v.ctypes.data_as(_dp), nf, nx, ny, dx, dy,
                            semi_sum.ctypes.data_as(_dp), counts.ctypes.data_as(_ip)))
    semi = _mean(semi_sum, counts[None, :, :])
    return (semi if many else semi[0]), counts
