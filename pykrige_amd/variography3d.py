"""Directional semivariograms and variogram maps of 3-D station sets on the GPU: the tools that check ``anisotropy_scaling_y/_z`` and
``anisotropy_angle_x/_y/_z`` of the 3-D classes.

ctypes binding of libmikvario3.so (include/mikvario3.h), a third library beside libmikrige.so and libmikvario.so (the 2-D tool,
variography.py), loaded on first use.  NumPy + ctypes only.  There is no CPU fallback: a missing library or no visible GPU raises.  Every
argument error is a ValueError raised here, before the library is loaded.

For a pair i < j in the caller's station order: dx = x[j] - x[i], dy = y[j] - y[i], dz = z[j] - z[i], d = sqrt(dx*dx + dy*dy + dz*dz),
g = 0.5 (v[i] - v[j])^2.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _dl

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmikvario3.so")

MKV3_OK, MKV3_EINVAL, MKV3_EHIP = 0, -1, -3
ABI_VERSION = 1  # include/mikvario3.h MKV3_ABI_VERSION
MAXLAGS, MAXDIRS, MAXCELLS = 64, 16, 4225  # MKV3_MAXLAGS, MKV3_MAXDIRS, MKV3_MAXCELLS

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)

# every entry point include/mikvario3.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mkv3_abi_version": (C.c_int, []),
    "mkv3_last_error": (C.c_char_p, []),
    "mkv3_directional": (C.c_int, [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, C.c_int32, _dp, C.c_int32, C.c_double, C.c_double, _dp,
                                   C.c_int32, _dp, _dp, _ip]),
    "mkv3_map": (C.c_int, [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                           C.c_double, _dp, _ip]),
}

_lib = None


def load():
    """dlopen libmikvario3.so and declare the signatures.  Raises ImportError if it has not been built or is stale."""
    global _lib
    if _lib is None:
        _lib = _dl.open_library(LIB_PATH, "mkv3", ABI_VERSION, SIGNATURES)
    return _lib


def _check(lib, rc):
    if rc != MKV3_OK:
        _dl.raise_for(lib, "mkv3", "libmikvario3", rc, MKV3_EINVAL)


def direction_vectors(azimuths, dips):
    """(A, 3) unit vectors ``u = (cos(dip) cos(az), cos(dip) sin(az), sin(dip))`` of A directions given in degrees: the azimuth
    counter-clockwise from +x in the x-y plane (the 2-D tool's convention), the dip upward from that plane toward +z, in [-90, 90].  cos and
    sin are the C library's (Python's ``math``) of ``degrees * (pi / 180)``, float64.  These three numbers per direction are what crosses
    the C ABI, and the device decides direction membership from them."""
    who = "direction_vectors"
    az = np.atleast_1d(np.asarray(azimuths, dtype=np.float64))
    dp = np.atleast_1d(np.asarray(dips, dtype=np.float64))
    if az.ndim != 1 or dp.ndim != 1 or az.size < 1 or az.shape != dp.shape:
        raise ValueError("%s: azimuths and dips must be non-empty one-dimensional sequences of equal length, in degrees" % who)
    if not (np.all(np.isfinite(az)) and np.all(np.isfinite(dp))):
        raise ValueError("%s: azimuths and dips must be finite" % who)
    if not np.all(np.abs(dp) <= 90.0):
        raise ValueError("%s: dips must be in [-90, 90] degrees" % who)
    rad = math.pi / 180.0
    out = np.empty((az.size, 3))
    for k, (a, d) in enumerate(zip(az.tolist(), dp.tolist())):
        cd = math.cos(d * rad)
        out[k] = (cd * math.cos(a * rad), cd * math.sin(a * rad), math.sin(d * rad))
    return out


def decision_constants(tolerance, bandwidth=None):
    """(tan2, bw2) as the library forms them: ``tan2 = tan(tolerance * (pi / 180))^2`` with the C library's tan and ``bw2 = bandwidth^2``
    (None without a bandwidth), one float64 multiplication each.  A pair belongs to a direction if ``across2 <= (along*along) * tan2``
    and, with a bandwidth, ``across2 <= bw2``."""
    t = math.tan(float(tolerance) * (math.pi / 180.0))
    return t * t, (None if bandwidth is None else float(bandwidth) * float(bandwidth))


def _stations(who, x, y, z, values):
    """x, y, z (N,), values (N,) or (N, F) -> x, y, z, field-major values (F, N), whether values came as (N, F)."""
    x = np.ascontiguousarray(np.atleast_1d(np.squeeze(np.asarray(x, dtype=np.float64))))
    y = np.ascontiguousarray(np.atleast_1d(np.squeeze(np.asarray(y, dtype=np.float64))))
    z = np.ascontiguousarray(np.atleast_1d(np.squeeze(np.asarray(z, dtype=np.float64))))
    v = np.asarray(values, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or x.shape != z.shape:
        raise ValueError("%s: x, y and z must be one-dimensional arrays of the same length" % who)
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
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(z))):
        raise ValueError("%s: station coordinates must be finite" % who)
    if not np.all(np.isfinite(v)):
        raise ValueError("%s: values must be finite (krige fields with gaps through execute_fields(valid=...))" % who)
    return x, y, z, np.ascontiguousarray(v.T), many


def _mean(total, counts):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts > 0, total / np.maximum(counts, 1), np.nan)


def _unit_directions(who, azimuths, dips, directions):
    if directions is not None:
        if azimuths is not None or dips is not None:
            raise ValueError("%s: give either azimuths and dips, or directions, not both" % who)
        u = np.asarray(directions, dtype=np.float64)
        if u.ndim == 1 and u.size == 3:
            u = u[None, :]
        if u.ndim != 2 or u.shape[1] != 3 or u.shape[0] < 1:
            raise ValueError("%s: directions must have shape (A, 3) with A >= 1, got %s" % (who, np.shape(directions)))
        if not np.all(np.isfinite(u)):
            raise ValueError("%s: directions must be finite" % who)
        norm = np.sqrt((u * u).sum(axis=1))
        if not np.all(norm > 0.0):
            raise ValueError("%s: directions must be nonzero vectors" % who)
        u = u / norm[:, None]
    else:
        if azimuths is None or dips is None:
            raise ValueError("%s: give either azimuths and dips (of equal length), or directions" % who)
        try:
            u = direction_vectors(azimuths, dips)
        except ValueError as e:
            raise ValueError(str(e).replace("direction_vectors", who, 1)) from None
    if u.shape[0] > MAXDIRS:
        raise ValueError("%s: at most %d directions per call (MKV3_MAXDIRS), got %d" % (who, MAXDIRS, u.shape[0]))
    return np.ascontiguousarray(u)


def directional_variogram_3d(x, y, z, values, azimuths=None, dips=None, directions=None, tolerance=22.5, nlags=6, maxlag=None, edges=None,
                             bandwidth=None):
    """Experimental semivariograms by direction in 3-D, all N (N - 1) / 2 pairs binned on the GPU.

    ``lags, semivariance, counts = directional_variogram_3d(x, y, z, values, azimuths=None, dips=None, directions=None, tolerance=22.5,
    nlags=6, maxlag=None, edges=None, bandwidth=None)``

    x, y, z: (N,) station coordinates.  values: (N,) or (N, F) -- F fields on the same stations, as in ``execute_fields``; the pair
    geometry is evaluated once for every eight fields.  The A directions are given either as azimuths and dips of equal length, in degrees
    -- the azimuth counter-clockwise from +x in the x-y plane, the dip upward from that plane toward +z, in [-90, 90], see
    ``direction_vectors`` -- or as directions, (A, 3) nonzero finite vectors, which are normalised here.  Directions are axial (u and -u
    are the same).  With ``core.anisotropy_axes(angles)`` as directions the three semivariograms are those along the principal axes of a
    candidate rotation: their ranges should stand as 1 : 1 / scaling_y : 1 / scaling_z.

    A pair with separation h = (dx, dy, dz) belongs to direction u if ``across2 <= (along*along) * tan2`` with ``along = dx*ux + dy*uy +
    dz*uz``, ``across2 = |h x u|^2`` and ``tan2 = tan(tolerance)^2`` (tolerance in degrees, in (0, 90]; 90 takes every pair: the
    omnidirectional variogram) and, if a bandwidth is given, ``across2 <= bandwidth^2``.  A pair may belong to several directions;
    coincident stations (d = 0) belong to all of them.

    Lag bin b holds the pairs with ``edges[b] <= d < edges[b + 1]``; pairs outside every bin are dropped.  edges (ascending, at most
    64 bins) overrides nlags and maxlag; without it ``edges = linspace(0, maxlag, nlags + 1)``, and maxlag=None is half the diagonal of
    the stations' bounding box.  At most 16 directions per call.

    Returns lags (A, nlags) -- the mean pair distance per bin --, semivariance (A, nlags), or (F, A, nlags) for (N, F) values -- the
    mean of 0.5 (v_i - v_j)^2 --, and counts (A, nlags), int64, which do not depend on the field.  Bins without a pair hold NaN.  Counts
    are exact; the means are float64 sums whose order may differ from run to run.  Argument errors raise ValueError before the library is
    loaded; there is no CPU fallback."""
    who = "directional_variogram_3d"
    x, y, z, v, many = _stations(who, x, y, z, values)
    u = _unit_directions(who, azimuths, dips, directions)
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
            raise ValueError("%s: at most %d lag bins (MKV3_MAXLAGS), got %d" % (who, MAXLAGS, nlags))
        if maxlag is None:
            ext = [float(c.max() - c.min()) for c in (x, y, z)]
            maxlag = 0.5 * math.sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2])
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
            raise ValueError("%s: at most %d lag bins (MKV3_MAXLAGS), got %d" % (who, MAXLAGS, e.size - 1))
        if not np.all(np.isfinite(e)):
            raise ValueError("%s: edges must be finite" % who)
    if not np.all(np.diff(e) > 0.0):
        raise ValueError("%s: edges must be ascending" % who)
    nb, na, nf, n = int(e.size - 1), int(u.shape[0]), int(v.shape[0]), int(x.size)
    lag_sum = np.zeros((na, nb))
    semi_sum = np.zeros((nf, na, nb))
    counts = np.zeros((na, nb), dtype=np.int64)
    lib = load()
    _check(lib, lib.mkv3_directional(_dl.device(), n, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), z.ctypes.data_as(_dp),
                                     v.ctypes.data_as(_dp), nf, u.ctypes.data_as(_dp), na, tol, bw, e.ctypes.data_as(_dp), nb,
                                     lag_sum.ctypes.data_as(_dp), semi_sum.ctypes.data_as(_dp), counts.ctypes.data_as(_ip)))
    semi = _mean(semi_sum, counts[None, :, :])
    return _mean(lag_sum, counts), (semi if many else semi[0]), counts


def variogram_map_3d(x, y, z, values, nx, ny, nz, dx, dy, dz):
    """3-D variogram map: the semivariance over a grid of lag vectors, all pairs binned on the GPU.

    ``semivariance, counts = variogram_map_3d(x, y, z, values, nx, ny, nz, dx, dy, dz)``

    The map has (2 nz + 1) x (2 ny + 1) x (2 nx + 1) cells of size dx x dy x dz centred on lag zero, at most 4225 cells in all (17 x 17
    x 13, for instance).  A pair i < j with separation h = (x[j] - x[i], y[j] - y[i], z[j] - z[i]) falls into cell ``[nz + floor(h_z / dz
    + 0.5), ny + floor(h_y / dy + 0.5), nx + floor(h_x / dx + 0.5)]`` and into the mirror cell of -h, and is dropped when outside the map:
    the map is exactly point-symmetric.  Coincident stations count twice in the centre cell.  values: (N,) or (N, F) as in
    ``directional_variogram_3d``.  ``semivariance[nz]`` is the horizontal slice through lag zero; with nz = 0 the map is the 2-D map of
    the pairs whose h_z rounds to the centre cell.

    Returns semivariance (2 nz + 1, 2 ny + 1, 2 nx + 1), or (F, 2 nz + 1, 2 ny + 1, 2 nx + 1) for (N, F) values -- the mean of
    0.5 (v_i - v_j)^2, NaN in cells without a pair -- and counts (2 nz + 1, 2 ny + 1, 2 nx + 1), int64.  Argument errors raise ValueError
    before the library is loaded."""
    who = "variogram_map_3d"
    x, y, z, v, many = _stations(who, x, y, z, values)
    for name, k in (("nx", nx), ("ny", ny), ("nz", nz)):
        if isinstance(k, bool) or int(k) != k or k < 0:
            raise ValueError("%s: %s must be a non-negative integer, got %r" % (who, name, k))
    nx, ny, nz = int(nx), int(ny), int(nz)
    ncell = (2 * nx + 1) * (2 * ny + 1) * (2 * nz + 1)
    if ncell > MAXCELLS:
        raise ValueError("%s: (2 nx + 1)(2 ny + 1)(2 nz + 1) = %d cells, at most %d (MKV3_MAXCELLS: half the map is kept in the LDS of a "
                         "workgroup)" % (who, ncell, MAXCELLS))
    dx, dy, dz = float(dx), float(dy), float(dz)
    if not (math.isfinite(dx) and math.isfinite(dy) and math.isfinite(dz) and dx > 0.0 and dy > 0.0 and dz > 0.0):
        raise ValueError("%s: dx, dy and dz must be positive and finite" % who)
    nf, n = int(v.shape[0]), int(x.size)
    shape = (2 * nz + 1, 2 * ny + 1, 2 * nx + 1)
    semi_sum = np.zeros((nf,) + shape)
    counts = np.zeros(shape, dtype=np.int64)
    lib = load()
    _check(lib, lib.mkv3_map(_dl.device(), n, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), z.ctypes.data_as(_dp), v.ctypes.data_as(_dp), nf,
                             nx, ny, nz, dx, dy, dz, semi_sum.ctypes.data_as(_dp), counts.ctypes.data_as(_ip)))
    semi = _mean(semi_sum, counts[None])
    return (semi if many else semi[0]), counts
