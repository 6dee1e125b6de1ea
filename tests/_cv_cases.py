"""Cases and references of the cross-validation tests (tests/test_cross_validate_host.py on the CPU, tests/test_cross_validate.py on
the GPU).

A case builds a pykrige_amd object and the KrigingState of the same problem (oracle/kriging_oracle.py), whose adjusted coordinates
are the object's own.  The reference is brute force: for each station i the state WITHOUT row i (coords_orig, coords_adj, values)
and the extended-precision solve (oracle/exact_kriging.py: exact_points) at station i.  References are computed once per session and
shared.

Bars (tests/_error_cases.C_BAR = 8): C u (cond_1(A) + M) max|v| on z and C u (cond_1(A) + M) max|b| on sigma^2 through ek.bars (so
capped at the float64 parity bars).  A is the FULL kriging matrix and M its order -- the identity reads the inverse of that matrix --
and max|b| the largest variogram value on station i's right-hand side."""
import dataclasses
import functools

import numpy as np
import scipy.linalg

from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _error_cases as ec


def _field(c):
    return np.sin(5 * c[:, 0]) * np.cos(3 * c[:, 1]) + 0.3 * c[:, -1]


def _fxyz(x, y, z):  # the functional drift of the 3-D universal case
    return x * y + 0.5 * z


def state_of(obj, **kw):
    """The KrigingState of a pykrige_amd object; coords_adj are the object's (what the device is handed)."""
    nd = obj._ndim
    orig = np.stack([obj.X_ORIG, obj.Y_ORIG] + ([obj.Z_ORIG] if nd == 3 else []), 1)
    geo = getattr(obj, "coordinates_type", "euclidean") == "geographic"
    st = ko.KrigingState(ndim=nd, coords_orig=orig, values=np.array(obj._values(), dtype=np.float64), model=obj.variogram_model,
                         params=[float(p) for p in obj.variogram_model_parameters], center=np.array(obj._center(), dtype=np.float64),
                         scaling=list(obj._scaling()), angle=list(obj._angle()), exact_values=bool(obj.exact_values), geographic=geo, **kw)
    if not geo:
        st.coords_adj = np.array(obj._coords_adj, dtype=np.float64)
    return st


def without(st, i):
    """The state without station i (same centre, same adjusted coordinates of the others)."""
    r = dataclasses.replace(st, coords_orig=np.delete(st.coords_orig, i, 0), values=np.delete(st.values, i),
                            center=np.array(st.center, dtype=np.float64))
    r.coords_adj = np.delete(st.coords_adj, i, 0)
    return r


# ------------------------------------------------------------------------------------------------------------- global form
def _ok2d_exp():
    import pykrige_amd as pa

    rng = np.random.default_rng(1101)
    c = rng.random((67, 2))  # M = 68 crosses k_cvec's 64-lane stride
    m = pa.OrdinaryKriging(c[:, 0], c[:, 1], _field(c), variogram_model="exponential", variogram_parameters=[1.0, 0.5, 0.02])
    return m, state_of(m)


def _ok2d_sph():
    import pykrige_amd as pa

    rng = np.random.default_rng(1102)
    c = rng.random((130, 2))  # spherical with a range inside the domain: the factor holds the stations in Hilbert order
    m = pa.OrdinaryKriging(c[:, 0], c[:, 1], 1e3 * _field(c), variogram_model="spherical", variogram_parameters=[1.0, 0.3, 0.02])
    return m, state_of(m)


def _uk2d_rl():
    import pykrige_amd as pa

    rng = np.random.default_rng(1103)
    c = rng.random((67, 2))
    m = pa.UniversalKriging(c[:, 0], c[:, 1], _field(c) + 2.0 * c[:, 0], variogram_model="linear", variogram_parameters=[1.0, 0.05],
                            drift_terms=["regional_linear"])
    return m, state_of(m, regional_linear=True)


def _ok3d_gau():
    import pykrige_amd as pa

    rng = np.random.default_rng(1104)
    c = rng.random((40, 3))
    m = pa.OrdinaryKriging3D(c[:, 0], c[:, 1], c[:, 2], _field(c), variogram_model="gaussian", variogram_parameters=[1.0, 0.5, 0.05],
                             anisotropy_scaling_y=1.5, anisotropy_scaling_z=0.7, anisotropy_angle_x=20.0, anisotropy_angle_y=10.0,
                             anisotropy_angle_z=30.0)
    return m, state_of(m)


def _uk3d_fn():
    import pykrige_amd as pa

    rng = np.random.default_rng(1105)
    c = rng.random((40, 3))
    m = pa.UniversalKriging3D(c[:, 0], c[:, 1], c[:, 2], _field(c) + c[:, 0] * c[:, 1], variogram_model="exponential",
                              variogram_parameters=[1.0, 0.5, 0.02], drift_terms=["functional"], functional_drift=[_fxyz])
    return m, state_of(m, functional=[_fxyz])


def _geo_ok():
    import pykrige_amd as pa

    rng = np.random.default_rng(1106)
    lon, lat = rng.uniform(-30, 40, 50), rng.uniform(20, 70, 50)
    v = np.cos(np.radians(lat)) * np.sin(np.radians(2 * lon))
    m = pa.OrdinaryKriging(lon, lat, v, variogram_model="exponential", variogram_parameters=[1.0, 40.0, 0.02],
                           coordinates_type="geographic")
    return m, state_of(m)


GLOBAL = {"ok2d_exponential_n67": _ok2d_exp, "ok2d_spherical_n130_values_1e3": _ok2d_sph, "uk2d_regional_linear_n67": _uk2d_rl,
          "ok3d_gaussian_aniso_n40": _ok3d_gau, "uk3d_functional_n40": _uk3d_fn, "geographic_ok_n50": _geo_ok}


@functools.lru_cache(maxsize=None)
def global_case(name):
    return GLOBAL[name]()


@functools.lru_cache(maxsize=None)
def global_reference(name):
    """Brute force: exact_points on the state without station i, at station i.  cond / order are the FULL matrix's."""
    _, st = global_case(name)
    n = st.n
    z, ss, bscale = np.zeros(n, dtype=ek.LD), np.zeros(n, dtype=ek.LD), np.zeros(n)
    for i in range(n):
        r = ek.exact_points(without(st, i), st.coords_adj[i:i + 1])
        z[i], ss[i], bscale[i] = r.z[0], r.ss[0], r.bscale[0]
    a = ko.kriging_matrix(st)
    cond = float(np.abs(a).sum(axis=0).max() * np.abs(scipy.linalg.inv(a)).sum(axis=0).max())
    return ek.ExactResult(z=z, ss=ss, cond=np.full(n, cond), order=np.full(n, a.shape[0]),
                          vscale=np.full(n, float(np.abs(st.values).max())), bscale=bscale)


def identity(st, values=None):
    """The NumPy restatement of the device's global form: B = inv(A), c = B[:, :n] v, zhat = v - c / diag(B), sigma^2 = 1 / diag(B)."""
    n = st.n
    v = st.values if values is None else values
    b = np.linalg.inv(ko.kriging_matrix(st))
    d = np.diag(b)[:n]
    return v - (b[:n, :n] @ v) / d, 1.0 / d


def ratios(ref, z, ss, c=ec.C_BAR):
    """(max |dz| / bar, max |dss| / bar) of float64 answers against an ExactResult."""
    bz, bs = ek.bars(ref, c)
    dz = np.abs(np.asarray(z, dtype=np.float64).ravel().astype(ek.LD) - ref.z).astype(np.float64)
    ds = np.abs(np.asarray(ss, dtype=np.float64).ravel().astype(ek.LD) - ref.ss).astype(np.float64)
    return float((dz / bz).max()), float((ds / bs).max())
