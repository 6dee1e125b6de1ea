"""The extended-precision kriging reference (oracle/exact_kriging.py) on the CPU: against mpmath at 40 digits on small systems of
every model, ordinary and universal kriging, 3-D, geographic coordinates, a moving window and exact hits; and the float64 oracle
within the bar of tests/test_kernel_error_bounds.py on every case of its matrix and on every execute fixture -- a correct float64
computation meets that bar, so it is not tuned to the kernels."""
import mpmath
import numpy as np
import pytest

from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _error_cases as ec
from tests import _fixtures as fx

mpmath.mp.dps = 40


def _gamma_mp(model, m, d):
    d = mpmath.mpf(float(d))
    p = [mpmath.mpf(float(v)) for v in m]
    if model == "linear":
        return p[0] * d + p[1]
    if model == "power":
        return p[0] * d ** p[1] + p[2]
    psill, rng, nugget = p
    if model == "gaussian":
        return psill * (1 - mpmath.exp(-(d * d) / (rng * 4 / 7) ** 2)) + nugget
    if model == "exponential":
        return psill * (1 - mpmath.exp(-d / (rng / 3))) + nugget
    if model == "spherical":
        return psill * ((3 * d) / (2 * rng) - d ** 3 / (2 * rng ** 3)) + nugget if d <= rng else psill + nugget
    q = d / (rng / 3)
    return psill * (1 - (1 - q) * mpmath.exp(-q)) + nugget


def _mp_solve(st, d_st, bd, drift_st, drift_pts, values):
    """z, sigma^2 of the system from the same float64 distances / drift columns, solved in mpmath."""
    n, p = d_st.shape[0], drift_st.shape[1]
    M = n + p + 1
    a = mpmath.matrix(M, M)
    for i in range(n):
        for j in range(n):
            a[i, j] = 0 if i == j else -_gamma_mp(st.model, st.params, d_st[i, j])
        for k in range(p):
            a[i, n + k] = a[n + k, i] = mpmath.mpf(float(drift_st[i, k]))
        a[i, M - 1] = a[M - 1, i] = 1
    zs, sss = [], []
    for q in range(bd.shape[0]):
        b = mpmath.matrix(M, 1)
        for j in range(n):
            b[j] = 0 if (st.exact_values and abs(bd[q, j]) <= ko.EPS) else -_gamma_mp(st.model, st.params, bd[q, j])
        for k in range(p):
            b[n + k] = mpmath.mpf(float(drift_pts[q, k]))
        b[M - 1] = 1
        x = mpmath.lu_solve(a, b)
        zs.append(mpmath.fsum(x[j] * mpmath.mpf(float(values[j])) for j in range(n)))
        sss.append(-mpmath.fsum(x[j] * b[j] for j in range(M)))
    return zs, sss


def _small_cases():
    rng = np.random.default_rng(77)
    out = []
    for i, model in enumerate(["linear", "power", "gaussian", "spherical", "exponential", "hole-effect"]):
        n = 12 + 4 * i
        c = rng.random((n, 2))
        pts = rng.random((3, 2))
        pts[0] = c[0]  # an exact hit
        pts[1] = c[1] + [3e-11, 0.0]  # within EPS
        kw = {}
        if model == "gaussian":  # universal kriging with both drifts
            kw = dict(regional_linear=True, point_log=np.array([[0.3, 0.7, 1.0]]))
        out.append((model, ec._state(c, ec._field(c), model, ec.USER[model], exact=(i % 2 == 0), **kw), pts))
    c0 = rng.random((20, 3))
    c = ko.adjust_for_anisotropy(c0, c0.mean(0), [1.5, 0.7], [20.0, 10.0, 30.0])
    out.append(("3d", ec._state(c, ec._field(c0), "exponential", ec.USER["exponential"]), c[:1] + 0.01))
    lon, lat = rng.uniform(-180, 180, 24), rng.uniform(-89.9, 89.9, 24)
    out.append(("geographic", ec._state(np.stack([lon, lat], 1), np.sin(np.radians(lon)), "spherical", [1.0, 120.0, 0.05],
                                        geographic=True), np.array([[179.9, 10.0], [-179.95, 89.95]])))
    return out


@pytest.mark.parametrize("i", range(8))
def test_exact_reference_against_mpmath(i):
    """Relative agreement <= 1e3 u_longdouble cond_1(A) (relative to max|v| on z and to max|b| on sigma^2)."""
    name, st, pts = _small_cases()[i]
    r = ek.exact_points(st, pts)
    d_st, bd = ek.station_distances(st), ek.point_distances(st, pts)
    dr_st = ko._drift_columns(st, st.coords_adj, [])
    dr_pt = ko._drift_columns(st, pts, [])
    zm, sm = _mp_solve(st, d_st, bd, dr_st, dr_pt, st.values)
    tol = 1e3 * ek.U_LD * float(r.cond.max())
    for q in range(pts.shape[0]):
        assert abs(float(mpmath.mpf(str(r.z[q])) - zm[q])) <= tol * r.vscale[q], (name, q)
        assert abs(float(mpmath.mpf(str(r.ss[q])) - sm[q])) <= tol * r.bscale[q], (name, q)


def test_exact_moving_window_against_mpmath():
    """The moving window: each point's (k+1) system, its neighbours from cKDTree, in mpmath."""
    rng = np.random.default_rng(78)
    c = rng.random((40, 2))
    st = ec._state(c, ec._field(c), "exponential", ec.USER["exponential"])
    pts = np.concatenate([rng.random((3, 2)), c[:1]])
    k = 9
    r = ek.exact_moving_window(st, pts, k)
    bd, idx = ek.neighbours(st, pts, k)
    d_st = ek.station_distances(st)
    for q in range(pts.shape[0]):
        sub = ec._state(c[idx[q]], st.values[idx[q]], "exponential", ec.USER["exponential"])
        zm, sm = _mp_solve(sub, d_st[np.ix_(idx[q], idx[q])], bd[q:q + 1], np.zeros((k, 0)), np.zeros((1, 0)), st.values[idx[q]])
        tol = 1e3 * ek.U_LD * r.cond[q]
        assert abs(float(mpmath.mpf(str(r.z[q])) - zm[0])) <= tol * r.vscale[q]
        assert abs(float(mpmath.mpf(str(r.ss[q])) - sm[0])) <= tol * r.bscale[q]


@pytest.mark.filterwarnings("ignore::scipy.linalg.LinAlgWarning")
def test_refinement_refuses_what_it_cannot_refine():
    a = np.array([[1.0, 1.0], [1.0, 1.0 + 1e-17]], dtype=ek.LD)
    with pytest.raises(ek.RefinementError):
        ek.refined_solve(a, np.ones((2, 1), dtype=ek.LD))


@pytest.mark.parametrize("cid", ec.ids())
def test_float64_oracle_meets_the_bar(cid):
    """The float64 oracle (inverse + dgemm; dense solves per window) within the device's bar on every case of the GPU matrix,
    golden fixtures included."""
    c = ec.case(cid)
    z, ss = ec.oracle(c)
    rz, rs, _, _ = ec.ratios(c, z, ss)
    assert rz <= 1.0 and rs <= 1.0, (cid, rz, rs)


@pytest.mark.parametrize("k", sorted(ec.CUSTOM_KS))
def test_float64_oracle_meets_the_bar_on_the_custom_variogram_cases(k):
    """The CPU twin of test_custom_variogram_within_the_extended_precision_bar: the float64 oracle on the named exponential model
    meets the bar on the state the device's custom callable is held to -- and that callable is the named model, to rounding."""
    c = ec.custom_state(k)
    z, ss = ec.oracle(c)
    rz, rs, _, _ = ec.ratios(c, z, ss)
    assert rz <= 1.0 and rs <= 1.0, (k, rz, rs)
    d = np.linspace(0.0, 1.5, 301)
    assert np.allclose(ec.custom_exponential(ec.USER["exponential"], d), ko.variogram("exponential", c["st"].params, d), rtol=1e-15, atol=0)


def test_every_execute_fixture_is_in_the_matrix():
    have = {c["golden"] for c in ec.cases() if c["group"] == "golden"}
    assert have == {n for n in fx.names() if "z" in fx.load(n)}
