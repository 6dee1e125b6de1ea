"""Cases and references of the windowed cross-validation tests (tests/test_cross_validate_window.py on the GPU,
tests/test_cross_validate_window_host.py on the CPU).

A case builds a pykrige_amd object, the KrigingState of the same problem (tests/_cv_cases.state_of: the adjusted coordinates are the
object's own) and a window k.  The reference is brute force in extended precision: for every station i

    ek.exact_moving_window(cv.without(st, i), st.coords_adj[i:i + 1], k)

-- the state without station i, kriged at station i from its k nearest stations.  reference() computes exactly that, but assembles the
long-double station matrix of ALL stations once and cuts every local system out of it (an entry depends on its two stations alone)
instead of assembling N matrices of N - 1 stations; the neighbour sets and their float64 distances are ek.neighbours' on the state
without station i.  All N entries are compared, none is skipped.

Bars: ek.bars(ref, C_BAR) with cond_1 and order = k + 1 of each station's LOCAL system, the bar the moving-window cases of
tests/test_kernel_error_bounds.py use.

Station coordinates come from a seeded generator.  A seed is accepted only if no station's k-th and (k + 1)-th other neighbours are
closer than 1e-9 relative to each other, for every window the station set is used with (tests/_error_cases._no_ties' idea: the device
and cKDTree may break a distance tie differently); else the next seed is drawn.  The isolated coincident pair is a tie at distance 0
between a station's own index and its partner's, which leaving out by index resolves; the check looks at the OTHER stations only."""
import functools

import numpy as np

from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _cv_cases as cv
from tests import _error_cases as ec

TIE_GAP = 1e-9
ANISO3 = dict(anisotropy_scaling_y=1.5, anisotropy_scaling_z=0.7, anisotropy_angle_x=20.0, anisotropy_angle_y=10.0,
              anisotropy_angle_z=30.0)  # of _cv_cases._ok3d_gau


def no_ties(st, ks):
    """True if for every k of ks and every station the k-th and (k + 1)-th OTHER neighbours differ by more than TIE_GAP (relative)."""
    n = st.n
    for k in ks:
        if k + 1 > n - 1:  # k = N - 1: every other station is in the window, no (k + 1)-th exists
            continue
        for i in range(n):
            bd, _ = ek.neighbours(cv.without(st, i), st.coords_adj[i:i + 1], k + 1)
            if not bd[0, k] - bd[0, k - 1] > TIE_GAP * bd[0, k]:
                return False
    return True


def _draw(seed, build, ks):
    """The first seed from `seed` on whose station set has no tie at any window of ks: (object, state)."""
    for s in range(seed, seed + 20):
        obj = build(np.random.default_rng(s))
        st = cv.state_of(obj)
        if no_ties(st, ks):
            return obj, st
    raise AssertionError("no tie-free station set within 20 seeds of %d" % seed)


def _ok2d(model, params, n, scale=1.0, **kw):
    import pykrige_amd as pa

    def build(rng):
        c = rng.random((n, 2))
        return pa.OrdinaryKriging(c[:, 0], c[:, 1], scale * cv._field(c), variogram_model=model, variogram_parameters=params, **kw)

    return build


def _ok3d(n):
    import pykrige_amd as pa

    def build(rng):
        c = rng.random((n, 3))
        return pa.OrdinaryKriging3D(c[:, 0], c[:, 1], c[:, 2], cv._field(c), variogram_model="exponential",
                                    variogram_parameters=[1.0, 0.5, 0.02], **ANISO3)

    return build


def _geo(n):
    import pykrige_amd as pa

    def build(rng):
        lon, lat = rng.uniform(-30, 40, n), rng.uniform(20, 70, n)
        v = np.cos(np.radians(lat)) * np.sin(np.radians(2 * lon))
        return pa.OrdinaryKriging(lon, lat, v, variogram_model="exponential", variogram_parameters=[1.0, 40.0, 0.02],
                                  coordinates_type="geographic")

    return build


def _pair(exact):
    """60 stations in the unit square and two at exactly (10, 10) with different values: no third station's window of 8 holds the pair."""
    import pykrige_amd as pa

    def build(rng):
        c = np.concatenate([rng.random((60, 2)), [[10.0, 10.0], [10.0, 10.0]]])
        v = np.concatenate([cv._field(c[:60]), [0.7, -0.4]])
        return pa.OrdinaryKriging(c[:, 0], c[:, 1], v, variogram_model="exponential", variogram_parameters=[1.0, 0.5, 0.02],
                                  exact_values=exact)

    return build


# station set -> (first seed, builder, every window it is used with)
SETS = {
    "ok2d_exponential_n300": (2101, _ok2d("exponential", ec.USER["exponential"], 300), (10, 257)),
    "ok2d_spherical_n300": (2102, _ok2d("spherical", ec.USER["spherical"], 300), (16, 17)),
    "ok2d_gaussian_n450_values_1e3": (2103, _ok2d("gaussian", ec.USER["gaussian"], 450, scale=1e3), (100,)),
    "ok3d_exponential_aniso_n400": (2104, _ok3d(400), (24,)),
    "geographic_ok_n200": (2105, _geo(200), (12,)),
    "hole_effect_n200": (2106, _ok2d("hole-effect", ec.USER["hole-effect"], 200), (20, 130)),
    "ok2d_exponential_n12": (2107, _ok2d("exponential", ec.USER["exponential"], 12), (11,)),
    "pair_exact": (2108, _pair(True), (8,)),
    "pair_inexact": (2108, _pair(False), (8,)),
}
PAIR = (60, 61)  # the two coincident stations of the pair sets

# case -> (station set, window, the solver that has to run: mik_timing.mw_kernel)
CASES = {
    "exponential_n300_k10": ("ok2d_exponential_n300", 10, 1),          # multi-cell grid, lane search + todo, LDL^T class {4, 4}
    "spherical_n300_k16": ("ok2d_spherical_n300", 16, 1),              # the last window of the lane search
    "spherical_n300_k17": ("ok2d_spherical_n300", 17, 1),              # the first wave-only window
    "gaussian_n450_k100_values_1e3": ("ok2d_gaussian_n450_values_1e3", 100, 1),  # multi-cell at target 100, class {8, 13}
    "ok3d_exponential_aniso_n400_k24": ("ok3d_exponential_aniso_n400", 24, 1),    # the 3-D search
    "geographic_n200_k12": ("geographic_ok_n200", 12, 1),
    "hole_effect_n200_k20": ("hole_effect_n200", 20, 2),               # pivoting Gauss-Jordan
    "hole_effect_n200_k130": ("hole_effect_n200", 130, 3),             # k_mw_solve_big
    "exponential_n300_k257": ("ok2d_exponential_n300", 257, 4),        # blocked Cholesky on a one-cell grid: the plain scan with exclusion
    "exponential_n12_k11": ("ok2d_exponential_n12", 11, 1),            # k = N - 1: every other station, the search ends on `all`
    "pair_exact_k8": ("pair_exact", 8, 1),
    "pair_inexact_k8": ("pair_inexact", 8, 1),
}


@functools.lru_cache(maxsize=None)
def station_set(name):
    seed, build, ks = SETS[name]
    return _draw(seed, build, ks)


def case(name):
    """(object, state, k, mw_kernel)"""
    sname, k, kernel = CASES[name]
    obj, st = station_set(sname)
    return obj, st, k, kernel


def _reference(st, k):
    n = st.n
    a_all = ek.assemble(st, ek.station_distances(st))  # (n + 1) x (n + 1) long double, once
    out = ek.ExactResult(z=np.zeros(n, dtype=ek.LD), ss=np.zeros(n, dtype=ek.LD), cond=np.zeros(n), order=np.full(n, k + 1),
                         vscale=np.zeros(n), bscale=np.zeros(n))
    for i in range(n):
        bd, idx = ek.neighbours(cv.without(st, i), st.coords_adj[i:i + 1], k)
        bd, idx = bd[0], idx[0]
        idx = idx + (idx >= i)  # positions in the state without station i -> station indices
        sel = np.concatenate((idx, [n]))
        a = a_all[sel[:, None], sel]
        b = np.zeros(k + 1, dtype=ek.LD)
        b[:k] = -ek.variogram_ld(st.model, st.params, bd)
        if st.exact_values:
            b[:k][np.absolute(bd) <= ko.EPS] = 0
        b[k] = 1
        x, cond = ek.refined_solve(a, b[:, None].copy())
        v = st.values[idx]
        out.z[i], out.ss[i] = ek._reduce(st, x[:, 0], b, v)
        out.cond[i], out.vscale[i], out.bscale[i] = cond, float(np.abs(v).max()), float(np.abs(b[:k]).max())
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute-force reference of a case, computed once per session and shared."""
    _, st, k, _ = case(name)
    return _reference(st, k)
