"""Cases and references of the execute_fields_window tests (tests/test_fields_window_gaps.py on the GPU,
tests/test_fields_window_gaps_host.py on the CPU): value fields with missing stations through the moving window.

A case is a station set (the builders of tests/_cvw_cases.py), a window k, one `valid` column per pattern and about 200 query points in
the stations' bounding box plus six that sit exactly on stations: three the first gap pattern has and three it misses.  Every pattern
carries one field; the entries of `values` where `valid` is False are NaN, so an ignored value that reached a result would show.

The reference of field f is brute force in extended precision:

    ek.exact_moving_window(subset(st, valid[:, f], values[:, f]), adjusted query points, k)

-- the state restricted to the stations field f has (tests/_cv_cases.state_of plus a subset, as cv.without does for one station).  All
points of all fields are compared, none is skipped.  Bars: ek.bars(ref, C_BAR) with cond_1 and order = k + 1 of each point's LOCAL
system, the moving-window bar of tests/_cvw_cases.py.

Seeds.  Stations, patterns and query points come from one seeded generator.  A seed is accepted only if for every pattern and every
query point the k-th and (k + 1)-th nearest VALID stations differ by more than _cvw_cases.TIE_GAP (relative), for every window the set
is used with (the device and cKDTree may break a distance tie differently); the check is skipped where a pattern has exactly k valid
stations.  Else the next seed is drawn, 20 at the most."""
import dataclasses
import functools

import numpy as np

from oracle import exact_kriging as ek
from tests import _cv_cases as cv
from tests import _cvw_cases as cw
from tests import _error_cases as ec
from tests.test_fields_gaps_host import adjusted

N_RANDOM = 200  # query points besides the six on stations


def subset(st, keep, values=None):
    """The state of the stations keep (boolean, (N,)) alone: same centre, same adjusted coordinates, same order."""
    v = st.values if values is None else np.asarray(values, dtype=np.float64)
    r = dataclasses.replace(st, coords_orig=st.coords_orig[keep], values=v[keep], center=np.array(st.center, dtype=np.float64))
    r.coords_adj = st.coords_adj[keep]
    return r


# ------------------------------------------------------------------------------------------------------------- patterns
def _none(st, rng):
    return np.ones(st.n, dtype=bool)


def _random(share=None, count=None):
    def make(st, rng):
        m = np.ones(st.n, dtype=bool)
        m[rng.choice(st.n, size=count if count is not None else int(round(share * st.n)), replace=False)] = False
        return m

    return make


def _disc(radius):
    """Every station within `radius` of the middle of the stations' bounding box is missing."""
    def make(st, rng):
        mid = 0.5 * (st.coords_orig.min(axis=0) + st.coords_orig.max(axis=0))
        return np.linalg.norm(st.coords_orig - mid, axis=1) > radius

    return make


def _one_partner(st, rng):
    m = np.ones(st.n, dtype=bool)
    m[cw.PAIR[1]] = False  # the second station of the coincident pair
    m[5] = False           # and one elsewhere
    return m


# station set -> (first seed, builder, every window it is used with, patterns[, True: the coincident-pair set of _cvw_cases])
SETS = {
    "ok2d_exponential_n300": (4101, cw._ok2d("exponential", ec.USER["exponential"], 300), (10,), (_none, _random(share=0.05), _disc(0.2))),
    "ok2d_spherical_n300": (4102, cw._ok2d("spherical", ec.USER["spherical"], 300), (16, 17), (_random(share=0.10),)),
    "ok3d_exponential_aniso_n400": (4103, cw._ok3d(400), (24,), (_random(share=0.10),)),
    "geographic_ok_n200": (4104, cw._geo(200), (12,), (_random(share=0.10),)),
    "hole_effect_n200": (4105, cw._ok2d("hole-effect", ec.USER["hole-effect"], 200), (20,), (_random(share=0.10), _random(share=0.10))),
    "ok2d_exponential_n300_20_missing": (4106, cw._ok2d("exponential", ec.USER["exponential"], 300), (257,), (_random(count=20),)),
    "ok2d_exponential_n12": (4107, cw._ok2d("exponential", ec.USER["exponential"], 12), (8,), (_random(count=4),)),
    "pair_exact": (4108, cw._pair(True), (8,), (_one_partner,), True),
}

# case -> (station set, window, the solver that has to run: mik_timing.mw_kernel)
CASES = {
    "exponential_n300_k10": ("ok2d_exponential_n300", 10, 1),       # multi-cell grid (lane pass + todo list without a gap); no gap, 5 %, an emptied disc
    "spherical_n300_k16": ("ok2d_spherical_n300", 16, 1),           # the last lane window of the unmasked search
    "spherical_n300_k17": ("ok2d_spherical_n300", 17, 1),           # the first wave-only window
    "ok3d_exponential_aniso_n400_k24": ("ok3d_exponential_aniso_n400", 24, 1),
    "geographic_n200_k12": ("geographic_ok_n200", 12, 1),
    "hole_effect_n200_k20": ("hole_effect_n200", 20, 2),            # pivoting solver, one field per launch, two patterns
    "exponential_n300_k257": ("ok2d_exponential_n300_20_missing", 257, 4),  # one-cell grid: the plain scan under the mask, blocked Cholesky
    "exponential_n12_k8": ("ok2d_exponential_n12", 8, 1),           # exactly k valid stations: the search ends on `all`
    "pair_exact_k8": ("pair_exact", 8, 1),
}


@dataclasses.dataclass
class Drawn:
    obj: object
    st: object
    valid: np.ndarray    # (N, F) bool, one column per pattern
    values: np.ndarray   # (N, F), NaN where valid is False
    pts: np.ndarray      # (npt, ndim) query points in the caller's coordinates; the last six sit on stations
    on_valid: tuple      # stations (of the first gap pattern's valid ones) the points npt - 6 .. npt - 4 sit on
    on_missing: tuple    # stations that pattern misses, under the last three points


def tie_free(st, valid, pts_adj, ks):
    for f in range(valid.shape[1]):
        sub = subset(st, valid[:, f])
        for k in ks:
            if sub.n == k:  # every valid station is in the window
                continue
            bd, _ = ek.neighbours(sub, pts_adj, k + 1)
            if not np.all(bd[:, k] - bd[:, k - 1] > cw.TIE_GAP * bd[:, k]):
                return False
    return True


def _draw_one(seed, build, patterns, pair=False):
    rng = np.random.default_rng(seed)
    obj = build(rng)
    st = cv.state_of(obj)
    valid = np.stack([p(st, rng) for p in patterns], axis=1)
    gap = next(f for f in range(valid.shape[1]) if not valid[:, f].all())
    have, miss = np.flatnonzero(valid[:, gap]), np.flatnonzero(~valid[:, gap])
    on_valid = tuple(int(i) for i in have[[0, have.size // 2, have.size - 1]])
    on_missing = tuple(int(i) for i in miss[[0, miss.size // 2, miss.size - 1]])
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    if pair:  # the pair sits far outside the cloud: random points in the cloud, the pair among the stations
        lo, hi = st.coords_orig[:60].min(axis=0), st.coords_orig[:60].max(axis=0)
        on_valid = (on_valid[0], on_valid[1], cw.PAIR[0])
    pts = np.concatenate([lo + (hi - lo) * rng.random((N_RANDOM, st.ndim)), st.coords_orig[list(on_valid + on_missing)]])
    values = np.stack([(1.0 + 0.25 * f) * st.values + 0.1 * f for f in range(valid.shape[1])], axis=1)
    values[~valid] = np.nan
    return Drawn(obj, st, valid, values, pts, on_valid, on_missing)


@functools.lru_cache(maxsize=None)
def station_set(name):
    seed, build, ks, patterns = SETS[name][:4]
    for s in range(seed, seed + 20):
        d = _draw_one(s, build, patterns, pair=len(SETS[name]) > 4)
        if tie_free(d.st, d.valid, adjusted(d.st, d.pts), ks):
            return d
    raise AssertionError("no tie-free draw within 20 seeds of %d" % seed)


def case(name):
    """(Drawn, k, mw_kernel)"""
    sname, k, kernel = CASES[name]
    return station_set(sname), k, kernel


@functools.lru_cache(maxsize=None)
def reference(name):
    """One ek.ExactResult per field, computed once per session and shared."""
    d, k, _ = case(name)
    pa_ = adjusted(d.st, d.pts)
    return tuple(ek.exact_moving_window(subset(d.st, d.valid[:, f], d.values[:, f]), pa_, k) for f in range(d.valid.shape[1]))


def call(d, k, values=None, valid="case", style="points", axes=None, **kw):
    """obj.execute_fields_window at the case's points (or `axes`) for either class."""
    values = d.values if values is None else values
    valid = d.valid if isinstance(valid, str) else valid
    axes = [d.pts[:, i] for i in range(d.st.ndim)] if axes is None else axes
    return d.obj.execute_fields_window(style, *axes, values, k, valid=valid, **kw)
