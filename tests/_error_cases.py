"""The case matrix of the extended-precision error bounds (tests/test_kernel_error_bounds.py on the GPU,
tests/test_exact_reference.py on the CPU): kriging problems at the shapes, magnitudes and edges where kernels go wrong, each with
its exact answer (oracle/exact_kriging.py) cached for the session.

The moving window has four per-point solvers (timing()["mw_kernel"]), and each has its own groups: `mw` puts a window on both sides
of every LDL^T register class (1: k_mw_chol); `mw_piv` on both sides of the six Gauss-Jordan classes of dispatch_mw_solve (2:
k_mw_solve, nb = K + 1 <= 16, 32, 48, 64, 96, 128), of the hand-off to the scratch-slot LU at K = 127 | 128 (3: k_mw_solve_big) and
of the wrap of its 256-thread row strides at nb = 256 | 257; `mw_blocked` on the 64-wide panel edges of k_mw_chol_blocked (4:
K = 64 | 65, 128 | 129, 320 | 321, 384 | 385), a single panel, a mostly padded last panel and the shift it reduces across its four
wavefronts for the unbounded models.  Each solver also meets a 3-D and a geographic station set-up.  custom_problem / custom_state
are the custom-variogram problems that only the class API can carry (a Python callable, its K x K table gtab).

A case is a dict: group, name, st (KrigingState whose coords_adj are what the device is given), pts (adjusted points), k (moving
window size or None), opts (library options), sparse (expected value of timing()["sparse"], or None), mw_kernel (expected value of
timing()["mw_kernel"], or absent) and, for the golden fixtures, golden / sel (the fixture name and the grid cells compared)."""
import functools

import numpy as np

from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _fixtures as fx

C_BAR = 8.0  # the bar's constant: C u (cond_1(A) + M) max|v| on z, C u (cond_1(A) + M) max|b| on sigma^2


def _state(coords, values, model, user, exact=True, **kw):
    """A state whose adjusted coordinates are `coords` exactly (no anisotropy round trip): the device is handed the same numbers."""
    st = ko.KrigingState(ndim=coords.shape[1], coords_orig=coords, values=values, model=model,
                         params=ko.internal_parameters(model, user), scaling=[1.0] * (coords.shape[1] - 1),
                         angle=[0.0] * (2 * coords.shape[1] - 3), exact_values=exact, **kw)
    if not st.geographic:
        st.coords_adj = np.array(coords, dtype=np.float64)
        if st.point_log is not None:
            st.wells_adj = np.array(st.point_log, dtype=np.float64)
    return st


def _field(c):
    return np.sin(5 * c[:, 0]) * np.cos(3 * c[:, 1]) + 0.3 * c[:, -1]


USER = {"linear": [1.0, 0.05], "power": [1.0, 1.3, 0.05], "gaussian": [1.0, 0.5, 0.05], "spherical": [1.0, 0.6, 0.05],
        "exponential": [1.0, 0.5, 0.02], "hole-effect": [1.0, 0.5, 0.05]}
MODELS = ["exponential", "spherical", "gaussian", "linear", "power", "hole-effect"]


def _dense_cases():
    ns, npts, kinds = [15, 16, 17, 127, 128, 129, 255, 257], [1, 127, 128, 129, 257], ["ok", "uk", "ok3d"]
    out = []
    for i in range(16):
        n, npt, kind, model = ns[i % 8], npts[(i * 3) % 5], kinds[i % 3], MODELS[i % 6]
        factor, sym, tri, chunk = i % 3, (i // 3) % 2, (i // 2) % 2, 128 if (i // 4) % 2 else None
        if model == "hole-effect" and factor == 1:
            factor = 2  # the sweep may refuse a matrix that is not positive definite
        rng = np.random.default_rng(100 + i)
        if kind == "ok3d":
            c0 = rng.random((n, 3))
            c = ko.adjust_for_anisotropy(c0, c0.mean(0), [1.5, 0.7], [20.0, 10.0, 30.0])
            p = ko.adjust_for_anisotropy(rng.random((npt, 3)), c0.mean(0), [1.5, 0.7], [20.0, 10.0, 30.0])
            st = _state(c, _field(c0), model, USER[model])
        else:
            c, p = rng.random((n, 2)), rng.uniform(-0.05, 1.05, (npt, 2))
            kw = dict(regional_linear=True, point_log=np.array([[0.31, 0.72, 1.0], [0.66, 0.25, -0.5]])) if kind == "uk" else {}
            st = _state(c, _field(c), model, USER[model], **kw)
        opts = dict(factor=factor, symmetric=sym, tri=tri, sparse=0)
        if chunk:
            opts["chunk"] = chunk
        out.append(dict(group="dense", name="%s_%s_n%d_p%d_f%d_s%d_t%d_c%s" % (kind, model, n, npt, factor, sym, tri, chunk),
                        st=st, pts=p, k=None, opts=opts, sparse=0))
    return out


MAGNITUDES = {  # name -> (value scale, sill / nugget scale, coordinate offset, coordinate extent)
    "values_1e-9": (1e-9, 1.0, (0.0, 0.0), 1.0), "values_1e9": (1e9, 1.0, (0.0, 0.0), 1.0),
    "sill_1e-6": (1.0, 1e-6, (0.0, 0.0), 1.0), "sill_1e6": (1.0, 1e6, (0.0, 0.0), 1.0),
    "utm": (1.0, 1.0, (5e5, 4.1e6), 1e4), "extent_1e-5": (1.0, 1.0, (0.0, 0.0), 1e-5)}


def _magnitude_cases():
    out = []
    for j, (mname, (vs, ss, off, ext)) in enumerate(MAGNITUDES.items()):
        for path, model in (("dense", "exponential"), ("sparse", "spherical"), ("mw", "gaussian")):
            rng = np.random.default_rng(200 + 3 * j + len(path))
            u = rng.random((150, 2))
            c = u * ext + np.array(off)
            p = rng.uniform(0.0, 1.0, (64, 2)) * ext + np.array(off)
            user = list(USER[model])
            user[0], user[2], user[1] = user[0] * ss, user[2] * ss, user[1] * ext * (0.5 if path == "sparse" else 1.0)
            st = _state(c, _field(u) * vs, model, user)
            opts = {"sparse": 1 if path == "sparse" else 0}
            out.append(dict(group="magnitude", name="%s_%s" % (mname, path), st=st, pts=p, k=24 if path == "mw" else None,
                            opts=opts, sparse=1 if path == "sparse" else (0 if path == "dense" else None)))
    return out


def _ring(center, radius, nang, rng):
    a = rng.uniform(0, 2 * np.pi, nang)
    return center + radius * np.stack([np.cos(a), np.sin(a)], 1)


def _sparse_cases():
    out = []
    user = [1.0, 0.15, 0.02]
    for dd in (1e-2, 1e-4, 1e-5, 1e-8):
        # stations at range (1 - d) from the point, just inside the spherical range: four short segments across the four axis
        # directions, so that the bounding box of their K tiles is as far from the point as the nearest of them; five stations well
        # inside the range; the rest outside a disk of 1.3 range.  (One point: its 128-point block's box is the point itself.)
        rng = np.random.default_rng(int(-np.log10(dd)))
        q, r = np.array([0.5, 0.5]), 0.15
        t = np.linspace(-0.003, 0.003, 9) * r
        seg = [q + np.stack([np.full(9, r * (1 - dd)), t], 1) @ np.array(m) for m in
               ([[1, 0], [0, 1]], [[0, 1], [-1, 0]], [[-1, 0], [0, -1]], [[0, -1], [1, 0]])]
        far = rng.random((400, 2))
        far = far[np.linalg.norm(far - q, axis=1) > 1.3 * r][:150]
        near = q + rng.uniform(-0.06, 0.06, (5, 2))
        c = np.concatenate([near, far] + seg)
        st = _state(c, _field(c), "spherical", user)
        out.append(dict(group="sparse", name="near_range_%g" % dd, st=st, pts=q[None, :].copy(), k=None, opts={"sparse": 1}, sparse=1))
    rng = np.random.default_rng(7)
    c = rng.random((200, 2))
    pts = np.concatenate([rng.random((40, 2)), rng.uniform(2.0, 3.0, (24, 2))])  # the last 24 have no station in range
    out.append(dict(group="sparse", name="no_station_in_range", st=_state(c, _field(c), "spherical", user), pts=pts, k=None,
                    opts={"sparse": 1}, sparse=1))
    out.append(dict(group="sparse", name="range_beyond_domain", st=_state(c, _field(c), "spherical", [1.0, 5.0, 0.02]),
                    pts=rng.random((64, 2)), k=None, opts={"sparse": 1}, sparse=1))
    c0 = rng.random((300, 3))
    c = ko.adjust_for_anisotropy(c0, c0.mean(0), [1.3, 0.6], [15.0, 25.0, 35.0])
    p = ko.adjust_for_anisotropy(rng.random((96, 3)), c0.mean(0), [1.3, 0.6], [15.0, 25.0, 35.0])
    out.append(dict(group="sparse", name="aniso_3d", st=_state(c, _field(c0), "spherical", [1.0, 0.3, 0.02]), pts=p, k=None,
                    opts={"sparse": 1}, sparse=1))
    for rng_deg in (100.0, 170.0):  # geographic: longitudes across +-180, latitudes within 0.1 degree of the poles
        rng = np.random.default_rng(int(rng_deg))
        lon = np.concatenate([rng.uniform(170, 180, 40), rng.uniform(-180, -170, 40), rng.uniform(-180, 180, 80)])
        lat = np.concatenate([rng.uniform(-60, 60, 80), rng.uniform(89.9, 90.0, 40), rng.uniform(-90.0, -89.9, 40)])
        c = np.stack([lon, lat], 1)
        plon = np.concatenate([rng.uniform(175, 180, 12), rng.uniform(-180, -175, 12), rng.uniform(-180, 180, 24)])
        plat = np.concatenate([rng.uniform(-50, 50, 24), rng.uniform(89.9, 90, 12), rng.uniform(-90, -89.9, 12)])
        st = _state(c, np.sin(np.radians(lon)) * np.cos(np.radians(lat)), "spherical", [1.0, rng_deg, 0.02], geographic=True)
        out.append(dict(group="sparse", name="geographic_range_%g" % rng_deg, st=st, pts=np.stack([plon, plat], 1), k=None,
                        opts={"sparse": 1}, sparse=1))
    return out


# mw_chol_class's limits (mik_mw.hip: the {G, RI} register classes of k_mw_chol), 127 | 128 inside class {16, 8} and the hand-off to
# k_mw_chol_blocked at MIK_MW_CHOL_KMAX = 256 | 257
MW_LIMITS = [16, 24, 32, 40, 48, 52, 64, 80, 88, 96, 104, 112, 128, 144, 160, 176, 192, 208, 224, 256]
MW_KS = sorted(set([k for L in MW_LIMITS for k in (L, L + 1)] + [127]))


def _no_ties(st, pts, k):
    """Neighbour sets without a distance tie at the k-th station (the device and cKDTree may break one differently)."""
    bd, _ = ek.neighbours(st, pts, min(k + 1, st.n))
    if k < st.n:
        assert np.all(bd[:, k] - bd[:, k - 1] > 1e-12 * bd[:, k]), "distance tie at the k-th neighbour"


def _mw_cases():
    out = []
    mw_models = ["exponential", "spherical", "gaussian", "linear", "power"]
    for i, k in enumerate(MW_KS):
        model = mw_models[i % 5]
        rng = np.random.default_rng(300 + k)
        c = rng.random((300, 2))
        p = rng.random((6, 2))
        st = _state(c, _field(c), model, USER[model])
        _no_ties(st, p, k)
        out.append(dict(group="mw", name="k%d_%s" % (k, model), st=st, pts=p, k=k, opts={}, sparse=None, mw_kernel=1 if k <= 256 else 4))
    rng = np.random.default_rng(399)
    c = rng.random((200, 2))
    for name, model, opts in (("hole_effect", "hole-effect", {}), ("mw_pivot", "exponential", {"mw_pivot": 1}),
                              ("linear_utm", "linear", {}), ("power_utm", "power", {})):
        cc, user = c, USER[model]
        if name.endswith("utm"):  # the SPD-shifted systems of the unbounded models at a large coordinate extent
            cc, user = c * 1e4 + np.array([5e5, 4.1e6]), [user[0] * 1e-4] + user[1:]
        p = rng.random((12, 2)) * (cc.max(0) - cc.min(0)) + cc.min(0)
        st = _state(cc, _field(c), model, user)
        _no_ties(st, p, 30)
        out.append(dict(group="mw", name=name, st=st, pts=p, k=30, opts=opts, sparse=None, mw_kernel=1 if name.endswith("utm") else 2))
    lon, lat = rng.uniform(-180, 180, 300), rng.uniform(-85, 85, 300)
    st = _state(np.stack([lon, lat], 1), np.cos(np.radians(lat)) * np.sin(np.radians(2 * lon)), "exponential", [1.0, 40.0, 0.02],
                geographic=True)
    p = np.stack([np.concatenate([rng.uniform(175, 180, 4), rng.uniform(-180, -175, 4)]), rng.uniform(-80, 80, 8)], 1)
    _no_ties(st, p, 20)
    out.append(dict(group="mw", name="geographic", st=st, pts=p, k=20, opts={}, sparse=None, mw_kernel=1))
    return out


# dispatch_mw_solve's class limits are nb = K + 1 <= 16, 32, 48, 64, 96, 128 (k_mw_solve, mw_kernel 2); from K = 128 = MIK_MW_KMAX + 1
# the system lives in a scratch slot (k_mw_solve_big, mw_kernel 3), whose 256-thread strides over nb rows wrap at nb = 256 | 257
PIV_KS = [2, 15, 16, 31, 32, 47, 48, 63, 64, 95, 96, 127, 128, 129, 255, 256, 257]
HOLE_GEOGRAPHIC = [1.0, 40.0, 0.05]  # hole-effect parameters on the sphere (range in degrees)


def _piv_kernel(k):
    return 2 if k <= 127 else 3


def _piv_points(rng, c, draw, k):
    """19 points for k_mw_solve (its smallest class packs 16 per block: one full block and a partial one), 6 for k_mw_solve_big; the first
    two coincide with stations (the exact-hit rule through the pivoting solvers)."""
    p = draw(19 if _piv_kernel(k) == 2 else 6)
    p[:2] = c[rng.choice(c.shape[0], 2, replace=False)]
    return p


def _aniso3(rng, n):
    """3-D stations with anisotropy-adjusted coordinates as _dense_cases builds them: (original, adjusted, the adjustment)."""
    c0 = rng.random((n, 3))
    adj = lambda x: ko.adjust_for_anisotropy(x, c0.mean(0), [1.5, 0.7], [20.0, 10.0, 30.0])  # noqa: E731
    return c0, adj(c0), adj


def _globe(rng, n):
    """Stations all over the sphere as mw/geographic has them: (lon / lat columns, values)."""
    lon, lat = rng.uniform(-180, 180, n), rng.uniform(-85, 85, n)
    return np.stack([lon, lat], 1), np.cos(np.radians(lat)) * np.sin(np.radians(2 * lon))


def _across_antimeridian(rng, npt):
    h = npt // 2
    return np.stack([np.concatenate([rng.uniform(175, 180, h), rng.uniform(-180, -175, npt - h)]), rng.uniform(-80, 80, npt)], 1)


def _mw_piv_cases():
    out = []

    def add(name, st, p, k, opts=None):
        _no_ties(st, p, k)
        out.append(dict(group="mw_piv", name=name, st=st, pts=p, k=k, opts=opts or {}, sparse=None, mw_kernel=_piv_kernel(k)))

    for k in PIV_KS:  # hole-effect: no positive definite station block, hence pivoting by default
        rng = np.random.default_rng(600 + k)
        c = rng.random((300, 2))
        add("hole_k%d" % k, _state(c, _field(c), "hole-effect", USER["hole-effect"]), _piv_points(rng, c, lambda m: rng.random((m, 2)), k), k)
    for k in (16, 64, 128):
        rng = np.random.default_rng(900 + k)
        c0, c, adj = _aniso3(rng, 300)
        add("hole_3d_k%d" % k, _state(c, _field(c0), "hole-effect", USER["hole-effect"]),
            _piv_points(rng, c, lambda m: adj(rng.random((m, 3))), k), k)
    for k in (40, 130):
        rng = np.random.default_rng(1100 + k)
        c, v = _globe(rng, 300)
        add("hole_geographic_k%d" % k, _state(c, v, "hole-effect", HOLE_GEOGRAPHIC, geographic=True),
            _piv_points(rng, c, lambda m: _across_antimeridian(rng, m), k), k)
    for model, k in (("linear", 48), ("linear", 49), ("power", 128)):  # "mw_pivot": the unshifted systems of the unbounded models
        rng = np.random.default_rng(1300 + k)
        c = rng.random((300, 2))
        add("pivot_%s_k%d" % (model, k), _state(c, _field(c), model, USER[model]), _piv_points(rng, c, lambda m: rng.random((m, 2)), k), k,
            {"mw_pivot": 1})
    rng = np.random.default_rng(1500)
    u = rng.random((300, 2))
    c = u * 1e4 + np.array([5e5, 4.1e6])  # mw/linear_utm's offset and extent
    add("pivot_linear_utm_k96", _state(c, _field(u), "linear", [USER["linear"][0] * 1e-4] + USER["linear"][1:]),
        _piv_points(rng, c, lambda m: rng.random((m, 2)) * 1e4 + np.array([5e5, 4.1e6]), 96), 96, {"mw_pivot": 1})
    return out


# k_mw_chol_blocked (mw_kernel 4) pads the system to ldc = 64 ceil(K / 64): panel edges at K = 320 | 321 and 384 | 385 by default
# (K > 256); "mw_class" 1 sends smaller windows to it: the smallest it takes (8), a single panel (63, 64), a last panel of one real
# row (65, 129) and a full second one (128)
def _mw_blocked_cases():
    out = []
    bounded = ["exponential", "spherical", "gaussian"]

    def add(name, st, p, k, opts=None):
        _no_ties(st, p, k)
        out.append(dict(group="mw_blocked", name=name, st=st, pts=p, k=k, opts=opts or {}, sparse=None, mw_kernel=4))

    for i, (k, n, opts) in enumerate([(k, 450, {}) for k in (320, 321, 384, 385)] + [(k, 300, {"mw_class": 1}) for k in (8, 63, 64, 65, 128, 129)]):
        model = bounded[i % 3]
        rng = np.random.default_rng(1700 + k)
        c = rng.random((n, 2))
        add("%sk%d_%s" % ("class1_" if opts else "", k, model), _state(c, _field(c), model, USER[model]), rng.random((6, 2)), k, opts)
    for model in ("linear", "power"):  # no sill: the shift is 4 max gamma of the window, reduced across the four wavefronts
        rng = np.random.default_rng(1900 + len(model))
        c = rng.random((450, 2))
        add("k270_%s" % model, _state(c, _field(c), model, USER[model]), rng.random((6, 2)), 270)
    rng = np.random.default_rng(2100)
    c0, c, adj = _aniso3(rng, 450)
    add("k270_3d_spherical", _state(c, _field(c0), "spherical", USER["spherical"]), adj(rng.random((6, 3))), 270)
    rng = np.random.default_rng(2101)
    c, v = _globe(rng, 450)
    add("k270_geographic_exponential", _state(c, v, "exponential", [1.0, 40.0, 0.02], geographic=True), _across_antimeridian(rng, 6), 270)
    return out


# Custom variograms reach the device through the class API alone (a Python callable evaluated on the host; the K x K table gtab of a
# point's station pairs enters k_mw_solve and k_mw_solve_big): window size -> the solver it exercises
CUSTOM_KS = {31: 2, 32: 2, 130: 3}


def custom_exponential(p, d):
    """The reference's exponential model written out.  A custom model's parameter list is used as it is given (no sill - nugget)."""
    return p[0] * (1 - np.exp(-d / (p[1] / 3))) + p[2]


@functools.lru_cache(maxsize=None)
def custom_problem(k):
    """(stations, values, points) of the custom-variogram case at window k, as the user hands them to OrdinaryKriging; two of the
    points coincide with stations."""
    rng = np.random.default_rng(2300 + k)
    c = rng.random((300, 2))
    p = rng.random((19 if CUSTOM_KS[k] == 2 else 6, 2))
    p[:2] = c[rng.choice(300, 2, replace=False)]
    return c, _field(c), p


def custom_state(k, xa=None, ya=None):
    """The custom case at window k as a case of the NAMED exponential model with the callable's parameters, on the kriging object's
    adjusted station coordinates xa, ya (default: the oracle's own adjustment about the same centre), and the points adjusted the same way."""
    c, v, p = custom_problem(k)
    center = (c.max(0) + c.min(0)) / 2.0  # ok.py:276-277
    ca = ko.adjust_for_anisotropy(c, center, [1.0], [0.0]) if xa is None else np.stack([xa, ya], 1)
    st = _state(ca, v, "exponential", USER["exponential"])
    st.params = [float(x) for x in USER["exponential"]]
    pa = ko.adjust_for_anisotropy(p, center, [1.0], [0.0])
    _no_ties(st, pa, k)
    return dict(group="custom", name="exponential_k%d%s" % (k, "" if xa is None else "_object"), st=st, pts=pa, k=k, opts={}, sparse=None,
                mw_kernel=CUSTOM_KS[k])


HIT_DISTANCES = [0.0, 1e-12, 5e-11, 2e-10, 1e-8]  # none within a few ulps of EPS = 1e-10


def _exact_hit_cases():
    out = []
    rng = np.random.default_rng(500)
    c = rng.random((180, 2))
    for exact in (True, False):
        for path in ("dense", "sparse", "mw"):
            idx = rng.choice(180, 4 * len(HIT_DISTANCES), replace=False)
            ang = rng.uniform(0, 2 * np.pi, idx.size)
            dist = np.repeat(HIT_DISTANCES, 4)
            p = c[idx] + dist[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
            model = "spherical" if path == "sparse" else "exponential"
            user = [1.0, 0.3, 0.05] if path == "sparse" else USER[model]
            st = _state(c, _field(c), model, user, exact=exact)
            out.append(dict(group="exact_hit", name="%s_exact%d" % (path, exact), st=st, pts=p, k=16 if path == "mw" else None,
                            opts={"sparse": 1 if path == "sparse" else 0}, sparse=None if path == "mw" else int(path == "sparse")))
    return out


GOLDEN_POINTS = 96  # grid cells of a fixture compared against the exact reference (strided; 16 for the 2000-station fixture)


def _golden_cases():
    out = []
    for name in fx.names():
        g = fx.load(name)
        if "z" not in g:
            continue
        st = fx.state_from(name, g)
        args = fx.grid_args(g)
        if st.ndim == 2:
            gx, gy = np.meshgrid(*args)
            pts = np.stack([gx.ravel(), gy.ravel()], 1)
        else:
            gz, gy, gx = np.meshgrid(args[2], args[1], args[0], indexing="ij")
            pts = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1)
        m = 16 if st.n > 1000 else GOLDEN_POINTS
        sel = np.unique(np.linspace(0, pts.shape[0] - 1, min(m, pts.shape[0])).astype(int))
        pa = pts[sel] if st.geographic else ko.adjust_for_anisotropy(pts[sel], st.center, st.scaling, st.angle)
        spec = [np.asarray(s).ravel()[sel] for s in fx.spec_point_arrays(g)]
        out.append(dict(group="golden", name=name, st=st, pts=pa, k=None, opts={}, sparse=None, golden=name, sel=sel, spec=spec))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_dense_cases() + _magnitude_cases() + _sparse_cases() + _mw_cases() + _mw_piv_cases() + _mw_blocked_cases() +
                 _exact_hit_cases() + _golden_cases())


def case(name):
    return {c["group"] + "/" + c["name"]: c for c in cases()}[name]


def ids():
    return [c["group"] + "/" + c["name"] for c in cases()]


_EXACT = {}


def exact(c):
    """The exact answer of a case (cached for the session)."""
    key = c["group"] + "/" + c["name"]
    if key not in _EXACT:
        if c["k"] is None:
            _EXACT[key] = ek.exact_points(c["st"], c["pts"], c.get("spec", ()))
        else:
            _EXACT[key] = ek.exact_moving_window(c["st"], c["pts"], c["k"])
    return _EXACT[key]


def oracle(c):
    """The float64 oracle's answer of a case (inverse + dgemm; the moving window's dense solves)."""
    if c["k"] is None:
        return ko.solve_points(c["st"], c["pts"], c.get("spec", ()))
    return ko.solve_points_moving_window(c["st"], c["pts"], c["k"])


def ratios(c, z, ss):
    """(max |dz| / bar_z, max |dss| / bar_ss, the exact result, the bars) of float64 answers z, ss against the exact reference."""
    r = exact(c)
    bz, bs = ek.bars(r, C_BAR)
    dz = np.abs(np.asarray(z, dtype=np.float64).ravel().astype(ek.LD) - r.z).astype(np.float64)
    ds = np.abs(np.asarray(ss, dtype=np.float64).ravel().astype(ek.LD) - r.ss).astype(np.float64)
    return float((dz / bz).max()), float((ds / bs).max()), r, (bz, bs)
