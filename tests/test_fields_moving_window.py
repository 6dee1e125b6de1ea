"""execute_fields with n_closest_points: F value fields on one station set through the moving window (include/mikrige.h:
mik_set_fields + mik_predict_moving_window).

zvalues[f] must be execute(..., n_closest_points=k) of an object built from the same stations and values[:, f] with the same
(explicit) variogram; sigma^2 is this object's execute() sigma^2.  The neighbour search and the local right-hand sides run once; the
fields enter only the per-point solvers (k_mw_chol: up to G - 2 of them per pass as further right-hand-side rows, eliminated with the
arithmetic of the single value row), so every comparison below is bit for bit."""
import numpy as np
import pytest

import pykrige_amd as pa
from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from tests import _error_cases as ec


def _bits(a, b):
    a, b = np.ma.getdata(a), np.ma.getdata(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def _values(n, nf, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, nf)) + np.linspace(0, 3, nf)[None, :]


# ------------------------------------------------------------------------------------------------------------- CPU
def test_the_ordinary_classes_take_a_window_and_the_universal_ones_do_not():
    import inspect

    for cls in (pa.OrdinaryKriging, pa.OrdinaryKriging3D):
        assert "n_closest_points" in inspect.signature(cls.execute_fields).parameters, cls.__name__
        assert "n_closest_points" in cls.execute_fields.__doc__
    for cls in (pa.UniversalKriging, pa.UniversalKriging3D):
        assert "n_closest_points" not in inspect.signature(cls.execute_fields).parameters, cls.__name__
    rng = np.random.default_rng(3)
    x, y, v = rng.random(20), rng.random(20), rng.random(20)
    uk = _no_device(pa.UniversalKriging(x, y, v, variogram_model="linear", variogram_parameters=[1.0, 0.1],
                                        drift_terms=["regional_linear"]))
    with pytest.raises(TypeError):
        uk.execute_fields("points", [0.5], [0.5], np.zeros((20, 2)), n_closest_points=4)


def test_window_argument_errors_raise_before_any_device_call():
    rng = np.random.default_rng(0)
    n = 20
    ok = _no_device(pa.OrdinaryKriging(rng.random(n), rng.random(n), rng.random(n), variogram_model="linear",
                                       variogram_parameters=[1.0, 0.1]))
    ok3 = _no_device(pa.OrdinaryKriging3D(rng.random(n), rng.random(n), rng.random(n), rng.random(n), variogram_model="linear",
                                          variogram_parameters=[1.0, 0.1]))
    g = [0.0, 0.5, 1.0]
    good = np.zeros((n, 2))
    for obj, axes in ((ok, (g, g)), (ok3, (g, g, g))):
        for k in (1, 0, -3):
            with pytest.raises(ValueError, match="at least two"):
                obj.execute_fields("grid", *axes, good, backend="loop", n_closest_points=k)
        with pytest.raises(ValueError, match="moving window is not supported"):
            obj.execute_fields("grid", *axes, good, n_closest_points=4)  # backend 'vectorized'
        with pytest.raises(ValueError, match="exceeds the number of stations"):
            obj.execute_fields("grid", *axes, good, backend="loop", n_closest_points=n + 1)
        for bad, what in ((np.zeros((n - 1, 2)), "rows"), (np.zeros(n + 1), "rows"), (np.zeros((n, 0)), "F = 0"),
                          (np.zeros((n, 2, 1)), "dimensions")):
            with pytest.raises(ValueError, match=what):
                obj.execute_fields("grid", *axes, bad, backend="loop", n_closest_points=4)
        bad = good.copy()
        bad[3, 1] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            obj.execute_fields("points", *axes, bad, backend="hip", n_closest_points=4)
    with pytest.raises(ValueError, match="backend"):
        ok3.execute_fields("grid", g, g, g, good, backend="C", n_closest_points=4)  # ok3d.py has no C backend


def _bar_cases():
    """The extended-precision cases of the moving window with three fields each: 400 stations, 40 points of which 4 hit a station."""
    out = []
    spec = [("exponential", [1.0, 0.4, 0.02], 2, (10, 24, 100, 300)), ("spherical", [1.0, 0.7, 0.05], 2, (16, 60)),
            ("gaussian", [1.0, 0.5, 0.05], 3, (12, 40)), ("hole-effect", [1.0, 0.4, 0.05], 2, (10, 30))]
    for i, (model, user, nd, ks) in enumerate(spec):
        rng = np.random.default_rng(700 + i)
        c = rng.random((400, nd))
        p = rng.random((40, nd))
        p[:4] = c[[5, 77, 150, 333]]
        fields = np.stack([ec._field(c), 100.0 * rng.standard_normal(400), 2.5 + 1e-3 * c[:, 0]], 1)
        for k in ks:
            out.append(dict(name="%s_%dd_k%d" % (model, nd, k), model=model, user=user, coords=c, pts=p, k=k, fields=fields))
    return out


BAR_CASES = _bar_cases()


def _field_state(c, f):
    st = ec._state(c["coords"], c["fields"][:, f], c["model"], c["user"])
    ec._no_ties(st, c["pts"], c["k"])
    return st


@pytest.mark.parametrize("c", BAR_CASES, ids=[c["name"] for c in BAR_CASES])
def test_float64_oracle_meets_the_bar_on_every_field(c):
    """The bar of test_every_field_within_the_extended_precision_bar (GPU) is met by the float64 oracle field by field: it is not
    tuned to the kernels.  A RefinementError fails the test."""
    for f in range(c["fields"].shape[1]):
        st = _field_state(c, f)
        r = ek.exact_moving_window(st, c["pts"], c["k"])
        bz, bs = ek.bars(r, ec.C_BAR)
        z, ss = ko.solve_points_moving_window(st, c["pts"], c["k"])
        rz = float((np.abs(np.asarray(z, dtype=np.float64).astype(ek.LD) - r.z).astype(np.float64) / bz).max())
        rs = float((np.abs(np.asarray(ss, dtype=np.float64).astype(ek.LD) - r.ss).astype(np.float64) / bs).max())
        print("%s field %d: |dz| / bar %.3g, |dss| / bar %.3g" % (c["name"], f, rz, rs))
        assert rz <= 1.0 and rs <= 1.0, (c["name"], f, rz, rs)


# ------------------------------------------------------------------------------------------------------------- GPU
def _cls_g(k):
    """Thread-grid width G of the LDL^T class the window takes (k_mw_chol: G - 2 fields per pass); 4 for the other solvers."""
    if k <= 40 or 48 < k <= 52:
        return 4
    if k <= 104:
        return 8
    if k <= 224:
        return 16
    if k <= 256:
        return 32
    return 4


def _field_counts(g):
    return sorted({1, g - 2, g - 1, 2 * (g - 2) + 1, 37})


class MwCase:
    def __init__(self, name, cls, coords, kw, axes, pts, k, backends, opts=None):
        self.name, self.cls, self.coords, self.kw, self.axes, self.pts, self.k = name, cls, coords, kw, axes, pts, k
        self.backends, self.opts = backends, opts or {}

    def make(self, values):
        o = self.cls(*self.coords, values, **self.kw)
        if self.opts:
            h = o._get_handle()
            for key, val in self.opts.items():
                h.set_option(key, val)
        return o

    def args(self, style):
        rng = np.random.default_rng(7)
        if style == "points":
            return list(self.pts), {}
        kw = {}
        if style == "masked":
            shape = tuple(len(a) for a in reversed(self.axes))
            m = rng.random(shape) < 0.3
            m.flat[0] = True
            kw["mask"] = m
        return list(self.axes), kw


def _check_against_singles(case, values, field_counts, styles=("grid", "masked", "points")):
    obj = case.make(_values(len(case.coords[0]), 1, seed=99)[:, 0])
    nmax = max(field_counts)
    runs = [(s, b) for s in styles for b in case.backends]
    ref = {r: [] for r in runs}
    for f in range(nmax):  # one single-field object at a time (each holds a handle)
        single = case.make(values[:, f])
        for style, backend in runs:
            axes, kw = case.args(style)
            ref[(style, backend)].append(single.execute(style, *axes, backend=backend, n_closest_points=case.k, **kw))
        del single
    for style, backend in runs:
        axes, kw = case.args(style)
        zo, so = obj.execute(style, *axes, backend=backend, n_closest_points=case.k, **kw)
        for nf in field_counts:
            zf, sf = obj.execute_fields(style, *axes, values[:, :nf], backend=backend, n_closest_points=case.k, **kw)
            what = (case.name, style, backend, nf)
            assert zf.shape == (nf,) + zo.shape and sf.shape == so.shape, what
            assert type(zf) is type(zo) and type(sf) is type(so), what
            assert _bits(sf, so), what + ("sigma^2",)
            if style == "masked":
                assert np.array_equal(np.ma.getmaskarray(zf), np.broadcast_to(np.ma.getmaskarray(zo), zf.shape)), what
                assert not np.ma.getdata(zf)[np.broadcast_to(kw["mask"], zf.shape)].any(), what
            for f in range(nf):
                zr, sr = ref[(style, backend)][f]
                assert _bits(zf[f], zr), what + (f,)
                assert _bits(sf, sr), what + (f, "sigma^2 of the single")
    return obj


def _problem2(n=400, seed=11):
    rng = np.random.default_rng(seed)
    x, y = rng.random(n), rng.random(n)
    return (x, y), (np.linspace(0, 1, 23), np.linspace(0, 1, 17)), [rng.random(90), rng.random(90)]


def _window_cases():
    coords, axes, pts = _problem2()
    expo = dict(variogram_model="exponential", variogram_parameters=[1.0, 0.4, 0.02])
    out = []
    for k in (2, 10, 16, 24, 40, 52, 64, 100, 104, 112, 200, 250, 256, 300):
        out.append(MwCase("exponential_k%d" % k, pa.OrdinaryKriging, coords, expo, axes, pts, k, ("loop", "C", "hip")))
    hole = dict(variogram_model="hole-effect", variogram_parameters=[1.0, 0.4, 0.05])
    for k in (10, 130):
        out.append(MwCase("hole_effect_k%d" % k, pa.OrdinaryKriging, coords, hole, axes, pts, k, ("loop", "C", "hip")))
    custom = dict(variogram_model="custom", variogram_parameters=[1.0, 0.3],
                  variogram_function=lambda p, d: p[0] * (1.0 - np.exp(-d / p[1])))
    out.append(MwCase("custom_k10", pa.OrdinaryKriging, coords, custom, axes, pts, 10, ("loop", "C", "hip")))
    rng = np.random.default_rng(31)
    lon, lat = rng.random(400) * 60 - 30, rng.random(400) * 40 - 20
    geo = dict(variogram_model="exponential", variogram_parameters=[1.0, 20.0, 0.05], coordinates_type="geographic")
    out.append(MwCase("geographic_k12", pa.OrdinaryKriging, (lon, lat), geo, (np.linspace(-30, 30, 19), np.linspace(-20, 20, 13)),
                      [rng.random(90) * 60 - 30, rng.random(90) * 40 - 20], 12, ("loop", "C", "hip")))
    x3, y3, z3 = rng.random(400), rng.random(400), rng.random(400)
    k3 = dict(variogram_model="gaussian", variogram_parameters=[1.0, 0.5, 0.05], anisotropy_scaling_y=1.5, anisotropy_angle_z=30.0)
    for k in (12, 40):
        out.append(MwCase("ok3d_k%d" % k, pa.OrdinaryKriging3D, (x3, y3, z3), k3,
                          (np.linspace(0, 1, 11), np.linspace(0, 1, 9), np.linspace(0, 1, 5)),
                          [rng.random(90), rng.random(90), rng.random(90)], k, ("loop", "hip")))
    return out


WINDOW_CASES = _window_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("case", WINDOW_CASES, ids=lambda c: c.name)
def test_every_field_is_bit_for_bit_a_single_field_moving_window(case):
    values = _values(len(case.coords[0]), 61)
    obj = _check_against_singles(case, values, _field_counts(_cls_g(case.k)))
    # the solver that ran: 1 = k_mw_chol, 2 = k_mw_solve, 3 = k_mw_solve_big, 4 = k_mw_chol_blocked
    want = {"hole": 2 if case.k <= 127 else 3, "cust": 2}.get(case.name[:4], 1 if case.k <= 256 else 4)
    assert obj.last_timing["mw_kernel"] == want, (case.name, obj.last_timing["mw_kernel"])


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [{"mw_pivot": 1}, {"mw_lds_cap": 0}, {"mw_static": 0}, {"mw_static": 1}],
                         ids=["mw_pivot1", "mw_lds_cap0", "mw_static0", "mw_static1"])
def test_forced_options_keep_the_bits(opts):
    coords, axes, pts = _problem2(seed=13)
    kw = dict(variogram_model="spherical", variogram_parameters=[1.0, 0.7, 0.05])
    for k in (10, 64):
        case = MwCase("spherical_k%d" % k, pa.OrdinaryKriging, coords, kw, axes, pts, k, ("hip",), opts)
        obj = _check_against_singles(case, _values(400, 37, seed=3), _field_counts(_cls_g(k)))
        if "mw_pivot" in opts:
            assert obj.last_timing["mw_kernel"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("sort_points", [0, 1])
def test_sorted_points_keep_the_bits(sort_points):
    """A shuffled list of 6000 points at k <= 16: with "sort_points" the window runs in Hilbert-curve order and every plane is put back."""
    coords, axes, _ = _problem2(seed=17)
    rng = np.random.default_rng(23)
    pts = [rng.random(6000), rng.random(6000)]
    kw = dict(variogram_model="exponential", variogram_parameters=[1.0, 0.4, 0.02])
    for k in (10, 16):
        case = MwCase("sorted_k%d" % k, pa.OrdinaryKriging, coords, kw, axes, pts, k, ("hip",), {"sort_points": sort_points})
        obj = _check_against_singles(case, _values(400, 37, seed=4), (1, 2, 3, 37), styles=("points",))
        assert obj.last_timing["points_sorted"] == sort_points


@pytest.mark.gpu
def test_fields_are_independent_of_each_other_and_of_earlier_calls():
    coords, axes, pts = _problem2(seed=19)
    kw = dict(variogram_model="exponential", variogram_parameters=[1.0, 0.4, 0.02])
    values = _values(400, 37, seed=6)
    obj = pa.OrdinaryKriging(*coords, values[:, 0], **kw)
    for k in (10, 100, 200):
        z, s = obj.execute_fields("grid", *axes, values, backend="hip", n_closest_points=k)
        perm = np.random.default_rng(k).permutation(37)
        zp, sp = obj.execute_fields("grid", *axes, values[:, perm], backend="hip", n_closest_points=k)
        assert _bits(zp, z[perm]) and _bits(sp, s), k
        z1, _ = obj.execute_fields("grid", *axes, values[:, :1], backend="hip", n_closest_points=k)
        assert _bits(z1[0], z[0]), k

    def fresh():
        return pa.OrdinaryKriging(*coords, values[:, 0], **kw)

    # no state left behind: window fields, then a plain execute, then dense fields -- each the bits of a fresh object
    steps = [lambda o: o.execute_fields("points", *pts, values[:, :9], backend="hip", n_closest_points=24),
             lambda o: o.execute("points", *pts, backend="hip"),
             lambda o: o.execute_fields("points", *pts, values[:, :9], backend="hip"),
             lambda o: o.execute("points", *pts, backend="hip", n_closest_points=24)]
    for i, step in enumerate(steps):
        got, want = step(obj), step(fresh())
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), i


def _run_bar_case(c):
    from pykrige_amd import _lib

    st = _field_state(c, 0)
    h = _lib.Handle(0)
    try:
        h.set_problem(ndim=st.ndim, xs=st.coords_adj[:, 0], ys=st.coords_adj[:, 1], zs=st.coords_adj[:, 2] if st.ndim == 3 else None,
                      values=st.values, model_id=_lib.MODEL_IDS[st.model], params=st.params, exact_values=st.exact_values)
        p = c["pts"]
        h.set_points(p[:, 0], p[:, 1], p[:, 2] if st.ndim == 3 else None)
        h.set_fields(c["fields"].T)
        h.predict_moving_window(c["k"])
        zf = h.get_field_results()
        z0, ss = [np.array(a) for a in h.get_results()]
        assert _bits(z0, zf[0])  # the C ABI: mik_get_results returns field 0
    finally:
        h.close()
    return zf, ss


@pytest.mark.gpu
@pytest.mark.parametrize("c", BAR_CASES, ids=[c["name"] for c in BAR_CASES])
def test_every_field_within_the_extended_precision_bar(c):
    zf, ss = _run_bar_case(c)
    for f in range(c["fields"].shape[1]):
        r = ek.exact_moving_window(_field_state(c, f), c["pts"], c["k"])
        bz, bs = ek.bars(r, ec.C_BAR)
        rz = float((np.abs(zf[f].astype(ek.LD) - r.z).astype(np.float64) / bz).max())
        rs = float((np.abs(ss.astype(ek.LD) - r.ss).astype(np.float64) / bs).max())
        print("%s field %d: |dz| / bar %.3g, |dss| / bar %.3g" % (c["name"], f, rz, rs))
        assert rz <= 1.0 and rs <= 1.0, (c["name"], f, rz, rs)


@pytest.mark.gpu
def test_an_aliased_device_group_returns_the_bits_of_one_device():
    from pykrige_amd import _lib

    coords, axes, _ = _problem2(seed=51)
    rng = np.random.default_rng(52)
    values = _values(400, 15, seed=7)
    mask = rng.random((17, 23)) < 0.25
    kw = dict(variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02])
    one = pa.OrdinaryKriging(*coords, values[:, 0], **kw)
    grp = pa.OrdinaryKriging(*coords, values[:, 0], **kw)
    h = _lib.Handle(0)
    h.set_devices(2, alias=True)
    grp._handle = h
    for k in (10, 100):
        for style, extra in (("grid", {}), ("masked", {"mask": mask}), ("points", None)):
            args = axes if extra is not None else (rng.random(3000), rng.random(3000))
            z1, s1 = one.execute_fields(style, *args, values, backend="hip", n_closest_points=k, **(extra or {}))
            zg, sg = grp.execute_fields(style, *args, values, backend="hip", n_closest_points=k, **(extra or {}))
            assert _bits(z1, zg) and _bits(s1, sg), (k, style)
            assert np.array_equal(np.ma.getmaskarray(z1), np.ma.getmaskarray(zg))
    assert grp.last_timing["n_devices"] == 2


def _rank_problem():
    coords, axes, _ = _problem2(seed=91)
    rng = np.random.default_rng(92)
    return coords, _values(400, 9, seed=10), axes, rng.random((17, 23)) < 0.3


def _rank_worker(rank, world, port, q):
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import pykrige_amd as pa2
    from pykrige_amd import _lib
    from pykrige_amd.dist import ShardedExecutor, SocketGroup

    pg = SocketGroup(rank=rank, world=world, addr="127.0.0.1", port=port)
    try:
        coords, values, axes, mask = _rank_problem()
        ok = pa2.OrdinaryKriging(*coords, values[:, 0], variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02])
        ex = ShardedExecutor(ok, group=pg, use_rccl=False, handle_factory=lambda: _lib.Handle(0))
        out = []
        for style, kw in (("grid", {}), ("masked", {"mask": mask})):
            z, ss = ex.execute_fields(style, *axes, values=values, backend="hip", n_closest_points=12, **kw)
            out.append((np.ma.getdata(z).copy(), np.ma.getmaskarray(z).copy(), np.ma.getdata(ss).copy()))
        q.put((rank, out))
    finally:
        pg.close()


@pytest.mark.gpu
def test_ranks_return_the_bits_of_one_process():
    """ShardedExecutor at world 2 with the window: no factor, no exchange; the gathered planes are the bits of one process.  (Before the
    window reached execute_fields the keyword vanished in **kw and the ranks kriged without a window.)"""
    import multiprocessing as mp
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    coords, values, axes, mask = _rank_problem()
    ok = pa.OrdinaryKriging(*coords, values[:, 0], variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02])
    for i, (style, kw) in enumerate((("grid", {}), ("masked", {"mask": mask}))):
        z, ss = ok.execute_fields(style, *axes, values, backend="hip", n_closest_points=12, **kw)
        for rank in range(2):
            zr, mr, sr = res[rank][1][i]
            assert _bits(zr, z) and _bits(sr, ss) and np.array_equal(mr, np.ma.getmaskarray(z)), (style, rank)


@pytest.mark.gpu
def test_many_stations_many_fields():
    """300 000 stations, k = 12, 40 fields, 2e5 points: fields 0, 17 and 39 against single-field execute(), and field 17 on 256 points
    against cKDTree + a dense solve of the same (k + 1) x (k + 1) systems (test_hip_parity's check of the single-field window)."""
    import scipy.linalg
    from scipy.spatial import cKDTree

    rng = np.random.default_rng(2025)
    n, k, nf = 300000, 12, 40
    x, y = rng.random(n), rng.random(n)
    values = np.sin(9 * x)[:, None] * np.cos(7 * y)[:, None] + 0.05 * rng.standard_normal((n, nf))
    user = [1.0, 0.05, 0.01]
    kw = dict(variogram_model="exponential", variogram_parameters=user)
    px, py = rng.random(200000), rng.random(200000)
    ok = pa.OrdinaryKriging(x, y, values[:, 0], **kw)
    zf, ss = ok.execute_fields("points", px, py, values, backend="loop", n_closest_points=k)
    assert zf.shape == (nf, 200000)
    for f in (0, 17, 39):
        zs, s1 = pa.OrdinaryKriging(x, y, values[:, f], **kw).execute("points", px, py, backend="loop", n_closest_points=k)
        assert _bits(zf[f], zs) and _bits(ss, s1), f
    par = ko.internal_parameters("exponential", user)
    d, idx = cKDTree(np.stack([x, y], 1)).query(np.stack([px[:256], py[:256]], 1), k=k)
    v = values[:, 17]
    for i in range(256):
        sel = idx[i]
        c = np.stack([x[sel], y[sel]], 1)
        a = np.zeros((k + 1, k + 1))
        a[:k, :k] = -ko.variogram("exponential", par, np.linalg.norm(c[:, None] - c[None], axis=2))
        np.fill_diagonal(a, 0.0)
        a[k, :k] = a[:k, k] = 1.0
        b = np.append(-ko.variogram("exponential", par, d[i]), 1.0)
        w = scipy.linalg.solve(a, b)
        assert abs(zf[17][i] - w[:k] @ v[sel]) <= 1e-8 and abs(ss[i] + w @ b) <= 1e-6
