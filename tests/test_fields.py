"""execute_fields: F value fields on one station set in one call (include/mikrige.h: mik_set_fields, mik_get_field_results).

zvalues[f] must be what execute() gives on an object built from the same stations and values[:, f], with the first object's
variogram given explicitly and every other constructor argument the same; sigma^2 is execute()'s.  On the device the fields share
the factor, the right-hand sides and the contraction, and each field's z is summed in the single-field order: the comparisons
below are bit for bit unless a test says otherwise."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = (pa.OrdinaryKriging, pa.UniversalKriging, pa.OrdinaryKriging3D, pa.UniversalKriging3D)
FC = 8  # fields per read-back pass of the device (MIK_FB)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_library_exports_the_field_entry_points():
    from pykrige_amd import build

    if not shutil.which("nm"):
        pytest.skip("binutils nm not on PATH")
    build.build_library()
    out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "mik_set_fields" in names and "mik_get_field_results" in names


def test_the_four_classes_have_execute_fields():
    for cls in CLASSES:
        assert callable(getattr(cls, "execute_fields", None)), cls.__name__
        assert "variogram is the object's" in cls.execute_fields.__doc__


def _no_device(obj):
    def boom():
        raise AssertionError("the device was touched before the arguments were checked")

    obj._get_handle = boom
    return obj


def _ok2d(n=20):
    rng = np.random.default_rng(0)
    return _no_device(pa.OrdinaryKriging(rng.random(n), rng.random(n), rng.random(n), variogram_model="linear",
                                         variogram_parameters=[1.0, 0.1]))


def test_argument_errors_raise_before_any_device_call():
    ok = _ok2d()
    g = [0.0, 0.5, 1.0]
    good = np.zeros((20, 2))
    for bad, what in ((np.zeros((19, 2)), "rows"), (np.zeros(21), "rows"), (np.zeros((20, 0)), "F = 0"),
                      (np.zeros((20, 2, 1)), "dimensions")):
        with pytest.raises(ValueError, match=what):
            ok.execute_fields("grid", g, g, bad)
    for v in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[3, 1] = v
        with pytest.raises(ValueError, match="non-finite"):
            ok.execute_fields("points", g, g, bad)
    with pytest.raises(ValueError, match="style"):
        ok.execute_fields("cells", g, g, good)
    with pytest.raises(ValueError, match="backend"):
        ok.execute_fields("grid", g, g, good, backend="cuda")
    with pytest.raises(ValueError):  # points of unequal length
        ok.execute_fields("points", g, g[:2], good)


def test_specified_drift_errors_raise_before_any_device_call():
    rng = np.random.default_rng(1)
    n = 15
    x, y, v = rng.random(n), rng.random(n), rng.random(n)
    uk = _no_device(pa.UniversalKriging(x, y, v, variogram_model="linear", variogram_parameters=[1.0, 0.1],
                                        drift_terms=["specified"], specified_drift=[x + y]))
    g = [0.0, 0.5, 1.0]
    vals = np.zeros((n, 3))
    with pytest.raises(ValueError):
        uk.execute_fields("grid", g, g, vals)  # no drift arrays
    with pytest.raises(ValueError):
        uk.execute_fields("grid", g, g, vals, specified_drift_arrays=[np.zeros((2, 2))])  # wrong shape
    with pytest.raises(ValueError):
        uk.execute_fields("points", g, g, vals, specified_drift_arrays=[np.zeros(4)])  # wrong length
    with pytest.raises(ValueError):
        uk.execute_fields("grid", g, g, vals, specified_drift_arrays=[np.zeros((3, 3)), np.zeros((3, 3))])  # too many terms
    z3 = rng.random(n)
    uk3 = _no_device(pa.UniversalKriging3D(x, y, z3, v, variogram_model="linear", variogram_parameters=[1.0, 0.1],
                                           drift_terms=["specified"], specified_drift=[x]))
    with pytest.raises(ValueError):
        uk3.execute_fields("points", g, g, g, vals, specified_drift_arrays=[np.zeros(2)])
    with pytest.raises(ValueError, match="rows"):
        uk3.execute_fields("points", g, g, g, vals[:-1], specified_drift_arrays=[np.zeros(3)])


# ------------------------------------------------------------------------------------------------------------- GPU helpers
def _bits(a, b):
    a, b = np.ma.getdata(a), np.ma.getdata(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _psill_dict(obj):
    p = [float(t) for t in obj.variogram_model_parameters]
    if obj.variogram_model == "linear":
        return {"slope": p[0], "nugget": p[1]}
    if obj.variogram_model == "power":
        return {"scale": p[0], "exponent": p[1], "nugget": p[2]}
    return {"psill": p[0], "range": p[1], "nugget": p[2]}


class Case:
    """One class set-up: how to build it from a value vector, and the execute arguments of each style."""

    def __init__(self, name, cls, coords, build_kw, ndim, axes, pts, spec=None):
        self.name, self.cls, self.coords, self.kw, self.ndim, self.axes, self.pts, self.spec = name, cls, coords, build_kw, ndim, axes, pts, spec

    def make(self, values, params=None):
        kw = dict(self.kw)
        if params is not None:
            kw["variogram_parameters"] = params
        return self.cls(*self.coords, values, **kw)

    def args(self, style):
        rng = np.random.default_rng(7)
        if style == "points":
            return list(self.pts), {}, (len(self.pts[0]),)
        shape = tuple(len(a) for a in reversed(self.axes))
        kw = {}
        if style == "masked":
            m = rng.random(shape) < 0.3
            m.flat[0] = True
            kw["mask"] = m
        return list(self.axes), kw, shape

    def spec_kw(self, style, shape):
        if self.spec is None:
            return {}
        return {"specified_drift_arrays": [self.spec(style, shape)]}


def _cases():
    rng = np.random.default_rng(11)
    n = 140
    x, y, z = rng.random(n), rng.random(n), rng.random(n)
    gx, gy, gz = np.linspace(0, 1, 23), np.linspace(0, 1, 17), np.linspace(0, 1, 7)
    p2 = [rng.random(90), rng.random(90)]
    p3 = [rng.random(90), rng.random(90), rng.random(90)]
    expo = {"sill": 1.0, "range": 0.4, "nugget": 0.02}

    def spec(style, shape):
        if style == "points":
            return p2[0] * 0.5 + p2[1]
        yy, xx = np.meshgrid(gy, gx, indexing="ij")
        return xx * 0.5 + yy

    return [
        Case("ok2d_aniso_fitted", pa.OrdinaryKriging, (x, y), dict(variogram_model="exponential", anisotropy_scaling=1.7,
                                                                   anisotropy_angle=25.0), 2, (gx, gy), p2),
        Case("uk2d_regional_linear_point_log", pa.UniversalKriging, (x, y),
             dict(variogram_model="exponential", variogram_parameters=expo, drift_terms=["regional_linear", "point_log"],
                  point_drift=np.array([[0.3, 0.4, 0.5], [1.4, -0.2, 0.2]])), 2, (gx, gy), p2),
        Case("uk2d_specified", pa.UniversalKriging, (x, y), dict(variogram_model="gaussian", variogram_parameters=expo,
                                                                 drift_terms=["specified"], specified_drift=[x * 0.5 + y]),
             2, (gx, gy), p2, spec=spec),
        Case("uk2d_functional", pa.UniversalKriging, (x, y), dict(variogram_model="power", variogram_parameters=[1.0, 1.3, 0.0],
                                                                  drift_terms=["functional"], functional_drift=[lambda a, b: a * b]),
             2, (gx, gy), p2),
        Case("ok3d_aniso", pa.OrdinaryKriging3D, (x, y, z), dict(variogram_model="exponential", variogram_parameters=[1.0, 0.6, 0.05],
                                                                 anisotropy_scaling_y=1.5, anisotropy_scaling_z=0.8,
                                                                 anisotropy_angle_z=30.0), 3, (gx, gy, gz), p3),
        Case("uk3d_aniso_rl", pa.UniversalKriging3D, (x, y, z), dict(variogram_model="linear", variogram_parameters=[1.0, 0.01],
                                                                     anisotropy_scaling_z=2.0, anisotropy_angle_x=15.0,
                                                                     drift_terms=["regional_linear"]), 3, (gx, gy, gz), p3),
    ]


def _values(n, nf, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, nf)) + np.linspace(0, 3, nf)[None, :]


def _check_against_singles(case, obj, values, styles=("grid", "masked", "points"), field_counts=(1, 3, FC, FC + 1, 37)):
    params = _psill_dict(obj)
    singles = [case.make(values[:, f], params) for f in range(values.shape[1])]
    for style in styles:
        axes, kw, shape = case.args(style)
        kw.update(case.spec_kw(style, shape))
        ref = [s.execute(style, *axes, **kw) for s in singles]
        zo, so = obj.execute(style, *axes, **kw)
        for nf in field_counts:
            zf, sf = obj.execute_fields(style, *axes, values[:, :nf], **kw)
            assert zf.shape == (nf,) + zo.shape and sf.shape == so.shape, (case.name, style, nf)
            assert type(zf) is type(zo) and type(sf) is type(so), (case.name, style, nf)
            assert _bits(sf, so), (case.name, style, nf, "sigma^2")
            if style == "masked":
                assert np.array_equal(np.ma.getmaskarray(zf), np.broadcast_to(np.ma.getmaskarray(zo), zf.shape))
                assert not np.ma.getdata(zf)[np.broadcast_to(kw["mask"], zf.shape)].any()
            for f in range(nf):
                assert _bits(zf[f], ref[f][0]), (case.name, style, nf, f)
                assert _bits(sf, ref[f][1]), (case.name, style, nf, f, "sigma^2 of the single")


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.name)
def test_every_field_is_bit_for_bit_a_single_field_execute_dense(case):
    n = len(case.coords[0])
    values = _values(n, 37)
    obj = case.make(_values(n, 1, seed=99)[:, 0])  # the object's own values (and, without parameters, the fitted variogram)
    _check_against_singles(case, obj, values)
    assert obj.last_timing["sparse"] == 0  # (the spherical model takes the range-aware path: the next test)


@pytest.mark.gpu
@pytest.mark.parametrize("sort_points", [0, 1])
def test_every_field_is_bit_for_bit_a_single_field_execute_range_aware(sort_points):
    """Spherical model, enough stations for the range-aware contraction: field 0 is kriged with the right-hand sides, the others
    read the candidate tiles of the same panel back in the same lane order."""
    rng = np.random.default_rng(21)
    n = 700
    x, y = rng.random(n), rng.random(n)
    gx, gy = np.linspace(0, 1, 70), np.linspace(0, 1, 66)
    case = Case("ok2d_spherical_sparse", pa.OrdinaryKriging, (x, y), dict(variogram_model="spherical",
                                                                          variogram_parameters=[1.0, 0.12, 0.01]),
                2, (gx, gy), [rng.random(5000), rng.random(5000)])
    values = _values(n, FC + 3)

    def make(v, params=None):
        o = case.cls(x, y, v, **dict(case.kw, **({} if params is None else {"variogram_parameters": params})))
        o._get_handle().set_option("sort_points", sort_points)
        return o

    case.make = make
    obj = make(values[:, 0] * 0.5)
    _check_against_singles(case, obj, values, styles=("grid", "points"), field_counts=(1, FC + 3))
    t = obj.last_timing
    assert t["sparse"] == 1 and t["points_sorted"] == sort_points


@pytest.mark.gpu
def test_geographic_custom_pseudo_inverse_and_exact_values_agree_with_single_fields():
    rng = np.random.default_rng(31)
    n = 120
    lon, lat = rng.random(n) * 60 - 30, rng.random(n) * 40 - 20
    x, y = rng.random(n), rng.random(n)
    xd, yd = np.concatenate([x, x[:5]]), np.concatenate([y, y[:5]])  # duplicated stations: a singular matrix
    cases = [
        (pa.OrdinaryKriging, (lon, lat), dict(variogram_model="exponential", variogram_parameters=[1.0, 20.0, 0.05],
                                              coordinates_type="geographic"), (np.linspace(-30, 30, 19), np.linspace(-20, 20, 13))),
        (pa.OrdinaryKriging, (x, y), dict(variogram_model="custom", variogram_parameters=[1.0, 0.3],
                                          variogram_function=lambda p, d: p[0] * (1.0 - np.exp(-d / p[1])))
         , (np.linspace(0, 1, 21), np.linspace(0, 1, 11))),
        (pa.OrdinaryKriging, (xd, yd), dict(variogram_model="linear", variogram_parameters=[1.0, 0.1], pseudo_inv=True),
         (np.linspace(0, 1, 21), np.linspace(0, 1, 11))),
        (pa.UniversalKriging, (x, y), dict(variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.1],
                                           exact_values=False, drift_terms=["regional_linear"]),
         (np.concatenate([x[:10], np.linspace(0, 1, 11)]), np.linspace(0, 1, 9))),
    ]
    for cls, coords, kw, axes in cases:
        m = len(coords[0])
        values = _values(m, 10)
        obj = cls(*coords, values[:, 9], **kw)
        zf, sf = obj.execute_fields("grid", *axes, values[:, :9])
        for f in range(9):
            z1, s1 = cls(*coords, values[:, f], **kw).execute("grid", *axes)
            scale = max(1.0, float(np.abs(np.ma.getdata(z1)).max()))
            assert float(np.abs(np.ma.getdata(zf[f]) - np.ma.getdata(z1)).max()) <= 1e-12 * scale, (kw, f)
            assert float(np.abs(np.ma.getdata(sf) - np.ma.getdata(s1)).max()) <= 1e-12 * max(1.0, float(np.abs(s1).max())), (kw, f)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ok2d", "uk2d"])
def test_fields_against_the_oracle(kind):
    from oracle import kriging_oracle as ko

    rng = np.random.default_rng(41)
    n = 80
    x, y = rng.random(n), rng.random(n)
    values = _values(n, 5)
    gx, gy = np.linspace(0, 1, 25), np.linspace(0, 1, 19)
    x[:4], y[:4] = gx[[1, 5, 9, 20]], gy[[2, 3, 11, 18]]  # stations on grid nodes: the exact-hit rule
    params = [1.0, 0.35, 0.05]
    if kind == "ok2d":
        obj = pa.OrdinaryKriging(x, y, values[:, 0], variogram_model="spherical", variogram_parameters=params)
        st = dict(ndim=2, coords_orig=np.stack([x, y], 1), model="spherical", params=ko.internal_parameters("spherical", params))
    else:
        obj = pa.UniversalKriging(x, y, values[:, 0], variogram_model="spherical", variogram_parameters=params,
                                  drift_terms=["regional_linear"])
        st = dict(ndim=2, coords_orig=np.stack([x, y], 1), model="spherical", params=ko.internal_parameters("spherical", params),
                  regional_linear=True)
    zf, sf = obj.execute_fields("grid", gx, gy, values)
    for f in range(5):
        zr, sr = ko.execute(ko.KrigingState(values=values[:, f], **st), "grid", gx, gy)
        assert float(np.abs(np.ma.getdata(zf[f]) - zr).max()) <= 1e-8, f
        assert float(np.abs(np.ma.getdata(sf) - sr).max()) <= 1e-6, f


@pytest.mark.gpu
def test_fields_against_the_reference_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "fields", "ok2d.npz")) as g:
        g = {k: g[k] for k in g.files}
    params = {"sill": float(g["sill"]), "range": float(g["range"]), "nugget": float(g["nugget"])}
    ok = pa.OrdinaryKriging(g["x"], g["y"], g["values"][:, 0], variogram_model="exponential", variogram_parameters=params)
    zf, sf = ok.execute_fields("grid", g["gx"], g["gy"], g["values"])
    assert zf.shape == g["z"].shape
    assert float(np.abs(np.ma.getdata(zf) - g["z"]).max()) <= 1e-8
    assert float(np.abs(np.ma.getdata(sf) - g["ss"]).max()) <= 1e-6


@pytest.mark.gpu
def test_an_aliased_device_group_returns_the_bits_of_one_device():
    from pykrige_amd import _lib

    rng = np.random.default_rng(51)
    n = 200
    x, y = rng.random(n), rng.random(n)
    values = _values(n, 9)
    gx, gy = np.linspace(0, 1, 61), np.linspace(0, 1, 47)
    mask = rng.random((47, 61)) < 0.25
    kw = dict(variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02])
    one = pa.OrdinaryKriging(x, y, values[:, 0], **kw)
    grp = pa.OrdinaryKriging(x, y, values[:, 0], **kw)
    h = _lib.Handle(0)
    h.set_devices(2, alias=True)
    grp._handle = h
    for style, extra in (("grid", {}), ("masked", {"mask": mask}), ("points", None)):
        args = (gx, gy) if extra is not None else (rng.random(3000), rng.random(3000))
        z1, s1 = one.execute_fields(style, *args, values, **(extra or {}))
        zg, sg = grp.execute_fields(style, *args, values, **(extra or {}))
        assert _bits(z1, zg) and _bits(s1, sg), style
        assert np.array_equal(np.ma.getmaskarray(z1), np.ma.getmaskarray(zg))
    assert grp.last_timing["n_devices"] == 2


@pytest.mark.gpu
def test_a_reused_handle_gives_the_bits_of_fresh_objects():
    from pykrige_amd import _lib

    rng = np.random.default_rng(61)
    n = 150
    x, y = rng.random(n), rng.random(n)
    values = _values(n, 12)
    gx, gy = np.linspace(0, 1, 31), np.linspace(0, 1, 29)
    kw = dict(variogram_model="gaussian", variogram_parameters=[1.0, 0.3, 0.05])
    obj = pa.OrdinaryKriging(x, y, values[:, 0], **kw)

    def fresh(nf):
        o = pa.OrdinaryKriging(x, y, values[:, 0], **kw)
        return o.execute_fields("grid", gx, gy, values[:, :nf]) if nf else o.execute("grid", gx, gy)

    for nf in (3, 0, 11, 0, 1):
        got = obj.execute_fields("grid", gx, gy, values[:, :nf]) if nf else obj.execute("grid", gx, gy)
        want = fresh(nf)
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), nf
    # the C ABI: with fields set, mik_get_results returns field 0; nf = 0 gives back the plain handle
    h = _lib.Handle(0)
    obj2 = pa.OrdinaryKriging(x, y, values[:, 5], **kw)
    obj2._handle = h
    z_plain, s_plain = [np.array(a) for a in obj2.execute("points", gx[:29], gy)]
    h.set_fields(values[:, [2, 7]].T)
    h.predict()
    zf = h.get_field_results()
    z0, s0 = [np.array(a) for a in h.get_results()]
    z2, _ = [np.array(a) for a in pa.OrdinaryKriging(x, y, values[:, 2], **kw).execute("points", gx[:29], gy)]
    assert _bits(z0, z2) and _bits(zf[0], z2) and _bits(s0, s_plain)
    h.set_fields(None)
    h.predict()
    z1, s1 = [np.array(a) for a in h.get_results()]
    assert _bits(z1, z_plain) and _bits(s1, s_plain)
    with pytest.raises(RuntimeError, match="no fields"):
        h._fields = 1
        h.get_field_results()


# ------------------------------------------------------------------------------------------------------------- several launches
def _optioned(cls, coords, kw, opts):
    def make(v, params=None):
        o = cls(*coords, v, **dict(kw, **({} if params is None else {"variogram_parameters": params})))
        h = o._get_handle()
        for k, val in opts.items():
            h.set_option(k, val)
        return o

    return make


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [{"chunk": 1024}], ids=["one_panel"])
def test_fields_over_several_launches_dense(opts):
    """Several launches of 1024 points: the planes of every field at each launch's offset."""
    rng = np.random.default_rng(71)
    n = 160
    x, y = rng.random(n), rng.random(n)
    case = Case("ok2d_chunks", pa.OrdinaryKriging, (x, y), dict(variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02]),
                2, (np.linspace(0, 1, 61), np.linspace(0, 1, 47)), [rng.random(3000), rng.random(3000)])
    case.make = _optioned(pa.OrdinaryKriging, (x, y), case.kw, opts)
    values = _values(n, FC + 3, seed=8)
    obj = case.make(values[:, 0] * 0.25)
    _check_against_singles(case, obj, values, field_counts=(FC + 3, 2))
    t = obj.last_timing
    assert t["contract_launches"] >= 3 and t["rhs_overlapped"] == 0 and t["sparse"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("sort_points", [0, 1])
def test_fields_over_several_launches_range_aware(sort_points):
    """Range-aware path over five launches: two lanes (the odd launches on the second stream), with and without the point sort; a second
    call with other fields on the same resident set-up."""
    rng = np.random.default_rng(81)
    n = 700
    x, y = rng.random(n), rng.random(n)
    case = Case("ok2d_spherical_chunks", pa.OrdinaryKriging, (x, y), dict(variogram_model="spherical",
                                                                          variogram_parameters=[1.0, 0.12, 0.01]),
                2, (np.linspace(0, 1, 70), np.linspace(0, 1, 66)), [rng.random(5000), rng.random(5000)])
    case.make = _optioned(pa.OrdinaryKriging, (x, y), case.kw, {"chunk": 1024, "sort_points": sort_points})
    values = _values(n, FC + 3, seed=9)
    obj = case.make(values[:, 0] * 0.5)
    _check_against_singles(case, obj, values, styles=("grid", "points"), field_counts=(FC + 3,))
    _check_against_singles(case, obj, values[:, ::-1].copy(), styles=("points",), field_counts=(FC + 1,))
    t = obj.last_timing
    assert t["sparse"] == 1 and t["points_sorted"] == sort_points and t["contract_launches"] >= 4


def _rank_worker(rank, world, port, q):
    import sys

    sys.path.insert(0, ROOT)
    import pykrige_amd as pa2
    from pykrige_amd import _lib
    from pykrige_amd.dist import ShardedExecutor, SocketGroup

    pg = SocketGroup(rank=rank, world=world, addr="127.0.0.1", port=port)
    try:
        x, y, values, gx, gy, mask = _rank_problem()
        ok = pa2.OrdinaryKriging(x, y, values[:, 0], variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02])
        ex = ShardedExecutor(ok, group=pg, use_rccl=False, handle_factory=lambda: _lib.Handle(0))
        out = []
        for style, kw in (("grid", {}), ("masked", {"mask": mask})):
            z, ss = ex.execute_fields(style, gx, gy, values=values, **kw)
            out.append((np.ma.getdata(z).copy(), np.ma.getmaskarray(z).copy(), np.ma.getdata(ss).copy()))
        zl, sl, (lo, hi) = ShardedExecutor(ok, group=pg, use_rccl=False, handle_factory=lambda: _lib.Handle(0),
                                           gather="local").execute_fields("points", gx[:40], gy[:40], values=values)
        q.put((rank, out, (zl.copy(), sl.copy(), lo, hi)))
    finally:
        pg.close()


def _rank_problem():
    rng = np.random.default_rng(91)
    n = 180
    x, y = rng.random(n), rng.random(n)
    gx, gy = np.linspace(0, 1, 53), np.linspace(0, 1, 41)
    return x, y, _values(n, 9, seed=10), gx, gy, rng.random((41, 53)) < 0.3


@pytest.mark.gpu
def test_ranks_return_the_bits_of_one_process():
    """pykrige_amd.dist: two ranks (one process each) shard the points; every rank forms C from its own inverse and kriges every field on
    its slab.  The gathered planes are the bits of one process's execute_fields."""
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
    x, y, values, gx, gy, mask = _rank_problem()
    ok = pa.OrdinaryKriging(x, y, values[:, 0], variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.02])
    for i, (style, kw) in enumerate((("grid", {}), ("masked", {"mask": mask}))):
        z, ss = ok.execute_fields(style, gx, gy, values, **kw)
        for rank in range(2):
            zr, mr, sr = res[rank][1][i]
            assert _bits(zr, z) and _bits(sr, ss) and np.array_equal(mr, np.ma.getmaskarray(z)), (style, rank)
    zp, sp = ok.execute_fields("points", gx[:40], gy[:40], values)
    for rank in range(2):
        zl, sl, lo, hi = res[rank][2]
        assert zl.shape == (9, hi - lo)
        assert _bits(zl, np.ma.getdata(zp)[:, lo:hi]) and _bits(sl, np.ma.getdata(sp)[lo:hi]), rank
