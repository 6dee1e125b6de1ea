"""execute_block without a GPU: the method exists on the four classes with the signature and the docstring the users read, every refusal
is raised before a handle is touched, mik_predict_block is declared and exported, the node offsets are GSLIB's, and the algebra the device
evaluates -- bbar = mean of the nodes' right-hand sides, z = c . bbar, sigma^2 = -gbar - bbar B bbar -- stays inside the bars the device is
held to, against the extended-precision brute force.

Also the home of what tests/test_execute_block.py (GPU) shares with this file: the blocks of a case, the cached brute-force reference and
its bars.  The reference: the raw nodes of every block through `adjusted`, ek.right_hand_sides averaged over the nodes in longdouble,
ek.refined_solve against ek.assemble, gbar in longdouble from the float64 distances of the adjusted offsets (0 where d <= ko.EPS).  The bar
of sigma^2 is execute_cov's, C_BAR u (cond_1(A) + M) bscale with bscale the largest |b| over the block's nodes, capped at
1e-6 max(1, max|sigma^2|); the bar of z is ek.bars' z bar."""
import functools
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from pykrige_amd import core
from tests import _cv_cases as cv
from tests import _error_cases as ec
from tests import test_execute_cov_host as ch
from tests.test_execute_cov_host import adjusted, points

ROOT = ch.ROOT
CLASSES = ch.CLASSES
CASES = sorted(n for n in cv.GLOBAL if "geographic" not in n)
P_BRUTE = 130  # two point blocks of 128
N_DISC = 3  # per axis: the centre node of a block on a station hits exact_values


# ------------------------------------------------------------------------------------------------------------- cases and references
def block_size(name):
    """About a twentieth of the station extent, unequal per axis."""
    _, st = cv.global_case(name)
    ext = st.coords_orig.max(axis=0) - st.coords_orig.min(axis=0)
    return tuple(float(v) for v in ext / 20.0 * np.array([1.0, 0.8, 1.25])[:st.ndim])


def per_axis(name, n):
    _, st = cv.global_case(name)
    return (n,) * st.ndim


def raw_nodes(name, n_disc, npt):
    """(npt, nd, ndim): the nodes of the blocks centred at the first npt of points(name), in the caller's coordinates."""
    _, st = cv.global_case(name)
    off = core.block_node_offsets(st.ndim, block_size(name), n_disc)
    return points(name)[:npt, None, :] + off[None, :, :]


def adjusted_offsets(name, n_disc):
    _, st = cv.global_case(name)
    return core.adjust_offsets(core.block_node_offsets(st.ndim, block_size(name), n_disc), st.ndim, st.scaling, st.angle)


@functools.lru_cache(maxsize=None)
def reference(name, n_disc, npt):
    """ek.ExactResult of the npt blocks: z, sigma^2 (longdouble), cond, order, vscale, bscale."""
    _, st = cv.global_case(name)
    nodes = raw_nodes(name, n_disc, npt)
    nd = nodes.shape[1]
    na = adjusted(st, nodes.reshape(-1, st.ndim))
    a = ek.assemble(st, ek.station_distances(st))
    b = ek.right_hand_sides(st, na, ek.point_distances(st, na)).reshape(npt, nd, a.shape[0])
    bbar = b.sum(axis=1) / ek.LD(nd)
    x, cond = ek.refined_solve(a, bbar.T.copy())
    d = ch.point_pair_distances(st, adjusted_offsets(name, n_disc))
    gam = ek.variogram_ld(st.model, st.params, d)
    gam[d <= ko.EPS] = 0
    gbar = gam.sum() / (ek.LD(nd) * ek.LD(nd))
    z = x.T[:, :st.n] @ st.values.astype(ek.LD)
    ss = -gbar - np.einsum("pi,pi->p", x.T, bbar)
    bscale = np.abs(b[:, :, :st.n]).max(axis=(1, 2)).astype(np.float64)
    return ek.ExactResult(z=z, ss=ss, cond=np.full(npt, cond), order=np.full(npt, a.shape[0]),
                          vscale=np.full(npt, float(np.abs(st.values).max())), bscale=bscale)


def bars(ref):
    """(z bar, sigma^2 bar) per block: ek.bars -- C_BAR u (cond + M) max|v| capped at 1e-8 max(1, max|z|), and C_BAR u (cond + M) bscale
    capped at 1e-6 max(1, max|sigma^2|)."""
    return ek.bars(ref, ec.C_BAR)


def worst_ratios(ref, z, ss):
    """max |z - ref| / bar and max |sigma^2 - ref| / bar over the leading len(z) blocks of ref."""
    z, ss = np.asarray(z, dtype=np.float64).ravel(), np.asarray(ss, dtype=np.float64).ravel()
    n = z.size
    bz, bs = bars(ref)
    dz = np.abs(z.astype(ek.LD) - ref.z[:n]).astype(np.float64)
    ds = np.abs(ss.astype(ek.LD) - ref.ss[:n]).astype(np.float64)
    return float((dz / bz[:n]).max()), float((ds / bs[:n]).max())


def restatement(name, n_disc, npt):
    """The device's stages in float64 NumPy: ko.rhs at the nodes summed in node order and divided once, np.linalg.inv."""
    _, st = cv.global_case(name)
    nodes = raw_nodes(name, n_disc, npt)
    nd = nodes.shape[1]
    na = adjusted(st, nodes.reshape(-1, st.ndim))
    b = ko.rhs(st, na).reshape(npt, nd, -1)
    bbar = b[:, 0, :].copy()
    for u in range(1, nd):
        bbar += b[:, u, :]
    bbar /= nd
    binv = np.linalg.inv(ko.kriging_matrix(st))
    binv = 0.5 * (binv + binv.T)
    d = ch.point_pair_distances(st, adjusted_offsets(name, n_disc))
    gbar = np.where(d <= ko.EPS, 0.0, ko.variogram(st.model, st.params, d)).sum() / float(nd * nd)
    z = bbar @ (binv[:, :st.n] @ st.values)
    ss = -np.einsum("pi,ij,pj->p", bbar, binv, bbar) - gbar
    return z, ss


# ------------------------------------------------------------------------------------------------------------- the interface
def test_the_four_classes_have_execute_block_with_the_documented_signature():
    for cls in CLASSES:
        sig = inspect.signature(cls.execute_block)
        coords = ["xpoints", "ypoints"] + (["zpoints"] if cls._ndim == 3 else [])
        assert list(sig.parameters) == ["self", "style"] + coords + ["block_size", "n_disc", "backend"], (cls, list(sig.parameters))
        assert sig.parameters["n_disc"].default == 4 and sig.parameters["backend"].default == "vectorized"
        assert sig.parameters["block_size"].default is inspect.Parameter.empty
        doc = " ".join(cls.execute_block.__doc__.split())
        for phrase in ("ARITHMETIC MEAN", "``execute_cov``'s matrix", "nugget", "averages down with ``nd``", "nd <= 512", "x fastest",
                       "((i + 0.5) / n - 0.5) L", "'masked'", "'geographic'", "pseudo_inv=True", "device group", "'custom'",
                       "NotImplementedError", "external_Z", "n_closest_points", "gamma*(d) = 0 if d <= eps"):
            assert phrase in doc, (cls.__name__, phrase)


def test_every_refusal_is_raised_before_any_device_call():
    for cls, obj, pts in ch._objects():
        with pytest.raises(ValueError, match="masked"):
            obj.execute_block("masked", *pts, 0.1)
        with pytest.raises(ValueError, match="style argument"):
            obj.execute_block("lattice", *pts, 0.1)
        with pytest.raises(ValueError, match="backend"):
            obj.execute_block("points", *pts, 0.1, backend="cuda")
        with pytest.raises(TypeError):
            obj.execute_block("points", *pts, 0.1, n_closest_points=4)
        with pytest.raises(TypeError):  # block_size has no default
            obj.execute_block("points", *pts)
        for bad in (0.0, -1.0, float("nan"), float("inf"), (0.1,) * (cls._ndim + 1), (0.1,) * (cls._ndim - 1), (0.1,) * (cls._ndim - 1) + (0.0,),
                    "wide"):
            with pytest.raises(ValueError, match="block_size"):
                obj.execute_block("points", *pts, bad)
        for bad in (0, -2, 2.5, (2,) * (cls._ndim + 1), (2,) * (cls._ndim - 1) + (0,), None):
            with pytest.raises(ValueError, match="n_disc"):
                obj.execute_block("points", *pts, 0.1, n_disc=bad)
        too_many = (23, 23) if cls._ndim == 2 else (9, 8, 8)  # 529 and 576 nodes
        with pytest.raises(ValueError, match="at most 512"):
            obj.execute_block("points", *pts, 0.1, n_disc=too_many)
        with pytest.raises(ValueError, match="same dimensions"):
            obj.execute_block("points", np.zeros(3), *[np.zeros(2) for _ in pts[1:]], 0.1)
    for cls, obj, pts in ch._objects(pseudo_inv=True):
        with pytest.raises(ValueError, match="pseudo_inv"):
            obj.execute_block("points", *pts, 0.1)
    for cls, obj, pts in ch._objects(variogram_model="custom", variogram_parameters=[1.0, 0.1], variogram_function=lambda p, d: p[0] * d + p[1]):
        with pytest.raises(NotImplementedError, match="custom"):
            obj.execute_block("points", *pts, 0.1)
    rng = np.random.default_rng(5)
    lon, lat, v = rng.uniform(0, 30, 20), rng.uniform(30, 60, 20), rng.random(20)
    geo = ch._no_device(pa.OrdinaryKriging(lon, lat, v, variogram_model="linear", variogram_parameters=[1.0, 0.1],
                                           coordinates_type="geographic"))
    with pytest.raises(ValueError, match="geographic"):
        geo.execute_block("points", np.array([10.0]), np.array([40.0]), 0.5)


def test_external_z_and_specified_drifts_are_not_built():
    rng = np.random.default_rng(2)
    n = 20
    x, y, z, v = rng.random(n), rng.random(n), rng.random(n), rng.random(n)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1])
    uk = ch._no_device(pa.UniversalKriging(x, y, v, drift_terms=["specified"], specified_drift=[rng.random(n)], **kw))
    ex = ch._no_device(pa.UniversalKriging(x, y, v, drift_terms=["external_Z"], external_drift=rng.random((5, 5)),
                                           external_drift_x=np.linspace(-0.5, 1.5, 5), external_drift_y=np.linspace(-0.5, 1.5, 5), **kw))
    uk3 = ch._no_device(pa.UniversalKriging3D(x, y, z, v, drift_terms=["specified"], specified_drift=[rng.random(n)], **kw))
    p = np.array([0.5, 0.25])
    for obj, pts in ((uk, (p, p)), (ex, (p, p)), (uk3, (p, p, p))):
        with pytest.raises(NotImplementedError, match="external_Z and specified"):
            obj.execute_block("points", *pts, 0.1)


def test_a_device_group_is_refused_before_the_device_is_touched():
    class Group:
        n_devices = 2

    for cls, obj, pts in ch._objects():
        obj._handle = Group()
        try:
            with pytest.raises(ValueError, match="device group of 2"):
                obj.execute_block("points", *pts, 0.1)
        finally:
            obj._handle = None


# ------------------------------------------------------------------------------------------------------------- the library
def test_library_declares_and_exports_mik_predict_block_at_abi_9():
    from pykrige_amd import _lib, build

    build.build_library()
    lib = _lib.load()
    assert lib.mik_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert hasattr(lib, "mik_predict_block") and "mik_predict_block" in _lib.SIGNATURES
    assert callable(getattr(_lib.Handle, "predict_block", None))
    header = open(os.path.join(ROOT, "include", "mikrige.h")).read()
    assert "int  mik_predict_block(mik_handle *h, const double *offsets /* nd x ndim, ADJUSTED */, int nd);" in header
    assert "mik_predict_block" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mik_predict_block" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_a_library_without_the_symbol_is_answered_as_stale(monkeypatch):
    from pykrige_amd import _lib

    real = _lib.load()

    class Old:
        def __getattr__(self, name):
            if name == "mik_predict_block":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mik_predict_block.*rebuild"):
        _lib.load()


# ------------------------------------------------------------------------------------------------------------- the nodes
def test_node_offsets_are_cell_centred_regular_and_x_fastest():
    assert np.array_equal(core.block_node_offsets(2, 3.0, 1), np.zeros((1, 2)))
    assert np.array_equal(core.block_node_offsets(3, (1.0, 2.0, 3.0), 1), np.zeros((1, 3)))
    assert np.array_equal(core.block_node_offsets(2, 2.0, 2), np.array([[-0.5, -0.5], [0.5, -0.5], [-0.5, 0.5], [0.5, 0.5]]))
    o3 = core.block_node_offsets(2, (3.0, 6.0), 3)
    assert o3.shape == (9, 2) and np.array_equal(o3[4], [0.0, 0.0])  # the centre node is exactly the centre
    assert np.allclose(o3[:3, 0], [-1.0, 0.0, 1.0], rtol=0, atol=1e-15) and np.all(o3[:3, 1] == o3[0, 1]) and np.isclose(o3[0, 1], -2.0)
    assert np.allclose(o3[::3, 1], [-2.0, 0.0, 2.0], rtol=0, atol=1e-15)
    o = core.block_node_offsets(3, (1.0, 2.0, 4.0), (2, 1, 3))  # per-axis sizes and counts
    assert o.shape == (6, 3)
    want = [(x, 0.0, z) for z in (-4.0 / 3.0, 0.0, 4.0 / 3.0) for x in (-0.25, 0.25)]
    assert np.allclose(o, want, rtol=0, atol=1e-15)
    for n, size in ((1, 0.7), (2, 0.7), (3, 0.7), ((3, 2), (0.7, 0.2))):
        o = core.block_node_offsets(2, size, n)
        nn, ss = (n, n) if np.ndim(n) == 0 else n, (size, size) if np.ndim(size) == 0 else size
        for k in range(2):
            assert np.allclose(np.unique(o[:, k]), ((np.arange(nn[k]) + 0.5) / nn[k] - 0.5) * ss[k], rtol=0, atol=1e-15)
        assert np.allclose(o.mean(axis=0), 0.0, atol=1e-16)
    assert core.block_node_offsets(3, 1.0, 8).shape == (512, 3)
    # the adjusted offsets are T u: the adjustment of centre + u minus the adjustment of the centre
    _, st = cv.global_case("ok3d_gaussian_aniso_n40")
    u = core.block_node_offsets(3, (0.1, 0.2, 0.3), 2)
    c = st.center + np.array([0.3, -0.2, 0.1])
    assert np.allclose(core.adjust_offsets(u, 3, st.scaling, st.angle), adjusted(st, c + u) - adjusted(st, c[None, :]), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("name", CASES)
def test_the_float64_restatement_of_the_stages_is_inside_the_bars(name):
    n_disc = per_axis(name, N_DISC)
    z, ss = restatement(name, n_disc, P_BRUTE)
    ref = reference(name, n_disc, P_BRUTE)
    rz, rs = worst_ratios(ref, z, ss)
    print("%s: worst err / bar z %.3g sigma^2 %.3g" % (name, rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)
    _, st = cv.global_case(name)
    assert st.exact_values
    # block kriging earns its keep: the variance of the mean is below the point variance at the centre, where that is not zero
    pt = ek.exact_points(st, adjusted(st, points(name)[:P_BRUTE]))
    off = [q for q in range(P_BRUTE) if q not in ch.ON_STATION]
    assert np.all(ref.ss[off] < pt.ss[off])
    # n_disc = 1 is the point problem
    one = reference(name, per_axis(name, 1), 9)
    bz, bs = bars(one)
    assert np.all(np.abs(one.z - pt.z[:9]).astype(np.float64) <= bz) and np.all(np.abs(one.ss - pt.ss[:9]).astype(np.float64) <= bs)
