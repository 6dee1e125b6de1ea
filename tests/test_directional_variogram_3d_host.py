"""directional_variogram_3d / variogram_map_3d without a GPU: the module and the two 3-D classes carry the signatures and docstrings the
users read, every refusal is raised before ctypes loads anything, include/mikvario3.h declares what libmikvario3.so exports and the ctypes
mirror agrees with it, the two other libraries hold nothing of the third, and a float64 NumPy restatement of the definitions agrees with the
extended-precision brute force inside the bars the device is held to.

Also the home of what tests/test_directional_variogram_3d.py (GPU) shares with this file: the station sets, the brute force and the bars.

The brute force evaluates the definitions of include/mikvario3.h over all pairs i < j in np.longdouble, from the float64 unit vectors that
cross the C ABI and the host's float64 tan2 / bw2 (variography3d.decision_constants) -- the numbers the device decides from.  It also
returns the MARGIN: the smallest relative distance of any pair to any decision boundary (a bin edge |d - e| / max(d, e); the tolerance cone
|across2 - along^2 tan2| / max of the two; the bandwidth |across2 - bw2| / max of the two; a cell border of the map, in cells).  A
coincident pair (dx = dy = dz = 0 exactly) sits on the boundaries it touches in every arithmetic and is left out of the margin.  Exact
counts are demanded only of inputs whose margin is >= 1e-9: every input of INPUTS / MAP_INPUTS is asserted to keep it, here, on the CPU
(test_every_input_keeps_its_margin; the smallest recorded: 6.0e-7 of relative distance, 8.9e-7 of a cell).

Bars: counts equal; |sum - ref| <= (count + 8) 2^-52 ref per bin -- the terms are non-negative, so any summation order of `count` terms
with a few roundings each stays inside (d in 3-D has one more square and one more add than in 2-D: 2 more roundings of the 8)."""
import ctypes
import functools
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import core
from pykrige_amd import variography3d as v3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = 2.0 ** -52
MARGIN = 1e-9
SIZES = (2, 63, 64, 65, 129, 600)
AZIMUTHS = (0.0, 30.0, 90.0, 135.0, 60.0, 0.0)
DIPS = (0.0, 0.0, 0.0, 20.0, -35.0, 90.0)
DIRS = v3.direction_vectors(AZIMUTHS, DIPS)
ANGLES = (20.0, 10.0, 30.0)  # a candidate rotation: its three axes are mutually perpendicular


# ------------------------------------------------------------------------------------------------------------- inputs
def stations(n, nf=1, seed=0, coincident=0, flat=False):
    """n random stations in a 10 x 7 x 4 box with nf fields (n, nf); the last `coincident` stations repeat the first ones; flat: all z
    equal."""
    rng = np.random.default_rng(9000 + 13 * n + seed)
    x, y, z = 10.0 * rng.random(n), 7.0 * rng.random(n), 4.0 * rng.random(n)
    v = np.sin(0.7 * x)[:, None] * np.cos(0.5 * y)[:, None] + 0.4 * z[:, None] + 0.3 * rng.standard_normal((n, nf))
    for k in range(coincident):
        x[n - 1 - k], y[n - 1 - k], z[n - 1 - k] = x[k], y[k], z[k]
    if flat:
        z[:] = 1.25
    return x, y, z, v


def edges_of(nlags, maxlag=6.0):
    return np.linspace(0.0, maxlag, nlags + 1)


def limit_directions():
    """16 directions: a spiral over the upper hemisphere."""
    k = np.arange(v3.MAXDIRS)
    return v3.direction_vectors(47.0 * k, 5.5 * k)


# name -> (stations kwargs, directions (A, 3), tolerance, bandwidth, edges): every directional input the GPU file compares with the brute force
INPUTS = {}
for _n in SIZES:
    INPUTS["n%d" % _n] = (dict(n=_n), DIRS, 22.5, None, edges_of(7))
    INPUTS["n%d_bandwidth" % _n] = (dict(n=_n), DIRS, 22.5, 0.8, edges_of(7))
INPUTS["partition_n129"] = (dict(n=129, coincident=2), core.anisotropy_axes(ANGLES), 35.0, None, edges_of(7))
INPUTS["omni_n129"] = (dict(n=129, coincident=2), DIRS[3:4], 90.0, None, edges_of(7))
INPUTS["axial_n129"] = (dict(n=129), np.vstack([DIRS[3], -DIRS[3], DIRS[4], -DIRS[4]]), 22.5, None, edges_of(7))
for _f in (1, 8, 9, 17):
    INPUTS["fields_f%d" % _f] = (dict(n=129, nf=_f, seed=1), DIRS, 22.5, None, edges_of(7))
INPUTS["coincident_n65"] = (dict(n=65, coincident=1), DIRS, 22.5, 0.8, edges_of(7))  # one coincident pair among 63 other stations
INPUTS["limits_n129"] = (dict(n=129, seed=2), limit_directions(), 22.5, None, edges_of(v3.MAXLAGS, 9.0))
INPUTS["flat_n129"] = (dict(n=129, seed=3, flat=True), v3.direction_vectors((0.0, 30.0, 90.0, 135.0), (0.0,) * 4), 22.5, 0.8, edges_of(7))
# name -> (stations kwargs, nx, ny, nz, dx, dy, dz): 3 x 5 x 3 cells and 17 x 17 x 13 = 3757 cells
MAP_INPUTS = {}
for _n in (65, 600):
    MAP_INPUTS["map_n%d_3x5x3" % _n] = (dict(n=_n, nf=2, coincident=1), 1, 2, 1, 2.5, 1.1, 1.2)
    MAP_INPUTS["map_n%d_17x17x13" % _n] = (dict(n=_n, nf=2, coincident=1), 8, 8, 6, 0.55, 0.4, 0.3)
MAP_INPUTS["map_flat_n129_9x7x1"] = (dict(n=129, nf=2, seed=3, flat=True), 4, 3, 0, 0.9, 1.1, 1.0)


# ------------------------------------------------------------------------------------------------------------- brute force
def _pairs(x, y, z, v, dtype):
    i, j = np.triu_indices(len(x), 1)
    x, y, z, v = (np.asarray(a, dtype=dtype) for a in (x, y, z, v))
    dx, dy, dz = x[j] - x[i], y[j] - y[i], z[j] - z[i]
    dv = v[i] - v[j]
    return dx, dy, dz, np.sqrt(dx * dx + dy * dy + dz * dz), dtype(0.5) * (dv * dv)


def _rel(a, b):
    m = np.maximum(np.abs(a), np.abs(b))
    return np.where(m > 0, np.abs(a - b) / np.where(m > 0, m, 1), np.inf)


def membership(dx, dy, dz, dirs, tol, bandwidth, dtype=LD):
    """(member (A, pairs) bool, margin) of the direction rule: across2 <= (along*along) * tan2 and across2 <= bw2."""
    tan2, bw2 = v3.decision_constants(tol, bandwidth)
    apart = ~((dx == 0) & (dy == 0) & (dz == 0))
    member = np.ones((len(dirs), dx.size), dtype=bool)
    margin = np.inf
    for a, (ux, uy, uz) in enumerate(np.asarray(dirs, dtype=np.float64)):
        ux, uy, uz = dtype(ux), dtype(uy), dtype(uz)
        along = dx * ux + dy * uy + dz * uz
        cx, cy, cz = dy * uz - dz * uy, dz * ux - dx * uz, dx * uy - dy * ux
        across2 = cx * cx + cy * cy + cz * cz
        if tol != 90.0:
            cone = (along * along) * dtype(tan2)
            member[a] &= across2 <= cone
            if apart.any():
                margin = min(margin, float(_rel(across2[apart], cone[apart]).min()))
        if bandwidth is not None:
            member[a] &= across2 <= dtype(bw2)
            if apart.any():
                margin = min(margin, float(_rel(across2[apart], dtype(bw2)).min()))
    return member, margin


def directional_sums(x, y, z, v, dirs, tol, bandwidth, edges, dtype=LD):
    """(counts (A, B) int64, lag sums (A, B), semi sums (F, A, B), margin) from the definitions, in `dtype`."""
    edges = np.asarray(edges, dtype=np.float64)
    dx, dy, dz, d, g = _pairs(x, y, z, v, dtype)
    apart = ~((dx == 0) & (dy == 0) & (dz == 0))
    na, nb, nf = len(dirs), len(edges) - 1, g.shape[1]
    counts = np.zeros((na, nb), dtype=np.int64)
    lag, semi = np.zeros((na, nb), dtype=dtype), np.zeros((nf, na, nb), dtype=dtype)
    e = edges.astype(dtype)
    member, margin = membership(dx, dy, dz, dirs, tol, bandwidth, dtype)
    if apart.any():
        margin = min(margin, float(min(_rel(d[apart], ek).min() for ek in e)))
    for b in range(nb):
        inbin = (d >= e[b]) & (d < e[b + 1])
        for a in range(na):
            sel = member[a] & inbin
            counts[a, b] = int(sel.sum())
            lag[a, b] = d[sel].sum(dtype=dtype)
            semi[:, a, b] = g[sel].sum(axis=0, dtype=dtype)
    return counts, lag, semi, margin


def map_sums(x, y, z, v, nx, ny, nz, cdx, cdy, cdz, dtype=LD):
    """(counts (2nz+1, 2ny+1, 2nx+1) int64, semi sums (F, ...), margin in cells): every pair into its cell and the mirror cell."""
    dx, dy, dz, _, g = _pairs(x, y, z, v, dtype)
    u = [h / dtype(c) + dtype(0.5) for h, c in ((dx, cdx), (dy, cdy), (dz, cdz))]
    q = [np.floor(t) for t in u]
    margin = float(min(np.minimum(t - f, f + 1 - t).min() for t, f in zip(u, q)))
    inside = (np.abs(q[0]) <= nx) & (np.abs(q[1]) <= ny) & (np.abs(q[2]) <= nz)
    ix, iy, iz = ((m + f[inside]).astype(np.int64) for m, f in zip((nx, ny, nz), q))
    shape = (2 * nz + 1, 2 * ny + 1, 2 * nx + 1)
    counts = np.zeros(shape, dtype=np.int64)
    semi = np.zeros((g.shape[1],) + shape, dtype=dtype)
    for sz, sy, sx in ((iz, iy, ix), (2 * nz - iz, 2 * ny - iy, 2 * nx - ix)):
        np.add.at(counts, (sz, sy, sx), 1)
        for f in range(g.shape[1]):
            np.add.at(semi[f], (sz, sy, sx), g[inside, f])
    return counts, semi, margin, int(inside.sum())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute force of INPUTS[name]: (counts, lag sums, semi sums, margin), computed once and shared; do not write into it."""
    kw, dirs, tol, bw, edges = INPUTS[name]
    x, y, z, v = stations(**kw)
    return directional_sums(x, y, z, v, dirs, tol, bw, edges)


@functools.lru_cache(maxsize=None)
def map_reference(name):
    """(counts, semi sums, margin in cells, pairs inside the map)."""
    kw, nx, ny, nz, cdx, cdy, cdz = MAP_INPUTS[name]
    x, y, z, v = stations(**kw)
    return map_sums(x, y, z, v, nx, ny, nz, cdx, cdy, cdz)


def worst_ratio(total, ref, counts):
    """max |total - ref| / ((count + 8) 2^-52 ref) over the bins with pairs (0 where both sums are 0); sums of empty bins must be 0."""
    total, ref = np.asarray(total, dtype=LD), np.asarray(ref, dtype=LD)
    counts = np.broadcast_to(counts, ref.shape)
    assert np.all(total[counts == 0] == 0)
    bar = (counts + 8) * LD(U) * np.abs(ref)
    err = np.abs(total - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def mean_ratio(mean, ref_sum, counts):
    """The same bar on the means the Python layer returns (sum / count: one more rounding, inside the + 8); NaN exactly where count is 0."""
    counts = np.broadcast_to(counts, np.shape(ref_sum))
    mean = np.asarray(mean, dtype=np.float64)
    assert np.array_equal(np.isnan(mean), counts == 0)
    return worst_ratio(np.where(counts > 0, mean, 0.0).astype(LD) * counts, ref_sum, counts)


# ------------------------------------------------------------------------------------------------------------- the interface
def test_signatures_and_docstrings():
    sig = inspect.signature(v3.directional_variogram_3d)
    assert list(sig.parameters) == ["x", "y", "z", "values", "azimuths", "dips", "directions", "tolerance", "nlags", "maxlag", "edges",
                                    "bandwidth"]
    assert [sig.parameters[k].default for k in ("azimuths", "dips", "directions", "tolerance", "nlags", "maxlag", "edges", "bandwidth")] \
        == [None, None, None, 22.5, 6, None, None, None]
    assert list(inspect.signature(v3.variogram_map_3d).parameters) == ["x", "y", "z", "values", "nx", "ny", "nz", "dx", "dy", "dz"]
    assert list(inspect.signature(v3.direction_vectors).parameters) == ["azimuths", "dips"]
    assert list(inspect.signature(core.anisotropy_axes).parameters) == ["angle"]
    for cls in (pa.OrdinaryKriging3D, pa.UniversalKriging3D):
        sig = inspect.signature(cls.directional_variogram_3d)
        assert list(sig.parameters) == ["self", "azimuths", "dips", "directions", "tolerance", "nlags", "maxlag", "edges", "bandwidth"]
        assert sig.parameters["tolerance"].default == 22.5 and sig.parameters["nlags"].default == 6
        assert sig.parameters["azimuths"].default is None and sig.parameters["directions"].default is None
        assert list(inspect.signature(cls.variogram_map_3d).parameters) == ["self", "nx", "ny", "nz", "dx", "dy", "dz"]
        for fn in (cls.directional_variogram_3d, cls.variogram_map_3d):
            doc = " ".join(fn.__doc__.split())
            for phrase in ("BEFORE the anisotropy adjustment", "device group", "2-D object", "ValueError"):
                assert phrase in doc, (cls.__name__, fn.__name__, phrase)
    doc = " ".join(v3.directional_variogram_3d.__doc__.split())
    for phrase in ("counter-clockwise from +x", "upward from that plane toward +z", "[-90, 90]", "axial", "anisotropy_axes",
                   "across2 <= (along*along) * tan2", "(0, 90]", "bandwidth", "edges[b] <= d < edges[b + 1]", "half the diagonal",
                   "(F, A, nlags)", "NaN", "at most 64 bins", "16 directions", "no CPU fallback", "1 : 1 / scaling_y : 1 / scaling_z"):
        assert phrase in doc, phrase
    doc = " ".join(v3.variogram_map_3d.__doc__.split())
    for phrase in ("(2 nz + 1) x (2 ny + 1) x (2 nx + 1)", "floor(h_x / dx + 0.5)", "mirror cell", "point-symmetric",
                   "twice in the centre cell", "4225", "NaN"):
        assert phrase in doc, phrase
    assert "variography3d" in pa.__all__ and pa.variography3d is v3


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(v3, "_lib", None)
    monkeypatch.setattr(v3, "load", boom)
    monkeypatch.setattr(v3.C, "CDLL", boom)


def test_every_refusal_is_raised_before_anything_is_loaded(no_library):
    x, y, z, v = stations(20)
    v = v[:, 0]
    d = v3.directional_variogram_3d
    one = dict(azimuths=[0.0], dips=[0.0])
    for kw, match in ((dict(), "either azimuths and dips"), (dict(azimuths=[0.0]), "either azimuths and dips"),
                      (dict(dips=[0.0]), "either azimuths and dips"), (dict(azimuths=[0.0, 1.0], dips=[0.0]), "equal length"),
                      (dict(azimuths=[], dips=[]), "non-empty"), (dict(azimuths=[0.0], dips=[0.0], directions=[[1.0, 0.0, 0.0]]), "not both"),
                      (dict(azimuths=[float("nan")], dips=[0.0]), "finite"), (dict(azimuths=[0.0], dips=[90.5]), r"\[-90, 90\]"),
                      (dict(azimuths=list(range(17)), dips=[0.0] * 17), "at most 16 directions"),
                      (dict(directions=np.eye(3)[[0] * 17]), "at most 16 directions"), (dict(directions=[[0.0, 0.0, 0.0]]), "nonzero"),
                      (dict(directions=[[1.0, float("inf"), 0.0]]), "finite"), (dict(directions=[[1.0, 0.0]]), r"shape \(A, 3\)"),
                      (dict(directions=np.zeros((0, 3))), r"shape \(A, 3\)"),
                      (dict(one, tolerance=0.0), r"\(0, 90\]"), (dict(one, tolerance=90.5), r"\(0, 90\]"),
                      (dict(one, tolerance=float("nan")), r"\(0, 90\]"), (dict(one, nlags=0), "nlags"), (dict(one, nlags=2.5), "nlags"),
                      (dict(one, nlags=65), "at most 64"), (dict(one, maxlag=0.0), "maxlag"), (dict(one, maxlag=float("inf")), "maxlag"),
                      (dict(one, edges=[0.0]), "edges"), (dict(one, edges=[0.0, 2.0, 1.0]), "ascending"),
                      (dict(one, edges=[0.0, 1.0, 1.0]), "ascending"), (dict(one, edges=[0.0, float("nan")]), "finite"),
                      (dict(one, edges=np.linspace(0, 1, 66)), "at most 64"), (dict(one, bandwidth=0.0), "bandwidth"),
                      (dict(one, bandwidth=float("inf")), "bandwidth")):
        with pytest.raises(ValueError, match=match):
            d(x, y, z, v, **kw)
    bad = v.copy()
    bad[3] = np.nan
    zbad = z.copy()
    zbad[0] = np.inf
    for call in (lambda *a: d(*a, **one), lambda *a: v3.variogram_map_3d(*a, 2, 2, 2, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="values must be finite"):
            call(x, y, z, bad)
        with pytest.raises(ValueError, match="coordinates must be finite"):
            call(x, y, zbad, v)
        with pytest.raises(ValueError, match="at least two stations"):
            call(x[:1], y[:1], z[:1], v[:1])
        with pytest.raises(ValueError, match="same length"):
            call(x, y, z[:-1], v)
        with pytest.raises(ValueError, match=r"shape \(N,\) or \(N, F\)"):
            call(x, y, z, v[:-1])
        with pytest.raises(ValueError, match=r"shape \(N,\) or \(N, F\)"):
            call(x, y, z, np.zeros((20, 2, 2)))
    for args, match in (((-1, 2, 2, 1.0, 1.0, 1.0), "nx"), ((2, 1.5, 2, 1.0, 1.0, 1.0), "ny"), ((2, 2, True, 1.0, 1.0, 1.0), "nz"),
                        ((8, 8, 7, 1.0, 1.0, 1.0), "at most 4225"), ((32, 32, 1, 1.0, 1.0, 1.0), "at most 4225"),
                        ((2, 2, 2, 0.0, 1.0, 1.0), "positive"), ((2, 2, 2, 1.0, float("nan"), 1.0), "positive"),
                        ((2, 2, 2, 1.0, 1.0, -1.0), "positive")):
        with pytest.raises(ValueError, match=match):
            v3.variogram_map_3d(x, y, z, v, *args)


def test_the_classes_refuse_the_other_dimension_and_device_groups_before_anything_is_loaded(no_library):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(20), rng.random(20), rng.random(20), rng.random(20)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1])
    calls3 = (lambda o: o.directional_variogram_3d([0.0, 90.0], [0.0, 0.0]), lambda o: o.variogram_map_3d(2, 2, 2, 0.1, 0.1, 0.1))
    calls2 = (lambda o: o.directional_variogram([0.0, 90.0]), lambda o: o.variogram_map(2, 2, 0.1, 0.1))
    for cls in (pa.OrdinaryKriging, pa.UniversalKriging):  # a 2-D object names the 2-D method
        obj = cls(x, y, v, **kw)
        for call, name in zip(calls3, ("directional_variogram", "variogram_map")):
            with pytest.raises(ValueError, match=r"2-D object; the 2-D classes have %s \(" % name):
                call(obj)

    class Group:
        n_devices = 2

    for cls in (pa.OrdinaryKriging3D, pa.UniversalKriging3D):
        obj = cls(x, y, z, v, **kw)
        for call, name in zip(calls2, ("directional_variogram_3d", "variogram_map_3d")):  # the 2-D methods go on refusing, and point here
            with pytest.raises(ValueError, match="3-D.*%s" % name):
                call(obj)
        obj._handle = Group()
        try:
            for call in calls3:
                with pytest.raises(ValueError, match="device group of 2"):
                    call(obj)
        finally:
            obj._handle = None
        with pytest.raises(ValueError, match="at most 16 directions"):  # the module's argument errors come through the method
            obj.directional_variogram_3d(list(range(17)), [0.0] * 17)
        with pytest.raises(ValueError, match="at most 4225"):
            obj.variogram_map_3d(8, 8, 7, 0.1, 0.1, 0.1)


# ------------------------------------------------------------------------------------------------------------- the libraries
def _declared():
    text = open(os.path.join(ROOT, "include", "mikvario3.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(mkv3_[a-z_0-9]+)\s*\(", text)))


def test_the_header_declares_what_the_library_exports_and_the_ctypes_mirror_agrees():
    from pykrige_amd import build

    build.build_library()
    assert os.path.exists(build.OUT_VARIO3) and build.OUT_VARIO3 == v3.LIB_PATH and build.API_VARIO3.endswith("mikvario3.h")
    text, names = _declared()
    assert names == sorted(v3.SIGNATURES) == ["mkv3_abi_version", "mkv3_directional", "mkv3_last_error", "mkv3_map"]
    lib = v3.load()
    assert lib.mkv3_abi_version() == v3.ABI_VERSION == int(re.search(r"#define MKV3_ABI_VERSION (\d+)", text).group(1)) == 1
    for macro, value in (("MKV3_MAXLAGS", v3.MAXLAGS), ("MKV3_MAXDIRS", v3.MAXDIRS), ("MKV3_MAXCELLS", v3.MAXCELLS), ("MKV3_EINVAL", "(-1)"),
                         ("MKV3_EHIP", "(-3)"), ("MKV3_FCHUNK", 8)):
        assert re.search(r"#define %s %s(?=\s)" % (macro, re.escape(str(value))), text), macro
    assert (v3.MAXLAGS, v3.MAXDIRS, v3.MAXCELLS) == (64, 16, 4225)
    # the argument lists, type by type
    ctype = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
             "const double *": v3._dp, "double *": v3._dp, "int64_t *": v3._ip}
    flat = " ".join(text.split())
    for name in ("mkv3_directional", "mkv3_map"):
        args = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        want = [ctype[re.match(r"\s*((?:const )?\w+ \*|\w+)", a).group(1)] for a in args]
        assert v3.SIGNATURES[name] == (ctypes.c_int, want), name
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "-C", build.OUT_VARIO3], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(names) <= exported
        kernels = sorted({m.group(1) for m in re.finditer(r"__device_stub__([A-Za-z_0-9]+)\(", out)})
        assert kernels == ["k_vario3_dir", "k_vario3_map", "k_vario3_sum", "k_vario3_sum_cnt"], kernels
        params = {}
        for line in out.splitlines():
            m = re.search(r"__device_stub__([A-Za-z_0-9]+)", line)
            if m:
                params.setdefault(m.group(1), set()).add(line[line.rindex("(") + 1:line.rindex(")")])
        assert all(len(p) == 1 for p in params.values()), params  # each name with one parameter list
        for other in (build.OUT, build.OUT_VARIO):  # nothing of the third library is linked into the two others
            sym = subprocess.run(["nm", "-D", "-C", other], capture_output=True, text=True, check=True).stdout
            assert "mkv3_" not in sym and "k_vario3" not in sym, other
        assert "mkv_directional" not in out and "k_vario_dir" not in out and "mik_" not in out  # nor the reverse
    # calls that are refused launch nothing and need no GPU: the library's own checks answer MKV3_EINVAL with a reason
    x = np.zeros(3)
    out, cnt = np.zeros(4), np.zeros(4, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(v3._dp)
    ip = cnt.ctypes.data_as(v3._ip)
    e, ok = np.array([0.0, 1.0, 0.5]), np.array([0.0, 1.0, 2.0])
    u = np.array([1.0, 0.0, 0.0])

    def directional(n=3, dirs=u, na=1, tol=22.5, bw=0.0, edges=ok, nlags=2, coords=x):
        return lib.mkv3_directional(0, n, p(coords), p(coords), p(coords), p(x), 1, p(dirs), na, tol, bw, p(edges), nlags, p(out), p(out), ip)

    for kw, reason in ((dict(edges=e), b"ascending"), (dict(n=1), b"two stations"), (dict(dirs=np.array([1.0, 0.0, 1e-5])), b"unit vector"),
                       (dict(dirs=np.array([0.0, 0.0, 0.0])), b"unit vector"), (dict(dirs=np.array([1.0, np.nan, 0.0])), b"finite"),
                       (dict(na=17), b"MKV3_MAXDIRS"), (dict(na=0), b"MKV3_MAXDIRS"), (dict(nlags=65), b"MKV3_MAXLAGS"),
                       (dict(tol=0.0), b"(0, 90]"), (dict(tol=91.0), b"(0, 90]"), (dict(bw=float("nan")), b"bandwidth"),
                       (dict(coords=np.array([0.0, np.inf, 1.0])), b"coordinates must be finite")):
        assert directional(**kw) == v3.MKV3_EINVAL and reason in lib.mkv3_last_error(), (kw, lib.mkv3_last_error())

    def cmap(nx=1, ny=1, nz=1, dx=1.0, dy=1.0, dz=1.0):
        return lib.mkv3_map(0, 3, p(x), p(x), p(x), p(x), 1, nx, ny, nz, dx, dy, dz, p(out), ip)

    for kw, reason in ((dict(nx=8, ny=8, nz=7), b"MKV3_MAXCELLS"), (dict(nx=2 ** 30, ny=2 ** 30, nz=2 ** 30), b"MKV3_MAXCELLS"),
                       (dict(nz=-1), b"negative"), (dict(dz=0.0), b"positive"), (dict(dx=-1.0), b"positive"),
                       (dict(dy=float("inf")), b"positive")):
        assert cmap(**kw) == v3.MKV3_EINVAL and reason in lib.mkv3_last_error(), (kw, lib.mkv3_last_error())


def test_a_missing_or_stale_library_is_answered_as_the_second_one_is(monkeypatch):
    monkeypatch.setattr(v3, "_lib", None)
    monkeypatch.setattr(v3, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    with pytest.raises(ImportError, match=r"is missing -- build it with `python -m pykrige_amd.build`"):
        v3.load()
    monkeypatch.undo()
    real = v3.load()

    class Old:
        def __getattr__(self, name):
            if name == "mkv3_map":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(v3, "_lib", None)
    monkeypatch.setattr(v3.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mkv3_map.*rebuild"):
        v3.load()


def test_the_third_library_is_a_unit_of_its_own():
    from pykrige_amd import build

    assert list(build.UNITS_VARIO3) == ["mik_vario3"] and list(build.UNITS_VARIO) == ["mik_vario"] and len(build.UNITS) == 10
    assert "mik_vario3" not in build.UNITS and not any("vario" in os.path.basename(d) for d in build.all_sources())
    assert build.OUT_VARIO3.endswith("libmikvario3.so") and "libmikvario3.so" in build.__doc__
    csrc = os.path.join(ROOT, "pykrige_amd", "csrc")
    hip, hdr = open(os.path.join(csrc, "mik_vario3.hip")).read(), open(os.path.join(csrc, "mik_k_vario3.h")).read()
    for text in (hip, hdr):  # self-contained: the 2-D kernels are not instantiated a second time; no options, no environment
        assert '"mik_k_vario.h"' not in text and "mikvario.h" not in text and "getenv" not in text and "strcmp" not in text
    assert "namespace mkv3" in hdr and "#pragma clang fp contract(off)" in hdr and "static_assert" in hip and "asm" not in hdr
    build.build_library()
    assert build.up_to_date()
    # the unit's command line is the other units': the same flags (the include path aside, which names the checkout that built it)
    plain = lambda flags: [c for c in flags if c not in build.COMPRESS and not c.startswith("-I")]
    assert plain(open(os.path.join(build.OBJ, "mik_vario3.flags")).read().split()) == plain(build.FLAGS)


# ------------------------------------------------------------------------------------------------------------- the definitions
def test_direction_vectors_are_the_definition():
    rad = math.pi / 180.0
    u = v3.direction_vectors(AZIMUTHS, DIPS)
    assert u.shape == (6, 3) and u.dtype == np.float64
    for k, (a, d) in enumerate(zip(AZIMUTHS, DIPS)):
        want = (math.cos(d * rad) * math.cos(a * rad), math.cos(d * rad) * math.sin(a * rad), math.sin(d * rad))
        assert tuple(u[k]) == want
    assert tuple(u[0]) == (1.0, 0.0, 0.0) and u[2, 1] == 1.0 and u[5, 2] == 1.0 and np.all(u[:3, 2] == 0.0)
    assert np.abs(np.sqrt((u * u).sum(axis=1)) - 1.0).max() <= 4 * U
    assert np.array_equal(v3.direction_vectors(30.0, 0.0), u[1:2])  # scalars are one direction
    t2, b2 = v3.decision_constants(22.5, 0.8)
    assert t2 == math.tan(22.5 * rad) * math.tan(22.5 * rad) and b2 == 0.8 * 0.8 and v3.decision_constants(35.0)[1] is None


def test_anisotropy_axes_are_the_rows_the_constructor_multiplies_by():
    for ang in (ANGLES, (0.0, 0.0, 0.0), (-75.0, 140.0, 3.5), [12.0, 0.0, 0.0]):
        rows = core.anisotropy_axes(ang)
        rot = core.anisotropy_matrices(3, [1.5, 0.7], ang)[0]
        assert rows.shape == (3, 3) and np.array_equal(rows.view(np.int64), rot.view(np.int64))
        assert np.abs(rows @ rows.T - np.eye(3)).max() <= 16 * U  # unit and mutually perpendicular (a dozen roundings per entry)
    assert np.array_equal(core.anisotropy_axes((0.0, 0.0, 0.0)), np.eye(3))
    # the adjusted coordinates of a raw vector are stretch . rows . h
    rng = np.random.default_rng(5)
    h = rng.standard_normal((7, 3))
    adj = core.adjust_for_anisotropy(h.copy(), [0.0, 0.0, 0.0], [1.5, 0.7], list(ANGLES))
    assert np.allclose(adj, (np.diag([1.0, 1.5, 0.7]) @ core.anisotropy_axes(ANGLES) @ h.T).T, rtol=0, atol=1e-14)
    for bad in ((1.0, 2.0), (1.0, 2.0, float("nan"))):
        with pytest.raises(ValueError, match="three finite angles"):
            core.anisotropy_axes(bad)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_every_input_keeps_its_margin(name):
    margin = reference(name)[3]
    print("%s: margin %.3g" % (name, margin))
    assert margin >= MARGIN, (name, margin)


@pytest.mark.parametrize("name", sorted(MAP_INPUTS))
def test_every_map_input_keeps_its_margin(name):
    margin = map_reference(name)[2]
    print("%s: margin %.3g cells" % (name, margin))
    assert margin >= MARGIN, (name, margin)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_float64_restatement_agrees_with_the_brute_force(name):
    kw, dirs, tol, bw, edges = INPUTS[name]
    x, y, z, v = stations(**kw)
    counts, lag, semi, _ = reference(name)
    c64, l64, s64, _ = directional_sums(x, y, z, v, dirs, tol, bw, edges, dtype=np.float64)
    assert np.array_equal(c64, counts)
    rl, rs = worst_ratio(l64, lag, counts), worst_ratio(s64, semi, counts[None])
    print("%s: worst err / bar lag %.3g semi %.3g" % (name, rl, rs))
    assert rl <= 1.0 and rs <= 1.0, (name, rl, rs)


@pytest.mark.parametrize("name", sorted(MAP_INPUTS))
def test_the_float64_restatement_of_the_map_agrees_with_the_brute_force(name):
    kw, nx, ny, nz, cdx, cdy, cdz = MAP_INPUTS[name]
    x, y, z, v = stations(**kw)
    counts, semi, _, inside = map_reference(name)
    c64, s64, _, i64 = map_sums(x, y, z, v, nx, ny, nz, cdx, cdy, cdz, dtype=np.float64)
    assert np.array_equal(c64, counts) and np.array_equal(counts, counts[::-1, ::-1, ::-1]) and i64 == inside
    assert counts.sum() == 2 * inside
    if kw.get("coincident"):
        assert counts[nz, ny, nx] >= 2  # the coincident pair: twice in the centre cell
    rs = worst_ratio(s64, semi, counts[None])
    print("%s: worst err / bar semi %.3g" % (name, rs))
    assert rs <= 1.0, (name, rs)


def test_the_brute_force_knows_the_properties_the_device_is_held_to():
    # three mutually perpendicular directions with a tolerance below atan(1 / sqrt 2) = 35.26 degrees never share a pair that lies apart:
    # at most one of the three squared direction cosines can exceed cos^2(35.26) = 2/3 ... a coincident pair is in all three
    kw, dirs, tol, bw, edges = INPUTS["partition_n129"]
    assert tol < math.degrees(math.atan(1.0 / math.sqrt(2.0)))
    x, y, z, v = stations(**kw)
    dx, dy, dz, d, _ = _pairs(x, y, z, v, LD)
    member, _ = membership(dx, dy, dz, dirs, tol, bw)
    apart = d > 0
    assert member[:, apart].sum(axis=0).max() == 1 and (~apart).sum() == 2 and member[:, ~apart].all()
    cp, co = reference("partition_n129")[0], reference("omni_n129")[0]
    extra = 3 * np.array([2, 0, 0, 0, 0, 0, 0])
    assert np.all(cp.sum(axis=0) - extra <= co[0] - extra // 3) and np.all(cp[:, 1:].sum(axis=0) < co[0, 1:])  # some pairs are in no cone
    ca = reference("axial_n129")[0]
    assert np.array_equal(ca[0], ca[1]) and np.array_equal(ca[2], ca[3]) and not np.array_equal(ca[0], ca[2])
    # a lone pair: one count at most per direction, in the bin of its distance
    c2 = reference("n2")[0]
    assert c2.sum() <= len(DIRS) and set(np.unique(c2)) <= {0, 1} and np.count_nonzero(c2.sum(axis=0)) <= 1
    # the flat input is the planar problem: z drops out of d, and dz = 0 exactly
    xf, yf, zf, _ = stations(**INPUTS["flat_n129"][0])
    assert np.all(zf == zf[0]) and np.all(INPUTS["flat_n129"][1][:, 2] == 0.0)
