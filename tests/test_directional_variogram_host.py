"""directional_variogram / variogram_map without a GPU: the module and the two 2-D classes carry the signatures and docstrings the users
read, every refusal is raised before ctypes loads anything, include/mikvario.h declares what libmikvario.so exports and the ctypes mirror
agrees with it, libmikrige.so is what it was, and a float64 NumPy restatement of the definitions agrees with the extended-precision brute
force inside the bars the device is held to.

Also the home of what tests/test_directional_variogram.py (GPU) shares with this file: the station sets, the brute force and the bars.

The brute force evaluates the definitions of include/mikvario.h over all pairs i < j in np.longdouble, with the host's float64 cos / sin /
tan of variography.direction_constants -- the three numbers the device decides from.  It also returns the MARGIN: the smallest relative
distance of any pair to any decision boundary (a bin edge |d - e| / max(d, e); the tolerance cone |across - along tan| / max of the two;
the bandwidth likewise; a cell border of the map, in cells).  A coincident pair (dx = dy = 0 exactly) sits on the boundaries it touches
in every arithmetic and is left out of the margin.  Exact counts are demanded only of inputs whose margin is >= 1e-9: every input of
INPUTS / MAP_INPUTS is asserted to keep it, here, on the CPU (test_every_input_keeps_its_margin; the smallest recorded: 5.5e-8 of relative distance, 8.6e-7 of a cell).

Bars: counts equal; |sum - ref| <= (count + 8) 2^-52 ref per bin -- the terms are non-negative, so any summation order of `count` terms
with a few roundings each stays inside.

libmikrige.so: 2 198 392 bytes built from the parent commit and 2 198 392 bytes built from this one, same compiler (HIP 7.2.26015), same
directory (the byte count moves with the length of the checkout's path: __FILE__ of the error macros)."""
import ctypes
import functools
import hashlib
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import variography as vg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = 2.0 ** -52
MARGIN = 1e-9
AZIMUTHS = (0.0, 30.0, 90.0, 135.0)
SIZES = (2, 63, 64, 65, 129, 600)


# ------------------------------------------------------------------------------------------------------------- inputs
def stations(n, nf=1, seed=0, coincident=0):
    """n random stations in a 10 x 7 box with nf fields (n, nf); the last `coincident` stations repeat the first ones."""
    rng = np.random.default_rng(7000 + 13 * n + seed)
    x, y = 10.0 * rng.random(n), 7.0 * rng.random(n)
    v = np.sin(0.7 * x)[:, None] * np.cos(0.5 * y)[:, None] + 0.3 * rng.standard_normal((n, nf))
    for k in range(coincident):
        x[n - 1 - k], y[n - 1 - k] = x[k], y[k]
    return x, y, v


def edges_of(nlags, maxlag=6.0):
    return np.linspace(0.0, maxlag, nlags + 1)


# name -> (stations kwargs, azimuths, tolerance, bandwidth, edges): every directional input the GPU file compares against the brute force
INPUTS = {}
for _n in SIZES:
    INPUTS["n%d" % _n] = (dict(n=_n), AZIMUTHS, 22.5, None, edges_of(7))
    INPUTS["n%d_bandwidth" % _n] = (dict(n=_n), AZIMUTHS, 22.5, 0.8, edges_of(7))
INPUTS["partition_n129"] = (dict(n=129, coincident=2), (20.0, 110.0), 45.0, None, edges_of(7))
INPUTS["omni_n129"] = (dict(n=129, coincident=2), (20.0,), 90.0, None, edges_of(7))
INPUTS["axial_n129"] = (dict(n=129), (35.0, 215.0), 22.5, None, edges_of(7))
for _f in (1, 8, 9, 17):
    INPUTS["fields_f%d" % _f] = (dict(n=129, nf=_f, seed=1), AZIMUTHS, 22.5, None, edges_of(7))
INPUTS["coincident_n65"] = (dict(n=65, coincident=1), AZIMUTHS, 22.5, 0.8, edges_of(7))
INPUTS["limits_n129"] = (dict(n=129, seed=2), tuple(11.25 * k for k in range(vg.MAXDIRS)), 22.5, None, edges_of(vg.MAXLAGS, 9.0))
# name -> (stations kwargs, nx, ny, dx, dy); 32 x 32 is the largest permitted cell count, 65 x 65
MAP_INPUTS = {}
for _n in (65, 600):
    MAP_INPUTS["map_n%d_5x3" % _n] = (dict(n=_n, nf=2, coincident=1), 5, 3, 0.9, 1.1)
    MAP_INPUTS["map_n%d_largest" % _n] = (dict(n=_n, nf=2, coincident=1), 32, 32, 0.21, 0.17)


# ------------------------------------------------------------------------------------------------------------- brute force
def _pairs(x, y, v, dtype):
    i, j = np.triu_indices(len(x), 1)
    x, y, v = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(v, dtype=dtype)
    dx, dy = x[j] - x[i], y[j] - y[i]
    dv = v[i] - v[j]
    return dx, dy, np.sqrt(dx * dx + dy * dy), dtype(0.5) * (dv * dv)


def _rel(a, b):
    m = np.maximum(np.abs(a), np.abs(b))
    return np.where(m > 0, np.abs(a - b) / np.where(m > 0, m, 1), np.inf)


def directional_sums(x, y, v, azimuths, tol, bandwidth, edges, dtype=LD):
    """(counts (A, B) int64, lag sums (A, B), semi sums (F, A, B), margin) from the definitions, in `dtype`."""
    cs, sn, tant = vg.direction_constants(azimuths, tol)
    edges = np.asarray(edges, dtype=np.float64)
    dx, dy, d, g = _pairs(x, y, v, dtype)
    apart = ~((dx == 0) & (dy == 0))
    na, nb, nf = len(cs), len(edges) - 1, g.shape[1]
    counts = np.zeros((na, nb), dtype=np.int64)
    lag, semi = np.zeros((na, nb), dtype=dtype), np.zeros((nf, na, nb), dtype=dtype)
    margin = np.inf
    e = edges.astype(dtype)
    if apart.any():
        margin = min(margin, float(min(_rel(d[apart], ek).min() for ek in e)))
    for a in range(na):
        along = np.abs(dx * dtype(cs[a]) + dy * dtype(sn[a]))
        across = np.abs(-dx * dtype(sn[a]) + dy * dtype(cs[a]))
        member = np.ones(d.shape, dtype=bool)
        if tol != 90.0:
            member &= across <= along * dtype(tant)
            if apart.any():
                margin = min(margin, float(_rel(across[apart], (along * dtype(tant))[apart]).min()))
        if bandwidth is not None:
            member &= across <= dtype(bandwidth)
            if apart.any():
                margin = min(margin, float(_rel(across[apart], dtype(bandwidth)).min()))
        for b in range(nb):
            sel = member & (d >= e[b]) & (d < e[b + 1])
            counts[a, b] = int(sel.sum())
            lag[a, b] = d[sel].sum(dtype=dtype)
            semi[:, a, b] = g[sel].sum(axis=0, dtype=dtype)
    return counts, lag, semi, margin


def map_sums(x, y, v, nx, ny, cdx, cdy, dtype=LD):
    """(counts (2ny+1, 2nx+1) int64, semi sums (F, 2ny+1, 2nx+1), margin in cells): every pair into its cell and the mirror cell."""
    dx, dy, _, g = _pairs(x, y, v, dtype)
    ux, uy = dx / dtype(cdx) + dtype(0.5), dy / dtype(cdy) + dtype(0.5)
    qx, qy = np.floor(ux), np.floor(uy)
    margin = float(min(np.minimum(ux - qx, qx + 1 - ux).min(), np.minimum(uy - qy, qy + 1 - uy).min()))
    inside = (np.abs(qx) <= nx) & (np.abs(qy) <= ny)
    ix, iy = (nx + qx[inside]).astype(np.int64), (ny + qy[inside]).astype(np.int64)
    counts = np.zeros((2 * ny + 1, 2 * nx + 1), dtype=np.int64)
    semi = np.zeros((g.shape[1], 2 * ny + 1, 2 * nx + 1), dtype=dtype)
    for sy, sx in ((iy, ix), (2 * ny - iy, 2 * nx - ix)):
        np.add.at(counts, (sy, sx), 1)
        for f in range(g.shape[1]):
            np.add.at(semi[f], (sy, sx), g[inside, f])
    return counts, semi, margin


@functools.lru_cache(maxsize=None)
def reference(name):
    """The brute force of INPUTS[name]: (counts, lag sums, semi sums, margin), computed once and shared; do not write into it."""
    kw, az, tol, bw, edges = INPUTS[name]
    x, y, v = stations(**kw)
    return directional_sums(x, y, v, az, tol, bw, edges)


@functools.lru_cache(maxsize=None)
def map_reference(name):
    kw, nx, ny, cdx, cdy = MAP_INPUTS[name]
    x, y, v = stations(**kw)
    return map_sums(x, y, v, nx, ny, cdx, cdy)


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
    sig = inspect.signature(vg.directional_variogram)
    assert list(sig.parameters) == ["x", "y", "values", "azimuths", "tolerance", "nlags", "maxlag", "edges", "bandwidth"]
    assert [sig.parameters[k].default for k in ("tolerance", "nlags", "maxlag", "edges", "bandwidth")] == [22.5, 6, None, None, None]
    assert list(inspect.signature(vg.variogram_map).parameters) == ["x", "y", "values", "nx", "ny", "dx", "dy"]
    for cls in (pa.OrdinaryKriging, pa.UniversalKriging):
        sig = inspect.signature(cls.directional_variogram)
        assert list(sig.parameters) == ["self", "azimuths", "tolerance", "nlags", "maxlag", "edges", "bandwidth"]
        assert sig.parameters["tolerance"].default == 22.5 and sig.parameters["nlags"].default == 6
        assert list(inspect.signature(cls.variogram_map).parameters) == ["self", "nx", "ny", "dx", "dy"]
        for fn in (cls.directional_variogram, cls.variogram_map):
            doc = " ".join(fn.__doc__.split())
            for phrase in ("BEFORE the anisotropy adjustment", "geographic", "device group", "3-D", "ValueError"):
                assert phrase in doc, (cls.__name__, fn.__name__, phrase)
    doc = " ".join(vg.directional_variogram.__doc__.split())
    for phrase in ("counter-clockwise from +x", "anisotropy_angle", "axial", "across <= along * tan(tolerance)", "(0, 90]", "bandwidth",
                   "edges[b] <= d < edges[b + 1]", "half the diagonal", "(F, A, nlags)", "NaN", "at most 64 bins", "16 azimuths", "no CPU fallback"):
        assert phrase in doc, phrase
    doc = " ".join(vg.variogram_map.__doc__.split())
    for phrase in ("(2 ny + 1) x (2 nx + 1)", "floor(h_x / dx + 0.5)", "mirror cell", "point-symmetric", "twice in the centre cell", "4225", "NaN"):
        assert phrase in doc, phrase
    assert "variography" in pa.__all__ and pa.variography is vg


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(vg, "_lib", None)
    monkeypatch.setattr(vg, "load", boom)
    monkeypatch.setattr(vg.C, "CDLL", boom)


def test_every_refusal_is_raised_before_anything_is_loaded(no_library):
    x, y, v = stations(20)
    v = v[:, 0]
    d = vg.directional_variogram
    for kw, match in ((dict(azimuths=[]), "azimuths"), (dict(azimuths=list(range(17))), "at most 16 azimuths"),
                      (dict(azimuths=[float("nan")]), "finite"), (dict(azimuths=[0.0], tolerance=0.0), r"\(0, 90\]"),
                      (dict(azimuths=[0.0], tolerance=90.5), r"\(0, 90\]"), (dict(azimuths=[0.0], tolerance=float("nan")), r"\(0, 90\]"),
                      (dict(azimuths=[0.0], nlags=0), "nlags"), (dict(azimuths=[0.0], nlags=2.5), "nlags"), (dict(azimuths=[0.0], nlags=65), "at most 64"),
                      (dict(azimuths=[0.0], maxlag=0.0), "maxlag"), (dict(azimuths=[0.0], maxlag=float("inf")), "maxlag"),
                      (dict(azimuths=[0.0], edges=[0.0]), "edges"), (dict(azimuths=[0.0], edges=[0.0, 2.0, 1.0]), "ascending"),
                      (dict(azimuths=[0.0], edges=[0.0, 1.0, 1.0]), "ascending"), (dict(azimuths=[0.0], edges=[0.0, float("nan")]), "finite"),
                      (dict(azimuths=[0.0], edges=np.linspace(0, 1, 66)), "at most 64"), (dict(azimuths=[0.0], bandwidth=0.0), "bandwidth"),
                      (dict(azimuths=[0.0], bandwidth=float("inf")), "bandwidth")):
        with pytest.raises(ValueError, match=match):
            d(x, y, v, **kw)
    bad = v.copy()
    bad[3] = np.nan
    xbad = x.copy()
    xbad[0] = np.inf
    for call in (lambda *a: d(*a, [0.0]), lambda *a: vg.variogram_map(*a, 2, 2, 1.0, 1.0)):
        with pytest.raises(ValueError, match="values must be finite"):
            call(x, y, bad)
        with pytest.raises(ValueError, match="coordinates must be finite"):
            call(xbad, y, v)
        with pytest.raises(ValueError, match="at least two stations"):
            call(x[:1], y[:1], v[:1])
        with pytest.raises(ValueError, match="same length"):
            call(x, y[:-1], v)
        with pytest.raises(ValueError, match=r"shape \(N,\) or \(N, F\)"):
            call(x, y, v[:-1])
        with pytest.raises(ValueError, match=r"shape \(N,\) or \(N, F\)"):
            call(x, y, np.zeros((20, 2, 2)))
    for args, match in (((-1, 2, 1.0, 1.0), "nx"), ((2, 1.5, 1.0, 1.0), "ny"), ((33, 32, 1.0, 1.0), "at most 4225"), ((2, 2, 0.0, 1.0), "positive"),
                        ((2, 2, 1.0, float("nan")), "positive")):
        with pytest.raises(ValueError, match=match):
            vg.variogram_map(x, y, v, *args)


def test_the_classes_refuse_3d_geographic_and_device_groups_before_anything_is_loaded(no_library):
    rng = np.random.default_rng(0)
    x, y, z, v = rng.random(20), rng.random(20), rng.random(20), rng.random(20)
    kw = dict(variogram_model="linear", variogram_parameters=[1.0, 0.1])
    calls = (lambda o: o.directional_variogram([0.0, 90.0]), lambda o: o.variogram_map(2, 2, 0.1, 0.1))
    for cls in (pa.OrdinaryKriging3D, pa.UniversalKriging3D):
        for call in calls:
            with pytest.raises(ValueError, match="3-D"):
                call(cls(x, y, z, v, **kw))
    geo = pa.OrdinaryKriging(30 * x, 30 + 30 * y, v, coordinates_type="geographic", **kw)
    for call in calls:
        with pytest.raises(ValueError, match="geographic"):
            call(geo)

    class Group:
        n_devices = 2

    for cls in (pa.OrdinaryKriging, pa.UniversalKriging):
        obj = cls(x, y, v, **kw)
        obj._handle = Group()
        try:
            for call in calls:
                with pytest.raises(ValueError, match="device group of 2"):
                    call(obj)
        finally:
            obj._handle = None
        with pytest.raises(ValueError, match="at most 16 azimuths"):  # the module's argument errors come through the method
            obj.directional_variogram(list(range(17)))
        with pytest.raises(ValueError, match="at most 4225"):
            obj.variogram_map(40, 40, 0.1, 0.1)


# ------------------------------------------------------------------------------------------------------------- the libraries
def _declared():
    text = open(os.path.join(ROOT, "include", "mikvario.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, sorted(set(re.findall(r"\b(mkv_[a-z_0-9]+)\s*\(", text)))


def test_the_header_declares_what_the_library_exports_and_the_ctypes_mirror_agrees():
    from pykrige_amd import build

    build.build_library()
    assert os.path.exists(build.OUT_VARIO) and build.OUT_VARIO == vg.LIB_PATH and build.OUT.endswith("libmikrige.so")
    text, names = _declared()
    assert names == sorted(vg.SIGNATURES) == ["mkv_abi_version", "mkv_directional", "mkv_last_error", "mkv_map"]
    lib = vg.load()
    assert lib.mkv_abi_version() == vg.ABI_VERSION == int(re.search(r"#define MKV_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MKV_MAXLAGS", vg.MAXLAGS), ("MKV_MAXDIRS", vg.MAXDIRS), ("MKV_MAXCELLS", vg.MAXCELLS), ("MKV_EINVAL", "(-1)"),
                         ("MKV_EHIP", "(-3)")):
        assert re.search(r"#define %s %s(?=\s)" % (macro, re.escape(str(value))), text), macro
    core_h = open(os.path.join(ROOT, "pykrige_amd", "csrc", "mik_k_core.h")).read()
    assert int(re.search(r"#define MIK_VG_MAXLAGS (\d+)", core_h).group(1)) == vg.MAXLAGS
    # the argument lists, type by type
    ctype = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
             "const double *": vg._dp, "double *": vg._dp, "int64_t *": vg._ip}
    flat = " ".join(text.split())
    for name in ("mkv_directional", "mkv_map"):
        args = re.search(r"int %s\((.*?)\);" % name, flat).group(1).split(",")
        want = [ctype[re.match(r"\s*((?:const )?\w+ \*|\w+)", a).group(1)] for a in args]
        assert vg.SIGNATURES[name] == (ctypes.c_int, want), name
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "-C", build.OUT_VARIO], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(names) <= exported
        kernels = sorted({m.group(1) for m in re.finditer(r"__device_stub__([A-Za-z_0-9]+)\(", out)})
        assert kernels == ["k_vario_dir", "k_vario_map", "k_vario_sum", "k_vario_sum_cnt"], kernels
        core = subprocess.run(["nm", "-D", "-C", build.OUT], capture_output=True, text=True, check=True).stdout
        assert "mkv_" not in core and "k_vario" not in core  # nothing of the second library is linked into the first
    # calls that are refused launch nothing and need no GPU: the library's own checks answer MKV_EINVAL with a reason
    x = np.zeros(3)
    out, cnt = np.zeros(4), np.zeros(4, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(vg._dp)
    e = np.array([0.0, 1.0, 0.5])
    rc = lib.mkv_directional(0, 3, p(x), p(x), p(x), 1, p(x), 1, 22.5, 0.0, p(e), 2, p(out), p(out), cnt.ctypes.data_as(vg._ip))
    assert rc == vg.MKV_EINVAL and b"ascending" in lib.mkv_last_error()
    rc = lib.mkv_map(0, 3, p(x), p(x), p(x), 1, 33, 32, 1.0, 1.0, p(out), cnt.ctypes.data_as(vg._ip))
    assert rc == vg.MKV_EINVAL and b"MKV_MAXCELLS" in lib.mkv_last_error()
    rc = lib.mkv_directional(0, 1, p(x), p(x), p(x), 1, p(x), 1, 22.5, 0.0, p(e), 2, p(out), p(out), cnt.ctypes.data_as(vg._ip))
    assert rc == vg.MKV_EINVAL and b"two stations" in lib.mkv_last_error()


def test_a_missing_or_stale_library_is_answered_as_the_first_one_is(monkeypatch):
    monkeypatch.setattr(vg, "_lib", None)
    monkeypatch.setattr(vg, "LIB_PATH", os.path.join(ROOT, "pykrige_amd", "no_such_library.so"))
    with pytest.raises(ImportError, match=r"is missing -- build it with `python -m pykrige_amd.build`"):
        vg.load()
    monkeypatch.undo()
    real = vg.load()

    class Old:
        def __getattr__(self, name):
            if name == "mkv_map":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(vg, "_lib", None)
    monkeypatch.setattr(vg.C, "CDLL", lambda path: Old())
    with pytest.raises(ImportError, match="does not export mkv_map.*rebuild"):
        vg.load()


# libmikrige.so as the parent commit builds it: the sha256 of build.all_sources() read in that order, the compiler, the length of the
# checkout's path (its bytes hold __FILE__), the size
PARENT_SOURCES = "4e7a5db8af8cd9e33a42fc3b868078ba2556fa3cb9a3c1d08b1ace2876fca1ba"
PARENT_BUILD = ("7.2.26015", 10, 2_198_392)


def test_the_first_library_is_built_as_before():
    """The ten units of libmikrige.so keep their command lines (the .flags stamps), the second library's unit is not among them, and while
    the library's sources are the parent commit's bytes it has the parent's size under the parent's compiler in a checkout path of the same
    length.  (A later commit that changes those sources is no longer held to the size: the bar of tests/test_abi_and_host.py stays.)"""
    from pykrige_amd import build

    build.build_library()
    assert len(build.UNITS) == 10 and "mik_vario" not in build.UNITS and list(build.UNITS_VARIO) == ["mik_vario"]
    compress = [c for c in build.COMPRESS]
    for name, (_, _, extra) in build.UNITS.items():
        stamp = open(os.path.join(build.OBJ, name + ".flags")).read().split()
        assert [c for c in stamp if c not in compress] == [c for c in build.FLAGS + extra if c not in compress], name
    assert not any("vario" in os.path.basename(d) for d in build.all_sources())
    h = hashlib.sha256()
    for f in build.all_sources():
        h.update(open(f, "rb").read())
    if h.hexdigest() != PARENT_SOURCES:
        return
    ver = subprocess.run([build.hipcc(), "--version"], capture_output=True, text=True).stdout
    stamps = [open(os.path.join(build.OBJ, n + ".flags")).read().split() for n in build.UNITS]
    if PARENT_BUILD[0] in ver and len(ROOT) == PARENT_BUILD[1] and all(set(compress) <= set(st) for st in stamps):
        assert os.path.getsize(build.OUT) == PARENT_BUILD[2], os.path.getsize(build.OUT)


# ------------------------------------------------------------------------------------------------------------- the definitions
def test_direction_constants_are_the_c_library_s():
    cs, sn, t = vg.direction_constants([0.0, 30.0, 90.0, 135.0], 22.5)
    assert cs[0] == 1.0 and sn[0] == 0.0 and sn[2] == 1.0 and cs[2] == math.cos(90.0 * (math.pi / 180.0))
    assert cs[1] == math.cos(30.0 * (math.pi / 180.0)) and sn[3] == math.sin(135.0 * (math.pi / 180.0)) and t == math.tan(22.5 * (math.pi / 180.0))


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
    kw, az, tol, bw, edges = INPUTS[name]
    x, y, v = stations(**kw)
    counts, lag, semi, _ = reference(name)
    c64, l64, s64, _ = directional_sums(x, y, v, az, tol, bw, edges, dtype=np.float64)
    assert np.array_equal(c64, counts)
    rl, rs = worst_ratio(l64, lag, counts), worst_ratio(s64, semi, counts[None])
    print("%s: worst err / bar lag %.3g semi %.3g" % (name, rl, rs))
    assert rl <= 1.0 and rs <= 1.0, (name, rl, rs)


@pytest.mark.parametrize("name", sorted(MAP_INPUTS))
def test_the_float64_restatement_of_the_map_agrees_with_the_brute_force(name):
    kw, nx, ny, cdx, cdy = MAP_INPUTS[name]
    x, y, v = stations(**kw)
    counts, semi, _ = map_reference(name)
    c64, s64, _ = map_sums(x, y, v, nx, ny, cdx, cdy, dtype=np.float64)
    assert np.array_equal(c64, counts) and np.array_equal(counts, counts[::-1, ::-1])
    dx, dy, _, _ = _pairs(x, y, v, np.float64)
    inside = (np.abs(np.floor(dx / cdx + 0.5)) <= nx) & (np.abs(np.floor(dy / cdy + 0.5)) <= ny)
    assert counts.sum() == 2 * inside.sum() and counts[ny, nx] >= 2  # the coincident pair: twice in the centre cell
    rs = worst_ratio(s64, semi, counts[None])
    print("%s: worst err / bar semi %.3g" % (name, rs))
    assert rs <= 1.0, (name, rs)


def test_the_brute_force_knows_the_properties_the_device_is_held_to():
    # theta and theta + 90 with tolerance 45 split the pairs that lie apart; a coincident pair is in both
    cp, _, _, _ = reference("partition_n129")
    co, _, _, _ = reference("omni_n129")
    x, y, _ = stations(**INPUTS["partition_n129"][0])
    assert np.array_equal(cp.sum(axis=0) - co[0], np.array([2, 0, 0, 0, 0, 0, 0]))  # two coincident pairs, bin 0
    ca, la, sa, _ = reference("axial_n129")
    assert np.array_equal(ca[0], ca[1])
    # a lone pair: one count, in the bin of its distance, in the directions whose cone holds it
    c2, l2, _, _ = reference("n2")
    assert c2.sum() <= 2 and set(np.unique(c2)) <= {0, 1}
