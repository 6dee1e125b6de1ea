"""directional_variogram_3d / variogram_map_3d on the GPU (libmikvario3.so: k_vario3_dir, k_vario3_map) against the extended-precision brute
force of tests/test_directional_variogram_3d_host.py, which also asserts (on the CPU) that every input here keeps a relative margin >= 1e-9
to every decision boundary -- the condition under which counts must be EQUAL.

Bars: counts equal; |device - ref| <= (count + 8) 2^-52 ref for the sums (the Python layer's means are multiplied back by the count).
Each test prints its worst err / bar.  The omnidirectional test compares with the object's own host binning (SciPy, float64) and runs on
the object's adjusted coordinates, the ones its constructor binned: its first edge is the smallest pair distance itself, so that input has
no margin to speak of and is not one of the brute-force inputs.  The planar tests compare with the 2-D tool (libmikvario.so), whose decision
is not squared: their input keeps the margin under both rules (asserted).

Recorded on an MI355X (worst err / bar, lags / semivariance): brute force n = 2: 0.023 / 0.032, 63: 0.054 / 0.057 (bandwidth 0.056 / 0.065),
64: 0.073 / 0.046 (0.073 / 0.093), 65: 0.063 / 0.066 (0.063 / 0.18), 129: 0.046 / 0.061 (0.046 / 0.069), 600: 0.021 / 0.0097 (0.021 /
0.015); flat stations 0.0054 / 0.0073 (the 2-D tool the same), flat map 0.0098 (the 2-D map the same); tolerance 90 against the constructor
0.030 / 0.0098; partition 0.055 / 0.063, omnidirectional 0.00058 / 0.0017; axial 0.037 / 0.027, reversed 0.026 / 0.027; fields F = 1, 8, 9,
17: 0.049 / 0.065, 0.12, 0.11, 0.11, single planes <= 0.11; coincident 0.052 / 0.14; map n = 65: 0.035 (3 x 5 x 3), 0.16 (17 x 17 x 13 cells),
n = 600: 0.0015, 0.082; limits (64 lags x 16 directions) 0.11 / 0.097.  The whole file: 25 tests in 1.8 s."""
import numpy as np
import pytest

from pykrige_amd import core
from pykrige_amd import variography as vg
from pykrige_amd import variography3d as v3
from tests import _cv_cases as cv
from tests import test_directional_variogram_3d_host as hh
from tests import test_directional_variogram_host as h2

pytestmark = pytest.mark.gpu


def _run(name, **over):
    kw, dirs, tol, bw, edges = hh.INPUTS[name]
    x, y, z, v = hh.stations(**kw)
    vals = v if v.shape[1] > 1 else v[:, 0]
    return v3.directional_variogram_3d(x, y, z, vals, directions=over.get("directions", dirs), tolerance=tol, edges=edges, bandwidth=bw)


def _check(name, lags, semi, counts):
    """Counts equal, means inside the bar, NaN exactly in the empty bins; returns the worst ratios."""
    rc, rl, rs, margin = hh.reference(name)
    assert margin >= hh.MARGIN
    assert counts.dtype == np.int64 and np.array_equal(counts, rc), name
    semi = semi if semi.ndim == 3 else semi[None]
    assert lags.shape == rc.shape and semi.shape == rs.shape
    wl, ws = hh.mean_ratio(lags, rl, rc), hh.mean_ratio(semi, rs, rc[None])
    print("%s: worst err / bar lags %.3g semivariance %.3g" % (name, wl, ws))
    assert wl <= 1.0 and ws <= 1.0, (name, wl, ws)
    return wl, ws


@pytest.mark.parametrize("bandwidth", ["", "_bandwidth"])
@pytest.mark.parametrize("n", hh.SIZES)
def test_against_the_brute_force(n, bandwidth):
    name = "n%d%s" % (n, bandwidth)
    _check(name, *_run(name))


def test_azimuths_and_dips_are_the_unit_vectors():
    kw, dirs, tol, bw, edges = hh.INPUTS["n65"]
    x, y, z, v = hh.stations(**kw)
    lags, semi, counts = v3.directional_variogram_3d(x, y, z, v[:, 0], hh.AZIMUTHS, hh.DIPS, tolerance=tol, edges=edges)
    _check("n65", lags, semi, counts)
    # directions are normalised on the host: any positive multiple is the same direction
    l2, s2, c2 = v3.directional_variogram_3d(x, y, z, v[:, 0], directions=dirs * np.array([[2.0], [0.5], [3.0], [1.0], [7.0], [0.25]]),
                                             tolerance=tol, edges=edges)
    assert np.array_equal(c2, counts)


def test_flat_stations_and_dip_zero_are_the_2d_tool():
    name = "flat_n129"
    kw, dirs, tol, bw, edges = hh.INPUTS[name]
    x, y, z, v = hh.stations(**kw)
    az = (0.0, 30.0, 90.0, 135.0)
    assert np.array_equal(dirs, v3.direction_vectors(az, (0.0,) * 4)) and np.all(z == z[0])
    assert hh.reference(name)[3] >= hh.MARGIN and h2.directional_sums(x, y, v, az, tol, bw, edges)[3] >= h2.MARGIN  # under both rules
    lags, semi, counts = _run(name)
    _check(name, lags, semi, counts)
    l2, s2, c2 = vg.directional_variogram(x, y, v[:, 0], az, tolerance=tol, edges=edges, bandwidth=bw)
    assert np.array_equal(counts, c2)
    rc, rl, rs, _ = hh.reference(name)
    wl, ws = hh.mean_ratio(l2, rl, rc), hh.mean_ratio(s2[None], rs, rc[None])  # the 2-D sums, within the bar of the 3-D reference
    print("2-D tool on the flat stations: worst err / bar lags %.3g semivariance %.3g" % (wl, ws))
    assert wl <= 1.0 and ws <= 1.0
    # the map with nz = 0: one z-slice, the 2-D map's counts
    mname = "map_flat_n129_9x7x1"
    kw, nx, ny, nz, cdx, cdy, cdz = hh.MAP_INPUTS[mname]
    x, y, z, v = hh.stations(**kw)
    rc, rs, margin, inside = hh.map_reference(mname)
    assert nz == 0 and margin >= hh.MARGIN and h2.map_sums(x, y, v, nx, ny, cdx, cdy)[2] >= h2.MARGIN
    m3, c3 = v3.variogram_map_3d(x, y, z, v, nx, ny, nz, cdx, cdy, cdz)
    m2, c2 = vg.variogram_map(x, y, v, nx, ny, cdx, cdy)
    assert c3.shape == (1, 2 * ny + 1, 2 * nx + 1) and np.array_equal(c3, rc) and np.array_equal(c3[0], c2)
    ws, w2 = hh.mean_ratio(m3, rs, rc[None]), hh.mean_ratio(m2[:, None], rs, rc[None])
    print("%s: worst err / bar %.3g, the 2-D map %.3g" % (mname, ws, w2))
    assert ws <= 1.0 and w2 <= 1.0


def test_tolerance_90_is_the_constructor_s_omnidirectional_variogram():
    obj, _ = cv.global_case("ok3d_gaussian_aniso_n40")
    from scipy.spatial.distance import pdist

    ca = obj._coords_adj
    d = pdist(ca, metric="euclidean")
    nl = obj._nlags
    width = (d.max() - d.min()) / nl
    edges = [d.min() + k * width for k in range(nl)] + [d.max() + 0.001]  # the constructor's bins (variogram_fit.experimental_variogram)
    lags, semi, counts = v3.directional_variogram_3d(ca[:, 0], ca[:, 1], ca[:, 2], obj._values(), [17.0], [40.0], tolerance=90.0, edges=edges)
    have = counts[0] > 0
    assert counts.sum() == d.size and np.array_equal(np.isnan(lags[0]), ~have)
    assert have.sum() == len(obj.lags) == len(obj.semivariance)
    c = counts[0][have]
    rl = np.abs(lags[0][have] - obj.lags) / ((c + 8) * hh.U * obj.lags)
    rs = np.abs(semi[0][have] - obj.semivariance) / ((c + 8) * hh.U * obj.semivariance)
    print("tolerance 90 vs the constructor: worst err / bar lags %.3g semivariance %.3g" % (rl.max(), rs.max()))
    assert rl.max() <= 1.0 and rs.max() <= 1.0
    # through the object the stations are the raw ones: the same number of pairs, other distances (this case is anisotropic)
    l2, s2, c2 = obj.directional_variogram_3d(directions=core.anisotropy_axes(obj._angle()), tolerance=90.0, nlags=nl, maxlag=10.0)
    assert c2.shape == (3, nl) and np.all(c2.sum(axis=1) == d.size) and np.array_equal(c2[0], c2[1])


def test_three_perpendicular_directions_below_35_degrees_never_share_a_pair():
    lp, sp, cp = _run("partition_n129")
    lo, so, co = _run("omni_n129")
    _check("partition_n129", lp, sp, cp)
    _check("omni_n129", lo, so, co)
    # the two coincident pairs belong to all three directions, in bin 0; every other pair to one at most (the brute force, which the counts
    # equal, holds the membership: tests/test_directional_variogram_3d_host.py)
    coincident = np.array([2, 0, 0, 0, 0, 0, 0])
    assert np.all(cp.sum(axis=0) - 3 * coincident <= co[0] - coincident)
    x, y, z, v = hh.stations(**hh.INPUTS["omni_n129"][0])
    assert co.sum() == 129 * 128 // 2 - int((hh._pairs(x, y, z, v, np.float64)[3] >= 6.0).sum())


def test_directions_are_axial_and_the_station_order_does_not_matter():
    lags, semi, counts = _run("axial_n129")
    _check("axial_n129", lags, semi, counts)
    assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[2], counts[3])
    kw, dirs, tol, bw, edges = hh.INPUTS["axial_n129"]
    x, y, z, v = hh.stations(**kw)
    lr, sr, cr = v3.directional_variogram_3d(x[::-1], y[::-1], z[::-1], v[::-1, 0], directions=dirs, tolerance=tol, edges=edges)
    assert np.array_equal(cr, counts)
    _check("axial_n129", lr, sr, cr)


def test_fields_share_the_pair_geometry():
    one = {}
    for nf in (1, 8, 9, 17):
        name = "fields_f%d" % nf
        lags, semi, counts = _run(name)
        assert semi.shape == ((nf,) + counts.shape if nf > 1 else counts.shape)
        _check(name, lags, semi, counts)
        one[nf] = counts
    kw, dirs, tol, bw, edges = hh.INPUTS["fields_f17"]
    x, y, z, v = hh.stations(**kw)
    rc, rl, rs, _ = hh.reference("fields_f17")
    for nf in (1, 8, 9):
        assert np.array_equal(one[nf], one[17])  # counts do not depend on F
    for f in (0, 7, 8, 16):  # plane f is the one-field call on column f
        l1, s1, c1 = v3.directional_variogram_3d(x, y, z, v[:, f], directions=dirs, tolerance=tol, edges=edges)
        assert np.array_equal(c1, rc)
        ws = hh.mean_ratio(s1[None], rs[f:f + 1], rc[None])
        print("field %d alone: worst err / bar %.3g" % (f, ws))
        assert ws <= 1.0


def test_a_coincident_pair_lands_in_bin_0_of_every_direction():
    kw, dirs, tol, bw, edges = hh.INPUTS["coincident_n65"]
    assert edges[0] == 0.0
    # alone: two stations on one spot
    lags, semi, counts = v3.directional_variogram_3d([3.0, 3.0], [1.5, 1.5], [0.5, 0.5], [1.0, 4.0], directions=dirs, tolerance=tol, edges=edges,
                                                     bandwidth=bw)
    want = np.zeros((len(dirs), len(edges) - 1), dtype=np.int64)
    want[:, 0] = 1
    assert np.array_equal(counts, want)
    assert np.all(lags[:, 0] == 0.0) and np.all(semi[:, 0] == 4.5) and np.isnan(lags[:, 1:]).all() and np.isnan(semi[:, 1:]).all()
    m, c = v3.variogram_map_3d([3.0, 3.0], [1.5, 1.5], [0.5, 0.5], [1.0, 4.0], 1, 1, 1, 1.0, 1.0, 1.0)
    assert c.sum() == 2 and c[1, 1, 1] == 2 and m[1, 1, 1] == 4.5 and np.isnan(m).sum() == 26
    # among 63 others: the brute force holds it in bin 0 of every direction, and no bin with pairs turns NaN
    lags, semi, counts = _run("coincident_n65")
    _check("coincident_n65", lags, semi, counts)
    x, y, z, v = hh.stations(**kw)
    assert x[64] == x[0] and y[64] == y[0] and z[64] == z[0]
    rest = hh.directional_sums(x[:64], y[:64], z[:64], v[:64], dirs, tol, bw, edges)[0]
    tail = lambda a: np.r_[a[1:64], a[64]]
    last = hh.directional_sums(tail(x), tail(y), tail(z), v[1:65], dirs, tol, bw, edges)[0] \
        - hh.directional_sums(x[1:64], y[1:64], z[1:64], v[1:64], dirs, tol, bw, edges)[0]
    assert np.array_equal(counts - rest - last, want)  # what station 64 adds beyond its pairs with stations 1 .. 63: the coincident pair
    assert np.isfinite(lags[counts > 0]).all() and np.isfinite(semi[counts > 0]).all()


@pytest.mark.parametrize("name", sorted(n for n in hh.MAP_INPUTS if "flat" not in n))
def test_the_map_against_the_brute_force(name):
    kw, nx, ny, nz, cdx, cdy, cdz = hh.MAP_INPUTS[name]
    x, y, z, v = hh.stations(**kw)
    semi, counts = v3.variogram_map_3d(x, y, z, v, nx, ny, nz, cdx, cdy, cdz)
    rc, rs, margin, inside = hh.map_reference(name)
    assert margin >= hh.MARGIN
    assert counts.dtype == np.int64 and counts.shape == (2 * nz + 1, 2 * ny + 1, 2 * nx + 1) and np.array_equal(counts, rc)
    ws = hh.mean_ratio(semi, rs, rc[None])
    print("%s: worst err / bar %.3g" % (name, ws))
    assert ws <= 1.0
    # exactly point-symmetric: the same counts and the same bits in mirrored cells
    assert np.array_equal(counts, counts[::-1, ::-1, ::-1])
    assert np.array_equal(semi.view(np.int64), semi[:, ::-1, ::-1, ::-1].copy().view(np.int64))
    assert counts.sum() == 2 * inside and counts[nz, ny, nx] >= 2  # total counts: twice the inside pairs; the coincident pair twice
    one, c1 = v3.variogram_map_3d(x, y, z, v[:, 1], nx, ny, nz, cdx, cdy, cdz)
    assert one.shape == counts.shape and np.array_equal(c1, counts)
    assert hh.mean_ratio(one[None], rs[1:2], rc[None]) <= 1.0


def test_the_limits_run_and_one_more_is_refused():
    name = "limits_n129"
    lags, semi, counts = _run(name)
    assert counts.shape == (v3.MAXDIRS, v3.MAXLAGS)
    _check(name, lags, semi, counts)
    kw, dirs, tol, bw, edges = hh.INPUTS[name]
    x, y, z, v = hh.stations(**kw)
    with pytest.raises(ValueError, match="at most 16 directions"):
        v3.directional_variogram_3d(x, y, z, v[:, 0], directions=np.vstack([dirs, [[0.0, 0.0, 1.0]]]), edges=edges)
    with pytest.raises(ValueError, match="at most 64 lag bins"):
        v3.directional_variogram_3d(x, y, z, v[:, 0], directions=dirs, edges=hh.edges_of(v3.MAXLAGS + 1, 9.0))
    with pytest.raises(ValueError, match="at most 64 lag bins"):
        v3.directional_variogram_3d(x, y, z, v[:, 0], directions=dirs, nlags=v3.MAXLAGS + 1)
    # the largest map, 65 x 65 x 1 = 4225 cells, runs; 4335 cells are refused
    m, c = v3.variogram_map_3d(x, y, z, v[:, 0], 32, 32, 0, 0.21, 0.17, 9.0)
    assert c.shape == (1, 65, 65) and np.array_equal(c, c[::-1, ::-1, ::-1]) and c.sum() > 0 and c.sum() % 2 == 0
    dx, dy, dz, _, _ = hh._pairs(x, y, z, v, np.float64)
    inside = (np.abs(np.floor(dx / 0.21 + 0.5)) <= 32) & (np.abs(np.floor(dy / 0.17 + 0.5)) <= 32) & (np.floor(dz / 9.0 + 0.5) == 0)
    assert c.sum() == 2 * inside.sum()
    with pytest.raises(ValueError, match="at most 4225"):
        v3.variogram_map_3d(x, y, z, v[:, 0], 8, 8, 7, 0.5, 0.5, 0.5)


def test_a_kriging_object_executes_the_same_bits_before_and_after():
    obj, _ = cv.global_case("ok3d_gaussian_aniso_n40")
    gx, gy, gz = np.linspace(0.0, 1.0, 11), np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 7)
    z0, s0 = obj.execute("grid", gx, gy, gz)
    z0, s0 = np.array(z0), np.array(s0)
    lags, semi, counts = obj.directional_variogram_3d([0.0, 45.0, 90.0, 0.0], [0.0, 0.0, 0.0, 90.0], nlags=5)
    assert counts.shape == (4, 5) and counts.sum() > 0
    la, sa, ca = obj.directional_variogram_3d(directions=core.anisotropy_axes(obj._angle()), tolerance=30.0, nlags=5)
    assert ca.shape == (3, 5) and ca.sum() > 0
    m, c = obj.variogram_map_3d(3, 3, 2, 0.15, 0.15, 0.2)
    assert c.shape == (5, 7, 7) and np.array_equal(c, c[::-1, ::-1, ::-1])
    z1, s1 = obj.execute("grid", gx, gy, gz)
    assert np.array_equal(np.asarray(z1).view(np.int64), z0.view(np.int64)) and np.array_equal(np.asarray(s1).view(np.int64), s0.view(np.int64))
