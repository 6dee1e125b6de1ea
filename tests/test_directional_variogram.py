"""directional_variogram / variogram_map on the GPU (libmikvario.so: k_vario_dir, k_vario_map) against the extended-precision brute force
of tests/test_directional_variogram_host.py, which also asserts (on the CPU) that every input here keeps a relative margin >= 1e-9 to
every decision boundary -- the condition under which counts must be EQUAL.

Bars: counts equal; |device - ref| <= (count + 8) 2^-52 ref for the sums (the Python layer's means are multiplied back by the count).
Each test prints its worst err / bar.  The omnidirectional test compares with the object's own host binning (SciPy, float64) and runs on
the object's adjusted coordinates, the ones its constructor binned: its first edge is the smallest pair distance itself, so that input has
no margin to speak of and is not one of the brute-force inputs.

Recorded on an MI355X (worst err / bar, lags / semivariance): brute force n = 2: 0 / 0, 63: 0.030 / 0.041, 64: 0.036 / 0.033, 65: 0.024 /
0.028, 129: 0.0062 / 0.0063, 600: 0.00085 / 0.0021 (the same with the bandwidth); tolerance 90 against the constructor 0.0070 / 0.0054;
partition 0.0027 / 0.0027, omnidirectional 0.0016 / 0.0039; axial 0.0099 / 0.011; fields F = 1, 8, 9, 17: 0.0077 / 0.0088, 0.014, 0.017,
0.021, single planes <= 0.0095; coincident 0.025 / 0.032; map n = 65: 0.034 (5 x 3), 0.16 (65 x 65 cells), n = 600: 0.0009, 0.093;
limits (64 lags x 16 directions) 0.11 / 0.12."""
import numpy as np
import pytest

from pykrige_amd import variography as vg
from tests import _cv_cases as cv
from tests import test_directional_variogram_host as hh

pytestmark = pytest.mark.gpu


def _run(name, **over):
    kw, az, tol, bw, edges = hh.INPUTS[name]
    x, y, v = hh.stations(**kw)
    vals = v if v.shape[1] > 1 else v[:, 0]
    return vg.directional_variogram(x, y, vals, over.get("azimuths", az), tolerance=tol, edges=edges, bandwidth=bw)


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


def test_tolerance_90_is_the_constructor_s_omnidirectional_variogram():
    obj, _ = cv.global_case("ok2d_spherical_n130_values_1e3")
    from scipy.spatial.distance import pdist

    ca = obj._coords_adj
    d = pdist(ca, metric="euclidean")
    nl = obj._nlags
    width = (d.max() - d.min()) / nl
    edges = [d.min() + k * width for k in range(nl)] + [d.max() + 0.001]  # the constructor's bins (variogram_fit.experimental_variogram)
    lags, semi, counts = vg.directional_variogram(ca[:, 0], ca[:, 1], obj._values(), [17.0], tolerance=90.0, edges=edges)
    have = counts[0] > 0
    assert counts.sum() == d.size and np.array_equal(np.isnan(lags[0]), ~have)
    assert have.sum() == len(obj.lags) == len(obj.semivariance)
    c = counts[0][have]
    rl = np.abs(lags[0][have] - obj.lags) / ((c + 8) * hh.U * obj.lags)
    rs = np.abs(semi[0][have] - obj.semivariance) / ((c + 8) * hh.U * obj.semivariance)
    print("tolerance 90 vs the constructor: worst err / bar lags %.3g semivariance %.3g" % (rl.max(), rs.max()))
    assert rl.max() <= 1.0 and rs.max() <= 1.0
    # and through the object, on its raw coordinates (this case has no anisotropy: the same stations up to the rounding of the centring)
    l2, s2, c2 = obj.directional_variogram([17.0], tolerance=90.0, edges=edges)
    assert c2.shape == (1, nl) and abs(int(c2.sum()) - d.size) <= 1 and np.allclose(s2[0][have], obj.semivariance, rtol=1e-9)


def test_two_perpendicular_directions_of_tolerance_45_partition_the_pairs():
    lp, sp, cp = _run("partition_n129")
    lo, so, co = _run("omni_n129")
    _check("partition_n129", lp, sp, cp)
    _check("omni_n129", lo, so, co)
    extra = cp.sum(axis=0) - co[0]
    assert np.array_equal(extra, [2, 0, 0, 0, 0, 0, 0]), extra  # the two coincident pairs belong to both directions, in bin 0
    assert co.sum() == 129 * 128 // 2 - int((hh._pairs(*hh.stations(**hh.INPUTS["omni_n129"][0]), np.float64)[2] >= 6.0).sum())


def test_directions_are_axial_and_the_station_order_does_not_matter():
    lags, semi, counts = _run("axial_n129")
    _check("axial_n129", lags, semi, counts)
    assert np.array_equal(counts[0], counts[1])
    kw, az, tol, bw, edges = hh.INPUTS["axial_n129"]
    x, y, v = hh.stations(**kw)
    lr, sr, cr = vg.directional_variogram(x[::-1], y[::-1], v[::-1, 0], az, tolerance=tol, edges=edges)
    assert np.array_equal(cr, counts)
    _check("axial_n129", lr, sr, cr)


def test_fields_share_the_pair_geometry():
    one = {}
    for nf in (1, 8, 9, 17):
        name = "fields_f%d" % nf
        lags, semi, counts = _run(name)
        assert semi.shape == ((nf,) + counts.shape if nf > 1 else counts.shape)
        _check(name, lags, semi, counts)
        one[nf] = (lags, semi if nf > 1 else semi[None], counts)
    kw = hh.INPUTS["fields_f17"][0]
    x, y, v = hh.stations(**kw)
    rc, rl, rs, _ = hh.reference("fields_f17")
    for nf in (1, 8, 9):
        assert np.array_equal(one[nf][2], one[17][2])  # counts do not depend on F
    for f in (0, 7, 8, 16):  # plane f is the one-field call on column f
        l1, s1, c1 = vg.directional_variogram(x, y, v[:, f], hh.AZIMUTHS, tolerance=22.5, edges=hh.edges_of(7))
        assert np.array_equal(c1, rc)
        ws = hh.mean_ratio(s1[None], rs[f:f + 1], rc[None])
        print("field %d alone: worst err / bar %.3g" % (f, ws))
        assert ws <= 1.0


def test_an_isolated_coincident_pair_lands_in_bin_0_of_every_direction():
    kw, az, tol, bw, edges = hh.INPUTS["coincident_n65"]
    assert edges[0] == 0.0
    # alone: two stations on one spot
    lags, semi, counts = vg.directional_variogram([3.0, 3.0], [1.5, 1.5], [1.0, 4.0], az, tolerance=tol, edges=edges, bandwidth=bw)
    want = np.zeros((len(az), len(edges) - 1), dtype=np.int64)
    want[:, 0] = 1
    assert np.array_equal(counts, want)
    assert np.all(lags[:, 0] == 0.0) and np.all(semi[:, 0] == 4.5) and np.isnan(lags[:, 1:]).all() and np.isnan(semi[:, 1:]).all()
    # among 63 others: the brute force holds it in bin 0 of every direction, and no bin with pairs turns NaN
    lags, semi, counts = _run("coincident_n65")
    _check("coincident_n65", lags, semi, counts)
    x, y, v = hh.stations(**kw)
    assert x[64] == x[0] and y[64] == y[0]
    rest = hh.directional_sums(x[:64], y[:64], v[:64], az, tol, bw, edges)[0]
    last = hh.directional_sums(np.r_[x[1:64], x[64]], np.r_[y[1:64], y[64]], v[1:65], az, tol, bw, edges)[0] \
        - hh.directional_sums(x[1:64], y[1:64], v[1:64], az, tol, bw, edges)[0]
    assert np.array_equal(counts - rest - last, want)  # what station 64 adds beyond its pairs with stations 1 .. 63: the coincident pair
    assert np.isfinite(lags[counts > 0]).all() and np.isfinite(semi[counts > 0]).all()


@pytest.mark.parametrize("name", sorted(hh.MAP_INPUTS))
def test_the_map_against_the_brute_force(name):
    kw, nx, ny, cdx, cdy = hh.MAP_INPUTS[name]
    x, y, v = hh.stations(**kw)
    semi, counts = vg.variogram_map(x, y, v, nx, ny, cdx, cdy)
    rc, rs, margin = hh.map_reference(name)
    assert margin >= hh.MARGIN
    assert counts.dtype == np.int64 and counts.shape == (2 * ny + 1, 2 * nx + 1) and np.array_equal(counts, rc)
    ws = hh.mean_ratio(semi, rs, rc[None])
    print("%s: worst err / bar %.3g" % (name, ws))
    assert ws <= 1.0
    # exactly point-symmetric: the same counts and the same bits in mirrored cells
    assert np.array_equal(counts, counts[::-1, ::-1])
    assert np.array_equal(semi.view(np.int64), semi[:, ::-1, ::-1].copy().view(np.int64))
    dx, dy, _, _ = hh._pairs(x, y, v, np.float64)
    inside = (np.abs(np.floor(dx / cdx + 0.5)) <= nx) & (np.abs(np.floor(dy / cdy + 0.5)) <= ny)
    assert counts.sum() == 2 * inside.sum() and counts[ny, nx] >= 2
    one, c1 = vg.variogram_map(x, y, v[:, 1], nx, ny, cdx, cdy)
    assert one.shape == counts.shape and np.array_equal(c1, counts)
    assert hh.mean_ratio(one[None], rs[1:2], rc[None]) <= 1.0


def test_the_limits_run_and_one_more_is_refused():
    name = "limits_n129"
    lags, semi, counts = _run(name)
    assert counts.shape == (vg.MAXDIRS, vg.MAXLAGS)
    _check(name, lags, semi, counts)
    kw, az, tol, bw, edges = hh.INPUTS[name]
    x, y, v = hh.stations(**kw)
    with pytest.raises(ValueError, match="at most 16 azimuths"):
        vg.directional_variogram(x, y, v[:, 0], list(az) + [5.0], edges=edges)
    with pytest.raises(ValueError, match="at most 64 lag bins"):
        vg.directional_variogram(x, y, v[:, 0], az, edges=hh.edges_of(vg.MAXLAGS + 1, 9.0))
    with pytest.raises(ValueError, match="at most 64 lag bins"):
        vg.directional_variogram(x, y, v[:, 0], az, nlags=vg.MAXLAGS + 1)


def test_a_kriging_object_executes_the_same_bits_before_and_after():
    obj, _ = cv.global_case("ok2d_exponential_n67")
    gx, gy = np.linspace(0.0, 1.0, 23), np.linspace(0.0, 1.0, 19)
    z0, s0 = obj.execute("grid", gx, gy)
    z0, s0 = np.array(z0), np.array(s0)
    lags, semi, counts = obj.directional_variogram([0.0, 45.0, 90.0, 135.0], nlags=5)
    assert counts.shape == (4, 5) and counts.sum() > 0
    m, c = obj.variogram_map(4, 4, 0.1, 0.1)
    assert c.shape == (9, 9) and np.array_equal(c, c[::-1, ::-1])
    z1, s1 = obj.execute("grid", gx, gy)
    assert np.array_equal(np.asarray(z1).view(np.int64), z0.view(np.int64)) and np.array_equal(np.asarray(s1).view(np.int64), s0.view(np.int64))
