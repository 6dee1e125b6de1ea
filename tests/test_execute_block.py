"""execute_block on the device: block kriging of cell averages from the one resident inverse (mik_k_block.h).

The reference is brute force in extended precision (tests/test_execute_block_host.py: reference, cached per session): the raw nodes of
every block through `adjusted`, ek.right_hand_sides averaged over the nodes in longdouble, ek.refined_solve, gbar in longdouble.  The bar
of sigma^2 is execute_cov's, C_BAR u (cond_1(A) + M) bscale with bscale the largest |b| over the block's nodes, capped at
1e-6 max(1, max|sigma^2|); the bar of z is ek.bars' z bar.  Every assertion is worst err / bar <= 1.

Worst err / bar (z, sigma^2) on an MI355X.  130 blocks of 3 nodes per axis: ok2d_exponential_n67 0.0035, 0.025;
ok2d_spherical_n130_values_1e3 0.0023, 0.015; ok3d_gaussian_aniso_n40 0.0034, 0.017; uk2d_regional_linear_n67 0.0015, 0.019;
uk3d_functional_n40 0.0035, 0.020.  Against the block means of execute_cov (9 blocks, 2 nodes per axis): at most 0.0007, 0.024.
n_disc = 1: execute()'s bits on the four dense cases; the spherical case 0.0022, 0.015 (its range-aware execute(): 0.0023, 0.0028).
P = 1, 7, 8, 9, 127, 128, 129: at most 0.0035, 0.025; 512 nodes (8 x 8 x 8, 9 blocks, 3-D): 0.0024, 0.0071."""
import numpy as np
import pytest

from pykrige_amd import _lib, core
from tests import _cv_cases as cv
from tests import test_execute_block_host as bh
from tests import test_execute_cov_host as ch

pytestmark = pytest.mark.gpu

EDGE = "ok2d_exponential_n67"
SPHERICAL = "ok2d_spherical_n130_values_1e3"
D3 = "ok3d_gaussian_aniso_n40"


def _bits(a, b):
    a, b = np.ascontiguousarray(np.asarray(a), dtype=np.float64), np.ascontiguousarray(np.asarray(b), dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cols(pts):
    return tuple(np.ascontiguousarray(pts[:, k]) for k in range(pts.shape[1]))


def _centres(name, npt):
    return _cols(ch.points(name)[:npt])


# ------------------------------------------------------------------------------------------------------------- against brute force
@pytest.mark.parametrize("name", bh.CASES)
def test_blocks_are_inside_the_bars_of_the_brute_force(name):
    """130 blocks (two point blocks; M = 131 of the spherical case gives two station blocks), 3 nodes per axis, block sizes about a
    twentieth of the station extent and unequal per axis.  Blocks 0, 1 and 2 are centred on stations: their centre node hits
    exact_values.  Always the dense path."""
    m, st = cv.global_case(name)
    n_disc = bh.per_axis(name, bh.N_DISC)
    z, ss = m.execute_block("points", *_centres(name, bh.P_BRUTE), bh.block_size(name), n_disc=n_disc)
    assert m.last_timing["sparse"] == 0 and m.last_timing["contract_launches"] == 1
    assert z.shape == (bh.P_BRUTE,) and ss.shape == (bh.P_BRUTE,)
    ref = bh.reference(name, n_disc, bh.P_BRUTE)
    rz, rs = bh.worst_ratios(ref, z, ss)
    print("%s: worst err / bar z %.3g sigma^2 %.3g" % (name, rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)
    z0, s0 = m.execute("points", *_centres(name, bh.P_BRUTE))
    assert type(z) is type(z0) and type(ss) is type(s0) and z.dtype == z0.dtype
    off = [q for q in range(bh.P_BRUTE) if q not in ch.ON_STATION]
    assert np.all(np.asarray(ss)[off] < np.asarray(s0)[off])  # the variance of a block mean is below the point variance at its centre


# ------------------------------------------------------------------------------------------------------------- against execute_cov
@pytest.mark.parametrize("name", bh.CASES)
def test_a_block_is_the_mean_of_its_nodes_in_execute_cov(name):
    """9 blocks of 2 nodes per axis: zvalues is the per-block mean of execute_cov's z on the nodes and sigmasq the mean of the matching
    nd x nd block of its matrix, both to the bars."""
    m, st = cv.global_case(name)
    npt, n_disc = 9, bh.per_axis(name, 2)
    nodes = bh.raw_nodes(name, n_disc, npt)
    nd = nodes.shape[1]
    zc, cov = m.execute_cov("points", *_cols(nodes.reshape(-1, st.ndim)))
    z, ss = m.execute_block("points", *_centres(name, npt), bh.block_size(name), n_disc=n_disc)
    zmean = np.asarray(zc).reshape(npt, nd).mean(axis=1)
    smean = np.array([cov[q * nd:(q + 1) * nd, q * nd:(q + 1) * nd].mean() for q in range(npt)])
    bz, bs = bh.bars(bh.reference(name, n_disc, npt))
    rz, rs = float((np.abs(np.asarray(z) - zmean) / bz).max()), float((np.abs(np.asarray(ss) - smean) / bs).max())
    print("%s: worst |block - mean of execute_cov| / bar z %.3g sigma^2 %.3g" % (name, rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)


# ------------------------------------------------------------------------------------------------------------- n_disc = 1
@pytest.mark.parametrize("name", bh.CASES)
def test_one_node_is_execute(name):
    """n_disc = 1: the node is the centre.  Where execute() takes the dense path the bits are execute()'s; the spherical case's execute()
    is range-aware (another rounding of the same numbers) and agrees to the bar."""
    m, st = cv.global_case(name)
    p = _centres(name, bh.P_BRUTE)
    z0, s0 = [np.array(a) for a in m.execute("points", *p)]
    sparse = m.last_timing["sparse"]
    assert sparse == (name == SPHERICAL)
    z, ss = m.execute_block("points", *p, bh.block_size(name), n_disc=1)
    assert m.last_timing["sparse"] == 0
    if not sparse:
        assert _bits(z, z0) and _bits(ss, s0)
    ref = bh.reference(name, bh.per_axis(name, 1), bh.P_BRUTE)
    rz, rs = bh.worst_ratios(ref, z, ss)
    r0z, r0s = bh.worst_ratios(ref, z0, s0)
    print("%s: n_disc = 1 worst err / bar z %.3g sigma^2 %.3g (execute: %.3g %.3g)" % (name, rz, rs, r0z, r0s))
    assert rz <= 1.0 and rs <= 1.0 and r0z <= 1.0 and r0s <= 1.0, (name, rz, rs, r0z, r0s)


# ------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("npt,nd3", [(1, 0), (7, 0), (8, 0), (9, 0), (127, 0), (128, 0), (129, 0), (9, 8)])
def test_edge_counts(npt, nd3):
    """P around the 8-point workgroup and the 128-point panel (3 x 3 nodes), and the most nodes a block can have: 8 x 8 x 8 = 512 on
    the 3-D case, 9 blocks."""
    name = D3 if nd3 else EDGE
    m, _ = cv.global_case(name)
    n_disc = bh.per_axis(name, nd3 or bh.N_DISC)
    z, ss = m.execute_block("points", *_centres(name, npt), bh.block_size(name), n_disc=n_disc)
    assert z.shape == (npt,) and ss.shape == (npt,)
    ref = bh.reference(name, n_disc, bh.P_BRUTE if not nd3 else npt)
    rz, rs = bh.worst_ratios(ref, z, ss)
    print("%s P = %d n_disc = %s: worst err / bar z %.3g sigma^2 %.3g" % (name, npt, n_disc, rz, rs))
    assert rz <= 1.0 and rs <= 1.0, (npt, n_disc, rz, rs)


# ------------------------------------------------------------------------------------------------------------- bits and independence
def _resident(h, n=30, npt=10, **kw):
    rng = np.random.default_rng(3)
    x, y, v = rng.random(n), rng.random(n), rng.random(n)
    h.set_problem(2, x, y, None, v, _lib.MODEL_IDS["exponential"], [1.0, 0.5, 0.02], **kw)
    h.set_points(rng.random(npt), rng.random(npt))


def test_bits_and_independence():
    m, st = cv.global_case(EDGE)
    size, n_disc = bh.block_size(EDGE), (3, 2)
    # chunk = 128 over 300 blocks gives the bits of one launch
    p = _centres(EDGE, ch.P_FULL)
    z1, s1 = [np.array(a) for a in m.execute_block("points", *p, size, n_disc=n_disc)]
    assert m.last_timing["contract_launches"] == 1
    h = m._get_handle()
    h.set_option("chunk", 128)
    try:
        z3, s3 = [np.array(a) for a in m.execute_block("points", *p, size, n_disc=n_disc)]
        assert m.last_timing["contract_launches"] == 3
    finally:
        h.set_option("chunk", 131072)
    assert _bits(z3, z1) and _bits(s3, s1)
    # 'grid' equals 'points' on the meshgrid, in 2-D, with a regional-linear drift and in 3-D with anisotropy
    for name in (EDGE, "uk2d_regional_linear_n67", D3):
        mm, sg = cv.global_case(name)
        lo, hi = sg.coords_orig.min(axis=0), sg.coords_orig.max(axis=0)
        axes = [np.linspace(lo[k], hi[k], n) for k, n in zip(range(sg.ndim), (13, 11, 2))]
        nd = bh.per_axis(name, 2)
        zg, sgd = mm.execute_block("grid", *axes, bh.block_size(name), n_disc=nd)
        assert zg.shape == tuple(a.size for a in reversed(axes)) and sgd.shape == zg.shape
        if sg.ndim == 2:
            gx, gy = np.meshgrid(axes[0], axes[1])
            flat = (gx.ravel(), gy.ravel())
        else:
            gz, gy, gx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
            flat = (gx.ravel(), gy.ravel(), gz.ravel())
        zp, sp = mm.execute_block("points", *flat, bh.block_size(name), n_disc=nd)
        assert _bits(np.asarray(zg).ravel(), zp) and _bits(np.asarray(sgd).ravel(), sp), name
        z0, _ = mm.execute("grid", *axes)
        assert type(zg) is type(z0) and zg.shape == z0.shape
    # execute, execute_fields(valid=...) and execute_cov return their earlier bits after an execute_block
    for name in (EDGE, SPHERICAL):
        mm, sg = cv.global_case(name)
        q = _centres(name, 130)
        rng = np.random.default_rng(7)
        values = sg.values[:, None] * (1.0 + 0.25 * np.arange(3)) + 0.1 * rng.standard_normal((sg.n, 3))
        valid = np.ones(values.shape, dtype=bool)
        valid[[3, 11, 40], 1] = valid[[3, 20], 2] = False

        def everything():
            out = [np.array(a) for a in mm.execute("points", *q)]
            out += [np.array(a) for a in mm.execute_fields("points", *q, values, valid=valid)]
            out += [np.array(a) for a in mm.execute_cov("points", *q)]
            return out

        before = everything()
        mm.execute_block("points", *q, bh.block_size(name), n_disc=2)
        after = everything()
        assert all(_bits(a, b) for a, b in zip(before, after)), name
    # the library's refusals come before any launch and leave the handle usable
    h = _lib.Handle(0)
    off = core.block_node_offsets(2, 0.1, 2)
    with pytest.raises(RuntimeError, match="set the problem first"):
        h.predict_block(off)
    _resident(h, pseudo_inv=1)
    with pytest.raises(ValueError, match="pseudo_inv"):
        h.predict_block(off)
    _resident(h)
    for bad in (np.zeros((0, 2)), np.zeros((513, 2))):
        with pytest.raises(ValueError, match="discretisation nodes"):
            h.predict_block(bad)
    with pytest.raises(ValueError, match="not finite"):
        h.predict_block(np.array([[0.0, np.nan]]))
    _resident(h, geographic=True)
    with pytest.raises(ValueError, match="geographic"):
        h.predict_block(off)
    _resident(h)
    rng = np.random.default_rng(8)
    h.set_fields(rng.random((2, 30)))
    try:
        with pytest.raises(ValueError, match="value fields"):
            h.predict_block(off)
    finally:
        h.set_fields(None)
    h.set_custom_variogram(lambda d: 0.1 + d)
    try:
        h.set_problem(2, rng.random(30), rng.random(30), None, rng.random(30), _lib.MODEL_IDS["custom"], [0.0, 0.0, 0.0])
        h.set_points(rng.random(10), rng.random(10))
        with pytest.raises(ValueError, match="custom variogram"):
            h.predict_block(off)
    finally:
        h.set_custom_variogram(None)
    z = np.empty(10)
    with pytest.raises(RuntimeError, match="predict first"):  # nothing ran
        _lib.check(h._lib.mik_get_results(h._h, _lib._ptr(z), _lib._ptr(z)))
    _resident(h)  # the same handle kriges blocks, and factors by itself (no factor() above)
    h.predict_block(off)
    zb, sb = [np.array(a) for a in h.get_results()]
    h.predict_block(np.zeros((1, 2)))
    z1, s1 = [np.array(a) for a in h.get_results()]
    h.predict()
    z0, s0 = [np.array(a) for a in h.get_results()]
    assert _bits(z1, z0) and _bits(s1, s0) and np.all(np.isfinite(zb)) and np.all(sb < s0)
    h.close()
    g = _lib.Handle(0)
    g.set_devices(2, alias=True)
    _resident(g)
    with pytest.raises(ValueError, match="device group"):
        g.predict_block(off)
    g.close()
