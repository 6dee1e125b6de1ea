"""execute_block_window() on the device: every block kriged from the k stations nearest to its centre (mik_predict_block_window).

Every case of tests/_mwblock_cases.py is held, over all its blocks, to the bar of the moving-window kernels -- C u (cond_1 + k + 1) max|v|
on z and C u (cond_1 + k + 1) max|b| on sigma^2 with cond_1 of each block's LOCAL system, max|b| over the block's nodes, C = 8 -- against
the brute-force extended-precision reference, and asserts the solver that ran where the case names one.  The bit-for-bit checks tie
n_disc = 1 to execute() with a window, show that the block right-hand sides read the centres in the order the job runs in, and that the
call and the existing ones leave each other's results alone.

Worst err / bar recorded on an MI355X (z, sigma^2): exponential_n300_k10_3x3 0.0051, 0.0034 (exact_values=False: 0.0051, 0.0034);
exponential_n300_k257_2x2 3.5e-05, 4.0e-05; gaussian_n450_k100_2x2 7.6e-05, 5.7e-05; hole_effect_n200_k130_2x2 6.6e-04, 3.2e-04;
hole_effect_n200_k20_2x2 0.0016, 0.0013; linear_n100_k10_3x3 0.0028, 0.0073; ok3d_aniso_n400_k24_2x2x2 0.0019, 0.0031;
ok3d_aniso_n400_k24_8x8x8 0.0101, 0.0057; spherical_n300_k16_2x3 0.0011, 0.0017; spherical_n300_k17_2x3 8.7e-04, 0.0020; k = N = 12 against
the global reference: the window 0.0038, 0.0029, execute_block 0.0050, 0.023."""
import numpy as np
import pytest

from tests import _cvw_cases as cw
from tests import _mwblock_cases as mb

pytestmark = pytest.mark.gpu


def _cols(ctr):
    return [np.ascontiguousarray(ctr[:, d]) for d in range(ctr.shape[1])]


def _run(obj, ctr, bsize, k, n_disc, style="points", **kw):
    return obj.execute_block_window(style, *_cols(ctr), bsize, k, n_disc=n_disc, **kw)


@pytest.mark.parametrize("name", sorted(mb.CASES))
def test_every_block_is_within_the_bar_of_its_local_system(name):
    obj, st, k, kernel, ctr, bsize, n_disc = mb.case(name)
    ref = mb.reference(name)
    z, ss = _run(obj, ctr, bsize, k, n_disc)
    assert z.shape == (len(ctr),) and ss.shape == (len(ctr),) and z.dtype == np.float64 and ss.dtype == np.float64
    rz, rs = mb.worst_ratios(ref, z, ss)
    print("%s: N %d k %d nd %d  mw_kernel %d  worst cond_1 %.3g  |dz| / bar %.3g  |dss| / bar %.3g" % (
        name, st.n, k, int(np.prod(n_disc)), obj.last_timing["mw_kernel"], float(ref.cond.max()), rz, rs))
    if kernel is not None:
        assert obj.last_timing["mw_kernel"] == kernel, (name, obj.last_timing["mw_kernel"])
    assert rz <= 1.0 and rs <= 1.0, (name, rz, rs)


def test_exact_values_false_on_a_rebuilt_object():
    name = mb.INEXACT
    obj, st, k, kernel, ctr, bsize, n_disc = mb.case(name)
    twin, _ = mb.inexact_twin(mb.CASES[name][0])
    ref = mb.reference(name, exact=False)
    z, ss = _run(twin, ctr, bsize, k, n_disc)
    rz, rs = mb.worst_ratios(ref, z, ss)
    print("%s, exact_values=False: |dz| / bar %.3g  |dss| / bar %.3g" % (name, rz, rs))
    assert twin.last_timing["mw_kernel"] == kernel
    assert rz <= 1.0 and rs <= 1.0, (rz, rs)
    # the station-centred blocks are where the two objects differ: the centre node is an exact hit for the one, not for the other
    ze, _ = _run(obj, ctr, bsize, k, n_disc)
    on = list(mb.ON_STATION)
    assert np.all(ze[on] != z[on])


def test_k_equal_n_and_the_global_execute_block_share_one_reference():
    obj, st, k, ctr, bsize, n_disc, gref = mb.k_is_n()
    zw, sw = _run(obj, ctr, bsize, k, n_disc)
    zg, sg = obj.execute_block("points", *_cols(ctr), bsize, n_disc=n_disc)
    for what, z, ss in (("window k = N", zw, sw), ("execute_block", zg, sg)):
        rz, rs = mb.worst_ratios(gref, z, ss)
        print("%s: |dz| / bar %.3g  |dss| / bar %.3g" % (what, rz, rs))
        assert rz <= 1.0 and rs <= 1.0, (what, rz, rs)


@pytest.mark.parametrize("name", ["exponential_n300_k10_3x3", "gaussian_n450_k100_2x2", "hole_effect_n200_k20_2x2"])
def test_n_disc_one_has_the_bits_of_execute_with_a_window(name):
    obj, st, k, _, ctr, bsize, _ = mb.case(name)
    cols = _cols(ctr)
    z1, s1 = obj.execute_block_window("points", *cols, bsize, k, n_disc=1)
    z0, s0 = obj.execute("points", *cols, backend="loop", n_closest_points=k)
    assert np.array_equal(np.asarray(z1), np.asarray(z0)) and np.array_equal(np.asarray(s1), np.asarray(s0))
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    gx, gy = np.linspace(lo[0], hi[0], 9), np.linspace(lo[1], hi[1], 7)
    zg1, sg1 = obj.execute_block_window("grid", gx, gy, bsize, k, n_disc=(1, 1))
    zg0, sg0 = obj.execute("grid", gx, gy, backend="loop", n_closest_points=k)
    assert zg1.shape == (7, 9) and np.array_equal(np.asarray(zg1), np.asarray(zg0)) and np.array_equal(np.asarray(sg1), np.asarray(sg0))


def test_the_answer_of_a_block_does_not_depend_on_the_call_it_is_in():
    """4224 shuffled centres at k = 10 run in Hilbert-curve order on the device: the block right-hand sides have to read the centres in
    that order, not in the caller's."""
    obj, st, k, _, ctr, bsize, n_disc = mb.case("exponential_n300_k10_3x3")
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    big = lo + (hi - lo) * np.random.default_rng(77).random((4224, 2))
    pick = np.random.default_rng(78).permutation(4224)[:130]
    zb, sb = _run(obj, big, bsize, k, n_disc)
    assert obj.last_timing["points_sorted"] == 1
    sub = big[pick]
    z1, s1 = _run(obj, sub, bsize, k, n_disc)
    assert np.array_equal(z1, zb[pick]) and np.array_equal(s1, sb[pick])
    for per in (1, 7, 64, 65):
        zs, ss = [], []
        for i in range(0, 130, per):
            z, s = _run(obj, sub[i:i + per], bsize, k, n_disc)
            zs.append(z), ss.append(s)
        assert np.array_equal(np.concatenate(zs), z1) and np.array_equal(np.concatenate(ss), s1), per


def test_a_block_has_a_lower_variance_than_its_centre():
    obj, st, k, _, ctr, bsize, n_disc = mb.case("exponential_n300_k10_3x3")
    off = [q for q in range(len(ctr)) if q not in mb.ON_STATION]
    _, sv = _run(obj, ctr, bsize, k, n_disc)
    _, sp = obj.execute("points", *_cols(ctr), backend="loop", n_closest_points=k)
    assert np.all(sv[off] < np.asarray(sp)[off])


def test_a_singular_window_raises_as_execute_does():
    """A window of 8 at (10, 10) holds the coincident pair of tests/_cvw_cases' pair sets.  With their nugget of 0.02 the two stations'
    rows differ by gamma(0) and the local system is regular: execute() with a window answers there, and so does the block call, inside the
    bar.  The same stations with a zero nugget make the two rows equal and the local system singular: both calls raise, LinAlgError for
    backend 'loop' and ValueError('Singular matrix') for 'C'."""
    import pykrige_amd as pa

    obj, st = cw.station_set("pair_inexact")
    ctr = np.array([[10.0, 10.0]])
    x, y = _cols(ctr)
    bsize, n_disc = (0.05, 0.05), (2, 2)
    assert set(mb.ek.neighbours(st, mb.adjusted(st, ctr), 8)[1][0]) >= set(cw.PAIR)
    obj.execute("points", x, y, backend="loop", n_closest_points=8)  # regular: no error
    for backend in ("loop", "C"):
        z, ss = obj.execute_block_window("points", x, y, bsize, 8, n_disc=n_disc, backend=backend)
        rz, rs = mb.worst_ratios(mb.window_reference(st, 8, ctr, bsize, n_disc), z, ss)
        assert rz <= 1.0 and rs <= 1.0, (backend, rz, rs)
    sing = pa.OrdinaryKriging(obj.X_ORIG, obj.Y_ORIG, obj.Z, variogram_model="exponential", variogram_parameters=[1.0, 0.5, 0.0],
                              exact_values=False)
    with pytest.raises(np.linalg.LinAlgError):
        sing.execute("points", x, y, backend="loop", n_closest_points=8)
    with pytest.raises(np.linalg.LinAlgError):
        sing.execute_block_window("points", x, y, bsize, 8, n_disc=n_disc, backend="loop")
    with pytest.raises(ValueError, match="Singular matrix"):
        sing.execute("points", x, y, backend="C", n_closest_points=8)
    with pytest.raises(ValueError, match="Singular matrix"):
        sing.execute_block_window("points", x, y, bsize, 8, n_disc=n_disc, backend="C")


def test_the_neighbouring_calls_are_unchanged_and_a_resident_factor_stays():
    obj, st, k, _, ctr, bsize, n_disc = mb.case("exponential_n300_k10_3x3")
    gx, gy = np.linspace(0.0, 1.0, 23), np.linspace(0.0, 1.0, 17)
    px, py = np.random.default_rng(9).random((2, 500))
    cols = _cols(ctr)

    def others():
        return (obj.execute("grid", gx, gy), obj.execute("points", px, py, n_closest_points=10, backend="loop"),
                obj.execute_block("points", *cols, bsize, n_disc=n_disc))

    before = others()
    w0 = _run(obj, ctr, bsize, k, n_disc)
    after = others()
    for (a0, a1), (b0, b1) in zip(before, after):
        assert np.array_equal(np.asarray(a0), np.asarray(b0)) and np.array_equal(np.asarray(a1), np.asarray(b1))
    w1 = _run(obj, ctr, bsize, k, n_disc)
    assert np.array_equal(w0[0], w1[0]) and np.array_equal(w0[1], w1[1])
    # a factor resident before the call is still used afterwards
    d0 = obj.execute("grid", gx, gy)
    t0 = dict(obj.last_timing)
    assert obj._factor_key is not None
    w2 = _run(obj, ctr, bsize, k, n_disc)
    d1 = obj.execute("grid", gx, gy)
    # (execute() did not factor again -- the library would refuse a predict without a factor -- and the timing still shows the one factorisation)
    assert obj.factor_reused and obj.last_timing["invert_ms"] == t0["invert_ms"] and obj.last_timing["assemble_ms"] == t0["assemble_ms"]
    assert np.array_equal(np.asarray(d0[0]), np.asarray(d1[0])) and np.array_equal(np.asarray(d0[1]), np.asarray(d1[1]))
    assert np.array_equal(w0[0], w2[0]) and np.array_equal(w0[1], w2[1])


def test_handle_level_refusals_and_the_point_form_of_one_node():
    from pykrige_amd import _lib

    obj, st, k, _, ctr, bsize, n_disc = mb.case("exponential_n300_k10_3x3")
    ca = np.array(obj._coords_adj, dtype=np.float64)
    pa_ = mb.adjusted(st, ctr)
    h = _lib.Handle()
    try:
        h.set_problem(ndim=2, xs=ca[:, 0], ys=ca[:, 1], zs=None, values=st.values, model_id=_lib.MODEL_IDS[obj.variogram_model],
                      params=obj.variogram_model_parameters, eps=obj.eps, exact_values=obj.exact_values)
        h.set_points(pa_[:, 0], pa_[:, 1])
        for bad in (np.zeros((0, 2)), np.zeros((513, 2)), np.array([[np.nan, 0.0]])):
            with pytest.raises(ValueError, match="mik_predict_block_window"):
                h.predict_block_window(bad, k)
        with pytest.raises(ValueError, match="at least two"):
            h.predict_block_window(np.zeros((1, 2)), 1)
        with pytest.raises(ValueError, match="exceeds the number of stations"):
            h.predict_block_window(np.zeros((1, 2)), st.n + 1)
        h.set_fields(np.zeros((2, st.n)))
        with pytest.raises(ValueError, match="value fields"):
            h.predict_block_window(np.zeros((1, 2)), k)
        h.set_fields(None)
        h.predict_block_window(np.zeros((1, 2)), k)
        z1, s1 = (np.array(a) for a in h.get_results())
        h.predict_moving_window(k)
        z0, s0 = h.get_results()
        assert np.array_equal(z1, z0) and np.array_equal(s1, s0)
    finally:
        h.close()
