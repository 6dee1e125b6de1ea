"""vecchia_grad.VecchiaGradPlan / neg_log_likelihood_vecchia_grad / fit_variogram_vecchia_grad on the GPU against the long-double
reference of tests/_vgrad_cases.py.

The bar (derived there, from the dense gradient's of tests/test_likelihood_grad.py): the elimination of a local system Sigma_p of
k_p + 1 rows leaves its inverse with a relative error of about (k_p + 1) 2^-52 kappa_2(Sigma_p); a trace tr(M D) moves by at most
|dM|_F |D|_F and a form a^T D b by about |a| |db| |D|_F.  The term of position p in dlogdet[k] is tr((u u^T / d_p) D) and the term in
dG[k][a][b] is -a_a^T D a_b + a~_a^T D_cc a~_b with a_w = Sigma_p^-1 [w_c ; w_p] and a~_w = S^-1 w_c, so
  |dlogdet[k] - ref| <= sum_p (k_p + 1) 2^-52 kappa_2(Sigma_p) (|u|^2 / d_p) |D|_F,
  |dG[k][a][b] - ref| <= sum_p (k_p + 1) 2^-52 kappa_2(Sigma_p) |D|_F (|a_a| |a_b| + |a~_a| |a~_b|),
D the local block of D_k; an entry whose bar is 0 (the spherical model beyond its range) must be exact.  No margin is added.

The cases sit at the size classes of k_vgrad_solve (m = 1, 16 | 17, 32 | 33, 64), at n = 2, at station counts that are no multiple of
the stations per workgroup, across the 1024-position blocks of the reduction (n = 1025, 2049) and, with a slab of 1024 positions, across
a slab edge, with 1, 8, 9 and 40 columns, ng = 0, 2 and 5, each model, 2-D and 3-D, one coincident pair and a spherical range shorter
than most neighbour distances.  logdet, G, nll and the neighbour lists are held to vecchia.VecchiaPlan's bit for bit.  Every figure is
printed before it is asserted; profiles/vecchia_grad_parity.txt holds them."""
import functools
import math
import os

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import likelihood as lk
from pykrige_amd import vecchia as vc
from pykrige_amd import vecchia_grad as vgd
from tests import _grad_cases as gc
from tests import _vgrad_cases as vg

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def record(line):
    """Print a figure, and append it to the file the environment variable VECCHIA_GRAD_PARITY_OUT names (never by default): how
    profiles/vecchia_grad_parity.txt is written."""
    print(line)
    path = os.environ.get("VECCHIA_GRAD_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def device(name):
    """(logdet, G, dlogdet, dG) of CASES[name] from the device, once; do not write into it."""
    case = vg.CASES[name]
    adj, dco, W, order, _ = vg.problem(name)
    with vgd.VecchiaGradPlan(adj, m=case["m"], order=order) as plan:
        return plan.grad(adj, dco, case["model"], case["par"], W)


@pytest.mark.parametrize("name", sorted(vg.CASES))
def test_the_derivatives_are_within_their_bar_and_the_pieces_are_grams_bit_for_bit(name):
    case = vg.CASES[name]
    adj, dco, W, order, nbr = vg.problem(name)
    ref = vg.reference(name)
    got = device(name)
    K, mc = 3 + case["ng"], case["cols"]
    assert got[2].shape == (K,) and got[3].shape == (K, mc, mc) and all(np.all(np.isfinite(g)) for g in got)
    fl, fg = vg.worst(got, name)
    record("plan.grad %-16s N %4d m %2d cols %2d ng %d worst kappa_2 %8.3g  |dlogdet - ref| / bar %8.3g  |dG - ref| / bar %8.3g"
           % (name, case["n"], case["m"], mc, case["ng"], ref[6], fl, fg))
    assert fl <= 1.0 and fg <= 1.0, (name, fl, fg)
    assert all(np.array_equal(got[3][k], got[3][k].T) for k in range(K))  # exactly symmetric
    with vc.VecchiaPlan(adj, m=case["m"], order=order) as plan6, vgd.VecchiaGradPlan(adj, m=case["m"], order=order) as plan:
        # logdet and G are mvc_plan_gram's bits, the neighbour lists mvc_plan_neighbours' (and the host's)
        logdet6, G6 = plan6.gram(adj, case["model"], case["par"], W)
        assert got[0] == logdet6 and np.array_equal(bits(got[1]), bits(G6))
        assert np.array_equal(plan.neighbours, plan6.neighbours) and np.array_equal(plan.neighbours, nbr)
        # two calls return the same bits
        assert same(plan.grad(adj, dco, case["model"], case["par"], W), got)
        # an entry depends only on its two columns: a permutation with a column added, and single columns
        pick = [mc - 1, 0] + ([mc // 2] if mc > 2 else [])
        sub = plan.grad(adj, dco, case["model"], case["par"], np.column_stack([W[:, pick], np.ones(len(W))]))
        for a_, a in enumerate(pick):
            for b_, b in enumerate(pick):
                assert np.array_equal(bits(sub[3][:, a_, b_]), bits(got[3][:, a, b])) and sub[1][a_, b_] == got[1][a, b], (name, a, b)
        assert np.array_equal(bits(sub[2]), bits(got[2]))
        # fewer geometry parameters leave the others alone
        if case["ng"]:
            none = plan.grad(adj, None, case["model"], case["par"], W)
            assert none[2].shape == (3,) and np.array_equal(bits(none[2]), bits(got[2][:3])) and np.array_equal(bits(none[3]), bits(got[3][:3]))


@pytest.mark.parametrize("name", vg.SLAB_CASES)
def test_a_slab_edge_changes_no_bit(name, monkeypatch):
    case = vg.CASES[name]
    adj, dco, W, order, _ = vg.problem(name)
    monkeypatch.setenv("MIK_VGRAD_SLAB", "1024")  # two or three slabs instead of one
    with vgd.VecchiaGradPlan(adj, m=case["m"], order=order) as plan:
        cut = plan.grad(adj, dco, case["model"], case["par"], W)
        monkeypatch.delenv("MIK_VGRAD_SLAB")
        whole = plan.grad(adj, dco, case["model"], case["par"], W)
    assert same(cut, device(name)) and same(whole, device(name))


def test_beyond_a_short_spherical_range_the_derivatives_are_exact_zeros():
    name = "g200_sph_short"
    case = vg.CASES[name]
    adj, dco, W, order, nbr = vg.problem(name)
    r, d, dr, dd = vg.pieces(adj, dco, order, nbr, case["model"], case["par"], W)
    alone = np.all(dr == 0, axis=(1, 2))  # positions whose neighbours all lie beyond the range
    assert alone.sum() > len(adj) // 2 and np.all(dd[alone][:, [1, 3, 4]] == 0) and np.all(dd[alone][:, [0, 2]] == 1)
    assert vg.worst(device(name), name) <= (1.0, 1.0)


def test_a_trial_that_is_not_positive_definite_answers_and_writes_nothing():
    from tests import _lik_cases as lc

    for cname, kind, station in (("notpd_n2", "identity", 2), ("notpd_n200", "identity", 151)):
        case, _ = lc.NOT_PD[cname]
        X, W = lc.inputs(case)
        order = np.arange(case["n"], dtype=np.int32)
        dco = np.zeros((2,) + X.shape)
        with vgd.VecchiaGradPlan(X, m=5, order=order) as plan:
            got = plan.grad(X, dco, case["model"], case["par"], W)
            assert got[0] == math.inf and all(np.all(np.isnan(g)) for g in got[1:]) and got[2].shape == (5,)
            # the C call: the station, and no result written
            import ctypes as C
            mc = W.shape[1]
            G, dl, dG = np.full((mc, mc), 7.0), np.full(5, 7.0), np.full((5, mc, mc), 7.0)
            logdet, info = C.c_double(7.0), C.c_int32(0)
            p = lambda a: a.ctypes.data_as(vgd._dp)
            ct, wt, dt = np.ascontiguousarray(X.T), np.ascontiguousarray(W.T), np.ascontiguousarray(dco.transpose(0, 2, 1))
            rc = vgd.load().mvg_plan_grad(plan._handle, p(ct), 2, p(dt), lk.MODEL_IDS[case["model"]], *case["par"], p(wt), mc, C.byref(logdet),
                                          p(G), p(dl), p(dG), C.byref(info))
            assert rc == vgd.MVG_ENOTPD and info.value == station and b"not positive definite" in vgd.load().mvg_last_error()
            assert logdet.value == 7.0 and np.all(G == 7.0) and np.all(dl == 7.0) and np.all(dG == 7.0)
        x, y = X[:, 0], X[:, 1]
        full = [case["par"][0] + case["par"][2], case["par"][1], case["par"][2]]
        nll, grad = vgd.neg_log_likelihood_vecchia_grad(x, y, W[:, 0], case["model"], full, m=5, order=order)
        assert nll == math.inf and grad.shape == (5,) and np.all(np.isnan(grad))


def _problem(n, ndim, seed, nf=1):
    rng = np.random.default_rng(seed)
    raw = rng.random((n, ndim)) * ([3.0, 2.0, 1.0][:ndim])
    v = np.sin(2.0 * raw[:, 0])[:, None] + 0.5 * raw[:, 1][:, None] + 0.4 * rng.standard_normal((n, nf))
    return raw, v


@pytest.mark.parametrize("ndim,drift", [(2, "array"), (3, "regional_linear")])
def test_nll_is_the_vecchia_likelihoods_bit_for_bit_and_plane_f_is_the_one_field_call(ndim, drift):
    raw, v = _problem(129, ndim, 11 + ndim, nf=3)
    full = [1.2, 0.9, 0.1]
    anis = dict(anisotropy_scaling=1.7, anisotropy_angle=25.0) if ndim == 2 else dict(
        anisotropy_scaling_y=1.4, anisotropy_scaling_z=0.6, anisotropy_angle_x=10.0, anisotropy_angle_y=-20.0, anisotropy_angle_z=35.0)
    names = lk.GRAD_NAMES_2D if ndim == 2 else lk.GRAD_NAMES_3D
    if drift == "array":
        drift = np.column_stack([raw[:, 0], raw[:, 0] * raw[:, 1]])
    for reml in (False, True):
        kw = dict(m=12, seed=3, drift=drift, reml=reml, **anis)
        nll, grad = vgd.neg_log_likelihood_vecchia_grad(*raw.T, v, "exponential", full, **kw)
        want = vc.neg_log_likelihood_vecchia(*raw.T, v, "exponential", full, **kw)
        assert nll.shape == (3,) and grad.shape == (3, len(names)) and np.array_equal(bits(nll), bits(want)) and np.all(np.isfinite(grad))
        for f in range(3):
            one, g1 = vgd.neg_log_likelihood_vecchia_grad(*raw.T, v[:, f], "exponential", full, **kw)
            assert isinstance(one, float) and one == nll[f] and g1.shape == (len(names),) and np.array_equal(bits(g1), bits(grad[f]))


def test_with_every_predecessor_as_neighbour_the_gradient_is_the_dense_one():
    """m >= n - 1 at n = 60: Vecchia's objective is the exact likelihood, so ``neg_log_likelihood_vecchia_grad`` and the dense
    ``neg_log_likelihood_grad`` agree within the sum of their bars.  The dense bar is tests/_grad_cases.py's; Vecchia's is this file's,
    taken through ``nll_grad_from_gram`` -- which is linear in dlogdet and dG -- entry by entry with the absolute values of its weights:
    1/2 [bar_dlogdet + bar_vv - 2 |beta|^T bar_xv + |beta|^T bar_xx |beta| + (REML) sum |G_xx^-1| bar_xx]."""
    name = "g60_exact"
    case = vg.CASES[name]
    raw, W = vg.inputs(name)
    sc, an = vg.anisotropy(case)
    anis = dict(anisotropy_scaling=sc[0], anisotropy_angle=an[0])
    v = W[:, 0]
    full = [case["par"][0] + case["par"][2], case["par"][1], case["par"][2]]
    adj, dco, _, order, nbr = vg.problem(name)
    X = np.ones((case["n"], 1))
    Wx = np.column_stack([v, X])
    r, d, dr, dd, nm = vg.pieces(adj, dco, order, nbr, case["model"], case["par"], Wx, norms=True)
    w = nm["size"] * vg.U * nm["kappa"]
    bar_l = np.sum((w * nm["uu"])[:, None] * nm["D"], axis=0)
    pair = nm["a"][:, :, None] * nm["a"][:, None, :] + nm["at"][:, :, None] * nm["at"][:, None, :]
    bar_G = np.einsum("p,pk,pab->kab", w, nm["D"], pair)
    _, G, _, _ = vg.totals(r, d, dr, dd)
    G = G.astype(np.float64)
    beta, gi = abs(G[1, 0] / G[1, 1]), abs(1.0 / G[1, 1])
    for reml in (False, True):
        nll, grad = vgd.neg_log_likelihood_vecchia_grad(*raw.T, v, case["model"], full, m=case["m"], reml=reml, **anis)
        nll_d, grad_d = lk.neg_log_likelihood_grad(*raw.T, v, case["model"], full, reml=reml, **anis)
        ref, scale, kappa = gc.gradient_ld(adj, dco, case["model"], case["par"], v[:, None], X, reml)
        bar_dense = case["n"] * gc.U * kappa * scale[0]
        bar_v = 0.5 * (bar_l + bar_G[:, 0, 0] + 2.0 * beta * bar_G[:, 1, 0] + beta * beta * bar_G[:, 1, 1] + (gi * bar_G[:, 1, 1] if reml else 0.0))
        frac = np.abs(grad - grad_d) / (bar_dense + bar_v)
        print("REML" if reml else "ML  ", "|vecchia - dense| / (sum of the bars):", " ".join("%.3g" % f for f in frac), " nll", nll, nll_d)
        assert np.all(frac <= 1.0)
        assert np.all(np.abs(grad.astype(gc.LD) - ref[0]) <= bar_dense + bar_v)


@functools.lru_cache(maxsize=None)
def _simulated():
    """A few hundred stations of a known anisotropic exponential model."""
    from tests import _lik_cases as lc

    rng = np.random.default_rng(77)
    n = 300
    raw = rng.random((n, 2)) * [4.0, 3.0]
    Cm = lc.covariance_ld(lk._adjust(raw, [2.0], [30.0]), "exponential", [0.95, 1.2, 0.05]).astype(np.float64)
    return raw[:, 0], raw[:, 1], 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)


def test_the_quasi_newton_fit_reaches_the_simplex_fit_in_fewer_evaluations():
    x, y, v = _simulated()
    start = [1.5, 0.6, 0.2]
    kw = dict(m=10, start=start, fit_anisotropy=True)
    at_start = vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=10)
    fit = vgd.fit_variogram_vecchia_grad(x, y, v, "exponential", **kw)
    simplex = vc.fit_variogram_vecchia(x, y, v, "exponential", **kw)
    print(fit, fit.message)
    print(simplex, simplex.message)
    assert isinstance(fit, lk.MLFit) and fit.success and math.isfinite(fit.nll) and fit.nll <= at_start
    assert fit.nll <= simplex.nll + 1e-6  # the simplex search's own tolerance in the objective (fatol)
    assert fit.n_evaluations < simplex.n_evaluations
    ok = pa.OrdinaryKriging(x, y, v, variogram_model="exponential", variogram_parameters=start)
    again = ok.fit_variogram_vecchia_grad(m=10, fit_anisotropy=True)
    assert again.nll == fit.nll and again.variogram_parameters == fit.variogram_parameters and again.anisotropy == fit.anisotropy
    nll, grad = vgd.neg_log_likelihood_vecchia_grad(x, y, v, "exponential", start, m=10)
    nll_c, grad_c = ok.neg_log_likelihood_vecchia_grad(m=10)
    assert nll == nll_c == at_start and np.array_equal(bits(grad), bits(grad_c))
    rng = np.random.default_rng(5)
    z = rng.random(len(x))
    ok3 = pa.OrdinaryKriging3D(x, y, z, v, variogram_model="exponential", variogram_parameters=start)
    nll3, grad3 = ok3.neg_log_likelihood_vecchia_grad(m=10)
    want3 = vgd.neg_log_likelihood_vecchia_grad(x, y, z, v, "exponential", start, m=10)
    assert nll3 == want3[0] == ok3.neg_log_likelihood_vecchia(m=10) and np.array_equal(bits(grad3), bits(want3[1])) and grad3.shape == (8,)
