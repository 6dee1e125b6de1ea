"""vecchia.VecchiaPlan / neg_log_likelihood_vecchia / fit_variogram_vecchia on the GPU against tests/_vecchia_cases.py: the neighbour sets
equal the NumPy restatement exactly, and log det and W^T C^-1 W are held to the long-double brute force within the project's bar --
N 2^-52 kappa_2(C) relative to sqrt(G_aa G_bb) for G, the same number absolutely for logdet, C the full covariance of the case.  The shapes
straddle the size classes of k_vec_solve (m = 15 | 16 | 17, 32 | 33, 64) and the stations one of its workgroups takes in each class
(N = 15 | 16 | 17, 7 | 8 | 9, 3 | 4 | 5), the 64-position blocks and 256-candidate tiles of k_vec_knn (N = 255 | 256 | 257, 512 | 513) and the
1024-position blocks of k_vec_reduce (N = 1023 | 1024 | 1025, 2048 | 2049).  Every figure is printed before it is asserted and appended to profiles/vecchia_parity.txt when the environment
variable VECCHIA_PARITY_OUT names a file."""
import ctypes
import math
import os

import numpy as np
import pytest

import pykrige_amd as pa
from pykrige_amd import core
from pykrige_amd import likelihood as lk
from pykrige_amd import vecchia as vc
from tests import _lik_cases as lc
from tests import _vecchia_cases as vcs

pytestmark = pytest.mark.gpu
LD = np.longdouble


def record(line, edge=False):
    """``edge``: a case of ``_vecchia_cases.EDGE_DEVICE``, also appended to the file FIT_EDGES_PARITY_OUT names."""
    print(line)
    for path in (os.environ.get("VECCHIA_PARITY_OUT"), os.environ.get("FIT_EDGES_PARITY_OUT") if edge else None):
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")


# ------------------------------------------------------------------------------------------------------------- neighbour sets
def _stations(n, ndim, seed=0):
    return np.random.default_rng(900 + 7 * n + ndim + seed).random((n, ndim))


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 333])
def test_the_neighbour_sets_are_the_reference_exactly(n, ndim):
    X = _stations(n, ndim)
    for m in (1, 15, 16, 17, 32, 33, 64):
        with vc.VecchiaPlan(X, m=m) as plan:
            assert plan.n == n and plan.m == m and np.array_equal(plan.order, vcs.order_of(n))
            got = plan.neighbours
        assert got.shape == (n, m) and got.dtype == np.int32
        assert np.array_equal(got, vcs.neighbours_ref(X, plan.order, m)), (n, ndim, m)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("n", vcs.KNN_EDGE_SIZES)
def test_the_neighbour_sets_at_the_edges_of_the_candidate_tile_are_the_reference_exactly(n, ndim):
    """k_vec_knn stages TC = 256 candidates at a time: N = 255 | 256 | 257 and 512 | 513 end on a tile that is one short of full, full,
    or holds a single candidate; m = 1, 16, 33, 64."""
    X = _stations(n, ndim)
    for m in vcs.KNN_EDGE_M:
        with vc.VecchiaPlan(X, m=m) as plan:
            got = plan.neighbours
        assert got.shape == (n, m) and np.array_equal(got, vcs.neighbours_ref(X, plan.order, m)), (n, ndim, m)


def test_forty_one_columns_are_refused_and_harm_nothing():
    """MVC_MAXCOLS = 40 is a case; 41 is refused by ``VecchiaPlan.gram`` with a ValueError, by the library with MVC_EINVAL, and the valid
    call that follows on the same plan returns the bits it returned before."""
    case = lc.CASES["n129_exp3d_m40"]
    X, W = lc.inputs(case)
    W41 = np.hstack([W, W[:, :1]])
    with vc.VecchiaPlan(X, m=30) as plan:
        first = plan.gram(X, case["model"], case["par"], W)
        with pytest.raises(ValueError, match="MVC_MAXCOLS"):
            plan.gram(X, case["model"], case["par"], W41)
        lib = vc.load()
        ct, wt = np.ascontiguousarray(X.T), np.ascontiguousarray(W41.T)
        out, ld, info = np.full((41, 41), 7.0), ctypes.c_double(7.0), ctypes.c_int32(-5)
        rc = lib.mvc_plan_gram(plan._handle, ct.ctypes.data_as(vc._dp), lk.MODEL_IDS[case["model"]], *case["par"], wt.ctypes.data_as(vc._dp), 41,
                               ctypes.byref(ld), out.ctypes.data_as(vc._dp), ctypes.byref(info))
        assert rc == vc.MVC_EINVAL and b"MVC_MAXCOLS" in lib.mvc_last_error() and ld.value == 7.0 and np.all(out == 7.0)
        again = plan.gram(X, case["model"], case["par"], W)
    assert again[0] == first[0] and np.array_equal(again[1].view(np.int64), first[1].view(np.int64))


def test_ties_go_to_the_smaller_position_and_every_order_is_served():
    g = (np.arange(12) + 0.5) / 12.0
    lattice = np.array([[a, b] for b in g for a in g])  # 12 x 12 in the unit square: many exact ties
    pair = _stations(129, 2, seed=1)
    pair[128] = pair[5]  # one coincident pair
    for X in (lattice, pair, _stations(129, 3, seed=2)):
        n = len(X)
        for order in ("random", "coordinate", np.arange(n - 1, -1, -1)):
            for m in (7, 33, 64):
                with vc.VecchiaPlan(X, m=m, order=order, seed=3) as plan:
                    want = order if not isinstance(order, str) else (
                        np.random.default_rng(3).permutation(n) if order == "random" else np.argsort(X.sum(axis=1), kind="stable"))
                    assert np.array_equal(plan.order, want)
                    assert np.array_equal(plan.neighbours, vcs.neighbours_ref(X, plan.order, m)), (n, order if isinstance(order, str) else "reversed", m)
    with vc.VecchiaPlan(pair, m=3, order=np.arange(129)) as plan:
        assert plan.neighbours[128, 0] == 5  # the coincident station comes first


# ------------------------------------------------------------------------------------------------------------- gram
@pytest.mark.parametrize("name,m", vcs.DEVICE + [("big", vcs.BIG_M)])
def test_gram_is_within_the_bar_symmetric_and_reproducible(name, m):
    case = vcs.case_of(name)
    X, W = vcs.inputs(name)
    order, nbr, ref_logdet, ref_G, kappa, bar = vcs.reference(name, m)
    assert kappa <= lc.KAPPA_MAX
    with vc.VecchiaPlan(X, m=m) as plan:
        assert np.array_equal(plan.neighbours, nbr)
        logdet, G = plan.gram(X, case["model"], case["par"], W)
        again_logdet, again_G = plan.gram(X, case["model"], case["par"], W)
    el, eg = vcs.errors(logdet, G, ref_logdet, ref_G)
    edge = (name, m) in vcs.EDGE_DEVICE
    record("%s%-16s N %4d m %2d cols %2d kappa_2 %9.3g bar %9.3g logdet error %9.3g G error %9.3g worst/bar %8.3g"
           % ("vecchia   " if edge else "", name, case["n"], m, case["m"], kappa, bar, el, eg, max(el, eg) / bar), edge)
    assert G.shape == (case["m"], case["m"]) and np.array_equal(G, G.T)
    assert el <= bar and eg <= bar, (name, m, el, eg, bar)
    assert again_logdet == logdet and np.array_equal(again_G.view(np.int64), G.view(np.int64))  # the same bits
    if m >= case["n"] - 1:  # the exact likelihood: also held to the dense reference
        if name in lc.CASES:
            dense_logdet, dense_G, _, dense_bar = lc.reference(name)
        else:  # (a case of this module alone: the same brute force, the bar of the same kappa_2)
            (dense_logdet, dense_G), dense_bar = lc.brute_force(X, case["model"], case["par"], W), bar
        el, eg = lc.errors(logdet, G, dense_logdet, dense_G)
        record("%-16s against the dense long-double reference: logdet error %9.3g G error %9.3g bar %9.3g" % (name, el, eg, dense_bar))
        assert el <= dense_bar and eg <= dense_bar


@pytest.mark.parametrize("name,m", [("n129_exp3d_m40", 30), ("n333_sph_m7", 20)])
def test_an_entry_of_g_does_not_depend_on_the_columns_beside_it(name, m):
    case = lc.CASES[name]
    X, W = lc.inputs(case)
    with vc.VecchiaPlan(X, m=m) as plan:
        logdet, G = plan.gram(X, case["model"], case["par"], W)
        perm = np.random.default_rng(1).permutation(case["m"])
        for cols in ([0], [2, 0], [case["m"] - 1, 1, 3], list(perm)):
            ld1, G1 = plan.gram(X, case["model"], case["par"], W[:, cols])
            assert ld1 == logdet and np.array_equal(G1.view(np.int64), np.ascontiguousarray(G[np.ix_(cols, cols)]).view(np.int64)), cols


def test_a_plan_serves_other_coordinates():
    """The plan is built in one metric; gram is called with coordinates adjusted by scaling 2, angle 30 degrees: the result is the
    reference on the plan's neighbour lists with the new coordinates."""
    name, m = "n129_pair_m7", 10
    case = lc.CASES[name]
    X, W = lc.inputs(case)
    order, nbr = vcs.reference(name, m)[:2]
    moved = core.adjust_for_anisotropy(X, [0.5, 0.5], [2.0], [30.0])
    ref_logdet, ref_G = vcs.brute_force(moved, order, nbr, case["model"], case["par"], W)
    own = vcs.neighbours_ref(moved, order, m)
    assert not np.array_equal(own, nbr)  # the moved metric would choose other neighbours
    ev = np.linalg.eigvalsh(lc.covariance_ld(moved, case["model"], case["par"]).astype(np.float64))
    bar = case["n"] * lc.U * float(ev[-1] / ev[0])
    with vc.VecchiaPlan(X, m=m) as plan:
        logdet, G = plan.gram(moved, case["model"], case["par"], W)
        assert np.array_equal(plan.neighbours, nbr)
    el, eg = vcs.errors(logdet, G, ref_logdet, ref_G)
    record("%-16s moved coordinates on the plan's lists: bar %9.3g logdet error %9.3g G error %9.3g" % (name, bar, el, eg))
    assert el <= bar and eg <= bar


@pytest.mark.parametrize("name", ["notpd_n2", "notpd_n200"])
@pytest.mark.parametrize("kind", ["identity", "reversed"])
def test_a_system_that_is_not_positive_definite_is_answered_and_harms_nothing(name, kind):
    case, _ = lc.NOT_PD[name]
    X, W = lc.inputs(case)
    order = vcs.order_of(case["n"], kind)
    nbr = vcs.neighbours_ref(X, order, 5)
    none, station = vcs.brute_force(X, order, nbr, case["model"], case["par"], W)
    assert none is None
    with vc.VecchiaPlan(X, m=5, order=order) as plan:
        logdet, G = plan.gram(X, case["model"], case["par"], W)
        assert logdet == math.inf and G.shape == (case["m"],) * 2 and np.all(np.isnan(G))
        lib = vc.load()
        ct, wt = np.ascontiguousarray(X.T), np.ascontiguousarray(W.T)
        out, ld, info = np.full((case["m"],) * 2, 7.0), ctypes.c_double(7.0), ctypes.c_int32(-5)
        rc = lib.mvc_plan_gram(plan._handle, ct.ctypes.data_as(vc._dp), lk.MODEL_IDS[case["model"]], *case["par"], wt.ctypes.data_as(vc._dp),
                               case["m"], ctypes.byref(ld), out.ctypes.data_as(vc._dp), ctypes.byref(info))
        record("%s %s: rc %d info %d (reference: station %d)" % (name, kind, rc, info.value, station))
        assert rc == vc.MVC_ENOTPD and info.value == station and b"not positive definite" in lib.mvc_last_error()
        assert ld.value == 7.0 and np.all(out == 7.0)  # never a partial result
        # the refusals that need a plan: non-finite input
        bad = ct.copy()
        bad[0, 0] = np.nan
        assert lib.mvc_plan_gram(plan._handle, bad.ctypes.data_as(vc._dp), 1, 1.0, 0.5, 0.1, wt.ctypes.data_as(vc._dp), case["m"], ctypes.byref(ld),
                                 out.ctypes.data_as(vc._dp), ctypes.byref(info)) == vc.MVC_EINVAL and b"coordinates must be finite" in lib.mvc_last_error()
        # a following good call on the same plan is within the bar: a nugget makes the pair harmless
        good = [1.0, 0.5, 0.1]
        logdet, G = plan.gram(X, case["model"], good, W)
        ref_logdet, ref_G = vcs.brute_force(X, order, nbr, case["model"], good, W)
        ev = np.linalg.eigvalsh(lc.covariance_ld(X, case["model"], good).astype(np.float64))
        bar = case["n"] * lc.U * float(ev[-1] / ev[0])
        el, eg = vcs.errors(logdet, G, ref_logdet, ref_G)
        assert ev[-1] / ev[0] <= lc.KAPPA_MAX and el <= bar and eg <= bar, (el, eg, bar)
    v = W[:, 0]
    full = [case["par"][0] + case["par"][2], case["par"][1], case["par"][2]]
    assert vc.neg_log_likelihood_vecchia(*X.T, v, case["model"], full, m=5, order=order) == math.inf


# ------------------------------------------------------------------------------------------------------------- the likelihood
def _problem(n, ndim, seed, nf=1):
    rng = np.random.default_rng(seed)
    raw = rng.random((n, ndim)) * ([3.0, 2.0, 1.0][:ndim])
    v = np.sin(2.0 * raw[:, 0])[:, None] + 0.5 * raw[:, 1][:, None] + 0.4 * rng.standard_normal((n, nf))
    return raw, v


def _reference_nll(raw, v, model, full, scaling, angle, drift, reml, m):
    """tests/test_likelihood.py's ``_reference_nll`` with the long-double pieces of Vecchia's covariance: the formulas of nll_from_gram
    on them, and the tolerance the device's pieces allow (derived there: G = D R D, every entry of R off by at most `bar`)."""
    n = len(raw)
    center = [(raw[:, c].max() + raw[:, c].min()) / 2.0 for c in range(raw.shape[1])]
    adj = core.adjust_for_anisotropy(raw, center, scaling, angle)
    par = [full[0] - full[2], full[1], full[2]]
    X = np.ones((n, 1)) if drift is None else np.hstack([np.ones((n, 1)), adj if isinstance(drift, str) else drift])
    F, p = v.shape[1], X.shape[1]
    order = vcs.order_of(n)
    logdet, G = vcs.brute_force(adj, order, vcs.neighbours_ref(adj, order, m), model, par, np.hstack([v, X]))
    ev = np.linalg.eigvalsh(lc.covariance_ld(adj, model, par).astype(np.float64))
    kappa = float(ev[-1] / ev[0])
    assert kappa <= lc.KAPPA_MAX
    bar = n * lc.U * kappa
    Xl = X.astype(LD)
    G64 = G.astype(np.float64)
    ldx = LD(np.linalg.slogdet((Xl.T @ Xl).astype(np.float64))[1])
    d = np.sqrt(np.diag(G64))
    R = G64 / d[:, None] / d[None, :]
    Rinv = np.linalg.inv(R[F:, F:])
    out, tol = np.zeros(F), np.zeros(F)
    lgx = LD(np.linalg.slogdet(G64[F:, F:])[1])
    for f in range(F):
        beta = np.linalg.solve(G64[F:, F:], G64[F:, f])
        q = G[f, f] - LD(G64[F:, f] @ beta)
        s = np.abs(Rinv @ R[F:, f]).sum()
        if reml:
            val = LD(0.5) * ((n - p) * LD(math.log(2 * math.pi)) - ldx + logdet + lgx + q)
            wobble = bar * (1.0 + float(G64[f, f]) * (1.0 + s) ** 2 + p + np.abs(Rinv).sum())
        else:
            val = LD(0.5) * (n * LD(math.log(2 * math.pi)) + logdet + q)
            wobble = bar * (1.0 + float(G64[f, f]) * (1.0 + s) ** 2)
        out[f], tol[f] = float(val), 0.5 * wobble + 16 * lc.U * abs(float(val))
    return out, tol, adj, bar


@pytest.mark.parametrize("ndim,drift", [(2, None), (2, "array"), (3, "regional_linear")])
def test_neg_log_likelihood_vecchia_is_the_formula_on_the_long_double_pieces(ndim, drift):
    raw, v = _problem(200, ndim, 11 + ndim, nf=3)
    full, m = [1.2, 0.9, 0.1], 12
    anis = dict(anisotropy_scaling=1.7, anisotropy_angle=25.0) if ndim == 2 else dict(
        anisotropy_scaling_y=1.4, anisotropy_scaling_z=0.6, anisotropy_angle_x=10.0, anisotropy_angle_y=-20.0, anisotropy_angle_z=35.0)
    sc, an = list(anis.values())[:ndim - 1], list(anis.values())[ndim - 1:]
    if drift == "array":
        drift = np.column_stack([raw[:, 0], raw[:, 0] * raw[:, 1]])
    for reml in (False, True):
        want, tol, adj, bar = _reference_nll(raw, v, "exponential", full, sc, an, drift, reml, m)
        got = vc.neg_log_likelihood_vecchia(*raw.T, v, "exponential", full, m=m, drift=drift, reml=reml, **anis)
        record("vecchia nll ndim %d reml %s: nll %s error %s tolerance %s" % (ndim, reml, got, np.abs(got - want), tol))
        assert got.shape == (3,) and np.all(np.abs(got - want) <= tol), (got, want, tol)
        with vc.VecchiaPlan(adj, m=m) as plan:
            on_plan = vc.neg_log_likelihood_vecchia(*raw.T, v, "exponential", full, plan=plan, drift=drift, reml=reml, **anis)
            assert np.array_equal(on_plan, got)
            for f in range(3):  # plane f of an (N, F) call is bit for bit the one-field call on the same plan
                one = vc.neg_log_likelihood_vecchia(*raw.T, v[:, f], "exponential", full, plan=plan, drift=drift, reml=reml, **anis)
                assert isinstance(one, float) and one == got[f]
    # every predecessor a neighbour (65 stations, m = 64): the exact likelihood, within twice the tolerance of the dense path's number
    small, vs = raw[:65], v[:65]
    ds = None if drift is None else (drift if isinstance(drift, str) else drift[:65])
    for reml in (False, True):
        exact = vc.neg_log_likelihood_vecchia(*small.T, vs, "exponential", full, m=64, drift=ds, reml=reml, **anis)
        dense = lk.neg_log_likelihood(*small.T, vs, "exponential", full, drift=ds, reml=reml, **anis)
        _, tol, _, _ = _reference_nll(small, vs, "exponential", full, sc, an, ds, reml, 64)
        record("vecchia nll ndim %d reml %s m >= N - 1: |vecchia - dense| %s, twice the tolerance %s" % (ndim, reml, np.abs(exact - dense), 2 * tol))
        assert np.all(np.abs(exact - dense) <= 2.0 * tol)


def test_the_methods_are_the_module_functions_on_the_objects_stations():
    raw, v = _problem(129, 3, 21)
    v = v[:, 0]
    x, y, z = raw.T
    kw = dict(variogram_model="gaussian", variogram_parameters=[1.0, 1.5, 0.2])
    a2, a3 = dict(anisotropy_scaling=2.0, anisotropy_angle=40.0), dict(anisotropy_scaling_y=1.5, anisotropy_scaling_z=0.5, anisotropy_angle_x=15.0)
    ok = pa.OrdinaryKriging(x, y, v, **kw, **a2)
    assert ok.neg_log_likelihood_vecchia(m=9) == vc.neg_log_likelihood_vecchia(x, y, v, "gaussian", [1.0, 1.5, 0.2], m=9, **a2)
    assert ok.neg_log_likelihood_vecchia([0.8, 1.0, 0.1], m=9, order="coordinate", reml=False, anisotropy_angle=10.0) == \
        vc.neg_log_likelihood_vecchia(x, y, v, "gaussian", [0.8, 1.0, 0.1], m=9, order="coordinate", reml=False, anisotropy_scaling=2.0,
                                      anisotropy_angle=10.0)
    ok3 = pa.OrdinaryKriging3D(x, y, z, v, **kw, **a3)
    assert ok3.neg_log_likelihood_vecchia(m=20) == vc.neg_log_likelihood_vecchia(x, y, z, v, "gaussian", [1.0, 1.5, 0.2], m=20, **a3)
    assert ok3.neg_log_likelihood_vecchia(m=20) != ok3.neg_log_likelihood_vecchia(m=5)
    fit = ok3.fit_variogram_vecchia(m=20)
    same = vc.fit_variogram_vecchia(x, y, z, v, "gaussian", m=20, start=[1.0, 1.5, 0.2], **a3)
    print(fit)
    assert fit.nll == same.nll and fit.variogram_parameters == same.variogram_parameters
    assert fit.nll <= ok3.neg_log_likelihood_vecchia(m=20) and set(fit.anisotropy) == set(lk._ANIS3) and fit.anisotropy["anisotropy_scaling_y"] == 1.5


def test_the_fit_is_never_worse_than_its_start_and_its_result_kriges():
    """400 stations of an exponential field simulated on the host (2 : 1 anisotropy at 30 degrees, fixed seed).  The fit returns finite
    parameters inside the bounds, its nll is no greater than the start's, and the moving window kriges with it.  No closeness to
    fit_variogram_ml's optimum is asserted: neither search is global."""
    rng = np.random.default_rng(2024)
    n = 400
    raw = rng.random((n, 2)) * [4.0, 3.0]
    center = [(raw[:, c].max() + raw[:, c].min()) / 2.0 for c in range(2)]
    adj = core.adjust_for_anisotropy(raw, center, [2.0], [30.0])
    Cm = lc.covariance_ld(adj, "exponential", [0.95, 1.2, 0.05]).astype(np.float64)
    v = 3.0 + np.linalg.cholesky(Cm) @ rng.standard_normal(n)
    x, y = raw.T
    start = [1.5, 0.6, 0.2]
    at_start = vc.neg_log_likelihood_vecchia(x, y, v, "exponential", start, m=20)
    fit = vc.fit_variogram_vecchia(x, y, v, "exponential", m=20, start=start, fit_anisotropy=True)
    record("fit_variogram_vecchia N 400 m 20: nll at the start %.6f, at the fit %.6f after %d evaluations: %r" % (at_start, fit.nll, fit.n_evaluations, fit))
    var, diag = float(np.var(v)), float(np.hypot(*(raw.max(axis=0) - raw.min(axis=0))))
    sill, rng_, nugget = fit.variogram_parameters
    assert all(math.isfinite(t) for t in fit.variogram_parameters + list(fit.anisotropy.values()))
    assert 1e-6 * var <= sill - nugget <= 100.0 * var and 1e-3 * diag <= rng_ <= 10.0 * diag and 0.0 <= nugget <= 100.0 * var
    assert 0.05 <= fit.anisotropy["anisotropy_scaling"] <= 20.0
    assert math.isfinite(fit.nll) and fit.nll <= at_start and fit.n_evaluations > 10
    ok = pa.OrdinaryKriging(x, y, v, variogram_model=fit.variogram_model, variogram_parameters=fit.variogram_parameters, **fit.anisotropy)
    zz, ss = ok.execute("grid", np.linspace(0.5, 3.5, 5), np.linspace(0.5, 2.5, 4), backend="loop", n_closest_points=10)
    assert zz.shape == (4, 5) and np.all(np.isfinite(zz)) and np.all(np.isfinite(ss))
    fit0 = vc.fit_variogram_vecchia(x, y, v, "exponential", m=20)  # the least-squares start of a subsample
    assert math.isfinite(fit0.nll) and fit0.success in (True, False)
