"""Cases and references of the block-kriging-through-the-moving-window tests (tests/test_execute_block_window.py on the GPU,
tests/test_execute_block_window_host.py on the CPU).

A case is a station set of tests/_cvw_cases.py (or the linear-variogram set built here), a window k, block centres, a block size and
n_disc.  The reference is brute force in extended precision, block by block:

    ek.neighbours(st, centre, k)                       the window: the k stations nearest to the adjusted CENTRE
    bbar = mean over the adjusted nodes of -ek.variogram_ld(node - station distances), 0 where exact_values and the float64 distance
           is <= ko.EPS (decided node by node)
    the local (k + 1) x (k + 1) matrix cut out of ONE ek.assemble of all stations, ek.refined_solve
    z = lam . Z_sel,  sigma^2 = -lam . bbar - mu - gbar,  gbar as tests/test_execute_block_host.reference forms it

Bars: ek.bars(ref, ec.C_BAR) with cond_1 and order = k + 1 of the LOCAL system, vscale the window's max|v| and bscale the largest |b| over
the block's nodes -- the moving-window kernels' bar, with the right-hand-side scale of the block tests.

Centres come from a seeded generator inside the station extent (the caller's coordinates); the first three are stations, so with odd
n_disc the centre node hits exact_values.  A seed is accepted only if for every centre the k-th and (k + 1)-th nearest stations differ by
more than _cvw_cases.TIE_GAP (relative), for every window the centres are used with; else the next seed is drawn.  No block is skipped in
any comparison."""
import functools

import numpy as np

from oracle import exact_kriging as ek
from oracle import kriging_oracle as ko
from pykrige_amd import core
from tests import _cv_cases as cv
from tests import _cvw_cases as cw
from tests import _error_cases as ec
from tests import test_execute_cov_host as ch
from tests.test_fields_gaps_host import adjusted

LINEAR = "ok2d_linear_n100"  # the one station set of this file: the SPD shift of the LDL^T solvers comes from max(-bbar)
ON_STATION = (0, 1, 2)       # the centres that sit on a station

# case -> (station set, k, the solver that has to run (mik_timing.mw_kernel; None: not asserted), centres, n_disc, what it covers)
CASES = {
    "exponential_n300_k10_3x3": ("ok2d_exponential_n300", 10, 1, 130, (3, 3)),            # exact hits at the three station-centred blocks
    "spherical_n300_k16_2x3": ("ok2d_spherical_n300", 16, None, 40, (2, 3)),              # the last window of the lane search
    "spherical_n300_k17_2x3": ("ok2d_spherical_n300", 17, None, 40, (2, 3)),              # the first wave-only window
    "gaussian_n450_k100_2x2": ("ok2d_gaussian_n450_values_1e3", 100, 1, 40, (2, 2)),      # class {8, 13}
    "ok3d_aniso_n400_k24_2x2x2": ("ok3d_exponential_aniso_n400", 24, None, 40, (2, 2, 2)),  # 3-D
    "ok3d_aniso_n400_k24_8x8x8": ("ok3d_exponential_aniso_n400", 24, None, 9, (8, 8, 8)),   # 512 nodes: the LDS table full
    "hole_effect_n200_k20_2x2": ("hole_effect_n200", 20, 2, 20, (2, 2)),                  # pivoting Gauss-Jordan
    "hole_effect_n200_k130_2x2": ("hole_effect_n200", 130, 3, 20, (2, 2)),                # k_mw_solve_big
    "exponential_n300_k257_2x2": ("ok2d_exponential_n300", 257, 4, 20, (2, 2)),           # blocked Cholesky
    "linear_n100_k10_3x3": (LINEAR, 10, 1, 40, (3, 3)),                                   # data-dependent shift from bbar
}
INEXACT = "exponential_n300_k10_3x3"  # repeated with exact_values=False on a rebuilt object
K_IS_N = ("ok2d_exponential_n12", 12, 20, (3, 3))  # every station in the window: the global block kriging


# ------------------------------------------------------------------------------------------------------------- station sets, centres
@functools.lru_cache(maxsize=None)
def station_set(name):
    """(object, state): tests/_cvw_cases.station_set, and the linear-variogram set of 100 stations."""
    if name != LINEAR:
        return cw.station_set(name)
    obj = cw._ok2d("linear", ec.USER["linear"], 100)(np.random.default_rng(2201))
    return obj, cv.state_of(obj)


@functools.lru_cache(maxsize=None)
def inexact_twin(name):
    """The 2-D station set `name` rebuilt with exact_values=False: (object, state)."""
    import pykrige_amd as pa

    obj, st = station_set(name)
    twin = pa.OrdinaryKriging(obj.X_ORIG, obj.Y_ORIG, obj.Z, variogram_model=obj.variogram_model,
                              variogram_parameters=ec.USER[obj.variogram_model], exact_values=False)
    st2 = cv.state_of(twin)
    assert np.array_equal(st2.coords_adj, st.coords_adj) and st2.params == st.params and not st2.exact_values
    return twin, st2


def block_size(st):
    """About a twentieth of the station extent, unequal per axis (the caller's coordinates)."""
    ext = st.coords_orig.max(axis=0) - st.coords_orig.min(axis=0)
    return tuple(float(v) for v in ext / 20.0 * np.array([1.0, 0.8, 1.25])[:st.ndim])


def tie_free(st, ctr_adj, ks):
    for k in ks:
        if k + 1 > st.n:  # k = N: every station is in the window
            continue
        bd, _ = ek.neighbours(st, ctr_adj, k + 1)
        if not np.all(bd[:, k] - bd[:, k - 1] > cw.TIE_GAP * bd[:, k]):
            return False
    return True


@functools.lru_cache(maxsize=None)
def centres(sname, n, ks, seed=3301):
    """(n, ndim) block centres in the caller's coordinates: inside the station extent, the first three on stations, tie-free at every
    window of ks."""
    _, st = station_set(sname)
    lo, hi = st.coords_orig.min(axis=0), st.coords_orig.max(axis=0)
    for s in range(seed, seed + 20):
        c = lo + (hi - lo) * np.random.default_rng(s).random((n, st.ndim))
        c[0], c[1], c[2] = st.coords_orig[7], st.coords_orig[st.n // 2], st.coords_orig[st.n - 1]
        if tie_free(st, adjusted(st, c), ks):
            return c
    raise AssertionError("no tie-free centres within 20 seeds of %d" % seed)


def case(name):
    """(object, state, k, mw_kernel, centres (raw), block_size, n_disc)"""
    sname, k, kernel, n, n_disc = CASES[name]
    obj, st = station_set(sname)
    ks = tuple(sorted({c[1] for c in CASES.values() if c[0] == sname and c[3] == n}))  # the centres of a set are shared by its windows
    return obj, st, k, kernel, centres(sname, n, ks), block_size(st), n_disc


# ------------------------------------------------------------------------------------------------------------- references
def gbar_ld(st, bsize, n_disc):
    """gbar in longdouble from the float64 distances of the adjusted offsets (0 where d <= ko.EPS): tests/test_execute_block_host.reference."""
    off = core.adjust_offsets(core.block_node_offsets(st.ndim, bsize, n_disc), st.ndim, st.scaling, st.angle)
    d = ch.point_pair_distances(st, off)
    gam = ek.variogram_ld(st.model, st.params, d)
    gam[d <= ko.EPS] = 0
    nd = off.shape[0]
    return gam.sum() / (ek.LD(nd) * ek.LD(nd))


def node_distances(st, ctr_raw, bsize, n_disc):
    """(npt, nd, n) float64 distances between the adjusted nodes of every block and all stations."""
    off = core.block_node_offsets(st.ndim, bsize, n_disc)
    nodes = np.asarray(ctr_raw)[:, None, :] + off[None, :, :]
    na = adjusted(st, nodes.reshape(-1, st.ndim))
    return ek.point_distances(st, na).reshape(nodes.shape[0], off.shape[0], st.n)


def window_reference(st, k, ctr_raw, bsize, n_disc):
    """ek.ExactResult of the blocks, each kriged from the k stations nearest to its centre."""
    npt = len(ctr_raw)
    a_all = ek.assemble(st, ek.station_distances(st))  # (n + 1) x (n + 1) long double, once
    _, idx_all = ek.neighbours(st, adjusted(st, ctr_raw), k)
    dn = node_distances(st, ctr_raw, bsize, n_disc)
    nd = dn.shape[1]
    gbar = gbar_ld(st, bsize, n_disc)
    out = ek.ExactResult(z=np.zeros(npt, dtype=ek.LD), ss=np.zeros(npt, dtype=ek.LD), cond=np.zeros(npt), order=np.full(npt, k + 1),
                         vscale=np.zeros(npt), bscale=np.zeros(npt))
    for i in range(npt):
        idx = idx_all[i]
        sel = np.concatenate((idx, [st.n]))
        a = a_all[sel[:, None], sel]
        d = dn[i][:, idx]  # (nd, k)
        g = -ek.variogram_ld(st.model, st.params, d)
        if st.exact_values:
            g[np.absolute(d) <= ko.EPS] = 0
        b = np.zeros(k + 1, dtype=ek.LD)
        b[:k] = g.sum(axis=0) / ek.LD(nd)
        b[k] = 1
        x, cond = ek.refined_solve(a, b[:, None].copy())
        v = st.values[idx]
        z, ss = ek._reduce(st, x[:, 0], b, v)
        out.z[i], out.ss[i] = z, ss - gbar
        out.cond[i], out.vscale[i], out.bscale[i] = cond, float(np.abs(v).max()), float(np.abs(g).max())
    return out


@functools.lru_cache(maxsize=None)
def reference(name, exact=True):
    """The brute-force reference of a case, computed once per session and shared (exact=False: on the exact_values=False twin)."""
    _, st, k, _, ctr, bsize, n_disc = case(name)
    if not exact:
        _, st = inexact_twin(CASES[name][0])
    return window_reference(st, k, ctr, bsize, n_disc)


def global_reference(st, ctr_raw, bsize, n_disc):
    """The blocks kriged from ALL stations by the one global system: tests/test_execute_block_host.reference's form."""
    npt = len(ctr_raw)
    off = core.block_node_offsets(st.ndim, bsize, n_disc)
    nd = off.shape[0]
    nodes = np.asarray(ctr_raw)[:, None, :] + off[None, :, :]
    na = adjusted(st, nodes.reshape(-1, st.ndim))
    a = ek.assemble(st, ek.station_distances(st))
    b = ek.right_hand_sides(st, na, ek.point_distances(st, na)).reshape(npt, nd, a.shape[0])
    bbar = b.sum(axis=1) / ek.LD(nd)
    x, cond = ek.refined_solve(a, bbar.T.copy())
    z = x.T[:, :st.n] @ st.values.astype(ek.LD)
    ss = -gbar_ld(st, bsize, n_disc) - np.einsum("pi,pi->p", x.T, bbar)
    bscale = np.abs(b[:, :, :st.n]).max(axis=(1, 2)).astype(np.float64)
    return ek.ExactResult(z=z, ss=ss, cond=np.full(npt, cond), order=np.full(npt, a.shape[0]),
                          vscale=np.full(npt, float(np.abs(st.values).max())), bscale=bscale)


@functools.lru_cache(maxsize=None)
def k_is_n():
    """(object, state, k, centres, block_size, n_disc, global reference) of the k = N case."""
    sname, k, n, n_disc = K_IS_N
    obj, st = station_set(sname)
    assert k == st.n
    ctr = centres(sname, n, (k,))
    return obj, st, k, ctr, block_size(st), n_disc, global_reference(st, ctr, block_size(st), n_disc)


def worst_ratios(ref, z, ss):
    """max |z - ref| / bar and max |sigma^2 - ref| / bar over all blocks of ref."""
    return cv.ratios(ref, z, ss, ec.C_BAR)


# ------------------------------------------------------------------------------------------------------------- the stages in float64
def restatement(st, k, ctr_raw, bsize, n_disc):
    """The device's stages in float64 NumPy: the window chosen by the centre, bbar summed in node order and divided once, an LU solve of
    the local system, -lam . bbar - mu - gbar."""
    npt = len(ctr_raw)
    a_all = ko.kriging_matrix(st)
    _, idx_all = ek.neighbours(st, adjusted(st, ctr_raw), k)
    dn = node_distances(st, ctr_raw, bsize, n_disc)
    nd = dn.shape[1]
    off = core.adjust_offsets(core.block_node_offsets(st.ndim, bsize, n_disc), st.ndim, st.scaling, st.angle)
    dp = ch.point_pair_distances(st, off)
    gbar = np.where(dp <= ko.EPS, 0.0, ko.variogram(st.model, st.params, dp)).sum() / float(nd * nd)
    z, ss = np.zeros(npt), np.zeros(npt)
    for i in range(npt):
        idx = idx_all[i]
        sel = np.concatenate((idx, [st.n]))
        d = dn[i][:, idx]
        g = -ko.variogram(st.model, st.params, d)
        if st.exact_values:
            g[np.absolute(d) <= ko.EPS] = 0.0
        b = np.ones(k + 1)
        acc = g[0].copy()
        for u in range(1, nd):
            acc += g[u]
        b[:k] = acc / nd
        x = np.linalg.solve(a_all[sel[:, None], sel], b)
        z[i] = x[:k] @ st.values[idx]
        ss[i] = -(x @ b) - gbar
    return z, ss
