"""Times directional_variogram and variogram_map (libmikvario.so) and writes profiles/directional_variogram_time.txt:

  four azimuths x 32 lags with 1 and with 32 fields, and a 65 x 65 variogram map, at BASELINE config 2's stations (N = 5000) and at
  10^5 random stations; beside each the NumPy route through the N x N distance matrix where that fits in memory, and the constructor's
  omnidirectional semivariogram (mik_experimental_variogram, one field, 32 lags) at the same N.

Wall times of the Python calls (upload, kernels, copy back), median of `--repeat` runs after one warm-up; pairs/s = N (N - 1) / 2 over
the median, all fields in one call.  Run on the GPU:  python scripts/directional_variogram_time.py"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AZIMUTHS, TOL, NLAGS = (0.0, 45.0, 90.0, 135.0), 22.5, 32


def median_ms(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def numpy_directional(x, y, v, edges):
    """The route through the N x N matrices, one field: what a user without the library writes."""
    from pykrige_amd import variography as vg

    cs, sn, tant = vg.direction_constants(AZIMUTHS, TOL)
    i, j = np.triu_indices(x.size, 1)
    dx, dy = x[j] - x[i], y[j] - y[i]
    d = np.sqrt(dx * dx + dy * dy)
    g = 0.5 * (v[i] - v[j]) ** 2
    b = np.searchsorted(edges, d, side="right") - 1
    ok = (b >= 0) & (b < edges.size - 1)
    out = []
    for a in range(len(cs)):
        m = ok & (np.abs(-dx * sn[a] + dy * cs[a]) <= np.abs(dx * cs[a] + dy * sn[a]) * tant)
        out.append((np.bincount(b[m], minlength=edges.size - 1), np.bincount(b[m], weights=g[m], minlength=edges.size - 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--numpy-max", type=int, default=20000, help="largest N the NumPy route is timed at (N^2 / 2 pairs x ~60 bytes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "directional_variogram_time.txt"))
    a = ap.parse_args()
    import bench
    from pykrige_amd import _lib
    from pykrige_amd import variography as vg

    cfg = bench.CONFIGS[2]
    lines = ["directional_variogram / variogram_map; wall ms of the Python call: median (min .. max) of %d runs after one warm-up; "
             "pairs/s over the median" % a.repeat]
    fmt = "  %-62s %10.3f ms (%.3f .. %.3f)  %9.3e pairs/s"
    for label, n in (("stations of bench.py config 2 (%s)" % cfg["name"], a.n), ("random stations in the unit square", a.big)):
        if label.startswith("stations"):
            (x, y), v1 = bench.synth(cfg["seed"], n, 2)
        else:
            rs = np.random.default_rng(n)
            x, y = rs.random(n), rs.random(n)
            v1 = np.sin(7 * x) + y
        rs = np.random.default_rng(n + 1)
        v32 = v1[:, None] + 0.1 * rs.standard_normal((n, 32))
        pairs = n * (n - 1) / 2.0
        maxlag = 0.5 * float(np.hypot(x.max() - x.min(), y.max() - y.min()))
        edges = np.linspace(0.0, maxlag, NLAGS + 1)
        cell = maxlag / 32.5
        lines.append("")
        lines.append("N = %d, %s: %.4g pairs" % (n, label, pairs))
        rep = a.repeat if n <= 20000 else max(2, a.repeat // 2)
        for name, fn in (("directional, 4 azimuths x 32 lags, 1 field", lambda: vg.directional_variogram(x, y, v1, AZIMUTHS, TOL, edges=edges)),
                         ("directional, 4 azimuths x 32 lags, 32 fields", lambda: vg.directional_variogram(x, y, v32, AZIMUTHS, TOL, edges=edges)),
                         ("variogram map 65 x 65, 1 field", lambda: vg.variogram_map(x, y, v1, 32, 32, cell, cell)),
                         ("variogram map 65 x 65, 32 fields", lambda: vg.variogram_map(x, y, v32, 32, 32, cell, cell))):
            t = median_ms(fn, rep)
            lines.append(fmt % ((name,) + t + (pairs / (t[0] * 1e-3),)))
        h = _lib.Handle()
        h.set_problem(ndim=2, xs=x, ys=y, zs=None, values=v1, model_id=0, params=[1.0, 0.0])
        t = median_ms(lambda: h.experimental_variogram(NLAGS), rep)
        lines.append(fmt % (("mik_experimental_variogram (omnidirectional, 32 lags, 1 field)",) + t + (pairs / (t[0] * 1e-3),)))
        h.close()
        if n <= a.numpy_max:
            t = median_ms(lambda: numpy_directional(x, y, v1, edges), 1 if n > 10000 else 3)
            lines.append(fmt % (("NumPy, 4 azimuths x 32 lags, 1 field (host)",) + t + (pairs / (t[0] * 1e-3),)))
        else:
            lines.append("  NumPy route: not timed (its N x N arrays do not fit: %.0f GB for the pair list alone)" % (pairs * 8 * 6 / 1e9))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
