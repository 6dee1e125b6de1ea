"""Times directional_variogram_3d and variogram_map_3d (libmikvario3.so) and writes profiles/directional_variogram_3d_time.txt:

  seven directions (the three principal axes of a candidate rotation plus four more) x 32 lags with 1 and with 32 fields, and a
  17 x 17 x 13 variogram map, at 5000 and at 10^5 random 3-D stations; beside each the 2-D call (libmikvario.so) on the same x, y at the
  same N, number of directions and lags -- the yardstick, see profiles/directional_variogram_time.txt -- and, at N = 5000, the NumPy route
  through the N (N - 1) / 2 pair arrays.

Wall times of the Python calls (upload, kernels, copy back), median of `--repeat` runs after one warm-up; pairs/s = N (N - 1) / 2 over
the median, all fields in one call.  Run on the GPU:  python scripts/directional_variogram_3d_time.py"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANGLES, TOL, NLAGS = (20.0, 10.0, 30.0), 22.5, 32
MORE_AZ, MORE_DIP = (0.0, 90.0, 45.0, 135.0), (0.0, 0.0, 30.0, -30.0)
AZ2D = (0.0, 25.0, 50.0, 75.0, 100.0, 125.0, 150.0)  # the 2-D yardstick: as many directions
MAP3, MAP2 = (8, 8, 6), (8, 8)


def median_ms(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def numpy_directional(x, y, z, v, dirs, edges):
    """The route through the pair arrays, one field: what a user without the library writes."""
    from pykrige_amd import variography3d as v3

    tan2, _ = v3.decision_constants(TOL)
    i, j = np.triu_indices(x.size, 1)
    dx, dy, dz = x[j] - x[i], y[j] - y[i], z[j] - z[i]
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    g = 0.5 * (v[i] - v[j]) ** 2
    b = np.searchsorted(edges, d, side="right") - 1
    ok = (b >= 0) & (b < edges.size - 1)
    out = []
    for ux, uy, uz in dirs:
        along = dx * ux + dy * uy + dz * uz
        cx, cy, cz = dy * uz - dz * uy, dz * ux - dx * uz, dx * uy - dy * ux
        m = ok & (cx * cx + cy * cy + cz * cz <= (along * along) * tan2)
        out.append((np.bincount(b[m], minlength=edges.size - 1), np.bincount(b[m], weights=g[m], minlength=edges.size - 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--numpy-max", type=int, default=20000, help="largest N the NumPy route is timed at (N^2 / 2 pairs x ~100 bytes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "directional_variogram_3d_time.txt"))
    a = ap.parse_args()
    from pykrige_amd import core
    from pykrige_amd import variography as vg
    from pykrige_amd import variography3d as v3

    dirs = np.vstack([core.anisotropy_axes(ANGLES), v3.direction_vectors(MORE_AZ, MORE_DIP)])
    lines = ["directional_variogram_3d / variogram_map_3d beside the 2-D calls; wall ms of the Python call: median (min .. max) of %d runs "
             "after one warm-up; pairs/s over the median" % a.repeat,
             "directions: the axes of anisotropy_angle_x/_y/_z = %s and azimuth / dip %s; tolerance %.1f; %d lags"
             % (ANGLES, list(zip(MORE_AZ, MORE_DIP)), TOL, NLAGS)]
    fmt = "  %-66s %10.3f ms (%.3f .. %.3f)  %9.3e pairs/s"
    for n in (a.n, a.big):
        rs = np.random.default_rng(n)
        x, y, z = rs.random(n), rs.random(n), 0.5 * rs.random(n)
        v1 = np.sin(7 * x) + y + 2.0 * z
        v32 = v1[:, None] + 0.1 * np.random.default_rng(n + 1).standard_normal((n, 32))
        pairs = n * (n - 1) / 2.0
        maxlag = 0.5 * float(np.sqrt(np.ptp(x) ** 2 + np.ptp(y) ** 2 + np.ptp(z) ** 2))
        edges = np.linspace(0.0, maxlag, NLAGS + 1)
        cx, cy, cz = maxlag / (MAP3[0] + 0.5), maxlag / (MAP3[1] + 0.5), 0.5 * maxlag / (MAP3[2] + 0.5)
        lines.append("")
        lines.append("N = %d random stations in a 1 x 1 x 0.5 box: %.4g pairs" % (n, pairs))
        rep = a.repeat if n <= 20000 else max(2, a.repeat // 2)
        cases = (
            ("3-D directional, 7 directions x 32 lags, 1 field", lambda: v3.directional_variogram_3d(x, y, z, v1, directions=dirs, tolerance=TOL, edges=edges)),
            ("2-D directional, 7 azimuths x 32 lags, 1 field (x, y only)", lambda: vg.directional_variogram(x, y, v1, AZ2D, TOL, edges=edges)),
            ("3-D directional, 7 directions x 32 lags, 32 fields", lambda: v3.directional_variogram_3d(x, y, z, v32, directions=dirs, tolerance=TOL, edges=edges)),
            ("2-D directional, 7 azimuths x 32 lags, 32 fields (x, y only)", lambda: vg.directional_variogram(x, y, v32, AZ2D, TOL, edges=edges)),
            ("3-D variogram map 17 x 17 x 13, 1 field", lambda: v3.variogram_map_3d(x, y, z, v1, *MAP3, cx, cy, cz)),
            ("2-D variogram map 17 x 17, 1 field (x, y only)", lambda: vg.variogram_map(x, y, v1, *MAP2, cx, cy)),
            ("3-D variogram map 17 x 17 x 13, 32 fields", lambda: v3.variogram_map_3d(x, y, z, v32, *MAP3, cx, cy, cz)),
            ("2-D variogram map 17 x 17, 32 fields (x, y only)", lambda: vg.variogram_map(x, y, v32, *MAP2, cx, cy)),
        )
        for name, fn in cases:
            t = median_ms(fn, rep)
            lines.append(fmt % ((name,) + t + (pairs / (t[0] * 1e-3),)))
        if n <= a.numpy_max:
            t = median_ms(lambda: numpy_directional(x, y, z, v1, dirs, edges), 1 if n > 10000 else 3)
            lines.append(fmt % (("NumPy, 7 directions x 32 lags, 1 field (host)",) + t + (pairs / (t[0] * 1e-3),)))
        else:
            lines.append("  NumPy route: not timed (its pair arrays do not fit: %.0f GB for the pair list alone)" % (pairs * 8 * 7 / 1e9))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
