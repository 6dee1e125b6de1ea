"""Times cross_validate_window at BASELINE config 2's stations (N = 5000, exponential model) and writes
profiles/cross_validate_window_time.txt:

  for k = 10, 50 and 100: cross_validate_window(k) beside execute('points', <the stations' own coordinates>, n_closest_points=k) on the
  same object (the same N local solves, the points in the caller's order instead of the search grid's) and beside the global
  cross_validate() (factor resident, and with the factorisation);
  10^6 random stations at k = 10 at handle level, which the global form cannot do (no 10^6 x 10^6 inverse).

Wall times of the Python calls, median of `--repeat` runs after one warm-up; the kernel split is mik_timing's of the last run.
Run on the GPU:  python scripts/cross_validate_window_time.py"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--big", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_validate_window_time.txt"))
    a = ap.parse_args()
    import bench
    import pykrige_amd as pa
    from pykrige_amd import _lib

    cfg = bench.CONFIGS[2]
    n = a.n
    (x, y), v = bench.synth(cfg["seed"], n, 2)
    m = pa.OrdinaryKriging(x, y, v, variogram_model=cfg["model"], variogram_parameters=cfg["params"])
    lines = ["cross_validate_window at the stations of bench.py config 2 (%s), N = %d; wall ms of the Python call: median (min .. max) of %d runs"
             % (cfg["name"], n, a.repeat)]
    fmt = "%-66s %9.3f ms (%.3f .. %.3f)"
    for k in (10, 50, 100):
        tw = median_ms(lambda: m.cross_validate_window(k), a.repeat)
        t = m.last_timing
        lines.append(fmt % (("k = %3d  cross_validate_window" % k,) + tw))
        lines.append("         device: whole pass %.3f ms = search + right-hand sides %.3f + solves %.3f (mw_kernel %d)" % (
            t["predict_ms"], t["rhs_ms"], t["contract_ms"], t["mw_kernel"]))
        te = median_ms(lambda: m.execute("points", x, y, n_closest_points=k, backend="loop"), a.repeat)
        t = m.last_timing
        lines.append(fmt % (("k = %3d  execute('points', stations, n_closest_points=k)" % k,) + te))
        lines.append("         device: whole pass %.3f ms = search + right-hand sides %.3f + solves %.3f (points sorted: %d)" % (
            t["predict_ms"], t["rhs_ms"], t["contract_ms"], t["points_sorted"]))
        lines.append("         cross_validate_window / execute = %.3f" % (tw[0] / te[0]))
    m.cross_validate()
    lines.append(fmt % (("global cross_validate() (factor resident)",) + median_ms(lambda: m.cross_validate(), a.repeat)))

    def cold():
        m._factor_key = None
        m.cross_validate()

    lines.append(fmt % (("global cross_validate() with mik_set_problem + mik_factor",) + median_ms(cold, a.repeat)))
    zg, _ = m.cross_validate()
    for k in (10, 50, 100):
        zw, _ = m.cross_validate_window(k)
        lines.append("residual rms: window k = %3d %.5g, global %.5g" % (k, float(np.sqrt(np.mean((v - zw) ** 2))), float(np.sqrt(np.mean((v - zg) ** 2)))))
    # many stations: only coordinates live on the device (no N x N matrix on this path)
    nb, k = a.big, 10
    rs = np.random.default_rng(nb + k)
    sx, sy = rs.random(nb), rs.random(nb)
    h = _lib.Handle()
    h.set_problem(ndim=2, xs=sx, ys=sy, zs=None, values=np.sin(7 * sx) + sy, model_id=_lib.MODEL_IDS["exponential"],
                  params=bench.internal_params("exponential", [1.0, 0.02, 0.0]))
    tb = median_ms(lambda: h.cross_validate_window(k), a.repeat)
    t = h.timing()
    lines.append("")
    lines.append("%d random stations in the unit square (exponential, range 0.02), handle level:" % nb)
    lines.append(fmt % (("k = %3d  Handle.cross_validate_window (with the copy back of 2 N doubles)" % k,) + tb))
    lines.append("         device: whole pass %.3f ms = search + right-hand sides %.3f + solves %.3f (mw_kernel %d)" % (
        t["predict_ms"], t["rhs_ms"], t["contract_ms"], t["mw_kernel"]))
    h.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
