"""Times cross_validate(folds=...) at BASELINE config 2's stations (N = 5000, exponential model) and writes
profiles/cross_validate_folds_time.txt:

  folds=5, folds=10 and the spatial blocks of a 15 x 15 cell grid (about 200 groups), each beside what it replaces: one mik_factor, the
  leave-one-out call, and K objects of N - m stations each with execute('points') at the held-out stations (a factorisation per fold).

Wall times of the Python calls, median of `--repeat` runs after one warm-up (the K-object loops: one run).
Run on the GPU:  python scripts/cross_validate_folds_time.py"""
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
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_validate_folds_time.txt"))
    a = ap.parse_args()
    import bench
    import pykrige_amd as pa

    cfg = bench.CONFIGS[2]
    n = a.n
    (x, y), v = bench.synth(cfg["seed"], n, 2)
    kw = dict(variogram_model=cfg["model"], variogram_parameters=cfg["params"])
    m = pa.OrdinaryKriging(x, y, v, **kw)
    lines = ["cross_validate(folds=...) at the stations of bench.py config 2 (%s), N = %d; wall ms of the Python call: median (min .. max) of %d runs"
             % (cfg["name"], n, a.repeat)]
    h = m._get_handle()
    m._upload_and_factor()

    def factor():
        m._set_problem(h)
        h.factor()

    t_factor = median_ms(factor, a.repeat)
    lines.append("mik_set_problem + mik_factor                          %10.2f ms (%.2f .. %.2f)" % t_factor)
    m._factor_key = None
    m.cross_validate()
    t_loo = median_ms(lambda: m.cross_validate(), a.repeat)
    lines.append("leave-one-out cross_validate (factor resident)        %10.2f ms (%.2f .. %.2f)" % t_loo)

    def cell(q):
        return np.minimum(((q - q.min()) / (q.max() - q.min()) * 15).astype(np.int64), 14)

    blocks = cell(x) * 15 + cell(y)
    for what, folds in (("folds=5", 5), ("folds=10", 10), ("%d blocks of a 15 x 15 grid" % np.unique(blocks).size, blocks)):
        lab, k = m._fold_labels(folds)
        sizes = np.bincount(lab)
        t = median_ms(lambda: m.cross_validate(folds=folds), a.repeat)
        z, ss = m.cross_validate(folds=folds)
        lines.append("%-32s (factor resident)     %10.2f ms (%.2f .. %.2f)   = %.2f x mik_factor, %.1f x leave-one-out; folds of %d .. %d stations"
                     % (what, t[0], t[1], t[2], t[0] / t_factor[0], t[0] / t_loo[0], sizes.min(), sizes.max()))
        t0 = time.perf_counter()
        zk, sk = np.empty(n), np.empty(n)
        for f in range(k):  # what it replaces: an object, a factorisation and an execute per fold
            s = lab == f
            o = pa.OrdinaryKriging(x[~s], y[~s], v[~s], **kw)
            zz, sz = o.execute("points", x[s], y[s])
            zk[s], sk[s] = np.ma.getdata(zz), np.ma.getdata(sz)
        tk = (time.perf_counter() - t0) * 1e3
        lines.append("  %d objects of N - m stations, execute('points') each  %10.2f ms   = %.1f x the fold call;  max |dz| %.3g  max |dss| %.3g; "
                     "rms residual %.4g, mean sigma^2 %.4g" % (k, tk, tk / t[0], float(np.abs(z - zk).max()), float(np.abs(ss - sk).max()),
                                                             float(np.sqrt(np.mean((v - z) ** 2))), float(ss.mean())))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
