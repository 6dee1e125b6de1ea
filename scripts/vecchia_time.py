"""Times vecchia.VecchiaPlan (the neighbour search) and one VecchiaPlan.gram (libmikvecchia.so) and writes profiles/vecchia_time.txt:

  the plan build and one gram with m = 10, 30 and 60 neighbours at bench.py config 2's 5000 stations, beside one dense likelihood.gram and
  |nll_vecchia - nll_dense| there (information only), and the same plan build and gram at 1e5 and 1e6 random stations in the unit square.

Every size is a child process under its own `timeout`; the first one that fails ends the run.
Run on the GPU:  python scripts/vecchia_time.py"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL, FULL = "exponential", [1.0, 0.3, 0.05]  # config 2's variogram with a nugget of 5 % of the sill
PAR = [FULL[0] - FULL[2], FULL[1], FULL[2]]
MS = (10, 30, 60)


def stations(n, config2):
    if config2:
        import bench

        (x, y), v = bench.synth(bench.CONFIGS[2]["seed"], n, 2)
    else:
        rs = np.random.default_rng(n)
        x, y = rs.random(n), rs.random(n)
        v = np.sin(7 * x) + y + 0.1 * rs.standard_normal(n)
    return np.column_stack([x, y]), v


def times_ms(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def child(n, config2, repeat):
    from pykrige_amd import likelihood as lk
    from pykrige_amd import vecchia as vc

    X, v = stations(n, config2)
    W = np.column_stack([v, np.ones(n)])
    pieces = lk._pieces(np.ones((n, 1)))
    print("\nN = %d, %s" % (n, "stations of bench.py config 2" if config2 else "random stations in the unit square"))
    dense = None
    if config2:
        logdet, G = lk.gram(X, MODEL, PAR, W)
        dense = float(lk.nll_from_gram(n, logdet, G, 1, True, pieces)[0])
        print("  dense likelihood.gram, 2 columns        %10.3f ms (%.3f .. %.3f)   REML nll %.6f" % (times_ms(lambda: lk.gram(X, MODEL, PAR, W), repeat) + (dense,)))
    with vc.VecchiaPlan(X, m=1):  # the first plan of the process loads the code objects
        pass
    for m in MS:
        t0 = time.perf_counter()
        plan = vc.VecchiaPlan(X, m=m)
        build = (time.perf_counter() - t0) * 1e3
        with plan:
            logdet, G = plan.gram(X, MODEL, PAR, W)
            nll = float(lk.nll_from_gram(n, logdet, G, 1, True, pieces)[0])
            line = "  m = %2d   plan (order, upload, k_vec_knn) %10.3f ms   gram, 2 columns %10.3f ms (%.3f .. %.3f)   REML nll %.6f" % (
                (m, build) + times_ms(lambda: plan.gram(X, MODEL, PAR, W), repeat) + (nll,))
        if dense is not None:
            line += "   |nll_vecchia - nll_dense| %.3e" % abs(nll - dense)
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--config2", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[100000, 1000000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecchia_time.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config2, a.repeat)
        return
    text = ["vecchia.VecchiaPlan and VecchiaPlan.gram (one mvc_plan_gram: upload of coordinates and W, k_vec_solve, k_vec_reduce, copy back); wall ms "
            "of the Python call: one plan build, gram median (min .. max) after one warm-up",
            "model %s, variogram_parameters %r, order 'random', seed 0" % (MODEL, FULL)]
    for n, config2, limit in [(5000, True, 240)] + [(n, False, 600) for n in a.sizes]:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(n), "--repeat", str(a.repeat)]
        r = subprocess.run(cmd + (["--config2"] if config2 else []), capture_output=True, text=True, cwd=ROOT)
        text.append(r.stdout.rstrip("\n"))
        if r.returncode != 0:
            text.append("N = %d: the child ended with status %d\n%s" % (n, r.returncode, r.stderr[-2000:]))
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    sys.exit(0 if r.returncode == 0 else 1)


if __name__ == "__main__":
    main()
