"""Times block kriging at BASELINE config 2 (OK2D, N = 5000, exponential, the 1000 x 1000 grid on the unit square) and writes
profiles/execute_block_time.txt.  Beside each other:

  1. execute('grid'): the point predict of the grid nodes;
  2. execute_block('grid', block_size = the grid spacing) with n_disc = 1, 4 x 4 and 8 x 8: every grid cell as a block.

Per call: the wall time of the Python call (best and worst of --repeats after one warm-up) and, from last_timing, the event-timed
rhs_ms (the right-hand sides: nd variogram values per station and block), contract_ms (the contraction: one per block whatever nd is)
and predict_ms, with the path the call took ("sparse").  What to read off: contract_ms of execute_block against that of execute on the
same points, and how rhs_ms grows with nd.

    python scripts/execute_block_time.py [--repeats 3] [--grid 1000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pykrige_amd as pa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--n-disc", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "execute_block_time.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)  # config 2's stations (bench.py: synth(2, 5000, 2))
    n = a.n
    x, y = rng.random(n), rng.random(n)
    v = np.sin(6 * x) * np.cos(4 * y) + 0.1 * rng.standard_normal(n)
    ok = pa.OrdinaryKriging(x, y, v, variogram_model="exponential", variogram_parameters=[1.0, 0.3, 0.0])
    gx = gy = np.linspace(0.0, 1.0, a.grid)
    cell = float(gx[1] - gx[0])

    def best(fn):
        fn()
        ts, tms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
            tms.append(dict(ok.last_timing))
        k = int(np.argmin(ts))
        return min(ts) * 1e3, max(ts) * 1e3, tms[k], tms, out

    def line(label, r):
        tm = r[2]
        return ("  %-34s %10.2f ms (%.2f)   device: rhs %9.2f  contract %8.2f  predict %9.2f ms   contract of every run: %s   sparse %d  launches %d"
                % (label, r[0], r[1], tm["rhs_ms"], tm["contract_ms"], tm["predict_ms"], " ".join("%.2f" % t["contract_ms"] for t in r[3]),
                   tm["sparse"], tm["contract_launches"]))

    lines = ["block kriging at config 2 (OK2D exponential, N = %d, %d x %d grid, block = one grid cell of %.6f); wall ms of the Python call: "
             "best (worst) of %d runs after a warm-up" % (n, a.grid, a.grid, cell, a.repeats), ""]
    r0 = best(lambda: ok.execute("grid", gx, gy))
    lines.append(line("execute('grid')", r0))
    z0, s0 = [np.asarray(q) for q in r0[4]]
    for nd in a.n_disc:
        r = best(lambda: ok.execute_block("grid", gx, gy, cell, n_disc=nd))
        lines.append(line("execute_block n_disc = %d x %d" % (nd, nd), r))
        z, s = [np.asarray(q) for q in r[4]]
        lines.append("      rhs_ms / execute's %.2f   contract_ms / execute's %.3f   mean sigma^2 %.6g (execute: %.6g)   max |z - execute's z| %.3g"
                     % (r[2]["rhs_ms"] / r0[2]["rhs_ms"], r[2]["contract_ms"] / r0[2]["contract_ms"], float(s.mean()), float(s0.mean()),
                        float(np.abs(z - z0).max())))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
