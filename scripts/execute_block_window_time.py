"""Times block kriging through the moving window at BASELINE config 2 (OK2D, N = 5000, exponential, the 1000 x 1000 grid on the unit
square) and writes profiles/execute_block_window_time.txt.  For k = 10, 50, 100, beside each other:

  1. execute('grid', n_closest_points=k): the point predict of the grid nodes through the window;
  2. execute_block_window('grid', block_size = the grid spacing, k) with n_disc = 1, 4 x 4 and 8 x 8: every grid cell as a block;

and once the global execute_block('grid') with the same n_disc (the dense contraction over the resident inverse).

Per call: the wall time of the Python call (best and worst of --repeats after one warm-up) and, from last_timing, the event-timed rhs_ms
(neighbour search + right-hand sides: nd k variogram values per block; for blocks also gbar and its subtraction), contract_ms (the
per-block solves: the same whatever nd is) and predict_ms, with the solver that ran.  What to read off: n_disc = 1 beside execute() with
the same window (the same kernels: its runs lie among that call's own), rhs_ms against contract_ms as nd grows (nd k variogram values beside
~k^3 / 6 multiply-adds), and the window beside the global form.

--bench LABEL=FILE (twice: parent=..., this=...) appends the `bench.py --moving-window K` result lines kept in FILE (one JSON line per
run) and the comparison the change of k_mw_rhs's argument list is held to: this commit's median ms_per_step must not exceed the parent's
slowest run by more than the parent's own max - min.

    python scripts/execute_block_window_time.py [--repeats 3] [--grid 1000] [--bench parent=FILE --bench this=FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_section(specs):
    """The bench.py --moving-window lines of parent and this commit, per window, and the verdict."""
    runs = {}
    for spec in specs:
        label, path = spec.split("=", 1)
        for ln in open(path):
            ln = ln.strip()
            if not ln.startswith("{"):
                continue
            d = json.loads(ln)
            if d.get("value") is None or "ms_per_step" not in d:
                continue
            k = int(d["config"]["n_closest_points"])
            ph = d.get("phases_ms_per_step", {})
            runs.setdefault(k, {}).setdefault(label, []).append((d["ms_per_step"], ph.get("rhs"), ph.get("contract")))
    lines = ["", "bench.py --gpus 1 --moving-window K (config 2, execute('grid', n_closest_points=K)): ms_per_step of every run [device rhs / contract ms]"]
    for k in sorted(runs):
        for label in sorted(runs[k]):
            lines.append("  k = %-4d %-7s %s" % (k, label, "   ".join("%.3f [%s / %s]" % (m, "%.3f" % r if r is not None else "-", "%.3f" % c if c is not None else "-")
                                                                     for m, r, c in runs[k][label])))
        if "parent" in runs[k] and "this" in runs[k]:
            p = [m for m, _, _ in runs[k]["parent"]]
            t = [m for m, _, _ in runs[k]["this"]]
            spread, med = max(p) - min(p), float(np.median(t))
            ok = med <= max(p) + spread
            lines.append("           parent slowest %.3f, parent max - min %.3f, this commit's median %.3f: %s (limit %.3f)"
                         % (max(p), spread, med, "within the parent's spread" if ok else "SLOWER than the parent's spread allows", max(p) + spread))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 50, 100])
    ap.add_argument("--n-disc", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--bench", action="append", default=[], metavar="LABEL=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "execute_block_window_time.txt"))
    a = ap.parse_args()
    import pykrige_amd as pa

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
        i = int(np.argmin(ts))
        return min(ts) * 1e3, max(ts) * 1e3, tms[i], tms, out

    def line(label, r):
        tm = r[2]
        return ("  %-44s %9.2f ms (%.2f)   device: rhs %8.2f  contract %8.2f  predict %8.2f ms   predict of every run: %s   mw_kernel %d"
                % (label, r[0], r[1], tm["rhs_ms"], tm["contract_ms"], tm["predict_ms"], " ".join("%.2f" % t["predict_ms"] for t in r[3]),
                   tm["mw_kernel"]))

    lines = ["block kriging through the moving window at config 2 (OK2D exponential, N = %d, %d x %d grid, block = one grid cell of %.6f); wall ms "
             "of the Python call: best (worst) of %d runs after a warm-up" % (n, a.grid, a.grid, cell, a.repeats), ""]
    for k in a.k:
        r0 = best(lambda: ok.execute("grid", gx, gy, backend="loop", n_closest_points=k))
        lines.append(line("execute(n_closest_points=%d)" % k, r0))
        z0, s0 = [np.asarray(q) for q in r0[4]]
        p0 = [t["predict_ms"] for t in r0[3]]
        for nd in a.n_disc:
            r = best(lambda: ok.execute_block_window("grid", gx, gy, cell, k, n_disc=nd))
            lines.append(line("execute_block_window k = %d, n_disc = %d x %d" % (k, nd, nd), r))
            z, s = [np.asarray(q) for q in r[4]]
            extra = ""
            if nd == 1:
                p1 = [t["predict_ms"] for t in r[3]]  # the same kernels: its runs should lie among execute()'s own
                extra = "   bits of execute(): %s   predict_ms %.2f .. %.2f beside execute()'s own %.2f .. %.2f: %s" % (
                    bool(np.array_equal(z, z0) and np.array_equal(s, s0)), min(p1), max(p1), min(p0), max(p0),
                    "the ranges overlap" if min(p1) <= max(p0) and min(p0) <= max(p1) else "the ranges do NOT overlap")
            lines.append("      rhs_ms / execute's %.2f   rhs_ms / contract_ms %.2f   mean sigma^2 %.6g (execute: %.6g)   max |z - execute's z| %.3g%s"
                         % (r[2]["rhs_ms"] / r0[2]["rhs_ms"], r[2]["rhs_ms"] / r[2]["contract_ms"], float(s.mean()), float(s0.mean()),
                            float(np.abs(z - z0).max()), extra))
        lines.append("")
    lines.append("the global form (the dense contraction over the resident inverse):")
    for nd in a.n_disc:
        ok.execute_block("grid", gx, gy, cell, n_disc=nd)  # warm-up (the first one factors)
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ok.execute_block("grid", gx, gy, cell, n_disc=nd)
            ts.append(time.perf_counter() - t0)
        tm = ok.last_timing
        lines.append("  %-44s %9.2f ms (%.2f)   device: rhs %8.2f  contract %8.2f  predict %8.2f ms"
                     % ("execute_block n_disc = %d x %d" % (nd, nd), min(ts) * 1e3, max(ts) * 1e3, tm["rhs_ms"], tm["contract_ms"], tm["predict_ms"]))
    if a.bench:
        lines += bench_section(a.bench)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
