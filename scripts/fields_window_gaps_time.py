"""Times execute_fields_window() at BASELINE config 2 (OK2D, N = 5000 stations, 1000 x 1000 grid, exponential) with 32 fields at
k = 10 / 50 / 100 and writes profiles/fields_window_gaps_time.txt.  Three gap settings -- no gaps, 1 % of the stations missing per field in
32 distinct patterns, 1 % missing in one pattern shared by all fields -- and for each, beside each other:

  1. execute_fields(..., n_closest_points=k) without valid (every station, one search for all fields);
  2. execute_fields_window(..., k, valid=...);
  3. execute(..., n_closest_points=k) of a subset object built from the stations of one pattern (what a caller without the call runs per
     pattern: a new object, the stations uploaded and gridded again), timed once, times the patterns it replaces.

Wall times of the Python calls (best and worst of --repeats after one warm-up) and the device phases of mik_timing (summed over the
patterns for 2).  No ratio is expected beyond: P distinct patterns cost about P one-field window calls, one shared pattern about one
multi-field call.  --append FILE adds the lines of FILE (e.g. bench runs recorded beside it) at the end.

    python scripts/fields_window_gaps_time.py [--fields 32] [--repeats 3] [--windows 10,50,100]"""
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
    ap.add_argument("--fields", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--windows", default="10,50,100")
    ap.add_argument("--append", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_window_gaps_time.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    n, nf = a.n, a.fields
    x, y = rng.random(n), rng.random(n)
    values = np.sin(6 * x)[:, None] * np.cos(4 * y)[:, None] + 0.1 * rng.standard_normal((n, nf))
    g = np.linspace(0.0, 1.0, a.grid)
    kw = dict(variogram_model="exponential", variogram_parameters={"psill": 1.0, "range": 0.3, "nugget": 0.01})
    ok = pa.OrdinaryKriging(x, y, values[:, 0], **kw)

    def best(fn):
        fn()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, max(ts) * 1e3

    m = max(1, n // 100)
    distinct = np.ones((n, nf), dtype=bool)
    for f in range(nf):
        distinct[rng.choice(n, m, replace=False), f] = False
    shared = np.ones((n, nf), dtype=bool)
    shared[rng.choice(n, m, replace=False), :] = False
    dev = lambda tm: "device: search + rhs %.2f  solves %.2f  all %.2f ms  mw_kernel %d" % (tm["rhs_ms"], tm["contract_ms"], tm["predict_ms"], tm["mw_kernel"])  # noqa: E731
    lines = ["execute_fields_window at config 2's stations and grid (OK2D exponential, N = %d, %d x %d grid), F = %d; wall ms of the Python "
             "call: best (worst) of %d runs after a warm-up" % (n, a.grid, a.grid, nf, a.repeats)]
    for k in [int(s) for s in a.windows.split(",")]:
        t1 = best(lambda: ok.execute_fields("grid", g, g, values, backend="loop", n_closest_points=k))
        tm1 = dict(ok.last_timing)
        lines += ["", "k = %d" % k, "  1. execute_fields(n_closest_points=k), no valid      %10.2f ms (%.2f)   %s" % (t1[0], t1[1], dev(tm1))]
        for what, valid in (("no gaps", np.ones((n, nf), dtype=bool)), ("%d missing per field, %d distinct patterns" % (m, nf), distinct),
                            ("%d missing, one shared pattern" % m, shared)):
            npat = len({valid[:, f].tobytes() for f in range(nf)})
            v = values.copy()
            v[~valid] = np.nan
            t2 = best(lambda: ok.execute_fields_window("grid", g, g, v, k, valid=valid))
            tm2 = dict(ok.last_timing)
            lines.append("  2. execute_fields_window, %-42s %10.2f ms (%.2f)   %s" % (what + ":", t2[0], t2[1], dev(tm2)))
            if not valid.all():
                keep = valid[:, 0]

                def subset():
                    o = pa.OrdinaryKriging(x[keep], y[keep], values[keep, 0], **kw)
                    return o.execute("grid", g, g, backend="loop", n_closest_points=k)

                t3 = best(subset)
                lines.append("  3. one subset object + execute(n_closest_points=k)        %10.2f ms (%.2f)   x %d patterns = %.2f ms"
                             % (t3[0], t3[1], npat, npat * t3[0]))
    if a.append:
        lines += ["", open(a.append).read().rstrip("\n")]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
