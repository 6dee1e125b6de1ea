"""Wall clock of execute_fields against execute() at BASELINE config 2 (OK2D, N = 5000 stations, 1000 x 1000 grid, exponential).

    python scripts/fields_time.py [--fields 1,8,32,128] [--repeats 3] [--loop-max 128] [--out FILE.json]

For every F: the best of --repeats execute_fields calls, next to the best single execute() and to F execute() calls, one per field on
an object built for that field (what a caller without execute_fields runs; timed once; beyond --loop-max fields the loop is not run).
The object of execute_fields is factored before any timing.  Each JSON line also carries the device phases of the last execute_fields."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pykrige_amd as pa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="1,8,32,128")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2)
    n = 5000
    x, y = rng.random(n), rng.random(n)
    counts = [int(f) for f in args.fields.split(",")]
    values = np.sin(6 * x)[:, None] * np.cos(4 * y)[:, None] + 0.1 * rng.standard_normal((n, max(counts)))
    g = np.linspace(0.0, 1.0, 1000)
    kw = dict(variogram_model="exponential", variogram_parameters={"psill": 1.0, "range": 0.3, "nugget": 0.01})
    ok = pa.OrdinaryKriging(x, y, values[:, 0], **kw)
    ok.execute("grid", g, g)  # factor + warm-up
    ok.execute_fields("grid", g, g, values[:, :2])

    def best(fn):
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    t_one = best(lambda: ok.execute("grid", g, g))
    rows = []
    for nf in counts:
        t_fields = best(lambda: ok.execute_fields("grid", g, g, values[:, :nf]))
        tm = ok.last_timing
        t_loop = None
        if nf <= args.loop_max:
            t0 = time.perf_counter()
            for f in range(nf):
                o = pa.OrdinaryKriging(x, y, values[:, f], **kw)
                o.execute("grid", g, g)
                del o
            t_loop = time.perf_counter() - t0
        row = {"config": "OK2D N=5000 1000x1000 exponential", "F": nf, "execute_fields_s": t_fields, "execute_s": t_one,
               "ratio_to_execute": t_fields / t_one, "F_executes_s": t_loop,
               "speedup_vs_F_executes": (t_loop / t_fields) if t_loop else None,
               "device_ms": {k: tm[k] for k in ("rhs_ms", "contract_ms", "predict_ms")}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
