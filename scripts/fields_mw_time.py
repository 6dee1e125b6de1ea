"""Wall clock of execute_fields with a moving window against F execute(..., n_closest_points=k) calls, at BASELINE config 2's stations
(OK2D, N = 5000, 1000 x 1000 grid, exponential).

    python scripts/fields_mw_time.py [--windows 10,100] [--fields 1,8,32] [--repeats 3] [--leg both|fields|loop] [--out FILE.json]

For every (k, F): the best of --repeats execute_fields calls, the best single execute(n_closest_points=k), and F such calls, one per
field on an object built for that field (what a caller without the moving-window execute_fields runs; timed once).  --leg loop times
only the F calls (so that a checkout of the parent commit can run that leg with this script), --leg fields only execute_fields.  Each
JSON line also carries the device phases of the last timed call."""
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
    ap.add_argument("--windows", default="10,100")
    ap.add_argument("--fields", default="1,8,32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--leg", default="both", choices=("both", "fields", "loop"))
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

    def best(fn):
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    def phases(tm):
        return {key: tm[key] for key in ("rhs_ms", "contract_ms", "predict_ms", "mw_kernel")}

    rows = []
    for k in (int(w) for w in args.windows.split(",")):
        ok.execute("grid", g, g, backend="hip", n_closest_points=k)  # warm-up
        t_one = best(lambda: ok.execute("grid", g, g, backend="hip", n_closest_points=k))
        one_ms = phases(ok.last_timing)
        for nf in counts:
            row = {"config": "OK2D N=5000 1000x1000 exponential", "k": k, "F": nf, "execute_s": t_one, "execute_device_ms": one_ms}
            if args.leg != "loop":
                ok.execute_fields("grid", g, g, values[:, :nf], backend="hip", n_closest_points=k)  # warm-up
                row["execute_fields_s"] = best(lambda: ok.execute_fields("grid", g, g, values[:, :nf], backend="hip", n_closest_points=k))
                row["ratio_to_execute"] = row["execute_fields_s"] / t_one
                row["device_ms"] = phases(ok.last_timing)
            if args.leg != "fields":
                t0 = time.perf_counter()
                for f in range(nf):
                    o = pa.OrdinaryKriging(x, y, values[:, f], **kw)
                    o.execute("grid", g, g, backend="hip", n_closest_points=k)
                    del o
                row["F_executes_s"] = time.perf_counter() - t0
            if "execute_fields_s" in row and "F_executes_s" in row:
                row["speedup_vs_F_executes"] = row["F_executes_s"] / row["execute_fields_s"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
