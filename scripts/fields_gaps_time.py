"""Times execute_fields(valid=...) at BASELINE config 2 (OK2D, N = 5000 stations, 1000 x 1000 grid, exponential) with 32 fields and
writes profiles/fields_gaps_time.txt.  Three gap settings -- no gaps, 1 % of the stations missing per field in distinct patterns, one
pattern shared by all fields -- and for each, beside each other:

  1. execute_fields without valid (the values at the missing entries as they are);
  2. the call with valid;
  3. one factor + execute of a subset object (what a caller without valid runs per pattern), timed once, times the patterns it replaces.

Wall times of the Python calls (best of --repeats after one warm-up) and the device phases of mik_timing.  predict_ms spans the
set-up of the patterns and every launch; the extra device time of the gaps is reported as predict_ms(2) - predict_ms(1), and the
achieved rate of the extra GEMM (2 . rows . Mp . points flops, rows as padded) over that difference as a LOWER bound beside
k_contract's rate from the same run (contract_flops_executed / contract_ms).  The library does not time the set-up and the GEMM apart.

    python scripts/fields_gaps_time.py [--fields 32] [--repeats 3]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_gaps_time.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    n, nf = a.n, a.fields
    x, y = rng.random(n), rng.random(n)
    values = np.sin(6 * x)[:, None] * np.cos(4 * y)[:, None] + 0.1 * rng.standard_normal((n, nf))
    g = np.linspace(0.0, 1.0, a.grid)
    kw = dict(variogram_model="exponential", variogram_parameters={"psill": 1.0, "range": 0.3, "nugget": 0.01})
    ok = pa.OrdinaryKriging(x, y, values[:, 0], **kw)
    ok.execute("grid", g, g)  # factor + warm-up
    mp = -(-(n + 1) // 128) * 128
    npt = a.grid * a.grid

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
    lines = ["execute_fields(valid=...) at config 2's stations and grid (OK2D exponential, N = %d, %d x %d grid), F = %d; wall ms of the "
             "Python call: best (worst) of %d runs after a warm-up" % (n, a.grid, a.grid, nf, a.repeats)]
    for what, valid in (("no gaps", np.ones((n, nf), dtype=bool)), ("%d missing per field, distinct patterns" % m, distinct),
                        ("%d missing, one shared pattern" % m, shared)):
        npat = len({valid[:, f].tobytes() for f in range(nf) if not valid[:, f].all()})
        rows = sum(-(-int((~valid[:, f]).sum()) // 16) * 16 for f in {valid[:, f].tobytes(): f for f in range(nf) if not valid[:, f].all()}.values())
        rows = -(-rows // 128) * 128
        t1 = best(lambda: ok.execute_fields("grid", g, g, values))
        tm1 = dict(ok.last_timing)
        t2 = best(lambda: ok.execute_fields("grid", g, g, values, valid=valid))
        tm2 = dict(ok.last_timing)
        lines.append("")
        lines.append("%s: %d patterns, %d rows of W" % (what, npat, rows))
        lines.append("  1. execute_fields without valid   %10.2f ms (%.2f)   device: rhs %.2f  contract %.2f  predict %.2f ms"
                     % (t1[0], t1[1], tm1["rhs_ms"], tm1["contract_ms"], tm1["predict_ms"]))
        lines.append("  2. execute_fields with valid      %10.2f ms (%.2f)   device: rhs %.2f  contract %.2f  predict %.2f ms"
                     % (t2[0], t2[1], tm2["rhs_ms"], tm2["contract_ms"], tm2["predict_ms"]))
        rate_c = tm2["contract_flops_executed"] / (tm2["contract_ms"] * 1e-3) / 1e12
        extra = tm2["predict_ms"] - tm1["predict_ms"]
        if npat:
            lines.append("     set-up + GEMM + reduce (predict_ms difference) %.2f ms; GEMM 2 x %d x %d x %d flops: >= %.2f Tflop/s; "
                         "k_contract in the same run %.2f Tflop/s" % (extra, rows, mp, npt, 2.0 * rows * mp * npt / (extra * 1e-3) / 1e12, rate_c))
            f = next(f for f in range(nf) if not valid[:, f].all())
            keep = valid[:, f]
            t0 = time.perf_counter()
            o = pa.OrdinaryKriging(x[keep], y[keep], values[keep, f], **kw)
            o.execute("grid", g, g)
            del o
            t3 = (time.perf_counter() - t0) * 1e3
            lines.append("  3. one subset object: construct + factor + execute %10.2f ms; x %d patterns = %.2f ms" % (t3, npat, t3 * npat))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
