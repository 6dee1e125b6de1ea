"""Times execute_cov at BASELINE config 2's stations (OK2D, N = 5000, exponential) for P = 4096 and 8192 random points and writes
profiles/execute_cov_time.txt.  Beside each other, per P:

  1. one execute('points') of the same points (z and sigma^2 alone);
  2. execute_cov: the same predict into one panel, the three stages of csrc/mik_k_cov.h and the copy back of P x P doubles;
  3. the host route a caller without it takes: get_matrix(1) (the inverse, Mp^2 doubles over the link), the right-hand sides and
     -gamma* in NumPy, then b @ B and (b @ B) @ b^T in NumPy's GEMM on the host's cores.

Wall times of the Python calls (best of --repeats after one warm-up).  The stages are timed by the library's own events
(MIK_COV_PROF=1 prints them to stderr; this script reads that line from a redirected stderr); their executed flops -- stage 1
2 Pp Mp kend, stage 2 the upper block triangle nPblk (nPblk + 1) / 2 tiles of 2 . 128 . 128 . kend -- over those times are given as
fractions of the fp64 matrix peak bench.py uses (78.6 Tflop/s).  The host route's result is compared with the device's.

    python scripts/execute_cov_time.py [--repeats 3]"""
import argparse
import os
import re
import sys
import tempfile
import time

os.environ["MIK_COV_PROF"] = "1"  # (read by the library at its first mik_predict_cov)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pykrige_amd as pa  # noqa: E402

PEAK = 78.6e12


def captured_stderr(fn):
    """fn() with file descriptor 2 redirected to a temporary file; returns (fn's result, what was written)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode("utf-8", "replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--points", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "execute_cov_time.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(2)
    n = a.n
    x, y = rng.random(n), rng.random(n)
    v = np.sin(6 * x) * np.cos(4 * y) + 0.1 * rng.standard_normal(n)
    params = {"psill": 1.0, "range": 0.3, "nugget": 0.01}
    ok = pa.OrdinaryKriging(x, y, v, variogram_model="exponential", variogram_parameters=params)

    def best(fn):
        fn()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return min(ts) * 1e3, max(ts) * 1e3, out

    lines = ["execute_cov at config 2's stations (OK2D exponential, N = %d); wall ms of the Python call: best (worst) of %d runs after a "
             "warm-up; fractions of the fp64 matrix peak of %.1f Tflop/s" % (n, a.repeats, PEAK / 1e12)]
    for npt in a.points:
        px, py = rng.random(npt), rng.random(npt)
        t1 = best(lambda: ok.execute("points", px, py))
        tm1 = dict(ok.last_timing)
        (t2, err) = captured_stderr(lambda: best(lambda: ok.execute_cov("points", px, py)))
        tm2 = dict(ok.last_timing)
        z, cov = t2[2]
        prof = [dict((k, float(val)) for k, val in re.findall(r"(\w+) ([-0-9.e+]+)", ln)) for ln in err.splitlines() if ln.startswith("mik_predict_cov:")]
        lines.append("")
        lines.append("P = %d" % npt)
        lines.append("  1. execute('points')   %10.2f ms (%.2f)   device: rhs %.2f  contract %.2f  predict %.2f ms"
                     % (t1[0], t1[1], tm1["rhs_ms"], tm1["contract_ms"], tm1["predict_ms"]))
        lines.append("  2. execute_cov         %10.2f ms (%.2f)   device: rhs %.2f  contract %.2f  predict %.2f ms"
                     % (t2[0], t2[1], tm2["rhs_ms"], tm2["contract_ms"], tm2["predict_ms"]))
        if prof:
            p = min(prof[1:] or prof, key=lambda d: d["stage1_ms"] + d["stage2_ms"])
            pp, mp, kend = p["Pp"], p["Mp"], p["kend"]
            nb = pp / 128
            f1, f2 = 2.0 * pp * mp * kend, nb * (nb + 1) / 2 * 2.0 * 128 * 128 * kend
            lines.append("     stage 0 (-gamma*) %.3f ms; stage 1 (Yt = Bt B^T, %.3g flop) %.3f ms = %.1f Tflop/s, %.2f of peak; stage 2 (triangle "
                         "of Bt Yt^T, %.3g flop) %.3f ms = %.1f Tflop/s, %.2f of peak; copy back of %.0f MB %.2f ms = %.1f GB/s"
                         % (p["stage0_ms"], f1, p["stage1_ms"], f1 / p["stage1_ms"] / 1e9, f1 / p["stage1_ms"] / 1e9 * 1e12 / PEAK,
                            f2, p["stage2_ms"], f2 / p["stage2_ms"] / 1e9, f2 / p["stage2_ms"] / 1e9 * 1e12 / PEAK,
                            8.0 * npt * npt / 1e6, p["copy_ms"], 8.0 * npt * npt / p["copy_ms"] / 1e6))
        else:
            lines.append("     (the library printed no MIK_COV_PROF line)")

        def host_route():
            h = ok._get_handle()
            binv = h.get_matrix(1)[:n + 1, :n + 1]
            d = np.hypot(px[:, None] - ok.X_ADJUSTED[None, :], py[:, None] - ok.Y_ADJUSTED[None, :])
            b = np.empty((npt, n + 1))
            b[:, :n] = -ok.variogram_function(ok.variogram_model_parameters, d)
            b[:, :n][d <= ok.eps] = 0.0
            b[:, n] = 1.0
            dpq = np.hypot(px[:, None] - px[None, :], py[:, None] - py[None, :])
            c = -np.where(dpq <= ok.eps, 0.0, ok.variogram_function(ok.variogram_model_parameters, dpq))
            return c - (b @ binv) @ b.T

        t0 = time.perf_counter()
        hc = host_route()
        t3 = (time.perf_counter() - t0) * 1e3
        lines.append("  3. host route (get_matrix + NumPy, once) %10.2f ms; max |device - host| %.3g (max |cov| %.3g)"
                     % (t3, float(np.abs(hc - cov).max()), float(np.abs(cov).max())))
        del hc, cov
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
