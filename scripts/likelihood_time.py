"""Times likelihood.gram and a whole REML fit (libmiklik.so) and writes profiles/likelihood_time.txt:

  one gram at bench.py config 2's 5000 stations with m = 1 and m = 33 columns, and at 20000 random stations, beside the host route
  scipy.linalg.cho_factor + cho_solve on the same matrix (16 threads); the share of k_lik_syrk in the device time of one gram at
  N = 5000 and the flops it executes as a fraction of the 78.6 TFLOP/s fp64 matrix peak (rocprofv3 --kernel-trace --stats); one whole
  REML fit with anisotropy at N = 5000.

Every GPU step is a child process under its own `timeout`; the first one that fails ends the run.
Run on the GPU:  python scripts/likelihood_time.py"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL, FULL = "exponential", [1.0, 0.3, 0.05]  # config 2's variogram with a nugget of 5 % of the sill
PAR = [FULL[0] - FULL[2], FULL[1], FULL[2]]
PEAK = 78.6e12
NB, TS = 64, 128  # mlk::NB, mlk::TS


def stations(n, config2):
    if config2:
        import bench

        (x, y), v = bench.synth(bench.CONFIGS[2]["seed"], n, 2)
    else:
        rs = np.random.default_rng(n)
        x, y = rs.random(n), rs.random(n)
        v = np.sin(7 * x) + y + 0.1 * rs.standard_normal(n)
    return np.column_stack([x, y]), v


def columns(v, m):
    rs = np.random.default_rng(m)
    return np.column_stack([v] + [rs.standard_normal(v.size) for _ in range(m - 1)])


def times_ms(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def host_route(X, W):
    """What a user without the library writes: SciPy's Cholesky of the same matrix."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.spatial.distance import cdist

    from pykrige_amd import core

    Cm = (PAR[0] + PAR[2]) - core.variogram_value(MODEL, PAR, cdist(X, X))
    Cm[np.diag_indices(len(X))] = PAR[0] + PAR[2]
    t0 = time.perf_counter()
    c = cho_factor(Cm, lower=True, overwrite_a=True, check_finite=False)
    G = W.T @ cho_solve(c, W, check_finite=False)
    logdet = 2.0 * float(np.sum(np.log(np.diag(c[0]))))
    return (time.perf_counter() - t0) * 1e3, logdet, G


def syrk_flops(n, m):
    """Flops k_lik_syrk executes in one gram: 2 * 128 * 128 * jb per tile, three quarters of that on a diagonal tile (one of its four waves
    lies above the diagonal and is idle)."""
    npad = n + (m + 15) // 16 * 16
    total = 0.0
    for k0 in range(0, n, NB):
        jb = min(NB, n - k0)
        t = (npad - k0 - jb + TS - 1) // TS
        total += 2.0 * TS * TS * jb * (t * (t - 1) / 2 + 0.75 * t)
    return total


def step(name, a):
    from pykrige_amd import likelihood as lk

    out = {}
    if name in ("gram5000", "gram20000"):
        n = a.n if name == "gram5000" else a.big
        X, v = stations(n, name == "gram5000")
        for m in ((1, 33) if name == "gram5000" else (1,)):
            W = columns(v, m)
            t = times_ms(lambda: lk.gram(X, MODEL, PAR, W), a.repeat if n <= 5000 else 2)
            logdet, G = lk.gram(X, MODEL, PAR, W)
            th, hl, hG = host_route(X, W)
            s = np.sqrt(np.diag(hG))
            out["m%d" % m] = dict(gpu=t, host=th, dlogdet=abs(hl - logdet), dG=float((np.abs(hG - G) / (s[:, None] * s[None, :])).max()))
    elif name == "profile5000":
        X, v = stations(a.n, True)
        lk.gram(X, MODEL, PAR, columns(v, 1))
    elif name == "fit5000":
        X, v = stations(a.n, True)
        t0 = time.perf_counter()
        fit = lk.fit_variogram_ml(X[:, 0], X[:, 1], v, MODEL, fit_anisotropy=True, reml=True)
        out = dict(seconds=time.perf_counter() - t0, fit=repr(fit), evaluations=fit.n_evaluations)
    print("RESULT " + json.dumps(out), flush=True)


def child(name, a, seconds, prefix=()):
    cmd = ["timeout", "-k", "10", str(seconds)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(a.n),
                                                                  "--big", str(a.big), "--repeat", str(a.repeat)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("step %s ended with status %d: nothing further is started" % (name, r.returncode))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--big", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--step", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_time.txt"))
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    lines = ["likelihood.gram (one mlk_gram: upload, assemble, factor, copy back, free) and a whole REML fit; wall ms of the Python call: "
             "median (min .. max) after one warm-up",
             "model %s, variogram_parameters %s; host route: scipy.linalg.cho_factor + cho_solve on the assembled matrix (assembly not "
             "timed), OMP_NUM_THREADS=%s" % (MODEL, FULL, os.environ.get("OMP_NUM_THREADS", "unset")), ""]
    for name, n, label, limit in (("gram5000", a.n, "stations of bench.py config 2", 300), ("gram20000", a.big, "random stations in the unit square", 600)):
        res = child(name, a, limit)
        lines.append("N = %d, %s (N^3 / 3 = %.3g flop)" % (n, label, n ** 3 / 3.0))
        for key, r in res.items():
            g = r["gpu"]
            lines.append("  gram, m = %-2s  GPU %10.3f ms (%.3f .. %.3f)   host %10.1f ms   host / GPU %.1f   |logdet difference| %.2e  G difference %.2e"
                         % (key[1:], g[0], g[1], g[2], r["host"], r["host"] / g[0], r["dlogdet"], r["dG"]))
            if not g[0] < r["host"]:
                lines.append("  -> the GPU gram is NOT faster than the host route here")
        lines.append("")
    with tempfile.TemporaryDirectory() as d:
        child("profile5000", a, 300, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "lik", "--"])
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        rows = []
        for path in stats:
            for ln in open(path).read().splitlines()[1:]:
                cells = ln.rsplit(",", 7)
                rows.append((cells[0].strip('"'), int(cells[1]), float(cells[2])))
    lik = [r for r in rows if "k_lik_" in r[0]]
    total = sum(r[2] for r in lik)
    lines.append("kernels of one gram at N = %d, m = 1 (rocprofv3 --kernel-trace --stats, one call in the process)" % a.n)
    for name, calls, ns in sorted(lik, key=lambda r: -r[2]):
        short = name[name.index("k_lik_"):].split("(")[0]
        lines.append("  %-16s %5d launches %10.3f ms  %5.1f %%" % (short, calls, ns / 1e6, 100.0 * ns / total))
        if short == "k_lik_syrk":
            fl = syrk_flops(a.n, 1)
            lines.append("  %-16s executes %.4g flop (N^3 / 3 = %.4g): %.2f TFLOP/s, %.3f of the %.1f TFLOP/s fp64 matrix peak"
                         % ("", fl, a.n ** 3 / 3.0, fl / (ns * 1e-9) / 1e12, fl / (ns * 1e-9) / PEAK, PEAK / 1e12))
    lines.append("  all k_lik_* kernels %10.3f ms" % (total / 1e6))
    lines.append("")
    res = child("fit5000", a, 900)
    lines.append("fit_variogram_ml(fit_anisotropy=True, reml=True) at N = %d, start = the least-squares fit: %.2f s, %d evaluations (%.2f ms each)"
                 % (a.n, res["seconds"], res["evaluations"], 1e3 * res["seconds"] / res["evaluations"]))
    lines.append("  " + res["fit"])
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
