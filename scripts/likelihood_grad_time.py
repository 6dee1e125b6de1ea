"""Times likelihood.gram_grad (libmikgrad.so) beside likelihood.gram (libmiklik.so) and a whole REML fit by both methods, and writes
profiles/likelihood_grad_time.txt:

  one gradient call (F = 1, p = 1, two geometry parameters, REML) beside one gram (m = 2) at bench.py config 2's 5000 stations and at
  20000 random stations; the per-kernel split of one gradient call at N = 5000 (rocprofv3 --kernel-trace --stats); one REML fit with
  fit_anisotropy=True at N = 5000 by method='nelder-mead' and by method='l-bfgs-b' from the same start: evaluations, seconds, final nll.

Every GPU step is a child process under its own `timeout`; the first one that fails ends the run.
Run on the GPU:  python scripts/likelihood_grad_time.py"""
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
SCALING, ANGLE = [1.5], [20.0]


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


def problem(n, config2):
    from pykrige_amd import likelihood as lk

    raw, v = stations(n, config2)
    adj = lk._adjust(raw, SCALING, ANGLE)
    return adj, lk.anisotropy_derivatives(raw, SCALING, ANGLE), v[:, None], np.ones((n, 1))


def step(name, a):
    from pykrige_amd import likelihood as lk

    out = {}
    if name in ("grad5000", "grad20000"):
        n = a.n if name == "grad5000" else a.big
        adj, dco, V, X = problem(n, name == "grad5000")
        repeat = a.repeat if n <= 5000 else 2
        W = np.hstack([V, X])
        out["gram"] = times_ms(lambda: lk.gram(adj, MODEL, PAR, W), repeat)
        out["grad"] = times_ms(lambda: lk.gram_grad(adj, dco, MODEL, PAR, V, X, True), repeat)
        logdet, G = lk.gram(adj, MODEL, PAR, W)
        got = lk.gram_grad(adj, dco, MODEL, PAR, V, X, True)
        out["same_bits"] = bool(logdet == got[0] and np.array_equal(G, got[1]))
        out["gradient"] = [float(t) for t in got[2][0]]
    elif name == "profile5000":
        adj, dco, V, X = problem(a.n, True)
        lk.gram_grad(adj, dco, MODEL, PAR, V, X, True)
    elif name in ("fit_nelder-mead", "fit_l-bfgs-b"):
        raw, v = stations(a.n, True)
        t0 = time.perf_counter()
        fit = lk.fit_variogram_ml(raw[:, 0], raw[:, 1], v, MODEL, fit_anisotropy=True, reml=True, method=name[4:])
        out = dict(seconds=time.perf_counter() - t0, fit=repr(fit), evaluations=fit.n_evaluations, nll=fit.nll, message=fit.message)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "likelihood_grad_time.txt"))
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    lines = ["likelihood.gram_grad (one mlg_grad: upload, assemble, seed, eliminate [[C], [W^T], [I]] over n columns, small algebra, k_grad_pairs, "
             "copy back, free) beside likelihood.gram (one mlk_gram); wall ms of the Python call: median (min .. max) after one warm-up",
             "model %s, variogram_parameters %s, anisotropy_scaling %s, anisotropy_angle %s; F = 1 field, p = 1 trend column, ng = 2, REML"
             % (MODEL, FULL, SCALING[0], ANGLE[0]), ""]
    for name, n, label, limit in (("grad5000", a.n, "stations of bench.py config 2", 300), ("grad20000", a.big, "random stations in the unit square", 600)):
        r = child(name, a, limit)
        g, d = r["gram"], r["grad"]
        lines.append("N = %d, %s" % (n, label))
        lines.append("  gram       %10.3f ms (%.3f .. %.3f)" % tuple(g))
        lines.append("  gram_grad  %10.3f ms (%.3f .. %.3f)   gram_grad / gram %.2f   logdet and G the same bits: %s"
                     % (d[0], d[1], d[2], d[0] / g[0], r["same_bits"]))
        lines.append("  gradient (psill, range, nugget, scaling, angle per degree): %s" % " ".join("%.6g" % t for t in r["gradient"]))
        lines.append("")
    with tempfile.TemporaryDirectory() as d:
        child("profile5000", a, 300, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "grad", "--"])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for ln in open(path).read().splitlines()[1:]:
                cells = ln.rsplit(",", 7)
                rows.append((cells[0].strip('"'), int(cells[1]), float(cells[2])))
    own = [r for r in rows if "k_lik_" in r[0] or "k_grad_" in r[0]]
    total = sum(r[2] for r in own)
    lines.append("kernels of one gram_grad at N = %d (rocprofv3 --kernel-trace --stats, one call in the process)" % a.n)
    for name, calls, ns in sorted(own, key=lambda r: -r[2]):
        at = name.index("k_lik_") if "k_lik_" in name else name.index("k_grad_")
        lines.append("  %-16s %5d launches %10.3f ms  %5.1f %%" % (name[at:].split("(")[0], calls, ns / 1e6, 100.0 * ns / total))
    lines.append("  all kernels      %10.3f ms" % (total / 1e6))
    lines.append("")
    lines.append("fit_variogram_ml(fit_anisotropy=True, reml=True) at N = %d, start = the least-squares fit" % a.n)
    for method in ("nelder-mead", "l-bfgs-b"):
        r = child("fit_" + method, a, 900)
        lines.append("  method=%-13r %7.2f s, %4d evaluations, final nll %.6f" % (method, r["seconds"], r["evaluations"], r["nll"]))
        lines.append("    " + r["fit"])
        lines.append("    message: " + r["message"])
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
