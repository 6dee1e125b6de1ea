"""Times one VecchiaGradPlan.grad (libmikvgrad.so) beside one VecchiaPlan.gram (libmikvecchia.so) of the same plan arguments and writes
profiles/vecchia_grad_time.txt:

  m = 10, 30 and 60 neighbours, ng = 0 and ng = 2 geometry parameters, 2 columns, at bench.py config 2's 5000 stations and at 1e6 random
  stations in the unit square; with --share the kernel times of one further child under rocprofv3 --kernel-trace --stats (1e6 stations,
  m = 30, ng = 2), for the share of k_vgrad_solve; with --fit a REML fit with anisotropy at 1e6 stations, m = 30, by
  fit_variogram_vecchia and by fit_variogram_vecchia_grad from the same start: evaluations, wall time, final nll.

Wall time of the Python call, median (min .. max) after one warm-up.  Every size is a child process under its own `timeout`; the first one
that fails ends the run.
Run on the GPU:  python scripts/vecchia_grad_time.py [--share] [--fit]"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.vecchia_time import FULL, MODEL, MS, PAR, stations, times_ms  # noqa: E402


def child(n, config2, repeat, ms, ngs):
    from pykrige_amd import likelihood as lk
    from pykrige_amd import vecchia as vc
    from pykrige_amd import vecchia_grad as vgd

    X, v = stations(n, config2)
    W = np.column_stack([v, np.ones(n)])
    dco = lk.anisotropy_derivatives(X, [1.0], [0.0])
    print("\nN = %d, %s" % (n, "stations of bench.py config 2" if config2 else "random stations in the unit square"))
    with vgd.VecchiaGradPlan(X, m=1):  # the first plan of the process loads the code objects
        pass
    for m in ms:
        with vc.VecchiaPlan(X, m=m) as plan6:
            gram = times_ms(lambda: plan6.gram(X, MODEL, PAR, W), repeat)
        with vgd.VecchiaGradPlan(X, m=m) as plan:
            for ng in ngs:
                grad = times_ms(lambda: plan.grad(X, dco[:ng], MODEL, PAR, W), repeat)
                print("  m = %2d ng = %d   gram, 2 columns %10.3f ms (%.3f .. %.3f)   grad, 2 columns %10.3f ms (%.3f .. %.3f)   grad / gram %.2f"
                      % ((m, ng) + gram + grad + (grad[0] / gram[0],)), flush=True)


def fit_child(n, m):
    from pykrige_amd import vecchia as vc
    from pykrige_amd import vecchia_grad as vgd

    X, v = stations(n, False)
    print("\nREML fit with anisotropy, N = %d random stations, m = %d, start %r" % (n, m, FULL))
    for name, fn in (("fit_variogram_vecchia_grad (L-BFGS-B)", vgd.fit_variogram_vecchia_grad), ("fit_variogram_vecchia (Nelder-Mead)", vc.fit_variogram_vecchia)):
        t0 = time.perf_counter()
        fit = fn(X[:, 0], X[:, 1], v, MODEL, m=m, start=FULL, fit_anisotropy=True)
        print("  %-40s %8.1f s  %5d evaluations  final nll %.6f  success %s\n    %r\n    %s"
              % (name, time.perf_counter() - t0, fit.n_evaluations, fit.nll, fit.success, fit, fit.message), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--fit-child", type=int, default=0)
    ap.add_argument("--config2", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--ms", type=int, nargs="*", default=list(MS))
    ap.add_argument("--ngs", type=int, nargs="*", default=[0, 2])
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000000])
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecchia_grad_time.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config2, a.repeat, a.ms, a.ngs)
        return
    if a.fit_child:
        fit_child(a.fit_child, 30)
        return
    me = [sys.executable, os.path.abspath(__file__)]
    text = ["vecchia_grad.VecchiaGradPlan.grad (one mvg_plan_grad: upload of coordinates, geometry sets and W, k_vec_solve, k_vec_reduce, k_vgrad_solve, "
            "k_vgrad_reduce, copy back) beside vecchia.VecchiaPlan.gram (one mvc_plan_gram); wall ms of the Python call: median (min .. max) after one warm-up",
            "model %s, variogram_parameters %r, order 'random', seed 0" % (MODEL, FULL)]
    jobs = [(["--child", "5000", "--config2"], 240)] + [(["--child", str(n)], 600) for n in a.sizes]
    jobs = [(j + ["--repeat", str(a.repeat), "--ms"] + [str(m) for m in a.ms] + ["--ngs"] + [str(g) for g in a.ngs], lim) for j, lim in jobs]
    rc = 0
    for job, limit in jobs:
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + me + job, capture_output=True, text=True, cwd=ROOT)
        text.append(r.stdout.rstrip("\n"))
        rc = r.returncode
        if rc != 0:
            text.append("%s: the child ended with status %d\n%s" % (" ".join(job), rc, r.stderr[-2000:]))
            break
    if rc == 0 and a.share:
        with tempfile.TemporaryDirectory() as d:
            job = ["--child", str(a.sizes[-1]), "--repeat", "3", "--ms", "30", "--ngs", "2"]
            r = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"] + me + job,
                               capture_output=True, text=True, cwd=ROOT)
            rc = r.returncode
            text.append("\nkernel times of %s under rocprofv3 --kernel-trace --stats (one plan with m = 1 and one with m = 30; 1 + 3 gram and 1 + 3 grad):"
                        % " ".join(job))
            for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
                text += [ln.rstrip("\n") for ln in open(path) if "k_v" in ln or ln.startswith('"Name"')]
            if rc != 0:
                text.append("the child ended with status %d\n%s" % (rc, r.stderr[-2000:]))
    if rc == 0 and a.fit:
        r = subprocess.run(["timeout", "-k", "10", "900"] + me + ["--fit-child", str(a.sizes[-1])], capture_output=True, text=True, cwd=ROOT)
        rc = r.returncode
        text.append(r.stdout.rstrip("\n"))
        if rc != 0:
            text.append("the fit child ended with status %d\n%s" % (rc, r.stderr[-2000:]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    sys.exit(0 if rc == 0 else 1)


if __name__ == "__main__":
    main()
