"""Times cross_validate at BASELINE config 2's stations (N = 5000, exponential model) and writes profiles/cross_validate_time.txt:

  cross_validate for F = 1 and F = 32 fields beside one mik_factor (the factor is resident: what the call adds to an execute()).

Wall times of the Python calls, median of `--repeat` runs after one warm-up.  Run on the GPU:  python scripts/cross_validate_time.py"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_validate_time.txt"))
    a = ap.parse_args()
    import bench
    import pykrige_amd as pa

    cfg = bench.CONFIGS[2]
    rng = np.random.default_rng(2)
    n = a.n
    (x, y), v = bench.synth(cfg["seed"], n, 2)
    m = pa.OrdinaryKriging(x, y, v, variogram_model=cfg["model"], variogram_parameters=cfg["params"])
    lines = ["cross_validate at the stations of bench.py config 2 (%s), N = %d; wall ms of the Python call: median (min .. max) of %d runs"
             % (cfg["name"], n, a.repeat)]
    h = m._get_handle()
    m._upload_and_factor()

    def factor():
        m._set_problem(h)
        h.factor()

    lines.append("mik_set_problem + mik_factor                      %9.2f ms (%.2f .. %.2f)" % median_ms(factor, a.repeat))
    lines.append("  factor phases of the last one: assemble %.2f ms, invert %.2f ms, probe %.2f ms" % (
        h.timing()["assemble_ms"], h.timing()["invert_ms"], h.timing()["verify_ms"]))
    m._factor_key = None
    m.cross_validate()
    assert m.factor_reused is False
    lines.append("global cross_validate, F = 1 (factor resident)     %9.2f ms (%.2f .. %.2f)" % median_ms(lambda: m.cross_validate(), a.repeat))
    assert m.factor_reused is True
    v32 = rng.standard_normal((n, 32))
    lines.append("global cross_validate, F = 32 (factor resident)    %9.2f ms (%.2f .. %.2f)" % median_ms(lambda: m.cross_validate(v32), a.repeat))
    zg, sg = m.cross_validate()
    lines.append("global residuals: rms %.4g, mean sigma^2 %.4g" % (float(np.sqrt(np.mean((v - zg) ** 2))), float(sg.mean())))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
