"""Write tests/golden/fields/ok2d.npz: several value fields on one station set, kriged by upstream PyKrige one field at a time.

    python scripts/make_golden_fields.py --reference-src PATH   # PATH: the directory that holds upstream's `pykrige` package

The fixture lives in a subdirectory because tests/_fixtures.names() treats every top-level .npz as an execute() fixture.
300 stations (12 of them on grid nodes: the exact-hit rule), F = 5 fields, a 40 x 30 grid, exponential variogram.  The variogram
is given explicitly, so each field's reference object uses the same one -- the rule of execute_fields.  Only inputs and the
reference's outputs are stored (tests/test_fields.py reads them).
"""
import argparse
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fields", "ok2d.npz")
PARAMS = {"sill": 1.2, "range": 0.35, "nugget": 0.05}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-src", required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference_src)
    import pykrige.ok as rok

    rng = np.random.default_rng(20261016)
    n, nf = 300, 5
    x, y = rng.random(n), rng.random(n)
    gx, gy = np.linspace(0.0, 1.0, 40), np.linspace(0.0, 1.0, 30)
    nodes = rng.choice(40 * 30, size=12, replace=False)
    x[:12], y[:12] = gx[nodes % 40], gy[nodes // 40]
    t = np.arange(nf)[None, :]
    values = np.sin((4 + t) * x[:, None] + t) * np.cos((3 + 0.5 * t) * y[:, None]) + 0.1 * rng.standard_normal((n, nf))
    zs, ss = [], None
    for f in range(nf):
        ok = rok.OrdinaryKriging(x, y, values[:, f], variogram_model="exponential", variogram_parameters=dict(PARAMS))
        z, s = ok.execute("grid", gx, gy, backend="vectorized")
        zs.append(np.ma.getdata(z))
        if ss is None:
            ss = np.ma.getdata(s)
        else:  # sigma^2 does not depend on the values
            assert np.allclose(ss, np.ma.getdata(s), rtol=0, atol=1e-12)
    np.savez_compressed(OUT, x=x, y=y, values=values, gx=gx, gy=gy, sill=PARAMS["sill"], range=PARAMS["range"],
                        nugget=PARAMS["nugget"], z=np.array(zs), ss=ss)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
