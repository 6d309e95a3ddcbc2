#!/usr/bin/env python
"""tests/golden/lpd/lpd_mp.npz: the log predictive density of every point of the test grid (tests/_lpd_ref.py: grid, GRID_LIKS,
GRID_NODES) from the mpmath restatement at 40 digits, rounded to float64 -- about three minutes of mpmath, which is why the values
are kept as a fixture.  tests/test_lpd_host.py recomputes a sample of them and compares the float64 restatement with all of them.

    python tools/make_lpd_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lpd_ref as Rf  # noqa: E402


def main():
    out = {}
    for name, lik in Rf.GRID_LIKS.items():
        y, mu, var = Rf.grid(name)
        out[f"{name}/y"], out[f"{name}/mu"], out[f"{name}/var"] = y, mu, var
        if name in Rf.QUAD:
            for n in Rf.GRID_NODES:
                x, w = Rf.gh_rule(n)
                out[f"{name}/lpd{n}"] = Rf.lpd_mp(lik, y, mu, var, x, w)
                print(name, n, flush=True)
        else:
            out[f"{name}/lpd"] = Rf.lpd_mp(lik, y, mu, var)
            print(name, flush=True)
    path = os.path.join(ROOT, "tests", "golden", Rf.GOLDEN)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main()
