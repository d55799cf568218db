#!/usr/bin/env python3
"""Accuracy of the float64 running sum, for DESIGN section 11: one column of 1e7 normal(0, 100) values, start 0; the largest
|got_i - E_i| / (u S_i), u = 2^-53, S_i = sum |x_j| (j <= i), over 1000 evenly spaced prefixes, for this library's tree scan and for the
sequential left-to-right sum (numpy's cumsum: the order, and so the bits, of Arrow's cumulative_sum).  E_i is exact: every float64 is an
integer times a power of two, and the running sum is kept as a Python integer on the grid 2^-1140.
Usage: python tools/scan_accuracy.py [--rows 1e7]   (one JSON line)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pandasarrow_amd import _lib as L  # noqa: E402
from pandasarrow_amd import column as K  # noqa: E402

GRID = 1140


def to_grid(x):
    n, d = float(x).as_integer_ratio()
    return n << (GRID - (d.bit_length() - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    n = int(ap.parse_args().rows)
    L.check(L.load().pdx_init(0))
    a = np.random.default_rng(2026).standard_normal(n) * 100
    got = K.cumulative(L.CUM_SUM, K.Column.from_numpy(a), 0.0).to_numpy()[0]
    seq = np.cumsum(a)
    sample = set(np.linspace(0, n - 1, 1000).astype(np.int64).tolist())
    exact = mag = 0
    worst = {"tree": 0.0, "sequential": 0.0}
    for i, x in enumerate(a.tolist()):
        g = to_grid(x)
        exact += g
        mag += abs(g)
        if i in sample:
            for name, r in (("tree", got), ("sequential", seq)):
                err = abs(to_grid(r[i]) - exact)
                worst[name] = max(worst[name], ((err << (53 + 16)) // mag) / 65536.0)
    print(json.dumps({"rows": n, "prefixes": len(sample), "largest_error_in_u_S": worst,
                      "bits_equal_rows": int((got == seq).sum())}), flush=True)


if __name__ == "__main__":
    main()
