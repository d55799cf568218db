"""Child process of test_gpu_nullruns.py::test_many_rounds_per_wave: pdx_aggregate over the golden recipes whose row numbers are given on
the command line; one JSON line per recipe: {"i": row, "res": [[is_null, bits], ...], "counts": [...]}.  The parent sets the environment
(the emit grid of the nullable sum is read once per process)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(rows):
    import torch

    import _nullruns as NR
    from conftest import Golden
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column as K

    L.check(L.load().pdx_init(0))
    g = Golden("nullruns_golden.npz")
    for i in rows:
        pattern, n, dtype = g.manifest["patterns"][g.z["pattern"][i]], int(g.z["n"][i]), g.manifest["dtypes"][g.z["dtype"][i]]
        col = NR.column(K, L, torch, dtype, NR.values(dtype, n, int(g.z["seed"][i])), NR.validity(pattern, n), offset=64 * (i & 1) + 1,
                        kind=int(g.z["poison"][i]))
        got = [K.aggregate(k, col) for k in NR.KINDS]
        print(json.dumps({"i": i, "res": [list(NR.encode(dtype, k, v)) for k, (v, _) in zip(NR.KINDS, got)], "counts": [c for _, c in got]}), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]])
