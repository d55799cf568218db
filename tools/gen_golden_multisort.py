#!/usr/bin/env python3
"""Golden vectors for pdx_sort_indices: Arrow 25.0.0's sort_indices (the kernel DataFrame::argsort calls, src/dataframe.cpp:1073-1091) on
the seeded case grid of tests/_multisort_ref.py -> tests/golden/multisort_golden.npz.

Per case: the digest of the inputs (they are regenerated from the seed, not stored), the digest of Arrow's answer, and the answer itself
up to FULL_OUTPUT_MAX_N rows.  Every case is sorted as a Table and as a RecordBatch; both answers must agree and are stored once.
Needs pyarrow; run from the repository root:  python tools/gen_golden_multisort.py"""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _multisort_ref as R  # noqa: E402


def arrow_array(v, valid, kind):
    if kind == "ts":
        return pa.array(v.astype("datetime64[ns]"), mask=~valid)
    return pa.array(v, mask=~valid)


def arrow_sort_indices(cols, descending):
    names = [f"c{k}" for k in range(len(cols))]
    table = pa.table({nm: arrow_array(*c) for nm, c in zip(names, cols)})
    keys = [(nm, "descending" if d else "ascending") for nm, d in zip(names, descending)]
    got = pc.sort_indices(table, sort_keys=keys).to_numpy()
    batches = table.to_batches()
    if batches:  # (an empty table has no batch)
        again = pc.sort_indices(batches[0], sort_keys=keys).to_numpy()
        assert np.array_equal(got, again), "Table and RecordBatch answers differ"
    return got.astype(np.int64)


def main():
    out, manifest = {}, {"arrow": pa.__version__, "cases": []}
    for name, cols, desc in R.golden_cases():
        got = arrow_sort_indices(cols, desc)
        manifest["cases"].append({"name": name, "n": int(len(got)), "inputs": R.case_digest(cols, desc), "answer": R.digest(got),
                                  "kinds": [c[2] for c in cols], "descending": [bool(d) for d in desc]})
        if len(got) <= R.FULL_OUTPUT_MAX_N:
            out[name + "/indices"] = got.astype(np.uint16 if len(got) <= 65536 else np.uint32)
    out["manifest"] = np.array(json.dumps(manifest))
    path = os.path.join(ROOT, "tests", "golden", "multisort_golden.npz")
    np.savez_compressed(path, **out)
    print(f"{len(manifest['cases'])} cases -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
