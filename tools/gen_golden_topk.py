"""Writes tests/golden/topk_golden.npz from pyarrow 25.0.0 (arrow::compute array_sort_indices): run once where pyarrow is installed.

    python tools/gen_golden_topk.py

Per case one column (values as bit images, so NaN payloads and signed zeros survive) and, per order, array_sort_indices(order)[:k] for k in
{0, 1, 2, numbers-1, numbers, numbers+1, numbers+nan, n-1, n, n+5}.  Those slices are prefixes of one another, so the file keeps the
longest (k = n + 5: all n indices) once per order and the list of k; tests/_topk_ref.py reads it back."""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _topk_ref as R  # noqa: E402

PA = {"i64": pa.int64(), "u64": pa.uint64(), "ts": pa.timestamp("ns"), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32()}
STORE = {"i64": pa.int64(), "u64": pa.uint64(), "ts": pa.int64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32()}


def to_arrow(a, valid, dt):
    arr = pa.array(np.ascontiguousarray(a), STORE[dt], mask=None if valid is None else ~np.asarray(valid, bool))
    return arr.view(PA[dt]) if dt == "ts" else arr


def special(dt):
    """values that are easy to get wrong, as an array of the dtype"""
    t = R.NP_DTYPES[dt]
    if dt in ("f64", "f32"):
        return np.array([1.0, np.nan, 0.0, -0.0, 5.0, -np.inf, np.inf, -2.5, 0.0, np.nan, -0.0, 5.0, 1e-30, -1e-30], t)
    if dt == "u64":
        return np.array([1, 2**63, 2**64 - 1, 0, 2**63 + 5, 5, 7, 2**63 - 1, 2**64 - 1, 0], np.uint64)
    if dt == "i32":
        return np.array([1, -2**31, 2**31 - 1, 0, -1, 5, 7, -5, 2**31 - 1, -2**31], np.int32)
    return np.array([1, -2**63, 2**63 - 1, 0, -1, 5, 7, -5, 2**40, 2**63 - 1, -2**63], np.int64)


def main():
    rng = np.random.default_rng(20261019)
    arrays, cases = {}, []

    def add(name, dt, a, valid):
        a = np.asarray(a, R.NP_DTYPES[dt])
        n = len(a)
        arr = to_arrow(a, valid, dt)
        numbers, nan, _ = R.counts(a, valid)
        ks = sorted({k for k in (0, 1, 2, numbers - 1, numbers, numbers + 1, numbers + nan, n - 1, n, n + 5) if k >= 0})
        arrays[name + "/a"] = R.bits(a)
        if valid is not None:
            arrays[name + "/a_ok"] = np.asarray(valid, bool)
        for order, key in (("ascending", "asc"), ("descending", "desc")):
            full = np.asarray(pc.array_sort_indices(arr, order=order).to_numpy(zero_copy_only=False), np.uint64)
            for k in ks:  # (every slice the case stands for is a prefix of the one that is stored)
                assert np.array_equal(np.asarray(pc.array_sort_indices(arr, order=order)[:k].to_numpy(zero_copy_only=False), np.uint64), full[:k])
            arrays[name + "/" + key] = full.astype(np.uint16 if n < 65536 else np.uint64)
        cases.append({"name": name, "dtype": dt, "rows": n, "numbers": numbers, "nan": nan, "ks": ks})

    for dt in R.TOPK_DTYPES:
        t = R.NP_DTYPES[dt]
        sp = special(dt)
        add(f"{dt}/empty", dt, sp[:0], None)
        add(f"{dt}/one", dt, sp[:1], None)
        add(f"{dt}/special", dt, sp, None)
        ok = np.ones(len(sp), bool)
        ok[[0, 3, len(sp) - 1]] = False
        add(f"{dt}/special_nulls", dt, sp, ok)
        add(f"{dt}/all_null", dt, sp, np.zeros(len(sp), bool))
        add(f"{dt}/all_equal", dt, np.full(37, sp[4], t), None)
        add(f"{dt}/all_equal_nulls", dt, np.full(70, sp[4], t), rng.random(70) > 0.3)
        if dt in ("f64", "f32"):
            add(f"{dt}/all_nan", dt, np.full(9, np.nan, t), None)
            add(f"{dt}/zeros_both_signs", dt, np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0, -0.0, 0.0], t), None)
            add(f"{dt}/nan_and_null", dt, np.array([np.nan, 5, np.nan, 1, 5], t), np.array([1, 0, 1, 1, 1], bool))
        for n in (2, 63, 65, 130, 300):
            pool = np.concatenate([sp, rng.integers(0, 12, 30).astype(t)])  # a small range: many ties
            a = pool[rng.integers(0, len(pool), n)]
            add(f"{dt}/fuzz_ties_{n}", dt, a, rng.random(n) > 0.25)
            add(f"{dt}/fuzz_ties_{n}_no_validity", dt, a, None)
        if dt in ("f64", "f32"):
            add(f"{dt}/fuzz_wide_300", dt, (rng.standard_normal(300) * 1e3).astype(t), rng.random(300) > 0.1)
        else:
            info = np.iinfo(t)
            add(f"{dt}/fuzz_wide_300", dt, rng.integers(info.min, info.max, 300, dtype=t, endpoint=True), rng.random(300) > 0.1)

    arrays["manifest"] = np.array(json.dumps({"arrow": pa.__version__, "cases": cases}))
    out = os.path.join(ROOT, "tests", "golden", "topk_golden.npz")
    np.savez_compressed(out, **arrays)
    print(f"{len(cases)} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
