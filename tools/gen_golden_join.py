#!/usr/bin/env python3
"""Generate tests/golden/join_golden.npz -- golden vectors for pdx_join_create / pdx_join_indices.

TEST INFRASTRUCTURE (same conventions as tools/gen_golden_scan.py).  For every case it records
  * the inputs: two key columns of one dtype (int64, uint64, timestamp[ns], int32) with their validity,
  * per join kind the ORDERED output of the numpy restatement tests/_join_ref.py (left index, left valid, right index, right valid),
  * where pyarrow imports, the multiset of (left row, right row) pairs of Arrow's own hash join (pyarrow.Table.join, Arrow C++ 25), taken
    by carrying a row-number column through it on each side and sorting the pairs (-1 = null).  Arrow's row order is unspecified, so
    only the multiset is comparable: it pins the null rule (a null key matches nothing) and the handling of duplicates on both sides.
tests/test_join_golden.py holds the restatement against this file; tests/test_gpu_join.py holds the kernels against both.

Run:  python tools/gen_golden_join.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _join_ref import HOWS, NP_KEY, join_ref, pair_multiset  # noqa: E402

try:
    import pyarrow as pa
except ImportError:  # the restatement alone is frozen
    pa = None

OUT = os.path.join(ROOT, "tests", "golden", "join_golden.npz")
ARROW_HOW = {"inner": "inner", "left": "left outer", "outer": "full outer", "semi": "left semi", "anti": "left anti"}
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def arrow_pairs(dtype, lk, lv, rk, rv, how):
    t = {"i64": pa.int64(), "u64": pa.uint64(), "ts": pa.timestamp("ns"), "i32": pa.int32()}[dtype]

    def table(k, v, row):
        col = pa.array(k, type=pa.int64() if dtype == "ts" else t, mask=~v)
        return pa.table({"k": col.cast(t), row: pa.array(np.arange(len(k), dtype=np.int64))})

    res = table(lk, lv, "lrow").join(table(rk, rv, "rrow"), keys="k", join_type=ARROW_HOW[how])
    a = np.array([-1 if x is None else x for x in res.column("lrow").to_pylist()], np.int64)
    if how in ("semi", "anti"):
        b = np.full(len(a), -1, np.int64)
    else:
        b = np.array([-1 if x is None else x for x in res.column("rrow").to_pylist()], np.int64)
    p = np.stack([a, b], axis=1) if len(a) else np.zeros((0, 2), np.int64)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def cases():
    rng = np.random.default_rng(20251020)
    out = []

    def add(name, dtype, lk, rk, lv=None, rv=None):
        dt = NP_KEY[dtype]
        lk, rk = np.asarray(lk, dt), np.asarray(rk, dt)
        lv = np.ones(len(lk), bool) if lv is None else np.asarray(lv, bool)
        rv = np.ones(len(rk), bool) if rv is None else np.asarray(rv, bool)
        out.append((name, dtype, lk, lv, rk, rv))

    # degenerate shapes
    add("both_empty", "i64", [], [])
    add("left_empty", "i64", [], [1, 2, 2])
    add("right_empty", "i64", [1, 2, 2], [])
    add("single_match", "i64", [7], [7])
    add("single_miss", "i64", [7], [8])
    add("disjoint", "i64", [1, 2, 3, 4], [5, 6, 7])
    add("left_all_null", "i64", [1, 2, 3], [1, 2, 3], lv=[0, 0, 0])
    add("right_all_null", "i64", [1, 2, 3], [1, 2, 3], rv=[0, 0, 0])
    add("null_meets_null", "i64", [5, 5, 9], [5, 5, 9], lv=[1, 0, 1], rv=[0, 1, 1])
    # key values: the group-by's reserved slot, the extremes of every dtype
    add("extremes_i64", "i64", [I64_MIN, 0, -1, I64_MAX, I64_MIN, 5], [I64_MAX, I64_MIN, -1, 0, 0, I64_MIN])
    add("extremes_u64", "u64", [0, 2**64 - 1, 2**63, 1, 2**64 - 1], [2**64 - 1, 0, 2**63, 2**63, 3])
    add("extremes_i32", "i32", [-2**31, 2**31 - 1, 0, -1, -2**31], [2**31 - 1, -1, -2**31, 7, -1])
    add("timestamps", "ts", [1_700_000_000_000_000_000, 0, -1, 1_700_000_000_000_000_000], [0, 1_700_000_000_000_000_000, 0, 42])
    # the OUTER tail: a right key that only null-key rows carry (row 1), one matched only by the last left row (key 9)
    add("outer_tail", "i64", [1, 2, 3, 9], [4, 6, 9, 1, 6, 8, 1], rv=[1, 0, 1, 1, 1, 1, 1])
    add("many_to_many", "i64", [3] * 7 + [1, 2], [3] * 5 + [2, 4])
    # random: duplicates on both sides, nulls on both sides, every dtype
    for i in range(24):
        dtype = ("i64", "u64", "ts", "i32")[i % 4]
        nl, nr = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        nk = int(rng.integers(1, 12))
        pool = {"i64": rng.integers(-2**62, 2**62, nk), "u64": rng.integers(0, 2**64, nk, dtype=np.uint64), "ts": rng.integers(0, 2**61, nk),
                "i32": rng.integers(-2**31, 2**31, nk)}[dtype]
        lk, rk = pool[rng.integers(0, nk, nl)], pool[rng.integers(0, nk, nr)]
        nulls = i % 3
        lv = rng.random(nl) > 0.2 if nulls in (1, 2) else None
        rv = rng.random(nr) > 0.2 if nulls == 2 else None
        add(f"random_{i:02d}_{dtype}", dtype, lk, rk, lv, rv)
    return out


def main():
    arrays, manifest = [], {"arrow": None if pa is None else pa.__version__, "cases": [], "arrays": {}}
    used = 0

    def put(name, a):
        nonlocal used
        a = np.ascontiguousarray(a)
        a = a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)
        manifest["arrays"][name] = [used, int(a.size)]
        arrays.append(a.ravel())
        used += int(a.size)

    for name, dtype, lk, lv, rk, rv in cases():
        manifest["cases"].append({"name": name, "dtype": dtype})
        put(f"{name}/lk", lk)
        put(f"{name}/lv", lv)
        put(f"{name}/rk", rk)
        put(f"{name}/rv", rv)
        for how in HOWS:
            li, lok, ri, rok = join_ref(lk, lv, rk, rv, how)
            put(f"{name}/{how}/li", li)
            put(f"{name}/{how}/lok", lok)
            if ri is not None:
                put(f"{name}/{how}/ri", ri)
                put(f"{name}/{how}/rok", rok)
            if pa is not None:
                put(f"{name}/{how}/arrow", arrow_pairs(dtype, lk, lv, rk, rv, how))
    blob = np.concatenate(arrays) if arrays else np.zeros(0, np.int64)
    np.savez_compressed(OUT, manifest=np.frombuffer(json.dumps(manifest).encode(), np.uint8), blob=blob)
    print(f"{OUT}: {len(manifest['cases'])} cases, {blob.size} values, {os.path.getsize(OUT)} bytes, arrow {manifest['arrow']}")


if __name__ == "__main__":
    main()
