#!/usr/bin/env python3
"""Timings of pdx_select_k under the forced `select` plan beside the path it replaces and beside one read of the same bytes, in the same
process, on float64 rows and their int32 twin:
  select_k        k in 10, 1e3, 1e5, 1e6, 1e7, 5e7 (k largest), PDX_SELECT_K_PLAN=select
  replaced path   pdx_argsort (int32: pdx_sort_indices) + pdx_take of all values + pdx_take of all index labels -- what n_largest cost before
  sort plan       pdx_select_k with PDX_SELECT_K_PLAN=sort, k = 10 (the full sort + the copy of k indices, without the two takes)
  floor           pdx_aggregate(SUM): one read of the column
HIP events around each call, median / min / max of 5 after 2 warm-up calls.  Not a test: nothing asserts on these numbers.
Usage: python tools/bench_topk.py [--rows 1e8] [--out profiles/bench_topk.jsonl]   (one JSON line per measurement)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pandasarrow_amd import _lib as L  # noqa: E402
from pandasarrow_amd import column as K  # noqa: E402


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms


def emit(what, dtype, n, ms, **extra):
    line = {"bench": what, "dtype": dtype, "rows": n, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    line.update(extra)
    text = json.dumps(line)
    print(text, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as fh:
            fh.write(text + "\n")
    return ms[len(ms) // 2]


def replaced_path(col, labels):
    """n_largest before pdx_select_k: the full stable sort, then values and index labels taken by all n indices"""
    idx = K.argsort(col, False) if col.dtype == L.FLOAT64 else K.sort_indices([col], [True])
    return K.take([col, labels], idx)


def main():
    L.check(L.load().pdx_init(0))
    n = int(ARGS.rows)
    g = torch.Generator(device="cuda").manual_seed(1)
    labels = K.Column(L.INT64, n, torch.arange(n, device="cuda", dtype=torch.int64))
    f64 = K.Column(L.FLOAT64, n, torch.randn((n,), generator=g, device="cuda", dtype=torch.float64))
    i32 = K.Column(L.INT32, n, torch.randint(-2**31, 2**31 - 1, (n,), generator=g, device="cuda", dtype=torch.int32))
    for name, col in (("float64", f64), ("int32", i32)):
        base = emit("aggregate sum (one read)", name, n, timed(lambda: K.aggregate(L.AGG_SUM, col)))
        os.environ.pop("PDX_SELECT_K_PLAN", None)
        old = emit("replaced path: full sort + 2 takes of n rows", name, n, timed(lambda: replaced_path(col, labels)), ratio_to_sum=None)
        os.environ["PDX_SELECT_K_PLAN"] = "sort"
        emit("select_k, plan=sort", name, n, timed(lambda: K.select_k(col, 10, False)), k=10, **{"plan_" + k: v for k, v in K.select_k_last_plan().items()})
        os.environ["PDX_SELECT_K_PLAN"] = "select"
        for k in (10, 1000, 100_000, 1_000_000, 10_000_000, 50_000_000):
            if not 0 < k < n:
                continue

            def top():
                idx = K.select_k(col, k, False)
                return K.take([col, labels], idx)

            ms = timed(lambda: K.select_k(col, k, False))
            plan = K.select_k_last_plan()
            emit("select_k, plan=select", name, n, ms, k=k, k_over_n=k / n, ratio_to_sum=ms[len(ms) // 2] / base, ratio_to_replaced=ms[len(ms) // 2] / old,
                 levels=int(plan["levels"]))
            ms = timed(top)
            emit("select_k + 2 takes of k rows", name, n, ms, k=k, k_over_n=k / n, ratio_to_replaced=ms[len(ms) // 2] / old)
        os.environ.pop("PDX_SELECT_K_PLAN", None)


if __name__ == "__main__":
    main()
