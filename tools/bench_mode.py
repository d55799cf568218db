#!/usr/bin/env python3
"""Timings of pdx_mode (n = 1 and n = 10) beside the two baselines of the same column in the same process: pdx_argsort / pdx_sort_indices
(the first step of the only route to a mode without pdx_mode) and pdx_aggregate(SUM) (one read of the same bytes: the floor); then
value_counts and GroupBy.mode at 1e6 groups beside pdx_groupby_quantile on the same handle; last, the counting path at value ranges of 4000
and 8000 (near its 8192-bin limit).
HIP events around each call, median / min / max of 5 after warm-up.  Not a test: nothing asserts on these numbers.
Usage: python tools/bench_mode.py [--rows 1e8] [--groups 1e6] [--out profiles/r10_bench_mode.jsonl]   (one JSON line per measurement)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--groups", type=float, default=1e6)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pandasarrow_amd import _lib as L  # noqa: E402
from pandasarrow_amd import column as K  # noqa: E402


def device_col(shape, n):
    g = torch.Generator(device="cuda").manual_seed(1)
    if shape == "int64 1e3 distinct":
        return K.Column(L.INT64, n, torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int64))
    if shape == "int64 1e6 distinct, full range":
        return K.Column(L.INT64, n, torch.randint(0, 1_000_000, (n,), generator=g, device="cuda", dtype=torch.int64) * -0x61C8864680B583EB)
    if shape == "float64 1e6 distinct":
        return K.Column(L.FLOAT64, n, torch.randint(0, 1_000_000, (n,), generator=g, device="cuda", dtype=torch.int64).to(torch.float64) * 0.37)
    if shape == "int32 1e3 distinct":
        return K.Column(L.INT32, n, torch.randint(-500, 500, (n,), generator=g, device="cuda", dtype=torch.int32))
    if shape == "int64 single value":
        return K.Column(L.INT64, n, torch.full((n,), 42, device="cuda", dtype=torch.int64))
    if shape == "int64 8000 distinct":
        return K.Column(L.INT64, n, torch.randint(0, 8000, (n,), generator=g, device="cuda", dtype=torch.int64))
    if shape == "int64 4000 distinct":
        return K.Column(L.INT64, n, torch.randint(0, 4000, (n,), generator=g, device="cuda", dtype=torch.int64))
    raise ValueError(shape)


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


def emit(what, n, ms, **extra):
    line = {"bench": what, "rows": n, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    line.update(extra)
    text = json.dumps(line)
    print(text, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as fh:
            fh.write(text + "\n")
    return ms[len(ms) // 2]


def column_shapes(n, shapes):
    for shape in shapes:
        col = device_col(shape, n)
        extra = {"shape": shape}
        base = emit("aggregate sum", n, timed(lambda: K.aggregate(L.AGG_SUM, col)), **extra)
        for want in (1, 10):
            ms = timed(lambda: K.mode(col, want))
            emit(f"mode n={want}", n, ms, path=K.mode_last_plan().get("path"), ratio_to_sum=ms[len(ms) // 2] / base, **extra)
        sort = (lambda: K.sort_indices([col])) if col.dtype == L.INT32 else (lambda: K.argsort(col))
        emit("sort indices of the column", n, timed(sort), **extra)
        del col
        L.load().pdx_trim_pool()


def main():
    L.check(L.load().pdx_init(0))
    n = int(ARGS.rows)
    column_shapes(n, ("int64 1e3 distinct", "int64 1e6 distinct, full range", "float64 1e6 distinct", "int32 1e3 distinct", "int64 single value"))
    G = int(ARGS.groups)
    keys, vals = K.synth_keys(0, n, G), K.synth_vals(0, n)
    codes = K.Column(L.INT64, n, torch.randint(0, 50, (n,), generator=torch.Generator(device="cuda").manual_seed(2), device="cuda", dtype=torch.int64))
    emit(f"value_counts, {G} distinct", n, timed(lambda: K.value_counts(keys)))
    gb = K.GroupByHandle.create(keys)
    emit(f"groupby sizes, {G} groups", n, timed(lambda: gb.sizes()))
    emit(f"groupby mode of 50 codes, {G} groups", n, timed(lambda: gb.mode(codes)))
    emit(f"groupby mode of float64 values, {G} groups", n, timed(lambda: gb.mode(vals)))
    emit(f"groupby quantile of float64 values, {G} groups (same handle)", n, timed(lambda: gb.quantile(vals, [0.5])))
    del gb, keys, vals, codes
    L.load().pdx_trim_pool()
    torch.cuda.empty_cache()
    column_shapes(n, ("int64 4000 distinct", "int64 8000 distinct"))


if __name__ == "__main__":
    main()
