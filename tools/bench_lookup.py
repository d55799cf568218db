#!/usr/bin/env python3
"""Timings of the lookup calls beside the chain each one replaces and beside one read of the same bytes, pdx_aggregate(SUM), in the same process:
  is_in / index_in  at set sizes 16, 2048 (both plan=lds) and 1e6 (plan=global); the chain for 16 entries is 16 pdx_compare + 15 pdx_logical
  arg_extreme       1 column and 8 columns of that many rows in one call; the chain is pdx_aggregate(MIN) + pdx_compare + pdx_indices_nonzero
  index             the match in the first row, in the middle, absent; the chain is pdx_compare + pdx_indices_nonzero
HIP events around each call, median / min / max of 7 after 3 warm-up calls.  Not a test: nothing asserts on these numbers.
Usage: python tools/bench_lookup.py [--rows 1e8] [--out profiles/bench_lookup.jsonl]   (one JSON line per measurement)."""
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


def timed(fn, reps=7, warm=3):
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


def is_in_chain(col, entries):
    """what is_in costs without pdx_is_in: one compare per set entry, or-ed together"""
    acc = None
    for v in entries:
        eq = K.compare(L.EQ, col, int(v))
        acc = eq if acc is None else K.logical(L.OR, acc, eq)
    return acc


def argmin_chain(col):
    m, _ = K.aggregate(L.AGG_MIN, col)
    return K.indices_nonzero(K.compare(L.EQ, col, m))


def main():
    L.check(L.load().pdx_init(0))
    n = int(ARGS.rows)
    g = torch.Generator(device="cuda").manual_seed(1)
    span = 4_000_000
    col = K.Column(L.INT64, n, torch.randint(0, span, (n,), generator=g, device="cuda", dtype=torch.int64))
    base = emit("aggregate sum (one read)", n, timed(lambda: K.aggregate(L.AGG_SUM, col)))
    for m in (16, 2048, 1_000_000):
        s = K.Column(L.INT64, m, torch.randint(0, span, (m,), generator=g, device="cuda", dtype=torch.int64))
        for name, fn in (("is_in", K.is_in), ("index_in", K.index_in)):
            ms = timed(lambda: fn(col, s))
            emit(name, n, ms, ratio_to_sum=ms[len(ms) // 2] / base, **K.lookup_last_plan())
        if m == 16:
            entries = s.to_numpy()[0].tolist()
            ms = timed(lambda: is_in_chain(col, entries), reps=3, warm=1)
            emit("chain: 16 compare + 15 logical", n, ms, set_size=m, ratio_to_sum=ms[len(ms) // 2] / base)
    # ---- arg_extreme
    for is_max in (False, True):
        ms = timed(lambda: K.arg_extreme([col], is_max))
        emit("arg_extreme 1 column", n, ms, is_max=is_max, ratio_to_sum=ms[len(ms) // 2] / base)
    ms = timed(lambda: argmin_chain(col), reps=3, warm=1)
    emit("chain: aggregate min + compare + indices_nonzero", n, ms, ratio_to_sum=ms[len(ms) // 2] / base)
    fcol = K.Column(L.FLOAT64, n, torch.rand((n,), generator=g, device="cuda", dtype=torch.float64))
    ms = timed(lambda: K.arg_extreme([fcol], False))
    emit("arg_extreme 1 column float64", n, ms, ratio_to_sum=ms[len(ms) // 2] / base)
    cols = [col] + [K.Column(L.INT64, n, torch.randint(0, span, (n,), generator=g, device="cuda", dtype=torch.int64)) for _ in range(7)]
    ms = timed(lambda: K.arg_extreme(cols, False))
    emit("arg_extreme 8 columns, one call", n, ms, ratio_to_8_sums=ms[len(ms) // 2] / (8 * base))
    ms = timed(lambda: [K.arg_extreme([c], False) for c in cols])
    emit("arg_extreme 8 columns, 8 calls", n, ms, ratio_to_8_sums=ms[len(ms) // 2] / (8 * base))
    del cols, fcol
    # ---- index
    col.values[0], col.values[n // 2] = span + 1, span + 2
    for where, value in (("front", span + 1), ("middle", span + 2), ("absent", span + 3)):
        ms = timed(lambda: K.index(col, value))
        emit(f"index, match {where}", n, ms, row=K.index(col, value), ratio_to_sum=ms[len(ms) // 2] / base)
    ms = timed(lambda: K.indices_nonzero(K.compare(L.EQ, col, span + 2)), reps=3, warm=1)
    emit("chain: compare + indices_nonzero", n, ms, ratio_to_sum=ms[len(ms) // 2] / base)


if __name__ == "__main__":
    main()
