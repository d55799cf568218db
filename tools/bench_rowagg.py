#!/usr/bin/env python3
"""Timings of pdx_row_aggregate (DataFrame::sum / min / std ... over axis = Columns), each beside two baselines measured in the same process:
  * the route a caller had before: a chain of C - 1 pdx_binary adds over the same columns (case 1 only; under nulls it computes something
    else, so it is a cost baseline, 24 (C - 1) B/row against 8 (C + 1))
  * pdx_aggregate(SUM) over ONE column of n x C rows: the rate at which the library streams the same input bytes
and one pdx_binary add alone, the rate k_binary_n reaches relative to that stream rate.
HIP events around each call, median / min / max of 5 after warm-up; bytes are the algorithmic ones, computed from the shapes.
Usage: python tools/bench_rowagg.py [--rows 1e8] [--wide-rows 1e7] [--out profiles/r08_bench_rowagg.jsonl]   (one JSON line per measurement)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--wide-rows", type=float, default=1e7)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pandasarrow_amd import _lib as L  # noqa: E402
from pandasarrow_amd import column as K  # noqa: E402


def device_cols(dt, n, C, nulls=False):
    g = torch.Generator(device="cuda").manual_seed(1)
    cols = []
    for _ in range(C):
        if dt == L.INT64:
            t = torch.randint(-2**62, 2**62, (n,), generator=g, device="cuda", dtype=torch.int64)
        else:
            t = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
        valid = None
        if nulls:  # the AND of four random bytes thins the nulls out to ~6 %
            acc = torch.full(((n + 7) // 8 + 16,), 255, device="cuda", dtype=torch.uint8)
            for _ in range(4):
                acc &= torch.randint(0, 256, acc.shape, generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
            valid = ~acc
        cols.append(K.Column(dt, n, t, valid))
    return cols


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


def emit(what, n, C, ms, nbytes, **extra):
    med = ms[len(ms) // 2]
    line = {"bench": what, "rows": n, "cols": C, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "bytes": nbytes, "GBps": nbytes / med / 1e6}
    line.update(extra)
    text = json.dumps(line)
    print(text, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as fh:
            fh.write(text + "\n")
    return med


def row_call(kind, cols, out, ddof=0):
    m = out.mut()
    L.check(L.load().pdx_row_aggregate(kind, K._col_array(cols), len(cols), 1, 0, ddof, m, K._stream()))


def add_chain(cols):
    acc = K.binary(L.ADD, cols[0], cols[1])
    for c in cols[2:]:
        acc = K.binary(L.ADD, acc, c)
    return acc


def stream_rate(dt, n, C):
    """pdx_aggregate(SUM) over one column of n x C rows"""
    (one,) = device_cols(dt, n * C, 1)
    ms = timed(lambda: K.aggregate(L.AGG_SUM, one))
    del one
    L.load().pdx_trim_pool()
    return ms


def case(name, kind, dt, n, C, nulls=False, ddof=0, chain=False, reads=1):
    cols = device_cols(dt, n, C, nulls)
    out = K.Column.empty(K.row_result_dtype(kind, dt), n, with_validity=kind not in (L.AGG_SUM,))
    vbytes = (C * n // 8) if nulls else 0
    nbytes = 8 * n * (reads * C + 1) + reads * vbytes + (0 if kind == L.AGG_SUM else n // 8)
    med = emit(name, n, C, timed(lambda: row_call(kind, cols, out, ddof)), nbytes, kind=kind, nulls=nulls)
    if chain:
        c_med = emit(name + ": chain of C-1 pdx_binary adds", n, C, timed(lambda: add_chain(cols)), 24 * n * (C - 1))
        emit(name + ": speedup over the add chain", n, C, [c_med / med] * 3, 0)
        b_med = emit("one pdx_binary add", n, 2, timed(lambda: K.binary(L.ADD, cols[0], cols[1])), 24 * n)
    del cols, out
    L.load().pdx_trim_pool()
    s_med = emit(name + ": pdx_aggregate(SUM) of one column of n x C rows", n * C, 1, stream_rate(dt, n, C), 8 * n * C)
    emit(name + ": time relative to that stream", n, C, [med / s_med] * 3, 0, bytes_ratio=nbytes / (8 * n * C))
    if chain:
        (two,) = device_cols(dt, 2 * n, 1)
        s2 = timed(lambda: K.aggregate(L.AGG_SUM, two))
        del two
        emit("one pdx_binary add: time relative to pdx_aggregate(SUM) of its 2 n input rows", n, 2, [b_med / s2[len(s2) // 2]] * 3, 0, bytes_ratio=1.5)


def main():
    L.check(L.load().pdx_init(0))
    n, wide = int(ARGS.rows), int(ARGS.wide_rows)
    case("1 float64 sum, C=8", L.AGG_SUM, L.FLOAT64, n, 8, chain=True)
    case("2 float64 sum, C=8, ~6 % nulls", L.AGG_SUM, L.FLOAT64, n, 8, nulls=True)
    case("3 int64 min, C=4", L.AGG_MIN, L.INT64, n, 4)
    case("4 float64 std, C=8", L.AGG_STDDEV, L.FLOAT64, n, 8, ddof=1, reads=2)
    case("5 float64 sum, C=64", L.AGG_SUM, L.FLOAT64, wide, 64)


if __name__ == "__main__":
    main()
