#!/usr/bin/env python3
"""Timings of the 32-bit column paths against their 64-bit twins, measured in the same process (not the contract bench): achieved GB/s
against each op's ALGORITHMIC bytes.  add / greater at 1e9 rows, float32 sum, float64 add at an odd offset, int64 + float64 add, the
int64 -> float64 cast (checked and not), filter of 1e8 rows x 9 int32 columns, take.
Usage: python tools/bench_narrow.py [--scale 1.0]   (prints one JSON line per op)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from bench_ops import report, timeit  # noqa: E402

from pandasarrow_amd import _lib as L  # noqa: E402
from pandasarrow_amd import column as K  # noqa: E402

TORCH = {L.INT32: torch.int32, L.FLOAT32: torch.float32, L.INT64: torch.int64, L.FLOAT64: torch.float64}


def device_col(dt, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dt in (L.FLOAT32, L.FLOAT64):
        t = torch.randn(n, generator=g, device="cuda", dtype=TORCH[dt])
    else:
        t = torch.randint(-1000, 1000, (n,), generator=g, device="cuda", dtype=TORCH[dt])
    return K.Column(dt, n, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    sc = ap.parse_args().scale
    L.check(L.load().pdx_init(0))
    n = int(1e9 * sc)
    for wide, narrow in ((L.INT64, L.INT32), (L.FLOAT64, L.FLOAT32)):
        for dt in (narrow, wide):
            w = 4 if dt == narrow else 8
            a, b = device_col(dt, n, 1), device_col(dt, n, 2)
            out = K.Column.empty(dt, n)
            ca, cb, m = a.c(), b.c(), out.mut()
            st = K._stream()
            lib = L.load()
            report(f"add_{K._TORCH_DT[dt]}".replace("torch.", ""), n, 3 * w * n, timeit(lambda: L.check(lib.pdx_binary(L.ADD, ca, cb, 0, m, st)), reps=5))
            bo = K.Column.empty(L.BOOL, n)
            mb = bo.mut()
            report(f"greater_{K._TORCH_DT[dt]}".replace("torch.", ""), n, 2 * w * n + n / 8,
                   timeit(lambda: L.check(lib.pdx_compare(L.GT, ca, cb, 0, mb, st)), reps=5))
            if dt in (L.FLOAT32, L.FLOAT64):
                report(f"sum_{K._TORCH_DT[dt]}".replace("torch.", ""), n, w * n, timeit(lambda: K.aggregate(L.AGG_SUM, a), reps=5))
            del a, b, out, bo
            torch.cuda.empty_cache()
    # float64 add of two slices at an odd element offset (not 16-byte aligned: the row-per-lane loop), and a mixed int64 + float64 add
    # (Arrow's checked cast of the int64 operand)
    lib, st = L.load(), K._stream()
    a, b = device_col(L.FLOAT64, n + 1, 1), device_col(L.FLOAT64, n + 1, 2)
    sa, sb, out = K.Column(L.FLOAT64, n, a.values, None, 1), K.Column(L.FLOAT64, n, b.values, None, 1), K.Column.empty(L.FLOAT64, n)
    ca, cb, m = sa.c(), sb.c(), out.mut()
    report("add_float64_offset1", n, 24 * n, timeit(lambda: L.check(lib.pdx_binary(L.ADD, ca, cb, 0, m, st)), reps=5))
    del a, sa
    ia = device_col(L.INT64, n, 3)
    ca, cb = ia.c(), K.Column(L.FLOAT64, n, b.values).c()
    report("add_int64_float64", n, 24 * n, timeit(lambda: L.check(lib.pdx_binary(L.ADD, ca, cb, 0, m, st)), reps=5))
    # int64 -> float64 cast: Arrow's checked cast and the unchecked one of the frame mean (pdx_cast_f64, checked = 1 / 0)
    for checked in (1, 0):
        report(f"cast_f64_int64_checked{checked}", n, 16 * n, timeit(lambda: L.check(lib.pdx_cast_f64(ca, checked, m, st)), reps=5))
    del ia, b, sb, out
    torch.cuda.empty_cache()
    nf = int(1e8 * sc)
    mask = K.compare(L.GT, device_col(L.FLOAT64, nf, 9), 0.0, scalar=True)
    for dt in (L.INT32, L.INT64):
        w = 4 if dt == L.INT32 else 8
        cols = [device_col(dt, nf, 10 + c) for c in range(9)]
        sel = K.filter_count(mask)
        report(f"filter_9x{K._TORCH_DT[dt]}".replace("torch.", ""), nf, nf / 8 + 9 * w * (nf + sel), timeit(lambda: K.filter(cols, mask), reps=5))
        idx = K.Column(L.INT64, nf // 10, torch.randint(0, nf, (nf // 10,), device="cuda", dtype=torch.int64))
        m = idx.length
        report(f"take_9x{K._TORCH_DT[dt]}".replace("torch.", ""), m, 8 * m + 9 * 2 * w * m, timeit(lambda: K.take(cols, idx), reps=5))
        del cols, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
