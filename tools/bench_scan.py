#!/usr/bin/env python3
"""Timings of the cumulative scans, fill_null and shift against pdx_unary(NEGATE) on the same column in the same process (NEGATE streams
the same algorithmic bytes: one read + one write of the values).  HIP events around each call, median / min / max of 5 after warm-up.
The library reads PDX_SCAN_CHUNK_ROWS once, so one process measures one variant: run it once as is (the plain three-phase form, the
default) and once with --chunk-rows 8388608 (chunks of 64 MiB of 8-byte input); every line carries the variant's chunk rows.
Usage: python tools/bench_scan.py [--rows 1e9] [--chunk-rows N] [--out profiles/r06_bench_scan.jsonl]   (one JSON line per op)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e9)
ap.add_argument("--chunk-rows", type=int, default=None)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
if ARGS.chunk_rows is not None:
    os.environ["PDX_SCAN_CHUNK_ROWS"] = str(ARGS.chunk_rows)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

import torch  # noqa: E402

from pandasarrow_amd import _lib as L  # noqa: E402
from pandasarrow_amd import column as K  # noqa: E402

TORCH = {L.INT32: torch.int32, L.FLOAT32: torch.float32, L.INT64: torch.int64, L.FLOAT64: torch.float64}
NAME = {L.INT32: "int32", L.FLOAT32: "float32", L.INT64: "int64", L.FLOAT64: "float64"}
VARIANT = "chunk_rows=" + (os.environ.get("PDX_SCAN_CHUNK_ROWS") or "0") + (" (plain)" if int(os.environ.get("PDX_SCAN_CHUNK_ROWS") or 0) <= 0 else "")


def device_col(dt, n, null_frac=0.0):
    g = torch.Generator(device="cuda").manual_seed(1)
    if dt in (L.FLOAT32, L.FLOAT64):
        t = torch.randn(n, generator=g, device="cuda", dtype=TORCH[dt])
    else:
        t = torch.randint(-1000, 1000, (n,), generator=g, device="cuda", dtype=TORCH[dt])
    valid = None
    if null_frac:
        valid = torch.randint(0, 256, ((n + 7) // 8 + 16,), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        if null_frac < 0.5:  # AND of bytes thins the nulls out: 4 draws ~ 6 % nulls
            valid = ~valid
            for _ in range(3):
                valid &= torch.randint(0, 256, valid.shape, generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
            valid = ~valid
    return K.Column(dt, n, t, valid)


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


def emit(op, n, width, ms, extra=None):
    line = {"op": op, "variant": VARIANT, "rows": n, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1],
            "algo_GB/s": 2 * width * n / (ms[len(ms) // 2] * 1e-3) / 1e9}
    line.update(extra or {})
    text = json.dumps(line)
    print(text, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as fh:
            fh.write(text + "\n")
    return line


def main():
    lib = L.load()
    L.check(lib.pdx_init(0))
    st = K._stream()
    for n in (int(ARGS.rows), 1_000_000):
        for dt, null_frac in ((L.INT64, 0), (L.FLOAT64, 0), (L.INT32, 0), (L.FLOAT32, 0), (L.FLOAT64, 0.05), (L.FLOAT64, 0.5)):
            w = 4 if dt in (L.INT32, L.FLOAT32) else 8
            a = device_col(dt, n, null_frac)
            out = K.Column.empty(dt, n, with_validity=null_frac > 0)
            ca, m = a.c(), out.mut()
            tag = NAME[dt] + (f"_nulls{null_frac}" if null_frac else "")
            neg = timed(lambda: L.check(lib.pdx_unary(L.NEGATE, C.byref(ca), C.byref(m), st)))
            emit(f"negate_{tag}", n, w, neg)
            limit = 1.5 * neg[len(neg) // 2] + (neg[-1] - neg[0])
            ops = []
            if null_frac == 0:
                ops.append(("cumsum", lambda: L.check(lib.pdx_cumulative(L.CUM_SUM, C.byref(ca), 0.0, 1, C.byref(m), st))))
                if dt == L.FLOAT64:
                    ops.append(("cummax", lambda: L.check(lib.pdx_cumulative(L.CUM_MAX, C.byref(ca), 0.0, 1, C.byref(m), st))))
                    ops.append(("shift", None))
            else:
                if null_frac < 0.5:
                    ops.append(("cumsum_skip", lambda: L.check(lib.pdx_cumulative(L.CUM_SUM, C.byref(ca), 0.0, 1, C.byref(m), st))))
                    ops.append(("cumsum_noskip", lambda: L.check(lib.pdx_cumulative(L.CUM_SUM, C.byref(ca), 0.0, 0, C.byref(m), st))))
                ops.append(("ffill", lambda: L.check(lib.pdx_fill_null(0, C.byref(ca), C.byref(m), st))))
            for name, fn in ops:
                if name == "shift":  # its output needs a bitmap (the vacated row is null): allocate it once, outside the timing
                    so = K.Column.empty(dt, n, with_validity=True)
                    sm = so.mut()
                    fn = lambda: L.check(lib.pdx_shift(C.byref(ca), 1, None, C.byref(sm), st))  # noqa: E731
                ms = timed(fn)
                emit(f"{name}_{tag}", n, w, ms, {"limit_ms_1.5x_negate_plus_spread": limit, "within_limit": ms[len(ms) // 2] <= limit})
            del a, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
