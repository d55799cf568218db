#!/usr/bin/env python3
"""Timings of the dt accessor's kernels against pdx_round_temporal(floor, day) on the same column in the same process: that kernel
streams 8 B read + 8 B written per row with one floor division, the traffic of a single int64 component.  HIP events around each call
into preallocated outputs, median / min / max of 5 after warm-up; every line carries the algorithmic bytes per row, the achieved rate
and its share of the yardstick's rate.
Usage: python tools/bench_temporal.py [--rows 1e9] [--out profiles/bench_temporal.jsonl]   (one JSON line per op)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e9)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C  # noqa: E402

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


def emit(op, n, bytes_per_row, ms, yard=None):
    med = ms[len(ms) // 2]
    line = {"op": op, "rows": n, "bytes_per_row": bytes_per_row, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1],
            "algo_GB/s": bytes_per_row * n / (med * 1e-3) / 1e9}
    if yard is not None:
        line["rate_vs_floor_day"] = line["algo_GB/s"] / yard["algo_GB/s"]
        line["time_vs_floor_day"] = med / yard["ms_median"]
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
        g = torch.Generator(device="cuda").manual_seed(1)
        # instants over 1970 .. 2100 at nanosecond resolution (every calendar branch, sub-second parts)
        ts = K.Column(L.TIMESTAMP_NS, n, torch.randint(0, 4102444800 * 10**9, (n,), generator=g, device="cuda", dtype=torch.int64))
        outs = [K.Column.empty(L.INT64, n) for _ in range(3)]
        ct = ts.c()
        m0 = outs[0].mut()
        m0.dtype = L.TIMESTAMP_NS
        yard = emit("floor_day", n, 16, timed(lambda: L.check(lib.pdx_round_temporal(0, C.byref(ct), 1, L.UNIT_DAY, 1, 0, C.byref(m0), st))))
        for name, comps in (("year", [L.TC_YEAR]), ("hour", [L.TC_HOUR]), ("iso_week", [L.TC_ISO_WEEK]),
                            ("year_month_day", [L.TC_YEAR, L.TC_MONTH, L.TC_DAY]), ("iso_calendar", [L.TC_ISO_YEAR, L.TC_ISO_WEEK, L.TC_ISO_DAY_OF_WEEK]),
                            ("list_year_month_hour", [L.TC_YEAR, L.TC_MONTH, L.TC_HOUR])):
            marr = K._mut_array(outs[:len(comps)])
            carr = (C.c_int * len(comps))(*comps)
            emit(name, n, 8 + 8 * len(comps), timed(lambda: L.check(lib.pdx_temporal_components(C.byref(ct), carr, len(comps), None, marr, st))), yard)
        b = K.Column(L.TIMESTAMP_NS, n, outs[1].values)  # (the year_month_day output: arbitrary bits are valid instants)
        cb, mo = b.c(), outs[2].mut()
        emit("days_between", n, 24, timed(lambda: L.check(lib.pdx_temporal_between(L.UNIT_DAY, C.byref(ct), C.byref(cb), C.byref(mo), st))), yard)
        mr = outs[0].mut()
        mr.dtype = L.TIMESTAMP_NS
        emit("round_nearest_day", n, 16, timed(lambda: L.check(lib.pdx_round_temporal(2, C.byref(ct), 1, L.UNIT_DAY, 1, 0, C.byref(mr), st))), yard)
        del ts, outs, b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
