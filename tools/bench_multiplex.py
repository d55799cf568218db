#!/usr/bin/env python3
"""Timings of pdx_coalesce, pdx_clip, drop_na (pdx_all_valid_mask + pdx_filter), pdx_replace_with_mask and pdx_indices_nonzero, each beside
two baselines measured in the same process:
  * the chain of calls that computed the same result before these entry points existed:
      coalesce : C - 1 pdx_if_else, each on the validity bitmap of a column handed over as a BOOL column (a zero-copy alias the ABI
                 itself cannot make, so the chain is priced without the pass that would build it)
      clip     : pdx_compare + pdx_if_else for the upper bound, the same for the lower one
      drop_na  : C - 1 pdx_logical ANDs over the bitmaps as BOOL columns, then pdx_filter
  * pdx_aggregate(SUM) over one column holding the same number of input bytes: the rate at which the library streams them
and one pdx_binary add over two columns, the element-wise rate the new kernels are expected to come near.
HIP events around each call, median / min / max of 5 after warm-up; bytes are the algorithmic ones, computed from the shapes.
Usage: python tools/bench_multiplex.py [--rows 1e8] [--out profiles/r09_bench_multiplex.jsonl]   (one JSON line per measurement)."""
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


def bitmap(n, g, rounds):
    """a validity bitmap whose nulls thin out with `rounds` (the AND of that many random bytes: 4 -> ~6 % nulls, 1 -> 50 %)"""
    acc = torch.full(((n + 7) // 8 + 16,), 255, device="cuda", dtype=torch.uint8)
    for _ in range(rounds):
        acc &= torch.randint(0, 256, acc.shape, generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    return ~acc


def device_cols(n, C, rounds=4, nulls=True):
    g = torch.Generator(device="cuda").manual_seed(1)
    return [K.Column(L.FLOAT64, n, torch.rand(n, generator=g, device="cuda", dtype=torch.float64) - 0.5, bitmap(n, g, rounds) if nulls else None) for _ in range(C)]


def as_flags(col):
    """the validity bitmap of `col` as a BOOL column without nulls"""
    return K.Column(L.BOOL, col.length, col.validity, None)


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


def stream(name, n_rows, med):
    """pdx_aggregate(SUM) over one float64 column of n_rows rows, and `med` relative to it"""
    g = torch.Generator(device="cuda").manual_seed(2)
    one = K.Column(L.FLOAT64, n_rows, torch.rand(n_rows, generator=g, device="cuda", dtype=torch.float64), None)
    s_med = emit(name + ": pdx_aggregate(SUM) over the same input bytes", n_rows, 1, timed(lambda: K.aggregate(L.AGG_SUM, one)), 8 * n_rows)
    emit(name + ": time relative to that stream", n_rows, 1, [med / s_med] * 3, 0)
    del one
    L.load().pdx_trim_pool()


def coalesce_chain(cols, flags):
    acc = cols[-1]
    for k in range(len(cols) - 2, -1, -1):
        acc = K.if_else(flags[k], cols[k], acc)
    return acc


def bench_coalesce(n, C, rounds, label):
    cols = device_cols(n, C, rounds)
    flags = [as_flags(c) for c in cols]
    med = emit(f"coalesce C={C}, {label}", n, C, timed(lambda: K.coalesce(cols)), 0)
    c_med = emit(f"coalesce C={C}, {label}: chain of C-1 pdx_if_else", n, C, timed(lambda: coalesce_chain(cols, flags)), 0)
    emit(f"coalesce C={C}, {label}: speedup over the chain", n, C, [c_med / med] * 3, 0)
    del cols, flags
    L.load().pdx_trim_pool()
    stream(f"coalesce C={C}, {label} (one column)", n, med)


def bench_clip(n):
    (x,) = device_cols(n, 1)
    lo, hi = K.Column.from_numpy([-0.25]), K.Column.from_numpy([0.25])
    med = emit("clip float64", n, 1, timed(lambda: K.clip(x, lo, hi)), 16 * n + n // 4)

    def chain():
        upper = K.if_else(K.compare(L.GT, x, 0.25), 0.25, x)
        return K.if_else(K.compare(L.LT, upper, -0.25), -0.25, upper)

    c_med = emit("clip float64: chain of 2 x (pdx_compare + pdx_if_else)", n, 1, timed(chain), 0)
    emit("clip float64: speedup over the chain", n, 1, [c_med / med] * 3, 0)
    y = device_cols(n, 1, nulls=False)[0]
    plain = K.Column(L.FLOAT64, n, x.values, None)
    b_med = emit("one pdx_binary add", n, 2, timed(lambda: K.binary(L.ADD, plain, y)), 24 * n)
    emit("clip float64: time relative to one pdx_binary add (16 B/row against 24)", n, 1, [med / b_med] * 3, 0)
    del x, y, plain
    L.load().pdx_trim_pool()
    stream("clip float64", n, med)


def bench_drop_na(n, C):
    cols = device_cols(n, C)
    flags = [as_flags(c) for c in cols]
    med = emit(f"drop_na C={C}, ~6 % nulls a column", n, C, timed(lambda: K.drop_na(cols)), 0)

    def chain():
        keep = flags[0]
        for f in flags[1:]:
            keep = K.logical(L.AND, keep, f)
        return K.filter(cols, keep, emit_null=False)

    c_med = emit(f"drop_na C={C}: chain of C-1 pdx_logical + pdx_filter", n, C, timed(chain), 0)
    emit(f"drop_na C={C}: speedup over the chain", n, C, [c_med / med] * 3, 0)
    keep = K.all_valid_mask(cols)
    f_med = emit(f"drop_na C={C}: pdx_filter alone, the mask given", n, C, timed(lambda: K.filter(cols, keep, emit_null=False)), 0)
    emit(f"drop_na C={C}: pdx_all_valid_mask alone", n, C, timed(lambda: K.all_valid_mask(cols)), C * n // 8 + n // 8)
    emit(f"drop_na C={C}: time relative to pdx_filter alone", n, C, [med / f_med] * 3, 0)
    del cols, flags, keep
    L.load().pdx_trim_pool()
    stream(f"drop_na C={C}", n * C, med)


def bench_replace_and_nonzero(n):
    a, repl = device_cols(n, 2)
    g = torch.Generator(device="cuda").manual_seed(3)
    mask = K.Column(L.BOOL, n, bitmap(n, g, 1), None)  # half the rows are replaced
    med = emit("replace_with_mask float64, half the rows", n, 1, timed(lambda: K.replace_with_mask(a, mask, repl)), 0)
    nz = emit("indices_nonzero float64", n, 1, timed(lambda: K.indices_nonzero(a)), 0)
    del a, repl, mask
    L.load().pdx_trim_pool()
    stream("replace_with_mask float64 (its array)", n, med)
    stream("indices_nonzero float64", n, nz)


def main():
    L.check(L.load().pdx_init(0))
    n = int(ARGS.rows)
    bench_coalesce(n, 4, 4, "~6 % nulls a column")
    bench_coalesce(n, 4, 1, "50 % nulls a column")
    bench_clip(n)
    bench_drop_na(n, 4)
    bench_replace_and_nonzero(n)


if __name__ == "__main__":
    main()
