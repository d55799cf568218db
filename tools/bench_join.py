#!/usr/bin/env python3
"""Timings of the hash join (pdx_join_create + pdx_join_indices) beside the only join the library could express before it, pdx_index_in +
pdx_cast + pdx_take (valid for a UNIQUE right key only), and beside one read of the left keys, pdx_aggregate(SUM), in the same process:
  unique   inner join of --rows left rows against --keys unique right keys (every left row matches once)
  dup4     the same against every right key four times (four output rows per left row)
  hot      one hot key at 5 % of the left rows against 64 right copies of it, the other left rows against unique keys
Each case is timed as create + indices (the handle is made, asked for its row count and destroyed inside the timed call; the outputs are
allocated outside it), then the two pdx_take calls that materialise one float64 column from each side, separately.  HIP events around each
call, median / min / max of 5 after 2 warm-up calls.  bytes_per_out_row is what the two index columns hold (16 B); GB/s is that over the
create + indices time.  Not a test: nothing asserts on these numbers.
Usage: python tools/bench_join.py [--rows 1e8] [--keys 1e6] [--out profiles/bench_join.jsonl]   (one JSON line per measurement)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--keys", type=float, default=1e6)
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


def emit(what, n, ms, **extra):
    line = {"bench": what, "rows": n, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    line.update(extra)
    text = json.dumps(line)
    print(text, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as fh:
            fh.write(text + "\n")
    return ms[len(ms) // 2]


def int_column(t):
    return K.Column(L.INT64, t.numel(), t)


def join_case(name, lkey, rkey, lval, rval, base):
    n = lkey.length
    probe = K.JoinHandle(lkey, rkey, "inner")
    rows, plan = probe.rows, probe.plan()
    probe.close()
    ol, orr = K.Column.empty(L.INT64, rows), K.Column.empty(L.INT64, rows)

    def run():
        h = K.JoinHandle(lkey, rkey, "inner")
        h.indices(ol, orr)
        h.close()

    ms = timed(run)
    med = emit(f"{name}: join create + indices", n, ms, out_rows=rows, bytes_per_out_row=16, out_gb_per_s=16e-6 * rows / ms[len(ms) // 2],
               ratio_to_sum=ms[len(ms) // 2] / base, **{k: v for k, v in plan.items() if k != "out_rows"})
    emit(f"{name}: take left value column", n, timed(lambda: K.take([lval], ol), reps=3, warm=1), out_rows=rows)
    emit(f"{name}: take right value column", n, timed(lambda: K.take([rval], orr), reps=3, warm=1), out_rows=rows)
    return med, ol, orr


def main():
    L.check(L.load().pdx_init(0))
    n, m = int(ARGS.rows), int(ARGS.keys)
    g = torch.Generator(device="cuda").manual_seed(1)
    spread = 2_654_435_761  # keys spread over a wide range: the group-by takes its hash path, as for keys of a real table
    uniq = torch.randperm(m, generator=g, device="cuda", dtype=torch.int64) * spread
    lkey = int_column(torch.randint(0, m, (n,), generator=g, device="cuda", dtype=torch.int64) * spread)
    lval = K.Column(L.FLOAT64, n, torch.rand((n,), generator=g, device="cuda", dtype=torch.float64))
    base = emit("aggregate sum of the left keys (one read)", n, timed(lambda: K.aggregate(L.AGG_SUM, lkey)))

    # ---- unique right keys, and the chain the join generalises
    rkey = int_column(uniq)
    rval = K.Column(L.FLOAT64, m, torch.rand((m,), generator=g, device="cuda", dtype=torch.float64))
    join_ms, ol, orr = join_case("unique", lkey, rkey, lval, rval, base)
    pos = [None]

    def chain():
        pos[0] = K.cast(K.index_in(lkey, rkey), L.INT64)

    chain_ms = emit("unique: chain index_in + cast", n, timed(chain), ratio_to_sum=None)
    emit("unique: chain take right value column", n, timed(lambda: K.take([rval], pos[0]), reps=3, warm=1))
    same = bool(torch.equal(pos[0].values[:n], orr.values[:n]))
    emit("unique: join / chain", n, [join_ms / chain_ms], same_right_indices=same)
    del ol, orr, pos

    # ---- every right key four times
    rkey4 = int_column(uniq.repeat(4)[torch.randperm(4 * m, generator=g, device="cuda")])
    rval4 = K.Column(L.FLOAT64, 4 * m, torch.rand((4 * m,), generator=g, device="cuda", dtype=torch.float64))
    join_case("dup4", lkey, rkey4, lval, rval4, base)
    del rkey4, rval4

    # ---- one hot key: 5 % of the left rows, 64 right copies
    hot = torch.tensor([-7], device="cuda", dtype=torch.int64)
    lhot = lkey.values.clone()
    lhot[torch.rand((n,), generator=g, device="cuda") < 0.05] = -7
    rhot = int_column(torch.cat([uniq, hot.repeat(64)]))
    rvalh = K.Column(L.FLOAT64, m + 64, torch.rand((m + 64,), generator=g, device="cuda", dtype=torch.float64))
    join_case("hot", int_column(lhot), rhot, lval, rvalh, base)


if __name__ == "__main__":
    main()
