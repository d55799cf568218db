#!/usr/bin/env python3
"""Timings of pdx_sort_indices (multi-key sort as range-compressed composite keys) on two shapes of --rows rows:
  (a) key 0 int64 with 1e4 distinct values, key 1 timestamp[ns] at second resolution over a day: one round expected;
  (b) two full-range int64 keys: two rounds expected;
against the only route the entry points offered before, a hand LSD chain
    p1 = argsort(k_last); g = take(k_first, p1); p2 = argsort(g); take(p1, p2)
and against one pdx_argsort of a single key of the same rows.  Exits non-zero when shape (a) is not faster than the hand chain; everything
else is reported.  HIP events around each call, median / min / max of 5 after warm-up; the stats and compose kernels are priced from the
library's own event pairs (pdx_profile_*) against the bytes they move.
Usage: python tools/bench_multisort.py [--rows 1e8] [--out profiles/bench_multisort.jsonl]   (one JSON line per measurement)."""
import argparse
import ctypes as C
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


def emit(what, n, ms, **extra):
    line = {"bench": what, "rows": n, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    line.update(extra)
    text = json.dumps(line)
    print(text, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as fh:
            fh.write(text + "\n")
    return ms[len(ms) // 2]


def hand_chain(k_first, k_last):
    """stable LSD by hand: sort by the last key, carry the first key along, sort by it, compose the two permutations"""
    p1 = K.argsort(k_last)
    (g,) = K.take([k_first], p1)
    p2 = K.argsort(g)
    (p,) = K.take([p1], p2)
    return p


def kernel_ms(fn):
    """{tag: (launches, ms)} of one call, from the library's event pairs"""
    lib = L.load()
    lib.pdx_profile_reset()
    lib.pdx_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.pdx_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    L.check(lib.pdx_profile_report(buf, len(buf)))
    return {t: (int(c), float(ms)) for t, c, ms in (ln.split() for ln in buf.value.decode().splitlines())}


def main():
    L.check(L.load().pdx_init(0))
    n = int(ARGS.rows)
    g = torch.Generator(device="cuda").manual_seed(1)
    day0 = 1_700_000_000 * 1_000_000_000

    def full_range():  # 64 random bits from two 32-bit draws
        hi = torch.randint(-2**31, 2**31, (n,), generator=g, device="cuda", dtype=torch.int64)
        return (hi << 32) | torch.randint(0, 2**32, (n,), generator=g, device="cuda", dtype=torch.int64)

    shapes = {
        "a: 1e4 symbols x seconds of a day": (
            K.Column(L.INT64, n, torch.randint(0, 10_000, (n,), generator=g, device="cuda", dtype=torch.int64)),
            K.Column(L.TIMESTAMP_NS, n, day0 + torch.randint(0, 86_400, (n,), generator=g, device="cuda", dtype=torch.int64) * 1_000_000_000), 1),
        "b: two full-range int64 keys": (
            K.Column(L.INT64, n, full_range()), K.Column(L.INT64, n, full_range()), 2),
    }
    failed = None
    for name, (k0, k1, want_rounds) in shapes.items():
        out, info = K.sort_indices([k0, k1], with_info=True)
        same = bool(torch.equal(out.values[:n], hand_chain(k0, k1).values[:n]))
        m_ms = emit(f"sort_indices ({name})", n, timed(lambda: K.sort_indices([k0, k1])), rounds=info[0], key_bits=info[1], passes=info[2],
                    rounds_expected=want_rounds, equals_hand_chain=same)
        h_ms = emit(f"hand LSD chain ({name})", n, timed(lambda: hand_chain(k0, k1)))
        a_ms = emit(f"one argsort of key 1 ({name})", n, timed(lambda: K.argsort(k1)))
        emit(f"ratios ({name})", n, [h_ms / m_ms] * 3, speedup_over_hand_chain=h_ms / m_ms, ratio_to_one_argsort=m_ms / a_ms)
        prof = kernel_ms(lambda: K.sort_indices([k0, k1]))
        for tag, bytes_per_row in (("sort_key_stats", 16), ("sort_compose", 16 + 12 + (8 if info[0] > 1 else 0))):
            if tag in prof:
                cnt, ms = prof[tag]
                # stats: both 8-byte keys read once.  compose: per launch the keys a round reads (both, at most) + 12 bytes written; rounds
                # after the first also read the 8-byte payload and gather.  Reported per launch against the larger figure: an upper bound.
                emit(f"kernel {tag} ({name})", n, [ms / cnt] * 3, launches=cnt, tb_per_s_upper_bound=bytes_per_row * n / (ms / cnt * 1e-3) / 1e12)
        if not same:
            failed = failed or f"{name}: pdx_sort_indices and the hand chain disagree"
        if name.startswith("a") and not m_ms < h_ms:
            failed = failed or f"shape (a): pdx_sort_indices took {m_ms:.2f} ms, the hand chain {h_ms:.2f} ms: it must be faster"
        del k0, k1, out
        L.load().pdx_trim_pool()
    if failed:
        raise SystemExit(failed)


if __name__ == "__main__":
    main()
