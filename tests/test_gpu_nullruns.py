"""GPU: pdx_aggregate sum / mean / min / max / count of nullable columns with STRUCTURED nulls (tests/_nullruns.py) against Arrow C++ 25
(tests/golden/nullruns_golden.npz) and the CPU oracle, bit for bit, at sizes on both sides of every launch boundary of sum_nullable
(aggregate.hip): the two segment scans' second block (n > 2,097,152), the emit waves' second round (n > 3,145,728), the state kernel's
second grid-stride round (n > 33,554,432) -- and the group-by / resample callers that hand groups of more than 2^22 nullable rows to the
same kernels.  Every null row, the rows in front of the slice and 130 rows behind it hold poison (NaN / 1e300 / INT_MIN / INT_MAX) with
the surrounding validity bits set: a validity bit read one row off, or a row read outside the slice, shows in the result.  The golden
recipes are chosen (oracle/gen_golden_nullruns.py) so that a sum over a wrong leaf grid has other bits than the right one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _nullruns as NR
import oracle as orc
from conftest import ROOT, Golden, assert_f64_bits

pytestmark = pytest.mark.gpu

GOLD = Golden("nullruns_golden.npz")
M = GOLD.manifest
Z = {k: GOLD.z[k] for k in ("family", "pattern", "n", "dtype", "seed", "poison", "count", "isnull", "exp")}
OFFSETS = (0, 1, 7, 63, 64, 65, 128, 1027)
MISALIGNED = [(off, mis) for off in (0, 64) for mis in (1, 3, 7)]  # validity pointer that many bytes past an 8-byte boundary


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column as K

    L.check(L.load().pdx_init(0))
    return L, K, torch


def recipe(i):
    return (M["patterns"][Z["pattern"][i]], int(Z["n"][i]), M["dtypes"][Z["dtype"][i]], int(Z["seed"][i]), int(Z["poison"][i]))


def aggregates(K, dtype, col):
    got = [K.aggregate(k, col) for k in NR.KINDS]
    res = [NR.encode(dtype, k, v) for k, (v, _) in zip(NR.KINDS, got)]
    return [r[0] for r in res], [r[1] for r in res], [c for _, c in got]


def check(i, got, oracle, what):
    """got == Arrow's golden == the oracle, in one assert: a disagreement names the side"""
    isnull, bits, counts = got
    gold = ([bool(x) for x in Z["isnull"][i]], [0 if nl else int(b) for nl, b in zip(Z["isnull"][i], Z["exp"][i])])
    orac = ([bool(x) for x in oracle[0]], [0 if nl else int(b) for nl, b in zip(oracle[0], oracle[1])])
    assert (isnull, bits) == gold == orac, f"{recipe(i)} {what}: gpu {bits} {isnull} / arrow {gold[1]} / oracle {orac[1]} (sum, mean, min, max, count)"
    assert counts == [int(Z["count"][i])] * 5, (recipe(i), what, counts)


def run_case(env, i, layouts):
    L, K, torch = env
    pattern, n, dtype, seed, kind = recipe(i)
    v, valid = NR.values(dtype, n, seed), NR.validity(pattern, n)
    oracle = NR.oracle_results(dtype, v, valid)
    for offset, mis in layouts:
        col = NR.column(K, L, torch, dtype, v, valid, offset, kind, mis)
        check(i, aggregates(K, dtype, col), oracle, f"offset={offset} misalign={mis}")
        if pattern == "all_valid_bitmap":  # a bitmap without a null (null_count unknown) == no bitmap
            dense = K.Column(col.dtype, n, col.values, None, offset, 0)
            check(i, aggregates(K, dtype, dense), oracle, f"dense offset={offset}")


def _ids(family, **want):
    return [i for i in GOLD.cases(family) if all(recipe(i)[{"n": 1, "dtype": 2}[k]] == x for k, x in want.items())]


def _param(i):
    p, n, dt, _, _ = recipe(i)
    return pytest.param(i, id=f"{p}-{n}-{dt}")


@pytest.mark.parametrize("dtype", NR.DTYPES)
@pytest.mark.parametrize("n", M["small_sizes"])
def test_small_every_pattern(env, n, dtype):
    """every pattern at every slice offset (the aligned-word fast path of the bitmap loads runs at 0, 64 and 128 only) and with the
    validity bytes off an 8-byte boundary"""
    ids = _ids("small", n=n, dtype=dtype)
    assert len(ids) + sum(1 for d in M["dropped"] if d[0] == "small" and d[2] == n and d[3] == dtype) == len(NR.PATTERNS) - len(NR.LARGE_ONLY)
    for i in ids:
        run_case(env, i, [(off, 0) for off in OFFSETS] + MISALIGNED)


def _large_layouts(i):
    return [(64, 0), (3, 0)] if i & 1 else [(0, 0), (65, 7)]


@pytest.mark.parametrize("i", [_param(i) for i in GOLD.cases("scan")])
def test_scan_boundary(env, i):
    """2048 segments: one block of the "latest" and leaf-count scans; 2052: two, the carry crosses the block aggregate"""
    run_case(env, i, _large_layouts(i))


@pytest.mark.parametrize("i", [_param(i) for i in GOLD.cases("pass")])
def test_whole_scan_block_of_pass(env, i):
    """6,300,007 rows with their nulls at the edges only: the carry set at row 5 arrives unchanged after 2048 or more "pass" segments"""
    run_case(env, i, _large_layouts(i))


@pytest.mark.parametrize("i", [_param(i) for i in GOLD.cases("emit")])
def test_emit_rounds(env, i):
    """3,145,728 rows: every emit wave takes exactly one segment; one row more: wave 0 prefetches and reduces a second one"""
    run_case(env, i, _large_layouts(i))


@pytest.mark.parametrize("i", [_param(i) for i in GOLD.cases("state")])
def test_state_kernel_second_round(env, i):
    """more tiles than the state kernel's capped grid holds: its waves take a second tile (134 MB of float32)"""
    run_case(env, i, [(64 * (i & 1), 0)])
    env[2].cuda.empty_cache()


def test_many_rounds_per_wave():
    """PDX_NULLSUM_WGS_PER_CU=1 (read once per process: a fresh child) shrinks the emit grid to 512 waves: 524,288 rows are one round,
    524,289 two, 3,150,855 seven -- the prefetched segment is consumed round after round.  (The child takes about 2.5 s, nearly all of it
    its start: the time limit of 30 s leaves room for the first import on a cold machine.  No retry; nothing else is started after a bad exit.)"""
    ids = GOLD.cases("child")
    assert len(ids) == 9
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_nullruns_child.py")] + [str(i) for i in ids], capture_output=True, text=True,
                       timeout=30, env=dict(os.environ, PDX_NULLSUM_WGS_PER_CU="1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert [x["i"] for x in lines] == ids
    for x in lines:
        i = x["i"]
        pattern, n, dtype, seed, _ = recipe(i)
        oracle = NR.oracle_results(dtype, NR.values(dtype, n, seed), NR.validity(pattern, n))
        check(i, ([bool(a) for a, _ in x["res"]], [int(b) for _, b in x["res"]], x["counts"]), oracle, "child, 1 workgroup per CU")


# ------------------------------------------------------------------ the callers that delegate to the same kernels
HUGE = 1 << 22  # gb_seg_reduce.hpp kHugeNullable: a nullable group of more rows goes through pdx_aggregate slice by slice
ALL_KINDS = [0, 1, 2, 3, 4]


def _compare_groups(outs, expected, what):
    for kind, out, (exp, eok) in zip(ALL_KINDS, outs, expected):
        got, ok = out.to_numpy()
        assert (ok is None and eok.all()) or np.array_equal(ok, eok), (what, kind)
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=f"{what} kind={kind}")
        else:
            assert np.array_equal(got[eok], exp[eok]), (what, kind, got, exp)


RUN_LENS = [1000, HUGE, HUGE + 4099]
_sorted_inputs = {}


def _sorted_case(pattern, dtype):
    """(values, validity, expected) of one sorted-key case, computed once for both of its offsets"""
    if (pattern, dtype) not in _sorted_inputs:
        _sorted_inputs.clear()  # (the two offsets of a case run back to back: one case is held at a time)
        n = sum(RUN_LENS)
        v, valid = NR.values(dtype, n, 3), NR.validity(pattern, n)
        ids = np.repeat(np.arange(3, dtype=np.uint32), RUN_LENS)
        _sorted_inputs[(pattern, dtype)] = (v, valid, [orc.groupby_agg(k, ids, 3, v, valid, nthreads=8) for k in ALL_KINDS])
    return _sorted_inputs[(pattern, dtype)]


@pytest.mark.parametrize("offset", [3, 64])  # (the topmost parameter varies fastest: the two offsets of a case run back to back)
@pytest.mark.parametrize("dtype", ["f64", "i64"])
@pytest.mark.parametrize("pattern", ["early_null", "period_1025", "null_segments", "random8"])
def test_sorted_key_runs(env, offset, pattern, dtype):
    """sorted keys: runs of 1000, 2^22 (the last size one wave still takes) and 2^22 + 4099 rows (reduce_huge_nullable_groups: the run is a
    slice of the caller's own values and bitmap at its own offset); the value column is itself a slice at offset 3 or at offset 64"""
    L, K, torch = env
    v, valid, expected = _sorted_case(pattern, dtype)
    gb = K.GroupByHandle.create(K.Column.from_numpy(np.repeat(np.arange(3, dtype=np.int64) * 10 + 5, RUN_LENS)))
    outs = gb.agg(NR.column(K, L, torch, dtype, v, valid, offset, kind=offset & 1), ALL_KINDS)
    assert gb.last_plan()["slots"] == "runs", gb.last_plan()
    _compare_groups(outs, expected, f"{pattern} {dtype} offset={offset}")
    gb.close()


@pytest.mark.parametrize("pattern", ["early_null", "period_1025", "null_segments", "random8"])
def test_resample_huge_bin(env, pattern):
    """one-minute bins of 3000, 2^22 + 4099 and 2500 rows: the middle bin goes through reduce_huge_nullable_groups"""
    L, K, torch = env
    lens = [3000, HUGE + 4099, 2500]
    minute = 60 * 10**9
    n = sum(lens)
    ts = 1_600_000_020 * 10**9 + np.repeat(np.arange(3, dtype=np.int64) * minute, lens) + np.arange(n, dtype=np.int64) % 2_000_000 * 1000
    ts = np.sort(ts)
    v, valid = NR.values("f64", n, 4), NR.validity(pattern, n)
    gb = K.GroupByHandle.resample(K.Column.from_numpy(ts, dtype=L.TIMESTAMP_NS), minute)
    assert gb.num_groups == 3
    outs = gb.agg(NR.column(K, L, torch, "f64", v, valid, 5, kind=1), ALL_KINDS)
    assert gb.last_plan()["slots"] == "bins", gb.last_plan()
    expected = [orc.resample_agg(k, ts, v, minute, valid=valid)[1:] for k in ALL_KINDS]
    _compare_groups(outs, expected, pattern)
    gb.close()


@pytest.mark.parametrize("pattern", ["early_null", "null_tiles"])
def test_hash_plan_hot_key(env, pattern):
    """the shape of test_groupby_huge_nullable_group -- one hot key with more than 2^22 of the rows -- with the pattern laid over
    the hot key's rows in row order: the validity of the grouped layout is rebuilt from the flag bit that travelled with the rows"""
    L, K, torch = env
    n = 6_500_003
    keys = orc.synth_keys(0, n, 50_000)
    keys[orc.synth_keys(7, n, 20) < 13] = 31337  # 65 % of the rows
    hot = np.flatnonzero(keys == 31337)
    assert len(hot) > HUGE
    valid = np.ones(n, bool)
    valid[hot] = NR.validity(pattern, len(hot))
    v = NR.values("f64", n, 5)
    gb = K.GroupByHandle.create(K.Column.from_numpy(keys))
    ids, uniq, _, _ = orc.group_ids(keys)
    outs = gb.agg(NR.column(K, L, torch, "f64", v, valid, 0, kind=0), ALL_KINDS)
    assert gb.last_plan()["slots"] not in ("runs", "bins"), gb.last_plan()
    expected = [orc.groupby_agg(k, ids, len(uniq), v, valid, nthreads=8) for k in ALL_KINDS]
    _compare_groups(outs, expected, pattern)
    gb.close()
