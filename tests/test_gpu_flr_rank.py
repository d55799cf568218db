"""The dense fused last-digit reduce (k_flr_reduce, plan reducer=flr_reduce_dense) on run shapes chosen for its ranking and its tile
loads: all ten 64-row steps of a wave's tile are ranked in one LDS exchange (wave_match_rank_batch), so what can go wrong depends on how
long a run is and how its rows' digits are spread over the lanes of a step; where a run starts and how close a full tile ends to the end
of the key array is what a key load wider than one byte would depend on (tried and dropped, DESIGN 24: the cases stay).

Geometry (derived from plan_fused / dense_build, and re-checked without a GPU by test_inputs_have_the_intended_runs):
  keys span [0, 2^17 - 2] with both ends present and n < 2^23 rows -> exact dense domain, slot = key, 2^17 slots = 17 slot bits;
  the top 6 bits are the fused digit (the group inside a run), the low 11 bits the run: 2048 runs, sorted by two narrowing passes
  (full plan 6+6+5, low plan 6+5: the first digits agree, so the pass-0 offsets of the create are usable) -> 1-byte digit keys.
  4 n + 1024 > 2^17 (the dense limit) needs n >= 32 512 rows.  The three PDX_FUSED_LAST_DIGIT_MIN_* switches lower the product
  thresholds (2^22 rows, 10 low bits, 1024 rows per run) exactly as tests/test_gpu_fuzz.py does; PDX_SORT_NARROW=0 keeps 4-byte slots
  (the uint32 key instantiation of the same kernel).
A run's rows keep their input order (the sort is stable), so a run's digit sequence is what the test writes down; tiles are 2560 rows
from the run's start, and row i of a run sits in lane i % 64 of step (i % 2560) // 64.
Everything is compared bit for bit with the oracle; no tolerances."""
import numpy as np
import pytest

import oracle as orc
from conftest import assert_f64_bits

SUM, MEAN, MIN, MAX, COUNT, VAR, STD = range(7)
SLOT_BITS, LOW_BITS = 17, 11
NRUNS = 1 << LOW_BITS
TILE = 2560
MIN_ROWS_DENSE = ((1 << SLOT_BITS) - 1024) // 4 + 1  # 4 n + 1024 > span of the keys


def _assemble(runs, seed):
    """runs: [(run index, digit sequence)] -> int64 keys; the rows of different runs are interleaved at random, every run's own rows stay
    in the order given.  Returns (keys, run index of every row)."""
    rng = np.random.default_rng(seed)
    runs = sorted(runs, key=lambda r: r[0])
    run_of_row = rng.permutation(np.repeat(np.array([r for r, _ in runs], np.int64), [len(d) for _, d in runs]))
    digits = np.empty(len(run_of_row), np.int64)
    digits[np.argsort(run_of_row, kind="stable")] = np.concatenate([np.asarray(d, np.int64) for _, d in runs])
    assert digits.min() >= 0 and digits.max() < 64
    return (digits << LOW_BITS) | run_of_row, run_of_row


def _shape_runs():
    rng = np.random.default_rng(2024)
    rnd = lambda n, groups=64: rng.integers(0, groups, n)
    runs = [(0, [0])]                                                   # one row (and the smallest key)
    runs += [(3, rnd(63)), (4, rnd(64)), (7, rnd(65))]                  # below / at / past one step
    runs += [(100, rnd(2559)), (101, rnd(2560)), (102, rnd(2561)), (500, rnd(5121))]  # ragged, full, full + 1 row, two full + 1 row
    runs += [(600, np.full(5121, 37)), (601, np.full(2561, 0))]         # one group holds every row: 64 lanes on one word in every step
    runs += [(700, np.tile([5, 58], 2561)[:5121])]                      # two groups alternating row by row
    runs += [(800, np.arange(2625) % 64), (801, 63 - np.arange(5121) % 64)]  # lane l holds digit l / digit 63 - l in every step
    runs += [(900, rnd(2600, 4))]                                       # four groups; group 1 gets the NaNs and infinities below
    runs += [(2046, np.concatenate([[63], rnd(69)]))]                   # (the largest key)
    return runs


def _shape_input():
    keys, run_of_row = _assemble(_shape_runs(), 5)
    n = len(keys)
    vals = orc.synth_vals(0, n) - 0.25
    # one group with NaNs of both signs, quiet and signalling, distinct payloads, and both infinities: the sum must hand on the bits
    # Arrow's x86 adds do (earlier NaN inside a leaf, later operand's at a merge, inf + -inf = the negative default NaN)
    g = np.flatnonzero(keys == ((1 << LOW_BITS) | 900))
    assert len(g) > 400
    rng = np.random.default_rng(9)
    pick = g[np.sort(rng.choice(len(g), 40, replace=False))]
    bits = (np.uint64(0x7FF0000000000000) | rng.integers(1, 1 << 51, 40).astype(np.uint64) | (rng.integers(0, 2, 40).astype(np.uint64) << np.uint64(51))
            | (rng.integers(0, 2, 40).astype(np.uint64) << np.uint64(63)))
    vals[pick] = bits.view(np.float64)
    vals[pick[5]], vals[pick[22]] = np.inf, -np.inf
    # a second group of the same run: infinities only (inf + -inf with no NaN operand)
    g2 = np.flatnonzero(keys == ((2 << LOW_BITS) | 900))
    vals[g2[3]], vals[g2[len(g2) // 2]] = -np.inf, np.inf
    return keys, vals


def _align_input(m):
    """a run of two full tiles + 1 row starting at a row index = m (mod 16), and a run of exactly one tile that ends t = m % 15 + 1 bytes
    before the end of the key array (behind it only the t rows of run 2047)"""
    rng = np.random.default_rng(100 + m)
    t = m % 15 + 1
    runs = [(0, np.concatenate([[0], rng.integers(0, 64, 31 + m)])), (1, rng.integers(0, 64, 2 * TILE + 1)), (1000, rng.integers(0, 64, 25000)),
            (2046, np.concatenate([[63], rng.integers(0, 64, TILE - 1)])), (2047, rng.integers(0, 63, t))]
    keys, _ = _assemble(runs, 200 + m)
    return keys, orc.synth_vals(m, len(keys)) - 0.25, t


def _run_table(keys):
    """(start, length) of every run in the sorted layout, from the keys alone"""
    lens = np.bincount(keys & (NRUNS - 1), minlength=NRUNS)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]), lens


def test_inputs_have_the_intended_runs():
    """no GPU: the inputs meet the preconditions the module docstring derives the plan from, and hold the run shapes they are meant to"""
    keys, vals = _shape_input()
    assert keys.min() == 0 and keys.max() == (1 << SLOT_BITS) - 2 and MIN_ROWS_DENSE <= len(keys) < (1 << 23)
    _, lens = _run_table(keys)
    assert set(lens[lens > 0]) >= {1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1} and (lens == 0).sum() > 2000
    for run, ngroups in ((600, 1), (601, 1), (700, 2), (800, 64), (801, 64)):
        assert len(np.unique(keys[(keys & (NRUNS - 1)) == run])) == ngroups
    d800 = keys[(keys & (NRUNS - 1)) == 800] >> LOW_BITS
    assert np.array_equal(d800, np.arange(len(d800)) % 64)
    assert np.isnan(vals).sum() == 38 and np.isinf(vals).sum() == 4
    seen_tail, seen_start = set(), set()
    for m in range(16):
        keys, _, t = _align_input(m)
        assert keys.min() == 0 and keys.max() == (1 << SLOT_BITS) - 2 and MIN_ROWS_DENSE <= len(keys) < (1 << 23)
        start, lens = _run_table(keys)
        assert start[1] % 16 == m and lens[1] == 2 * TILE + 1
        assert lens[2046] == TILE and len(keys) - (start[2046] + TILE) == t == lens[2047]
        seen_start.add(int(start[1] % 16))
        seen_tail.add(t)
    assert seen_start == set(range(16)) and seen_tail == set(range(1, 16))


@pytest.fixture(scope="module")
def px():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column

    L.check(L.load().pdx_init(0))

    class NS:
        pass

    ns = NS()
    ns.L, ns.K, ns.Column = L, column, column.Column
    return ns


@pytest.fixture(scope="module")
def shape_case():
    keys, vals = _shape_input()
    ids, uniq, _, _ = orc.group_ids(keys)
    ek, es, em, ec = orc.groupby_sum_mean_count(keys, vals)
    return dict(keys=keys, vals=vals, ids=ids, uniq=uniq, ek=ek, es=es, em=em, ec=ec)


def _fused_env(monkeypatch, narrow):
    monkeypatch.setenv("PDX_FUSED_LAST_DIGIT_MIN_ROWS", "0")
    monkeypatch.setenv("PDX_FUSED_LAST_DIGIT_MIN_LOW_BITS", "4")
    monkeypatch.setenv("PDX_FUSED_LAST_DIGIT_MIN_RUN", "0")
    if not narrow:
        monkeypatch.setenv("PDX_SORT_NARROW", "0")


def _profile(px, fn):
    import ctypes as C

    lib = px.L.load()
    px.L.check(lib.pdx_profile_reset())
    px.L.check(lib.pdx_profile_enable(1))
    try:
        res = fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        px.L.check(lib.pdx_profile_report(buf, 1 << 16))
        lib.pdx_profile_enable(0)
        lib.pdx_profile_reset()
    tags = {}
    for line in buf.value.decode().splitlines():
        tag, count, _ms = line.split()
        tags[tag] = int(count)
    return tags, res


def _assert_dense_fused(plan, narrow):
    assert plan["slots"] == "dense" and plan["layout"] == "fused" and plan["reducer"] == "flr_reduce_dense" and "side" not in plan, plan
    assert plan["sort"] == ("narrow:6+5" if narrow else "lsd:skip6"), plan


@pytest.mark.gpu
@pytest.mark.parametrize("narrow", [True, False], ids=["byte_keys", "slot_keys"])
def test_run_shapes_sum_mean_count(px, monkeypatch, shape_case, narrow):
    """runs of 1 / 63 / 64 / 65 / 2559 / 2560 / 2561 / 5121 rows between empty runs, one group per run, two alternating groups, lane = digit
    and its reverse, NaN payloads and infinities in one group: sum, mean and count of every key equal the oracle's bits"""
    _fused_env(monkeypatch, narrow)
    c = shape_case
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(c["keys"]))
    tags, (s, m, cnt) = _profile(px, lambda: gb.agg(px.Column.from_numpy(c["vals"]), [SUM, MEAN, COUNT]))
    _assert_dense_fused(gb.last_plan(), narrow)
    assert tags.get("fused_last_digit_reduce") == 1 and "seg_reduce" not in tags, tags
    assert np.array_equal(gb.unique_keys().to_numpy()[0], c["ek"])
    assert_f64_bits(s.to_numpy()[0], c["es"], what="sum")
    assert_f64_bits(m.to_numpy()[0], c["em"], what="mean")
    assert np.array_equal(cnt.to_numpy()[0], c["ec"])


@pytest.mark.gpu
@pytest.mark.parametrize("narrow", [True, False], ids=["byte_keys", "slot_keys"])
def test_run_shapes_variance(px, monkeypatch, shape_case, narrow):
    """variance and mean on the same input: the mean pass and the squared-deviation pass share the dense instantiation (three launches)"""
    _fused_env(monkeypatch, narrow)
    c = shape_case
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(c["keys"]))
    tags, outs = _profile(px, lambda: gb.agg(px.Column.from_numpy(c["vals"]), [VAR, MEAN]))
    _assert_dense_fused(gb.last_plan(), narrow)
    assert tags.get("fused_last_digit_reduce") == 3 and "seg_reduce" not in tags, tags
    assert np.array_equal(gb.unique_keys().to_numpy()[0], c["uniq"])
    for kind, out in zip([VAR, MEAN], outs):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, c["ids"], len(c["uniq"]), c["vals"], None, nthreads=4)
        assert ok is None or np.array_equal(ok, eok), kind
        assert_f64_bits(got, exp, valid=eok, what=f"kind={kind}")


@pytest.mark.gpu
def test_run_shapes_int64_mean_count(px, monkeypatch, shape_case):
    """int64 values, mean and count: the other value type of the dense instantiation"""
    _fused_env(monkeypatch, True)
    c = shape_case
    vals = np.random.default_rng(17).integers(-10**15, 10**15, len(c["keys"])).astype(np.int64)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(c["keys"]))
    outs = gb.agg(px.Column.from_numpy(vals), [MEAN, COUNT])
    _assert_dense_fused(gb.last_plan(), True)
    for kind, out in zip([MEAN, COUNT], outs):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, c["ids"], len(c["uniq"]), vals, None, nthreads=4)
        assert ok is None or np.array_equal(ok, eok), kind
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=f"kind={kind}")
        else:
            assert np.array_equal(got[eok], exp[eok]), kind


@pytest.mark.gpu
@pytest.mark.parametrize("m", range(16))
def test_run_start_alignment_and_array_end(px, monkeypatch, m):
    """a long run starting at a row index = m (mod 16) -- the misalignment of its tiles' key bytes -- and a full tile that ends
    m % 15 + 1 bytes before the end of the key array, where no load of a tile's keys may reach past it"""
    _fused_env(monkeypatch, True)
    keys, vals, _ = _align_input(m)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    s, mean, cnt = gb.agg(px.Column.from_numpy(vals), [SUM, MEAN, COUNT])
    _assert_dense_fused(gb.last_plan(), True)
    ek, es, em, ec = orc.groupby_sum_mean_count(keys, vals)
    assert np.array_equal(gb.unique_keys().to_numpy()[0], ek)
    assert_f64_bits(s.to_numpy()[0], es, what="sum")
    assert_f64_bits(mean.to_numpy()[0], em, what="mean")
    assert np.array_equal(cnt.to_numpy()[0], ec)
