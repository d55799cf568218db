"""GPU: value_counts / is_unique (pandasarrow_amd/column.py over pdx_groupby_create + pdx_groupby_unique_keys + pdx_groupby_sizes),
pdx_groupby_sizes and pdx_groupby_mode against tests/golden/mode_golden.npz (Arrow C++ 25) and the numpy restatement tests/_mode_ref.py.
Bit-exact.  No pyarrow."""
import ctypes as C

import numpy as np
import pytest

import _mode_ref as R

pytestmark = pytest.mark.gpu

GOLD = R.ModeGolden()


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column as K

    lib = L.load()
    L.check(lib.pdx_init(0))
    dts = {"i64": L.INT64, "u64": L.UINT64, "f64": L.FLOAT64, "i32": L.INT32, "f32": L.FLOAT32, "ts": L.TIMESTAMP_NS, "bool": L.BOOL}
    return type("Env", (), {"torch": torch, "L": L, "K": K, "api": api, "lib": lib, "dts": dts})


def column(env, a, valid, dt, offset=0):
    return env.K.Column.from_numpy(np.asarray(a), valid, dtype=env.dts[dt], offset=offset)


def check_value_counts(env, a, valid, dt, offset=0):
    a = np.asarray(a, R.NP_DTYPES[dt])
    col = column(env, a, valid, dt, offset)
    v, c = env.K.value_counts(col)
    got, got_ok = v.to_numpy()
    got_ok = np.ones(v.length, bool) if got_ok is None else got_ok
    want, want_ok, want_counts = R.value_counts(a, valid)
    assert v.dtype == env.dts[dt] and c.dtype == env.L.INT64
    assert np.array_equal(got_ok, want_ok), dt
    assert R.same_values(np.asarray(got)[got_ok].astype(want.dtype, copy=False), want[want_ok]), dt
    assert np.array_equal(c.to_numpy()[0], want_counts), dt
    assert env.K.is_unique(col) == R.is_unique(a, valid)


@pytest.mark.parametrize("dt", ["i64", "u64", "ts", "f64", "bool"])
def test_golden_value_counts(env, dt):
    cases = [c for c in GOLD.cases if c["kind"] == "value_counts" and c["dtype"] == dt]
    assert len(cases) >= 4
    for c in cases:
        a, valid = GOLD.inputs(c)
        want, want_ok, want_counts = GOLD.expected(c)
        v, cnt = env.K.value_counts(column(env, a, None if valid.all() else valid, dt))
        got, got_ok = v.to_numpy()
        got_ok = np.ones(v.length, bool) if got_ok is None else got_ok
        assert np.array_equal(got_ok, want_ok), c["name"]
        assert R.same_values(np.asarray(got)[got_ok].astype(want.dtype, copy=False), want[want_ok]), c["name"]
        assert np.array_equal(cnt.to_numpy()[0], want_counts), c["name"]


@pytest.mark.parametrize("dt", ["i64", "u64", "ts", "f64", "bool"])
@pytest.mark.parametrize("nulls", ["absent", "first", "middle"])
def test_value_counts_shapes(env, dt, nulls):
    rng = np.random.default_rng(21)
    n = 5000
    if dt == "f64":
        a = rng.choice(np.array([0.0, -0.0, 1.5, np.nan, -np.nan, np.inf, 2.5e300]), n)
    elif dt == "bool":
        a = rng.random(n) < 0.3
    elif dt == "u64":
        a = rng.integers(0, 40, n).astype(np.uint64) * np.uint64(2**58) + np.uint64(7)
    else:
        a = rng.integers(-20, 20, n).astype(np.int64) * (10**15 if dt == "ts" else 1)
    valid = None
    if nulls != "absent":
        valid = rng.random(n) > 0.1
        valid[0] = nulls == "middle"
        valid[1:40] = True
        valid[40] = False
    check_value_counts(env, a, valid, dt, offset=3 if nulls == "middle" else 0)


def test_value_counts_facade_and_is_unique(env):
    s = env.api.Series(np.array([5, 3, 5, 5, 9, 3], np.int64))
    df = s.value_counts()
    assert df.names == ["values", "counts"]
    assert df.cols[0].to_numpy()[0].tolist() == [5, 3, 9] and df.cols[1].to_numpy()[0].tolist() == [3, 2, 1]
    assert not s.is_unique()
    assert env.api.Series(np.array([5, 3, 9], np.int64)).is_unique()
    two_nulls = env.api.Series(column(env, np.arange(5), np.array([True, False, True, False, True]), "i64"))
    assert not two_nulls.is_unique()
    one_null = env.api.Series(column(env, np.arange(5), np.array([True, False, True, True, True]), "i64"))
    assert one_null.is_unique()
    assert env.api.Series(np.zeros(0, np.int64)).is_unique() and env.api.Series(np.zeros(0, np.int64)).value_counts().num_rows() == 0


@pytest.mark.parametrize("dt", ["i32", "f32"])
def test_value_counts_refuses_four_byte_columns(env, dt):
    col = column(env, np.array([1, 2, 2], R.NP_DTYPES[dt]), None, dt)
    for f in (env.K.value_counts, env.K.is_unique):
        with pytest.raises(env.L.PdxError) as e:
            f(col)
        assert e.value.status == env.L.NOT_IMPLEMENTED and {"i32": "int32", "f32": "float32"}[dt] in str(e.value)


def handle_sizes(env, h):
    ids = h.group_ids().cpu().numpy().view(np.uint32)
    sizes = h.sizes().to_numpy()[0]
    assert np.array_equal(sizes, np.bincount(ids, minlength=h.num_groups)), (h.num_groups, len(ids))
    assert sizes.sum() == h.num_rows
    return sizes


def test_groupby_sizes(env):
    rng = np.random.default_rng(31)
    n = 30_000
    valid = rng.random(n) > 0.05
    dense = env.K.GroupByHandle.create(column(env, rng.integers(0, 700, n).astype(np.int64), valid, "i64"))
    handle_sizes(env, dense)
    spread = env.K.GroupByHandle.create(column(env, rng.integers(0, 3000, n).astype(np.int64) * 6364136223846793005 + 1442695040888963407, valid, "i64", offset=5))
    handle_sizes(env, spread)
    # after a COUNT of a column without nulls the handle serves the sizes it already holds
    vals = column(env, rng.random(n), None, "f64")
    before = handle_sizes(env, spread)
    spread.agg(vals, [env.L.AGG_COUNT])
    assert np.array_equal(handle_sizes(env, spread), before)
    ts = np.sort(rng.integers(0, 3_600 * 10**9, n)).astype(np.int64) + 1_700_000_000 * 10**9
    res = env.K.GroupByHandle.resample(column(env, ts, None, "ts"), 60 * 10**9)
    handle_sizes(env, res)
    sorted_keys = env.K.GroupByHandle.create(column(env, np.sort(rng.integers(0, 900, n)).astype(np.int64), None, "i64"))
    handle_sizes(env, sorted_keys)


@pytest.mark.parametrize("keys", ["dense_700", "dense_300000", "spread_3000"])
def test_groupby_sizes_through_the_lds_count(env, keys):
    """above 2^20 rows a hash / dense handle counts its sizes through the LDS accumulators (no value column is read); the handle keeps
    them, and a later COUNT of a column without nulls must agree"""
    rng = np.random.default_rng(33)
    n = (1 << 20) + 4097
    k = rng.integers(0, int(keys.split("_")[1]), n).astype(np.int64)
    if keys.startswith("spread"):
        k = k * 6364136223846793005 + 1442695040888963407
    valid = rng.random(n) > 0.02 if keys == "dense_700" else None
    h = env.K.GroupByHandle.create(column(env, k, valid, "i64"))
    sizes = handle_sizes(env, h)
    assert np.array_equal(handle_sizes(env, h), sizes)  # (the second call copies what the handle holds)
    (cnt,) = h.agg(column(env, rng.random(n), None, "f64"), [env.L.AGG_COUNT])
    assert np.array_equal(cnt.to_numpy()[0], sizes)


def check_group_mode(env, keys, a, valid, dt, keys_valid=None, handle=None):
    a = np.asarray(a, R.NP_DTYPES[dt])
    h = handle or env.K.GroupByHandle.create(column(env, keys, keys_valid, "i64"))
    modes, counts = h.mode(column(env, a, valid, dt, offset=2))
    ids = h.group_ids().cpu().numpy().view(np.uint32).astype(np.int64)
    G = h.num_groups
    want, want_ok, want_counts = R.group_mode(ids, G, a, valid)
    got, got_ok = modes.to_numpy()
    assert modes.length == G and counts.length == G
    assert np.array_equal(got_ok, want_ok) and modes.null_count == int((~want_ok).sum()) and counts.null_count == 0
    assert np.array_equal(counts.to_numpy()[0], want_counts)
    got = np.asarray(got).astype(want.dtype, copy=False)
    assert R.same_values(got, want), dt  # (a null mode's value bytes are zero)
    return got, got_ok


@pytest.mark.parametrize("dt", ["f64", "i64", "u64"])
def test_golden_group_mode(env, dt):
    for c in (c for c in GOLD.cases if c["kind"] == "group" and c["dtype"] == dt):
        a, valid = GOLD.inputs(c)
        want, want_ok, want_counts = GOLD.expected(c)
        h = env.K.GroupByHandle.create(column(env, GOLD.keys(c), None, "i64"))
        modes, counts = h.mode(column(env, a, valid, dt))
        got, got_ok = modes.to_numpy()
        # both sides number the groups by first occurrence
        order_here = h.unique_keys().to_numpy()[0]
        order_gold = GOLD.keys(c)[np.sort(np.unique(GOLD.keys(c), return_index=True)[1])]
        assert np.array_equal(order_here, order_gold), c["name"]
        assert np.array_equal(got_ok, want_ok) and np.array_equal(counts.to_numpy()[0], want_counts), c["name"]
        assert R.same_values(np.asarray(got).astype(want.dtype, copy=False)[got_ok], want[want_ok]), c["name"]


@pytest.mark.parametrize("dt", ["f64", "i64", "u64"])
def test_group_mode_shapes(env, dt):
    rng = np.random.default_rng(41)

    def values(n):
        if dt == "f64":
            a = rng.integers(-4, 5, n) * 0.5
            a[rng.random(n) < 0.1] = np.nan
            a[rng.random(n) < 0.05] = -0.0
            return a
        if dt == "u64":
            return rng.integers(0, 6, n).astype(np.uint64) + np.uint64(2**63 - 3)
        return rng.integers(-3, 4, n).astype(np.int64) * 10**12

    for G, n in ((1, 700), (3, 900), (5000, 20_000)):
        keys = rng.integers(0, G, n).astype(np.int64) * 11 - 40
        check_group_mode(env, keys, values(n), rng.random(n) > 0.25, dt)
        check_group_mode(env, keys, values(n), None, dt)
    # one group of 10 000 rows among groups of 1 to 3 rows
    small = np.repeat(np.arange(1, 2001), rng.integers(1, 4, 2000))
    keys = np.concatenate([small[:1500], np.zeros(10_000, np.int64), small[1500:]])
    n = len(keys)
    a = values(n)
    a[2000:9000] = a[1999]  # a run of the big group longer than a sort tile
    check_group_mode(env, keys, a, rng.random(n) > 0.1, dt)
    # groups that are all null, all NaN; ties; a null key
    keys = np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 4, 4, 4, 4, 0], np.int64)
    if dt == "f64":
        a = np.array([np.nan, 1.0, 5.0, -np.nan, 2.0, 5.0, np.nan, 3.0, 4.0, 7.0, np.nan, 7.0, np.nan, 1.0])
    else:
        a = np.array([9, 1, 5, 9, 2, 5, 9, 3, 4, 7, 8, 7, 8, 1], R.NP_DTYPES[dt])
    valid = np.array([1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1], bool)
    got, ok = check_group_mode(env, keys, a, valid, dt, keys_valid=np.array([1] * 13 + [0], bool))
    assert ok.tolist() == [True, False, True, True, True]
    assert got[3] == 7  # a tie between 7 and 8 / NaN: the smaller value
    if dt == "f64":
        assert int(R.bits(got[:1])[0]) == 0x7FF8000000000000  # the all-NaN group: the canonical NaN


def test_group_mode_on_resample_handle(env):
    rng = np.random.default_rng(43)
    n = 8000
    ts = np.sort(rng.integers(0, 600 * 10**9, n)).astype(np.int64) + 1_700_000_000 * 10**9
    h = env.K.GroupByHandle.resample(column(env, ts, None, "ts"), 7 * 10**9)
    check_group_mode(env, None, rng.integers(0, 5, n).astype(np.int64), rng.random(n) > 0.3, "i64", handle=h)


def test_group_mode_refusals(env):
    L = env.L
    h = env.K.GroupByHandle.create(column(env, np.array([1, 1, 2], np.int64), None, "i64"))
    vals = column(env, np.array([4, 4, 5], np.int64), np.array([True, True, False]), "i64")

    lengths = []

    def call(values, modes, counts):
        cv, mm, mc = values.c(), modes.mut(), counts.mut()
        rc = env.lib.pdx_groupby_mode(h._h, C.byref(cv), C.byref(mm), C.byref(mc), env.K._stream())
        lengths.append((mm.length, mc.length))
        return rc, env.lib.pdx_last_error().decode() if rc != L.OK else ""

    E = env.K.Column.empty
    rc, msg = call(vals, E(L.INT64, 2), E(L.INT64, 2))  # group 2 has no valid value and the output has no validity buffer
    assert rc == L.INVALID and "validity" in msg and lengths[-1] == (0, 0)  # (the outputs come back empty)
    rc, msg = call(vals, E(L.INT64, 2, with_validity=True), E(L.INT64, 2))
    assert rc == L.OK, msg
    rc, msg = call(vals, E(L.FLOAT64, 2, with_validity=True), E(L.INT64, 2))
    assert rc == L.INVALID and "dtype" in msg
    rc, msg = call(vals, E(L.INT64, 1, with_validity=True), E(L.INT64, 2))
    assert rc == L.INVALID and "too small" in msg
    rc, msg = call(column(env, np.array([4, 4], np.int64), None, "i64"), E(L.INT64, 2, with_validity=True), E(L.INT64, 2))
    assert rc == L.INVALID and "differ in length" in msg
    for dt, name in (("i32", "int32"), ("f32", "float32"), ("bool", "bool"), ("ts", "timestamp[ns]")):
        v = column(env, np.array([1, 0, 1], R.NP_DTYPES[dt]), None, dt)
        rc, msg = call(v, E(env.dts[dt], 2, with_validity=True), E(L.INT64, 2))
        assert rc == L.NOT_IMPLEMENTED and name in msg, msg
    # the facade: GroupBy.mode of one name and of several
    df = env.api.DataFrame({"k": np.array([1, 1, 2, 2, 2], np.int64), "a": np.array([4, 4, 5, 6, 6], np.int64), "b": np.array([1.5, 2.5, 2.5, 2.5, 0.5])})
    gb = df.group_by("k")
    assert gb.mode("a").values().tolist() == [4, 6]
    both = gb.mode(["a", "b"])
    assert both.names == ["a", "b"] and both.cols[1].to_numpy()[0].tolist() == [1.5, 2.5]
