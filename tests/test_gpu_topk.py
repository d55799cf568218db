"""GPU: pdx_select_k / pdx_partition_nth through the C ABI (pandasarrow_amd/column.py) against tests/golden/topk_golden.npz (Arrow C++ 25) and
the numpy restatement tests/_topk_ref.py, which tests/test_topk_golden.py holds against that file.  Every comparison is exact equality of
index arrays.  No pyarrow."""
import ctypes as C

import numpy as np
import pytest

import _topk_ref as R

pytestmark = pytest.mark.gpu

GOLD = R.TopkGolden()
CHUNK = 65536  # rows of one workgroup of the counting / writing reads (pandasarrow_amd/csrc/select_k.hip, sk_grid) at these sizes
SIZES = [4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536 + 1, 300001]
PATTERN = 0x5A


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column as K

    lib = L.load()
    L.check(lib.pdx_init(0))
    dts = {"i64": L.INT64, "u64": L.UINT64, "f64": L.FLOAT64, "i32": L.INT32, "f32": L.FLOAT32, "ts": L.TIMESTAMP_NS}
    return type("Env", (), {"torch": torch, "L": L, "K": K, "api": api, "lib": lib, "dts": dts})


def column(env, a, valid, dt, offset=0):
    return env.K.Column.from_numpy(np.asarray(a, R.NP_DTYPES[dt]), valid, dtype=env.dts[dt], offset=offset)


def expected_plan(n, k, forced):
    if k == 0 or n == 0:
        return "empty"
    return "select" if forced == "select" and 0 < k < n else "sort"


def run_select_k(env, col, k, ascending, n, forced, what):
    got = env.K.select_k(col, k, ascending)
    plan = env.K.select_k_last_plan()
    assert plan["plan"] == expected_plan(n, k, forced) and plan["k"] == str(k) and plan["rows"] == str(n), (what, plan)
    assert got.dtype == env.L.UINT64 and got.length == min(k, n) and got.validity is None, what
    return got.to_numpy()[0][: got.length], plan


# ---------------------------------------------------------------- the golden file through the C ABI
@pytest.mark.parametrize("forced", ["select", "sort"])
@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("dt", R.TOPK_DTYPES)
def test_golden_through_the_abi(env, monkeypatch, dt, offset, forced):
    monkeypatch.setenv("PDX_SELECT_K_PLAN", forced)
    for c in (c for c in GOLD.cases if c["dtype"] == dt):
        a, valid = GOLD.column(c)
        col = column(env, a, valid, dt, offset)
        for ascending in (True, False):
            for k in c["ks"]:
                got, _ = run_select_k(env, col, k, ascending, c["rows"], forced, (c["name"], k))
                assert np.array_equal(got, GOLD.want(c, ascending, k)), (c["name"], k, ascending, offset, forced)


# ---------------------------------------------------------------- boundary shapes against the restatement
def three_values(n, k):
    """-> columns of {0, 1, 2} in which the k smallest are three 0s and k - 3 of the 1s (the tie group at the threshold).  The ties are spread
    from row 0 on, so the group spans every workgroup boundary in front of the place where the LAST tie that is needed sits: inside the
    second workgroup in one column, inside the last workgroup in the other.  Ten more ties follow, which must not be taken."""
    out = []
    zeros = np.unique([1, n // 2, n - 2])
    allowed = np.setdiff1d(np.arange(n), zeros)
    r = k - len(zeros)
    if r < 1:
        return out
    for name, e in (("second", min(CHUNK + 1000, n - 4)), ("last", n - 4)):
        e_idx = int(np.searchsorted(allowed, e))
        if r - 1 > e_idx:
            continue  # (more ties are needed than rows in front of that place)
        a = np.full(n, 2, np.int64)
        a[zeros] = 0
        a[allowed[np.linspace(0, e_idx, r).astype(np.int64)]] = 1
        a[allowed[e_idx + 1:e_idx + 11]] = 1
        assert (a == 1).sum() >= r and (a == 0).sum() == len(zeros)
        out.append((f"three_values_{name}", a))
    return out


def null_runs(n):
    """about half the rows null, in alternating runs of 63 / 64 / 65 rows: the validity words straddle the lanes' 64-row steps"""
    ok = np.ones(n, bool)
    at, j, flag = 0, 0, True
    while at < n:
        run = (63, 64, 65)[j % 3]
        ok[at:at + run] = flag
        at, j, flag = at + run, j + 1, not flag
    return ok


def shapes(n, k, narrow, rng):
    """-> [(name, dtype, values, validity)]: the 8-byte inputs, or their 4-byte twins"""
    it, ft = ("i32", "f32") if narrow else ("i64", "f64")
    out = [("all_equal", it, np.full(n, 7), None)]
    out += [(nm, it, a, None) for nm, a in three_values(n, k)]
    out.append(("decreasing", it, n - np.arange(n), None))
    out.append(("decreasing_f", ft, (n - np.arange(n)).astype(np.float64) * 0.5, None))
    out.append(("null_runs", it, rng.integers(0, 1000, n), null_runs(n)))
    pool = np.array([np.nan, 0.0, -0.0, 1.5, -1.5, 0.0, -0.0, np.inf, -np.inf, 2.0])
    out.append(("nan_and_zeros", ft, pool[rng.integers(0, len(pool), n)], rng.random(n) > 0.1))
    if narrow:  # the top 11 bits are the same in every value: the select's first level has one bin
        out.append(("constant_top_bits", "i32", (0x3F5 << 21) | rng.integers(0, 1 << 21, n), None))
    else:       # the top 22 bits are: two levels with one bin
        out.append(("constant_top_bits", "u64", (np.uint64(0xABCDE5) << np.uint64(42)) | rng.integers(0, 1 << 42, n).astype(np.uint64), None))
    return out


@pytest.mark.parametrize("narrow", [False, True], ids=["8byte", "4byte"])
@pytest.mark.parametrize("n", SIZES)
def test_select_k_boundary_shapes(env, monkeypatch, n, narrow):
    monkeypatch.setenv("PDX_SELECT_K_PLAN", "select")
    rng = np.random.default_rng(n)
    ks = sorted({1, 64, 65, 4096, 4097, n // 3, n - 1})
    built = {}
    for k in ks:
        for name, dt, a, valid in shapes(n, k, narrow, rng):
            a = np.asarray(a, R.NP_DTYPES[dt])
            key = name if not name.startswith("three_values") else (name, k)
            if key not in built:  # one column and one reference sort per order serve every k
                built[key] = (column(env, a, valid, dt), {asc: R.argsort(a, valid, asc) for asc in (True, False)}, a)
            col, want, a0 = built[key]
            for ascending in (True, False):
                got, plan = run_select_k(env, col, k, ascending, n, "select", (name, k))
                assert np.array_equal(got, want[ascending][:k]), (name, dt, n, k, ascending)
                if name == "all_equal":
                    assert np.array_equal(got, np.arange(min(k, n), dtype=np.uint64))
                if name == "constant_top_bits" and 0 < k < n and n > 4096:  # (a bin of at most 4096 rows is finished in LDS after one level)
                    assert int(plan["levels"]) >= 2, plan
            if name.startswith("three_values"):  # the mirrored column puts the same tie group at the threshold of the k LARGEST
                mirrored = (2 - a0).astype(a0.dtype)
                got, _ = run_select_k(env, column(env, mirrored, valid, dt), k, False, n, "select", (name, k))
                assert np.array_equal(got, want[True][:k]), (name, "mirrored", n, k)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_k_beyond_the_numbers_spills_into_nan_then_null_rows(env, monkeypatch, dt):
    monkeypatch.setenv("PDX_SELECT_K_PLAN", "select")
    n = 2 * CHUNK + 77
    rng = np.random.default_rng(5)
    a = rng.integers(0, 50, n).astype(R.NP_DTYPES[dt])
    a[rng.random(n) < 0.2] = np.nan
    valid = rng.random(n) > 0.2
    numbers, nan, nulls = R.counts(a, valid)
    assert nan > 100 and nulls > 100
    col = column(env, a, valid, dt)
    for ascending in (True, False):
        want = R.argsort(a, valid, ascending)
        for k in (numbers + 1, numbers + nan - 1, numbers + nan, numbers + nan + 3, n - 1):
            got, _ = run_select_k(env, col, k, ascending, n, "select", k)
            assert np.array_equal(got, want[:k]), (dt, k, ascending)
        k = numbers + nan + 3
        rows = np.arange(n, dtype=np.uint64)
        _, cls = R.keys_and_classes(a, valid)
        assert np.array_equal(want[numbers:k], np.concatenate([rows[cls == 1], rows[cls == 2][:3]]))  # NaN rows, then null rows, in row order


def test_the_default_plan_follows_k(env, monkeypatch):
    monkeypatch.delenv("PDX_SELECT_K_PLAN", raising=False)
    a = np.random.default_rng(1).integers(-1000, 1000, 5000)
    col = column(env, a, None, "i64")
    want = R.argsort(a, None, False)
    for k, plan in ((0, "empty"), (3, "select"), (4999, "sort"), (5000, "sort"), (5005, "sort")):
        got = env.K.select_k(col, k, False)
        assert env.K.select_k_last_plan()["plan"] == plan, k
        assert np.array_equal(got.to_numpy()[0][: got.length], want[:k]), k
    assert env.K.select_k(column(env, a[:0], None, "i64"), 4, True).length == 0 and env.K.select_k_last_plan()["plan"] == "empty"


# ---------------------------------------------------------------- partition_nth: the contract and the deterministic layout
@pytest.mark.parametrize("narrow", [False, True], ids=["8byte", "4byte"])
@pytest.mark.parametrize("n", SIZES)
def test_partition_nth_boundary_shapes(env, n, narrow):
    rng = np.random.default_rng(n)
    for name, dt, a, valid in shapes(n, n // 3, narrow, rng):
        a = np.asarray(a, R.NP_DTYPES[dt])
        col = column(env, a, valid, dt)
        numbers = R.counts(a, valid)[0]
        sk = R.sorted_number_keys(a, valid)
        for pivot in sorted({p for p in (0, 1, n // 2, numbers - 1, numbers, n - 1, n) if 0 <= p <= n}):
            got = env.K.partition_nth(col, pivot)
            assert got.dtype == env.L.UINT64 and got.length == n and got.validity is None
            idx = got.to_numpy()[0]
            R.check_partition(a, valid, pivot, idx, sk)
            assert np.array_equal(idx, R.partition_nth(a, valid, pivot, sk)), (name, dt, n, pivot)


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("dt", R.TOPK_DTYPES)
def test_partition_nth_on_the_golden_columns(env, dt, offset):
    for c in (c for c in GOLD.cases if c["dtype"] == dt):
        a, valid = GOLD.column(c)
        col = column(env, a, valid, dt, offset)
        n, m = c["rows"], c["numbers"]
        for pivot in sorted({p for p in (0, 1, n // 2, m - 1, m, n - 1, n) if 0 <= p <= n}):
            idx = env.K.partition_nth(col, pivot).to_numpy()[0][:n]
            R.check_partition(a, valid, pivot, idx)
            assert np.array_equal(idx, R.partition_nth(a, valid, pivot)), (c["name"], pivot, offset)


# ---------------------------------------------------------------- refusals (nothing is launched)
def test_refusals(env):
    L, K = env.L, env.K
    a = column(env, [3, 1, 2], None, "i64")
    b = K.Column.from_numpy(np.array([True, False, True]))
    for fn in (lambda: K.select_k(b, 1), lambda: K.partition_nth(b, 1)):
        with pytest.raises(L.PdxError) as e:
            fn()
        assert e.value.status == L.NOT_IMPLEMENTED and "bool" in str(e.value)
    ca = a.c()
    ok3 = K.Column.empty(L.UINT64, 3)
    for fn in (lambda: env.lib.pdx_select_k(C.byref(ca), -1, 1, C.byref(ok3.mut()), None), lambda: env.lib.pdx_partition_nth(C.byref(ca), -1, C.byref(ok3.mut()), None),
               lambda: env.lib.pdx_partition_nth(C.byref(ca), 4, C.byref(ok3.mut()), None)):
        assert fn() == L.INVALID
    short, wrong = K.Column.empty(L.UINT64, 1).mut(), K.Column.empty(L.INT64, 3).mut()
    assert env.lib.pdx_select_k(C.byref(ca), 2, 1, C.byref(short), None) == L.INVALID
    assert env.lib.pdx_select_k(C.byref(ca), 2, 1, C.byref(wrong), None) == L.INVALID
    short, wrong = K.Column.empty(L.UINT64, 2).mut(), K.Column.empty(L.INT64, 3).mut()
    assert env.lib.pdx_partition_nth(C.byref(ca), 1, C.byref(short), None) == L.INVALID
    assert env.lib.pdx_partition_nth(C.byref(ca), 1, C.byref(wrong), None) == L.INVALID
    # a capacity of min(k, length) is enough, and pivot == length is legal
    m = K.Column.empty(L.UINT64, 3).mut()
    assert env.lib.pdx_select_k(C.byref(ca), 100, 1, C.byref(m), None) == L.OK and m.length == 3
    assert K.partition_nth(a, 3).to_numpy()[0].tolist() == [1, 2, 0]  # (T = the largest key: the rows below it in row order, then its row)


# ---------------------------------------------------------------- junk independence
@pytest.mark.parametrize("forced", ["select", "sort"])
@pytest.mark.parametrize("k", [5, 4097, 9000])
def test_nothing_is_written_past_the_result(env, monkeypatch, forced, k):
    monkeypatch.setenv("PDX_SELECT_K_PLAN", forced)
    n = 7000
    rng = np.random.default_rng(k)
    a = rng.standard_normal(n)
    a[rng.random(n) < 0.1] = np.nan
    valid = rng.random(n) > 0.2
    col = column(env, a, valid, "f64")
    cap = max(k, n) + 70
    out = env.K.Column.empty(env.L.UINT64, cap)
    out.values.view(env.torch.uint8).fill_(PATTERN)
    m, ca = out.mut(), col.c()
    env.L.check(env.lib.pdx_select_k(C.byref(ca), k, 0, C.byref(m), env.K._stream()))
    env.torch.cuda.synchronize()
    rows = min(k, n)
    assert m.length == rows and m.null_count == 0
    vals = out.values.cpu().numpy().view(np.uint64)
    assert np.array_equal(vals[:rows], R.select_k(a, valid, k, False))
    assert (vals[rows:].view(np.uint8) == PATTERN).all(), "entries beyond min(k, n) were written"
    # partition_nth: exactly n entries
    out.values.view(env.torch.uint8).fill_(PATTERN)
    m = out.mut()
    env.L.check(env.lib.pdx_partition_nth(C.byref(ca), min(k, n), C.byref(m), env.K._stream()))
    env.torch.cuda.synchronize()
    vals = out.values.cpu().numpy().view(np.uint64)
    assert m.length == n and np.array_equal(vals[:n], R.partition_nth(a, valid, min(k, n)))
    assert (vals[n:].view(np.uint8) == PATTERN).all(), "entries beyond n were written"


# ---------------------------------------------------------------- the Python facade
def _frame(s):
    return s.col.to_numpy(), s.index.to_numpy()


def _same(x, y):
    (xv, xok), (xi, _) = x
    (yv, yok), (yi, _) = y
    ok = np.ones(len(xv), bool) if xok is None else xok
    return len(xv) == len(yv) and np.array_equal(ok, np.ones(len(yv), bool) if yok is None else yok) and np.array_equal(R.bits(xv)[ok], R.bits(yv)[ok]) and np.array_equal(xi, yi)


@pytest.mark.parametrize("dt", ["i64", "u64", "f64", "ts"])
def test_n_largest_and_n_smallest_equal_sort_sliced(env, dt):
    api, K = env.api, env.K
    n = 3000
    rng = np.random.default_rng(11)
    a = rng.integers(0, 40, n).astype(R.NP_DTYPES[dt])
    if dt == "f64":
        a[rng.random(n) < 0.1] = np.nan
        a[rng.random(n) < 0.1] = -0.0
    valid = rng.random(n) > 0.15
    labels = K.Column.from_numpy(rng.permutation(n).astype(np.int64) * 3)
    for index in (None, labels):
        s = api.Series(column(env, a, valid, dt), index=index, name="v")
        for k in (0, 1, 7, n - 1, n, n + 9):
            for fn, asc in ((s.n_largest, False), (s.n_smallest, True)):
                full, top = s.sort(asc), fn(k)
                assert top.name == "v" and top.size() == min(k, n)
                want = (tuple(None if x is None else x[:k] for x in full.col.to_numpy()), tuple(None if x is None else x[:k] for x in full.index.to_numpy()))
                assert _same(_frame(top), want), (dt, k, asc, index is not None)


@pytest.mark.parametrize("dt", ["i32", "f32"])
def test_the_facade_takes_four_byte_columns(env, dt):
    api = env.api
    a = np.array([5, -3, 9, 9, 0, -3, 7], R.NP_DTYPES[dt])
    valid = np.array([1, 1, 1, 0, 1, 1, 1], bool)
    s = api.Series(column(env, a, valid, dt), name="v")
    top = s.n_largest(3)
    assert top.col.dtype == env.dts[dt] and top.col.to_numpy()[0].tolist() == [9, 7, 5] and top.index.to_numpy()[0].tolist() == [2, 6, 0]
    low = s.n_smallest(4)
    assert low.col.to_numpy()[0].tolist() == [-3, -3, 0, 5] and low.index.to_numpy()[0].tolist() == [1, 5, 4, 0]
    everything = s.n_smallest(50)
    assert everything.size() == 7 and everything.index.to_numpy()[0].tolist() == [1, 5, 4, 0, 6, 2, 3] and everything.col.null_count == 1
    nth = s.nth_element(2)
    assert nth.col.dtype == env.L.UINT64 and nth.col.to_numpy()[0].tolist() == [1, 5, 4, 0, 2, 6, 3]


def test_nth_element_keeps_the_index(env):
    api, K = env.api, env.K
    labels = K.Column.from_numpy(np.array([10, 20, 30, 40], np.int64))
    s = api.Series(np.array([4.0, 1.0, 3.0, 1.0]), index=labels, name="v")
    r = s.nth_element(1)
    assert r.index is labels and r.col.to_numpy()[0].tolist() == [1, 3, 0, 2]
    assert s.nth_element().col.to_numpy()[0].tolist() == [1, 3, 0, 2]
    with pytest.raises(env.L.PdxError):
        s.nth_element(5)
