"""GPU: pdx_is_in / pdx_index_in / pdx_index / pdx_arg_extreme / pdx_dictionary_encode through the C ABI (pandasarrow_amd/column.py) against
tests/golden/lookup_golden.npz (Arrow C++ 25) and the numpy restatement tests/_lookup_ref.py, which tests/test_lookup_golden.py holds against
that file.  Everything is bit-exact.  No pyarrow."""
import ctypes as C
import os

import numpy as np
import pytest

import _lookup_ref as R

pytestmark = pytest.mark.gpu

GOLD = R.LookupGolden()
LDS_MAX = 2048  # kLkLdsMaxEntries (pandasarrow_amd/csrc/lookup.hip)
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


def slots_for(m):
    s = 2
    while s < 2 * m:
        s *= 2
    return s


def expected_plan(m, lds_max=LDS_MAX):
    return {"plan": "empty" if m == 0 else "lds" if m <= lds_max else "global", "set_size": str(m), "slots": str(slots_for(m))}


def check_set(env, a, valid, s, svalid, dt, skip, offset=0, want=None, lds_max=LDS_MAX, what=""):
    """is_in and index_in of one input against the restatement (or `want` = (index, ok) from the golden file), the plan, the null counts"""
    a, s = np.asarray(a, R.NP_DTYPES[dt]), np.asarray(s, R.NP_DTYPES[dt])
    ca, cs = column(env, a, valid, dt, offset), column(env, s, svalid, dt, offset)
    widx, wok = want if want is not None else R.index_in(a, valid, s, svalid, skip)
    got = env.K.is_in(ca, cs, skip)
    assert env.K.lookup_last_plan() == expected_plan(len(s), lds_max), (what, env.K.lookup_last_plan())
    assert got.dtype == env.L.BOOL and got.length == len(a) and got.null_count == 0, what
    assert np.array_equal(got.to_numpy()[0], wok), (what, "is_in", dt, len(a), len(s), skip, offset)
    got = env.K.index_in(ca, cs, skip)
    assert env.K.lookup_last_plan() == expected_plan(len(s), lds_max), (what, env.K.lookup_last_plan())
    gv, gok = got.to_numpy()
    assert got.dtype == env.L.INT32 and got.length == len(a), what
    assert np.array_equal(gok, wok), (what, "index_in validity", dt, len(a), len(s), skip, offset)
    assert np.array_equal(gv, widx), (what, "index_in", dt, len(a), len(s), skip, offset)  # (zero under a null)
    assert got.null_count == int((~wok).sum()), what


# ---------------------------------------------------------------- the golden file through the C ABI
@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("dt", R.LOOKUP_DTYPES)
def test_golden_sets_through_the_abi(env, dt, offset):
    for c in (c for c in GOLD.cases if c["kind"] == "set" and c["dtype"] == dt):
        (a, valid), (s, svalid) = GOLD.column(c, "a"), GOLD.column(c, "set")
        check_set(env, a, valid, s, svalid, dt, c["skip_nulls"], offset, want=(GOLD.arr(c, "index_in"), GOLD.arr(c, "index_in_ok")), what=c["name"])


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("dt", R.LOOKUP_DTYPES)
def test_golden_index_argext_dict_through_the_abi(env, dt, offset):
    for c in (c for c in GOLD.cases if c["dtype"] == dt and c["kind"] != "set"):
        a, valid = GOLD.column(c, "a")
        col = column(env, a, valid, dt, offset)
        if c["kind"] == "index":
            value = None if c["value_null"] else R.from_bits(np.array([c["value_bits"]], np.uint64), dt)[0].item()
            assert env.K.index(col, value) == c["row"], c["name"]
        elif c["kind"] == "argext":
            assert env.K.arg_extreme([col], False) == [c["argmin"]], c["name"]
            assert env.K.arg_extreme([col], True) == [c["argmax"]], c["name"]
        else:
            check_dict(env, col, GOLD.arr(c, "codes"), GOLD.arr(c, "codes_ok"), GOLD.arr(c, "dict"), c["name"])


def check_dict(env, col, wcodes, wok, wdict_bits, what):
    codes, dic = env.K.dictionary_encode(col)
    gv, gok = codes.to_numpy()
    assert codes.dtype == env.L.INT32 and codes.length == len(wcodes) and dic.dtype == col.dtype and dic.null_count == 0, what
    assert np.array_equal(np.ones(len(wok), bool) if gok is None else gok, wok), what
    assert np.array_equal(gv, wcodes), what
    assert codes.null_count == int((~wok).sum()), what
    assert np.array_equal(R.bits(dic.to_numpy()[0]), wdict_bits), what


# ---------------------------------------------------------------- shapes the golden file does not hold
def fuzz_input(rng, dt, n, m):
    """input and set over a range about twice the set's size, so that about half of the rows hit; floats carry NaN payloads and both zeros"""
    t = R.NP_DTYPES[dt]
    span = max(4, 2 * m + 3)
    base = {"u64": 2**63 - 7, "i64": -5, "ts": -5, "i32": -5}.get(dt, 0)
    if dt in ("f64", "f32"):
        a, s = (rng.integers(0, span, n) - 3).astype(t) * t(0.5), (rng.integers(0, span, m) - 3).astype(t) * t(0.5)
        u = np.uint32 if dt == "f32" else np.uint64
        nan = np.array([np.nan], t).view(u)[0]
        odd = np.array([nan, nan + u(1), nan | (u(1) << u(t().itemsize * 8 - 1)), np.array([-0.0], t).view(u)[0]], u).view(t)
        if n > 8:
            a[rng.integers(0, n, max(1, n // 8))] = odd[rng.integers(0, 4, max(1, n // 8))]
        if m > 1:
            s[rng.integers(0, m, max(1, m // 8))] = odd[rng.integers(0, 4, max(1, m // 8))]
        return a, s
    if dt == "u64":
        return (rng.integers(0, span, n).astype(np.uint64) + np.uint64(base)), (rng.integers(0, span, m).astype(np.uint64) + np.uint64(base))
    return (rng.integers(0, span, n) + base).astype(t), (rng.integers(0, span, m) + base).astype(t)


@pytest.mark.parametrize("m", [0, 1, 2, LDS_MAX, LDS_MAX + 1, 70_000])
def test_row_counts_and_set_sizes(env, m):
    """rows at the wave and tile edges and on the grid-stride path; set sizes on both sides of the LDS budget"""
    rng = np.random.default_rng(1000 + m)
    for n in (0, 1, 63, 64, 65, 4099, 200_000):
        a, s = fuzz_input(rng, "i64", n, m)
        check_set(env, a, rng.random(n) > 0.2, s, rng.random(m) > 0.1, "i64", skip=n % 2, what=f"n={n} m={m}")
    for dt in ("f64", "u64", "i32", "f32", "ts"):
        a, s = fuzz_input(rng, dt, 4099, m)
        check_set(env, a, rng.random(4099) > 0.2, s, rng.random(m) > 0.1, dt, skip=0, what=f"{dt} m={m}")
        check_set(env, a, None, s, None, dt, skip=1, offset=3, what=f"{dt} m={m} no validity")


def test_the_override_forces_the_global_plan_at_a_small_set(env):
    rng = np.random.default_rng(7)
    a, s = fuzz_input(rng, "f64", 4099, 5)
    old = os.environ.get("PDX_LOOKUP_LDS_MAX")
    os.environ["PDX_LOOKUP_LDS_MAX"] = "4"
    try:
        check_set(env, a, rng.random(4099) > 0.2, s, np.array([1, 1, 0, 1, 1], bool), "f64", skip=0, lds_max=4, what="override")
        assert env.K.lookup_last_plan()["plan"] == "global"
        check_set(env, a, None, s[:4], None, "f64", skip=0, lds_max=4, what="override, at the bound")
        assert env.K.lookup_last_plan()["plan"] == "lds"
    finally:
        if old is None:
            del os.environ["PDX_LOOKUP_LDS_MAX"]
        else:
            os.environ["PDX_LOOKUP_LDS_MAX"] = old


@pytest.mark.parametrize("plan", ["lds", "global"])
def test_power_of_two_strides_at_load_factor_one_half(env, plan):
    """entries k * 2^j: the worst case for a hash that keeps low bits.  2048 of them fill 4096 slots to exactly one half."""
    k = np.arange(1, 513, dtype=np.int64)
    s = np.concatenate([k << j for j in (0, 12, 32, 45)])[:LDS_MAX]
    assert len(np.unique(s)) > 1900 and slots_for(len(s)) == 2 * len(s)
    rng = np.random.default_rng(3)
    a = np.concatenate([s[rng.integers(0, len(s), 3000)], (k << 20)[:500], s[:599] + 1])
    old = os.environ.get("PDX_LOOKUP_LDS_MAX")
    if plan == "global":
        os.environ["PDX_LOOKUP_LDS_MAX"] = "0"
    try:
        for dt in ("i64", "u64"):
            check_set(env, a, None, s, None, dt, skip=0, lds_max=LDS_MAX if plan == "lds" else 0, what=plan)
    finally:
        if plan == "global":
            if old is None:
                del os.environ["PDX_LOOKUP_LDS_MAX"]
            else:
                os.environ["PDX_LOOKUP_LDS_MAX"] = old


def test_duplicates_first_position_wins_and_uint64_above_2_63(env):
    s = np.array([2**63 + 9, 5, 2**63 + 9, 2**64 - 1, 5, 5, 0, 2**64 - 1], np.uint64)
    a = np.array([5, 2**64 - 1, 2**63 + 9, 1, 0, 2**63 - 1, 2**63], np.uint64)
    for skip in (0, 1):
        check_set(env, a, None, s, None, "u64", skip)
    got = env.K.index_in(column(env, a, None, "u64"), column(env, s, None, "u64")).to_numpy()
    assert got[0].tolist() == [1, 3, 0, 0, 6, 0, 0] and got[1].tolist() == [True, True, True, False, True, False, False]
    big = np.repeat(np.arange(100, dtype=np.int64), 30)[::-1].copy()  # 3000 entries, every value 30 times: global plan
    check_set(env, np.arange(-5, 120, dtype=np.int64), None, big, None, "i64", 0)


@pytest.mark.parametrize("index", [False, True])
@pytest.mark.parametrize("n", [1, 13, 64, 67, 129, 4099])
def test_output_bits_and_rows_beyond_n_are_kept(env, n, index):
    rng = np.random.default_rng(n)
    a, s = fuzz_input(rng, "i64", n, 9)
    valid = rng.random(n) > 0.3
    ca, cs = column(env, a, valid, "i64"), column(env, s, None, "i64")
    cap = n + 70
    out = env.K.Column.empty(env.L.INT32 if index else env.L.BOOL, cap, with_validity=index)
    out.values.view(env.torch.uint8).fill_(PATTERN)
    if index:
        out.validity.fill_(PATTERN)
    before_bits = (out.validity if index else out.values).cpu().numpy().copy()
    m, a_, s_ = out.mut(), ca.c(), cs.c()
    fn = env.lib.pdx_index_in if index else env.lib.pdx_is_in
    env.L.check(fn(C.byref(a_), C.byref(s_), 0, C.byref(m), env.K._stream()))
    env.torch.cuda.synchronize()
    assert m.length == n
    after_bits = (out.validity if index else out.values).cpu().numpy()
    want = R.index_in(a, valid, s, None, 0)
    assert np.array_equal(np.unpackbits(after_bits, bitorder="little")[:n].astype(bool), want[1])
    assert np.array_equal(np.unpackbits(after_bits, bitorder="little")[n:], np.unpackbits(before_bits, bitorder="little")[n:]), "bits beyond n were written"
    if index:
        vals = out.values.cpu().numpy()
        assert np.array_equal(vals[:n], want[0]) and (vals[n:].view(np.uint8) == PATTERN).all(), "rows beyond n were written"
        assert m.null_count == int((~want[1]).sum())
    else:
        assert m.null_count == 0


# ---------------------------------------------------------------- index / arg_extreme
def test_index_first_match_and_tiles(env):
    rng = np.random.default_rng(5)
    for dt in R.LOOKUP_DTYPES:
        t = R.NP_DTYPES[dt]
        for n in (1, 63, 64, 65, 4099, 200_000):
            a = (rng.integers(10, 50, n)).astype(t)
            valid = rng.random(n) > 0.2
            for pos in {0, n // 2, n - 1}:
                b = a.copy()  # (no 7 anywhere yet)
                b[pos] = 7
                b[n - 1] = 7
                v = valid.copy()
                col = column(env, b, v, dt, offset=3)
                assert env.K.index(col, 7) == R.index(b, v, 7), (dt, n, pos)
                assert env.K.index(column(env, b, None, dt), 7) == pos, (dt, n, pos)
            assert env.K.index(column(env, a, valid, dt), 99) == -1
            assert env.K.index(column(env, a, valid, dt), None) == -1
    # a scalar that the column's width cannot hold equals no row (no truncation to 5, no rounding to float32(0.1))
    i32 = column(env, [5, 7, -1], None, "i32")
    assert env.K.index(i32, 2**32 + 5) == -1 and env.K.index(i32, -2**31 - 1) == -1 and env.K.index(i32, -1) == 2
    f32 = column(env, [0.5, np.float32(0.1), 3.0], None, "f32")
    assert env.K.index(f32, 0.1) == -1 and env.K.index(f32, float(np.float32(0.1))) == 1 and env.K.index(f32, 0.5) == 0
    z = np.array([3.0, -0.0, 0.0, np.nan], np.float64)
    assert env.K.index(column(env, z, None, "f64"), 0.0) == 1 and env.K.index(column(env, z, None, "f64"), -0.0) == 1
    assert env.K.index(column(env, z, None, "f64"), float("nan")) == -1
    assert env.K.index(column(env, z, np.array([1, 0, 1, 1], bool), "f64"), -0.0) == 2


def arg_both(env, cols):
    return env.K.arg_extreme(cols, False), env.K.arg_extreme(cols, True)


def test_arg_extreme_ties_zeros_nan_null(env):
    nz = -0.0
    cases = [("f64", [4, 9, 1, 9, 4, 1], None), ("i64", [4, 9, 1, 9, 4, 1], None), ("u64", [2**63 + 1, 0, 2**64 - 1, 0, 2**64 - 1], None),
             ("f64", [3, 0.0, nz, 3], None), ("f64", [3, nz, 0.0, 3], None), ("f64", [-3, 0.0, nz, -3], None), ("f64", [-3, nz, 0.0, -3], None),
             ("f32", [-3, nz, 0.0, -3], None), ("f64", [np.nan, np.nan], None), ("f64", [np.nan, 2, 1, 2, np.nan], None), ("f64", [1, 2], [0, 0]),
             ("f64", [], None), ("i32", [-2**31, 2**31 - 1, -2**31, 2**31 - 1], None), ("f64", [np.nan, 5, np.nan], [1, 0, 1]),
             ("f64", [np.inf, -np.inf, np.nan, np.inf, -np.inf], None), ("ts", [5, -7, 5, -7], [1, 0, 1, 1])]
    for dt, a, valid in cases:
        a = np.asarray(a, R.NP_DTYPES[dt])
        valid = None if valid is None else np.asarray(valid, bool)
        for offset in (0, 3):
            got = arg_both(env, [column(env, a, valid, dt, offset)])
            assert got == ([R.arg_extreme(a, valid, False)], [R.arg_extreme(a, valid, True)]), (dt, a, valid, offset)


def test_arg_extreme_mixed_frame_one_call_and_final_partial_tile(env):
    rng = np.random.default_rng(9)
    n = 4099
    host = {"f64": rng.normal(size=n), "i64": rng.integers(-1000, 1000, n), "f32": rng.normal(size=n).astype(np.float32),
            "u64": rng.integers(0, 2**63, n).astype(np.uint64) * np.uint64(2), "i32": rng.integers(-50, 50, n)}
    host = {dt: np.asarray(a, R.NP_DTYPES[dt]) for dt, a in host.items()}
    host["f64"][4098], host["f64"][4097] = -100.0, 100.0   # both extremes in the last, partial tile
    host["f32"][0], host["f32"][4098] = np.nan, np.nan
    valids = {dt: rng.random(n) > 0.3 for dt in host}
    valids["f64"][4097:] = True
    valids["i32"][:] = False                                # one all-null column
    valids["u64"] = None
    cols = [column(env, host[dt], valids[dt], dt, offset=3 if dt == "i64" else 0) for dt in host]
    lo, hi = arg_both(env, cols)
    for j, dt in enumerate(host):
        assert lo[j] == R.arg_extreme(host[dt], valids[dt], False) and hi[j] == R.arg_extreme(host[dt], valids[dt], True), dt
    assert (lo[0], hi[0]) == (4098, 4097) and (lo[4], hi[4]) == (-1, -1)
    big = rng.integers(0, 1000, 200_000).astype(np.int64)  # many workgroups, ties everywhere
    bv = rng.random(200_000) > 0.5
    assert arg_both(env, [column(env, big, bv, "i64"), column(env, big[:65], None, "i64")]) == (
        [R.arg_extreme(big, bv, False), R.arg_extreme(big[:65], None, False)], [R.arg_extreme(big, bv, True), R.arg_extreme(big[:65], None, True)])


# ---------------------------------------------------------------- properties
@pytest.mark.parametrize("seed", range(20))
def test_properties_on_fuzzed_data(env, seed):
    rng = np.random.default_rng(seed)
    dt = R.LOOKUP_DTYPES[seed % len(R.LOOKUP_DTYPES)]
    n = int(rng.integers(1, 50_000))
    a, s = fuzz_input(rng, dt, n, int(rng.integers(1, 5000)))
    valid = None if seed % 4 == 0 else rng.random(n) > 0.15
    col = column(env, a, valid, dt, offset=seed % 5)
    codes, dic = env.K.dictionary_encode(col)
    wcodes, wok, wdict = R.dictionary_encode(a, valid)
    assert np.array_equal(R.bits(dic.to_numpy()[0]), R.bits(wdict)) and np.array_equal(codes.to_numpy()[0], wcodes)
    again = env.K.index_in(col, dic)  # index_in(x, unique(x)) is dictionary_encode(x)'s codes
    assert np.array_equal(again.to_numpy()[0], wcodes) and np.array_equal(again.to_numpy()[1], wok)
    assert again.null_count == codes.null_count == int((~wok).sum())
    cs = column(env, s, rng.random(len(s)) > 0.1, dt)
    for skip in (0, 1):
        assert np.array_equal(env.K.is_in(col, cs, skip).to_numpy()[0], env.K.index_in(col, cs, skip).to_numpy()[1])


# ---------------------------------------------------------------- refusals (nothing is launched)
def test_refusals(env):
    L, K = env.L, env.K
    a, s = column(env, [1, 2, 3], None, "i64"), column(env, [2], None, "i64")
    b = K.Column.from_numpy(np.array([True, False, True]))
    for fn in (lambda: K.is_in(b, b), lambda: K.index_in(b, b), lambda: K.is_in(a, b), lambda: K.index(b, 1), lambda: K.arg_extreme([a, b]),
               lambda: K.dictionary_encode(b)):
        with pytest.raises(L.PdxError) as e:
            fn()
        assert e.value.status == L.NOT_IMPLEMENTED and "bool" in str(e.value)
    for other in ("f64", "u64", "i32", "ts"):
        for fn in (K.is_in, K.index_in):
            with pytest.raises(L.PdxError) as e:
                fn(a, column(env, [2], None, other))
            assert e.value.status == L.INVALID and "value set" in str(e.value)
    ca, cs = a.c(), s.c()
    small, nov = K.Column.empty(L.BOOL, 2).mut(), K.Column.empty(L.INT32, 3).mut()
    wrong = K.Column.empty(L.INT64, 3, with_validity=True).mut()
    assert env.lib.pdx_is_in(C.byref(ca), C.byref(cs), 0, C.byref(small), None) == L.INVALID
    assert env.lib.pdx_index_in(C.byref(ca), C.byref(cs), 0, C.byref(nov), None) == L.INVALID   # no validity buffer
    assert env.lib.pdx_index_in(C.byref(ca), C.byref(cs), 0, C.byref(wrong), None) == L.INVALID  # int64 instead of int32
    codes, dic = K.Column.empty(L.INT32, 3).mut(), K.Column.empty(L.INT64, 2).mut()
    assert env.lib.pdx_dictionary_encode(C.byref(ca), C.byref(codes), C.byref(dic), None) == L.INVALID  # dictionary capacity < rows
    sc = L.PdxScalar(L.FLOAT64, 1)
    row = C.c_int64(5)
    assert env.lib.pdx_index(C.byref(ca), C.byref(sc), C.byref(row), None) == L.INVALID          # a float64 scalar for an int64 column
    null = L.PdxScalar(L.INT64, 0)
    assert env.lib.pdx_index(C.byref(ca), C.byref(null), C.byref(row), None) == L.OK and row.value == -1  # a null scalar is not an error
    assert env.lib.pdx_arg_extreme(0, C.byref(ca), 0, C.byref(row), None) == L.INVALID


# ---------------------------------------------------------------- the Python facade
def test_facade(env):
    api, K, L = env.api, env.K, env.L
    ts = np.array(["2024-01-01", "2024-01-02", "2024-01-03", "2024-01-04"], "datetime64[ns]")
    s = api.Series(K.Column.from_numpy(np.array([3.0, -1.0, 7.0, -1.0]), np.array([1, 1, 1, 0], bool)), index=K.Column.from_numpy(ts))
    assert s.argmin() == 1 and s.argmax() == 2 and s.index_of(7.0) == 2 and s.index_of(api.Scalar(8.0)) == -1
    assert s.idxMin().value == ts[1].astype(np.int64) and s.idxMax().value == ts[2].astype(np.int64)
    m = s.is_in([7.0, 3.0])
    assert m.index is s.index and m.to_numpy()[0].tolist() == [True, False, True, False]
    assert s[m].to_numpy()[0].tolist() == [3.0, 7.0]
    ix = s.index_in(api.Series(np.array([7.0, 3.0])))
    assert ix.to_numpy()[0].tolist() == [1, 0, 0, 0] and ix.to_numpy()[1].tolist() == [True, False, True, False]
    with pytest.raises(L.PdxError):
        api.Series(K.Column.from_numpy(np.zeros(3), np.zeros(3, bool))).idxMin()
    df = api.DataFrame({"a": np.array([5, 1, 9, 1]), "b": np.array([2.5, 8.0, -1.0, 8.0])}, index=K.Column.from_numpy(ts))
    assert {k: v.value for k, v in df.idxMin().items()} == {"a": ts[1].astype(np.int64), "b": ts[2].astype(np.int64)}
    assert {k: v.value for k, v in df.idxMax().items()} == {"a": ts[2].astype(np.int64), "b": ts[1].astype(np.int64)}
    i32 = api.Series(np.array([4, 4, 9]), dtype=L.INT32)
    assert i32.is_in(api.Series(np.array([9, 1]), dtype=L.INT32)).to_numpy()[0].tolist() == [False, False, True]
    with pytest.raises(L.PdxError):
        i32.is_in(np.array([2**40]))
    # unique / nunique / dictionary_encode beyond the integer dtypes
    nan = np.array([np.nan]).view(np.uint64)[0]
    f = np.array([0, nan, nan + 1, 2**63, 0, nan + 1], np.uint64).view(np.float64)  # 0.0, nan, nan', -0.0, 0.0, nan'
    fs = api.Series(K.Column.from_numpy(f))
    assert R.bits(fs.unique().to_numpy()[0]).tolist() == [0, int(nan), int(nan) + 1, 2**63] and fs.nunique() == 4
    codes, dic = fs.dictionary_encode()
    assert codes.to_numpy()[0].tolist() == [0, 1, 2, 3, 0, 2] and R.bits(dic.to_numpy()[0]).tolist() == [0, int(nan), int(nan) + 1, 2**63]
    n32 = api.Series(K.Column.from_numpy(np.array([7, 8, 0, 7, 9, 0], np.int32), np.array([1, 1, 0, 1, 1, 0], bool), dtype=L.INT32))
    u, ok = n32.unique().to_numpy()
    assert u[ok].tolist() == [7, 8, 9] and ok.tolist() == [True, True, False, True] and n32.nunique() == 3
    f32 = api.Series(K.Column.from_numpy(np.array([0.0, -0.0, 1.5, 0.0], np.float32)))
    assert R.bits(f32.unique().to_numpy()[0]).tolist() == [0, 2**31, int(R.bits(np.array([1.5], np.float32))[0])]
    bs = api.Series(K.Column.from_numpy(np.array([True, False, True]), np.array([1, 1, 0], bool)))
    assert bs.nunique() == 2 and bs.unique().size() == 3
