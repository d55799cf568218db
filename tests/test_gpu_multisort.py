"""GPU: pdx_sort_indices (multi-key sort as range-compressed composite keys, csrc/align.hip) through the C ABI and through
DataFrame.argsort / DataFrame.sort_values, against the lexsort restatement of Arrow's sort_indices (tests/_multisort_ref.py; pinned to
Arrow 25.0.0 by tests/test_multisort_golden.py).  pdx_sort_info proves which path ran (rounds, key bits, radix passes)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _multisort_ref as R

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX, U64_MAX = -2**63, 2**63 - 1, 2**64 - 1


@pytest.fixture(scope="module")
def lib():
    import torch

    from pandasarrow_amd import _lib as L

    assert torch.cuda.is_available()
    L.check(L.load().pdx_init(0))
    return L


def _dt(L, kind):
    return {"f64": L.FLOAT64, "i64": L.INT64, "u64": L.UINT64, "ts": L.TIMESTAMP_NS, "i32": L.INT32, "f32": L.FLOAT32}[kind]


def dev(L, col, offset=0):
    from pandasarrow_amd.column import Column

    v, valid, kind = col
    return Column.from_numpy(v, valid=None if valid is None or bool(np.all(valid)) and offset == 0 else valid, dtype=_dt(L, kind), offset=offset)


def gpu_sort(L, cols, desc, offsets=None, info=False):
    from pandasarrow_amd import column as K

    dcols = [dev(L, c, 0 if offsets is None else offsets[i]) for i, c in enumerate(cols)]
    out = K.sort_indices(dcols, desc, with_info=info)
    if info:
        return out[0].to_numpy()[0].astype(np.int64), out[1]
    return out.to_numpy()[0].astype(np.int64)


def check(L, cols, desc, offsets=None, what=""):
    got, info = gpu_sort(L, cols, desc, offsets, info=True)
    ref = R.sort_indices_ref(cols, desc)
    assert np.array_equal(got, ref), f"{what}: first difference at {int(np.flatnonzero(got != ref)[0])} of {len(ref)}; info {info}"
    return info


def col(values, kind, valid=None):
    v = np.asarray(values, dtype=R.NP_DTYPE[kind])
    return v, (np.ones(len(v), bool) if valid is None else np.asarray(valid, bool)), kind


_cases = None


def golden_cases_with_ref():
    """every case of the golden grid with the restatement's answer, computed once"""
    global _cases
    if _cases is None:
        _cases = [(name, cols, desc, R.sort_indices_ref(cols, desc)) for name, cols, desc in R.golden_cases()]
    return _cases


def _host_take(colv, ref):
    v, valid, _ = colv
    return v[ref], valid[ref]


@pytest.mark.parametrize("n", list(R.GOLDEN_NS))
def test_golden_cases_abi_and_python_methods(lib, n):
    """every golden case of n rows: the ABI, DataFrame.argsort, and DataFrame.sort_values as take-by-argsort of the rows and of the index"""
    from pandasarrow_amd import api
    from pandasarrow_amd import column as K

    ran = 0
    for name, cols, desc, ref in golden_cases_with_ref():
        if len(ref) != n:
            continue
        ran += 1
        dcols = [dev(lib, c) for c in cols]
        got = K.sort_indices(dcols, desc).to_numpy()[0].astype(np.int64)
        assert np.array_equal(got, ref), name
        names = [f"c{k}" for k in range(len(cols))]
        labels = (np.arange(n, dtype=np.int64) * 3 + 11)[::-1].copy()
        df = api.DataFrame(dict(zip(names, dcols)), index=labels if n else None)
        asc = [not d for d in desc]
        s = df.argsort(names, asc)
        assert s.col.dtype == lib.UINT64 and s.index is None
        assert np.array_equal(s.col.to_numpy()[0].astype(np.int64), ref), name
        if n == 0:
            continue
        out = df.sort_values(names, asc)
        assert np.array_equal(out.index.to_numpy()[0], labels[ref]), name
        for k, c in enumerate(cols):
            ev, eok = _host_take(c, ref)
            gv, gok = out.cols[k].to_numpy()
            gok = np.ones(n, bool) if gok is None else gok
            assert np.array_equal(gok, eok), (name, k)
            width = np.uint32 if ev.dtype.itemsize == 4 else np.uint64
            assert np.array_equal(np.ascontiguousarray(gv).view(width)[eok], np.ascontiguousarray(ev).view(width)[eok]), (name, k)
    assert ran >= 24


def test_sort_values_implicit_index_and_one_order_for_all(lib):
    from pandasarrow_amd import api

    a = col([2, 1, 2, 1, 3], "i64")
    b = col([50, 40, 10, 40, 5], "ts")
    v = col([0.5, 1.5, 2.5, 3.5, 4.5], "f64")
    df = api.DataFrame({"sym": dev(lib, a), "t": dev(lib, b), "v": dev(lib, v)})
    out = df.sort_values(["sym", "t"])
    assert out.index.to_numpy()[0].tolist() == [1, 3, 2, 0, 4]
    assert out["v"].col.to_numpy()[0].tolist() == [1.5, 3.5, 2.5, 0.5, 4.5]
    assert df.sort_values(["sym", "t"], ascending=False).index.to_numpy()[0].tolist() == [4, 0, 2, 1, 3]
    assert df.argsort("t").col.to_numpy()[0].tolist() == [4, 2, 1, 3, 0]
    with pytest.raises(lib.PdxError, match="nope not in schema"):
        df.argsort(["sym", "nope"])
    with pytest.raises(lib.PdxError, match="nope not in schema"):
        df.sort_values(["nope"])
    with pytest.raises(lib.PdxError):
        df.argsort(["sym", "t"], [True])


# ---------------------------------------------------------------- shapes that force a path
def test_two_narrow_keys_are_one_round(lib):
    n = 5000
    sym = 10 + R.pick(7, 1, n, 1000)
    sym[:2] = (10, 1009)  # range 999 -> 10 bits
    ts = 1_700_000_000_000_000_000 + R.pick(7, 2, n, 86400) * 1_000_000_000
    ts[2:4] = (1_700_000_000_000_000_000, 1_700_000_000_000_000_000 + 86399 * 1_000_000_000)  # a day in seconds, as ns -> 47 bits
    bits = (999).bit_length() + (86399 * 1_000_000_000).bit_length()
    assert bits == 10 + 47
    for desc in ([False, False], [True, False], [True, True]):
        rounds, key_bits, passes = check(lib, [col(sym, "i64"), col(ts, "ts")], desc)
        assert (rounds, key_bits, passes) == (1, bits, (bits + 7) // 8)
    # nulls in the first key add its 2-bit class field: still one round
    valid = R.uniform(7, 3, n) > 0.1
    rounds, key_bits, passes = check(lib, [col(sym, "i64", valid), col(ts, "ts")], [False, True])
    assert (rounds, key_bits, passes) == (1, bits + 2, 8)


def test_two_full_range_nullable_int64_keys_chain_rounds(lib):
    n = 3000
    pool = np.array([I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1], np.int64)
    a, b = pool[R.pick(8, 1, n, 7)], pool[R.pick(8, 2, n, 7)]
    a[:2] = b[:2] = (I64_MIN, I64_MAX)
    va, vb = R.uniform(8, 3, n) > 0.2, R.uniform(8, 4, n) > 0.2
    va[:2] = vb[:2] = True
    for desc in ([False, False], [True, False], [False, True]):
        rounds, key_bits, passes = check(lib, [col(a, "i64", va), col(b, "i64", vb)], desc)
        assert rounds >= 3 and key_bits == 64 + 2 + 64 + 2
        assert passes == 8 + 1 + 8 + 1  # a field is never split: (64), (2), (64), (2)


def test_uint64_full_range_shifts_by_64(lib):
    n = 2000
    pool = np.array([0, U64_MAX, 1, U64_MAX - 1, 2**63, 2**63 - 1], np.uint64)
    a = pool[R.pick(9, 1, n, 6)]
    a[:2] = (0, U64_MAX)
    tie = col(R.pick(9, 2, n, 3), "i32")
    for d in (False, True):
        assert check(lib, [col(a, "u64")], [d]) == (1, 64, 8)
        rounds, key_bits, _ = check(lib, [col(a, "u64"), tie], [d, not d])
        assert (rounds, key_bits) == (2, 66)
        rounds, key_bits, _ = check(lib, [tie, col(a, "u64")], [d, d])
        assert (rounds, key_bits) == (2, 66)


def test_constant_all_null_and_all_nan_keys(lib):
    n = 1000
    b = col(R.pick(10, 1, n, 50), "i64")
    const = col(np.full(n, 42), "i64")
    assert check(lib, [const, b], [False, True]) == (1, 6, 1)  # the leading key has width 0
    all_null = col(np.arange(n), "i64", np.zeros(n, bool))
    assert check(lib, [all_null, b], [True, False]) == (1, 2 + 6, 1)
    assert check(lib, [all_null], [False]) == (1, 2, 1)
    all_nan = col(np.full(n, np.nan), "f64")
    assert check(lib, [all_nan, b], [False, False]) == (1, 2 + 6, 1)
    some_null_nan = col(np.full(n, np.nan), "f32", R.uniform(10, 2, n) > 0.5)  # NaN < null decides, then b
    assert check(lib, [some_null_nan, b], [True, True]) == (1, 2 + 6, 1)
    got, info = gpu_sort(lib, [const, col(np.full(n, -0.0), "f64"), col(np.full(n, 7), "u64")], [False, True, False], info=True)
    assert info == (0, 0, 0) and np.array_equal(got, np.arange(n))  # every key constant: the rows as they are


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 40003])
def test_sizes_around_the_sort_tile(lib, n):
    a = col(R.pick(11, 1, n, 9) - 4, "i32", R.uniform(11, 2, n) > 0.1)
    b = col((R.pick(11, 3, n, 41) - 20) / 4.0, "f32")
    b[0][R.uniform(11, 4, n) < 0.1] = np.nan
    c = col(R.splitmix(11, 5, n).view(np.int64), "i64")  # 64 random bits
    check(lib, [a, b, c], [False, True, False], what=f"n={n}")
    check(lib, [c, a], [True, True], what=f"n={n}")


def test_sliced_columns_share_validity_bytes(lib):
    """offsets 1, 7 and 9: the validity bit offset is no multiple of 8 and differs from key to key"""
    from pandasarrow_amd import column as K

    n = 777
    cols = [R.make_column(12, k, n, kind, True, fine=(k == 2)) for k, kind in enumerate(("i32", "f64", "ts"))]
    for offsets in ((1, 7, 9), (9, 1, 7), (7, 9, 1)):
        check(lib, cols, [False, True, False], offsets=offsets, what=str(offsets))
    # a slice out of the middle of longer columns, validity bits of the neighbours in the same bytes
    start, m = 3, n - 8
    dcols = [dev(lib, c, offset=o).slice(start, m) for c, o in zip(cols, (1, 7, 9))]
    got = K.sort_indices(dcols, [True, False, False]).to_numpy()[0].astype(np.int64)
    part = [(v[start:start + m], ok[start:start + m], kind) for v, ok, kind in cols]
    assert np.array_equal(got, R.sort_indices_ref(part, [True, False, False]))


def test_non_default_stream(lib):
    import torch

    n = 20000
    cols = [R.make_column(13, k, n, kind, True, fine=True) for k, kind in enumerate(("u64", "f32"))]
    ref = R.sort_indices_ref(cols, [True, False])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = gpu_sort(lib, cols, [True, False])
    st.synchronize()
    assert np.array_equal(got, ref)


def test_every_order_mix_of_three_keys(lib):
    n = 1500
    cols = [R.make_column(14, 0, n, "f64", True), R.make_column(14, 1, n, "i64", True), R.make_column(14, 2, n, "f32", False, fine=True)]
    for desc in itertools.product((False, True), repeat=3):
        check(lib, cols, list(desc), what=str(desc))


def test_negative_zero_ties_with_zero(lib):
    a = col([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], "f64")
    b = col([3, 2, 1, 0, 0, 0], "i64")
    assert gpu_sort(lib, [a, b], [False, False]).tolist() == [5, 3, 2, 1, 0, 4]
    assert gpu_sort(lib, [a, b], [True, True]).tolist() == [4, 0, 1, 2, 3, 5]
    a32 = col([0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45], "f32")  # the smallest denormals stay apart from the zeros
    assert gpu_sort(lib, [a32, b], [False, False]).tolist() == [5, 3, 2, 1, 0, 4]


def test_random_small_cases(lib):
    """200 seeded cases: n <= 300, 1 to 5 keys, all six dtypes, with and without nulls, wide and narrow ranges"""
    seen = set()
    for t in range(200):
        seed = 5000 + t
        n = int(R.pick(seed, 0, 1, 301)[0])
        nk = 1 + int(R.pick(seed, 1, 1, 5)[0])
        kinds = [R.KINDS[i] for i in R.pick(seed, 2, nk, 6)]
        shape = R.pick(seed, 3, nk, 4)
        nulls = R.pick(seed, 4, nk, 2)
        cols = [R.make_column(seed, 10 + k, n, kinds[k], bool(nulls[k]), wide=shape[k] == 0, fine=shape[k] == 1) for k in range(nk)]
        check(lib, cols, [bool(f) for f in R.pick(seed, 5, nk, 2)], what=f"case {t}")
        seen |= set(kinds)
    assert seen == set(R.KINDS)


# ---------------------------------------------------------------- refusals
def test_refusals(lib):
    from pandasarrow_amd.column import Column

    h = lib.load()
    n = 8
    good = Column.from_numpy(np.arange(n, dtype=np.int64))
    out = Column.empty(lib.UINT64, n)

    def call(cols, m, nkeys=None):
        arr = (lib.PdxColumn * max(len(cols), 1))(*cols)
        info = lib.PdxSortInfo(9, 9, 9, 9)
        status = h.pdx_sort_indices(arr, len(cols) if nkeys is None else nkeys, None, C.byref(m), C.byref(info), None)
        return status, h.pdx_last_error().decode()

    assert call([], out.mut())[0] == lib.INVALID
    assert call([good.c()] * 17, out.mut())[0] == lib.INVALID
    assert call([good.c()] * 16, out.mut())[0] == lib.OK
    status, msg = call([good.c(), Column.from_numpy(np.ones(n, bool)).c()], out.mut())
    assert status == lib.NOT_IMPLEMENTED and "keys only" in msg
    status, msg = call([good.c(), Column.from_numpy(np.arange(n + 1, dtype=np.int64)).c()], out.mut())
    assert status == lib.INVALID and "same length" in msg
    status, msg = call([good.c()], Column.empty(lib.UINT64, n - 1).mut())
    assert status == lib.INVALID and "too small" in msg
    status, msg = call([good.c()], Column.empty(lib.INT64, n).mut())
    assert status == lib.INVALID and "uint64" in msg
    # more than 2^31-1 rows: descriptors with only the length set -- refused before anything is read or allocated
    big = 2**31
    key = lib.PdxColumn(lib.INT64, 0, big, 0, 0, None, None)
    status, msg = call([key, key], lib.PdxMutColumn(lib.UINT64, 0, big, -1, None, None))
    assert status == lib.NOT_IMPLEMENTED and "2^31-1" in msg


def test_empty_input_and_output_validity(lib):
    from pandasarrow_amd import column as K
    from pandasarrow_amd.column import Column

    empty = Column.from_numpy(np.zeros(0, np.float64))
    out, info = K.sort_indices([empty, empty], [False, True], with_info=True)
    assert out.length == 0 and info == (0, 0, 0)
    # an output validity bitmap is set to all ones
    n = 21
    key = Column.from_numpy(np.arange(n, dtype=np.int64)[::-1].copy())
    o = Column.empty(lib.UINT64, n, with_validity=True)
    m, kc = o.mut(), key.c()
    lib.check(lib.load().pdx_sort_indices(C.byref(kc), 1, None, C.byref(m), None, None))
    vals, valid = o._adopt(m).to_numpy()
    assert vals.tolist() == list(range(n - 1, -1, -1)) and valid.all() and m.null_count == 0


def test_argsort_still_refuses_narrow_columns(lib):
    """pdx_sort_indices widens int32 / float32 keys in its loader; pdx_argsort is not routed through it"""
    from pandasarrow_amd import column as K
    from pandasarrow_amd.column import Column

    c = Column.from_numpy(np.arange(5, dtype=np.int32), dtype=lib.INT32)
    with pytest.raises(lib.PdxError):
        K.argsort(c)
    assert K.sort_indices([c], [True]).to_numpy()[0].tolist() == [4, 3, 2, 1, 0]
