"""GPU tests of the 32-bit columns (PDX_INT32 / PDX_FLOAT32): every golden case of tools/gen_golden_narrow.py (Arrow 25) through the
C ABI, bit for bit, at offset 0 and at a non-zero offset; selection with mixed 4- and 8-byte columns; and the entry points outside the
feature, which must refuse a 4-byte column instead of reading it as 8-byte elements."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "narrow_golden.npz")
Z = np.load(GOLDEN)
CASES = json.loads(str(Z["manifest"]))["cases"]


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column as K

    assert torch.cuda.is_available()
    L.check(L.load().pdx_init(0))
    return L, K


def _dt(L, kind):
    return {"i32": L.INT32, "f32": L.FLOAT32, "i64": L.INT64, "f64": L.FLOAT64}[kind]


def _col(env, case, name, kind, offset):
    L, K = env
    a = Z[f"{case}/{name}"]
    return K.Column.from_numpy(a, Z[f"{case}/{name}_valid"], dtype=_dt(L, kind), offset=offset)


def _bits(v):
    v = np.asarray(v)
    return v.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize]) if v.dtype.kind == "f" else v.astype(np.int64)


def _check(got_col, case, exp_dtype_code, ulp=0):
    assert got_col.dtype == exp_dtype_code, (case, got_col.dtype, exp_dtype_code)
    got, ok = got_col.to_numpy()
    ok = np.ones(len(got), bool) if ok is None else ok
    ev, eok = Z[f"{case}/out"], Z[f"{case}/out_valid"]
    assert np.array_equal(ok, eok), case
    g, e = got[ok], ev[ok]
    if e.dtype.kind == "f":
        assert g.dtype == e.dtype, (case, g.dtype, e.dtype)
        if ulp:
            gb, eb = _bits(g).astype(np.int64), _bits(e).astype(np.int64)
            nan = np.isnan(e)
            assert np.array_equal(np.isnan(g), nan), case
            assert np.all(np.abs(gb[~nan] - eb[~nan]) <= ulp), case
        else:
            assert np.array_equal(_bits(g), _bits(e)), (case, g, e)
    else:
        assert np.array_equal(g.astype(np.int64), e.astype(np.int64)), (case, g, e)


def _out_code(L, kind, case):
    e = Z[f"{case}/out"]
    return {np.dtype(np.int32): L.INT32, np.dtype(np.float32): L.FLOAT32, np.dtype(np.int64): L.INT64, np.dtype(np.float64): L.FLOAT64,
            np.dtype(bool): L.BOOL}[e.dtype]


def _cases(kind):
    return sorted(k for k, c in CASES.items() if c["kind"] == kind)


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("case", _cases("binary"))
def test_binary(env, case, offset):
    L, K = env
    c = CASES[case]
    a, b = _col(env, case, "a", c["a"], offset), _col(env, case, "b", c["b"], offset)
    if c["error"]:
        with pytest.raises(L.PdxError) as ei:
            K.binary(c["op"], a, b, scalar=c["side"])
        assert str(ei.value) == c["error"]
        return
    _check(K.binary(c["op"], a, b, scalar=c["side"]), case, _out_code(L, "binary", case))


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("case", _cases("compare"))
def test_compare(env, case, offset):
    L, K = env
    c = CASES[case]
    a, b = _col(env, case, "a", c["a"], offset), _col(env, case, "b", c["b"], offset)
    if c["error"]:
        with pytest.raises(L.PdxError) as ei:
            K.compare(c["op"], a, b, scalar=c["side"])
        assert str(ei.value) == c["error"]
        return
    _check(K.compare(c["op"], a, b, scalar=c["side"]), case, L.BOOL)


@pytest.mark.parametrize("offset", [0, 7])
@pytest.mark.parametrize("case", _cases("if_else"))
def test_if_else(env, case, offset):
    L, K = env
    c = CASES[case]
    cond = K.Column.from_numpy(Z[f"{case}/cond"], Z[f"{case}/cond_valid"], offset=offset)
    a, b = _col(env, case, "a", c["a"], offset), _col(env, case, "b", c["b"], offset)
    n = cond.length
    out_dt = K.promote_dtype(a.dtype, b.dtype)
    out = K.Column.empty(out_dt, n, with_validity=True)
    cc, ca, cb, m = cond.c(), a.c(), b.c(), out.mut()
    rc = L.load().pdx_if_else(C.byref(cc), C.byref(ca), C.byref(cb), c["side"], C.byref(m), K._stream())
    if c["error"]:
        assert rc == L.INVALID and L.load().pdx_last_error().decode() == c["error"]
        return
    L.check(rc)
    _check(out._adopt(m), case, _out_code(L, "if_else", case))


@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("case", _cases("unary"))
def test_unary(env, case, offset):
    L, K = env
    c = CASES[case]
    a = _col(env, case, "a", c["a"], offset)
    r = K.unary(c["op"], a)
    if c["op"] == L.SIGN and c["a"] == "i32":
        want = L.INT64  # Arrow's int8 has no dtype here: the int64 path's answer
    else:
        want = _out_code(L, "unary", case)
    _check(r, case, want, ulp=2 if c["op"] == L.EXP else 0)


def _agg(L, K, kind, col):
    s = L.PdxScalar()
    ca = col.c()
    L.check(L.load().pdx_aggregate(kind, C.byref(ca), C.byref(s), K._stream()))
    return s


@pytest.mark.parametrize("offset", [0, 9])
@pytest.mark.parametrize("case", _cases("aggregate"))
def test_aggregate(env, case, offset):
    L, K = env
    c = CASES[case]
    a = _col(env, case, "a", c["a"], offset)
    narrow = _dt(L, c["a"])
    for name, kind in (("sum", L.AGG_SUM), ("mean", L.AGG_MEAN), ("min", L.AGG_MIN), ("max", L.AGG_MAX), ("count", L.AGG_COUNT)):
        s = _agg(L, K, kind, a)
        ev, eok = Z[f"{case}/out_{name}"], Z[f"{case}/out_{name}_valid"]
        assert bool(s.is_valid) == bool(eok[0]), (case, name)
        want_dt = {L.AGG_SUM: L.INT64 if narrow == L.INT32 else L.FLOAT64, L.AGG_MEAN: L.FLOAT64, L.AGG_COUNT: L.INT64}.get(kind, narrow)
        assert s.dtype == want_dt, (case, name, s.dtype)
        if not s.is_valid:
            continue
        if s.dtype in (L.FLOAT64, L.FLOAT32):
            got = np.float64(s.v.f64)
            e = np.float64(ev[0])
            assert _bits(np.array([got])) == _bits(np.array([e])) or (np.isnan(got) and np.isnan(e)), (case, name, got, e)
        else:
            assert s.v.i64 == int(ev[0]), (case, name, s.v.i64, ev[0])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", _cases("cast"))
def test_cast(env, case, offset):
    L, K = env
    c = CASES[case]
    a = _col(env, case, "a", c["a"], offset)
    if c["error"]:
        with pytest.raises(L.PdxError) as ei:
            K.cast(a, _dt(L, c["to"]))
        assert str(ei.value) == c["error"]
        return
    _check(K.cast(a, _dt(L, c["to"])), case, _dt(L, c["to"]))


@pytest.mark.parametrize("offset", [0, 6])
def test_concat_int32(env, offset):
    L, K = env
    case = "concat_i32"
    parts = [_col(env, case, f"p{i}", "i32", offset) for i in range(CASES[case]["parts"])]
    _check(K.concat(parts), case, L.INT32)


def test_concat_promotes_through_cast(env):
    L, K = env
    a = K.Column.from_numpy(np.array([1, 2], np.int32), dtype=L.INT32)
    b = K.Column.from_numpy(np.array([0.5], np.float32))
    r = K.concat([a, b])
    assert r.dtype == L.FLOAT32 and np.array_equal(r.to_numpy()[0], np.array([1, 2, 0.5], np.float32))


def _mixed_frame(L, K, rng, n, offset, nulls):
    host = [rng.integers(-2**31, 2**31, n).astype(np.int32), rng.standard_normal(n).astype(np.float32), rng.integers(-2**40, 2**40, n),
            rng.standard_normal(n), rng.integers(-5, 5, n).astype(np.int32)]
    valids = [(rng.random(n) > 0.2) if nulls else None for _ in host]
    dts = [L.INT32, L.FLOAT32, L.INT64, L.FLOAT64, L.INT32]
    cols = [K.Column.from_numpy(h, v, dtype=d, offset=offset) for h, v, d in zip(host, valids, dts)]
    return host, valids, cols


def _same(got_col, want, want_valid):
    got, ok = got_col.to_numpy()
    if want_valid is None:
        assert ok is None or ok.all()
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))
    else:
        assert np.array_equal(ok, want_valid)
        assert got.dtype == want.dtype and np.array_equal(_bits(got[ok]), _bits(want[ok]))


@pytest.mark.parametrize("n", [0, 1, 1000, 100_003])
@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("nulls", [False, True])
def test_filter_take_scatter_mixed_widths(env, n, offset, nulls):
    """one multi-column call over 4- and 8-byte columns"""
    L, K = env
    rng = np.random.default_rng(n + offset + nulls)
    host, valids, cols = _mixed_frame(L, K, rng, n, offset, nulls)
    mask = rng.random(n) > 0.4
    outs = K.filter(cols, K.Column.from_numpy(mask, offset=offset))
    for o, h, v in zip(outs, host, valids):
        _same(o, h[mask], None if v is None else v[mask])
    idx = rng.integers(0, max(n, 1), 777) if n else np.zeros(0, np.int64)
    outs = K.take(cols, K.Column.from_numpy(idx.astype(np.int64)))
    for o, h, v in zip(outs, host, valids):
        _same(o, h[idx], None if v is None else v[idx])
    perm = rng.permutation(n).astype(np.int64)
    dst = [K.Column.empty(c.dtype, n, with_validity=nulls) for c in cols]
    K.scatter(cols, K.Column.from_numpy(perm), dst)
    for o, h, v in zip(dst, host, valids):
        inv_h, inv_v = np.empty_like(h), np.ones(n, bool)
        inv_h[perm] = h
        if v is not None:
            inv_v[perm] = v
        _same(o, inv_h, None if v is None else inv_v)


def test_from_numpy_widths(env):
    L, K = env
    f = K.Column.from_numpy(np.array([1.5, np.nan], np.float32))
    assert f.dtype == L.FLOAT32 and f.to_numpy()[0].dtype == np.float32
    assert K.Column.from_numpy(np.array([1, 2], np.int32)).dtype == L.INT64  # (default: widened, as before)
    i = K.Column.from_numpy(np.array([1, 2], np.int32), dtype=L.INT32)
    assert i.dtype == L.INT32 and i.to_numpy()[0].dtype == np.int32
    from pandasarrow_amd import api

    s = api.Series(np.array([1.0, np.nan, 3.0], np.float32))
    assert s.dtype() == L.FLOAT32 and s.col.to_numpy()[1].tolist() == [True, False, True]  # NaN -> null at construction
    assert api.Series([1, 2, 3, 4, 5], dtype=L.INT32).dtype() == L.INT32
    big = K.binary(L.MUL, K.Column.from_numpy(np.array([65536], np.int32), dtype=L.INT32), K.Column.from_numpy(np.array([65536], np.int32), dtype=L.INT32))
    assert big.dtype == L.INT32 and big.to_numpy()[0].tolist() == [0]  # wraps at 32 bits
    two = K.binary(L.ADD, i, 2)  # a python int is an int64 scalar, as in pyarrow
    assert two.dtype == L.INT64 and two.to_numpy()[0].tolist() == [3, 4]


@pytest.mark.parametrize("n", [0, 1, 4097, 1_000_003])
def test_large_elementwise_against_numpy(env, n):
    """the 16-byte vector paths (aligned) and the row-per-lane paths (offset 1) over sizes with ragged tails"""
    L, K = env
    rng = np.random.default_rng(n)
    a = rng.integers(-2**31, 2**31, n).astype(np.int32)
    b = rng.integers(-2**31, 2**31, n).astype(np.int32)
    fa, fb = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    for off in (0, 1):
        ca, cb = K.Column.from_numpy(a, dtype=L.INT32, offset=off), K.Column.from_numpy(b, dtype=L.INT32, offset=off)
        assert np.array_equal(K.binary(L.ADD, ca, cb).to_numpy()[0], (a.astype(np.int64) + b).astype(np.int32))
        assert np.array_equal(K.compare(L.GT, ca, cb).to_numpy()[0], a > b)
        cf, cg = K.Column.from_numpy(fa, offset=off), K.Column.from_numpy(fb, offset=off)
        assert np.array_equal(_bits(K.binary(L.MUL, cf, cg).to_numpy()[0]), _bits(fa * fb))
        assert np.array_equal(K.compare(L.LE, cf, cg, scalar=False).to_numpy()[0], fa <= fb)
        assert np.array_equal(K.compare(L.LT, cf, K.Column.from_numpy(np.array([0.25], np.float32)), scalar=True).to_numpy()[0], fa < np.float32(0.25))


@pytest.mark.parametrize("n", [0, 1, 16, 4096, 4113, 1_000_000])
@pytest.mark.parametrize("nulls", [False, True])
def test_float32_sum_against_oracle(env, n, nulls):
    """sum / mean of float32 == the oracle's float64 pairwise tree over the widened values"""
    import oracle as orc

    L, K = env
    rng = np.random.default_rng(n)
    v = (rng.random(n) * 100).astype(np.float32)
    valid = (rng.random(n) > 0.05) if nulls else None
    col = K.Column.from_numpy(v, valid, offset=5)
    for kind in (L.AGG_SUM, L.AGG_MEAN):
        got, cnt = K.aggregate(kind, col)
        want, wcnt = orc.agg(kind, v.astype(np.float64), valid)
        assert cnt == wcnt and (got is None) == (want is None)
        if got is not None:
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (kind, got, want)


def test_float32_sum_2pow30_rows(env):
    """~1.07e9 float32 rows.  2^30 rows are 2^26 full 16-row leaves, so Arrow's tree is the balanced one: the sum is the balanced
    combination of the oracle's sums of the 8 aligned 2^27-row chunks (the host never holds the whole column as float64)"""
    import oracle as orc
    import torch

    L, K = env
    n, chunk = 1 << 30, 1 << 27
    dev = torch.empty(n, dtype=torch.float32, device="cuda")
    part = []
    for q in range(n // chunk):
        v = (np.random.default_rng(100 + q).random(chunk, dtype=np.float32) * 10).astype(np.float32)
        dev[q * chunk:(q + 1) * chunk].copy_(torch.from_numpy(v))
        part.append(orc.agg(L.AGG_SUM, v.astype(np.float64))[0])
    while len(part) > 1:
        part = [part[i] + part[i + 1] for i in range(0, len(part), 2)]
    got, cnt = K.aggregate(L.AGG_SUM, K.Column(L.FLOAT32, n, dev))
    assert cnt == n and np.float64(got).view(np.uint64) == np.float64(part[0]).view(np.uint64), (got, part[0])
    del dev
    torch.cuda.empty_cache()


def test_entry_points_outside_the_feature_refuse_32_bit_columns(env):
    L, K = env
    lib = L.load()
    st = K._stream()
    i32 = K.Column.from_numpy(np.arange(64, dtype=np.int32), dtype=L.INT32)
    f32 = K.Column.from_numpy(np.arange(64, dtype=np.float32))
    i64 = K.Column.from_numpy(np.arange(64))
    out = K.Column.empty(L.INT64, 64, with_validity=True)
    ci, cf, c64, m = i32.c(), f32.c(), i64.c(), out.mut()

    def refused(rc, what):
        assert rc == L.NOT_IMPLEMENTED, (what, rc)
        msg = lib.pdx_last_error().decode()
        assert "int32" in msg or "float32" in msg, (what, msg)

    refused(lib.pdx_argsort(C.byref(ci), 1, C.byref(m), st), "argsort")
    refused(lib.pdx_index_union(C.byref(ci), C.byref(ci), 1, C.byref(m), st), "index_union")
    refused(lib.pdx_index_intersection(C.byref(ci), C.byref(ci), C.byref(m), st), "index_intersection")
    refused(lib.pdx_reindex_indices(C.byref(ci), C.byref(c64), C.byref(m), st), "reindex")
    refused(lib.pdx_power(C.byref(cf), 2.0, C.byref(m), st), "power")
    gb = C.c_void_p()
    refused(lib.pdx_groupby_create(C.byref(ci), st, C.byref(gb)), "groupby_create")
    with pytest.raises(L.PdxError) as ei:
        K.GroupByHandle.create(i64).agg(f32, [L.AGG_SUM])
    assert ei.value.status == L.NOT_IMPLEMENTED
    h = C.c_void_p()
    refused(lib.pdx_groupby_sum_mean_count_chunked(C.byref(ci), C.byref(cf), 16, st, C.byref(h)), "chunked")
    kinds = (C.c_int * 1)(L.AGG_MIN)
    refused(lib.pdx_groupby_order_free_chunked(C.byref(c64), C.byref(cf), kinds, 1, 16, st, C.byref(h)), "order_free_chunked")
    refused(lib.pdx_resample_create(C.byref(ci), 10, 0, 0, L.ORIGIN_START_DAY, 0, 0, st, C.byref(gb)), "resample")
    refused(lib.pdx_downsample_create(C.byref(ci), 1, L.UNIT_SECOND, 0, 1, 0, 0, st, C.byref(gb)), "downsample")
    g64 = K.GroupByHandle.create(i64)
    grouped = C.c_void_p()
    refused(lib.pdx_groupby_group_values(g64._h, C.byref(cf), st, C.byref(grouped)), "group_values (the partial-tree entry)")
    refused(lib.pdx_groupby_bind(g64._h, C.byref(cf), st), "groupby_bind")
    from pandasarrow_amd import dist as pdist

    cd = pdist.CDist("rccl")  # world size 1
    try:
        refused(lib.pdx_dist_concat(cd._h, C.byref(cf), C.byref(m), st), "dist_concat")
    finally:
        cd.close()


def test_series_facade_with_narrow_columns(env):
    """reindex with a fill value keeps the 4-byte width (or refuses a fill of another kind); a 4-byte index compares as 4-byte labels"""
    L, K = env
    from pandasarrow_amd import api

    idx = K.Column.from_numpy(np.array([10, 20, 30, 40]))
    s = api.Series(np.array([1, 2, 3, 4], np.int32), index=idx, dtype=L.INT32)
    r = s.reindex(K.Column.from_numpy(np.array([20, 99, 40])), fill_value=7)
    assert r.dtype() == L.INT32 and r.col.values.dtype.itemsize == 4
    assert r.col.to_numpy()[0].tolist() == [2, 7, 4]
    assert (r + r).col.to_numpy()[0].tolist() == [4, 14, 8]  # later kernels read the buffer at its real width
    with pytest.raises(L.PdxError, match="Cannot append scalar of type int64 to builder for type int32"):
        s.reindex(K.Column.from_numpy(np.array([99])), fill_value=2**31)
    f = api.Series(np.array([0.5, 1.5], np.float32), index=K.Column.from_numpy(np.array([1, 2])))
    rf = f.reindex(K.Column.from_numpy(np.array([2, 3])), fill_value=0.25)
    assert rf.dtype() == L.FLOAT32 and rf.col.to_numpy()[0].tolist() == [1.5, 0.25]
    with pytest.raises(L.PdxError, match="type int64 to builder for type float"):
        f.reindex(K.Column.from_numpy(np.array([3])), fill_value=1)
    # a float32 index: equal labels compare as 4-byte patterns (an 8-byte view would read past the buffer)
    fidx = K.Column.from_numpy(np.array([0.5, 1.5, 2.5], np.float32))
    a = api.Series(np.array([1.0, 2.0, 3.0]), index=fidx)
    b = api.Series(np.array([10.0, 20.0, 30.0]), index=K.Column.from_numpy(np.array([0.5, 1.5, 2.5], np.float32)))
    assert (a + b).col.to_numpy()[0].tolist() == [11.0, 22.0, 33.0]
    c = api.Series(np.array([10.0, 20.0, 30.0]), index=K.Column.from_numpy(np.array([0.5, 1.5, 3.5], np.float32)))
    with pytest.raises(L.PdxError) as ei:  # aligning unequal 4-byte indexes is not built: refused, not misread
        a + c
    assert ei.value.status == L.NOT_IMPLEMENTED
    # construction refuses what an int32 array cannot hold
    for bad in ([1.5], [2**31], [np.nan]):
        with pytest.raises(L.PdxError, match="int32"):
            api.Series(bad, dtype=L.INT32)
    assert api.Series([1.0, -2.0], dtype=L.INT32).col.to_numpy()[0].tolist() == [1, -2]
    # frame mean over 4-byte columns: values widened exactly, as Arrow's mean
    df = api.DataFrame({"x": api.Series(np.array([1, 2, 4], np.int32), dtype=L.INT32), "y": api.Series(np.array([8, 16, 32], np.int32), dtype=L.INT32)})
    assert df.mean().value == 63 / 6
