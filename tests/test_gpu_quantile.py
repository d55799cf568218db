"""GPU: pdx_quantile / pdx_groupby_quantile through the C ABI and the Python facade, against tests/golden/quantile_golden.npz (Arrow C++ 25)
and the numpy restatement tests/_quantile_ref.py.  Everything is bit-exact; a NaN result is compared as "is NaN".  No pyarrow."""
import ctypes as C

import numpy as np
import pytest

import _quantile_ref as R

pytestmark = pytest.mark.gpu

GOLD = R.QuantileGolden()
DTS = ("i64", "u64", "f64", "i32", "f32")


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


def result_dtype(dt, interp):
    return np.float64 if interp in ("linear", "midpoint") else R.NP_DTYPES[dt]


def call(env, col, qs, interp, skip=1, min_count=0, stream=None):
    """one pdx_quantile call -> (status, values | message, is_valid, counts)"""
    L = env.L
    qarr = (C.c_double * max(len(qs), 1))(*qs)
    outs = (L.PdxScalar * max(len(qs), 1))()
    ca = col.c()
    rc = env.lib.pdx_quantile(C.byref(ca), qarr, len(qs), R.INTERPOLATIONS.index(interp), int(skip), int(min_count), outs, env.K._stream() if stream is None else stream)
    if rc != L.OK:
        return rc, env.lib.pdx_last_error().decode(), None, None
    np_dt = {L.FLOAT64: np.float64, L.FLOAT32: np.float32, L.INT64: np.int64, L.INT32: np.int32, L.UINT64: np.uint64}
    vals, ok, counts = [], [], []
    for s in outs[:len(qs)]:
        ok.append(bool(s.is_valid))
        counts.append(int(s.count))
        vals.append(s.v.f64 if s.dtype in (L.FLOAT64, L.FLOAT32) else s.v.u64 if s.dtype == L.UINT64 else s.v.i64)
    dt = np_dt[outs[0].dtype]
    return rc, np.array(vals, np.float64).astype(dt) if dt in (np.float64, np.float32) else np.array(vals, dt), np.array(ok, bool), counts


def check_against_ref(env, a, valid, dt, qs, interp, skip=1, min_count=0, offset=0):
    rc, got, ok, counts = call(env, column(env, a, valid, dt, offset=offset), qs, interp, skip, min_count)
    assert rc == env.L.OK, got
    want, want_ok, n = R.quantile(a, valid, qs, interp, bool(skip), min_count)
    assert got.dtype == want.dtype
    assert counts == [n] * len(qs)
    assert R.same(got, ok, R.bits(want), want_ok), (dt, interp, len(a))
    return got, ok


@pytest.mark.parametrize("interp", R.INTERPOLATIONS)
@pytest.mark.parametrize("dt", DTS)
def test_golden_through_the_abi(env, dt, interp):
    for c in (c for c in GOLD.cases if c["kind"] == "column" and c["dtype"] == dt and c["interpolation"] == interp):
        a, valid = GOLD.inputs(c)
        want, want_ok = GOLD.expected(c)
        rc, got, ok, _ = call(env, column(env, a, None if valid.all() else valid, dt), c["q"], interp, c["skip_nulls"], c["min_count"])
        assert rc == env.L.OK, got
        assert got.dtype == result_dtype(dt, interp)
        assert R.same(got, ok, want, want_ok), c["name"]


@pytest.mark.parametrize("interp", R.INTERPOLATIONS)
@pytest.mark.parametrize("dt", DTS)
def test_golden_through_the_facade(env, dt, interp):
    """EVERY golden column case through api.Series.quantile with the case's own skip_nulls / min_count, by keyword and by position"""
    cases = [c for c in GOLD.cases if c["kind"] == "column" and c["dtype"] == dt and c["interpolation"] == interp]
    assert len(cases) >= 100
    for i, c in enumerate(cases):
        a, valid = GOLD.inputs(c)
        want, want_ok = GOLD.expected(c)
        s = env.api.Series(column(env, a, None if valid.all() else valid, dt))
        if i % 2:
            res = s.quantile(c["q"], interp, bool(c["skip_nulls"]), c["min_count"])
        else:
            res = s.quantile(q=c["q"], min_count=c["min_count"], skip_nulls=bool(c["skip_nulls"]), interpolation=interp)
        got = np.array([0 if r.value is None else r.value for r in res], result_dtype(dt, interp))
        assert R.same(got, [r.isValid() for r in res], want, want_ok), c["name"]
        one = s.quantile(c["q"][-1], interp, bool(c["skip_nulls"]), c["min_count"])  # a single q gives a single Scalar
        assert one.isValid() == bool(want_ok[-1])
        assert not one.isValid() or R.same(np.array([one.value], got.dtype), [True], want[-1:], [True]), c["name"]


def test_frame_quantile_by_column_name(env):
    a, b = np.arange(5, dtype=np.int64), np.array([4.0, 5.0, 6.0, 7.0, np.nan])
    df = env.api.DataFrame({"a": column(env, a, np.array([1, 1, 1, 1, 0], bool), "i64"), "b": column(env, b, None, "f64")})
    r = df.quantile(0.5)
    assert r["a"].value == 1.5 and r["b"].value == 5.5
    r = df.quantile(0.5, "lower", False, 0)  # skip_nulls = False: the column with a null is null, the other is not
    assert not r["a"].isValid() and r["b"].value == 5.0
    r = df.quantile(0.5, "higher", True, 5)  # min_count = 5 non-null rows (NaN rows count): only b has them
    assert not r["a"].isValid() and r["b"].value == 6.0
    r = df.quantile([0.0, 1.0], interpolation="nearest")
    assert [x.value for x in r["a"]] == [0, 3] and [x.value for x in r["b"]] == [4.0, 7.0]


def test_errors(env):
    L = env.L
    for c in (c for c in GOLD.cases if c["kind"] == "error"):
        a = np.array([1, 2], np.int64) if c["dtype"] in ("i64", "ts") else np.array([True, False]) if c["dtype"] == "bool" else np.array([1.0, 2.0])
        rc, msg, _, _ = call(env, column(env, a, None, c["dtype"]), c["q"], "linear")
        assert rc == (L.INVALID if c["status"] == "invalid" else L.NOT_IMPLEMENTED)
        assert msg == c["error"]
    rc, msg, _, _ = call(env, column(env, np.array([1.0]), None, "f64"), [float("nan")], "linear")
    assert (rc, msg) == (L.INVALID, "Quantile must be between 0 and 1")
    with pytest.raises(L.PdxError):
        env.api.Series(column(env, np.array([1.0]), None, "f64")).quantile(0.5, interpolation="cubic")


def test_both_zeros_keep_their_row_order(env):
    """this backend's rule (not Arrow's): the zero that comes first in pdx_argsort's stable order"""
    a = np.array([-0.0, 0.0, -0.0, 1.0, 0.0, -1.0])
    want, _, _ = R.quantile(a, None, [0.2, 0.4, 0.6, 0.8], "lower")
    assert list(np.signbit(want)) == [True, False, True, False]
    for dt in ("f64", "f32"):
        got, _ = check_against_ref(env, a.astype(R.NP_DTYPES[dt]), None, dt, [0.0, 0.2, 0.4, 0.6, 0.8, 1.0], "lower")
        assert list(np.signbit(got)) == [True, True, False, True, False, False]
    rng = np.random.default_rng(5)
    big = np.where(rng.random(300_000) < 0.5, -0.0, 0.0)
    big[rng.integers(0, len(big), 1000)] = rng.standard_normal(1000)
    valid = rng.random(len(big)) > 0.1
    for interp in ("lower", "higher", "nearest"):
        check_against_ref(env, big, valid, "f64", [0.1, 0.3, 0.5, 0.77, 0.9], interp)


@pytest.mark.parametrize("n", [1_000_000, 10_000_000])
@pytest.mark.parametrize("dt", DTS)
def test_random_against_the_restatement(env, dt, n):
    rng = np.random.default_rng(n % 1000 + len(dt))
    if dt in ("f64", "f32"):
        a = rng.standard_normal(n).astype(R.NP_DTYPES[dt])
        a[rng.integers(0, n, 100)] = np.nan
    elif dt == "u64":
        a = rng.integers(0, 2**64, n, dtype=np.uint64)
    else:
        info = np.iinfo(R.NP_DTYPES[dt])
        a = rng.integers(info.min, info.max, n, dtype=R.NP_DTYPES[dt])
    valid = rng.random(n) > 0.06
    qs = [0.0, 1.0, 0.5, 0.25, 1 / 3, 0.999, 0.001]
    for interp in R.INTERPOLATIONS:
        check_against_ref(env, a, valid if interp != "higher" else None, dt, qs, interp)


@pytest.mark.parametrize("shape", ["constant", "two_values", "low_bits", "sorted", "reverse", "half_nan", "mostly_null"])
def test_adversarial_distributions(env, shape):
    n = 3_000_001
    rng = np.random.default_rng(11)
    valid = None
    if shape == "constant":
        a = np.full(n, 3.25)
    elif shape == "two_values":
        a = np.where(rng.random(n) < 0.5, 1.0, np.nextafter(1.0, 2.0))
    elif shape == "low_bits":
        a = (np.float64(1.0).view(np.uint64) + rng.integers(0, 7, n).astype(np.uint64)).view(np.float64)
    elif shape == "sorted":
        a = np.sort(rng.standard_normal(n))
    elif shape == "reverse":
        a = np.sort(rng.standard_normal(n))[::-1].copy()
    elif shape == "half_nan":
        a = rng.standard_normal(n)
        a[rng.random(n) < 0.5] = np.nan
    else:
        a = rng.standard_normal(n)
        valid = rng.random(n) < 0.1
    qs = [0.0, 0.5, 1 / 3, 0.9999, 1.0]
    for interp in ("linear", "nearest", "midpoint"):
        check_against_ref(env, a, valid, "f64", qs, interp)
    if shape in ("constant", "two_values", "low_bits"):
        i = a.view(np.int64)
        check_against_ref(env, i, valid, "i64", qs, "linear")
        check_against_ref(env, (i >> 29).astype(np.int32), valid, "i32", qs, "higher")


def test_64_quantiles_in_one_call_equal_64_calls(env):
    rng = np.random.default_rng(3)
    a = rng.standard_normal(2_000_000)
    col = column(env, a, rng.random(len(a)) > 0.05, "f64")
    qs = [float(x) for x in rng.random(64)]
    for interp in ("linear", "nearest"):
        rc, got, ok, _ = call(env, col, qs, interp)
        assert rc == env.L.OK and ok.all()
        for k in range(64):
            rc, one, _, _ = call(env, col, [qs[k]], interp)
            assert rc == env.L.OK and R.bits(one)[0] == R.bits(got)[k]
    rc, base, _, _ = call(env, col, qs, "linear")
    rc, many, ok, _ = call(env, col, qs + qs + [0.5], "linear")  # more than one read's worth
    assert rc == env.L.OK and ok.all() and np.array_equal(R.bits(many)[:64], R.bits(base)) and np.array_equal(R.bits(many)[64:128], R.bits(base))


@pytest.mark.parametrize("dt", ["f64", "i32"])
def test_offsets_streams_repeats_and_unknown_null_count(env, dt):
    rng = np.random.default_rng(8)
    n = 200_000
    a = rng.integers(-10**6, 10**6, n + 16).astype(R.NP_DTYPES[dt])
    valid = rng.random(n + 16) > 0.2
    qs = [0.5, 0.123, 0.9]
    whole = column(env, a, valid, dt)
    for off in range(0, 9):
        sl = whole.slice(off, n - 3 * off)
        rc, got, ok, counts = call(env, sl, qs, "linear")
        want, want_ok, cnt = R.quantile(a[off:off + n - 3 * off], valid[off:off + n - 3 * off], qs, "linear")
        assert rc == env.L.OK and counts == [cnt] * 3 and R.same(got, ok, R.bits(want), want_ok), off
    sl = whole.slice(5, n)
    rc, first, _, _ = call(env, sl, qs, "linear")
    rc, again, _, _ = call(env, sl, qs, "linear")
    assert np.array_equal(R.bits(first), R.bits(again))
    s2 = env.torch.cuda.Stream()
    env.torch.cuda.synchronize()
    rc, other, _, _ = call(env, sl, qs, "linear", stream=s2.cuda_stream)
    assert rc == env.L.OK and np.array_equal(R.bits(first), R.bits(other))
    assert sl.null_count == -1  # (a slice does not know its null count: every call above ran with -1)
    sl.null_count = int((~valid[5:5 + n]).sum())
    rc, known, _, _ = call(env, sl, qs, "linear")
    assert rc == env.L.OK and np.array_equal(R.bits(first), R.bits(known))
    dense = column(env, a, None, dt)  # null_count 0 with validity == NULL
    assert dense.validity is None
    check_against_ref(env, a, None, dt, qs, "midpoint")


def group_call(env, gb, col, qs, interp, skip=1, min_count=0):
    outs = gb.quantile(col, qs, interp, bool(skip), min_count)
    res = []
    for o in outs:
        v, ok = o.to_numpy()
        res.append((v, np.ones(len(v), bool) if ok is None else ok, o.null_count))
    return res


@pytest.mark.parametrize("dt", ["f64", "i64", "u64"])
def test_golden_groups(env, dt):
    handles = {}
    for c in (c for c in GOLD.cases if c["kind"] == "group" and c["dtype"] == dt):
        a, valid = GOLD.inputs(c)
        keys = GOLD.keys(c)
        if c["keys"] not in handles:
            handles[c["keys"]] = env.K.GroupByHandle.create(column(env, keys, None, "i64"))
        gb = handles[c["keys"]]
        want, want_ok = GOLD.expected(c)
        (got, ok, nulls), = group_call(env, gb, column(env, a, valid, dt), c["q"], c["interpolation"], c["skip_nulls"], c["min_count"])
        assert got.dtype == result_dtype(dt, c["interpolation"])
        assert nulls == int((~want_ok).sum())
        assert R.same(got, ok, want, want_ok), c["name"]


@pytest.mark.parametrize("dt", ["f64", "i64", "u64"])
def test_golden_groups_through_the_facade(env, dt):
    """EVERY golden group case through api.DataFrame.group_by(...).quantile with the case's own options: one column -> Series, and the
    list form -> DataFrame in which column args[i] uses qs[i]"""
    frames = {}
    cases = [c for c in GOLD.cases if c["kind"] == "group" and c["dtype"] == dt]
    assert len(cases) == 135
    for i, c in enumerate(cases):
        if c["keys"] not in frames:
            a, valid = GOLD.inputs(c)
            df = env.api.DataFrame({"k": column(env, GOLD.keys(c), None, "i64"), "v": column(env, a, valid, dt), "w": column(env, a, valid, dt)})
            frames[c["keys"]] = (df.group_by("k"), R.group_ids(GOLD.keys(c))[1])
        g, uniq = frames[c["keys"]]
        want, want_ok = GOLD.expected(c)
        interp, skip, mc, q = c["interpolation"], bool(c["skip_nulls"]), c["min_count"], c["q"][0]
        s = g.quantile("v", q, interp, skip, mc) if i % 2 else g.quantile("v", q=q, min_count=mc, skip_nulls=skip, interpolation=interp)
        v, ok = s.col.to_numpy()
        assert v.dtype == result_dtype(dt, interp) and s.name == "v"
        assert R.same(v, np.ones(len(v), bool) if ok is None else ok, want, want_ok), c["name"]
        assert np.array_equal(s.index.to_numpy()[0], uniq)
        if i % 9 == 0:  # the paired form: "w" takes this case's q, "v" another one
            f = g.quantile(["v", "w"], [0.0, q], interp, skip, mc)
            v, ok = f["w"].col.to_numpy()
            assert R.same(v, np.ones(len(v), bool) if ok is None else ok, want, want_ok), c["name"]
            a, valid = GOLD.inputs(c)
            w0, w0_ok = R.group_quantile(GOLD.keys(c), a, valid, 0.0, interp, skip, mc)
            v, ok = f["v"].col.to_numpy()
            assert R.same(v, np.ones(len(v), bool) if ok is None else ok, R.bits(w0), w0_ok), c["name"]


def test_groups_equal_the_whole_column_call_on_each_groups_rows(env):
    rng = np.random.default_rng(21)
    n, G = 200_000, 37
    keys = rng.integers(0, G, n).astype(np.int64)
    a = rng.standard_normal(n)
    a[rng.random(n) < 0.01] = np.nan
    valid = rng.random(n) > 0.1
    kcol, vcol = column(env, keys, None, "i64"), column(env, a, valid, "f64")
    gb = env.K.GroupByHandle.create(kcol)
    rows, offsets = gb.groupings()
    offsets = offsets.cpu().numpy()
    qs = [0.5, 0.05, 1.0]
    plan_before = gb.last_plan()
    for interp in ("linear", "lower", "nearest"):
        res = group_call(env, gb, vcol, qs, interp)
        for g in range(gb.num_groups):
            idx = env.K.Column(env.L.INT64, int(offsets[g + 1] - offsets[g]), rows[offsets[g]:offsets[g + 1]].contiguous())
            taken, = env.K.take([vcol], idx)
            rc, one, ok, _ = call(env, taken, qs, interp)
            assert rc == env.L.OK
            for k in range(len(qs)):
                assert bool(res[k][1][g]) == bool(ok[k])
                assert not ok[k] or R.bits(res[k][0][g:g + 1])[0] == R.bits(one[k:k + 1])[0]
    assert gb.last_plan() == plan_before and gb.bound_bytes() == 0
    # facade: Series for one column, DataFrame pairing args[i] with qs[i]; a Resampler inherits both
    df = env.api.DataFrame({"k": kcol, "v": vcol, "w": column(env, keys * 2, None, "i64")})
    g = df.group_by("k")
    s = g.quantile("v", 0.5)
    want, want_ok = R.group_quantile(keys, a, valid, 0.5)
    v, ok = s.col.to_numpy()
    assert R.same(v, np.ones(len(v), bool) if ok is None else ok, R.bits(want), want_ok)
    f = g.quantile(["v", "w"], [0.25, 0.75], interpolation="higher")
    want, want_ok = R.group_quantile(keys, keys * 2, None, 0.75, "higher")
    v, ok = f["w"].col.to_numpy()
    assert R.same(v, np.ones(len(v), bool) if ok is None else ok, R.bits(want), want_ok)
    with pytest.raises(env.L.PdxError):
        g.quantile(["v", "w"], [0.5])
    ts = np.arange(1000, dtype=np.int64) * 60_000_000_000
    rs = env.api.DataFrame({"x": column(env, np.arange(1000.0), None, "f64")}, index=column(env, ts, None, "ts")).resample("60T")
    v, _ = rs.quantile("x", 0.5).col.to_numpy()
    assert v[0] == 29.5 and v[1] == 89.5
    # (narrow values stay refused by every group-by call)
    with pytest.raises(env.L.PdxError) as e:
        gb.quantile(column(env, keys.astype(np.int32), None, "i32"), [0.5])
    assert e.value.status == env.L.NOT_IMPLEMENTED
