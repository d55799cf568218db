"""GPU: the dt accessor -- pdx_temporal_components, pdx_temporal_between and round-to-nearest -- bit-exact against Arrow C++ 25
(tests/golden/temporal_golden.npz) and, for inputs the file does not hold, against tests/_temporal_ref.py, which
tests/test_temporal_golden.py holds to the same file."""
import ctypes as C
import os

import numpy as np
import pytest

import _temporal_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "temporal_golden.npz"))
ROUND_CASES = sorted({k.split("_", 2)[2] for k in G.files if k.startswith("round_")})
# 4 * 256 * 3 + 5: the tail of k_round_temporal's four-in-flight loop; + 64 more: the first length at which a wave of the component kernels
# (whose four batches must be whole 64-row words) takes its four-in-flight loop while its neighbours finish a ragged word in the tail loop
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1027, 4 * 256 * 3 + 5, 4 * 256 * 3 + 64 + 5]
SINGLE = [c for c in R.COMPONENTS if c != "week"]


@pytest.fixture(scope="module")
def px():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column as K

    L.check(L.load().pdx_init(0))

    class P:
        pass

    P.L, P.K, P.api, P.Column, P.torch = L, K, api, K.Column, torch
    return P


def tc(px, name):
    return getattr(px.L, "TC_" + name.upper())


def ts_col(px, ts, valid=None, offset=0):
    return px.Column.from_numpy(np.asarray(ts, np.int64), valid=valid, dtype=px.L.TIMESTAMP_NS, offset=offset)


def same_bits(got, exp):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8))


@pytest.fixture(scope="module")
def golden_ts(px):
    return ts_col(px, G["ts"]), ts_col(px, G["b_ts"]), ts_col(px, G["r_ts"])


@pytest.fixture(scope="module")
def ref_components():
    """every single component of the golden instants by the restatement, computed once (for slices and lengths)"""
    return {c: R.component(c, G["ts"]) for c in SINGLE}


# ------------------------------------------------------------------ against the golden file
@pytest.mark.parametrize("name", SINGLE)
def test_component_golden(px, golden_ts, name):
    (out,) = px.K.temporal_components(golden_ts[0], [tc(px, name)])
    vals, valid = out.to_numpy()
    assert valid is None and out.null_count == 0
    same_bits(vals, G["comp_" + name])


@pytest.mark.parametrize("opts", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
def test_week_options_golden(px, golden_ts, opts):
    (out,) = px.K.temporal_components(golden_ts[0], [px.L.TC_WEEK], opts)
    same_bits(out.to_numpy()[0], G["week_%d%d%d" % opts])


def test_week_default_options_are_iso(px, golden_ts):
    same_bits(px.K.temporal_components(golden_ts[0], [px.L.TC_WEEK])[0].to_numpy()[0], G["comp_iso_week"])


@pytest.mark.parametrize("unit", R.BETWEEN_UNITS)
def test_between_golden(px, golden_ts, unit):
    out = px.K.temporal_between(R.UNITS.index(unit), golden_ts[0], golden_ts[1])
    vals, valid = out.to_numpy()
    assert valid is None and out.dtype == px.L.INT64
    same_bits(vals, G["between_" + unit])


@pytest.mark.parametrize("case", ROUND_CASES)
def test_round_golden(px, golden_ts, case):
    unit, mult, wsm, cbo = case.split("_")
    for how, kw in (("floor", {}), ("ceil", {"ceil": True}), ("round", {"nearest": True})):
        out = px.K.round_temporal(golden_ts[2], int(mult), R.UNITS.index(unit), week_starts_monday=bool(int(wsm)), calendar_based_origin=bool(int(cbo)), **kw)
        assert out.dtype == px.L.TIMESTAMP_NS
        same_bits(out.to_numpy()[0], G[f"round_{how}_{case}"])


# ------------------------------------------------------------------ lengths, slices, nulls
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(px, ref_components, n):
    """every output dtype (int64 / bool / float64) at every length, single and fused, plus between and nearest"""
    ts, b = np.resize(G["ts"], n), np.resize(G["b_ts"], n)  # (the golden instants, repeated where n is larger)
    T, B = ts_col(px, ts), ts_col(px, b)
    names = ["iso_week", "is_leap_year", "subsecond", "day", "hour"]
    fused = px.K.temporal_components(T, [tc(px, c) for c in names])
    for c, out in zip(names, fused):
        assert out.length == n
        same_bits(out.to_numpy()[0], np.resize(ref_components[c], n))
        same_bits(px.K.temporal_components(T, [tc(px, c)])[0].to_numpy()[0], np.resize(ref_components[c], n))
    same_bits(px.K.temporal_between(px.L.UNIT_DAY, T, B).to_numpy()[0], np.resize(G["between_day"], n))
    r = np.resize(G["r_ts"], n)
    same_bits(px.K.round_temporal(ts_col(px, r), 1, px.L.UNIT_HOUR, nearest=True).to_numpy()[0], np.resize(G["round_round_hour_1_1_0"], n))


@pytest.mark.parametrize("offset", [3, 13])
@pytest.mark.parametrize("nulls", ["none", "some", "all"])
def test_slices_and_nulls(px, ref_components, offset, nulls):
    """a value offset and a validity bit offset that is not byte aligned, with int64, bool and float64 outputs"""
    n = 1027
    ts, b = G["ts"][:n], G["b_ts"][:n]
    rng = np.random.default_rng(offset)
    valid = {"none": None, "some": rng.random(n) < 0.7, "all": np.zeros(n, bool)}[nulls]
    vb = None if valid is None else np.roll(valid, 5)
    T, B = ts_col(px, ts, valid, offset), ts_col(px, b, vb, offset)
    names = ["year", "is_leap_year", "subsecond", "us_week"]
    for outs in (px.K.temporal_components(T, [tc(px, c) for c in names]), [px.K.temporal_components(T, [tc(px, c)])[0] for c in names]):
        for c, out in zip(names, outs):
            vals, ok = out.to_numpy()
            if valid is None:
                assert ok is None
                same_bits(vals, ref_components[c][:n])
            else:
                assert np.array_equal(ok, valid)
                same_bits(vals[valid], ref_components[c][:n][valid])
    vals, ok = px.K.temporal_between(px.L.UNIT_WEEK, T, B).to_numpy()
    both = np.ones(n, bool) if valid is None else valid & vb
    assert (ok is None) if valid is None else np.array_equal(ok, both)
    same_bits(vals[both], G["between_week"][:n][both])
    vals, ok = px.K.round_temporal(T, 1, px.L.UNIT_DAY, nearest=True).to_numpy()
    keep = np.ones(n, bool) if valid is None else valid
    assert (ok is None) if valid is None else np.array_equal(ok, valid)
    same_bits(vals[keep], R.round_temporal(ts, 1, "day")[keep])


# ------------------------------------------------------------------ fused calls
@pytest.mark.parametrize("names", [["minute"], ["year", "month", "day"], ["iso_year", "iso_week", "iso_day_of_week"], ["hour", "is_leap_year", "subsecond"],
                                   ["day_of_week", "iso_day_of_week"], ["year", "quarter", "is_leap_year", "hour", "subsecond", "iso_week", "us_year", "week"]])
def test_fused_equals_single_calls(px, golden_ts, names):
    opts = (0, 1, 1)
    fused = px.K.temporal_components(golden_ts[0], [tc(px, c) for c in names], opts)
    assert len(fused) == len(names)
    for c, out in zip(names, fused):
        single = px.K.temporal_components(golden_ts[0], [tc(px, c)], opts)[0]
        assert out.dtype == single.dtype == px.K.temporal_component_dtype(tc(px, c))
        same_bits(out.to_numpy()[0], single.to_numpy()[0])
        same_bits(out.to_numpy()[0], G["week_011"] if c == "week" else G["comp_" + c])


def test_random_instants_against_restatement(px):
    rng = np.random.default_rng(7)
    lo, hi = np.iinfo(np.int64).min + 1, np.iinfo(np.int64).max
    ts = rng.integers(lo, hi, 200_000, endpoint=True)
    b = ts // 2 + rng.integers(-10**17, 10**17, len(ts))
    T, B = ts_col(px, ts), ts_col(px, b)
    for chunk in (SINGLE[:8], SINGLE[8:16], SINGLE[16:]):
        for c, out in zip(chunk, px.K.temporal_components(T, [tc(px, c) for c in chunk])):
            same_bits(out.to_numpy()[0], R.component(c, ts))
    same_bits(px.K.temporal_components(T, [px.L.TC_WEEK], (0, 0, 1))[0].to_numpy()[0], R.week(ts, False, False, True))
    for unit in R.BETWEEN_UNITS:
        same_bits(px.K.temporal_between(R.UNITS.index(unit), T, B).to_numpy()[0], R.between(unit, ts, b))
    mid = ts // 2  # (far enough from the ends of the range for every ceil)
    M = ts_col(px, mid)
    for unit, mult in (("minute", 15), ("day", 1), ("week", 1), ("month", 1), ("quarter", 2)):
        same_bits(px.K.round_temporal(M, mult, R.UNITS.index(unit), nearest=True).to_numpy()[0], R.round_temporal(mid, mult, unit))


# ------------------------------------------------------------------ documented errors (a status, not a fault)
def test_errors(px, golden_ts):
    L, K = px.L, px.K
    T = golden_ts[0]
    n = T.length
    ints = px.Column.from_numpy(np.arange(n))
    with pytest.raises(L.PdxError, match="PDX_TIMESTAMP_NS") as e:
        K.temporal_components(ints, [L.TC_YEAR])
    assert e.value.status == L.INVALID
    with pytest.raises(L.PdxError, match="PDX_TIMESTAMP_NS") as e:
        K.temporal_between(L.UNIT_DAY, T, ints)
    assert e.value.status == L.INVALID
    for comps in ([], [L.TC_YEAR] * 9):
        with pytest.raises(L.PdxError, match="between 1 and 8") as e:
            K.temporal_components(T, comps)
        assert e.value.status == L.INVALID
    with pytest.raises(L.PdxError, match="unknown component") as e:
        K.temporal_components(T, [20])
    assert e.value.status == L.INVALID
    for comp, wrong in ((L.TC_YEAR, L.FLOAT64), (L.TC_IS_LEAP_YEAR, L.INT64), (L.TC_SUBSECOND, L.INT64), (L.TC_HOUR, L.TIMESTAMP_NS)):
        out = px.Column.empty(wrong, n)
        m, ct, arr = out.mut(), T.c(), (C.c_int * 1)(comp)
        assert L.load().pdx_temporal_components(C.byref(ct), arr, 1, None, C.byref(m), None) == L.INVALID
    short = px.Column.empty(L.INT64, n - 1)
    m, ct, arr = short.mut(), T.c(), (C.c_int * 1)(L.TC_YEAR)
    assert L.load().pdx_temporal_components(C.byref(ct), arr, 1, None, C.byref(m), None) == L.INVALID
    odd = px.Column.empty(L.BOOL, n)  # a bit-packed output that does not start on an 8-byte boundary
    m, ct, leap = odd.mut(), T.c(), (C.c_int * 1)(L.TC_IS_LEAP_YEAR)
    m.values = odd.values.data_ptr() + 1
    assert L.load().pdx_temporal_components(C.byref(ct), leap, 1, None, C.byref(m), None) == L.INVALID
    assert b"8-byte aligned" in L.load().pdx_last_error()
    with pytest.raises(L.PdxError, match="Array arguments must all be the same length") as e:
        K.temporal_between(L.UNIT_DAY, T, T.slice(0, n - 1))
    assert e.value.status == L.INVALID
    for unit in (L.UNIT_MONTH, 11, -1):
        with pytest.raises(L.PdxError) as e:
            K.temporal_between(unit, T, T)
        assert e.value.status == L.INVALID
    out = px.Column.empty(L.FLOAT64, n)
    m, ca = out.mut(), T.c()
    assert L.load().pdx_temporal_between(L.UNIT_DAY, C.byref(ca), C.byref(ca), C.byref(m), None) == L.INVALID
    nulls = ts_col(px, G["ts"][:64], valid=np.arange(64) % 2 == 0)
    out = px.Column.empty(L.INT64, 64)  # nulls in, no validity buffer out
    m, ct = out.mut(), nulls.c()
    assert L.load().pdx_temporal_components(C.byref(ct), arr, 1, None, C.byref(m), None) == L.INVALID
    with pytest.raises(L.PdxError) as e:
        K.round_temporal(T, 1, L.UNIT_YEAR, nearest=True)
    assert e.value.status == L.NOT_IMPLEMENTED
    empty = ts_col(px, np.zeros(0, np.int64))
    assert K.temporal_components(empty, [L.TC_YEAR, L.TC_IS_LEAP_YEAR])[1].length == 0 and K.temporal_between(L.UNIT_YEAR, empty, empty).length == 0


# ------------------------------------------------------------------ the Python facade
def test_series_dt_accessor(px):
    api, L = px.api, px.L
    ts = G["ts"][:500]
    index = px.Column.from_numpy(np.arange(500) * 3)
    s = api.Series(px.Column.from_numpy(ts, dtype=L.TIMESTAMP_NS), index=index, name="t")
    dt = s.dt
    for name in SINGLE:
        if name == "iso_day_of_week":
            continue  # (a field of iso_calendar only, as in Arrow)
        out = getattr(dt, name)()
        assert out.index is index and out.name == ""
        same_bits(out.values(), G["comp_" + name][:500])
    same_bits(dt.week(False, True, False).values(), G["week_010"][:500])
    ymd, iso = dt.year_month_day(), dt.iso_calendar()
    assert ymd.names == ["year", "month", "day"] and iso.names == ["iso_year", "iso_week", "iso_day_of_week"] and ymd.index is index
    for k, c in enumerate(("year", "month", "day")):
        same_bits(ymd[c].values(), G["comp_" + c][:500])
    same_bits(np.stack([iso[c].values() for c in iso.names], axis=1), G["isocal"][:500])
    other = api.Series(px.Column.from_numpy(G["b_ts"][:500], dtype=L.TIMESTAMP_NS))
    for unit in R.BETWEEN_UNITS:
        out = getattr(dt, unit + "s_between")(other)
        assert out.index is index
        same_bits(out.values(), G["between_" + unit][:500])
    r = api.Series(px.Column.from_numpy(G["r_ts"], dtype=L.TIMESTAMP_NS)).dt
    same_bits(r.round(5, "hour", True, False, True).values(), G["round_round_hour_5_1_1"])
    same_bits(r.floor(2, L.UNIT_WEEK, False).values(), G["round_floor_week_2_0_0"])
    same_bits(r.ceil(3, "day").values(), G["round_ceil_day_3_1_0"])
    same_bits(r.round().values(), G["round_round_day_1_1_0"])
    assert r.round().dtype() == L.TIMESTAMP_NS
    # an int64 Series goes through Arrow's cast (a reinterpretation); every other type has no cast to timestamp
    same_bits(api.Series(ts).dt.year().values(), G["comp_year"][:500])
    for bad, name in ((np.array([1.5]), "double"), (np.array([True]), "bool"), (np.array([1.5], np.float32), "float")):
        with pytest.raises(L.PdxError, match=f"Unsupported cast from {name} to timestamp using function cast_timestamp") as e:
            api.Series(bad).dt
        assert e.value.status == L.NOT_IMPLEMENTED
    for call in (lambda: dt.is_dst(), lambda: dt.strftime("%Y"), lambda: dt.day_time_interval_between(other), lambda: dt.month_interval_between(other),
                 lambda: dt.month_day_nano_interval_between(other), lambda: dt.ceil(1, "day", True, True)):
        with pytest.raises(L.PdxError, match="DateTimeLike") as e:
            call()
        assert e.value.status == L.NOT_IMPLEMENTED
    with pytest.raises(L.PdxError, match="Array arguments must all be the same length"):
        dt.days_between(api.Series(px.Column.from_numpy(ts[:7], dtype=L.TIMESTAMP_NS)))


# ------------------------------------------------------------------ integration: calendar keys into the group-by
def test_group_by_hour_of_day(px):
    api, L = px.api, px.L
    rng = np.random.default_rng(11)
    n = 50_000
    ts = np.int64(1_600_000_000) * 10**9 + rng.integers(0, 400 * R.NS_DAY, n)
    x = rng.integers(-1000, 1000, n)
    s = api.Series(px.Column.from_numpy(ts, dtype=L.TIMESTAMP_NS))
    df = api.DataFrame({"hour": s.dt.hour(), "x": x})
    out = df.group_by("hour").sum("x")
    hours = ts // (3600 * 10**9) % 24
    got = dict(zip(out.index.to_numpy()[0].tolist(), out.values().tolist()))
    assert got == {h: int(x[hours == h].sum()) for h in range(24)}


def test_group_by_year_month_key(px):
    api, L = px.api, px.L
    rng = np.random.default_rng(12)
    n = 50_000
    ts = np.int64(946_684_800) * 10**9 + rng.integers(0, 3000 * R.NS_DAY, n)  # 2000-01-01 + up to ~8 years
    x = rng.integers(0, 100, n)
    s = api.Series(px.Column.from_numpy(ts, dtype=L.TIMESTAMP_NS))
    ym = s.dt.components(["year", "month"])
    key = ym["year"] * 100 + ym["month"]
    out = api.DataFrame({"ym": key, "x": x}).group_by("ym").count("x")
    months = ts.view("M8[ns]").astype("M8[M]").astype(np.int64)
    exp_key = (months // 12 + 1970) * 100 + months % 12 + 1
    uk, cnt = np.unique(exp_key, return_counts=True)
    got = dict(zip(out.index.to_numpy()[0].tolist(), out.values().tolist()))
    assert got == dict(zip(uk.tolist(), cnt.tolist()))
