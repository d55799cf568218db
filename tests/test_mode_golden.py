"""CPU-only: tests/golden/mode_golden.npz (Arrow C++ 25's `mode` and `value_counts`, written by tools/gen_golden_mode.py) against the numpy
restatement tests/_mode_ref.py that the GPU tests use for the shapes too large to freeze; what the golden covers."""
import os

import numpy as np
import pytest

import _mode_ref as R

GOLD = R.ModeGolden()
MODE_CASES = [c for c in GOLD.cases if c["kind"] == "mode"]


def test_golden_file_is_small():
    assert os.path.getsize(R.GOLDEN) < 300 * 1024


def test_only_the_zeros_cases_hold_both_zeros():
    """which zero Arrow returns from a column with both is its unstable sort's choice: only cases named zeros_* may hold both"""
    for c in GOLD.cases:
        if c["kind"] in ("mode", "group"):
            a, valid = GOLD.inputs(c)
            assert R.holds_both_zeros(a, valid) == c["name"].startswith("zeros_"), c["name"]


@pytest.mark.parametrize("dt", R.MODE_DTYPES)
def test_restatement_reproduces_mode_cases(dt):
    cases = [c for c in MODE_CASES if c["dtype"] == dt]
    assert len(cases) >= 190
    for c in cases:
        a, valid = GOLD.inputs(c)
        want, _, want_counts = GOLD.expected(c)
        got, counts = R.mode(a, valid, c["n"], bool(c["skip_nulls"]), c["min_count"])
        assert R.same_values(got, want, ignore_zero_sign=c["name"].startswith("zeros_")), c["name"]
        assert np.array_equal(counts, want_counts), c["name"]
        nans = np.isnan(want) if want.dtype.kind == "f" else np.zeros(len(want), bool)
        assert (R.bits(want[nans]) == R.bits(np.array([R.canonical_nan(want.dtype)]))[0]).all(), c["name"]  # Arrow returns the canonical NaN


def test_restatement_reproduces_value_counts_and_is_unique():
    cases = [c for c in GOLD.cases if c["kind"] == "value_counts"]
    assert {c["dtype"] for c in cases} == {"i64", "u64", "ts", "f64", "bool"}
    for c in cases:
        a, valid = GOLD.inputs(c)
        want, want_ok, want_counts = GOLD.expected(c)
        got, ok, counts = R.value_counts(a, valid)
        assert np.array_equal(ok, want_ok) and np.array_equal(counts, want_counts), c["name"]
        assert R.same_values(got[ok], want[want_ok]), c["name"]
        assert R.is_unique(a, valid) == (len(want) == len(a)), c["name"]
    by = GOLD.by_name
    assert len(GOLD.expected(by["vc_f64_zeros_distinct"])[0]) == 3  # 0.0 and -0.0 are two entries
    assert R.is_unique(*GOLD.inputs(by["vc_i64_unique"])) and not R.is_unique(*GOLD.inputs(by["vc_i64_two_nulls"]))
    for dt in ("i64", "u64", "ts", "f64", "bool"):
        assert not GOLD.expected(by[f"vc_{dt}_first"])[1][0] and GOLD.expected(by[f"vc_{dt}_absent"])[1].all()
        assert len(GOLD.expected(by[f"vc_{dt}_empty"])[0]) == 0


@pytest.mark.parametrize("dt", ["f64", "i64", "u64"])
def test_restatement_reproduces_group_cases(dt):
    cases = [c for c in GOLD.cases if c["kind"] == "group" and c["dtype"] == dt]
    assert len(cases) == 3
    for c in cases:
        a, valid = GOLD.inputs(c)
        ids, G = R.group_ids(GOLD.keys(c))
        want, want_ok, want_counts = GOLD.expected(c)
        got, ok, counts = R.group_mode(ids, G, a, valid)
        assert np.array_equal(ok, want_ok) and np.array_equal(counts, want_counts), c["name"]
        assert R.same_values(got[ok], want[want_ok]), c["name"]


def test_errors_follow_arrow_25():
    by = GOLD.by_name
    assert by["err_n_zero"]["error"] == by["err_n_negative"]["error"] == R.N_ERROR and by["err_n_zero"]["status"] == "invalid"
    assert by["err_timestamp"]["error"] == R.TS_ERROR and by["err_timestamp"]["status"] == "not_implemented"
    for n in (0, -1):
        with pytest.raises(ValueError) as e:
            R.mode(np.array([1, 2]), None, n)
        assert str(e.value) == R.N_ERROR


def test_golden_coverage():
    by = GOLD.by_name
    assert {c["dtype"] for c in MODE_CASES} == set(R.MODE_DTYPES)

    def res(name):
        v, _, c = GOLD.expected(by[name])
        return v, c

    # every empty-result rule
    for dt in R.MODE_DTYPES:
        assert len(res(f"m_{dt}_all_63_n1_s1m0")[0]) == 0            # no valid value
        assert len(res(f"m_{dt}_third_63_n1_s0m0")[0]) == 0          # skip_nulls == 0 and a null
        assert len(res(f"m_{dt}_third_63_n1_s1mN")[0]) == 0          # fewer than min_count valid rows
        assert len(res(f"m_{dt}_third_63_n1_s1mV")[0]) == 1          # exactly min_count valid rows
        assert len(res(f"m_{dt}_none_0_n1_s1m0")[0]) == 0            # length 0
        assert len(res(f"m_{dt}_none_63_n1_s0m0")[0]) == 1           # skip_nulls == 0 without a null
        v, _ = res(f"m_{dt}_none_700_n1000_s1m0")                     # n beyond the number of distinct values
        assert 1 < len(v) < 1000
    assert len(res("sp_only_nulls")[0]) == 0 and len(res("sp_skip_nulls_0_null")[0]) == 0 and len(res("sp_skip_nulls_0_no_null")[0]) == 1
    v, c = res("sp_n_beyond_distinct")
    assert v.tolist() == [4, -4, 0] and c.tolist() == [2, 1, 1]
    v, c = res("sp_tie_at_nth")                                       # ties at the n-th place go to the smaller values
    assert v.tolist() == [3, 5, 7] and c.tolist() == [2, 2, 2]
    v, c = res("sp_nan_wins")
    assert np.isnan(v[0]) and c.tolist() == [3, 2] and v[1] == 1
    v, c = res("sp_nan_ties_number")                                  # NaN tied with numbers: behind +inf
    assert c.tolist() == [2, 2, 2, 1] and v[0] == 2.0 and np.isinf(v[1]) and np.isnan(v[2]) and v[3] == -1.0
    v, c = res("sp_only_nan")
    assert len(v) == 1 and np.isnan(v[0]) and c.tolist() == [3]
    assert res("sp_only_nan_min_count")[1].tolist() == [3]            # NaN rows count as valid for min_count
    v, c = res("sp_int64_extremes")
    assert v.tolist() == [-2**63, 2**63 - 1, 0] and c.tolist() == [2, 2, 1]
    v, c = res("sp_bool_tie")
    assert v.tolist() == [False, True] and c.tolist() == [2, 2]
    v, c = res("zeros_block")
    assert v[0] == 0 and c.tolist() == [40, 3]                        # the zeros' counts add
    # timestamp: refused for mode, kept for value_counts
    assert by["err_timestamp"]["status"] == "not_implemented" and by["vc_ts_middle"]["dtype"] == "ts"
    # groups: all null, all NaN
    ok = GOLD.expected(by["g_f64_3"])[1]
    assert not ok[1] and np.isnan(GOLD.expected(by["g_f64_3"])[0][2])
