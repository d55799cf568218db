"""CPU: the numpy restatement of the row-wise aggregates (tests/_rowagg_ref.py) equals Arrow C++ 25 on every case of
tests/golden/rowagg_golden.npz (tools/gen_golden_rowagg.py), bit for bit -- NaN payloads of sum / mean / first / last included; a NaN that
min / max / product / variance / stddev return is compared as "is NaN" (_rowagg_ref.NAN_PAYLOAD_FREE).  No pyarrow, no GPU."""
import numpy as np
import pytest

import _rowagg_ref as R

GOLD = R.RowaggGolden()


def test_golden_covers_what_the_generator_promises():
    assert GOLD.arrow_version.startswith("25.")
    seen = {(c["dtype"], c["C"]) for c in GOLD.cases}
    assert seen == {(dt, C) for dt in R.ACCEPTED for C in (1, 2, 15, 16, 17, 31, 32, 33, 48, 65, 100)}
    for case in GOLD.cases:
        kinds = {r["kind"] for r in case["runs"]}
        assert kinds == set(R.ACCEPTED[case["dtype"]]), case["name"]
        assert {r["skip_nulls"] for r in case["runs"]} == {0, 1}
        if case["C"] in (1, 2, 17, 100):
            assert {r["min_count"] for r in case["runs"]} == {0, 1, case["C"], case["C"] + 1}
        if "variance" in kinds:
            assert {r["ddof"] for r in case["runs"] if r["kind"] == "stddev"} == {0, 1, case["C"]}


@pytest.mark.parametrize("dt", list(R.ACCEPTED))
def test_restatement_equals_arrow(dt):
    ran = 0
    for case in GOLD.cases:
        if case["dtype"] != dt:
            continue
        a, valid = GOLD.inputs(case)
        cache = {}
        for run in case["runs"]:
            key = (run["kind"], run["ddof"])
            if key not in cache:
                cache[key] = R.row_values(run["kind"], dt, a, valid, run["ddof"])
            vals, nv = cache[key]
            ok = R.row_validity(run["kind"], a, valid, nv, run["skip_nulls"], run["min_count"], run["ddof"])
            want, want_ok = GOLD.expected(case, run)
            assert vals.dtype == want.dtype, (case["name"], run["key"], vals.dtype, want.dtype)
            bad = R.same_result(run["kind"], vals, ok, want, want_ok)
            assert not bad, (case["name"], run["key"], bad[:5], vals[bad[:5]], want[bad[:5]])
            ran += 1
    assert ran >= 11 * 2 * len(R.ACCEPTED[dt])


def test_the_reference_facades_defaults():
    """what DataFrame::sum(AxisType::Columns) etc. pass (min_count = 0): a row without valid cells sums to 0, multiplies to 1, averages to a
    valid NaN, and has no min / max / first / last"""
    a = np.array([[1.5, 7.0], [2.5, 9.0]])
    valid = np.array([[True, False], [True, False]])
    for kind, want, ok in (("sum", 0.0, True), ("product", 1.0, True), ("min", None, False), ("max", None, False), ("first", None, False),
                           ("last", None, False), ("stddev", None, False)):
        vals, v = R.row_aggregate(kind, "f64", a, valid, True, 0, 1)
        assert v[1] == ok and (want is None or vals[1] == want), kind
        assert v[0]
    vals, v = R.row_aggregate("mean", "f64", a, valid, True, 0)
    assert v[1] and np.isnan(vals[1]) and vals[0] == 2.0
    assert list(R.row_aggregate("count_null", "f64", a, valid)[0]) == [0, 2]
