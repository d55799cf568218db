"""CPU: the numpy restatement of pdx_select_k (tests/_topk_ref.py) equals tests/golden/topk_golden.npz (Arrow C++ 25.0.0:
array_sort_indices(order)[:k]) for every case, order and k, bit for bit; the partition_nth layout of the restatement passes its own contract
checker.  This is what validates the reference that tests/test_gpu_topk.py leans on for shapes the golden file does not hold.  No pyarrow, no
GPU."""
import numpy as np
import pytest

import _topk_ref as R

GOLD = R.TopkGolden()


def test_the_golden_file_covers_every_dtype_and_shape():
    assert GOLD.arrow == "25.0.0"
    assert {c["dtype"] for c in GOLD.cases} == set(R.TOPK_DTYPES)
    for dt in R.TOPK_DTYPES:
        names = {c["name"].split("/", 1)[1] for c in GOLD.cases if c["dtype"] == dt}
        assert {"empty", "all_null", "all_equal", "special", "special_nulls"} <= names, dt
        if dt in ("f64", "f32"):
            assert {"all_nan", "zeros_both_signs"} <= names, dt
        assert max(c["rows"] for c in GOLD.cases if c["dtype"] == dt) == 300
    for c in GOLD.cases:
        n, m, nan = c["rows"], c["numbers"], c["nan"]
        assert set(c["ks"]) == {k for k in (0, 1, 2, m - 1, m, m + 1, m + nan, n - 1, n, n + 5) if k >= 0}, c["name"]
        assert R.counts(*GOLD.column(c))[:2] == (m, nan), c["name"]


def test_the_special_values_are_in_the_file():
    a, _ = GOLD.column(next(c for c in GOLD.cases if c["name"] == "f64/special"))
    assert np.isnan(a).any() and (np.signbit(a) & (a == 0)).any() and (~np.signbit(a) & (a == 0)).any()
    a, _ = GOLD.column(next(c for c in GOLD.cases if c["name"] == "i64/special"))
    assert a.min() == np.iinfo(np.int64).min and a.max() == np.iinfo(np.int64).max
    a, _ = GOLD.column(next(c for c in GOLD.cases if c["name"] == "u64/special"))
    assert a.max() == np.uint64(2**64 - 1) and (a > np.uint64(2**63)).sum() >= 2


@pytest.mark.parametrize("ascending", [True, False])
@pytest.mark.parametrize("dt", R.TOPK_DTYPES)
def test_select_k_equals_arrow(dt, ascending):
    for c in (c for c in GOLD.cases if c["dtype"] == dt):
        a, valid = GOLD.column(c)
        for k in c["ks"]:
            want = GOLD.want(c, ascending, k)
            assert len(want) == min(k, c["rows"]), (c["name"], k)
            assert np.array_equal(R.select_k(a, valid, k, ascending), want), (c["name"], k, ascending)


@pytest.mark.parametrize("dt", R.TOPK_DTYPES)
def test_the_partition_layout_passes_its_contract(dt):
    for c in (c for c in GOLD.cases if c["dtype"] == dt):
        a, valid = GOLD.column(c)
        n, m = c["rows"], c["numbers"]
        for pivot in sorted({p for p in (0, 1, n // 2, m - 1, m, n - 1, n) if 0 <= p <= n}):
            R.check_partition(a, valid, pivot, R.partition_nth(a, valid, pivot))


def test_the_contract_checker_rejects_wrong_answers():
    a = np.array([5, 1, 4, 1, 9, 3], np.int64)
    good = R.partition_nth(a, None, 2)
    assert good.tolist() == [1, 3, 5, 0, 2, 4]
    R.check_partition(a, None, 2, good)
    with pytest.raises(AssertionError):
        R.check_partition(a, None, 2, np.array([1, 3, 0, 5, 2, 4], np.uint64))  # the pivot's place holds 5, not 3
    with pytest.raises(AssertionError):
        R.check_partition(a, None, 2, np.array([1, 1, 5, 0, 2, 4], np.uint64))  # not a permutation
    f = np.array([np.nan, 2.0, 1.0])
    with pytest.raises(AssertionError):
        R.check_partition(f, None, 1, np.array([0, 2, 1], np.uint64))  # a NaN row in front of the numbers
