"""CPU: the numpy restatement of the lookup rules (tests/_lookup_ref.py) equals tests/golden/lookup_golden.npz (Arrow C++ 25.0.0: is_in, index_in,
index, index(min()) / index(max()), dictionary_encode) for every case, bit for bit.  This is what validates the reference that
tests/test_gpu_lookup.py leans on for shapes the golden file does not hold.  No pyarrow, no GPU."""
import numpy as np
import pytest

import _lookup_ref as R

GOLD = R.LookupGolden()


def cases(kind):
    return [c for c in GOLD.cases if c["kind"] == kind]


def test_the_golden_file_covers_every_dtype_and_kind():
    assert {c["dtype"] for c in GOLD.cases} == set(R.LOOKUP_DTYPES)
    for kind in ("set", "index", "argext", "dict"):
        assert {c["dtype"] for c in cases(kind)} == set(R.LOOKUP_DTYPES), kind


@pytest.mark.parametrize("dt", R.LOOKUP_DTYPES)
def test_is_in_and_index_in(dt):
    for c in (c for c in cases("set") if c["dtype"] == dt):
        (a, valid), (s, svalid) = GOLD.column(c, "a"), GOLD.column(c, "set")
        idx, ok = R.index_in(a, valid, s, svalid, c["skip_nulls"])
        assert np.array_equal(ok, GOLD.arr(c, "index_in_ok")), c["name"]
        assert np.array_equal(idx, GOLD.arr(c, "index_in")), c["name"]
        assert np.array_equal(R.is_in(a, valid, s, svalid, c["skip_nulls"]), GOLD.arr(c, "is_in")), c["name"]
        assert np.array_equal(GOLD.arr(c, "is_in"), GOLD.arr(c, "index_in_ok")), c["name"]  # (Arrow's own two kernels agree)


def test_the_issues_example_is_in_the_golden_file():
    c = next(c for c in GOLD.cases if c["name"] == "f64/sp_null_in_set_skip0")
    (a, valid), (s, svalid) = GOLD.column(c, "a"), GOLD.column(c, "set")
    assert np.isnan(s[0]) and np.signbit(s[1]) and s[1] == 0 and not svalid[2] and s[3:].tolist() == [5.0, 5.0, 7.0]
    got = dict(zip(R.bits(a)[GOLD.arr(c, "index_in_ok")].tolist(), GOLD.arr(c, "index_in")[GOLD.arr(c, "index_in_ok")].tolist()))
    assert got[int(R.bits(np.array([5.0]))[0])] == 3 and got[int(R.bits(np.array([7.0]))[0])] == 5
    assert got[int(R.bits(np.array([-0.0]))[0])] == 1 and int(R.bits(np.array([0.0]))[0]) not in got
    assert set(GOLD.arr(c, "index_in")[~valid].tolist()) == {2}  # a null row finds the set's null


@pytest.mark.parametrize("dt", R.LOOKUP_DTYPES)
def test_index(dt):
    for c in (c for c in cases("index") if c["dtype"] == dt):
        a, valid = GOLD.column(c, "a")
        value = None if c["value_null"] else R.from_bits(np.array([c["value_bits"]], np.uint64), dt)[0]
        assert R.index(a, valid, value) == c["row"], c["name"]


@pytest.mark.parametrize("dt", R.LOOKUP_DTYPES)
def test_argmin_argmax(dt):
    for c in (c for c in cases("argext") if c["dtype"] == dt):
        a, valid = GOLD.column(c, "a")
        assert R.arg_extreme(a, valid, False) == c["argmin"], c["name"]
        assert R.arg_extreme(a, valid, True) == c["argmax"], c["name"]


@pytest.mark.parametrize("dt", R.LOOKUP_DTYPES)
def test_dictionary_encode(dt):
    for c in (c for c in cases("dict") if c["dtype"] == dt):
        a, valid = GOLD.column(c, "a")
        codes, ok, d = R.dictionary_encode(a, valid)
        assert np.array_equal(ok, GOLD.arr(c, "codes_ok")), c["name"]
        assert np.array_equal(codes, GOLD.arr(c, "codes")), c["name"]
        assert np.array_equal(R.bits(d), GOLD.arr(c, "dict")), c["name"]
