"""The numpy restatement of the join contract (tests/_join_ref.py) against tests/golden/join_golden.npz (tools/gen_golden_join.py): its
ordered output is frozen there, and its multiset of (left row, right row) pairs must equal the one Arrow's own hash join gave for the same
inputs -- which pins the null rule (a null key matches nothing) and the handling of duplicate keys against Arrow itself.  No GPU."""
import numpy as np
import pytest

from _join_ref import HOWS, golden_inputs, join_ref, load_golden, pair_multiset

MAN, GET = load_golden()
CASES = MAN["cases"]


def test_golden_file_covers_the_contract():
    assert len(CASES) >= 24
    assert {c["dtype"] for c in CASES} == {"i64", "u64", "ts", "i32"}
    assert MAN["arrow"] is not None, "the golden file was generated without pyarrow: regenerate it where pyarrow imports"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_golden_and_arrow(case):
    lk, lv, rk, rv = golden_inputs(case, GET)
    name = case["name"]
    for how in HOWS:
        li, lok, ri, rok = join_ref(lk, lv, rk, rv, how)
        assert np.array_equal(li, GET(f"{name}/{how}/li")), how
        assert np.array_equal(lok, GET(f"{name}/{how}/lok").astype(bool)), how
        if how in ("semi", "anti"):
            assert ri is None and rok is None
        else:
            assert np.array_equal(ri, GET(f"{name}/{how}/ri")), how
            assert np.array_equal(rok, GET(f"{name}/{how}/rok").astype(bool)), how
            assert np.all(ri[~rok] == 0) and np.all(li[~lok] == 0), "value slots under a null index are zero"
        if MAN["arrow"] is not None:
            assert np.array_equal(pair_multiset(li, lok, ri, rok), GET(f"{name}/{how}/arrow").reshape(-1, 2)), f"{how}: pairs differ from Arrow's"


def test_order_contract_on_a_literal_case():
    # left keys 2, null, 1, 2; right keys 2, 1, 2, null, 3
    lk, lv = np.array([2, 0, 1, 2]), np.array([1, 0, 1, 1], bool)
    rk, rv = np.array([2, 1, 2, 0, 3]), np.array([1, 1, 1, 0, 1], bool)
    li, lok, ri, rok = join_ref(lk, lv, rk, rv, "inner")
    assert li.tolist() == [0, 0, 2, 3, 3] and ri.tolist() == [0, 2, 1, 0, 2] and lok.all() and rok.all()
    li, lok, ri, rok = join_ref(lk, lv, rk, rv, "left")
    assert li.tolist() == [0, 0, 1, 2, 3, 3] and ri.tolist() == [0, 2, 0, 1, 0, 2] and rok.tolist() == [1, 1, 0, 1, 1, 1]
    li, lok, ri, rok = join_ref(lk, lv, rk, rv, "outer")
    assert li.tolist() == [0, 0, 1, 2, 3, 3, 0, 0] and lok.tolist() == [1] * 6 + [0, 0]
    assert ri.tolist() == [0, 2, 0, 1, 0, 2, 3, 4] and rok.tolist() == [1, 1, 0, 1, 1, 1, 1, 1]
    assert join_ref(lk, lv, rk, rv, "semi")[0].tolist() == [0, 2, 3]
    assert join_ref(lk, lv, rk, rv, "anti")[0].tolist() == [1]
