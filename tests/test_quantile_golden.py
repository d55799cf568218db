"""CPU-only: tests/golden/quantile_golden.npz (Arrow C++ 25's exact `quantile`, written by tools/gen_golden_quantile.py) against the numpy
restatement tests/_quantile_ref.py that the GPU tests use for inputs too large to freeze; header / binding agreement on pdx_interpolation."""
import os
import re

import numpy as np
import pytest

import _quantile_ref as R
from conftest import ROOT

GOLD = R.QuantileGolden()


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(R.GOLDEN) < 1 << 20
    names = {c["name"] for c in GOLD.cases}
    for dt in ("i64", "u64", "f64", "i32", "f32"):
        for interp in R.INTERPOLATIONS:
            for shape in ("none", "tenth", "ends", "all"):
                for n in (0, 1, 2, 63, 64, 65, 4097):
                    for tag in ("s1m0", "s0m0", "s1m1", "s1mN"):
                        assert (shape != "none" and n == 0) or f"q_{dt}_{shape}_{n}_{interp}_{tag}" in names
    assert sum(1 for c in GOLD.cases if c["kind"] == "error") == 5
    assert {c["dtype"] for c in GOLD.cases if c["kind"] == "group"} == {"f64", "i64", "u64"}
    for c in GOLD.cases:  # -0.0 and 0.0 never meet in a golden input (Arrow's pick between them is not a rule)
        if c["kind"] != "error" and c["dtype"] in ("f64", "f32"):
            a, valid = GOLD.inputs(c)
            z = a[valid & (a == 0)]
            assert len(z) == 0 or np.signbit(z).all() or not np.signbit(z).any()


@pytest.mark.parametrize("interp", R.INTERPOLATIONS)
@pytest.mark.parametrize("dt", ["i64", "u64", "f64", "i32", "f32"])
def test_restatement_reproduces_column_cases(dt, interp):
    cases = [c for c in GOLD.cases if c["kind"] == "column" and c["dtype"] == dt and c["interpolation"] == interp]
    assert len(cases) >= 100
    for c in cases:
        a, valid = GOLD.inputs(c)
        want, want_ok = GOLD.expected(c)
        got, ok, _ = R.quantile(a, valid, c["q"], interp, bool(c["skip_nulls"]), c["min_count"])
        assert R.same(got, ok, want, want_ok), c["name"]


def test_special_values_follow_arrow_25():
    """the corner values include/pdx/abi.h documents, as pyarrow 25.0.0 returned them"""
    by = {c["name"]: c for c in GOLD.cases}

    def f64(name):
        b, ok = GOLD.expected(by[name])
        assert ok.all()
        return b.view(np.float64)

    assert f64("sp_one_inf_linear")[0] == 1.0  # f == 0 returns v[lo] alone, not 0 * inf
    assert np.isnan(f64("sp_inf_inf_linear")[1])
    assert f64("sp_big_i64_linear")[1] == 4.611686018427388e+18
    assert f64("sp_huge_f64_midpoint")[0] == 1.35e308  # halves first
    assert GOLD.expected(by["sp_tie_even4_nearest"])[0][0] == 3 and GOLD.expected(by["sp_tie_even6_nearest"])[0][0] == 3
    assert f64("sp_subnormal_midpoint")[0] == 5e-324  # f == 0: v[lo] itself, not v[lo] / 2 + v[lo] / 2


@pytest.mark.parametrize("interp", R.INTERPOLATIONS)
@pytest.mark.parametrize("dt", ["i64", "u64", "f64"])
def test_restatement_reproduces_group_cases(dt, interp):
    cases = [c for c in GOLD.cases if c["kind"] == "group" and c["dtype"] == dt and c["interpolation"] == interp]
    assert len(cases) == 27
    for c in cases:
        a, valid = GOLD.inputs(c)
        want, want_ok = GOLD.expected(c)
        got, ok = R.group_quantile(GOLD.keys(c), a, valid, c["q"][0], interp, bool(c["skip_nulls"]), c["min_count"])
        assert R.same(got, ok, want, want_ok), c["name"]


@pytest.mark.parametrize("case", [c for c in GOLD.cases if c["kind"] == "error" and c["status"] == "invalid"], ids=lambda c: c["name"])
def test_restatement_reproduces_argument_errors(case):
    with pytest.raises(ValueError) as e:
        R.quantile(np.array([1.0, 2.0]), None, case["q"])
    assert str(e.value) == case["error"]


def test_header_and_binding_agree_on_interpolation():
    from pandasarrow_amd import _lib as L

    src = open(os.path.join(ROOT, "include", "pdx", "abi.h")).read()
    body = re.search(r"typedef enum pdx_interpolation \{(.*?)\} pdx_interpolation;", src, re.S).group(1)
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"PDX_INTERP_(\w+) = (\d+)", body)}
    assert header == {name.upper(): i for i, name in enumerate(R.INTERPOLATIONS)}
    for name, v in header.items():
        assert getattr(L, "INTERP_" + name) == v
    from pandasarrow_amd import column as K

    assert K.INTERPOLATIONS == {name: i for i, name in enumerate(R.INTERPOLATIONS)}
