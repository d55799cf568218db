"""CPU-only: tests/golden/scan_golden.npz (Arrow C++ 25's cumulative_sum / prod / max / min, fill_null_forward / backward) against the numpy
restatement tests/_scan_ref.py that the GPU tests use as their reference, the a-priori bound of the float sum / product against Arrow's
own results, and header / binding agreement on pdx_cum_op."""
import os
import re

import numpy as np
import pytest

import _scan_ref as R
from conftest import ROOT

GOLD = R.ScanGolden()


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(R.GOLDEN) < 1 << 20
    names = {c["name"] for c in GOLD.cases}
    for op in ("sum", "prod", "max", "min"):
        for dt in ("i64", "u64", "f64", "i32", "f32"):
            for skip in (0, 1):
                for shape in ("none", "tenth", "ends", "all"):
                    for n in (0, 1, 63, 64, 65, 4097):
                        assert (shape != "none" and n == 0) or f"cum_{op}_{dt}_s{skip}_{shape}_{n}" in names
    assert sum(1 for c in GOLD.cases if "error" in c) == 6 + 8


@pytest.mark.parametrize("case", [c for c in GOLD.cases if c["fn"] == "cum" and c.get("compare") == "exact"], ids=lambda c: c["name"])
def test_restatement_reproduces_cumulative(case):
    a, valid = GOLD.inputs(case)
    want, want_valid = GOLD.expected(case)
    got, got_valid = R.cumulative(case["op"], a, valid, float(case["start"]), bool(case["skip_nulls"]))
    assert np.array_equal(got_valid, want_valid)
    assert np.array_equal(R.bits(got)[want_valid], want[want_valid])


@pytest.mark.parametrize("case", [c for c in GOLD.cases if c["fn"] == "fill"], ids=lambda c: c["name"])
def test_restatement_reproduces_fill(case):
    a, valid = GOLD.inputs(case)
    if "slice" in case:
        lo, n = case["slice"]
        a, valid = a[lo:lo + n], valid[lo:lo + n]
    want, want_valid = GOLD.expected(case)
    got, got_valid = R.fill_null(a, valid, bool(case["backward"]))
    assert np.array_equal(got_valid, want_valid)
    assert np.array_equal(R.bits(got)[want_valid], want[want_valid])


@pytest.mark.parametrize("case", [c for c in GOLD.cases if "error" in c and c["status"] == "invalid"], ids=lambda c: c["name"])
def test_restatement_reproduces_start_errors(case):
    a, valid = GOLD.inputs(case)
    with pytest.raises(R.StartError) as e:
        R.cumulative(case["op"], a, valid, float(case["start"]))
    assert str(e.value) == case["error"]


@pytest.mark.parametrize("case", [c for c in GOLD.cases if c.get("compare") in ("rounded", "nanpos")], ids=lambda c: c["name"])
def test_arrow_itself_is_inside_the_bound(case):
    """the tolerance of the float sum / product is derived, not measured: the reference's own (sequential) results must pass it"""
    a, valid = GOLD.inputs(case)
    want, want_valid = GOLD.expected(case)
    arrow = want.view(a.dtype)
    seq, seq_valid = R.cumulative(case["op"], a, valid, float(case["start"]), bool(case["skip_nulls"]))
    assert np.array_equal(seq_valid, want_valid) and R.same_special(seq[want_valid], arrow[want_valid])
    bad, worst = R.bound_violations(case["op"], arrow, a, valid, float(case["start"]))
    print(case["name"], "largest error of Arrow's result in u * S_i:", worst)
    assert not bad, bad[:5]


def test_regenerating_reproduces_the_frozen_file():
    pa = pytest.importorskip("pyarrow")
    if not pa.__version__.startswith("25."):
        pytest.skip(f"the goldens were frozen with pyarrow 25, this is {pa.__version__}")
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_golden_scan", os.path.join(ROOT, "tools", "gen_golden_scan.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = R.ScanGolden(gen.generate())
    assert [c for c in fresh.cases] == GOLD.cases
    for key in GOLD.manifest["arrays"]:
        name, field = key.rsplit("/", 1)
        assert np.array_equal(fresh.get(name, field), GOLD.get(name, field)), key


def test_header_and_binding_agree_on_cum_ops():
    from pandasarrow_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "pdx", "abi.h")).read()
    enum = re.search(r"typedef enum pdx_cum_op \{(.*?)\}", text, re.S).group(1)
    vals = {k: int(v) for k, v in re.findall(r"PDX_(CUM_[A-Z]+) = (\d+)", enum)}
    assert vals == {"CUM_SUM": L.CUM_SUM, "CUM_PROD": L.CUM_PROD, "CUM_MAX": L.CUM_MAX, "CUM_MIN": L.CUM_MIN} and len(vals) == 4
    for name in ("pdx_cumulative", "pdx_fill_null", "pdx_shift"):
        assert name in L.ABI_SYMBOLS
