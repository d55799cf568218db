"""CPU tests (no GPU) of the 32-bit column goldens (tools/gen_golden_narrow.py, Arrow 25 through pyarrow): the header's dtype enum and
the binding's constants agree, the frozen file stays small, and regenerating it in memory reproduces it bit for bit."""
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "narrow_golden.npz")


def test_header_enum_matches_binding():
    from pandasarrow_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "pdx", "abi.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\bPDX_(INT32|FLOAT32)\s*=\s*(\d+)", text))
    assert enum == {"INT32": L.INT32, "FLOAT32": L.FLOAT32} == {"INT32": 5, "FLOAT32": 6}
    assert "pdx_cast" in L.ABI_SYMBOLS


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 1 << 20
    z = np.load(GOLDEN)
    cases = json.loads(str(z["manifest"]))["cases"]
    kinds = {c["kind"] for c in cases.values()}
    assert kinds == {"binary", "compare", "if_else", "unary", "aggregate", "cast", "concat"}
    errors = [c["error"] for c in cases.values() if c["error"]]
    assert "divide by zero" in errors
    assert "Integer value 16777217 not in range: -16777216 to 16777216" in errors
    assert z["agg_i32_1_0/out_sum"][0] == 3 * (2**31 - 1)  # sum(int32) -> int64, no wrap
    assert z["bin_mul_i32_i32_s0/out"].dtype == np.int32 and z["bin_add_f32_f32_s0/out"].dtype == np.float32


def test_regenerated_goldens_match_frozen_file():
    pa = pytest.importorskip("pyarrow")
    if not pa.__version__.startswith("25."):
        pytest.skip(f"goldens are frozen against Arrow 25 (pyarrow {pa.__version__} here)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_golden_narrow as gen
    finally:
        sys.path.pop(0)
    fresh = gen.generate()
    z = np.load(GOLDEN)
    assert sorted(fresh) == sorted(z.files)
    for k in z.files:
        a, b = np.asarray(fresh[k]), z[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        else:
            assert np.array_equal(a, b), k
