"""GPU: runs the C++ facade's selection / null-handling test program (tests/cpp/test_facade_multiplex.cpp): DataFrame::coalesce / drop_na,
Series::clip / replace_with_mask / drop_na / indices_nonzero through pandasarrow_amd/cpp/pdx.hpp -> C ABI -> HIP kernels."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_facade_multiplex_cases():
    import __graft_entry__ as ge

    exe = os.path.join(ROOT, "tests", "cpp", "test_facade_multiplex")
    if not os.path.exists(exe):
        ge.build_hip()
        exe = ge.build_cpp_multiplex_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
