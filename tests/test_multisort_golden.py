"""CPU: the lexsort restatement of Arrow's sort_indices (tests/_multisort_ref.py) gives Arrow 25.0.0's answer on every case of
tests/golden/multisort_golden.npz (tools/gen_golden_multisort.py); the GPU tests compare pdx_sort_indices with that restatement."""
import json
import os

import numpy as np
import pytest

import _multisort_ref as R
from conftest import GOLDEN_DIR


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, "multisort_golden.npz"))
    return z, {c["name"]: c for c in json.loads(str(z["manifest"]))["cases"]}


def test_grid_is_the_one_the_golden_file_was_made_from(gold):
    _, manifest = gold
    cases = R.golden_cases()
    assert [c[0] for c in cases] == list(manifest)
    assert len(cases) == 6 * 4 * 2 * 3 + 1
    assert {k for _, cols, _ in cases for _, _, k in cols} == set(R.KINDS)
    assert max(len(cols) for _, cols, _ in cases) == 16
    for name, cols, desc in cases:
        assert R.case_digest(cols, desc) == manifest[name]["inputs"], name


def test_restatement_equals_arrow_on_every_case(gold):
    z, manifest = gold
    for name, cols, desc in R.golden_cases():
        ref = R.sort_indices_ref(cols, desc)
        assert len(ref) == manifest[name]["n"], name
        if len(ref) <= R.FULL_OUTPUT_MAX_N:
            assert np.array_equal(ref, z[name + "/indices"].astype(np.int64)), name
        assert R.digest(ref) == manifest[name]["answer"], name


def test_restatement_by_hand():
    """numbers < NaN < null in both orders; -0.0 ties with 0.0 and the next key decides; full ties keep row order"""
    a = (np.array([0.0, np.nan, -0.0, 1.0, 5.0, 1.0]), np.array([1, 1, 1, 1, 0, 1], bool), "f64")
    b = (np.array([2, 0, 1, 7, 0, 7], np.int64), None, "i64")
    assert R.sort_indices_ref([a, b], [False, False]).tolist() == [2, 0, 3, 5, 1, 4]
    assert R.sort_indices_ref([a, b], [True, False]).tolist() == [3, 5, 2, 0, 1, 4]
    assert R.sort_indices_ref([a, b], [False, True]).tolist() == [0, 2, 3, 5, 1, 4]
