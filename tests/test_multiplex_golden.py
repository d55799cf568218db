"""CPU: the numpy restatement of coalesce, min / max_element_wise, clip, replace_with_mask, indices_nonzero and the drop_null row mask
(tests/_multiplex_ref.py) equals Arrow C++ 25 on every case of tests/golden/multiplex_golden.npz (tools/gen_golden_multiplex.py), bit for
bit; a NaN that min / max / clip return is compared as "is NaN" (_multiplex_ref.same_minmax).  No GPU.  Where pyarrow is installed the
restatement is also held against it on seeded random cases."""
import numpy as np
import pytest

import _multiplex_ref as R

GOLD = R.MultiplexGolden()


def operands(case):
    dt = case["dtype"]
    return [(GOLD.get(f"{case['name']}/op{k}", dt), GOLD.get(f"{case['name']}/ok{k}") if case["has_valid"][k] else None, sc)
            for k, sc in enumerate(case["scalar"])]


def test_golden_covers_what_the_generator_promises():
    assert GOLD.arrow_version.startswith("25.")
    assert {(c["dtype"], c["C"]) for c in GOLD.of("coalesce")} >= {(dt, C) for dt in R.ALL_DTYPES for C in (1, 2, 3, 17)} | {("f64", 65), ("bool", 65)}
    assert {c["dtype"] for c in GOLD.of("minmax")} == set(R.MINMAX_DTYPES)
    for c in GOLD.of("minmax"):
        assert {(r["is_max"], r["skip_nulls"]) for r in c["runs"]} >= {(0, 1), (1, 1)}
    assert {c["name"].split("_", 2)[2] for c in GOLD.of("clip")} >= {"lo_lt_hi", "lo_gt_hi", "null_lo", "null_hi", "null_both", "nan_lo", "nan_hi", "zeros"}
    assert {c["dtype"] for c in GOLD.of("replace_with_mask")} == set(R.ALL_DTYPES)
    assert {c["dtype"] for c in GOLD.of("indices_nonzero")} == set(R.NONZERO_DTYPES)
    assert {c["C"] for c in GOLD.of("drop_null")} == {1, 3, 17}


def test_coalesce():
    for case in GOLD.of("coalesce"):
        dt, C, n = case["dtype"], case["C"], case["n"]
        a = GOLD.get(case["name"] + "/a", dt).reshape(C, n)
        valid = GOLD.get(case["name"] + "/valid").reshape(C, n) if case["has_valid"] else None
        got, ok = R.coalesce(a, valid)
        bad = R.same_bits(got, ok, GOLD.get(case["name"] + "/out", dt), GOLD.get(case["name"] + "/ok"))
        assert not bad, (case["name"], bad[:5])


def test_element_wise_minmax():
    ran = 0
    for case in GOLD.of("minmax"):
        ops = operands(case)
        for run in case["runs"]:
            got, ok = R.element_wise_minmax(run["is_max"], ops, run["skip_nulls"], case["n"])
            want, want_ok = GOLD.get(f"{case['name']}/{run['key']}/out", case["dtype"]), GOLD.get(f"{case['name']}/{run['key']}/ok")
            bad = R.same_minmax(got, ok, want, want_ok)
            assert not bad, (case["name"], run["key"], bad[:5], got[bad[:5]], want[bad[:5]])
            ran += 1
    assert ran >= 6 * 7 * 4


def test_clip():
    for case in GOLD.of("clip"):
        dt, nm = case["dtype"], case["name"]
        x, xv = GOLD.get(nm + "/x", dt), GOLD.get(nm + "/x_ok")
        lo, hi = GOLD.get(nm + "/lo", dt), GOLD.get(nm + "/hi", dt)
        for run in case["runs"]:
            got, ok = R.clip(x, xv, lo, np.array([case["lo_ok"]]), hi, np.array([case["hi_ok"]]), run["skip_nulls"])
            want, want_ok = GOLD.get(f"{nm}/{run['key']}/out", dt), GOLD.get(f"{nm}/{run['key']}/ok")
            bad = R.same_minmax(got, ok, want, want_ok)
            assert not bad, (nm, run["key"], bad[:5], got[bad[:5]], want[bad[:5]])


def test_replace_with_mask():
    for case in GOLD.of("replace_with_mask"):
        dt, nm = case["dtype"], case["name"]
        hv = case["has_valid"]
        got, ok = R.replace_with_mask(GOLD.get(nm + "/a", dt), GOLD.get(nm + "/a_ok") if hv[0] else None, GOLD.get(nm + "/mask"),
                                      GOLD.get(nm + "/mask_ok") if hv[1] else None, GOLD.get(nm + "/repl", dt), GOLD.get(nm + "/repl_ok") if hv[2] else None)
        bad = R.same_bits(got, ok, GOLD.get(nm + "/out", dt), GOLD.get(nm + "/ok"))
        assert not bad, (nm, bad[:5])
    errors = GOLD.of("replace_with_mask_errors")[0]["errors"]
    a, mask = np.arange(5), np.array([True, False, True, True, False])
    with pytest.raises(R.Invalid) as e:
        R.replace_with_mask(a, None, mask, None, np.arange(2), None)
    assert str(e.value) == errors["short_repl"] == "Replacement array must be of appropriate length (expected 3 items but got 2 items)"
    with pytest.raises(R.Invalid) as e:
        R.replace_with_mask(a, None, mask[:4], None, np.arange(3), None)
    assert str(e.value) == errors["mask_length"] == "Mask must be of same length as array (expected 5 items but got 4 items)"


def test_indices_nonzero_and_the_refusals():
    for case in GOLD.of("indices_nonzero"):
        dt, nm = case["dtype"], case["name"]
        got = R.indices_nonzero(GOLD.get(nm + "/a", dt), GOLD.get(nm + "/a_ok") if case["has_valid"] else None)
        want = GOLD.get(nm + "/out")
        assert got.dtype == want.dtype == np.uint64 and np.array_equal(got, want), nm
    errors = GOLD.of("not_implemented")[0]["errors"]
    assert errors["ts"] == f"Function 'indices_nonzero' has no kernel matching input types ({R.ARROW_NAME['ts']})"
    assert errors["minmax_bool"] == "Function 'min_element_wise' has no kernel matching input types (bool, bool)"


def test_drop_null_row_mask():
    for case in GOLD.of("drop_null"):
        C, n, nm = case["C"], case["n"], case["name"]
        valid = GOLD.get(nm + "/valid").reshape(C, n)
        keep = R.all_valid_mask(list(valid) if case["has_valid"] else [None] * C, n)
        assert np.array_equal(np.flatnonzero(keep), GOLD.get(nm + "/rows")), nm


# ---------------------------------------------------------------- live pyarrow, where it exists
def test_restatement_equals_live_pyarrow():
    pa = pytest.importorskip("pyarrow")
    import pyarrow.compute as pc

    if not pa.__version__.startswith("25."):
        pytest.skip("the rules are pinned to Arrow 25")
    rng = np.random.default_rng(7)
    pa_t = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32(), "bool": pa.bool_()}

    def arrow(a, valid, dt):
        return pa.array(np.ascontiguousarray(a), type=pa_t[dt], mask=None if valid is None else ~valid)

    def back(arr, dt):
        ok = np.asarray(pc.is_valid(arr).to_numpy(zero_copy_only=False), bool)
        if dt == "bool":
            return np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), bool), ok
        raw = np.frombuffer(arr.buffers()[1], dtype=R.NP_T[dt], count=len(arr) + arr.offset)[arr.offset:]
        return np.where(ok, raw, np.zeros(1, raw.dtype)), ok

    def draw(dt, n):
        if dt == "bool":
            return rng.random(n) < 0.5
        if dt[0] == "f":
            a = rng.integers(-2, 3, n).astype(R.NP_T[dt])
            a[rng.random(n) < 0.15] = np.nan
            a[rng.random(n) < 0.15] = -0.0
            return a
        return rng.integers(0 if dt == "u64" else -3, 4, n).astype(R.NP_T[dt])

    for trial in range(300):
        dt = ("i64", "u64", "f64", "i32", "f32", "bool")[trial % 6]
        n, C = int(rng.integers(1, 40)), int(rng.integers(1, 5))
        a = np.stack([draw(dt, n) for _ in range(C)])
        valid = rng.random((C, n)) >= rng.choice([0.0, 0.3, 0.8])
        cols = [arrow(a[c], valid[c], dt) for c in range(C)]
        want, want_ok = back(pc.coalesce(*cols), dt)
        got, ok = R.coalesce(a, valid)
        assert not R.same_bits(got, ok, want.astype(got.dtype), want_ok), ("coalesce", trial)
        if dt != "bool":
            for is_max in (0, 1):
                skip = bool(rng.integers(0, 2))
                fn = pc.max_element_wise if is_max else pc.min_element_wise
                want, want_ok = back(fn(*cols, skip_nulls=skip), dt)
                got, ok = R.element_wise_minmax(is_max, [(a[c], valid[c], False) for c in range(C)], skip)
                assert not R.same_minmax(got, ok, want, want_ok), ("minmax", trial, is_max, skip)
        mask, mv = rng.random(n) < 0.5, rng.random(n) >= 0.2
        need = int((mask & mv).sum())
        repl, rv = draw(dt, need + trial % 3), rng.random(need + trial % 3) >= 0.3
        want, want_ok = back(pc.replace_with_mask(cols[0], pa.array(mask, mask=~mv), arrow(repl, rv, dt)), dt)
        got, ok = R.replace_with_mask(a[0], valid[0], mask, mv, repl, rv)
        assert not R.same_bits(got, ok, want.astype(got.dtype), want_ok), ("replace_with_mask", trial)
        assert np.array_equal(R.indices_nonzero(a[0], valid[0]), pc.indices_nonzero(cols[0]).to_numpy()), ("indices_nonzero", trial)
