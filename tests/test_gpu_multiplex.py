"""GPU: pdx_coalesce, pdx_element_wise_minmax, pdx_clip, pdx_replace_with_mask, pdx_indices_nonzero(_count) and pdx_all_valid_mask
through pandasarrow_amd.column against every case of tests/golden/multiplex_golden.npz (Arrow C++ 25) and, on seeded random inputs at the
lengths / offsets / column counts where the kernels change path, against the numpy restatement tests/_multiplex_ref.py.  No pyarrow.

The comparison is bitwise and no case is skipped or filtered, with one exception: a NaN that pdx_element_wise_minmax / pdx_clip return is
compared as "is NaN" (_multiplex_ref.same_minmax: the payload gap of min / max).  pdx_coalesce and pdx_replace_with_mask copy
bits: their NaNs are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _multiplex_ref as R

pytestmark = pytest.mark.gpu

GOLD = R.MultiplexGolden()
TILE = 4096  # kCompactTile (pandasarrow_amd/csrc/compact.hpp)
LENGTHS = [0, 1, 63, 64, 65, 255, 257, TILE - 1, TILE + 1, 3 * TILE + 37]
OFFSETS = [0, 1, 7, 13, 64 + 5]
COLS = [1, 2, 3, 17, 65]
PATTERNS = ["none", "all_null", "last_only", "sparse", "word"]


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column as K

    lib = L.load()
    L.check(lib.pdx_init(0))
    dts = {"i64": L.INT64, "u64": L.UINT64, "f64": L.FLOAT64, "i32": L.INT32, "f32": L.FLOAT32, "ts": L.TIMESTAMP_NS, "bool": L.BOOL}
    return type("Env", (), {"torch": torch, "L": L, "K": K, "api": api, "lib": lib, "dts": dts})


def col(env, a, valid, dt, offset=0):
    return env.K.Column.from_numpy(np.asarray(a), valid, dtype=env.dts[dt], offset=offset)


def guarded(env, fn, *args):
    """a column.py call -> (status, result | message); a HIP error ends the session: nothing more is started on a device that may have faulted"""
    try:
        return env.L.OK, fn(*args)
    except env.L.PdxError as e:
        if e.status == env.L.DEVICE:
            pytest.exit(f"{fn.__name__}: {e}", returncode=3)
        return e.status, str(e)


def host(c, dt):
    vals, valid = c.to_numpy()
    vals = np.asarray(vals)
    return (vals if dt == "bool" else vals.view(R.NP_T[dt])), valid


def draw(rng, dt, n):
    t = R.NP_T[dt]
    if dt == "bool":
        return rng.random(n) < 0.5
    if dt in ("f64", "f32"):
        a = rng.integers(-3, 4, n).astype(t)
        nan_bits = np.array([0x7FF8000000000000, 0xFFF8000000000123], np.uint64).view(np.float64) if dt == "f64" else \
            np.array([0x7FC00000, 0xFFC00123], np.uint32).view(np.float32)
        pick = rng.random(n)
        a = np.where(pick < 0.08, rng.choice(nan_bits, n), a)
        a = np.where((pick >= 0.08) & (pick < 0.16), t(-0.0), a)
        a = np.where((pick >= 0.16) & (pick < 0.2), rng.choice(np.array([np.inf, -np.inf], t), n), a)
        return a.astype(t)
    if dt == "u64":
        pool = np.array([0, 2**63, 2**63 + 1, 2**64 - 1], np.uint64)
    else:
        info = np.iinfo(t)
        pool = np.array([info.min, info.max, info.min + 1, 0], t)
    a = rng.integers(0 if dt == "u64" else -3, 4, n).astype(t)
    return np.where(rng.random(n) < 0.25, rng.choice(pool, n), a).astype(t)


def pattern(rng, kind, Cn, n):
    v = np.ones((Cn, n), bool)
    if kind == "none":
        return None
    if kind == "all_null":
        v[:] = False
    elif kind == "last_only":
        v[:-1] = False
    elif kind == "sparse":
        v = rng.random((Cn, n)) >= 0.05
    elif kind == "word":
        v = rng.random((Cn, n)) >= 0.3
        v[:, 64:192] = False
        v[:, :64][:, ::2] = False
    return v


def frame(env, rng, dt, Cn, n, kind, shift=0):
    """-> (a, valid | None, device columns): column c at offset OFFSETS[(c + shift) % 5]; with validity every fourth column that has no
    null goes without a bitmap"""
    a = np.stack([draw(rng, dt, n) for _ in range(Cn)]) if Cn else np.zeros((0, n), R.NP_T[dt])
    valid = pattern(rng, kind, Cn, n)
    cols = []
    for c in range(Cn):
        v = None if valid is None or (c % 4 == 3 and valid[c].all()) else valid[c]
        cols.append(col(env, a[c], v, dt, OFFSETS[(c + shift) % len(OFFSETS)]))
    return a, valid, cols


# ---------------------------------------------------------------- every golden case
def test_golden_coalesce(env):
    for i, case in enumerate(GOLD.of("coalesce")):
        dt, Cn, n, nm = case["dtype"], case["C"], case["n"], case["name"]
        a = GOLD.get(nm + "/a", dt).reshape(Cn, n)
        valid = GOLD.get(nm + "/valid").reshape(Cn, n)
        cols = [col(env, a[c], valid[c] if case["has_valid"] else None, dt, OFFSETS[(c + i) % 5]) for c in range(Cn)]
        rc, out = guarded(env, env.K.coalesce, cols)
        assert rc == env.L.OK, (nm, out)
        got, ok = host(out, dt)
        want_ok = GOLD.get(nm + "/ok")
        assert not R.same_bits(got, ok, GOLD.get(nm + "/out", dt), want_ok), nm
        assert out.null_count == int((~want_ok).sum()), nm


def test_golden_minmax_and_clip(env):
    ran = 0
    for i, case in enumerate(GOLD.of("minmax")):
        dt, nm = case["dtype"], case["name"]
        cols = [col(env, GOLD.get(f"{nm}/op{k}", dt), GOLD.get(f"{nm}/ok{k}") if case["has_valid"][k] else None, dt, OFFSETS[(k + i) % 5])
                for k in range(len(case["scalar"]))]
        for run in case["runs"]:
            rc, out = guarded(env, env.K.element_wise_minmax, run["is_max"], cols, run["skip_nulls"])
            assert rc == env.L.OK, (nm, run["key"], out)
            got, ok = host(out, dt)
            want, want_ok = GOLD.get(f"{nm}/{run['key']}/out", dt), GOLD.get(f"{nm}/{run['key']}/ok")
            bad = R.same_minmax(got, ok, want, want_ok)
            assert not bad, (nm, run["key"], bad[:5], got[bad[:5]], want[bad[:5]])
            assert out.null_count == int((~want_ok).sum()), (nm, run["key"])
            ran += 1
    for i, case in enumerate(GOLD.of("clip")):
        dt, nm = case["dtype"], case["name"]
        x = col(env, GOLD.get(nm + "/x", dt), GOLD.get(nm + "/x_ok"), dt, OFFSETS[i % 5])
        lo = col(env, GOLD.get(nm + "/lo", dt), np.array([case["lo_ok"]]), dt, OFFSETS[(i + 1) % 5])
        hi = col(env, GOLD.get(nm + "/hi", dt), np.array([case["hi_ok"]]), dt, OFFSETS[(i + 2) % 5])
        for run in case["runs"]:
            rc, out = guarded(env, env.K.clip, x, lo, hi, run["skip_nulls"])
            assert rc == env.L.OK, (nm, run["key"], out)
            got, ok = host(out, dt)
            want, want_ok = GOLD.get(f"{nm}/{run['key']}/out", dt), GOLD.get(f"{nm}/{run['key']}/ok")
            bad = R.same_minmax(got, ok, want, want_ok)
            assert not bad, (nm, run["key"], bad[:5], got[bad[:5]], want[bad[:5]])
            assert out.null_count == int((~want_ok).sum()), (nm, run["key"])
            ran += 1
    assert ran == sum(len(c["runs"]) for c in GOLD.of("minmax") + GOLD.of("clip"))


def test_golden_replace_nonzero_drop_null(env):
    K = env.K
    for i, case in enumerate(GOLD.of("replace_with_mask")):
        dt, nm, hv = case["dtype"], case["name"], case["has_valid"]
        a = col(env, GOLD.get(nm + "/a", dt), GOLD.get(nm + "/a_ok") if hv[0] else None, dt, OFFSETS[i % 5])
        mask = col(env, GOLD.get(nm + "/mask"), GOLD.get(nm + "/mask_ok") if hv[1] else None, "bool", OFFSETS[(i + 1) % 5])
        repl = col(env, GOLD.get(nm + "/repl", dt), GOLD.get(nm + "/repl_ok") if hv[2] else None, dt, OFFSETS[(i + 2) % 5])
        rc, out = guarded(env, K.replace_with_mask, a, mask, repl)
        assert rc == env.L.OK, (nm, out)
        got, ok = host(out, dt)
        want_ok = GOLD.get(nm + "/ok")
        assert not R.same_bits(got, ok, GOLD.get(nm + "/out", dt), want_ok), nm
        assert out.null_count == int((~want_ok).sum()), nm
    for i, case in enumerate(GOLD.of("indices_nonzero")):
        dt, nm = case["dtype"], case["name"]
        rc, out = guarded(env, K.indices_nonzero, col(env, GOLD.get(nm + "/a", dt), GOLD.get(nm + "/a_ok") if case["has_valid"] else None, dt, OFFSETS[i % 5]))
        assert rc == env.L.OK and out.dtype == env.L.UINT64 and out.null_count == 0, (nm, out)
        assert np.array_equal(out.to_numpy()[0], GOLD.get(nm + "/out")), nm
    for i, case in enumerate(GOLD.of("drop_null")):
        Cn, n, nm = case["C"], case["n"], case["name"]
        valid = GOLD.get(nm + "/valid").reshape(Cn, n)
        cols = [col(env, np.arange(n) * (c + 1), valid[c] if case["has_valid"] else None, "i64", OFFSETS[(c + i) % 5]) for c in range(Cn)]
        rows = GOLD.get(nm + "/rows")
        rc, mask = guarded(env, K.all_valid_mask, cols)
        assert rc == env.L.OK and mask.null_count == 0 and np.array_equal(np.flatnonzero(mask.to_numpy()[0]), rows), nm
        rc, outs = guarded(env, K.drop_na, cols + [col(env, np.arange(n), None, "i64")])
        assert rc == env.L.OK and all(o.null_count == 0 for o in outs), nm
        assert np.array_equal(outs[-1].to_numpy()[0], rows) and np.array_equal(outs[0].to_numpy()[0], rows), nm


# ---------------------------------------------------------------- shapes at which the kernels change path, against the restatement
def test_coalesce_shapes(env):
    rng = np.random.default_rng(11)
    i = 0
    combos = [(n, Cn, R.ALL_DTYPES[k % 7], PATTERNS[k % 5]) for k, (n, Cn) in enumerate((n, Cn) for n in LENGTHS for Cn in COLS)]
    combos += [(257, 3, dt, p) for dt in R.ALL_DTYPES for p in PATTERNS] + [(n, 2, dt, "sparse") for n in (TILE + 1, 1023, 1025) for dt in ("i32", "f32")]
    for n, Cn, dt, kind in combos:
        a, valid, cols = frame(env, rng, dt, Cn, n, kind, shift=i)
        if dt in ("i32", "f32") and i % 2:  # 16-byte aligned streams: four rows per lane
            cols = [col(env, a[c], None if valid is None else valid[c], dt, 0) for c in range(Cn)]
        rc, out = guarded(env, env.K.coalesce, cols)
        assert rc == env.L.OK, (n, Cn, dt, kind, out)
        want, want_ok = R.coalesce(a, valid)
        got, ok = host(out, dt)
        assert out.length == n and not R.same_bits(got, ok, want, want_ok), (n, Cn, dt, kind)
        assert out.null_count == int((~want_ok).sum()), (n, Cn, dt, kind)
        i += 1


def test_minmax_and_clip_shapes(env):
    rng = np.random.default_rng(12)
    i = 0
    for n in LENGTHS:
        for dt in R.MINMAX_DTYPES:
            Cn, kind = COLS[i % 5], PATTERNS[(i // 2) % 5]
            a, valid, cols = frame(env, rng, dt, Cn, n, kind, shift=i)
            ops = [(a[c], None if valid is None else valid[c], False) for c in range(Cn)]
            if i % 3 == 0 and n > 1:  # a valid and a null broadcast operand among the arrays
                s1, s2 = draw(rng, dt, 1), draw(rng, dt, 1)
                cols = [col(env, s1, None, dt, 7)] + cols + [col(env, s2, np.array([False]), dt, 1)]
                ops = [(s1, None, True)] + ops + [(s2, np.array([False]), True)]
            for is_max, skip in ((i % 2, 1), (1 - i % 2, 0)):
                rc, out = guarded(env, env.K.element_wise_minmax, is_max, cols, skip)
                assert rc == env.L.OK, (n, dt, Cn, kind, out)
                want, want_ok = R.element_wise_minmax(is_max, ops, skip, n)
                got, ok = host(out, dt)
                bad = R.same_minmax(got, ok, want, want_ok)
                assert out.length == n and not bad, (n, dt, Cn, kind, is_max, skip, bad[:5])
                assert out.null_count == int((~want_ok).sum()), (n, dt, Cn, kind, is_max, skip)
            # clip: bounds in both orders, null and NaN bounds, zeros of both signs
            t = R.NP_T[dt]
            x, xv = a[0], None if valid is None else valid[0]
            bounds = [(t(1), True, t(2), True), (t(2), True, t(1), True), (t(0), False, t(2), True), (t(1), True, t(0), False), (t(0), False, t(0), False)]
            if dt in ("f64", "f32"):
                bounds += [(t(np.nan), True, t(2), True), (t(-1), True, t(np.nan), True), (t(-0.0), True, t(0.0), True), (t(0.0), True, t(-0.0), True)]
            lo, lo_ok, hi, hi_ok = bounds[i % len(bounds)]
            for skip in (1, 0):
                rc, out = guarded(env, env.K.clip, col(env, x, xv, dt, OFFSETS[i % 5]), col(env, [lo], np.array([lo_ok]), dt, 13),
                                  col(env, [hi], np.array([hi_ok]), dt, 69), skip)
                assert rc == env.L.OK, (n, dt, out)
                want, want_ok = R.clip(x, xv, np.array([lo], t), np.array([lo_ok]), np.array([hi], t), np.array([hi_ok]), skip)
                got, ok = host(out, dt)
                bad = R.same_minmax(got, ok, want, want_ok)
                assert out.length == n and not bad, ("clip", n, dt, lo, lo_ok, hi, hi_ok, skip, bad[:5])
                assert out.null_count == int((~want_ok).sum()), ("clip", n, dt, skip)
            i += 1


def test_replace_with_mask_shapes(env):
    rng = np.random.default_rng(13)
    L, K = env.L, env.K
    i = 0
    for n in LENGTHS:
        for dt in (R.ALL_DTYPES[i % 7], R.ALL_DTYPES[(i + 3) % 7]):
            a, av = draw(rng, dt, n), (rng.random(n) >= 0.1 if i % 2 else None)
            p_true = (0.5, 0.0, 1.0, 0.05)[i % 4]
            mask, mv = rng.random(n) < p_true, (rng.random(n) >= 0.1 if i % 3 else None)
            need = int((mask & (True if mv is None else mv)).sum())
            for extra in (0, 3):  # exactly as long as the true count, and longer
                repl, rv = draw(rng, dt, need + extra), (rng.random(need + extra) >= 0.2 if i % 2 == 0 else None)
                cols = (col(env, a, av, dt, OFFSETS[i % 5]), col(env, mask, mv, "bool", OFFSETS[(i + 1) % 5]), col(env, repl, rv, dt, OFFSETS[(i + 2) % 5]))
                rc, out = guarded(env, K.replace_with_mask, *cols)
                assert rc == L.OK, (n, dt, out)
                want, want_ok = R.replace_with_mask(a, av, mask, mv, repl, rv)
                got, ok = host(out, dt)
                assert out.length == n and not R.same_bits(got, ok, want, want_ok), (n, dt, extra)
                assert out.null_count == int((~want_ok).sum()), (n, dt, extra)
            if need:  # one short: the error and its text
                rc, msg = guarded(env, K.replace_with_mask, cols[0], cols[1], col(env, draw(rng, dt, need - 1), None, dt, 1))
                assert rc == L.INVALID and msg == f"Replacement array must be of appropriate length (expected {need} items but got {need - 1} items)", (n, dt, msg)
            i += 1
    # an all-false mask with an empty replacement
    a = draw(rng, "f64", 300)
    rc, out = guarded(env, K.replace_with_mask, col(env, a, None, "f64", 7), col(env, np.zeros(300, bool), None, "bool", 13), col(env, np.zeros(0), None, "f64"))
    assert rc == L.OK and out.null_count == 0 and np.array_equal(R.bits(host(out, "f64")[0]), R.bits(a))
    # length 1 against length 1 is not special
    rc, out = guarded(env, K.replace_with_mask, col(env, [5], None, "i64"), col(env, [True], None, "bool"), col(env, [9], None, "i64"))
    assert rc == L.OK and list(out.to_numpy()[0]) == [9]


def test_indices_nonzero_and_all_valid_mask_shapes(env):
    rng = np.random.default_rng(14)
    K = env.K
    i = 0
    for n in LENGTHS:
        for dt in R.NONZERO_DTYPES:
            a = draw(rng, dt, n)
            if i % 4 == 1:
                a[:] = 0
            av = None if i % 3 == 0 else rng.random(n) >= 0.2
            c = col(env, a, av, dt, OFFSETS[i % 5])
            rc, out = guarded(env, K.indices_nonzero, c)
            want = R.indices_nonzero(a, av)
            assert rc == env.L.OK and out.length == len(want) and out.null_count == 0, (n, dt, out)
            assert np.array_equal(out.to_numpy()[0], want), (n, dt)
            i += 1
        for Cn in COLS:
            kind = PATTERNS[i % 5]
            _, valid, cols = frame(env, rng, ("i64", "f32", "bool")[i % 3], Cn, n, kind, shift=i)
            rc, mask = guarded(env, K.all_valid_mask, cols)
            want = R.all_valid_mask([None] * Cn if valid is None else list(valid), n)
            assert rc == env.L.OK and mask.length == n and mask.null_count == 0 and mask.validity is None, (n, Cn, kind, mask)
            assert np.array_equal(mask.to_numpy()[0], want), (n, Cn, kind)
            i += 1
    # drop_na: a frame and its index, filtered by one mask; the kept rows carry no null
    n = 3 * TILE + 37
    a, valid, cols = frame(env, rng, "f64", 3, n, "sparse")
    idx = col(env, np.arange(n), None, "i64", 13)
    rc, outs = guarded(env, K.drop_na, cols + [idx])
    keep = R.all_valid_mask(list(valid), n)
    assert rc == env.L.OK and [o.length for o in outs] == [int(keep.sum())] * 4 and all(o.null_count == 0 for o in outs)
    assert np.array_equal(outs[3].to_numpy()[0], np.flatnonzero(keep))
    for c in range(3):
        assert np.array_equal(R.bits(outs[c].to_numpy()[0]), R.bits(a[c][keep])), c


# ---------------------------------------------------------------- the contract around the values
def test_refusals(env):
    L, K = env.L, env.K
    f, g = col(env, np.arange(10.0), None, "f64"), col(env, np.arange(10.0) * 2, np.arange(10) % 3 != 0, "f64")
    ints, flags = col(env, np.arange(10), None, "i64"), col(env, np.arange(10) % 2 == 0, None, "bool")
    ts = col(env, np.arange(10), None, "ts")
    scratch_out = K.Column.empty(L.FLOAT64, 10, True)
    m = scratch_out.mut()
    for bad in (0, -1, 2047):
        assert env.lib.pdx_coalesce(K._col_array([f] * 2), bad, C.byref(m), K._stream()) == L.INVALID
        assert env.lib.pdx_element_wise_minmax(0, K._col_array([f] * 2), bad, 1, C.byref(m), K._stream()) == L.INVALID
        assert env.lib.pdx_all_valid_mask(K._col_array([f] * 2), bad, C.byref(m), K._stream()) == L.INVALID
    # coalesce: mixed dtypes name the pair; lengths; output shape; validity needed exactly when cols[0] can be null
    rc, msg = guarded(env, K.coalesce, [f, ints])
    assert rc == L.NOT_IMPLEMENTED and "int64" in msg and "float64" in msg, msg
    rc, msg = guarded(env, K.coalesce, [f, col(env, np.arange(9.0), None, "f64")])
    assert rc == L.INVALID and "same length" in msg, msg

    def coalesce_into(cols, out):
        mm = out.mut()
        rc = env.lib.pdx_coalesce(K._col_array(cols), len(cols), C.byref(mm), K._stream())
        return rc, env.lib.pdx_last_error().decode()

    rc, msg = coalesce_into([f, g], K.Column.empty(L.FLOAT64, 9, True))
    assert rc == L.INVALID and "too small" in msg
    rc, msg = coalesce_into([f, g], K.Column.empty(L.INT64, 10, True))
    assert rc == L.INVALID and "dtype" in msg
    rc, msg = coalesce_into([g, f], K.Column.empty(L.FLOAT64, 10, False))
    assert rc == L.INVALID and "validity" in msg
    rc, msg = coalesce_into([f, g], K.Column.empty(L.FLOAT64, 10, False))
    assert rc == L.OK, msg
    # min / max: bool, two dtypes, operands that are neither n nor 1 long
    for is_max, name in ((0, "min_element_wise"), (1, "max_element_wise")):
        rc, msg = guarded(env, K.element_wise_minmax, is_max, [flags, flags])
        assert rc == L.NOT_IMPLEMENTED and msg == f"Function '{name}' has no kernel matching input types (bool, bool)", msg
    rc, msg = guarded(env, K.clip, flags, col(env, [False], None, "bool"), col(env, [True], None, "bool"))
    assert rc == L.NOT_IMPLEMENTED and msg == "Function 'min_element_wise' has no kernel matching input types (bool, bool)", msg
    rc, msg = guarded(env, K.element_wise_minmax, 0, [f, ints])
    assert rc == L.NOT_IMPLEMENTED and "int64" in msg and "float64" in msg, msg
    rc, msg = guarded(env, K.element_wise_minmax, 0, [f, col(env, np.arange(3.0), None, "f64")])
    assert rc == L.INVALID and "same length" in msg, msg
    rc, msg = guarded(env, K.clip, f, col(env, [1.0, 2.0], None, "f64"), col(env, [3.0], None, "f64"))
    assert rc == L.INVALID and "length 1" in msg, msg
    # replace_with_mask: the mask's length (Arrow's text), the replacement's dtype
    rc, msg = guarded(env, K.replace_with_mask, f, col(env, np.ones(8, bool), None, "bool"), f)
    assert rc == L.INVALID and msg == "Mask must be of same length as array (expected 10 items but got 8 items)", msg
    rc, msg = guarded(env, K.replace_with_mask, f, flags, ints)
    assert rc == L.INVALID and msg == "Function 'replace_with_mask' has no kernel matching input types (double, bool, int64)", msg
    rc, msg = guarded(env, K.replace_with_mask, f, flags, col(env, np.arange(4.0), None, "f64"))
    assert rc == L.INVALID and msg == "Replacement array must be of appropriate length (expected 5 items but got 4 items)", msg
    # indices_nonzero: timestamps, a fill buffer that is too small
    rc, msg = guarded(env, K.indices_nonzero, ts)
    assert rc == L.NOT_IMPLEMENTED and msg == "Function 'indices_nonzero' has no kernel matching input types (timestamp[ns])", msg
    small_out = K.Column.empty(L.UINT64, 3)
    small = small_out.mut()
    ci = ints.c()
    assert env.lib.pdx_indices_nonzero(C.byref(ci), C.byref(small), K._stream()) == L.INVALID and b"too small" in env.lib.pdx_last_error()
    # all_valid_mask: lengths, the mask's dtype
    rc, msg = guarded(env, K.all_valid_mask, [f, col(env, np.arange(9.0), None, "f64")])
    assert rc == L.INVALID and "same length" in msg, msg
    assert env.lib.pdx_all_valid_mask(K._col_array([f]), 1, C.byref(m), K._stream()) == L.INVALID  # (a float64 output)


@pytest.mark.parametrize("n", [1, 61, 64, 130])
def test_nothing_beyond_length_is_touched(env, n):
    """value bytes and validity bits of `out` from the result length on keep what they held, the bits that share the last row's byte included"""
    K, L, torch = env.K, env.L, env.torch
    rng = np.random.default_rng(n)

    def preset(dtype, rows):
        out = K.Column.empty(dtype, rows, with_validity=True)
        out.values.view(torch.uint8).fill_(0x5A)
        out.validity.fill_(0xA5)
        return out, out.values.view(torch.uint8).cpu().numpy().copy(), out.validity.cpu().numpy().copy()

    def untouched(out, before_vals, before_bits, rows, what, valid_rows=None):
        valid_rows = rows if valid_rows is None else valid_rows
        after_vals, after_bits = out.values.view(torch.uint8).cpu().numpy(), out.validity.cpu().numpy()
        if out.dtype == L.BOOL:
            assert np.array_equal(np.unpackbits(after_vals, bitorder="little")[rows:], np.unpackbits(before_vals, bitorder="little")[rows:]), what
        else:
            width = 4 if out.dtype in (L.INT32, L.FLOAT32) else 8
            assert np.array_equal(after_vals[rows * width:], before_vals[rows * width:]), what
        return np.array_equal(np.unpackbits(after_bits, bitorder="little")[valid_rows:], np.unpackbits(before_bits, bitorder="little")[valid_rows:])

    for dt in ("f64", "f32", "bool"):
        a, valid, cols = frame(env, rng, dt, 3, n, "sparse" if n > 1 else "all_null")
        valid[:, 0] = False
        aligned = dt == "f32" and n in (64, 130)  # (16-byte aligned 4-byte streams: the four-rows-per-lane form)
        cols = [col(env, a[c], valid[c], dt, 0 if aligned else OFFSETS[c]) for c in range(3)]
        # coalesce
        out, bv, bb = preset(env.dts[dt], n + 200)
        m = out.mut()
        assert env.lib.pdx_coalesce(K._col_array(cols), 3, C.byref(m), K._stream()) == L.OK
        out._adopt(m)
        want, want_ok = R.coalesce(a, valid)
        got, ok = host(out, dt)
        assert out.length == n and not R.same_bits(got, ok, want, want_ok) and untouched(out, bv, bb, n, ("coalesce", dt)), ("coalesce", dt)
        # replace_with_mask
        mask = rng.random(n) < 0.5
        repl = draw(rng, dt, int(mask.sum()))
        out, bv, bb = preset(env.dts[dt], n + 200)
        m = out.mut()
        mask_col, repl_col = col(env, mask, None, "bool", 7), col(env, repl, None, dt, 1)  # (held: the structs below only borrow their memory)
        ca, cm, cr = cols[0].c(), mask_col.c(), repl_col.c()
        assert env.lib.pdx_replace_with_mask(C.byref(ca), C.byref(cm), C.byref(cr), C.byref(m), K._stream()) == L.OK
        out._adopt(m)
        want, want_ok = R.replace_with_mask(a[0], valid[0], mask, None, repl, None)
        got, ok = host(out, dt)
        assert out.length == n and not R.same_bits(got, ok, want, want_ok) and untouched(out, bv, bb, n, ("replace", dt)), ("replace", dt)
        if dt == "bool":
            continue
        # min / max and clip
        for which in ("minmax", "clip"):
            out, bv, bb = preset(env.dts[dt], n + 200)
            m = out.mut()
            if which == "minmax":
                assert env.lib.pdx_element_wise_minmax(1, K._col_array(cols), 3, 1, C.byref(m), K._stream()) == L.OK
                want, want_ok = R.element_wise_minmax(1, [(a[c], valid[c], False) for c in range(3)], True)
            else:
                t = R.NP_T[dt]
                lo_col, hi_col = col(env, [t(-1)], None, dt, 1), col(env, [t(1)], np.array([False]), dt, 7)
                cx, cl, ch = cols[0].c(), lo_col.c(), hi_col.c()
                assert env.lib.pdx_clip(C.byref(cx), C.byref(cl), C.byref(ch), 0, C.byref(m), K._stream()) == L.OK
                want, want_ok = R.clip(a[0], valid[0], np.array([-1], t), None, np.array([1], t), np.array([False]), False)
            out._adopt(m)
            got, ok = host(out, dt)
            assert out.length == n and not R.same_minmax(got, ok, want, want_ok) and untouched(out, bv, bb, n, (which, dt)), (which, dt)
    # indices_nonzero: rows past the count; all_valid_mask: bits past n (its validity buffer is not touched at all)
    a = draw(rng, "i64", n)
    out, bv, bb = preset(L.UINT64, n + 200)
    m = out.mut()
    a_col = col(env, a, None, "i64", 13)
    ca = a_col.c()
    assert env.lib.pdx_indices_nonzero(C.byref(ca), C.byref(m), K._stream()) == L.OK
    out._adopt(m)
    want = R.indices_nonzero(a, None)
    assert out.length == len(want) and np.array_equal(out.to_numpy()[0], want) and untouched(out, bv, bb, len(want), "nonzero", 0)
    a, valid, cols = frame(env, rng, "i64", 3, n, "sparse" if n > 1 else "all_null")
    out, bv, bb = preset(L.BOOL, n + 200)
    m = out.mut()
    assert env.lib.pdx_all_valid_mask(K._col_array(cols), 3, C.byref(m), K._stream()) == L.OK
    out._adopt(m)
    assert np.array_equal(out.to_numpy()[0], R.all_valid_mask(list(valid), n)) and untouched(out, bv, bb, n, "all_valid", 0) and m.null_count == 0


def test_same_bits_on_two_streams(env):
    torch, K = env.torch, env.K
    rng = np.random.default_rng(9)
    n = 3 * TILE + 37
    a, valid, cols = frame(env, rng, "f64", 5, n, "sparse")
    mask = col(env, rng.random(n) < 0.4, rng.random(n) >= 0.1, "bool", 7)
    repl = col(env, draw(rng, "f64", n), rng.random(n) >= 0.1, "f64", 1)
    lo, hi = col(env, [-1.0], None, "f64"), col(env, [1.0], None, "f64")
    calls = {"coalesce": lambda: K.coalesce(cols), "max": lambda: K.element_wise_minmax(1, cols, False), "clip": lambda: K.clip(cols[0], lo, hi, True),
             "replace": lambda: K.replace_with_mask(cols[0], mask, repl), "nonzero": lambda: K.indices_nonzero(cols[1]),
             "drop_na": lambda: K.drop_na(cols[:2])[1]}
    for name, fn in calls.items():
        seen = set()
        for k in range(3):
            s = torch.cuda.current_stream() if k == 0 else torch.cuda.Stream()
            with torch.cuda.stream(s):
                rc, out = guarded(env, fn)
                assert rc == env.L.OK, (name, out)
                vals, ok = out.to_numpy()
                s.synchronize()
            seen.add(R.bits(np.asarray(vals)).tobytes() + (b"" if ok is None else ok.tobytes()) + str(out.null_count).encode())
        assert len(seen) == 1, name


# ---------------------------------------------------------------- the Python facade
def test_series_and_dataframe_methods(env):
    api, L = env.api, env.L
    idx = env.K.Column.from_numpy(np.arange(4) * 10)
    a, b, c = np.array([np.nan, 10.0, np.nan, np.nan]), np.array([20.0, 21.0, np.nan, np.nan]), np.array([30.0, np.nan, 32.0, np.nan])
    df = api.DataFrame({"a": a, "b": b, "c": c}, index=idx)  # (NaN is a null on construction)
    s = df.coalesce()
    assert s.name == "" and s.index is idx
    vals, ok = s.to_numpy()
    assert list(ok) == [True, True, True, False] and list(vals[:3]) == [20.0, 10.0, 32.0] and s.col.null_count == 1
    assert list(df.coalesce(["c", "a"]).to_numpy()[0][:2]) == [30.0, 10.0]
    mixed = api.DataFrame({"x": np.array([np.nan, 2.5]), "n": np.array([7, 8])}).coalesce()  # int64 beside float64 is promoted
    assert mixed.dtype() == L.FLOAT64 and list(mixed.values()) == [7.0, 2.5]
    with pytest.raises(L.PdxError):
        api.DataFrame({"x": np.array([1.0]), "f": np.array([True])}).coalesce()
    kept = df.drop_na()
    assert kept.num_rows() == 0
    kept = api.DataFrame({"a": np.array([1.0, np.nan, 3.0]), "n": np.array([7, 8, 9])}, index=np.array([1, 4, 5])).drop_na()
    assert list(kept["a"].values()) == [1.0, 3.0] and list(kept["n"].values()) == [7, 9] and list(kept.index.to_numpy()[0]) == [1, 5]
    x = api.Series(np.array([-5.0, 0.5, np.nan, 7.0]), index=idx)
    clipped = x.clip(x, 0.0, 2.0)
    assert list(clipped.values()) == [0.0, 0.5, 2.0, 2.0] and clipped.index is idx
    assert list(x.clip(x, 0, 2, False).to_numpy()[1]) == [True, True, False, True]
    assert list(x.clip(x, api.Scalar(0.0), None).values())[3] == 7.0  # a null bound does not bound when nulls are skipped
    assert x.clip(x, 0.0, None, False).col.null_count == 4
    ints = api.Series(np.array([1, 2, 3, 4, 5, 6, 7]))
    r = ints.replace_with_mask(api.Series(np.array([True, True, True, False, False, True, True])), api.Series(np.array([10, 20, 30, 40, 50, 60, 70])))
    assert list(r.values()) == [10, 20, 30, 4, 5, 40, 50]
    with pytest.raises(L.PdxError, match="replace_with_mask error: valid precondition"):
        ints.replace_with_mask(api.Series(np.array([True] * 7)), api.Series(np.array([1, 2, 3])))
    assert list(api.Series(np.array([0, 0, 0, 1, 2, 0, 3, 0, 4, 5, 0])).indices_nonzero().values()) == [3, 4, 6, 8, 9]
    labelled = api.Series(np.array([5.0, np.nan, 7.0, np.nan]), index=idx).drop_na()  # a shorter result keeps the LAST labels, as the reference does
    assert list(labelled.values()) == [5.0, 7.0] and list(labelled.index.to_numpy()[0]) == [20, 30]
