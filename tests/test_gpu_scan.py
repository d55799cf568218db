"""GPU: pdx_cumulative / pdx_fill_null / pdx_shift through the C ABI and the Python facade, against tests/golden/scan_golden.npz (Arrow C++ 25)
and the numpy restatement tests/_scan_ref.py.  No pyarrow, no oracle binaries.

Bit-exact: integer sum / product, max / min, fills, shift, and float sums / products whose partial results are exactly representable.
Float sum / product otherwise: deterministic (same bits at any slice offset, on any stream, with any chunk length), inside the a-priori
bound of any summation order (exact arithmetic in fractions), NaN / infinities where Arrow has them."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _scan_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = R.ScanGolden()
OPS = {"sum": 0, "prod": 1, "max": 2, "min": 3}


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column as K

    lib = L.load()
    L.check(lib.pdx_init(0))
    dts = {"i64": L.INT64, "u64": L.UINT64, "f64": L.FLOAT64, "i32": L.INT32, "f32": L.FLOAT32, "ts": L.TIMESTAMP_NS, "bool": L.BOOL}
    return type("Env", (), {"torch": torch, "L": L, "K": K, "api": api, "lib": lib, "dts": dts})


def column(env, a, valid, dt, offset=0):
    return env.K.Column.from_numpy(np.asarray(a), valid, dtype=env.dts[dt], offset=offset)


def call(env, fn, col, with_validity, *args):
    """one ABI call into a fresh output column -> (status, values, valid | None, null_count)"""
    K, L = env.K, env.L
    out = K.Column.empty(col.dtype, col.length, with_validity=with_validity)
    ca, m = col.c(), out.mut()
    st = K._stream()
    if fn == "cum":
        op, start, skip = args
        rc = env.lib.pdx_cumulative(op, C.byref(ca), float(start), int(skip), C.byref(m), st)
    elif fn == "fill":
        rc = env.lib.pdx_fill_null(int(args[0]), C.byref(ca), C.byref(m), st)
    else:
        rc = env.lib.pdx_shift(C.byref(ca), int(args[0]), args[1], C.byref(m), st)
    if rc != L.OK:
        return rc, env.lib.pdx_last_error().decode(), None, None
    out._adopt(m)
    vals, valid = out.to_numpy()
    return rc, vals, valid, out.null_count


def check_exact(got, got_valid, nulls, want_bits, want_valid):
    if got_valid is None:
        assert want_valid.all()
        got_valid = np.ones(len(got), bool)
    assert np.array_equal(got_valid, want_valid)
    assert nulls == int((~want_valid).sum())
    assert np.array_equal(R.bits(got)[want_valid], want_bits[want_valid])


# ---------------------------------------------------------------- goldens
@pytest.mark.parametrize("offset", [0, 3])
def test_golden_cumulative(env, offset):
    ran = 0
    for case in GOLD.cases:
        if case["fn"] != "cum" or "error" in case:
            continue
        a, valid = GOLD.inputs(case)
        want, want_valid = GOLD.expected(case)
        col = column(env, a, valid, case["dtype"], offset)
        for with_validity in ((True, False) if valid is None else (True,)):
            rc, got, got_valid, nulls = call(env, "cum", col, with_validity, OPS[case["op"]], float(case["start"]), case["skip_nulls"])
            assert rc == env.L.OK, (case["name"], got)
            if case["compare"] == "exact":
                check_exact(got, got_valid, nulls, want, want_valid)
            else:
                arrow = want.view(a.dtype)
                assert got_valid is None or np.array_equal(got_valid, want_valid), case["name"]
                assert nulls == int((~want_valid).sum())
                assert R.same_special(got[want_valid], arrow[want_valid]), case["name"]
                bad, worst = R.bound_violations(case["op"], got, a, valid, float(case["start"]))
                print(case["name"], "offset", offset, "largest error in u * S_i:", worst)
                assert not bad, (case["name"], bad[:5])
            ran += 1
    assert ran > 1000


@pytest.mark.parametrize("offset", [0, 3])
def test_golden_fill(env, offset):
    ran = 0
    for case in GOLD.cases:
        if case["fn"] != "fill":
            continue
        a, valid = GOLD.inputs(case)
        col = column(env, a, valid, case["dtype"], offset)
        if "slice" in case:
            col = col.slice(*case["slice"])
        want, want_valid = GOLD.expected(case)
        for with_validity in ((True, False) if valid is None else (True,)):
            rc, got, got_valid, nulls = call(env, "fill", col, with_validity, case["backward"])
            assert rc == env.L.OK, (case["name"], got)
            check_exact(got, got_valid, nulls, want, want_valid)
            ran += 1
    assert ran > 280


def test_golden_errors_verbatim(env):
    ran = 0
    for case in GOLD.cases:
        if "error" not in case:
            continue
        a, valid = GOLD.inputs(case)
        col = column(env, a, valid, case["dtype"])
        rc, msg, _, _ = call(env, "cum", col, True, OPS[case["op"]], float(case["start"]), 1)
        assert rc == (env.L.NOT_IMPLEMENTED if case["status"] == "not_implemented" else env.L.INVALID), case["name"]
        assert msg == case["error"], case["name"]
        ran += 1
    assert ran == 14
    b = column(env, np.array([True, False]), None, "bool")
    for fn, args in (("fill", (0,)), ("shift", (1, None))):
        rc, msg, _, _ = call(env, fn, b, True, *args)
        assert rc == env.L.NOT_IMPLEMENTED and "bool" in msg


def test_refusals(env):
    K, L = env.K, env.L
    col = column(env, np.arange(10.0), None, "f64")
    ca = col.c()
    m = col.mut()  # in place: out aliases the input
    for rc in (env.lib.pdx_cumulative(0, C.byref(ca), 0.0, 1, C.byref(m), K._stream()), env.lib.pdx_fill_null(0, C.byref(ca), C.byref(m), K._stream()),
               env.lib.pdx_shift(C.byref(ca), 1, None, C.byref(m), K._stream())):
        assert rc == L.INVALID and "in-place" in env.lib.pdx_last_error().decode()
    valid = np.arange(10) % 3 != 0
    nulls = column(env, np.arange(10.0), valid, "f64")
    for fn, args in (("cum", (0, 0.0, 1)), ("fill", (0,)), ("shift", (1, None))):  # a result that can hold nulls needs a validity buffer
        rc, msg, _, _ = call(env, fn, nulls, False, *args)
        assert rc == L.INVALID and "validity" in msg
    rc, msg, _, _ = call(env, "shift", col, False, 2, None)
    assert rc == L.INVALID and "validity" in msg
    wrong = L.PdxScalar(L.INT64, 1)
    rc, msg, _, _ = call(env, "shift", col, True, 1, C.byref(wrong))
    assert rc == L.INVALID and "fill value" in msg
    rc, msg, _, _ = call(env, "cum", col, True, 9, 0.0, 1)
    assert rc == L.INVALID


# ---------------------------------------------------------------- random columns against the restatement
def random_values(rng, op, dt, n, exact=True):
    t = R.NP_T[dt]
    if dt[0] == "f":
        if op == "sum":
            return (rng.integers(-1000, 1000, n) / 8.0).astype(t) if exact else (rng.standard_normal(n) * 100).astype(t)
        if op == "prod":
            if not exact:
                return (1 + rng.uniform(-0.05, 0.05, n)).astype(t)
            # +-1 with about a hundred factors of 2 or 1/2: whichever rows are null, no partial product leaves 2^+-120, so that
            # every order of evaluation is exact in float32 as well
            e = np.where(rng.random(n) < 1e-4 * min(1.0, 1e6 / n), rng.choice([-1, 1], n), 0)
            return (2.0 ** e * rng.choice([-1.0, 1.0], n)).astype(t)
        v = rng.standard_normal(n) * 100
        v[rng.integers(0, n, n // 50)] = np.nan
        v[rng.integers(0, n, n // 50)] = 0.0
        v[rng.integers(0, n, n // 50)] = -0.0
        return v.astype(t)
    info = np.iinfo(t)
    return rng.integers(info.min // 2 if op != "prod" else -9, info.max // 2 if op != "prod" else 9, n).astype(t)


@pytest.mark.parametrize("dt", ["i64", "u64", "f64", "i32", "f32"])
@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
def test_random_columns(env, op, dt):
    rng = np.random.default_rng(zlib.crc32(f"{op}-{dt}".encode()))  # the same columns in every run
    n = 1_000_037
    a = random_values(rng, op, dt, n) if dt != "u64" else np.abs(random_values(rng, op, "i64", n)).astype(np.uint64)
    valid = rng.random(n) >= 0.1
    start = 3.0 if dt == "u64" else -3.0
    for v, skip, offset in ((None, 1, 0), (valid, 1, 0), (valid, 0, 5), (valid, 1, 3)):
        want, want_valid = R.cumulative(op, a, v, start, bool(skip))
        rc, got, got_valid, nulls = call(env, "cum", column(env, a, v, dt, offset), True, OPS[op], start, skip)
        assert rc == env.L.OK, got
        check_exact(got, got_valid, nulls, R.bits(want), want_valid)


@pytest.mark.parametrize("dt", ["i64", "u64", "f64", "i32", "f32", "ts"])
def test_random_fill_and_shift(env, dt):
    rng = np.random.default_rng(7)
    n = 1_000_037
    a = rng.integers(0, 2**31 - 1, n).astype(R.NP_T[dt])
    valid = rng.random(n) >= 0.5
    valid[:70] = False
    valid[-70:] = False
    for back in (0, 1):
        for offset in (0, 3):
            want, want_valid = R.fill_null(a, valid, bool(back))
            rc, got, got_valid, nulls = call(env, "fill", column(env, a, valid, dt, offset), True, back)
            assert rc == env.L.OK, got
            check_exact(got, got_valid, nulls, R.bits(want), want_valid)
    L = env.L
    fill = L.PdxScalar(env.dts[dt], 1)
    if dt[0] == "f":
        fill.v.f64 = 2.5
    else:
        fill.v.i64 = 41
    fill_py = 2.5 if dt[0] == "f" else 41
    for periods in (0, 1, -2, n, -n - 3, 4099):
        for v in (None, valid):
            for f in (None, fill):
                want, want_valid = R.shift(a, v, periods, None if f is None else fill_py)
                rc, got, got_valid, nulls = call(env, "shift", column(env, a, v, dt, 3), True, periods, None if f is None else C.byref(f))
                assert rc == env.L.OK, got
                check_exact(got, got_valid, nulls, R.bits(want), want_valid)
    rc, got, got_valid, nulls = call(env, "shift", column(env, a, None, dt), False, -5, C.byref(fill))  # no nulls possible: no bitmap needed
    assert rc == env.L.OK and got_valid is None and nulls == 0
    assert np.array_equal(got, R.shift(a, None, -5, fill_py)[0])


# ---------------------------------------------------------------- the float contract
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("op", ["sum", "prod"])
def test_float_results_stay_inside_the_a_priori_bound(env, op, dt):
    rng = np.random.default_rng(11)
    n = 100_000 if op == "sum" else 20_000
    a = random_values(rng, op, dt, n, exact=False)
    valid = rng.random(n) >= 0.05
    start = 0.25 if op == "sum" else 1.0
    for v in (None, valid):
        rc, got, got_valid, _ = call(env, "cum", column(env, a, v, dt), True, OPS[op], start, 1)
        assert rc == env.L.OK, got
        bad, worst = R.bound_violations(op, got, a, v, start)
        seq = R.cumulative(op, a, v, start)[0]
        _, worst_seq = R.bound_violations(op, seq, a, v, start)
        print(f"{op} {dt} n={n} nulls={v is not None}: largest error in u * S_i: this library {worst:.3f}, sequential (Arrow's order) {worst_seq:.3f}")
        assert not bad, bad[:5]


def test_float_special_values_sit_where_arrows_do(env):
    a = np.array([1.0, np.inf, 2.0, -np.inf, 3.0, np.nan, 4.0] + [1.0] * 5000)
    for op in ("sum", "prod"):
        for cut in (7, len(a)):
            x = a[:cut].copy()
            want = R.cumulative(op, x, None, 1.0)[0]
            rc, got, _, _ = call(env, "cum", column(env, x, None, "f64"), True, OPS[op], 1.0, 1)
            assert rc == env.L.OK and R.same_special(got, want)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def determinism_inputs():
    rng = np.random.default_rng(5)
    n = 1_000_037
    out = {}
    for dt in ("f64", "f32"):
        out["sum", dt] = (rng.standard_normal(n) * 100).astype(R.NP_T[dt])
        out["prod", dt] = (1 + rng.uniform(-0.05, 0.05, n)).astype(R.NP_T[dt])
    return out, rng.random(n) >= 0.1


def test_float_bits_do_not_depend_on_offset_or_stream(env):
    torch = env.torch
    data, valid = determinism_inputs()
    for (op, dt), a in data.items():
        seen = set()
        for offset in (0, 1, 5):
            rc, got, _, _ = call(env, "cum", column(env, a, valid, dt, offset), True, OPS[op], 0.5, 1)
            assert rc == env.L.OK
            seen.add(digest(R.bits(got)[valid]))
        for _ in range(2):
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                rc, got, _, _ = call(env, "cum", column(env, a, valid, dt, 1), True, OPS[op], 0.5, 1)
                s.synchronize()
            assert rc == env.L.OK
            seen.add(digest(R.bits(got)[valid]))
        assert len(seen) == 1, (op, dt)


CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import test_gpu_scan as T
from pandasarrow_amd import _lib as L, column as K
L.check(L.load().pdx_init(0))
data, valid = T.determinism_inputs()
for (op, dt), a in sorted(data.items()):
    col = K.Column.from_numpy(a, valid, dtype={{"f64": L.FLOAT64, "f32": L.FLOAT32}}[dt])
    got = K.cumulative(T.OPS[op], col, 0.5).to_numpy()[0]
    print("DIGEST", op, dt, T.digest(T.R.bits(got)[valid]))
ints = np.random.default_rng(9).integers(-2**62, 2**62, 300_001)
want = T.R.cumulative("sum", ints, valid[:300_001], -3.0)[0]
got = K.cumulative(0, K.Column.from_numpy(ints, valid[:300_001]), -3.0).to_numpy()[0]
print("INT64", bool(np.array_equal(got[valid[:300_001]], want[valid[:300_001]])))
"""


def run_child(chunk_rows):
    e = dict(os.environ)
    e.pop("PDX_SCAN_CHUNK_ROWS", None)
    if chunk_rows is not None:
        e["PDX_SCAN_CHUNK_ROWS"] = str(chunk_rows)
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-s", "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(("DIGEST", "INT64"))]
    assert len(lines) == 5 and lines[-1] == "INT64 True", lines
    return lines


def test_float_bits_do_not_depend_on_the_chunk_length(env):
    """the library reads PDX_SCAN_CHUNK_ROWS once: each setting runs in a fresh child process"""
    default, small, plain = run_child(None), run_child(8192), run_child(0)
    assert default == small == plain
    data, valid = determinism_inputs()
    for line in default[:4]:
        _, op, dt, d = line.split()
        rc, got, _, _ = call(env, "cum", column(env, data[op, dt], valid, dt, 5), True, OPS[op], 0.5, 1)
        assert digest(R.bits(got)[valid]) == d


# ---------------------------------------------------------------- full size: one chunk (the default) and many chunks
def full_size_case():
    """int64 cumsum and float64 cummax of 3e8 rows with 1 % nulls against the restatement, bit for bit, with the exact null count"""
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column as K

    L.check(L.load().pdx_init(0))
    n = 300_000_000
    rng = np.random.default_rng(3)
    valid = rng.random(n) >= 0.01
    for op, dt in (("sum", L.INT64), ("max", L.FLOAT64)):
        a = rng.integers(-2**40, 2**40, n) if dt == L.INT64 else rng.standard_normal(n)
        want, want_valid = R.cumulative(op, a, valid, -7.0)
        col = K.Column.from_numpy(a, valid, dtype=dt)
        out = K.cumulative(OPS[op], col, -7.0)
        assert out.null_count == int((~valid).sum())
        got, got_valid = out.to_numpy()
        assert np.array_equal(got_valid, want_valid)
        assert np.array_equal(R.bits(got)[valid], R.bits(want)[valid])
        del col, out, got, want
        torch.cuda.empty_cache()


def test_full_size_one_chunk(env):
    """the shipped default: the whole column in one round of reduce / scan / apply"""
    full_size_case()


# 4133 tiles per chunk: 36 chunks whose boundaries cut groups of 64 tiles and supergroups of 4096, byte offsets beyond 2^31
FULL_SIZE_CHUNK_ROWS = (1 << 23) + 37 * 2048
FULL_SIZE_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_scan as T
T.full_size_case()
print("FULL SIZE OK")
"""


def test_full_size_many_chunks():
    """the same case walked in chunks, in a fresh child process (the library reads PDX_SCAN_CHUNK_ROWS once), under its own time limit"""
    e = dict(os.environ, PDX_SCAN_CHUNK_ROWS=str(FULL_SIZE_CHUNK_ROWS))
    code = FULL_SIZE_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-s", "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FULL SIZE OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


# ---------------------------------------------------------------- facades
def test_series_and_dataframe_methods(env):
    api, L = env.api, env.L
    v = np.array([1.0, np.nan, 3.0, np.nan, np.nan, 6.0, np.nan])
    idx = env.K.Column.from_numpy(np.arange(7) * 10)
    s = api.Series(v, index=idx, name="px")
    ok = ~np.isnan(v)
    for name, args, want in (("cumsum", (), R.cumulative("sum", v, ok, 0.0)), ("cumprod", (), R.cumulative("prod", v, ok, 1.0)),
                             ("cummax", (2.0,), R.cumulative("max", v, ok, 2.0)), ("cummin", (2.0,), R.cumulative("min", v, ok, 2.0)),
                             ("cumsum", (1.0, False), R.cumulative("sum", v, ok, 1.0, False)), ("ffill", (), R.fill_null(v, ok)),
                             ("bfill", (), R.fill_null(v, ok, True)), ("shift", (), R.shift(v, ok, 1)), ("shift", (-2, 9.0), R.shift(v, ok, -2, 9.0))):
        r = getattr(s, name)(*args)
        got, got_valid = r.to_numpy()
        got_valid = np.ones(7, bool) if got_valid is None else got_valid
        assert np.array_equal(got_valid, want[1]) and np.array_equal(got[want[1]], want[0][want[1]]), name
        assert r.name == "px" and r.index is idx, name
    with pytest.raises(TypeError):
        s.cummax()
    with pytest.raises(L.PdxError, match="truncated converting to int64"):
        api.Series(np.array([1, 2, 3])).cumsum(0.5)
    i32 = api.Series(np.array([2**31 - 1, 1]), dtype=L.INT32).cumsum()
    assert i32.dtype() == L.INT32 and list(i32.values()) == [2**31 - 1, -2**31]
    df = api.DataFrame({"a": api.Series(v), "b": api.Series(np.array([1, 2, 3, 4, 5, 6, 7]), valid=ok)}, index=idx)
    for back in (False, True):
        r = df.bfill() if back else df.ffill()
        for name, src in (("a", v), ("b", np.arange(1, 8))):
            want, want_valid = R.fill_null(src, ok, back)
            got, got_valid = r[name].to_numpy()
            assert np.array_equal(got_valid, want_valid) and np.array_equal(got[want_valid], want[want_valid])
        assert r.index is idx
    flags = api.DataFrame({"a": api.Series(v), "flag": api.Series(np.array([True, False] * 3 + [True]))})
    with pytest.raises(L.PdxError, match="bool"):
        flags.ffill()
