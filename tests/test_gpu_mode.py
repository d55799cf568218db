"""GPU: pdx_mode through the C ABI (pandasarrow_amd/column.py) against tests/golden/mode_golden.npz (Arrow C++ 25) and the numpy
restatement tests/_mode_ref.py.  Everything is bit-exact, a NaN by its bits; the sign of a returned zero is ignored only against the golden's
zeros_* cases (Arrow's pick), never against the restatement, which states this library's rule (the first zero in row order).  No pyarrow."""
import ctypes as C

import numpy as np
import pytest

import _mode_ref as R

pytestmark = pytest.mark.gpu

GOLD = R.ModeGolden()
BINS = 8192  # kModeBins (pandasarrow_amd/csrc/mode.hip)
PATTERN = 0x5A


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


def run(env, a, valid, dt, n=1, skip=True, min_count=0, offset=0):
    modes, counts = env.K.mode(column(env, a, valid, dt, offset), n, skip, min_count)
    assert modes.length == counts.length and modes.null_count == 0 and counts.null_count == 0
    return modes.to_numpy()[0], counts.to_numpy()[0], env.K.mode_last_plan()


def check(env, a, valid, dt, n=1, skip=True, min_count=0, offset=0, path=None):
    a = np.asarray(a, R.NP_DTYPES[dt])
    got, counts, plan = run(env, a, valid, dt, n, skip, min_count, offset)
    want, want_counts = R.mode(a, valid, n, skip, min_count)
    assert R.same_values(got, want), (dt, len(a), n, got[:4], want[:4])
    assert np.array_equal(counts, want_counts), (dt, len(a), n)
    if path:
        assert plan["path"] == path, plan
    return plan


@pytest.mark.parametrize("dt", R.MODE_DTYPES)
def test_golden_through_the_abi(env, dt):
    for c in (c for c in GOLD.cases if c["kind"] == "mode" and c["dtype"] == dt):
        a, valid = GOLD.inputs(c)
        want, _, want_counts = GOLD.expected(c)
        got, counts, _ = run(env, a, None if valid.all() else valid, dt, c["n"], bool(c["skip_nulls"]), c["min_count"])
        assert R.same_values(got, want, ignore_zero_sign=c["name"].startswith("zeros_")), c["name"]
        assert np.array_equal(counts, want_counts), c["name"]


def test_golden_through_the_facade(env):
    for name in ("sp_nan_wins", "sp_tie_at_nth", "sp_bool_tie", "sp_only_nulls", "sp_n_beyond_distinct"):
        c = GOLD.by_name[name]
        a, valid = GOLD.inputs(c)
        want, _, want_counts = GOLD.expected(c)
        s = env.api.Series(env.K.Column.from_numpy(a, None if valid.all() else valid, dtype=env.dts[c["dtype"]]))
        res = s.mode(c["n"], bool(c["skip_nulls"]), c["min_count"])
        assert [m.count for m in res] == want_counts.tolist(), name
        got = np.array([m.mode.value for m in res], want.dtype)
        assert R.same_values(got, want), name


def random_column(rng, dt, n, distinct):
    if dt in ("f64", "f32"):
        a = (rng.integers(0, distinct, n) - distinct // 2).astype(R.NP_DTYPES[dt]) * R.NP_DTYPES[dt](1.5)
        if n > 8:
            a[rng.integers(0, n, max(1, n // 16))] = np.nan
            a[rng.integers(0, n, max(1, n // 32))] = -0.0
    elif dt == "bool":
        a = rng.random(n) < 0.5
    elif dt == "u64":
        a = rng.integers(0, distinct, n).astype(np.uint64) + np.uint64(2**63 - distinct // 2)
    else:
        a = (rng.integers(0, distinct, n) - distinct // 2).astype(R.NP_DTYPES[dt])
    return a


@pytest.mark.parametrize("dt", R.MODE_DTYPES)
def test_lengths_at_wave_and_tile_edges(env, dt):
    rng = np.random.default_rng(11)
    for n in (0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1):
        for distinct in (7, 20000):  # counting path, sort path (integers)
            a = random_column(rng, dt, n, distinct)
            valid = rng.random(n) > 0.2
            check(env, a, valid, dt, 1)
            check(env, a, None, dt, 3)


@pytest.mark.parametrize("dt", R.MODE_DTYPES)
@pytest.mark.parametrize("offset", [0, 1, 7, 13])
def test_offsets_and_validity_shapes(env, dt, offset):
    rng = np.random.default_rng(100 + offset)
    for distinct in (5, 30000):
        a = random_column(rng, dt, 1000, distinct)
        valid = rng.random(1000) > 0.3
        check(env, a, valid, dt, 4, offset=offset)         # validity at bit offset `offset`, null_count -1
        check(env, a, None, dt, 4, offset=offset)          # no validity buffer at all


@pytest.mark.parametrize("dt", ["i64", "f64", "i32", "bool"])
def test_many_workgroups(env, dt):
    """300 000 rows: more than one workgroup adds to the global histogram, and a run crosses many sort tiles"""
    rng = np.random.default_rng(5)
    a = random_column(rng, dt, 300_000, 50)
    valid = rng.random(300_000) > 0.1
    check(env, a, valid, dt, 10, path="bool" if dt == "bool" else "sort" if dt == "f64" else "count")
    if dt != "bool":
        a = random_column(rng, dt, 300_000, 100_000)
        a[1000:120_000] = a[0]  # one long run over many tiles
        check(env, a, valid, dt, 5, path="sort")


@pytest.mark.parametrize("dt", ["i64", "u64", "i32"])
def test_counting_threshold(env, dt):
    """a value range of exactly kModeBins is counted, of kModeBins + 1 sorted: asserted through pdx_mode_last_plan"""
    rng = np.random.default_rng(9)
    np_dt = R.NP_DTYPES[dt]
    base = {"i64": -4000, "u64": 2**63 - 4000, "i32": -4000}[dt]
    for width, path in ((BINS, "count"), (BINS + 1, "sort")):
        a = rng.integers(0, width, 20_000).astype(np_dt) + np_dt(base)
        a[0], a[1] = np_dt(base), np_dt(base + width - 1)
        a[2:40] = np_dt(base + width - 1)  # the mode lies in the last bin
        plan = check(env, a, None, dt, 3, path=path)
        if path == "count":
            assert int(plan["width"]) == BINS and int(plan["bins"]) == BINS
    # min / max are taken over the VALID rows: a null row far outside the range does not widen it
    valid = np.ones(20_000, bool)
    valid[1] = False
    a[1] = np_dt(base + 2 * BINS)
    check(env, a, valid, dt, 2, path="sort")  # (valid rows still span kModeBins + 1 values)
    a[a == np_dt(base + BINS)] = np_dt(base)
    a[1] = np_dt(base + 2 * BINS)
    check(env, a, valid, dt, 2, path="count")


def test_counting_path_extremes(env):
    i64 = np.array([-2**63, 2**63 - 1, 2**63 - 1, -2**63, 5, 2**63 - 1], np.int64)
    check(env, i64, None, "i64", 3, path="sort")  # the width wraps to 0 in 64 bits: not a narrow range
    check(env, np.array([2**63 - 1] * 3 + [2**63 - 2], np.int64), None, "i64", 2, path="count")
    check(env, np.array([-2**63] * 3 + [-2**63 + 7] * 4, np.int64), None, "i64", 2, path="count")
    u = np.array([2**63 - 1, 2**63, 2**63 + 1, 2**63, 2**63 + 1, 2**63 - 1, 2**63], np.uint64)
    check(env, u, None, "u64", 3, path="count")
    check(env, np.array([2**64 - 1, 2**64 - 1, 0, 2**64 - 2], np.uint64), None, "u64", 3, path="sort")
    check(env, np.array([2**64 - 1, 2**64 - 1, 2**64 - 3], np.uint64), None, "u64", 3, path="count")
    check(env, np.array([-5, -7, -7, -2**31, -5, -7, 3], np.int32), None, "i32", 4, path="sort")
    check(env, np.array([-5, -7, -7, -900, -5, -7, 3], np.int32), None, "i32", 4, path="count")


@pytest.mark.parametrize("share", [0.9, 1.0])
def test_hot_value(env, share):
    rng = np.random.default_rng(3)
    n = 70_001
    a = rng.integers(-100, 100, n).astype(np.int64)
    a[rng.random(n) < share] = 42
    if share == 1.0:
        a[:] = 42
    check(env, a, None, "i64", 1, path="count")
    check(env, a, rng.random(n) > 0.5, "i64", 3, path="count")
    check(env, a.astype(np.int32), None, "i32", 2, path="count")


def test_bool_shapes(env):
    t, f = True, False
    check(env, [t, f, t], np.zeros(3, bool), "bool", 2, path="empty")               # 0 distinct valid values
    check(env, [t, t, f], np.array([t, t, f]), "bool", 2, path="bool")              # 1
    check(env, [f, f, t], np.array([t, t, f]), "bool", 2, path="bool")
    check(env, [t, f, t, t], None, "bool", 2, path="bool")                          # 2
    check(env, [t, f, t, f], None, "bool", 2, path="bool")                          # an exact tie: false first
    check(env, [t, f, t, f], None, "bool", 1, path="bool")
    rng = np.random.default_rng(2)
    for n in (64, 65, 129, 5000):
        check(env, rng.random(n) < 0.5, rng.random(n) < 0.7, "bool", 2, offset=5)


def test_sort_path_runs(env):
    n = 4096 * 3
    b = np.arange(n, dtype=np.int64) * 1_000_003
    b[-5:] = b[4095]  # sorted: a run of 6 that starts at position 4095, the last row of the first tile
    check(env, b, None, "i64", 2, path="sort")
    check(env, b.astype(np.float64), None, "f64", 2, path="sort")
    # two runs of equal count: the smaller value first
    c = np.array([9e15, -9e15, 9e15, -9e15, 1e300, 3.5], np.float64)
    got, counts, _ = run(env, c, None, "f64", 2)
    assert got.tolist() == [-9e15, 9e15] and counts.tolist() == [2, 2]
    check(env, np.array([2**62, -2**62, 2**62, -2**62, 7], np.int64), None, "i64", 3, path="sort")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_nan_runs_and_zeros(env, dt):
    np_dt = R.NP_DTYPES[dt]
    ut = np.uint32 if dt == "f32" else np.uint64
    qnan = int(R.bits(np.array([np.nan], np_dt))[0])
    sign = 1 << (np.dtype(np_dt).itemsize * 8 - 1)
    nans = np.array([qnan, qnan | 1, qnan | sign, qnan | sign | 77, qnan | 2], ut).view(np_dt)
    a = np.concatenate([nans, np.array([1.5, 1.5, np.inf, -np.inf, 1.5], np_dt), nans[:2]])
    got, counts, _ = run(env, a, None, dt, 2)
    assert int(R.bits(got)[0]) == qnan and counts.tolist() == [7, 3]  # every NaN is one value, returned canonical
    check(env, a, None, dt, 5, path="sort")
    valid = np.ones(len(a), bool)
    valid[[0, 6]] = False
    check(env, a, valid, dt, 5, path="sort")
    # both zeros interleaved: one value, returned as the first zero in row order -- with its sign
    z = np.array([3.0, -0.0, 0.0, -0.0, 0.0, 3.0, 0.0], np_dt)
    got, counts, _ = run(env, z, None, dt, 1)
    assert counts.tolist() == [5] and got[0] == 0 and np.signbit(got[0])
    got, counts, _ = run(env, z[::-1].copy(), None, dt, 2)
    assert counts.tolist() == [5, 2] and got[0] == 0 and not np.signbit(got[0])
    vz = np.ones(7, bool)
    vz[1] = False  # the first zero is null: the next one counts
    got, counts, _ = run(env, z, vz, dt, 1)
    assert counts.tolist() == [4] and not np.signbit(got[0])
    check(env, z, vz, dt, 3)
    rng = np.random.default_rng(8)
    big = rng.choice(np.array([0.0, -0.0, 1.0, np.nan], np_dt), 9000)
    check(env, big, rng.random(9000) > 0.2, dt, 4, offset=3)


@pytest.mark.parametrize("dt", ["i64", "f64", "i32"])
def test_n_values(env, dt):
    rng = np.random.default_rng(4)
    for distinct in (37, 9001):
        a = random_column(rng, dt, 12_000, distinct)
        d = len(R.mode(a, None, 2**40)[0])
        for n in (1, 2, d, d + 1, 2**40):
            got, counts, _ = run(env, a, None, dt, n)
            want, want_counts = R.mode(a, None, n)
            assert len(got) == min(n, d)
            assert R.same_values(got, want) and np.array_equal(counts, want_counts), (dt, distinct, n)


def raw_call(env, col, n, modes, counts, skip=1, min_count=0, stream=None):
    ca, mm, mc = col.c(), modes.mut(), counts.mut()
    rc = env.lib.pdx_mode(C.byref(ca), int(n), int(skip), int(min_count), C.byref(mm), C.byref(mc), env.K._stream() if stream is None else stream)
    return rc, env.lib.pdx_last_error().decode() if rc != env.L.OK else "", mm, mc


def patterned(env, dt, n):
    c = env.K.Column.empty(env.dts[dt], n)
    c.values.view(env.torch.uint8).fill_(PATTERN)
    return c


def test_refusals_leave_the_outputs_alone(env):
    L, K = env.L, env.K
    a = column(env, np.array([3, 1, 3, 2, 2, 3, 9], np.int64), None, "i64")
    ts = column(env, np.array([3, 1], np.int64), None, "ts")

    def refused(col, n, modes_dt, counts_dt, cap, status, text):
        modes, counts = patterned(env, modes_dt, cap), patterned(env, counts_dt, cap)
        rc, msg, _, _ = raw_call(env, col, n, modes, counts)
        assert rc == status and text in msg, (rc, msg)
        for c in (modes, counts):
            assert (c.values.view(env.torch.uint8) == PATTERN).all()

    refused(a, 0, "i64", "i64", 4, L.INVALID, R.N_ERROR)
    refused(a, -1, "i64", "i64", 4, L.INVALID, R.N_ERROR)
    refused(a, 3, "f64", "i64", 4, L.INVALID, "the modes have the input's dtype")
    refused(a, 3, "i64", "f64", 4, L.INVALID, "the counts are int64")
    refused(a, 3, "i64", "i64", 2, L.INVALID, "output too small")          # capacity one short of min(n, length)
    refused(a, 100, "i64", "i64", 6, L.INVALID, "output too small")
    refused(ts, 1, "ts", "i64", 4, L.NOT_IMPLEMENTED, R.TS_ERROR)
    # a success writes k rows and nothing beyond them
    for col, dt, k_want in ((a, "i64", 3), (column(env, np.array([1e300, 2.0, 2.0, 1e300, 5.0]), None, "f64"), "f64", 2)):
        modes, counts = patterned(env, dt, 6), patterned(env, "i64", 6)
        rc, msg, mm, mc = raw_call(env, col, k_want, modes, counts)
        assert rc == L.OK, msg
        assert mm.length == k_want and mc.length == k_want and mm.null_count == 0
        assert (modes.values.view(env.torch.uint8)[8 * k_want:] == PATTERN).all() and (counts.values.view(env.torch.uint8)[8 * k_want:] == PATTERN).all()
    assert counts.values[:2].cpu().tolist() == [2, 2] and modes.values[:2].cpu().tolist() == [2.0, 1e300]
    # bool: the bits beyond k stay
    b = column(env, np.array([True, False, True]), None, "bool")
    modes, counts = K.Column.empty(L.BOOL, 8), patterned(env, "i64", 8)
    modes.values.fill_(0xAA)
    rc, msg, mm, _ = raw_call(env, b, 5, modes, counts)
    assert rc == L.OK and mm.length == 2
    assert int(modes.values[0]) == (0xAA & ~3) | 0b01 and (modes.values[1:] == 0xAA).all()  # (true, 2), (false, 1)
    # an empty result writes nothing
    modes, counts = patterned(env, "i64", 4), patterned(env, "i64", 4)
    rc, msg, mm, mc = raw_call(env, a, 2, modes, counts, min_count=100)
    assert rc == L.OK and mm.length == 0 and mc.length == 0 and (modes.values.view(env.torch.uint8) == PATTERN).all()


@pytest.mark.parametrize("dt", ["i64", "f64", "f32", "bool"])
def test_two_streams_same_bytes(env, dt):
    rng = np.random.default_rng(6)
    a = random_column(rng, dt, 50_000, 300)
    col = column(env, a, rng.random(50_000) > 0.1, dt)
    outs = []
    for _ in range(2):
        st = env.torch.cuda.Stream()
        with env.torch.cuda.stream(st):
            modes, counts = env.K.mode(col, 7)
            st.synchronize()
            outs.append((modes.values.cpu().numpy().tobytes()[: 8 if dt == "bool" else modes.length * modes.values.element_size()], counts.values.cpu().numpy()[: counts.length].tobytes()))
    assert outs[0] == outs[1]
