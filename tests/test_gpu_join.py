"""GPU: pdx_join_create / pdx_join_rows / pdx_join_indices through the C ABI (pandasarrow_amd/column.py) against tests/golden/join_golden.npz and
the numpy restatement tests/_join_ref.py, which tests/test_join_golden.py holds against that file and against Arrow's hash join.  Everything
is bit-exact, and every call writes into buffers pre-filled with 0x5A that are longer than the result: rows, bytes and validity bits beyond
the result must stay as they were, value slots under a null index must be zero.  No pyarrow."""
import ctypes as C
import os

import numpy as np
import pytest

import _join_ref as R

pytestmark = pytest.mark.gpu

MAN, GET = R.load_golden()
JOIN_TILE = 2048  # kJoinTile (pandasarrow_amd/csrc/join.hip): the output rows of one workgroup of the expand kernel
SCAN_TILE = 2048  # kScanTile (pandasarrow_amd/csrc/scan.hpp)
LDS_MAX = 2048    # kLkLdsMaxEntries (pandasarrow_amd/csrc/lookup_table.hpp)
PATTERN = 0x5A
SLACK = 70        # rows of guard band behind the result


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column as K

    lib = L.load()
    L.check(lib.pdx_init(0))
    dts = {"i64": L.INT64, "u64": L.UINT64, "ts": L.TIMESTAMP_NS, "i32": L.INT32, "f64": L.FLOAT64, "f32": L.FLOAT32, "bool": L.BOOL}
    return type("Env", (), {"torch": torch, "L": L, "K": K, "lib": lib, "dts": dts})


def column(env, a, valid, dt, offset=0, exact_null_count=False):
    col = env.K.Column.from_numpy(np.asarray(a, R.NP_KEY[dt]), valid, dtype=env.dts[dt], offset=offset)
    if exact_null_count and valid is not None:
        col.null_count = int((~np.asarray(valid, bool)).sum())
    return col


def guarded(env, rows, with_validity=True):
    """an INT64 output of rows + SLACK rows, values and validity filled with 0x5A"""
    out = env.K.Column.empty(env.L.INT64, rows + SLACK, with_validity=with_validity)
    out.values.view(env.torch.uint8).fill_(PATTERN)
    if with_validity:
        out.validity.fill_(PATTERN)
    return out


def check_output(env, out, rows, want_idx, want_ok, what):
    vals = out.values.cpu().numpy()
    bits = np.unpackbits(out.validity.cpu().numpy(), bitorder="little")
    assert out.length == rows, what
    assert np.array_equal(vals[:rows], want_idx), (what, "indices (zero under a null)")
    assert (vals[rows:].view(np.uint8) == PATTERN).all(), (what, "rows beyond the result were written")
    assert np.array_equal(bits[:rows].astype(bool), want_ok), (what, "validity")
    untouched = np.unpackbits(np.full(len(out.validity), PATTERN, np.uint8), bitorder="little")
    assert np.array_equal(bits[rows:], untouched[rows:]), (what, "validity bits beyond the result were written")
    assert out.null_count == int((~want_ok).sum()), (what, "null_count")


def expected_plan(rk, rv, rows, lds_max=LDS_MAX):
    rv = np.ones(len(rk), bool) if rv is None else np.asarray(rv, bool)
    groups = len(np.unique(np.asarray(rk)[rv])) + (1 if (~rv).any() else 0)
    plan = "empty" if len(rk) == 0 else "lds" if groups <= lds_max else "global"
    return {"plan": plan, "build_rows": str(len(rk)), "distinct": str(groups), "out_rows": str(rows)}


def check_join(env, lk, lv, rk, rv, dt, hows=R.HOWS, offset=0, want=None, lds_max=LDS_MAX, exact_null_count=False, what=""):
    """every join kind of one pair of key columns against the restatement (or want[how] from the golden file): row count, plan, both index
    columns with their validity and null counts, the guard band"""
    cl, cr = column(env, lk, lv, dt, offset, exact_null_count), column(env, rk, rv, dt, offset, exact_null_count)
    for how in hows:
        li, lok, ri, rok = want[how] if want is not None else R.join_ref(lk, lv, rk, rv, how)
        tag = (what, how, dt, offset)
        h = env.K.JoinHandle(cl, cr, how)
        try:
            assert h.rows == len(li), tag
            assert h.plan() == expected_plan(rk, rv, len(li), lds_max), (tag, h.plan())
            ol = guarded(env, h.rows)
            orr = guarded(env, h.rows) if ri is not None else None
            h.indices(ol, orr)
            check_output(env, ol, len(li), li, lok, tag + ("left",))
            if ri is not None:
                check_output(env, orr, len(li), ri, rok, tag + ("right",))
        finally:
            h.close()


def golden_want(name):
    want = {}
    for how in R.HOWS:
        li, lok = GET(f"{name}/{how}/li"), GET(f"{name}/{how}/lok").astype(bool)
        if how in ("semi", "anti"):
            want[how] = (li, lok, None, None)
        else:
            want[how] = (li, lok, GET(f"{name}/{how}/ri"), GET(f"{name}/{how}/rok").astype(bool))
    return want


# ---------------------------------------------------------------- the golden file through the C ABI
# (degenerate shapes, the extreme key values of every dtype, nulls on both sides, the OUTER tail: tools/gen_golden_join.py)
@pytest.mark.parametrize("dt", ["i64", "u64", "ts", "i32"])
def test_golden_through_the_abi(env, dt):
    for c in (c for c in MAN["cases"] if c["dtype"] == dt):
        lk, lv, rk, rv = R.golden_inputs(c, GET)
        for offset in (0, 3):
            check_join(env, lk, lv, rk, rv, dt, offset=offset, want=golden_want(c["name"]), what=c["name"])


def test_null_count_given_and_columns_without_validity(env):
    c = next(c for c in MAN["cases"] if c["name"].startswith("random_02"))  # (nulls on both sides)
    lk, lv, rk, rv = R.golden_inputs(c, GET)
    assert (~lv).any() and (~rv).any()
    check_join(env, lk, lv, rk, rv, c["dtype"], offset=13, exact_null_count=True, want=golden_want(c["name"]), what="exact null_count")
    check_join(env, lk, None, rk, None, c["dtype"], what="no validity")


# ---------------------------------------------------------------- plan edge: the table in LDS / in global memory
def test_plan_edge_at_the_lds_bound(env):
    for distinct in (LDS_MAX, LDS_MAX + 1):
        rng = np.random.default_rng(distinct)
        keys = rng.permutation(np.arange(distinct, dtype=np.int64) * 7919 - 5_000_000)
        rk = np.concatenate([keys, keys[:300]])  # 300 keys twice
        lk = np.concatenate([keys[rng.integers(0, distinct, 2500)], np.arange(200, dtype=np.int64) * 7919 + 1])  # (the last 200 miss)
        lv = rng.random(len(lk)) > 0.1
        check_join(env, lk, lv, rk, None, "i64", what=f"distinct={distinct}")
        cl, cr = column(env, lk, lv, "i64"), column(env, rk, None, "i64")
        h = env.K.JoinHandle(cl, cr, "inner")
        assert h.plan()["plan"] == ("lds" if distinct <= LDS_MAX else "global"), distinct
        h.close()


def test_the_override_forces_the_global_plan_at_a_small_table(env):
    rk = np.array([10, 20, 30, 40, 50, 30], np.int64)  # five distinct keys
    lk = np.array([30, 5, 50, 10, 30, 60, 20], np.int64)
    old = os.environ.get("PDX_LOOKUP_LDS_MAX")
    os.environ["PDX_LOOKUP_LDS_MAX"] = "4"
    try:
        check_join(env, lk, None, rk, None, "i64", lds_max=4, what="override")
        for dt in ("i32", "u64"):
            check_join(env, lk, None, rk, None, dt, lds_max=4, what="override")
        check_join(env, lk, None, rk[:4], None, "i64", lds_max=4, what="override, four keys")  # (four keys still fit)
    finally:
        if old is None:
            del os.environ["PDX_LOOKUP_LDS_MAX"]
        else:
            os.environ["PDX_LOOKUP_LDS_MAX"] = old


# ---------------------------------------------------------------- expand: tile edges
def test_output_of_one_tile_minus_one_to_plus_one(env):
    for total in (JOIN_TILE - 1, JOIN_TILE, JOIN_TILE + 1):
        rk = np.arange(50, dtype=np.int64)
        lk = np.arange(total, dtype=np.int64) % 50
        check_join(env, lk, None, rk, None, "i64", what=f"total={total}")
        # the same totals from matches of several right rows: 3 per left row, the remainder from a key with one
        rk3 = np.concatenate([np.repeat(np.arange(50, dtype=np.int64), 3), [99]])
        lk3 = np.concatenate([np.arange(total // 3, dtype=np.int64) % 50, np.full(total % 3, 99)])
        check_join(env, lk3, None, rk3, None, "i64", hows=("inner", "left", "outer"), what=f"total={total} by threes")


def test_one_hot_key_is_spread_over_tiles(env):
    hot = 3 * JOIN_TILE + 1
    rng = np.random.default_rng(11)
    rk = np.concatenate([np.arange(100, dtype=np.int64), np.full(hot, 1000)])
    rk = rk[rng.permutation(len(rk))]
    lk = np.concatenate([np.arange(700, dtype=np.int64) % 130, [1000], np.arange(900, dtype=np.int64) % 130])  # (keys 100 .. 129 miss)
    check_join(env, lk, None, rk, None, "i64", what="hot key")


def test_a_run_of_rows_without_output_at_a_tile_boundary(env):
    rk = np.arange(64, dtype=np.int64)
    run = JOIN_TILE + 5  # more left rows than the window a workgroup stages
    lk = np.concatenate([np.arange(JOIN_TILE, dtype=np.int64) % 64, np.full(run, -1), np.arange(100, dtype=np.int64) % 64])
    check_join(env, lk, None, rk, None, "i64", what="zero run at the boundary")
    lk2 = np.concatenate([np.arange(JOIN_TILE - 3, dtype=np.int64) % 64, np.full(run, -1), np.arange(100, dtype=np.int64) % 64])
    check_join(env, lk2, None, rk, None, "i64", hows=("inner",), what="zero run across the boundary")
    lk3 = np.concatenate([np.full(run, -1), np.arange(10, dtype=np.int64)])
    check_join(env, lk3, None, rk, None, "i64", hows=("inner", "semi"), what="zero run first")


def test_left_join_null_key_rows_at_the_ends_of_a_tile(env):
    n = 2 * JOIN_TILE + 9
    lk = np.arange(n, dtype=np.int64) % 40
    lv = np.ones(n, bool)
    lv[[0, JOIN_TILE - 1, JOIN_TILE, 2 * JOIN_TILE - 1, 2 * JOIN_TILE, n - 1]] = False  # one output row per left row: these are tile edges
    check_join(env, lk, lv, np.arange(40, dtype=np.int64), None, "i64", hows=("left", "outer", "anti"), what="null rows at tile edges")


# ---------------------------------------------------------------- scan edges: left rows around the scan's tile
def test_left_rows_around_the_scan_tile(env):
    for nl in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 1):
        rng = np.random.default_rng(nl)
        rk = np.array([4, 7, 7, 9, 4, 4, 11], np.int64)
        rv = np.array([1, 1, 1, 1, 1, 0, 1], bool)
        lk = rng.integers(0, 13, nl)
        lv = rng.random(nl) > 0.15
        check_join(env, lk, lv, rk, rv, "i64", what=f"nl={nl}")


# ---------------------------------------------------------------- many to many
def test_many_to_many_300_by_300(env):
    rng = np.random.default_rng(5)
    lk = np.concatenate([np.full(300, 77), rng.integers(0, 60, 200)])
    rk = np.concatenate([np.full(300, 77), rng.integers(30, 90, 200)])
    lk, rk = lk[rng.permutation(len(lk))], rk[rng.permutation(len(rk))]
    lv, rv = rng.random(len(lk)) > 0.05, rng.random(len(rk)) > 0.05
    for dt in ("i64", "i32"):
        check_join(env, lk, lv, rk, rv, dt, offset=5, what="300 x 300")
    li = R.join_ref(lk, lv, rk, rv, "inner")[0]
    assert len(li) >= int(((lk == 77) & lv).sum()) * int(((rk == 77) & rv).sum()) > 70_000


# ---------------------------------------------------------------- the OUTER tail
def test_outer_tail_order(env):
    rng = np.random.default_rng(9)
    nr = 5000  # more than one compaction tile of right rows
    rk = rng.integers(0, 400, nr)
    rv = rng.random(nr) > 0.1
    rk[rv & (rk == 399)] = 398
    rk[~rv & (rng.random(nr) > 0.5)] = 399  # a key that only null-key rows carry
    lk = np.concatenate([rng.integers(0, 800, 3000) * 2, [397]])  # odd keys stay unmatched; 397 is matched by the last left row only
    assert 397 not in lk[:-1]
    check_join(env, lk, None, rk, rv, "i64", hows=("outer",), what="outer tail")


# ---------------------------------------------------------------- determinism
def test_same_bytes_twice_and_on_a_second_stream(env):
    rng = np.random.default_rng(21)
    lk, rk = rng.integers(0, 3000, 9000), rng.integers(0, 3000, 7000)  # (the global plan: the table is built with atomics)
    lv, rv = rng.random(9000) > 0.1, rng.random(7000) > 0.1
    cl, cr = column(env, lk, lv, "i64"), column(env, rk, rv, "i64")
    env.torch.cuda.synchronize()

    def run():
        outs = []
        for how in R.HOWS:
            a, b = env.K.join_indices(cl, cr, how)
            for c in (a, b):
                if c is not None:
                    outs.append(c.values[:c.length].cpu().numpy().tobytes())
                    if c.validity is not None:
                        outs.append(np.unpackbits(c.validity.cpu().numpy(), bitorder="little")[:c.length].tobytes())
        return outs

    first = run()
    assert run() == first
    with env.torch.cuda.stream(env.torch.cuda.Stream()):
        assert run() == first
    env.torch.cuda.synchronize()


# ---------------------------------------------------------------- refusals, each before anything is launched
def create_status(env, cl, cr, how):
    h = C.c_void_p()
    a, b = cl.c(), cr.c()
    st = env.lib.pdx_join_create(C.byref(a), C.byref(b), how, None, C.byref(h))
    if st == env.L.OK:
        env.lib.pdx_join_destroy(h)
    return st, env.lib.pdx_last_error().decode()


def test_unsupported_key_dtypes_are_named(env):
    for np_dt, name in ((np.float64, "float64"), (np.float32, "float32"), (bool, "bool")):
        col = env.K.Column.from_numpy(np.array([1, 0, 1], np_dt))
        st, msg = create_status(env, col, col, env.L.JOIN_INNER)
        assert st == env.L.NOT_IMPLEMENTED and name in msg, (name, msg)


def test_key_dtype_mismatch_and_bad_how_are_invalid(env):
    a, b = column(env, [1, 2], None, "i64"), column(env, [1, 2], None, "i32")
    st, msg = create_status(env, a, b, env.L.JOIN_INNER)
    assert st == env.L.INVALID and "int64" in msg and "int32" in msg, msg
    st, msg = create_status(env, a, column(env, [1, 2], None, "ts"), env.L.JOIN_LEFT)
    assert st == env.L.INVALID, msg
    assert create_status(env, a, a, 5)[0] == env.L.INVALID and create_status(env, a, a, -1)[0] == env.L.INVALID


def test_output_refusals_leave_the_buffers_untouched(env):
    lk, rk = np.array([1, 2, 3, 4, 2], np.int64), np.array([2, 2, 5], np.int64)
    cl, cr = column(env, lk, None, "i64"), column(env, rk, None, "i64")

    def status(how, ol, orr):
        h = env.K.JoinHandle(cl, cr, how)
        ml, mr = ol.mut(), (orr.mut() if orr is not None else None)
        st = env.lib.pdx_join_indices(h._h, C.byref(ml), None if mr is None else C.byref(mr), None)
        h.close()
        for o in (ol, orr):
            if o is not None:
                assert (o.values.view(env.torch.uint8).cpu().numpy() == PATTERN).all(), "a refused call wrote values"
                assert o.validity is None or (o.validity.cpu().numpy() == PATTERN).all(), "a refused call wrote validity"
        return st

    rows = {how: len(R.join_ref(lk, None, rk, None, how)[0]) for how in R.HOWS}
    # missing validity where the join kind requires it
    assert status("left", guarded(env, rows["left"]), guarded(env, rows["left"], with_validity=False)) == env.L.INVALID
    assert status("outer", guarded(env, rows["outer"], with_validity=False), guarded(env, rows["outer"])) == env.L.INVALID
    assert status("outer", guarded(env, rows["outer"]), guarded(env, rows["outer"], with_validity=False)) == env.L.INVALID
    # a capacity one short, on either side
    for how in ("inner", "left", "outer"):
        short = guarded(env, rows[how] - 1 - SLACK)
        assert short.length == rows[how] - 1
        assert status(how, short, guarded(env, rows[how])) == env.L.INVALID, how
        assert status(how, guarded(env, rows[how]), guarded(env, rows[how] - 1 - SLACK)) == env.L.INVALID, how
    assert status("semi", guarded(env, rows["semi"] - 1 - SLACK), None) == env.L.INVALID
    # the wrong dtype, a missing right output
    wrong = env.K.Column.empty(env.L.UINT64, rows["inner"] + SLACK, with_validity=True)
    wrong.values.view(env.torch.uint8).fill_(PATTERN)
    wrong.validity.fill_(PATTERN)
    assert status("inner", wrong, guarded(env, rows["inner"])) == env.L.INVALID
    assert status("inner", guarded(env, rows["inner"]), None) == env.L.INVALID
    # SEMI / ANTI have no right output: a non-NULL out_right is refused (include/pdx/abi.h)
    assert status("semi", guarded(env, rows["semi"]), guarded(env, rows["semi"])) == env.L.INVALID
    assert status("anti", guarded(env, rows["anti"]), guarded(env, rows["anti"])) == env.L.INVALID


def test_inner_accepts_outputs_without_validity_and_indices_can_be_asked_twice(env):
    lk, rk = np.array([1, 2, 3, 4, 2], np.int64), np.array([2, 2, 5], np.int64)
    h = env.K.JoinHandle(column(env, lk, None, "i64"), column(env, rk, None, "i64"), "inner")
    li, _, ri, _ = R.join_ref(lk, None, rk, None, "inner")
    for _ in range(2):
        ol, orr = guarded(env, h.rows, with_validity=False), guarded(env, h.rows, with_validity=False)
        h.indices(ol, orr)
        assert np.array_equal(ol.values.cpu().numpy()[:h.rows], li) and np.array_equal(orr.values.cpu().numpy()[:h.rows], ri)
        assert ol.null_count == 0 and orr.null_count == 0
    h.close()


def test_take_by_the_join_indices_gives_the_joined_rows(env):
    rng = np.random.default_rng(2)
    lk, rk = rng.integers(0, 20, 50), rng.integers(10, 30, 40)
    lval, rval = rng.random(50), rng.integers(0, 1000, 40)
    li, lok, ri, rok = R.join_ref(lk, None, rk, None, "outer")
    gl, gr = env.K.join_indices(column(env, lk, None, "i64"), column(env, rk, None, "i64"), "outer")
    (tl,) = env.K.take([env.K.Column.from_numpy(lval)], gl)
    (tr,) = env.K.take([env.K.Column.from_numpy(rval)], gr)
    v, ok = tl.to_numpy()
    assert np.array_equal(ok, lok) and np.array_equal(v[lok], lval[li[lok]])
    v, ok = tr.to_numpy()
    assert np.array_equal(ok, rok) and np.array_equal(v[rok], rval[ri[rok]])
