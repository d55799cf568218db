"""GPU: DataFrame.merge / DataFrame.join of the Python facade (pandasarrow_amd/api.py -> pdx_join_create, pdx_join_indices, pdx_take) against
the numpy restatement tests/_join_ref.py applied to whole frames: every `how` ("right" included), suffixes on clashing names, the single
key column under `on` and its coalesce for "outer", mixed 8-byte and 4-byte value columns, null cells carried through, join on int64 and
timestamp indexes, and the unique-key inner merge against the index_in + take chain.  Everything is bit-exact."""
import numpy as np
import pytest

import _join_ref as R

pytestmark = pytest.mark.gpu

HOWS = ("inner", "left", "right", "outer", "semi", "anti")


@pytest.fixture(scope="module")
def env():
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column as K

    L.check(L.load().pdx_init(0))
    return type("Env", (), {"L": L, "K": K, "api": api})


def plan(lk, lv, rk, rv, how):
    """-> (left idx, left ok, right idx | None, right ok | None) of `how`, "right" as a left join with the sides swapped"""
    if how == "right":
        ri, rok, li, lok = R.join_ref(rk, rv, lk, lv, "left")
        return li, lok, ri, rok
    return R.join_ref(lk, lv, rk, rv, how)


def taken(values, valid, idx, ok):
    """(values, valid) of a host column taken by nullable indices"""
    values = np.asarray(values)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    if len(values) == 0:
        return np.zeros(len(idx), values.dtype), np.zeros(len(idx), bool)
    return values[idx], ok & valid[idx]


def assert_column(series, want_values, want_valid, what):
    v, ok = series.to_numpy()
    ok = np.ones(len(v), bool) if ok is None else ok
    assert len(v) == len(want_values), what
    assert np.array_equal(ok, want_valid), (what, "validity")
    assert np.array_equal(np.asarray(v)[ok].view(np.uint8), np.asarray(want_values, np.asarray(v).dtype)[ok].view(np.uint8)), (what, "values")


@pytest.fixture(scope="module")
def frames(env):
    rng = np.random.default_rng(31)
    nl, nr = 700, 500
    host = {
        "lk": rng.integers(0, 60, nl), "lkv": rng.random(nl) > 0.1,
        "rk": rng.integers(20, 90, nr), "rkv": rng.random(nr) > 0.1,
        "a": rng.random(nl), "av": rng.random(nl) > 0.2,                       # float64 with null cells
        "c": rng.integers(-2**31, 2**31, nl).astype(np.int32),                  # int32
        "v_l": rng.integers(0, 10**12, nl),                                     # clashes with the right's v
        "b": rng.random(nr).astype(np.float32), "bv": rng.random(nr) > 0.2,    # float32 with null cells
        "v_r": rng.integers(-10**12, 0, nr),
    }
    S, Lb = env.api.Series, env.L
    left = env.api.DataFrame({"k": S(host["lk"], host["lkv"]), "a": S(host["a"], host["av"]), "c": S(host["c"], dtype=Lb.INT32), "v": S(host["v_l"])})
    right = env.api.DataFrame({"k": S(host["rk"], host["rkv"]), "b": S(host["b"], host["bv"], dtype=Lb.FLOAT32), "v": S(host["v_r"])})
    return host, left, right


def test_merge_on_one_key(env, frames):
    for how in HOWS:
        h, left, right = frames
        li, lok, ri, rok = plan(h["lk"], h["lkv"], h["rk"], h["rkv"], how)
        m = left.merge(right, on="k", how=how)
        assert m.index is None and m.num_rows() == len(li), how
        if how in ("semi", "anti"):
            assert m.names == ["k", "a", "c", "v"], how
            assert_column(m["k"], *taken(h["lk"], h["lkv"], li, lok), (how, "k"))
            assert_column(m["a"], *taken(h["a"], h["av"], li, lok), (how, "a"))
            assert_column(m["v"], *taken(h["v_l"], None, li, lok), (how, "v"))
            continue
        assert m.names == ["k", "a", "c", "v_x", "b", "v_y"], how  # the key once; the clashing name takes the suffixes
        assert m["c"].dtype() == env.L.INT32 and m["b"].dtype() == env.L.FLOAT32 and m["a"].dtype() == env.L.FLOAT64
        lkey, lkey_ok = taken(h["lk"], h["lkv"], li, lok)
        rkey, rkey_ok = taken(h["rk"], h["rkv"], ri, rok)
        if how == "right":
            assert_column(m["k"], rkey, rkey_ok, (how, "k"))
        elif how == "outer":  # coalesce(left key, right key)
            assert_column(m["k"], np.where(lkey_ok, lkey, rkey), lkey_ok | rkey_ok, (how, "k"))
            assert (rkey_ok & ~lok).any() and (~lkey_ok & ~rkey_ok).any(), "the case holds an unmatched right key and null keys"
        else:
            assert_column(m["k"], lkey, lkey_ok, (how, "k"))
        assert_column(m["a"], *taken(h["a"], h["av"], li, lok), (how, "a"))
        assert_column(m["c"], *taken(h["c"], None, li, lok), (how, "c"))
        assert_column(m["v_x"], *taken(h["v_l"], None, li, lok), (how, "v_x"))
        assert_column(m["b"], *taken(h["b"], h["bv"], ri, rok), (how, "b"))
        assert_column(m["v_y"], *taken(h["v_r"], None, ri, rok), (how, "v_y"))


def test_merge_left_on_right_on_and_suffixes(env, frames):
    h, left, right = frames
    r2 = env.api.DataFrame({"rk": right["k"], "b": right["b"], "v": right["v"], "a": right["v"]})
    m = left.merge(r2, left_on="k", right_on="rk", how="inner", suffixes=("_left", "_right"))
    assert m.names == ["k", "a_left", "c", "v_left", "rk", "b", "v_right", "a_right"]  # two key names: both stay
    li, lok, ri, rok = R.join_ref(h["lk"], h["lkv"], h["rk"], h["rkv"], "inner")
    assert_column(m["k"], *taken(h["lk"], h["lkv"], li, lok), "k")
    assert_column(m["rk"], *taken(h["rk"], h["rkv"], ri, rok), "rk")
    assert_column(m["a_right"], *taken(h["v_r"], None, ri, rok), "a_right")
    same = left.merge(right, left_on="k", right_on="k", how="inner")  # equal names behave as `on`
    assert same.names == ["k", "a", "c", "v_x", "b", "v_y"]
    with pytest.raises(env.L.PdxError):
        left.merge(right, on="k", left_on="k")
    with pytest.raises(env.L.PdxError):
        left.merge(right)
    with pytest.raises(env.L.PdxError):
        left.merge(right, on="k", how="cross")
    with pytest.raises(env.L.PdxError):
        left.merge(right, on="nope")
    with pytest.raises(env.L.PdxError) as e:
        left.merge(right, left_on="a", right_on="k")  # a float64 key
    assert e.value.status == env.L.NOT_IMPLEMENTED and "float64" in str(e.value)
    clash = env.api.DataFrame({"k": right["k"], "v": right["v"], "v_y": right["v"]})
    with pytest.raises(env.L.PdxError):
        clash.merge(right, on="k", suffixes=("", "_y"))  # "v_y" twice


def test_inner_merge_on_a_unique_right_key_equals_the_index_in_take_chain(env):
    rng = np.random.default_rng(8)
    rk = rng.permutation(5000)[:3000]  # unique
    rval = rng.random(3000)
    lk = rng.integers(0, 5000, 20_000)
    lv = rng.random(20_000) > 0.05
    lval = rng.integers(0, 1000, 20_000)
    S = env.api.Series
    left, right = env.api.DataFrame({"k": S(lk, lv), "x": S(lval)}), env.api.DataFrame({"k": S(rk), "y": S(rval)})
    m = left.merge(right, on="k", how="inner")
    # the chain: index_in finds each left key's (only) position in the right key, take gathers the right rows (a null position gives a
    # null row), and the rows without a match drop out
    pos = left["k"].index_in(right["k"], skip_nulls=True)
    y = env.K.take([right["y"].col], env.K.cast(pos.col, env.L.INT64))[0]
    chain = env.K.drop_na([left["k"].col, left["x"].col, y])
    assert m.num_rows() == chain[0].length > 10_000
    for name, want in zip(("k", "x", "y"), chain):
        got = m[name].to_numpy()
        assert np.array_equal(got[0].view(np.uint8), want.to_numpy()[0].view(np.uint8)), name
        assert got[1] is None or got[1].all(), name


@pytest.mark.parametrize("labels", ["int64", "timestamp"])
def test_join_on_the_index(env, labels):
    rng = np.random.default_rng(4)
    lix = rng.permutation(400)[:250].astype(np.int64) * 1000  # unique labels on each side, about half shared
    rix = rng.permutation(400)[:220].astype(np.int64) * 1000
    if labels == "timestamp":
        lix, rix = (lix + 1_700_000_000_000_000_000).astype("datetime64[ns]"), (rix + 1_700_000_000_000_000_000).astype("datetime64[ns]")
    a, b = rng.random(250), rng.integers(0, 99, 220)
    bv = rng.random(220) > 0.3
    S = env.api.Series
    left = env.api.DataFrame({"a": S(a)}, index=lix)
    right = env.api.DataFrame({"b": S(b, bv)}, index=rix)
    for how in HOWS:
        j = left.join(right, how=how)
        lk, rk = lix.astype(np.int64), rix.astype(np.int64)
        li, lok, ri, rok = plan(lk, None, rk, None, how)
        assert j.index.dtype == (env.L.TIMESTAMP_NS if labels == "timestamp" else env.L.INT64), how
        ix, ixok = j.index.to_numpy()
        assert ixok is None or ixok.all(), (how, "every result row has a label")
        if ri is None:
            assert j.names == ["a"] and np.array_equal(ix, lk[li]), how
        else:
            assert j.names == ["a", "b"]
            assert np.array_equal(ix, np.where(lok, lk[li], rk[ri])), (how, "coalesce(left labels, right labels)")
            assert_column(j["b"], *taken(b, bv, ri, rok), (how, "b"))
        assert_column(j["a"], *taken(a, None, li, lok), (how, "a"))


def test_join_without_an_index_and_refusals(env):
    S = env.api.Series
    p, q = env.api.DataFrame({"a": S(np.array([1, 2, 3]))}), env.api.DataFrame({"b": S(np.array([4, 5]))})
    j = p.join(q)  # the row numbers are the labels
    assert_column(j["b"], np.array([4, 5, 0]), np.array([1, 1, 0], bool), "b")
    assert np.array_equal(j.index.to_numpy()[0], [0, 1, 2])
    with pytest.raises(env.L.PdxError):
        p.join(p)  # the names overlap
    with pytest.raises(env.L.PdxError):
        p.join(q, how="cross")
