"""GPU parity tests (run with `-m gpu` on an MI355X).  Every check goes HIP kernels -> C ABI (libpdx_hip.so) -> ctypes,
and is compared bit-for-bit with the CPU oracle and with the committed golden vectors (Arrow 25.0.0 outputs and the
reference's own known-answer tests).  Tolerances: none -- integer, index and fp64 results must be bit-identical."""
import os

import numpy as np
import pytest

import oracle as orc
from _create_plans import pinned_plan, pinned_slots
from conftest import assert_f64_bits, golden

pytestmark = pytest.mark.gpu

G = golden()


@pytest.fixture(scope="module")
def px():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column

    L.check(L.load().pdx_init(0))

    class NS:
        pass

    ns = NS()
    ns.L, ns.K, ns.api, ns.Column, ns.torch = L, column, api, column.Column, torch
    return ns


def _valid_or_none(v):
    return None if v is None or np.all(v) else v


# ------------------------------------------------------------------ synthetic generators
def test_synth_matches_oracle(px):
    n = 100_003
    assert np.array_equal(px.K.synth_keys(5, n, 1000).to_numpy()[0], orc.synth_keys(5, n, 1000))
    assert_f64_bits(px.K.synth_vals(7, n, 3).to_numpy()[0], orc.synth_vals(7, n, 3))
    assert np.array_equal(px.K.synth_ts(2, n, 946684800 * 10**9, 10**8).to_numpy()[0], orc.synth_ts(2, n, 946684800 * 10**9, 10**8))


# ------------------------------------------------------------------ element-wise
OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3}
CMPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5}


@pytest.mark.parametrize("name", [c for c in G.cases("elementwise") if c.startswith("ew_")])
@pytest.mark.parametrize("offset", [0, 5])
def test_elementwise_golden(px, name, offset):
    c = G.case(name)
    scalar = c["b"].ndim == 0
    va, vb = _valid_or_none(c["va"]), (None if scalar else _valid_or_none(c["vb"]))
    A = px.Column.from_numpy(c["a"], va, offset=offset)
    B = c["b"].item() if scalar else px.Column.from_numpy(c["b"], vb, offset=offset)
    for k, op in OPS.items():
        out = px.K.binary(op, A, B)
        vals, valid = out.to_numpy()
        ev = c[f"{k}_valid"]
        if valid is not None:
            assert np.array_equal(valid, ev), f"{name} {k} validity"
        else:
            assert ev.all()
        if vals.dtype == np.float64:
            assert_f64_bits(vals, c[k], valid=ev, what=f"{name} {k}", nan_bits=True)  # x86 NaN operand rule: sign and payload too
        else:
            assert np.array_equal(vals[ev], c[k][ev]), f"{name} {k}"
    for k, op in CMPS.items():
        vals, valid = px.K.compare(op, A, B).to_numpy()
        ev = c[f"{k}_valid"]
        assert np.array_equal(vals[ev], c[k][ev]), f"{name} {k}"
        if valid is not None:
            assert np.array_equal(valid, ev)


@pytest.mark.parametrize("name", [c for c in G.cases("elementwise") if c.startswith("logic_")])
def test_logical_golden(px, name):
    c = G.case(name)
    A = px.Column.from_numpy(c["a"], c["va"], offset=3)
    B = px.Column.from_numpy(c["b"], c["vb"], offset=11)
    for k, op in (("and_", 0), ("or_", 1)):
        vals, valid = px.K.logical(op, A, B).to_numpy()
        ev = c[f"{k}valid"]
        assert np.array_equal(valid, ev)
        assert np.array_equal(vals[ev], c[k][ev])
    vals, valid = px.K.invert(A).to_numpy()
    assert np.array_equal(valid, c["inv_valid"])
    assert np.array_equal(vals[c["inv_valid"]], c["inv"][c["inv_valid"]])


def test_elementwise_errors_and_kat(px, kat):
    S = px.api.Series
    with pytest.raises(RuntimeError, match="divide by zero"):
        S(np.array([7, 1])) / S(np.array([2, 0]))
    r = S(np.array([7, 1])) / S(np.array([2, 0]), valid=np.array([True, False]))  # the zero hides under a null
    vals, valid = r.to_numpy()
    assert vals[0] == 3 and list(valid) == [True, False]
    # different lengths = different (range) indexes: Series::broadcast aligns on the union of the labels (src/series.cpp:212-227)
    r = S(np.arange(5)) + S(np.arange(3))
    vals, valid = r.to_numpy()
    assert list(valid) == [True, True, True, False, False] and list(vals[:3]) == [0, 2, 4]
    for k in kat["binary"]:
        if k["dtype"] == "int64":
            a = S(np.array(k["a"], np.int64))
            b = k["b_scalar"] if "b_scalar" in k else S(np.array(k["b"], np.int64))
            for name, res in (("add", a + b), ("sub", a - b), ("mul", a * b), ("div", a / b)):
                assert res.dtype() == px.L.INT64 and res.name == "" and list(res.values()) == k[name], (k["src"], name)
        else:
            res = S(np.array(k["a"])) - S(np.array(k["b"], np.int64))
            assert res.dtype() == px.L.FLOAT64 and np.allclose(res.values(), k["sub_approx"])
    assert list((-S(np.array([1, 2, 3]))).values()) == [-1, -2, -3]


def test_elementwise_large_vs_oracle(px):
    n = 3_000_017
    a, b = orc.synth_vals(0, n, 1), orc.synth_vals(0, n, 2) - 0.5
    A, B = px.K.synth_vals(0, n, 1), px.Column.from_numpy(b)
    for op in OPS.values():
        assert_f64_bits(px.K.binary(op, A, B).to_numpy()[0], orc.binary(op, a, b)[0], what=f"op{op}", nan_bits=True)
    for op in CMPS.values():
        assert np.array_equal(px.K.compare(op, A, B).to_numpy()[0], orc.compare(op, a, b)[0])
    m1, m2 = px.K.compare(4, A, 0.5), px.K.compare(2, B, 0.0)
    assert np.array_equal(px.K.logical(0, m1, m2).to_numpy()[0], (a > 0.5) & (b < 0.0))
    # slices at an odd element offset are not 16-byte aligned: the row-per-lane loops (main part and tail), on one or both sides
    ia = (np.arange(n, dtype=np.int64) * 7919) % 200_003 - 100_000
    ib = (np.arange(n, dtype=np.int64) * 104_729) % 999 + 1
    for x, y in ((a, b), (ia, ib), (ia, b)):
        for ox, oy in ((3, 0), (0, 1), (1, 5)):
            X, Y = px.Column.from_numpy(x, offset=ox), px.Column.from_numpy(y, offset=oy)
            for op in OPS.values():
                got = px.K.binary(op, X, Y).to_numpy()[0]
                exp = orc.binary(op, x, y)[0]
                if got.dtype == np.float64:
                    assert_f64_bits(got, exp, what=f"op{op} offsets {ox},{oy}", nan_bits=True)
                else:
                    assert np.array_equal(got, exp), (op, ox, oy)
            for op in CMPS.values():
                assert np.array_equal(px.K.compare(op, X, Y).to_numpy()[0], orc.compare(op, x, y)[0]), (op, ox, oy)


# ------------------------------------------------------------------ whole-array aggregates
AGG = {"sum": 0, "mean": 1, "min": 2, "max": 3}


@pytest.mark.parametrize("name", [c for c in G.cases("aggregate") if c.startswith("agg_f64") and "synth" not in c])
@pytest.mark.parametrize("offset", [0, 3])
def test_aggregate_f64_golden(px, name, offset):
    c = G.case(name)
    col = px.Column.from_numpy(c["v"], _valid_or_none(c["valid"]), offset=offset)
    for j, kind in enumerate(AGG.values()):
        val, cnt = px.K.aggregate(kind, col)
        assert cnt == int(c["count"])
        if c["isnull"][j]:
            assert val is None
        else:
            assert_f64_bits([val], [c["exp"][j]], what=f"{name} kind={kind}")
    assert px.K.aggregate(4, col)[0] == int(c["count"])


@pytest.mark.parametrize("name", [c for c in G.cases("aggregate") if c.startswith("agg_i64")])
def test_aggregate_i64_golden(px, name):
    c = G.case(name)
    col = px.Column.from_numpy(c["v"], _valid_or_none(c["valid"]), offset=2)
    s, cnt = px.K.aggregate(0, col)
    m, _ = px.K.aggregate(1, col)
    lo, _ = px.K.aggregate(2, col)
    hi, _ = px.K.aggregate(3, col)
    assert cnt == int(c["count"])
    if c["isnull"][0]:
        assert s is None and m is None and lo is None and hi is None
    else:
        assert (s, lo, hi) == tuple(int(x) for x in c["exp_i"])
        assert_f64_bits([m], [c["exp_mean"]])


@pytest.mark.parametrize("name", [c for c in G.cases("aggregate") if "synth" in c])
def test_aggregate_synth_golden(px, name):
    c = G.case(name)
    col = px.K.synth_vals(0, int(c["n"]), int(c["seed_off"]))
    got = [px.K.aggregate(k, col)[0] for k in AGG.values()]
    assert_f64_bits(got, c["exp"], what=name)


@pytest.mark.parametrize("n", [4096, 4097, 65536 + 17, 256 * 4096, 256 * 4096 + 4095, 20_000_003])
def test_aggregate_sum_sizes_vs_oracle(px, n):
    v = orc.synth_vals(0, n, 5) - 0.25
    col = px.Column.from_numpy(v)
    for kind in AGG.values():
        assert_f64_bits([px.K.aggregate(kind, col)[0]], [orc.agg(kind, v)[0]], what=f"n={n} kind={kind}")
    if n <= 2_000_000:
        valid = (orc.synth_keys(0, n, 10) != 3)
        colv = px.Column.from_numpy(v, valid, offset=7)
        for kind in AGG.values():
            assert_f64_bits([px.K.aggregate(kind, colv)[0]], [orc.agg(kind, v, valid)[0]], what=f"nulls n={n} kind={kind}")
        # long valid runs with isolated nulls + int64 mean
        valid2 = np.ones(n, bool)
        valid2[::1013] = False
        vi = orc.synth_keys(0, n, 1 << 40) - (1 << 39)
        coli = px.Column.from_numpy(vi, valid2)
        for kind in (0, 1, 2, 3, 4):
            assert px.K.aggregate(kind, coli)[0] == orc.agg(kind, vi, valid2)[0]


def test_aggregate_kat(px, kat):
    S = px.api.Series
    for k in kat["aggregate"]:
        s = S(np.array(k["v"], np.int64), valid=np.array(k["valid"], bool))
        if "min" in k:
            assert s.min() == k["min"] and s.max() == k["max"]
        if "mean" in k:
            assert s.mean() == k["mean"]
        if "count" in k:
            assert s.count() == k["count"]


# ------------------------------------------------------------------ filter / take / concat
@pytest.mark.parametrize("name", [c for c in G.cases("filter_take") if c.startswith("filter_")])
def test_filter_golden(px, name):
    c = G.case(name)
    col = px.Column.from_numpy(c["v"], _valid_or_none(c["valid"]), offset=3)
    mask = px.Column.from_numpy(c["mask"], _valid_or_none(c["mvalid"]), offset=9)
    for emit, key in ((True, "emit"), (False, "drop")):
        assert px.K.filter_count(mask, emit) == len(c[key])
        (out,) = px.K.filter([col], mask, emit)
        vals, ok = out.to_numpy()
        ev = c[f"{key}_valid"]
        assert len(vals) == len(c[key])
        if ok is not None:
            assert np.array_equal(ok, ev)
            assert out.null_count == int((~ev).sum())
        else:
            assert ev.all()
        assert_f64_bits(vals, c[key], valid=ev, what=name)


@pytest.mark.parametrize("name", [c for c in G.cases("filter_take") if c.startswith("take_")])
def test_take_golden(px, name):
    c = G.case(name)
    col = px.Column.from_numpy(c["v"], _valid_or_none(c["valid"]), offset=2)
    idx = px.Column.from_numpy(c["idx"], _valid_or_none(c["ivalid"]), offset=1)
    (out,) = px.K.take([col], idx)
    vals, ok = out.to_numpy()
    if ok is not None:
        assert np.array_equal(ok, c["out_valid"])
    assert np.array_equal(vals[c["out_valid"]], c["out"][c["out_valid"]])


def test_filter_take_errors_and_kat(px, kat):
    S, DF = px.api.Series, px.api.DataFrame
    s1 = S(np.array([1, 2, 3, 4, 5]))
    with pytest.raises(RuntimeError):  # tests/series_indexing_test.cpp:27-36: mask of a different size
        s1.where(S(np.array([False, True, True])))
    with pytest.raises(RuntimeError):  # tests/series_indexing_test.cpp:57-60: take with a boolean mask
        s1.take(S(np.array([False, True, True, True, False])))
    with pytest.raises(RuntimeError):  # tests/series_indexing_test.cpp:17-25: where on an index Series
        S(np.array([1, 2, 3, 4, 5]), is_index=True).where(S(np.array([True, False, True, False, True])))
    with pytest.raises(RuntimeError, match=G.manifest["take_oob_message"]):
        S(np.array([1, 2, 3])).take(S(np.array([0, 5])))
    with pytest.raises(RuntimeError, match="out of bounds"):
        S(np.array([1, 2, 3])).take(S(np.array([-1])))
    for k in kat["take"]:
        assert list(S(np.array(k["v"], np.int64)).take(S(np.array(k["idx"]))).values()) == k["out"]
    # DataFrame mask filter + take over 8 fp64 columns + explicit index (config C2 shape, small)
    n = 200_003
    cols = {f"c{j}": orc.synth_vals(0, n, 20 + j) for j in range(8)}
    df = DF(cols, index=np.arange(n, dtype=np.uint64) * 3)
    mask = df["c0"] > 0.5
    out = df[mask]
    mh = cols["c0"] > 0.5
    for j in range(8):
        assert_f64_bits(out[f"c{j}"].values(), cols[f"c{j}"][mh])
    assert np.array_equal(out.index.to_numpy()[0], (np.arange(n, dtype=np.uint64) * 3)[mh])
    idx = (orc.synth_keys(0, n // 2, n)).astype(np.int64)
    tk = df.take(S(idx))
    for j in range(8):
        assert_f64_bits(tk[f"c{j}"].values(), cols[f"c{j}"][idx])


def test_concat(px, kat):
    DF = px.api.DataFrame
    for k in kat["concat"]:
        a, b = (DF({"number": np.array(p, np.int64)}) for p in k["parts"])
        r = px.api.concat([a, b])
        assert list(r["number"].values()) == k["out"]
        assert list(r.index.to_numpy()[0]) == k["index"]
    rng = np.random.default_rng(5)
    parts, valids = [], []
    for n in (0, 1, 63, 64, 65, 1000, 7):
        parts.append(rng.standard_normal(n))
        valids.append(rng.random(n) > 0.3 if n % 2 else None)
    cols = [px.Column.from_numpy(p, v, offset=i) for i, (p, v) in enumerate(zip(parts, valids))]
    out = px.K.concat(cols)
    vals, ok = out.to_numpy()
    ev, eok = orc.concat(parts, valids)
    assert np.array_equal(ok, eok) and out.null_count == int((~eok).sum())
    assert_f64_bits(vals, ev, valid=eok)


# ------------------------------------------------------------------ group-by
GB = {"sum": 0, "mean": 1, "min": 2, "max": 3, "count": 4}


@pytest.mark.parametrize("hashmode", ["default", "partitioned", "global"])
@pytest.mark.parametrize("name", [c for c in G.cases("groupby") if "synth" not in c])
def test_groupby_golden(px, monkeypatch, name, hashmode):
    if hashmode != "default":  # force the open-addressing table (no dense-domain shortcut), partitioned (2) or global (0) build
        monkeypatch.setenv("PDX_GROUPBY_DENSE", "0")
        monkeypatch.setenv("PDX_HASH_PARTITION", "2" if hashmode == "partitioned" else "0")
    c = G.case(name)
    kvalid = _valid_or_none(c["kvalid"]) if "kvalid" in c else None
    key = px.Column.from_numpy(c["keys"], kvalid, offset=1)
    gb = px.K.GroupByHandle.create(key)
    Gn = len(c["uniq"])
    assert gb.num_groups == Gn
    if Gn == 0:
        return
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), c["ids"])
    uk, uok = gb.unique_keys().to_numpy()
    if "uniq_valid" in c:
        assert np.array_equal(uok, c["uniq_valid"])
        assert np.array_equal(uk[uok], c["uniq"][c["uniq_valid"]])
    else:
        assert uok.all() and np.array_equal(uk, c["uniq"])
    vvalid = _valid_or_none(c["vvalid"]) if "vvalid" in c else None
    for col, keyname in (("f", "vf"), ("i", "vi")):
        if keyname not in c:
            continue
        vcol = px.Column.from_numpy(c[keyname], vvalid, offset=2)
        outs = gb.agg(vcol, list(GB.values()))  # all five from one grouped pass
        assert gb.last_plan()["slots"] == pinned_slots("groupby_golden", name, hashmode)
        assert gb.last_plan() == pinned_plan("groupby_golden", name, hashmode, col)
        for (k, kind), out in zip(GB.items(), outs):
            vals, ok = out.to_numpy()
            exp = c[f"{col}_{k}"]
            eok = np.ones(Gn, bool) if k == "count" else c[f"{col}_ok"]
            if ok is not None:
                assert np.array_equal(ok, eok), f"{name} {col} {k} validity"
            else:
                assert eok.all()
            if vals.dtype == np.float64:
                assert_f64_bits(vals, exp, valid=eok, what=f"{name} {col} {k}")
            else:
                assert np.array_equal(vals[eok], exp[eok]), f"{name} {col} {k}"
        # single-kind calls take the specialised kernels
        for k in ("sum", "min"):
            vals, ok = gb.agg(vcol, [GB[k]])[0].to_numpy()
            eok = c[f"{col}_ok"]
            if vals.dtype == np.float64:
                assert_f64_bits(vals, c[f"{col}_{k}"], valid=eok, what=f"{name} {col} {k} single")
            else:
                assert np.array_equal(vals[eok], c[f"{col}_{k}"][eok])


def test_groupby_synth_golden(px):
    c = G.case("gb_synth_300000_1000")
    n, nk = int(c["n"]), int(c["num_keys"])
    gb = px.K.GroupByHandle.create(px.K.synth_keys(0, n, nk))
    outs = gb.agg(px.K.synth_vals(0, n), [0, 1, 4, 2, 3])
    assert np.array_equal(gb.unique_keys().to_numpy()[0], c["uniq"])
    for out, k in zip(outs, ("sum", "mean", "count", "min", "max")):
        vals = out.to_numpy()[0]
        if k == "count":
            assert np.array_equal(vals, c["f_count"])
        else:
            assert_f64_bits(vals, c[f"f_{k}"], what=k)


def test_groupby_kat(px, kat):
    DF = px.api.DataFrame
    for k in kat["groupby"]:
        cols = {"__key": np.array(k["keys"], np.int64)}
        cols.update({nm: np.array(v, np.int64) for nm, v in k["cols"].items()})
        gb = DF(cols).group_by("__key")
        assert gb.groupSize() == len(k["uniques"])
        assert list(gb.unique().to_numpy()[0]) == k["uniques"], k["src"]
        for agg in ("sum", "mean", "min", "max", "count"):
            for cname, exp in k.get(agg, {}).items():
                got = getattr(gb, agg)(cname).values()
                assert list(got) == exp, (k["src"], agg, cname)
        if "frame_sum" in k:
            r = gb.sum(list(k["cols"].keys()))
            tot = sum(r[c].values() for c in k["cols"])
            assert list(tot) == k["frame_sum"]


@pytest.mark.parametrize("dense", ["1", "0", "0-global"])
@pytest.mark.parametrize("n,nk", [(1, 1), (70_001, 1), (1_000_003, 100_003), (2_500_000, 7), (5_000_000, 1_000_000), (6_000_000, 2_500_000),
                                  (4_000_000, 400_000_000), (6_000_000, 5_000)])
def test_groupby_sizes_vs_oracle(px, monkeypatch, n, nk, dense):
    if dense == "0-global":
        dense = "0"
        monkeypatch.setenv("PDX_HASH_PARTITION", "0")
    """group sizes from 1 row to millions of rows (multi-chunk counter path); both key->slot paths: the dense-domain fast
    path (slot = key - min) and the open-addressing hash table incl. table growth (nk > 70 % of the initial 2^21 slots)."""
    monkeypatch.setenv("PDX_GROUPBY_DENSE", dense)
    keys, vals = orc.synth_keys(0, n, nk), orc.synth_vals(0, n) - 0.5
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    s, m, cnt, lo, hi = gb.agg(px.Column.from_numpy(vals), [0, 1, 4, 2, 3])
    assert gb.last_plan()["slots"] == pinned_slots("groupby_sizes_vs_oracle", n, nk, dense, os.environ.get("PDX_HASH_PARTITION", "default"))
    assert gb.last_plan() == pinned_plan("groupby_sizes_vs_oracle", n, nk, dense, os.environ.get("PDX_HASH_PARTITION", "default"))
    ek, es, em, ec = orc.groupby_sum_mean_count(keys, vals, nthreads=8)
    assert np.array_equal(gb.unique_keys().to_numpy()[0], ek)
    assert np.array_equal(cnt.to_numpy()[0], ec)
    assert_f64_bits(s.to_numpy()[0], es, what="sum")
    assert_f64_bits(m.to_numpy()[0], em, what="mean")
    ids, uniq, _, first = orc.group_ids(keys)
    assert np.array_equal(gb.first_rows().cpu().numpy(), first)
    assert_f64_bits(lo.to_numpy()[0], orc.groupby_agg(orc.AGG_MIN, ids, len(uniq), vals, nthreads=8)[0], what="min")
    assert_f64_bits(hi.to_numpy()[0], orc.groupby_agg(orc.AGG_MAX, ids, len(uniq), vals, nthreads=8)[0], what="max")


@pytest.mark.parametrize("dense", ["1", "0"])
@pytest.mark.parametrize("n,nk,dtype", [(300_007, 100_000, "f"), (300_007, 100_000, "i"), (1_200_011, 900_000, "f"), (70_001, 40_000, "f"),
                                        (2_000_003, 50_000, "f")])
def test_groupby_skewed_vs_oracle(px, monkeypatch, n, nk, dtype, dense):
    """both key->slot paths, float64 and int64 values, all five aggregates; skewed group sizes (2 hot keys holding ~1/7 and
    ~1/11 of the rows) so single groups span many sort tiles, many leaves and the multi-chunk counter path."""
    monkeypatch.setenv("PDX_GROUPBY_DENSE", dense)
    monkeypatch.setenv("PDX_HASH_PARTITION", "2")
    keys = orc.synth_keys(0, n, nk)
    keys[::7] = 5
    keys[1::11] = nk - 1
    vals = (orc.synth_vals(0, n) - 0.5) * 1e6 if dtype == "f" else orc.synth_keys(9, n, 1 << 40) - (1 << 39)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    ids, uniq, _, _ = orc.group_ids(keys)
    outs = gb.agg(px.Column.from_numpy(vals), [0, 1, 4, 2, 3])
    assert gb.last_plan()["slots"] == pinned_slots("groupby_skewed_vs_oracle", n, nk, dtype, dense)
    assert gb.last_plan() == pinned_plan("groupby_skewed_vs_oracle", n, nk, dtype, dense)
    assert np.array_equal(gb.unique_keys().to_numpy()[0], uniq)
    for out, kind in zip(outs, (orc.AGG_SUM, orc.AGG_MEAN, orc.AGG_COUNT, orc.AGG_MIN, orc.AGG_MAX)):
        got = out.to_numpy()[0]
        exp = orc.groupby_agg(kind, ids, len(uniq), vals, nthreads=8)[0]
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, what=f"kind={kind}")
        else:
            assert np.array_equal(got, exp), f"kind={kind}"
    for kind in (orc.AGG_SUM, orc.AGG_COUNT, orc.AGG_MAX):  # single-kind specialisations
        got = gb.agg(px.Column.from_numpy(vals), [kind])[0].to_numpy()[0]
        exp = orc.groupby_agg(kind, ids, len(uniq), vals, nthreads=8)[0]
        assert (np.array_equal(got.view(np.uint64), exp.view(np.uint64)) if exp.dtype == np.float64 else np.array_equal(got, exp)), f"single kind={kind}"


@pytest.mark.parametrize("dense", ["1", "0", "0-global"])
def test_groupby_dense_with_nulls_and_negative_keys(px, monkeypatch, dense):
    if dense == "0-global":
        dense = "0"
        monkeypatch.setenv("PDX_HASH_PARTITION", "0")
    monkeypatch.setenv("PDX_GROUPBY_DENSE", dense)
    n = 300_001
    keys = orc.synth_keys(0, n, 5000) - 2500
    valid = orc.synth_keys(3, n, 17) != 0
    vals = orc.synth_vals(0, n)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys, valid, offset=3))
    ids, uniq, isnull, first = orc.group_ids(keys, valid)
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), ids)
    uk, uok = gb.unique_keys().to_numpy()
    assert np.array_equal(uok, ~isnull) and np.array_equal(uk[uok], uniq[~isnull])
    assert np.array_equal(gb.first_rows().cpu().numpy(), first)
    s = gb.agg(px.Column.from_numpy(vals), [0])[0].to_numpy()[0]
    assert gb.last_plan()["slots"] == pinned_slots("groupby_dense_with_nulls_and_negative_keys", dense, os.environ.get("PDX_HASH_PARTITION", "default"))
    assert gb.last_plan() == pinned_plan("groupby_dense_with_nulls_and_negative_keys", dense, os.environ.get("PDX_HASH_PARTITION", "default"))
    assert_f64_bits(s, orc.groupby_agg(orc.AGG_SUM, ids, len(uniq), vals)[0])


@pytest.mark.parametrize("part", ["2", "0"])
def test_groupby_special_keys(px, monkeypatch, part):
    monkeypatch.setenv("PDX_HASH_PARTITION", part)
    keys = np.array([np.iinfo(np.int64).min, 5, np.iinfo(np.int64).min, 0, 5, np.iinfo(np.int64).max, 0], np.int64)
    valid = np.array([1, 1, 1, 0, 1, 1, 1], bool)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys, valid))
    ids, uniq, isnull, _ = orc.group_ids(keys, valid)
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), ids)
    uk, uok = gb.unique_keys().to_numpy()
    assert np.array_equal(uok, ~isnull) and np.array_equal(uk[uok], uniq[~isnull])


# ------------------------------------------------------------------ resample
@pytest.mark.parametrize("name", G.cases("resample"))
def test_resample_golden(px, name):
    c = G.case(name)
    S = px.api.Series
    ts = px.Column.from_numpy(c["ts"], dtype=px.L.TIMESTAMP_NS)
    ser = S(c["v"], index=ts, name="v")
    kw = dict(closed_right=bool(c["closed_right"]), label_right=bool(c["label_right"]))
    if bool(c["upsampling"]):
        with pytest.raises(RuntimeError, match="upSampling"):
            ser.resample(int(c["freq"]), **kw)
        return
    r = ser.resample(int(c["freq"]), **kw)
    assert np.array_equal(r.index().to_numpy()[0], c["labels"]), name
    assert_f64_bits(r.mean()["v"].values(), c["mean"], what=name)
    assert_f64_bits(r.sum()["v"].values(), c["sum"], what=name)
    assert np.array_equal(r.count()["v"].values(), c["counts"])
    assert np.array_equal(r._h.row_labels().cpu().numpy(), orc.resample_row_labels(c["ts"], int(c["freq"]), **kw))


def test_resample_kat_and_errors(px, kat):
    S = px.api.Series
    for k in kat["resample"]:
        ts = px.K.synth_ts(0, k["n"], k["t0_ns"], k["step_ns"])
        ser = S(np.array(k["values"], np.int64), index=ts, name="i")
        r = ser.resample("3T", closed_right=k["closed_right"], label_right=k["label_right"])
        assert list(r.index().to_numpy()[0]) == k["labels"], k["src"]
        assert list(r.sum()["i"].values()) == k["sum"], k["src"]
    with pytest.raises(RuntimeError, match="sorted"):
        S(np.arange(4.0), index=px.Column.from_numpy(np.array([5, 4, 7, 8]) * 10**9, dtype=px.L.TIMESTAMP_NS)).resample("1S")


@pytest.mark.parametrize("density", [0.03, 0.5, 0.97])
def test_resample_and_groupby_null_values_vs_oracle(px, density):
    """null VALUES restart Arrow's 16-row leaves at every run of valid rows: long runs, alternating rows and mostly-null columns,
    through both layouts of the nullable segmented reduce (contiguous resample bins and sorted hash groups)."""
    n = 400_003
    t0, step = 946_684_800 * 10**9, 100_000_000
    ts, v = orc.synth_ts(0, n, t0, step), (orc.synth_vals(0, n) - 0.5) * 1e3
    valid = orc.synth_vals(0, n, 77) >= density
    valid[1000:9000] = True       # a run of 8000 valid rows spanning many windows and chunks
    valid[20000:20040:2] = False  # alternating
    r = px.api.Series(px.Column.from_numpy(v, valid, offset=5), index=px.Column.from_numpy(ts, dtype=px.L.TIMESTAMP_NS), name="v").resample("1min")
    for agg, kind in (("sum", orc.AGG_SUM), ("mean", orc.AGG_MEAN), ("min", orc.AGG_MIN), ("max", orc.AGG_MAX), ("count", orc.AGG_COUNT)):
        labels, exp, eok = orc.resample_agg(kind, ts, v, 60 * 10**9, valid)
        got, gok = getattr(r, agg)()["v"].to_numpy()
        if gok is not None:
            assert np.array_equal(gok, eok), agg
        else:
            assert eok.all()
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=agg)
        else:
            assert np.array_equal(got[eok], exp[eok]), agg
    keys = orc.synth_keys(0, n, 300)
    keys[::3] = 7  # one group with > 130 000 rows (many chunks)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    ids, uniq, _, _ = orc.group_ids(keys)
    for kind in (orc.AGG_SUM, orc.AGG_MEAN, orc.AGG_COUNT, orc.AGG_MAX):
        got, gok = gb.agg(px.Column.from_numpy(v, valid), [kind])[0].to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), v, valid)
        if gok is not None:
            assert np.array_equal(gok, eok)
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=f"gb kind={kind}")
        else:
            assert np.array_equal(got[eok], exp[eok])


def test_resample_large_vs_oracle(px):
    n = 2_000_000  # C5 shape: 100 ms spacing, 1-minute bins -> 600 rows per bin
    t0, step = 946_684_800 * 10**9, 100_000_000
    ts, v = orc.synth_ts(0, n, t0, step), orc.synth_vals(0, n)
    r = px.api.Series(px.K.synth_vals(0, n), index=px.K.synth_ts(0, n, t0, step), name="v").resample("1min")
    labels, means, _ = orc.resample_agg(orc.AGG_MEAN, ts, v, 60 * 10**9)
    assert np.array_equal(r.index().to_numpy()[0], labels)
    assert_f64_bits(r.mean()["v"].values(), means)


@pytest.mark.parametrize("case", ["uniform", "outlier_small", "outlier_huge", "null_keys", "negative", "window_edge", "no_spec", "two_keys"])
def test_groupby_dense_speculation(px, monkeypatch, case):
    """>= 2^23 rows: the dense build speculates on the width of the key window from a 65536-key sample and computes the exact
    min/max in the same pass (residue slots, key & mask).  Accepted guesses, rejected guesses (an unsampled outlier widens the
    window -> exact dense domain, or far outlier -> hash table), null keys (extra slot), negative keys and windows that straddle a
    multiple of 2^b must all give the oracle's groups in first-occurrence order with bit-equal sums."""
    n = 9_000_011
    keys = orc.synth_keys(0, n, 100_000)
    kvalid = None
    if case == "outlier_small":
        keys = keys % 1000
        keys[1] = 5000            # index 1 is not a sample point (stride ~137 rows): sample says 10 bits, exact span needs 13
    elif case == "outlier_huge":
        keys[12345] = 1 << 40
    elif case == "null_keys":
        kvalid = np.ones(n, bool)
        kvalid[::9] = False
    elif case == "negative":
        keys = keys - 50_000
    elif case == "window_edge":
        keys = keys + (1 << 17) - 7    # [2^17 - 7, 2^17 - 7 + 1e5): residues wrap around
    elif case == "no_spec":
        monkeypatch.setenv("PDX_DENSE_SPECULATE", "0")
    elif case == "two_keys":
        keys = keys % 2               # 4.5 M rows per group: 68 sub-segments each -> the 64-wide level-12 butterfly + a serial tail
    vals = orc.synth_vals(0, n) - 0.5
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys, kvalid))
    s, m, cnt = gb.agg(px.Column.from_numpy(vals), [0, 1, 4])
    ids, uniq, uniq_null, first = orc.group_ids(keys, kvalid)
    uk, uk_valid = gb.unique_keys().to_numpy()
    if kvalid is None:
        assert np.array_equal(uk, uniq)
    else:
        assert np.array_equal(~np.asarray(uk_valid, bool), uniq_null) and np.array_equal(uk[~uniq_null], uniq[~uniq_null])
    assert np.array_equal(gb.first_rows().cpu().numpy(), first)
    G = len(uniq)
    assert_f64_bits(s.to_numpy()[0], orc.groupby_agg(orc.AGG_SUM, ids, G, vals, nthreads=8)[0], what="sum")
    assert_f64_bits(m.to_numpy()[0], orc.groupby_agg(orc.AGG_MEAN, ids, G, vals, nthreads=8)[0], what="mean")
    assert np.array_equal(cnt.to_numpy()[0], np.bincount(ids, minlength=G))
    assert np.array_equal(gb.group_ids().cpu().numpy(), ids)


# ---------------------------------------------------------------- variance / stddev / product / first / last per group
GB_NEXT = {"variance": 5, "stddev": 6, "product": 7, "first": 8, "last": 9}


@pytest.mark.parametrize("hashmode", ["default", "partitioned"])
@pytest.mark.parametrize("name", [c for c in G.cases("groupby") if "synth" not in c])
def test_groupby_next_aggs_golden(px, monkeypatch, name, hashmode):
    """golden vectors made with Arrow's scalar variance / stddev / product kernels and positional first / last per group"""
    if hashmode != "default":
        monkeypatch.setenv("PDX_GROUPBY_DENSE", "0")
        monkeypatch.setenv("PDX_HASH_PARTITION", "2")
    c = G.case(name)
    Gn = len(c["uniq"])
    if Gn == 0:
        return
    kvalid = _valid_or_none(c["kvalid"]) if "kvalid" in c else None
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(c["keys"], kvalid, offset=1))
    vvalid = _valid_or_none(c["vvalid"]) if "vvalid" in c else None
    for col, keyname in (("f", "vf"), ("i", "vi")):
        if keyname not in c:
            continue
        vcol = px.Column.from_numpy(c[keyname], vvalid, offset=2)
        outs = gb.agg(vcol, [0] + list(GB_NEXT.values()))  # together with a standard kind in one call
        assert gb.last_plan()["slots"] == pinned_slots("groupby_next_aggs_golden", name, hashmode)
        assert gb.last_plan() == pinned_plan("groupby_next_aggs_golden", name, hashmode, col)
        for (k, kind), out in zip(GB_NEXT.items(), outs[1:]):
            vals, ok = out.to_numpy()
            exp = c[f"{col}_{k}"]
            eok = c[f"{col}_ok_{k}"] if k in ("first", "last") else c[f"{col}_ok"]
            assert (ok is None and eok.all()) or np.array_equal(ok, eok), f"{name} {col} {k} validity"
            if vals.dtype == np.float64:
                assert_f64_bits(vals, exp, valid=eok, what=f"{name} {col} {k}")
            else:
                assert np.array_equal(vals[eok], exp[eok]), f"{name} {col} {k}"


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("n,nk,dtype", [(300_007, 1000, "f"), (300_007, 3, "f"), (1_200_011, 300_000, "i"), (70_001, 1, "f")])
def test_groupby_next_aggs_vs_oracle(px, n, nk, dtype, nulls):
    """group sizes from a few rows to > 65536 rows (the many-waves path under the variance passes), float64 and int64 values"""
    rng = np.random.default_rng(n + nk)
    keys = orc.synth_keys(0, n, nk)
    vals = (1.0 + (orc.synth_vals(0, n) - 0.5) * 1e-3) if dtype == "f" else rng.integers(-3, 4, n).astype(np.int64)
    vvalid = (rng.random(n) > 0.15) if nulls else None
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    outs = gb.agg(px.Column.from_numpy(vals, vvalid), list(GB_NEXT.values()))
    ids, uniq, _, _ = orc.group_ids(keys)
    for (k, kind), out in zip(GB_NEXT.items(), outs):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, vvalid, nthreads=8)
        assert (ok is None and eok.all()) or np.array_equal(ok, eok), k
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=k)
        else:
            assert np.array_equal(got[eok], exp[eok]), k


def test_resample_next_aggs_vs_oracle(px):
    """the resample handle is a group-by handle over bins: same kinds, values in their original order"""
    n, minute = 200_003, 60 * 10**9
    rng = np.random.default_rng(9)
    ts = 1_600_000_000 * 10**9 + np.sort(rng.integers(0, 700 * minute, n)).astype(np.int64)
    vals = 1.0 + rng.standard_normal(n) * 1e-3
    vvalid = rng.random(n) > 0.1
    gb = px.K.GroupByHandle.resample(px.Column.from_numpy(ts, dtype=px.L.TIMESTAMP_NS), 5 * minute)
    outs = gb.agg(px.Column.from_numpy(vals, vvalid), list(GB_NEXT.values()))
    for (k, kind), out in zip(GB_NEXT.items(), outs):
        got, ok = out.to_numpy()
        _, exp, eok = orc.resample_agg(kind, ts, vals, 5 * minute, valid=vvalid)
        assert np.array_equal(ok, eok), k
        assert_f64_bits(got, exp, valid=eok, what=k)


def test_groupby_split_partition_special_keys(px, monkeypatch):
    """general keys with millions of groups (second partition level), null keys and the INT64_MIN key (both live in dedicated
    slots outside the partitioned table) and nullable values"""
    monkeypatch.setenv("PDX_GROUPBY_DENSE", "0")
    n = 5_000_003
    rng = np.random.default_rng(77)
    keys = orc.synth_keys(0, n, 3_000_000) * 1000003 - 12345
    keys[::50021] = np.iinfo(np.int64).min
    kvalid = rng.random(n) > 0.01
    vals = orc.synth_vals(0, n) - 0.5
    vvalid = rng.random(n) > 0.1
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys, kvalid))
    ids, uniq, isnull, first = orc.group_ids(keys, kvalid)
    assert gb.num_groups == len(uniq)
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), ids)
    uk, uok = gb.unique_keys().to_numpy()
    assert np.array_equal(uok, ~isnull) and np.array_equal(uk[uok], uniq[~isnull])
    assert np.array_equal(gb.first_rows().cpu().numpy(), first)
    s, c, mx = gb.agg(px.Column.from_numpy(vals, vvalid), [0, 4, 3])
    assert gb.last_plan()["slots"] == pinned_slots("groupby_split_partition_special_keys")
    assert gb.last_plan() == pinned_plan("groupby_split_partition_special_keys")
    for out, kind in ((s, 0), (c, 4), (mx, 3)):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, vvalid, nthreads=8)
        assert ok is None or np.array_equal(ok, eok)
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=str(kind))
        else:
            assert np.array_equal(got[eok], exp[eok])


@pytest.mark.parametrize("keyform", ["dense", "hashed"])
def test_groupby_sort_ranked_first_occurrence(px, monkeypatch, keyform):
    """every row its own group and more than 2^22 of them (G > 2^22 and 8 G > n): the groups' first-occurrence order comes from a sort
    of the (first row, slot) pairs instead of the first-row bitmap.  n = 2^22 + 4097 is the smallest shape that takes the branch with a
    ragged last sort tile; a fixed permutation of 0..n-1 as it is (dense slots), and spread by an odd factor (hash table)."""
    monkeypatch.setenv("PDX_GROUPBY_SORTED", "0")  # a permutation is never sorted, but the runs path must not be a matter of luck
    n = (1 << 22) + 4097
    keys = np.random.default_rng(422).permutation(n).astype(np.int64)
    if keyform == "hashed":
        monkeypatch.setenv("PDX_GROUPBY_DENSE", "0")
        keys = keys * 1_000_003 - 987_654_321
    vals = orc.synth_vals(0, n) - 0.5
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    ids, uniq, _, first = orc.group_ids(keys)
    assert gb.num_groups == len(uniq) == n
    assert np.array_equal(gb.unique_keys().to_numpy()[0], uniq)
    assert np.array_equal(gb.first_rows().cpu().numpy(), first)
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), ids)
    s = gb.agg(px.Column.from_numpy(vals), [0])[0].to_numpy()[0]
    slots = gb.last_plan()["slots"]
    assert (slots == "dense") if keyform == "dense" else slots.startswith("hash"), slots
    assert_f64_bits(s, orc.groupby_agg(orc.AGG_SUM, ids, len(uniq), vals, nthreads=8)[0], what="sum")


@pytest.mark.parametrize("narrow", ["default", "0"])
@pytest.mark.parametrize("nulls", [False, True])
def test_groupby_fused_last_digit_and_skew_fallback(px, monkeypatch, nulls, narrow):
    """>= 2^22 rows with >= 2^16 slots: the fused last-digit reduce; a hot key makes one run longer than 2^19 rows, which takes the
    fallback (one more sort pass + the classic reducers).  Both must equal the oracle bit for bit.  Values without nulls go through
    the narrowing sort (4 -> 2 -> 1 byte keys, run / group starts from the scatter offsets) unless PDX_SORT_NARROW=0."""
    if narrow != "default":
        monkeypatch.setenv("PDX_SORT_NARROW", narrow)
    n = 5_000_011
    rng = np.random.default_rng(5)
    vals = orc.synth_vals(0, n) - 0.5
    vvalid = (rng.random(n) > 0.07) if nulls else None
    for hot in (False, True):
        keys = orc.synth_keys(0, n, 300_000)
        if hot:
            keys[rng.random(n) < 0.3] = 4242
        gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
        ids, uniq, _, _ = orc.group_ids(keys)
        # all five kinds (min / max force the literal replay), then sum / mean / count alone (dense thread-per-leaf form / literal
        # replay of nullable values), then the opt-in nullable thread-per-leaf form
        for kinds, env in (([0, 1, 4, 2, 3], None), ([0, 1, 4], None), ([0, 1, 4], "1")):
            if env is not None:
                if not nulls:
                    continue
                monkeypatch.setenv("PDX_FLR_NULL_PW", env)
            outs = gb.agg(px.Column.from_numpy(vals, vvalid), kinds)
            monkeypatch.delenv("PDX_FLR_NULL_PW", raising=False)
            for kind, out in zip(kinds, outs):
                got, ok = out.to_numpy()
                exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, vvalid, nthreads=8)
                assert ok is None or np.array_equal(ok, eok), (hot, kind)
                if exp.dtype == np.float64:
                    assert_f64_bits(got, exp, valid=eok, what=f"hot={hot} kind={kind} kinds={kinds}")
                else:
                    assert np.array_equal(got[eok], exp[eok]), (hot, kind)


@pytest.mark.parametrize("null_pw", ["0", "1"])
@pytest.mark.parametrize("pattern", ["alternate", "runs", "int_mean", "variance"])
def test_groupby_fused_last_digit_nullable_leaf_patterns(px, monkeypatch, pattern, null_pw):
    """null patterns for the thread-per-leaf nullable form of the fused last-digit kernel: runs of valid rows of every length
    1..40 between nulls (leaves cut by nulls, by the 16-value limit and by tile ends), nulls on a group's first rows, an int64 column
    (mean = pairwise sum of the values as doubles) and variance (two fused passes, the second on squared deviations)"""
    monkeypatch.setenv("PDX_FLR_NULL_PW", null_pw)  # 1: thread-per-leaf form (opt-in), 0: literal per-lane replay
    n = 4_600_007
    rng = np.random.default_rng(99)
    keys = orc.synth_keys(0, n, 180_000)
    ids, uniq, _, _ = orc.group_ids(keys)
    if pattern == "alternate":
        vvalid = (np.arange(n) % 3 != 0)
    else:
        gaps = rng.integers(1, 41, n // 8)
        cut = np.cumsum(gaps)
        vvalid = np.ones(n, dtype=bool)
        vvalid[cut[cut < n]] = False
        vvalid[: 200_000] = rng.random(200_000) > 0.7  # mostly null head: groups whose first rows are null
    if pattern == "int_mean":
        vals = rng.integers(-10**12, 10**12, n).astype(np.int64)
        kinds = [1, 4]
    elif pattern == "variance":
        vals = orc.synth_vals(0, n) * 1000.0 - 500.0
        kinds = [5, 1]
    else:
        vals = orc.synth_vals(0, n) - 0.5
        kinds = [0, 1, 4]
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    outs = gb.agg(px.Column.from_numpy(vals, vvalid), kinds)
    for kind, out in zip(kinds, outs):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, vvalid, nthreads=8)
        assert ok is None or np.array_equal(ok, eok), kind
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=f"{pattern} kind={kind}")
        else:
            assert np.array_equal(got[eok], exp[eok]), kind


def test_groupby_fused_last_digit_many_short_leaves(px):
    """nullable values that alternate valid / null inside a ~5e5-row group: every valid row is a leaf of its own, so the per-lane
    binary counter of the fused last-digit kernel climbs to its 19th level (its LDS column holds 20)"""
    n = 4_500_003
    keys = orc.synth_keys(0, n, 200_000)
    keys[:500_000] = 77          # one group of ~5e5 rows: the longest run stays under 2^19 rows, the fused path is taken
    vals = orc.synth_vals(0, n) - 0.5
    vvalid = (np.arange(n) % 2 == 0)
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    ids, uniq, _, _ = orc.group_ids(keys)
    s, m, c = gb.agg(px.Column.from_numpy(vals, vvalid), [0, 1, 4])
    for out, kind in ((s, 0), (m, 1), (c, 4)):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, vvalid, nthreads=8)
        assert ok is None or np.array_equal(ok, eok)
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=str(kind))
        else:
            assert np.array_equal(got[eok], exp[eok])


@pytest.mark.parametrize("dtype", ["f", "i"])
def test_groupby_huge_nullable_group(px, dtype):
    """one group of > 2^22 rows with nullable values (skewed keys): not left to one wave -- its contiguous slice of the grouped
    values goes through the whole-column kernels; all five aggregates must still match the oracle bit for bit"""
    n = 9_000_017
    rng = np.random.default_rng(21)
    keys = orc.synth_keys(0, n, 50_000)
    keys[rng.random(n) < 0.6] = 31337
    vals = (orc.synth_vals(0, n) - 0.5) if dtype == "f" else rng.integers(-1000, 1000, n).astype(np.int64)
    vvalid = rng.random(n) > 0.08
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys))
    ids, uniq, _, _ = orc.group_ids(keys)
    outs = gb.agg(px.Column.from_numpy(vals, vvalid), [0, 1, 2, 3, 4])
    for kind, out in zip([0, 1, 2, 3, 4], outs):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, vvalid, nthreads=8)
        assert ok is None or np.array_equal(ok, eok), kind
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=f"kind={kind}")
        else:
            assert np.array_equal(got[eok], exp[eok]), kind


@pytest.mark.parametrize("head", ["default", "4096"])
@pytest.mark.parametrize("shape", ["random", "late_keys", "hot"])
def test_groupby_hash_half_null_keys(px, monkeypatch, shape, head):
    """general keys where half of the rows carry a null key and a tenth the INT64_MIN key: their two dedicated slots take their
    first rows through an LDS minimum per workgroup (not one global atomic per row).  Such rows share one hash bucket: a bucket
    much longer than the average is built from its head rows by one workgroup and finished in chunks (k_hash_probe_lds_tail;
    head = 4096 forces that split on every bucket; `late_keys`: keys grow with the row number, so the chunks meet keys the head
    never saw and insert them memory-side).  ids, first rows, uniques and sums must match the oracle."""
    monkeypatch.setenv("PDX_GROUPBY_DENSE", "0")
    if head != "default":
        monkeypatch.setenv("PDX_HASH_HEAD_ROWS", head)
    n = 3_000_017
    rng = np.random.default_rng(123)
    if shape == "late_keys":
        keys = (np.arange(n, dtype=np.int64) // 37) * 7_000_003 - 99
    else:
        keys = orc.synth_keys(0, n, 40_000) * 7_000_003 - 99
    if shape == "hot":
        keys[rng.random(n) < 0.6] = 123456789012345
    keys[rng.random(n) < 0.1] = np.iinfo(np.int64).min
    kvalid = rng.random(n) > 0.5
    kvalid[:3] = True            # the null group must not come first by construction
    vals = orc.synth_vals(0, n) - 0.5
    gb = px.K.GroupByHandle.create(px.Column.from_numpy(keys, kvalid))
    ids, uniq, isnull, first = orc.group_ids(keys, kvalid)
    assert gb.num_groups == len(uniq)
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), ids)
    uk, uok = gb.unique_keys().to_numpy()
    assert np.array_equal(uok, ~isnull) and np.array_equal(uk[uok], uniq[~isnull])
    assert np.array_equal(gb.first_rows().cpu().numpy(), first)
    s, c = gb.agg(px.Column.from_numpy(vals), [0, 4])
    assert gb.last_plan()["slots"] == pinned_slots("groupby_hash_half_null_keys", shape, head)
    assert gb.last_plan() == pinned_plan("groupby_hash_half_null_keys", shape, head)
    for out, kind in ((s, 0), (c, 4)):
        got, ok = out.to_numpy()
        exp, eok = orc.groupby_agg(kind, ids, len(uniq), vals, None, nthreads=8)
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=str(kind))
        else:
            assert np.array_equal(got[eok], exp[eok])


@pytest.mark.parametrize("stream", ["default", "0"])
@pytest.mark.parametrize("n", [1, 63, 4097, 300_017])
@pytest.mark.parametrize("sel", [0.0, 0.03, 0.5, 1.0])
def test_filter_streaming_vs_gather(px, monkeypatch, n, sel, stream):
    """columns without validity take the streaming filter (every column read once, selected values written in order); the
    compacted-row-id gather (PDX_FILTER_STREAM=0) must give the same bytes.  Five columns (odd count: the kernel batches two),
    sliced columns and mask (offsets), a mask with nulls under DROP, and all-false / all-true masks."""
    if stream != "default":
        monkeypatch.setenv("PDX_FILTER_STREAM", stream)
    rng = np.random.default_rng(n + int(sel * 100))
    cols_np = [rng.integers(-2**62, 2**62, n).astype(np.int64) if c % 2 else rng.standard_normal(n) for c in range(5)]
    mask = rng.random(n) < sel
    mvalid = rng.random(n) > 0.2
    cols = [px.Column.from_numpy(a, offset=c) for c, a in enumerate(cols_np)]
    for mv, emit in ((None, True), (mvalid, False)):
        M = px.Column.from_numpy(mask, mv, offset=13)
        keep = mask if mv is None else (mask & mv)
        assert px.K.filter_count(M, emit) == int(keep.sum())
        outs = px.K.filter(cols, M, emit)
        for a, out in zip(cols_np, outs):
            got, ok = out.to_numpy()
            assert ok is None or ok.all()
            assert out.null_count == 0
            assert np.array_equal(got.view(np.uint64), a[keep].view(np.uint64))


# ------------------------------------------------------------------ sort / argsort / n_largest
def _sort_golden():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sort_golden.npz"))
    return g, sorted({k[:-2] for k in g.files if k.endswith("_v")})


@pytest.mark.parametrize("name", _sort_golden()[1])
def test_argsort_golden(px, name):
    g, _ = _sort_golden()
    v, valid = g[name + "_v"], g[name + "_valid"]
    col = px.Column.from_numpy(v, None if valid.all() else valid, offset=3)
    for asc, key in ((True, "_asc"), (False, "_desc")):
        got, ok = px.K.argsort(col, asc).to_numpy()
        assert ok is None or ok.all()
        assert np.array_equal(got.astype(np.uint64), g[name + key]), (name, key)


@pytest.mark.parametrize("dtype", ["f64", "i64", "ts"])
def test_argsort_large_vs_oracle_and_series_sort(px, dtype):
    n = 1_500_011
    rng = np.random.default_rng(5)
    if dtype == "f64":
        v = np.round(rng.standard_normal(n) * 1000.0, 1)  # many duplicates: stability matters
        v[rng.random(n) < 0.01] = np.nan
        v[rng.random(n) < 0.01] = -0.0
    elif dtype == "i64":
        v = rng.integers(-2**62, 2**62, n).astype(np.int64)
        v[rng.random(n) < 0.3] = 7
    else:
        v = (946_684_800 * 10**9 + rng.integers(0, 10**6, n) * 10**9).astype("datetime64[ns]")
    valid = rng.random(n) > 0.05
    col = px.Column.from_numpy(v, valid)
    vi = v.astype(np.int64) if dtype == "ts" else v
    for asc in (True, False):
        got, _ = px.K.argsort(col, asc).to_numpy()
        assert np.array_equal(got.astype(np.uint64), orc.argsort(vi, valid, asc)), (dtype, asc)
    # Series::sort = Take of values and index by the sort indices; n_largest = sort(descending) + Slice
    S = px.api.Series
    s = S(v if dtype != "ts" else vi, valid=valid, index=px.Column.from_numpy(np.arange(n, dtype=np.uint64)[::-1].copy()), name="x")
    top = s.n_largest(10)
    order = orc.argsort(vi, valid, False)[:10]
    tv, tok = top.col.to_numpy()
    assert len(tv) == 10 and (tok is None or tok.all() or np.array_equal(tok, valid[order]))
    assert np.array_equal(tv.view(np.uint64), vi[order].view(np.uint64))
    assert np.array_equal(top.index.to_numpy()[0], (np.arange(n, dtype=np.uint64)[::-1])[order])


@pytest.mark.parametrize("stream", ["default", "0"])
@pytest.mark.parametrize("n", [1, 65, 4097, 250_013])
def test_filter_streaming_with_nulls_vs_oracle(px, monkeypatch, n, stream):
    """columns WITH validity and a mask with null slots, both FilterOptions: EMIT_NULL (a null slot selects the row and nulls it in
    every column) and DROP.  The streaming form presets the output bitmaps and clears the bits of null rows; the gather form
    (PDX_FILTER_STREAM=0) assembles them with ballots.  Values of valid rows, validity and null counts must match the oracle."""
    if stream != "default":
        monkeypatch.setenv("PDX_FILTER_STREAM", stream)
    rng = np.random.default_rng(n)
    cols_np = [rng.standard_normal(n), rng.integers(-2**62, 2**62, n).astype(np.int64), rng.standard_normal(n)]
    valids = [rng.random(n) > 0.1, None, rng.random(n) > 0.6]
    mask = rng.random(n) < 0.4
    mvalid = rng.random(n) > 0.15
    cols = [px.Column.from_numpy(a, v, offset=i + 1) for i, (a, v) in enumerate(zip(cols_np, valids))]
    for mv in (None, mvalid):
        for emit in (True, False):
            M = px.Column.from_numpy(mask, mv, offset=5)
            outs = px.K.filter(cols, M, emit)
            for a, v, out in zip(cols_np, valids, outs):
                exp, eok = orc.filter(a, mask, v, mv, emit_null=emit)
                got, ok = out.to_numpy()
                assert len(got) == len(exp)
                ev = np.ones(len(exp), bool) if eok is None else eok
                assert np.array_equal(np.ones(len(exp), bool) if ok is None else ok, ev), (mv is None, emit)
                assert out.null_count == int((~ev).sum())
                assert np.array_equal(got.view(np.uint64)[ev], exp.view(np.uint64)[ev])
