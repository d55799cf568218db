#!/usr/bin/env python3
"""Generate tests/golden/narrow_golden.npz -- golden vectors for the 32-bit columns (PDX_INT32 / PDX_FLOAT32).

TEST INFRASTRUCTURE (same conventions as oracle/gen_golden_r3.py).  Drives Arrow C++ 25 through pyarrow:
  * add / subtract / multiply / divide / bit_wise_* / shift_* between every pair of {int32, float32, int64, float64} in which one
    operand is 32 bits wide, array-array and with a scalar on either side (Arrow's implicit promotion, its checked casts, wrap,
    divide by zero, fp32 rounding, subnormals, NaN payloads)
  * the six comparisons and if_else over the same pairs
  * negate / abs / sign / sqrt / exp / bit_wise_not of int32 and float32
  * sum / mean / min / max / count of int32 and float32 (with nulls)
  * Cast int32 -> int64 / float64, float32 -> float64, int32 / int64 -> float32 (safe), and concat of int32 parts

Every case stores its inputs (`a`, `a_valid`, `b`, `b_valid`, ...) and either the result (`out`, `out_valid`) or the error text
(manifest field "error").  generate() returns the whole store; tests/test_narrow_golden.py regenerates it in memory and compares.

Run:  python tools/gen_golden_narrow.py
"""
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "narrow_golden.npz")

PA_T = {"i32": pa.int32(), "f32": pa.float32(), "i64": pa.int64(), "f64": pa.float64()}
NP_T = {"i32": np.int32, "f32": np.float32, "i64": np.int64, "f64": np.float64}
PAIRS = [("i32", "i32"), ("f32", "f32"), ("i32", "i64"), ("i64", "i32"), ("i32", "f64"), ("f64", "i32"), ("f32", "f64"), ("f64", "f32"),
         ("i32", "f32"), ("f32", "i32"), ("i64", "f32"), ("f32", "i64")]
ARITH = {"add": 0, "sub": 1, "mul": 2, "div": 3}
BITS = {"bit_or": 4, "bit_and": 5, "bit_xor": 6, "shl": 7, "shr": 8}
PC_BIN = {"add": "add", "sub": "subtract", "mul": "multiply", "div": "divide", "bit_or": "bit_wise_or", "bit_and": "bit_wise_and",
          "bit_xor": "bit_wise_xor", "shl": "shift_left", "shr": "shift_right"}
CMPS = {"eq": "equal", "ne": "not_equal", "lt": "less", "le": "less_equal", "gt": "greater", "ge": "greater_equal"}
AGGS = {"sum": 0, "mean": 1, "min": 2, "max": 3, "count": 4}
UNARY = {"negate": "negate", "abs": "abs", "sign": "sign", "sqrt": "sqrt", "exp": "exp", "bit_not": "bit_wise_not"}


def f32_bits(*u):
    return np.array(u, np.uint32).view(np.float32)


def values(kind, n, rng, nonzero=False):
    """n values of `kind` with the edge cases of that kind up front"""
    if kind == "i32":
        edge = np.array([65536, -65536, 2**31 - 1, -(2**31), -1, 1, 0, 7, -7, 16777216, -16777216, 46341], np.int64)
        v = np.concatenate([edge, rng.integers(-1000, 1000, max(n - len(edge), 0))])[:n].astype(np.int32)
    elif kind == "i64":
        edge = np.array([2**40, -(2**40), 2**31, -1, 0, 3, 16777216, -16777216], np.int64)
        v = np.concatenate([edge, rng.integers(-10**6, 10**6, max(n - len(edge), 0))])[:n].astype(np.int64)
    elif kind == "f32":
        edge = np.concatenate([f32_bits(0x7FC00001, 0xFFC00123, 0x00000001, 0x80000005, 0x007FFFFF, 0x7F800000, 0xFF800000),
                               np.array([0.0, -0.0, 1.0 / 3.0, 16777217.0, 3.4e38, 1e-38, 0.1], np.float32)])
        v = np.concatenate([edge, (rng.standard_normal(max(n - len(edge), 0)) * 100).astype(np.float32)])[:n].astype(np.float32)
    else:
        edge = np.array([np.nan, 1.0 / 3.0, -0.0, 1e300, 2.5, 1e-310], np.float64)
        v = np.concatenate([edge, rng.standard_normal(max(n - len(edge), 0)) * 100])[:n]
    if nonzero and kind[0] == "i":
        v = np.where(v == 0, 3, v).astype(v.dtype)
    return v


def in_f32_range(v, kind):
    """integers inside +-2^24 (the checked int -> float32 cast passes)"""
    if kind[0] != "i":
        return v
    return np.clip(v, -16777216, 16777216).astype(v.dtype)


class Store:
    def __init__(self):
        self.arrays, self.cases = {}, {}

    def put(self, case, meta, **arrays):
        assert case not in self.cases, case
        self.cases[case] = meta
        for k, v in arrays.items():
            self.arrays[f"{case}/{k}"] = np.asarray(v)

    def done(self):
        out = dict(self.arrays)
        out["manifest"] = np.array(json.dumps({"arrow_version": pa.__version__, "cases": self.cases}, sort_keys=True))
        return out


def pa_arr(v, valid, kind):
    return pa.array(np.asarray(v, NP_T[kind]), type=PA_T[kind], mask=~np.asarray(valid, bool))


def pa_operand(v, valid, kind, scalar):
    if scalar:
        return pa.scalar(v[0].item() if valid[0] else None, type=PA_T[kind])
    return pa_arr(v, valid, kind)


def result(fn):
    """-> (out values, out valid, error text): nulls read as zeros"""
    try:
        r = fn()
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
        return None, None, str(e)
    if isinstance(r, pa.Scalar):
        return np.array([r.as_py() if r.is_valid else 0]), np.array([r.is_valid]), ""
    valid = np.asarray(r.is_valid().to_numpy(zero_copy_only=False), bool)
    fill = False if pa.types.is_boolean(r.type) else 0
    return np.asarray(r.fill_null(fill).to_numpy(zero_copy_only=False)), valid, ""


def binary_cases(st, rng):
    n = 40
    for da, db in PAIRS:
        both_int = da[0] == "i" and db[0] == "i"
        to_f32 = "f32" in (da, db) and "f64" not in (da, db) and (da[0] == "i" or db[0] == "i")
        ops = dict(ARITH, **(BITS if both_int else {}))
        for name, code in ops.items():
            for side in (0, 1, 2):
                a = values(da, n, rng, nonzero=False)
                b = values(db, n, rng, nonzero=name == "div")
                if name in ("shl", "shr"):
                    b = np.array(([-1, 0, 1, 30, 31, 32, 63, 64] * n)[:n], NP_T[db])
                if to_f32:
                    a, b = in_f32_range(a, da), in_f32_range(b, db)
                av = rng.random(n) > 0.15
                bv = rng.random(n) > 0.15
                if side == 1:
                    b, bv = b[:1].copy(), np.array([True])
                if side == 2:
                    a, av = a[:1].copy(), np.array([True])
                if name == "div" and db[0] == "i":  # no zero divisor at a valid slot (the error cases below)
                    b = np.where(b == 0, 5, b).astype(b.dtype)
                out, ov, err = result(lambda: pc.call_function(PC_BIN[name], [pa_operand(a, av, da, side == 2), pa_operand(b, bv, db, side == 1)]))
                st.put(f"bin_{name}_{da}_{db}_s{side}", {"kind": "binary", "op": code, "side": side, "a": da, "b": db, "error": err},
                       a=a, a_valid=av, b=b, b_valid=bv, **({} if err else {"out": out, "out_valid": ov}))
    # failures: integer divide by zero at a valid slot; the checked int -> float32 cast (the first offending row is named)
    for da, db, a, b, side, op in [("i32", "i32", [1, 2, 3], [1, 0, 1], 0, "div"), ("i32", "i32", [4], [0], 1, "div"),
                                   ("i32", "f32", [1, 16777217, -16777218], [1, 1, 1], 0, "add"),
                                   ("f32", "i32", [1, 1, 1], [0, 5, 16777217], 0, "mul"), ("i64", "f32", [2**40], [1.5], 0, "sub"),
                                   ("f32", "i64", [1.5, 2.5], [3, 2**30], 0, "div"), ("i32", "f32", [16777217], [1, 2], 2, "add")]:
        a, b = np.array(a, NP_T[da]), np.array(b, NP_T[db])
        av, bv = np.ones(len(a), bool), np.ones(len(b), bool)
        out, ov, err = result(lambda: pc.call_function(PC_BIN[op], [pa_operand(a, av, da, side == 2), pa_operand(b, bv, db, side == 1)]))
        assert err, (da, db, op)
        st.put(f"binerr_{op}_{da}_{db}_s{side}_{len(a)}", {"kind": "binary", "op": ARITH[op], "side": side, "a": da, "b": db, "error": err},
               a=a, a_valid=av, b=b, b_valid=bv)
    # a null slot is not looked at by the checked cast
    a, b = np.array([16777217, 2], np.int32), np.array([1.0, 2.0], np.float32)
    av, bv = np.array([False, True]), np.ones(2, bool)
    out, ov, err = result(lambda: pc.add(pa_arr(a, av, "i32"), pa_arr(b, bv, "f32")))
    st.put("bin_add_i32_f32_nullskip", {"kind": "binary", "op": 0, "side": 0, "a": "i32", "b": "f32", "error": err},
           a=a, a_valid=av, b=b, b_valid=bv, out=out, out_valid=ov)


def compare_cases(st, rng):
    n = 40
    for da, db in PAIRS:
        to_f32 = "f32" in (da, db) and "f64" not in (da, db) and (da[0] == "i" or db[0] == "i")
        for name, fn in CMPS.items():
            for side in (0, 1, 2):
                a, b = values(da, n, rng), values(db, n, rng)
                b[5:15] = np.clip(np.nan_to_num(np.asarray(a[5:15], np.float64), posinf=1.0, neginf=-1.0), -2**31, 2**31 - 1).astype(b.dtype)  # ties
                if to_f32:
                    a, b = in_f32_range(a, da), in_f32_range(b, db)
                av, bv = rng.random(n) > 0.15, rng.random(n) > 0.15
                if side == 1:
                    b, bv = b[7:8].copy(), np.array([True])
                if side == 2:
                    a, av = a[7:8].copy(), np.array([True])
                out, ov, err = result(lambda: pc.call_function(fn, [pa_operand(a, av, da, side == 2), pa_operand(b, bv, db, side == 1)]))
                st.put(f"cmp_{name}_{da}_{db}_s{side}", {"kind": "compare", "op": list(CMPS).index(name), "side": side, "a": da, "b": db,
                                                          "error": err}, a=a, a_valid=av, b=b, b_valid=bv, out=out, out_valid=ov)
    a, b = np.array([1, -16777217], np.int32), np.array([1.0, 2.0], np.float32)
    out, ov, err = result(lambda: pc.less(pa_arr(a, np.ones(2, bool), "i32"), pa_arr(b, np.ones(2, bool), "f32")))
    assert err
    st.put("cmperr_lt_i32_f32", {"kind": "compare", "op": 2, "side": 0, "a": "i32", "b": "f32", "error": err},
           a=a, a_valid=np.ones(2, bool), b=b, b_valid=np.ones(2, bool))


def if_else_cases(st, rng):
    n = 70
    for da, db in PAIRS:
        to_f32 = "f32" in (da, db) and "f64" not in (da, db) and (da[0] == "i" or db[0] == "i")
        for side in (0, 1, 2):
            a, b = values(da, n, rng), values(db, n, rng)
            if to_f32:
                a, b = in_f32_range(a, da), in_f32_range(b, db)
            av, bv = rng.random(n) > 0.15, rng.random(n) > 0.15
            cond, cv = rng.random(n) > 0.5, rng.random(n) > 0.1
            if side == 1:
                b, bv = b[3:4].copy(), np.array([True])
            if side == 2:
                a, av = a[3:4].copy(), np.array([True])
            out, ov, err = result(lambda: pc.if_else(pa.array(cond, mask=~cv), pa_operand(a, av, da, side == 2), pa_operand(b, bv, db, side == 1)))
            st.put(f"ifelse_{da}_{db}_s{side}", {"kind": "if_else", "side": side, "a": da, "b": db, "error": err},
                   cond=cond, cond_valid=cv, a=a, a_valid=av, b=b, b_valid=bv, out=out, out_valid=ov)
    # a checked operand fails on an unselected row too: Arrow casts it whole first
    cond = np.array([True, True])
    a, b = np.array([1.0, 2.0], np.float32), np.array([3, 16777217], np.int32)
    out, ov, err = result(lambda: pc.if_else(pa.array(cond), pa_arr(a, np.ones(2, bool), "f32"), pa_arr(b, np.ones(2, bool), "i32")))
    assert err
    st.put("ifelseerr_f32_i32", {"kind": "if_else", "side": 0, "a": "f32", "b": "i32", "error": err},
           cond=cond, cond_valid=np.ones(2, bool), a=a, a_valid=np.ones(2, bool), b=b, b_valid=np.ones(2, bool))


def unary_cases(st, rng):
    n = 60
    for da in ("i32", "f32"):
        for name, fn in UNARY.items():
            if name == "bit_not" and da == "f32":
                continue
            a = values(da, n, rng)
            av = rng.random(n) > 0.15
            out, ov, err = result(lambda: pc.call_function(fn, [pa_arr(a, av, da)]))
            st.put(f"un_{name}_{da}", {"kind": "unary", "op": list(UNARY).index(name), "a": da, "error": err}, a=a, a_valid=av, out=out, out_valid=ov)


def aggregate_cases(st, rng):
    rows = {"i32": [values("i32", 200, rng), np.array([2**31 - 1] * 3, np.int32), rng.integers(-2**31, 2**31, 2000).astype(np.int32)],
            "f32": [values("f32", 200, rng)[7:], (rng.random(6000) * 1000).astype(np.float32), np.full(3000, 0.1, np.float32),
                    np.array([np.nan, np.nan], np.float32), np.array([0.0, -0.0], np.float32)]}
    for da, arrays in rows.items():
        for k, a in enumerate(arrays):
            for nulls in (False, True):
                av = (rng.random(len(a)) > 0.1) if nulls else np.ones(len(a), bool)
                res = {}
                for name in AGGS:  # one case per input: out_<kind> / out_<kind>_valid (a scalar each)
                    out, ov, err = result(lambda: pc.call_function(name, [pa_arr(a, av, da)]))
                    assert not err
                    res[f"out_{name}"], res[f"out_{name}_valid"] = out, ov
                st.put(f"agg_{da}_{k}_{int(nulls)}", {"kind": "aggregate", "a": da, "error": ""}, a=a, a_valid=av, **res)


def cast_cases(st, rng):
    for da, dt in (("i32", "i64"), ("i32", "f64"), ("f32", "f64"), ("i32", "f32"), ("i64", "f32")):
        a = in_f32_range(values(da, 50, rng), da) if dt == "f32" else values(da, 50, rng)
        av = rng.random(50) > 0.1
        out, ov, err = result(lambda: pc.cast(pa_arr(a, av, da), PA_T[dt], safe=True))
        st.put(f"cast_{da}_{dt}", {"kind": "cast", "a": da, "to": dt, "error": err}, a=a, a_valid=av, out=out, out_valid=ov)
    for da, a in (("i32", np.array([5, -16777217, 16777217], np.int32)), ("i64", np.array([2**25 + 1], np.int64))):
        out, ov, err = result(lambda: pc.cast(pa_arr(a, np.ones(len(a), bool), da), pa.float32(), safe=True))
        assert err
        st.put(f"casterr_{da}_f32", {"kind": "cast", "a": da, "to": "f32", "error": err}, a=a, a_valid=np.ones(len(a), bool))
    parts = [values("i32", 13, rng), values("i32", 0, rng), values("i32", 40, rng)]
    valids = [rng.random(len(p)) > 0.2 for p in parts]
    r = pa.concat_arrays([pa_arr(p, v, "i32") for p, v in zip(parts, valids)])
    assert r.type == pa.int32()
    out, ov, _ = result(lambda: r)
    st.put("concat_i32", {"kind": "concat", "a": "i32", "parts": len(parts), "error": ""},
           **{f"p{i}": p for i, p in enumerate(parts)}, **{f"p{i}_valid": v for i, v in enumerate(valids)}, out=out, out_valid=ov)


def generate():
    rng = np.random.default_rng(20261016)
    st = Store()
    binary_cases(st, rng)
    compare_cases(st, rng)
    if_else_cases(st, rng)
    unary_cases(st, rng)
    aggregate_cases(st, rng)
    cast_cases(st, rng)
    return st.done()


if __name__ == "__main__":
    store = generate()
    np.savez_compressed(OUT, **store)
    print(f"wrote {OUT}: {len(json.loads(str(store['manifest']))['cases'])} cases, {os.path.getsize(OUT)} bytes")
