"""Writes tests/golden/mode_golden.npz from pyarrow 25.0.0 (arrow::compute::Mode / ValueCounts): run once where pyarrow is installed.

    python tools/gen_golden_mode.py

Inputs are small-range values (they tie, and they compress).  No input holds both zeros except the cases named zeros_*: which zero Arrow
returns from such a column is its unstable sort's choice, not a rule (include/pdx/abi.h)."""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mode_ref as R  # noqa: E402

PA = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32(), "bool": pa.bool_(), "ts": pa.timestamp("ns")}
LENGTHS = (0, 1, 2, 63, 65, 700)
SHAPES = ("none", "third", "all")


def make_input(dt, n, rng):
    if dt in ("f64", "f32"):
        a = (rng.integers(-12, 12, n) / 4.0).astype(R.NP_DTYPES[dt])
        a[a == 0] = 0.125
        if n >= 63:
            b = a.view(np.uint32 if dt == "f32" else np.uint64)
            nan = R.bits(np.array([np.nan], a.dtype))[0]
            for j, payload in zip(rng.integers(0, n, 9), (0, 1, 2, 0, 5, 0, 1, 0, 7)):
                b[j] = (nan + payload) | ((1 << (a.itemsize * 8 - 1)) if payload == 1 else 0)  # NaNs of several payloads and both signs
            a[rng.integers(0, n, 2)] = np.inf
            a[rng.integers(0, n)] = -np.inf
        return a
    if dt == "bool":
        return rng.random(n) < 0.45
    if dt == "u64":
        return (rng.integers(0, 9, n).astype(np.uint64) + np.uint64(2**63 - 4))
    return rng.integers(-5, 6, n).astype(R.NP_DTYPES[dt])


def make_valid(shape, n, rng):
    v = np.ones(n, bool)
    if shape == "third":
        v[rng.random(n) < 0.3] = False
    elif shape == "all":
        v[:] = False
    return v


def arrow_mode(a, valid, dt, n, skip, min_count):
    r = pc.mode(pa.array(a, PA[dt], mask=~valid), n=int(n), skip_nulls=bool(skip), min_count=int(min_count))
    assert r.null_count == 0 and r.field("mode").null_count == 0 and r.field("count").null_count == 0
    m = r.field("mode").to_numpy(zero_copy_only=False).astype(R.NP_DTYPES[dt])
    return R.bits(m), np.ones(len(m), bool), r.field("count").to_numpy(zero_copy_only=False).astype(np.int64)


def main():
    rng = np.random.default_rng(20261018)
    arrays, cases = {}, []
    all_bits, all_ok, all_counts = [], [], []

    def expect(b, ok, counts):
        off = sum(len(x) for x in all_bits)
        all_bits.append(np.asarray(b, np.uint64))
        all_ok.append(np.asarray(ok, bool))
        all_counts.append(np.asarray(counts, np.int64))
        return [off, len(b)]

    def store(name, a, valid):
        if name + "/in" not in arrays:
            arrays[name + "/in"] = a.view(np.uint32 if a.dtype == np.float32 else np.uint64) if a.dtype.kind == "f" else a
            if not valid.all():
                arrays[name + "/valid"] = valid
        return name + "/in", (name + "/valid" if not valid.all() else None)

    def add_mode(name, dt, a, valid, n, skip=1, min_count=0, base=None):
        a = np.asarray(a, R.NP_DTYPES[dt])
        valid = np.asarray(valid, bool)
        in_name, valid_name = store(base or name, a, valid)
        cases.append({"name": name, "kind": "mode", "dtype": dt, "input": in_name, "valid": valid_name, "n": int(n), "skip_nulls": int(skip), "min_count": int(min_count),
                      "expect": expect(*arrow_mode(a, valid, dt, n, skip, min_count))})

    for dt in R.MODE_DTYPES:
        for n in LENGTHS:
            for shape in SHAPES:
                if n == 0 and shape != "none":
                    continue
                a, valid = make_input(dt, n, rng), make_valid(shape, n, rng)
                nvalid = int(valid.sum())
                base = f"m_{dt}_{shape}_{n}"
                for want in (1, 3, 1000):
                    for skip, mc, tag in ((1, 0, "s1m0"), (0, 0, "s0m0"), (1, nvalid, "s1mV"), (1, nvalid + 1, "s1mN")):
                        add_mode(f"{base}_n{want}_{tag}", dt, a, valid, want, skip, mc, base=base)
    one = np.ones
    nan, inf = np.nan, np.inf
    add_mode("sp_nan_wins", "f64", [nan, nan, nan, 1, 1], one(5, bool), 2)
    add_mode("sp_nan_ties_number", "f64", [nan, 2.0, nan, 2.0, inf, inf, -1.0], one(7, bool), 4)
    add_mode("sp_nan_ties_number_f32", "f32", [nan, 2.0, nan, 2.0, inf, inf, -1.0], one(7, bool), 4)
    add_mode("sp_only_nan", "f64", [nan, -nan, nan], one(3, bool), 5)
    add_mode("sp_only_nan_min_count", "f64", [nan, nan, nan], one(3, bool), 1, 1, 3)  # NaN rows count as valid
    add_mode("sp_only_nulls", "i64", [1, 2, 3], np.zeros(3, bool), 1)
    add_mode("sp_tie_at_nth", "i64", [5, 5, 3, 3, 9, 9, 1, 7, 7], one(9, bool), 3)  # four values tie with 2 rows: the three smallest
    add_mode("sp_tie_at_nth_u64", "u64", [2**63 + 5, 2**63 + 5, 3, 3, 2**64 - 1, 2**64 - 1], one(6, bool), 2)
    add_mode("sp_n_beyond_distinct", "i32", [4, -4, 4, 0], one(4, bool), 2**40)
    add_mode("sp_int64_extremes", "i64", [-2**63, 2**63 - 1, 2**63 - 1, -2**63, 0], one(5, bool), 3)
    add_mode("sp_bool_tie", "bool", [True, False, True, False], one(4, bool), 2)
    add_mode("sp_bool_one_value", "bool", [True, True, True], np.array([True, False, True]), 2)
    add_mode("sp_skip_nulls_0_no_null", "i64", [1, 1, 2], one(3, bool), 1, 0, 0)
    add_mode("sp_skip_nulls_0_null", "i64", [1, 1, 2], np.array([True, True, False]), 1, 0, 0)
    # both zeros: the count is the sum; the sign of the returned zero is not compared (names start with zeros_)
    add_mode("zeros_block", "f64", [-0.0] * 20 + [0.0] * 20 + [1.0] * 3, one(43, bool), 2)
    add_mode("zeros_three", "f64", [-0.0, 0.0, 1.0], one(3, bool), 3)
    add_mode("zeros_f32", "f32", [0.0, -0.0, 2.0, -0.0, 2.0], one(5, bool), 2)
    # errors
    for name, dt, a, n in (("err_n_zero", "i64", [1, 2], 0), ("err_n_negative", "f64", [1.0], -1), ("err_timestamp", "ts", [1, 2], 1)):
        try:
            pc.mode(pa.array(a, PA[dt]), n=n)
            raise SystemExit(name + ": no error")
        except (pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
            cases.append({"name": name, "kind": "error", "dtype": dt, "n": n, "error": str(e).split("\n")[0],
                          "status": "invalid" if isinstance(e, pa.ArrowInvalid) else "not_implemented"})

    # value_counts: first-occurrence order, a null is one entry
    def add_vc(name, dt, a, valid):
        a = np.asarray(a, R.NP_DTYPES[dt]) if not isinstance(a, np.ndarray) else a
        valid = np.asarray(valid, bool)
        in_name, valid_name = store(name, a, valid)
        r = pc.value_counts(pa.array(a, PA[dt], mask=~valid))
        v = r.field("values")
        ok = np.array([x.is_valid for x in v], bool)
        if dt == "ts":
            vals = np.array([x.value if x.is_valid else 0 for x in v], np.int64)
        else:
            vals = np.array([x.as_py() if x.is_valid else 0 for x in v], R.NP_DTYPES[dt])
            if a.dtype.kind == "f":  # as_py loses nothing of a float64, but take the buffer: payloads
                vals = v.fill_null(0).to_numpy(zero_copy_only=False).astype(a.dtype)
        cases.append({"name": name, "kind": "value_counts", "dtype": dt, "input": in_name, "valid": valid_name,
                      "expect": expect(R.bits(vals), ok, r.field("counts").to_numpy(zero_copy_only=False).astype(np.int64))})

    for dt in ("i64", "u64", "ts", "f64", "bool"):
        for where in ("absent", "first", "middle"):
            n = 300
            a = make_input("i64" if dt == "ts" else dt, n, rng)
            if dt == "ts":
                a = a * 1_000_000_000 + 1_700_000_000_000_000_000
            valid = np.ones(n, bool)
            if where == "first":
                valid[[0, 17, 200]] = False
            elif where == "middle":
                valid[[150, 151, 299]] = False
            add_vc(f"vc_{dt}_{where}", dt, a, valid)
        add_vc(f"vc_{dt}_empty", dt, np.zeros(0, R.NP_DTYPES[dt]), np.ones(0, bool))
    add_vc("vc_f64_zeros_distinct", "f64", [0.0, -0.0, 0.0, 1.0, -0.0], np.ones(5, bool))
    add_vc("vc_i64_unique", "i64", np.arange(50)[::-1].copy(), np.ones(50, bool))
    add_vc("vc_i64_two_nulls", "i64", np.arange(6), np.array([True, False, True, True, False, True]))

    # grouped: per group one Arrow call over the group's rows, groups in first-occurrence order
    for dt in ("f64", "i64", "u64"):
        for G, n in ((1, 200), (3, 300), (400, 2500)):
            keys = rng.integers(0, G, n).astype(np.int64) * 7 - 11
            a, valid = make_input(dt, n, rng), make_valid("third", n, rng)
            ids, ng = R.group_ids(keys)
            if G == 3:
                valid[ids == 1] = False  # a group that is all null
                if dt == "f64":
                    a[ids == 2] = np.nan  # a group that is all NaN
            base = f"g_{dt}_{G}"
            arrays[base + "/keys"] = keys
            in_name, valid_name = store(base, a, valid)
            bb, oo, cc = [], [], []
            for g in range(ng):
                rows = np.flatnonzero(ids == g)
                b, ok, c = arrow_mode(a[rows], valid[rows], dt, 1, 1, 0)
                bb.append(b[0] if len(b) else 0)
                oo.append(len(b) == 1)
                cc.append(c[0] if len(c) else 0)
            cases.append({"name": base, "kind": "group", "dtype": dt, "keys": base + "/keys", "input": in_name, "valid": valid_name, "expect": expect(bb, oo, cc)})
    arrays["expected_bits"], arrays["expected_ok"], arrays["expected_counts"] = np.concatenate(all_bits), np.concatenate(all_ok), np.concatenate(all_counts)
    arrays["cases"] = np.frombuffer(json.dumps(cases).encode(), np.uint8)
    out = os.path.join(ROOT, "tests", "golden", "mode_golden.npz")
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(cases)} cases, {os.path.getsize(out)} bytes (pyarrow {pa.__version__})")
    assert os.path.getsize(out) < 300 * 1024


if __name__ == "__main__":
    main()
