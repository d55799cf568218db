#!/usr/bin/env python3
"""Generate tests/golden/scan_golden.npz -- golden vectors for pdx_cumulative / pdx_fill_null (cumsum, cumprod, cummax, cummin, ffill, bfill).

TEST INFRASTRUCTURE (same conventions as tools/gen_golden_narrow.py).  Drives Arrow C++ 25 through pyarrow:
  * cumulative_sum / prod / max / min over int64, uint64, float64, int32, float32 x skip_nulls 0 / 1 x {no nulls, ~10 % nulls, leading and
    trailing nulls, all null} x lengths 0, 1, 63, 64, 65, 4097
  * the edge values: wrap at both widths, signed-zero ties, NaN in values and in start, inf - inf, fp32 overflow and start rounding, every
    start-cast error, the two dtypes Arrow has no kernel for
  * fill_null_forward / fill_null_backward over six dtypes with the same null shapes, and a sliced input

Every case is a manifest entry {name, fn, dtype, start, skip_nulls, compare | error} plus the arrays `name/a`, `name/a_valid`, `name/out`,
`name/out_valid` (floats are stored as their bits' unsigned view so that NaN payloads and signed zeros survive).  compare:
  "exact"   bit for bit (integer sum / product, max / min, fills, and float sums / products whose every partial result is exactly
            representable: any order of evaluation gives these bits)
  "rounded" float sum / product of values that round: held to the a-priori error bound of any summation order, not to Arrow's bits
  "nanpos"  float sum / product with NaN / infinities: the rows that are NaN, +inf, -inf are compared, finite rows as "rounded"

Run:  python tools/gen_golden_scan.py
"""
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "scan_golden.npz")

PA_T = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32(), "ts": pa.timestamp("ns"),
        "bool": pa.bool_()}
NP_T = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "f32": np.float32, "ts": np.int64}
BITS_T = {"i64": np.uint64, "u64": np.uint64, "f64": np.uint64, "i32": np.uint32, "f32": np.uint32, "ts": np.uint64}
CUM = {"sum": "cumulative_sum", "prod": "cumulative_prod", "max": "cumulative_max", "min": "cumulative_min"}
CUM_DT = ["i64", "u64", "f64", "i32", "f32"]
LENGTHS = [0, 1, 63, 64, 65, 4097]
NULL_SHAPES = ["none", "tenth", "ends", "all"]


class Store:
    def __init__(self):
        self.arrays, self.cases = {}, []

    def add(self, name, meta, **arrays):
        assert all(c["name"] != name for c in self.cases), name
        self.cases.append(dict(meta, name=name))
        for k, v in arrays.items():
            self.arrays[f"{name}/{k}"] = v

    def done(self):
        """a zip member per array would cost more than the data: the arrays are packed into one blob per element type, and the manifest's
        "arrays" maps `name/field` to [blob, first element, elements] (tests/_scan_ref.py load_golden unpacks them)"""
        blobs, index = {}, {}
        for key, v in self.arrays.items():
            v = np.ascontiguousarray(v)
            blob = "blob_" + v.dtype.name
            parts = blobs.setdefault(blob, [])
            index[key] = [blob, int(sum(len(p) for p in parts)), int(len(v))]
            parts.append(v)
        out = {k: np.concatenate(p) for k, p in blobs.items()}
        out["manifest"] = np.array(json.dumps({"arrow_version": pa.__version__, "cases": self.cases, "arrays": index}, sort_keys=True))
        return out


def bits(a, dt):
    return np.ascontiguousarray(a).view(BITS_T[dt])


def validity(shape, n, rng):
    if shape == "none":
        return None
    if shape == "all":
        return np.zeros(n, bool)
    if shape == "tenth":
        return rng.random(n) >= 0.1
    v = rng.random(n) >= 0.05  # "ends": nulls at both ends and a few inside
    k = max(1, min(5, n // 3))
    v[:k] = False
    v[n - k:] = False
    return v


def arrow_array(a, valid, dt):
    mask = None if valid is None else ~valid
    if dt == "ts":
        return pa.array(a.astype(np.int64), type=pa.int64(), mask=mask).cast(pa.timestamp("ns"))
    return pa.array(a, type=PA_T[dt], mask=mask)


def result_arrays(r, dt):
    valid = np.asarray(r.is_valid().to_numpy(zero_copy_only=False), bool)
    if dt == "ts":
        r = r.cast(pa.int64())
    vals = r.fill_null(0).to_numpy(zero_copy_only=False).astype(NP_T[dt])
    return bits(vals, dt), valid


def sparse(rng, n, pool):
    """mostly zeros: the long cases' running sums stay piecewise constant, which is what keeps the file under 1 MiB"""
    v = np.zeros(n)
    k = rng.random(n) < 0.15
    v[k] = rng.choice(pool, int(k.sum()))
    return v


def values(op, dt, n, rng, rounded):
    """inputs whose accumulation is interesting and, unless `rounded`, exact in every order of evaluation"""
    if dt in ("f64", "f32"):
        if op == "sum":
            v = rng.standard_normal(n) * 100 if rounded else sparse(rng, n, [-20.5, 1.125, 3.0, 77.75, -0.0, 512.5])  # dyadic: partial sums exact
        elif op == "prod":
            v = 1 + rng.uniform(-0.05, 0.05, n) if rounded else 2.0 ** rng.integers(-1, 2, n) * rng.choice([-1.0, 1.0], n)
            if not rounded and n > 64:  # keep the running exponent bounded: alternate so that the product stays within 2^+-40
                e = rng.integers(-1, 2, n)
                e[1::2] = -e[0::2][:len(e[1::2])]
                v = 2.0 ** e * rng.choice([-1.0, 1.0], n)
        else:
            v = rng.choice(np.arange(-8, 8) * 12.25, n)
            if n > 4:  # NaN are skipped; signed zeros tie
                v[rng.integers(0, n, max(n // 16, 1))] = np.nan
                v[rng.integers(0, n, max(n // 16, 1))] = 0.0
                v[rng.integers(0, n, max(n // 16, 1))] = -0.0
        return v.astype(NP_T[dt])
    # small magnitudes keep the file small (it must stay under 1 MiB); the wrap of both widths is in the edge cases
    if op == "prod":  # mostly ones: wraps within ~2000 rows all the same
        v = np.ones(n, np.int64)
        k = rng.random(n) < 0.03
        v[k] = rng.choice([2, 3, 7] if dt == "u64" else [2, 3, -1, -5], int(k.sum()))
        return v.astype(NP_T[dt])
    if op == "sum":
        return sparse(rng, n, [1, 2, 40, 1000] if dt == "u64" else [1, -2, 40, -1000, 7]).astype(NP_T[dt])
    return rng.choice(np.arange(0, 16) if dt == "u64" else np.arange(-8, 8), n).astype(NP_T[dt])


def start_for(op, dt, rng):
    if op == "prod":
        return 1.0 if dt[0] == "f" else 3.0
    if op == "sum":
        return 0.0 if dt == "u64" else -2.0
    return 5.0 if dt == "u64" else -3.0


def add_cum(st, name, op, dt, a, valid, start, skip, compare):
    meta = {"fn": "cum", "op": op, "dtype": dt, "start": repr(float(start)), "skip_nulls": int(skip)}
    arrays = {"a": bits(a, dt) if dt != "bool" else a}
    if valid is not None:
        arrays["a_valid"] = valid
    try:
        r = getattr(pc, CUM[op])(arrow_array(a, valid, dt) if dt != "bool" else pa.array(a), start=start, skip_nulls=bool(skip))
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
        meta["error"] = str(e).split("\n")[0]
        meta["status"] = "not_implemented" if isinstance(e, pa.ArrowNotImplementedError) else "invalid"
        st.add(name, meta, **arrays)
        return
    meta["compare"] = compare
    out, out_valid = result_arrays(r, dt)
    st.add(name, meta, out=out, out_valid=out_valid, **arrays)


def cumulative_cases(st, rng):
    for op in CUM:
        for dt in CUM_DT:
            for skip in (1, 0):
                for shape in NULL_SHAPES:
                    for n in LENGTHS:
                        if shape != "none" and n == 0:
                            continue
                        a = values(op, dt, n, rng, False)
                        v = validity(shape, n, rng)
                        add_cum(st, f"cum_{op}_{dt}_s{skip}_{shape}_{n}", op, dt, a, v, start_for(op, dt, rng), skip, "exact")
    # rounded float sums / products (contract point 3)
    for dt in ("f64", "f32"):
        for op in ("sum", "prod"):
            for shape in ("none", "tenth"):
                for n in (65, 1025):
                    a = values(op, dt, n, rng, True)
                    add_cum(st, f"cumr_{op}_{dt}_{shape}_{n}", op, dt, a, validity(shape, n, rng), 0.25 if op == "sum" else 1.0, 1, "rounded")
    f64, f32, i64, i32, u64 = np.float64, np.float32, np.int64, np.int32, np.uint64
    edge = [
        ("wrap_i32", "sum", "i32", np.array([2**31 - 1, 1, 5], i32), None, 0.0, 1, "exact"),
        ("wrap_i64", "sum", "i64", np.array([2**63 - 1, 1, 5], i64), None, 0.0, 1, "exact"),
        ("wrap_u64", "sum", "u64", np.array([2**64 - 1, 2, 5], u64), None, 0.0, 1, "exact"),
        ("wrap_prod_i32", "prod", "i32", np.array([65536, 65536, 3], i32), None, 1.0, 1, "exact"),
        ("wrap_prod_i64", "prod", "i64", np.array([2**62, 4, 3, -1], i64), None, 1.0, 1, "exact"),
        ("f32_overflow", "sum", "f32", np.array([1e38, 3e38], f32), None, 0.0, 1, "nanpos"),
        ("f32_start_rounds", "sum", "f32", np.array([1, 2], f32), None, 0.1, 1, "exact"),
        ("min_signed_zero", "min", "f64", np.array([0.0, -0.0, 0.0], f64), None, 1.0, 1, "exact"),
        ("max_signed_zero", "max", "f64", np.array([-0.0, 0.0, -0.0], f64), None, -1.0, 1, "exact"),
        ("min_signed_zero_f32", "min", "f32", np.array([0.0, -0.0, 0.0], f32), None, 1.0, 1, "exact"),
        ("max_nan_values", "max", "f64", np.array([np.nan, 1, 9, .5, 3], f64), np.array([1, 1, 0, 1, 1], bool), 0.0, 1, "exact"),
        ("max_nan_start", "max", "f64", np.array([np.nan, 1, np.nan, .5, 3], f64), None, np.nan, 1, "exact"),
        ("min_nan_start_f32", "min", "f32", np.array([np.nan, np.nan, 2, 7], f32), None, np.nan, 1, "exact"),
        ("max_nan_noskip", "max", "f64", np.array([np.nan, 1, 9, .5, 3], f64), np.array([1, 1, 0, 1, 1], bool), 0.0, 0, "exact"),
        ("inf_minus_inf", "sum", "f64", np.array([np.inf, -np.inf, 1], f64), None, 0.0, 1, "nanpos"),
        ("sum_nan_value", "sum", "f64", np.array([1, np.nan, 2], f64), None, 0.0, 1, "nanpos"),
        ("prod_inf_zero", "prod", "f64", np.array([2, np.inf, 0, 5], f64), None, 1.0, 1, "nanpos"),
        ("start_fraction_i64", "sum", "i64", np.array([1, 2], i64), None, 1.5, 1, None),
        ("start_range_i32", "sum", "i32", np.array([1, 2], i32), None, 3e9, 1, None),
        ("start_negative_u64", "sum", "u64", np.array([1, 2], u64), None, -1.0, 1, None),
        ("start_nan_i64", "max", "i64", np.array([1, 2], i64), None, np.nan, 1, None),
        ("start_2p63_i64", "min", "i64", np.array([1, 2], i64), None, 2.0**63, 1, None),
        ("start_fraction_i32", "prod", "i32", np.array([1, 2], i32), None, -0.25, 1, None),
        ("start_big_f32", "sum", "f32", np.array([1, 2], f32), None, 1e300, 1, "nanpos"),
    ]
    for name, op, dt, a, v, start, skip, compare in edge:
        add_cum(st, "edge_" + name, op, dt, a, v, start, skip, compare)
    for op in CUM:
        add_cum(st, f"edge_ts_{op}", op, "ts", np.array([1, 2, 3], np.int64), None, 0.0, 1, None)
        add_cum(st, f"edge_bool_{op}", op, "bool", np.array([True, False]), None, 0.0, 1, None)


def fill_cases(st, rng):
    for dt in CUM_DT + ["ts"]:
        for shape in NULL_SHAPES:
            for n in LENGTHS:
                if shape != "none" and n == 0:
                    continue
                a = (rng.choice(np.arange(-8, 8) * 12.25, n) if dt[0] == "f" else rng.choice(np.arange(0, 16) * 1001, n)).astype(NP_T[dt])
                v = validity(shape, n, rng)
                for back in (0, 1):
                    r = (pc.fill_null_backward if back else pc.fill_null_forward)(arrow_array(a, v, dt))
                    out, out_valid = result_arrays(r, dt)
                    arrays = {"a": bits(a, dt), "out": out, "out_valid": out_valid}
                    if v is not None:
                        arrays["a_valid"] = v
                    st.add(f"fill_{'b' if back else 'f'}_{dt}_{shape}_{n}", {"fn": "fill", "backward": back, "dtype": dt, "compare": "exact"}, **arrays)
    # a slice is filled from its own first row, not from the rows before it
    a = np.arange(40, dtype=np.float64)
    v = np.ones(40, bool)
    v[[3, 4, 5, 6, 20, 21, 36, 37]] = False
    for back in (0, 1):
        full = arrow_array(a, v, "f64")
        sl = full.slice(5, 32)
        r = (pc.fill_null_backward if back else pc.fill_null_forward)(sl)
        out, out_valid = result_arrays(r, "f64")
        st.add(f"fill_{'b' if back else 'f'}_slice", {"fn": "fill", "backward": back, "dtype": "f64", "compare": "exact", "slice": [5, 32]},
               a=bits(a, "f64"), a_valid=v, out=out, out_valid=out_valid)


def generate():
    rng = np.random.default_rng(20261016)
    st = Store()
    cumulative_cases(st, rng)
    fill_cases(st, rng)
    return st.done()


if __name__ == "__main__":
    store = generate()
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    print(f"wrote {OUT}: {len(json.loads(str(store['manifest']))['cases'])} cases, {size} bytes")
