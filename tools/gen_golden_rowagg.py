#!/usr/bin/env python3
"""Generate tests/golden/rowagg_golden.npz -- golden vectors for pdx_row_aggregate (DataFrame::sum / mean / min / ... over axis = Columns).

TEST INFRASTRUCTURE (same conventions as tools/gen_golden_scan.py).  Drives Arrow C++ 25 through pyarrow, one
pc.call_function(kind, [the row as an array], options) per row, as the reference's DataFrame::forAxis does:
  * every kind x every dtype that takes it, C in 1, 2, 15, 16, 17, 31, 32, 33, 48, 65, 100 columns, skip_nulls 0 / 1, min_count 0
  * min_count 1, C, C + 1 (both skip_nulls) at C = 1, 2, 17, 100; ddof 0, 1, C for variance / stddev at every C
  * rows: no nulls; all null; one valid cell at the first / middle / last column; alternating nulls (every leaf of the sum has one value);
    valid runs of exactly 16, 17 and 32 cells; NaNs with payloads and both signs (tests/_nanbits_inputs.py), +-inf, 0.0 / -0.0 ties,
    all NaN; cancelling magnitudes from 1e-300 to 1e300; integers that wrap, uint64 above 2^63, float32 subnormals; random nulls

Every case is a manifest entry {name, dtype, C, n, runs: [{key, kind, skip_nulls, min_count, ddof}]} plus the arrays `name/a` (C x n,
column after column, as the bits' unsigned view), `name/valid` and per run `name/key/out` (bits; zero under a null) and `name/key/ok`.

Run:  python tools/gen_golden_rowagg.py
"""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rowagg_ref as R  # noqa: E402  (names and dtype tables only: no result in the file comes from the restatement)
from _nanbits_inputs import special_values  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rowagg_golden.npz")
PA_T = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32(), "ts": pa.timestamp("ns"),
        "bool": pa.bool_()}
COLS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 65, 100]
MIN_COUNT_COLS = [1, 2, 17, 100]
ROWS = 36


class Store:
    def __init__(self):
        self.arrays, self.cases = {}, []

    def add(self, case, **arrays):
        self.cases.append(case)
        for k, v in arrays.items():
            self.arrays[f"{case['name']}/{k}"] = v

    def done(self):
        """one blob per element type; the manifest's "arrays" maps `name/field` to [blob, first element, elements]"""
        blobs, index = {}, {}
        for key, v in self.arrays.items():
            v = np.ascontiguousarray(v).reshape(-1)
            blob = "blob_" + v.dtype.name
            parts = blobs.setdefault(blob, [])
            index[key] = [blob, int(sum(len(p) for p in parts)), int(len(v))]
            parts.append(v)
        out = {k: np.concatenate(p) for k, p in blobs.items()}
        out["manifest"] = np.array(json.dumps({"arrow_version": pa.__version__, "cases": self.cases, "arrays": index}, sort_keys=True))
        return out


def run_valid(C, first_run):
    """a valid run of exactly `first_run` cells, one null, then valid cells again"""
    v = np.ones(C, bool)
    if C > first_run:
        v[first_run] = False
    return v


def make_rows(dt, C, rng):
    """-> (a, valid), both (ROWS, C)"""
    t = R.NP_T[dt]
    a = np.zeros((ROWS, C), t)
    valid = np.ones((ROWS, C), bool)
    mid = C // 2
    for r in range(ROWS):
        kind = r % 24
        # ---- values
        if dt == "bool":
            p = (0.5, 0.97, 0.03, 1.0, 0.0)[r % 5]
            a[r] = rng.random(C) < p
        elif dt == "ts":
            a[r] = rng.integers(-2**40, 2**62, C)
        elif dt[0] == "f":
            x = rng.standard_normal(C) * 10.0 ** rng.integers(-3, 4, C)
            if kind in (10, 11):
                x = special_values(rng, C, 0.3, 0.0)
            elif kind == 12:
                x = special_values(rng, C, 0.0, 0.4)
            elif kind in (13, 14):
                x = rng.choice(np.array([0.0, -0.0]), C)
            elif kind == 15:
                x = rng.choice(np.array([0.0, -0.0]), C)
                x[rng.integers(0, C)] = np.nan
            elif kind == 16:  # every value beside its negation, in random order, magnitudes 1e-300 .. 1e300 (float32: 1e-30 .. 1e30)
                e = rng.uniform(-300, 300, (C + 1) // 2) if dt == "f64" else rng.uniform(-30, 30, (C + 1) // 2)
                half = rng.uniform(1, 10, len(e)) * 10.0 ** e
                x = rng.permutation(np.concatenate([half, -half]))[:C]
            elif kind == 17:
                x = special_values(rng, C, 1.0, 0.0)
            elif kind == 20:
                x = rng.choice(np.array([1.5, -2.0, 0.5, 1.0, -1.0]), C)  # a product that stays exact
            elif kind == 21 and dt == "f32":
                x = rng.integers(-2**22, 2**22, C) * 2.0 ** -149  # subnormals
            elif kind == 22:
                x = special_values(rng, C, 0.05, 0.05)
            if dt == "f32" and kind in (10, 11, 17, 22):  # NaNs of float32 with their own payloads
                x = x.astype(np.float32)
                nan = np.isnan(x)
                payload = rng.integers(1, 2**22, C).astype(np.uint32) | np.uint32(0x7FC00000) | (rng.integers(0, 2, C).astype(np.uint32) << np.uint32(31))
                x[nan] = payload.view(np.float32)[nan]
            a[r] = x.astype(t)
        else:
            info = np.iinfo(t)
            if kind in (7, 8, 9, 16):  # sums and products that wrap
                a[r] = rng.integers(info.max // 2, info.max, C, dtype=np.uint64 if dt == "u64" else np.int64).astype(t)
            elif kind == 12 and dt != "u64":
                a[r] = rng.integers(info.min, info.min // 2, C).astype(t)
            elif kind in (13, 14):
                a[r] = rng.choice(np.array([0, 1], t), C)
            elif kind == 20:
                a[r] = rng.choice(np.array([1, 2, 3, 1, 1], t) if dt == "u64" else np.array([1, -2, 3, -1, 1], t), C)
            else:
                a[r] = rng.integers(0 if dt == "u64" else -1000, 1000, C).astype(t)
        # ---- validity
        v = np.ones(C, bool)
        if kind == 1:
            v[:] = False
        elif kind in (2, 3, 4):
            v[:] = False
            v[{2: 0, 3: C - 1, 4: mid}[kind]] = True
        elif kind == 5:
            v[1::2] = False
        elif kind == 6:
            v[0::2] = False
        elif kind in (7, 8, 9):
            v = run_valid(C, {7: 16, 8: 17, 9: 32}[kind])
        elif kind in (11, 14, 18, 22):
            v = rng.random(C) >= 0.15
        elif kind == 19:
            v = rng.random(C) >= 0.5
        elif kind == 23:
            v[0] = False
            v[C - 1] = False
        valid[r] = v
    return a, valid


def arrow_rows(dt, a, valid):
    rows = []
    for r in range(a.shape[0]):
        mask = None if valid[r].all() else ~valid[r]
        if dt == "ts":
            rows.append(pa.array(a[r], type=pa.int64(), mask=mask).cast(pa.timestamp("ns")))
        else:
            rows.append(pa.array(a[r], type=PA_T[dt], mask=mask))
    return rows


def scalar_value(s, rdt):
    if not s.is_valid:
        return 0
    if rdt == "ts":
        return s.value
    return s.as_py()


def run_one(kind, rows, dt, skip, min_count, ddof):
    if kind in ("count", "count_null"):
        opts = pc.CountOptions(mode="only_null" if kind == "count_null" else "only_valid")
        fn = "count"
    elif kind in ("variance", "stddev"):
        opts = pc.VarianceOptions(ddof=ddof, skip_nulls=bool(skip), min_count=min_count)
        fn = kind
    else:
        opts = pc.ScalarAggregateOptions(skip_nulls=bool(skip), min_count=min_count)
        fn = kind
    rdt = R.result_dtype(kind, dt)
    res = [pc.call_function(fn, [row], opts) for row in rows]
    want_t = PA_T[rdt]
    assert all(s.type == want_t for s in res), (kind, dt, res[0].type)
    ok = np.array([s.is_valid for s in res], bool)
    if rdt in ("f64", "f32"):  # through Python floats: a C double either way, NaN payloads survive
        out = np.array([scalar_value(s, rdt) for s in res], np.float64)
        if rdt == "f32":
            wide = out
            out = wide.astype(np.float32)
            nan = np.isnan(wide)  # (keep a float32 NaN's payload through the narrowing)
            out.view(np.uint32)[nan] = ((wide.view(np.uint64)[nan] >> np.uint64(29)) & np.uint64(0x7FFFFF) | np.uint64(0x7F800000)
                                        | ((wide.view(np.uint64)[nan] >> np.uint64(63)) << np.uint64(31))).astype(np.uint32)
    elif rdt == "bool":
        out = np.array([bool(scalar_value(s, rdt)) for s in res], bool)
    elif rdt == "u64":
        out = np.array([scalar_value(s, rdt) for s in res], np.uint64)
    else:
        out = np.array([scalar_value(s, rdt) for s in res], np.int64).astype(R.NP_T[rdt])
    return R.bits(out), ok


def generate():
    rng = np.random.default_rng(20261018)
    st = Store()
    for dt in ("f64", "i64", "u64", "i32", "f32", "ts", "bool"):
        for C in COLS:
            a, valid = make_rows(dt, C, rng)
            rows = arrow_rows(dt, a, valid)
            combos = []
            for kind in R.ACCEPTED[dt]:
                is_var = kind in ("variance", "stddev")
                is_count = kind in ("count", "count_null")
                for skip in (1, 0):
                    combos.append((kind, skip, 0, 1 if is_var else 0))
                    if is_count:
                        break
                if C in MIN_COUNT_COLS and not is_count:
                    for mc in (1, C, C + 1):
                        for skip in (1, 0):
                            combos.append((kind, skip, mc, 0))
                if is_var:
                    for ddof in (0, C):
                        combos.append((kind, 1, 0, ddof))
                    combos.append((kind, 0, 0, 0))
            combos = sorted(set(combos), key=combos.index)
            runs, arrays = [], {"a": R.bits(a.T), "valid": valid.T}
            for kind, skip, mc, ddof in combos:
                key = f"{kind}_s{skip}_m{mc}_d{ddof}"
                out, ok = run_one(kind, rows, dt, skip, mc, ddof)
                runs.append({"key": key, "kind": kind, "skip_nulls": skip, "min_count": mc, "ddof": ddof})
                arrays[key + "/out"] = out
                arrays[key + "/ok"] = ok
            st.add({"name": f"{dt}_c{C}", "dtype": dt, "C": C, "n": ROWS, "runs": runs}, **arrays)
    return st.done()


if __name__ == "__main__":
    store = generate()
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    m = json.loads(str(store["manifest"]))
    print(f"wrote {OUT}: {len(m['cases'])} cases, {sum(len(c['runs']) for c in m['cases'])} runs, {size} bytes")
