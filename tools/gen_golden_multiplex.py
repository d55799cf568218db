#!/usr/bin/env python3
"""Generate tests/golden/multiplex_golden.npz -- golden vectors for pdx_coalesce, pdx_element_wise_minmax / pdx_clip,
pdx_replace_with_mask, pdx_indices_nonzero and pdx_all_valid_mask (drop_null).

TEST INFRASTRUCTURE (same conventions as tools/gen_golden_rowagg.py).  Drives Arrow C++ 25 through pyarrow:
  * coalesce            : every dtype, C = 1, 2, 3, 17 (65 for float64 and bool) columns; rows without nulls, all null, null in all but the
                          last column, 5 % nulls, a whole 64-row word null; floats with NaN payloads of both signs, +-0.0, +-inf
  * min / max_element_wise : the six dtypes, both skip_nulls, operand shapes AA, AS, SA, AAA, ASS, SAS, A S(null) A, with signed zeros in
                          both orders, quiet and signalling NaNs, infinities, uint64 above 2^63, the int64 / int32 extremes
  * clip                : max_element_wise(min_element_wise(x, hi), lo) with lo < hi, lo > hi, null lo / hi / both, NaN bounds, zero bounds
  * replace_with_mask   : every dtype; mask / array / replacement with and without nulls; replacement exactly as long as needed and
                          longer; an all-false mask with an empty replacement; the two error messages
  * indices_nonzero     : the six dtypes it takes, with and without nulls
  * drop_null           : record batches of 1, 3 and 17 columns plus a row-id column: the row ids that survive

Every case is a manifest entry {fn, name, dtype, ...} plus the arrays it names (`name/field`; values as the bits' unsigned view, zero
under a null).

Run:  python tools/gen_golden_multiplex.py
"""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _multiplex_ref as R  # noqa: E402  (names and dtype tables only: no result in the file comes from the restatement)

OUT = os.path.join(ROOT, "tests", "golden", "multiplex_golden.npz")
PA_T = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32(), "ts": pa.timestamp("ns"),
        "bool": pa.bool_()}
N = 70


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


def to_arrow(a, valid, dt):
    """numpy -> Arrow without touching a bit of a valid value"""
    a = np.ascontiguousarray(a)
    mask = None if valid is None else ~np.asarray(valid, bool)
    if dt == "ts":
        return pa.array(a.astype(np.int64), mask=mask).view(pa.timestamp("ns"))
    return pa.array(a, type=PA_T[dt], mask=mask)


def to_scalar(a, valid, dt):
    return to_arrow(a, valid, dt)[0]


def from_arrow(arr, dt):
    """Arrow -> (bits, ok): the value buffer as it is, zero under a null"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    assert arr.type == PA_T[dt], (arr.type, dt)
    ok = np.asarray(pc.is_valid(arr).to_numpy(zero_copy_only=False), bool)
    if dt == "bool":
        vals = np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), bool)
        return vals, ok
    t = R.NP_T[dt]
    raw = np.frombuffer(arr.buffers()[1], dtype=t, count=len(arr) + arr.offset)[arr.offset:] if len(arr) else np.zeros(0, t)
    return R.bits(np.where(ok, raw, np.zeros(1, t)).astype(t)), ok


def float_pool(dt):
    if dt == "f64":
        nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123, 0xFFF800000000BEEF, 0x7FF0000000000001, 0xFFF4000000000000],
                        np.uint64).view(np.float64)
        tiny, big = 5e-324, 1.7976931348623157e308
    else:
        nans = np.array([0x7FC00000, 0xFFC00000, 0x7FC00123, 0xFFC0BEEF, 0x7F800001, 0xFFA00000], np.uint32).view(np.float32)
        tiny, big = 1e-45, 3.4028235e38
    t = R.NP_T[dt]
    return nans, np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, big, -big, 1.0, -1.0, 2.5], t)


def values(dt, n, rng, special=0.35):
    """n values of dtype dt: small numbers with many ties, the special values of the dtype mixed in"""
    t = R.NP_T[dt]
    if dt == "bool":
        return rng.random(n) < 0.5
    if dt in ("f64", "f32"):
        nans, others = float_pool(dt)
        a = rng.integers(-3, 4, n).astype(t)
        pick = rng.random(n)
        a = np.where(pick < special * 0.4, rng.choice(nans, n), a)
        a = np.where((pick >= special * 0.4) & (pick < special), rng.choice(others, n), a)
        return a.astype(t)
    if dt == "ts":
        pool = np.array([np.iinfo(np.int64).min + 1, np.iinfo(np.int64).max, 0, -1, 1_700_000_000_000_000_000], np.int64)
    elif dt == "u64":
        pool = np.array([0, 1, 2**63, 2**63 + 1, 2**64 - 1, 2**63 - 1], np.uint64)
    else:
        info = np.iinfo(t)
        pool = np.array([info.min, info.max, info.min + 1, info.max - 1, 0, -1], t)
    a = rng.integers(0 if dt == "u64" else -3, 4, n).astype(t)
    return np.where(rng.random(n) < special, rng.choice(pool, n), a).astype(t)


def validity(kind, C, n, rng):
    """(C, n) bool"""
    v = np.ones((C, n), bool)
    if kind == "none":
        return None
    if kind == "all_null":
        v[:] = False
    elif kind == "last_only":
        v[:-1] = False
    elif kind == "sparse":
        v = rng.random((C, n)) >= 0.05
    elif kind == "word":
        v = rng.random((C, n)) >= 0.3
        v[:, :64] = False
        v[-1, :32] = True
    elif kind == "dense":
        v = rng.random((C, n)) >= 0.6
    return v


# ---------------------------------------------------------------- the functions
def gen_coalesce(st, rng):
    for dt in R.ALL_DTYPES:
        for C in (1, 2, 3, 17) + ((65,) if dt in ("f64", "bool") else ()):
            for vk in ("none", "all_null", "last_only", "sparse", "word", "dense"):
                if C == 65 and vk not in ("dense", "last_only"):
                    continue
                a = np.stack([values(dt, N, rng) for _ in range(C)])
                valid = validity(vk, C, N, rng)
                res = pc.coalesce(*[to_arrow(a[c], None if valid is None else valid[c], dt) for c in range(C)])
                out, ok = from_arrow(res, dt)
                st.add({"fn": "coalesce", "name": f"coalesce_{dt}_c{C}_{vk}", "dtype": dt, "C": C, "n": N, "has_valid": valid is not None},
                       a=R.bits(a), valid=np.ones((C, N), bool) if valid is None else valid, out=out, ok=ok)


SHAPES = ("AA", "AS", "SA", "AAA", "ASS", "SAS", "AnA")  # A array, S scalar, n a null scalar


def gen_minmax(st, rng):
    for dt in R.MINMAX_DTYPES:
        for shape in SHAPES:
            ops, args = [], []
            for k, ch in enumerate(shape):
                m = 1 if ch in "Sn" else N
                a = values(dt, m, rng, 0.5)
                if ch == "A":
                    valid = rng.random(m) >= 0.25 if k != 1 or shape != "AAA" else None
                else:
                    valid = np.array([ch == "S"])
                ops.append((a, valid, ch != "A"))
                args.append(to_scalar(a, valid, dt) if ch != "A" else to_arrow(a, valid, dt))
            arrays = {}
            for k, (a, valid, sc) in enumerate(ops):
                arrays[f"op{k}"] = R.bits(a)
                arrays[f"ok{k}"] = np.ones(len(a), bool) if valid is None else valid
            runs = []
            for is_max in (0, 1):
                for skip in (1, 0):
                    fn = pc.max_element_wise if is_max else pc.min_element_wise
                    out, ok = from_arrow(fn(*args, skip_nulls=bool(skip)), dt)
                    key = f"{'max' if is_max else 'min'}_s{skip}"
                    runs.append({"key": key, "is_max": is_max, "skip_nulls": skip})
                    arrays[key + "/out"], arrays[key + "/ok"] = out, ok
            st.add({"fn": "minmax", "name": f"minmax_{dt}_{shape}", "dtype": dt, "n": N, "scalar": [ch != "A" for ch in shape],
                    "has_valid": [v is not None for _, v, _ in ops], "runs": runs}, **arrays)
        # signed zeros in both orders, against each other and against every operand kind (floats)
        if dt in ("f64", "f32"):
            t = R.NP_T[dt]
            z = np.array([0.0, -0.0, 0.0, -0.0], t)
            w = np.array([-0.0, 0.0, 0.0, -0.0], t)
            for shape, (x, y) in (("AA", (z, w)), ("AS", (z, w[:1])), ("SA", (z[:1], w)), ("AS", (w, z[:1])), ("SA", (w[:1], z))):
                args = [to_scalar(v, None, dt) if ch == "S" else to_arrow(v, None, dt) for ch, v in zip(shape, (x, y))]
                arrays = {"op0": R.bits(x), "ok0": np.ones(len(x), bool), "op1": R.bits(y), "ok1": np.ones(len(y), bool)}
                runs = []
                for is_max in (0, 1):
                    fn = pc.max_element_wise if is_max else pc.min_element_wise
                    out, ok = from_arrow(fn(*args), dt)
                    key = f"{'max' if is_max else 'min'}_s1"
                    runs.append({"key": key, "is_max": is_max, "skip_nulls": 1})
                    arrays[key + "/out"], arrays[key + "/ok"] = out, ok
                name = f"minmax_{dt}_zeros_{shape}_{'neg' if np.signbit(y[0]) else 'pos'}"
                st.add({"fn": "minmax", "name": name, "dtype": dt, "n": max(len(x), len(y)), "scalar": [ch == "S" for ch in shape],
                        "has_valid": [False, False], "runs": runs}, **arrays)


def gen_clip(st, rng):
    for dt in R.MINMAX_DTYPES:
        t = R.NP_T[dt]
        bounds = [("lo_lt_hi", -1 if dt != "u64" else 1, True, 2, True), ("lo_gt_hi", 2, True, -1 if dt != "u64" else 1, True),
                  ("null_lo", 0, False, 2, True), ("null_hi", -1 if dt != "u64" else 1, True, 0, False), ("null_both", 0, False, 0, False),
                  ("equal", 0, True, 0, True)]
        if dt in ("f64", "f32"):
            nans, _ = float_pool(dt)
            bounds += [("nan_lo", nans[2], True, 2.0, True), ("nan_hi", -1.0, True, nans[1], True), ("snan_hi", -1.0, True, nans[4], True),
                       ("zeros", -0.0, True, 0.0, True), ("zeros_rev", 0.0, True, -0.0, True), ("inf", -np.inf, True, np.inf, True)]
        if dt == "u64":
            bounds += [("big", 2**63, True, 2**64 - 2, True)]
        if dt in ("i64", "ts", "i32"):
            info = np.iinfo(t)
            bounds += [("extremes", info.min, True, info.max, True)]
        x = values(dt, N, rng, 0.5)
        xv = rng.random(N) >= 0.2
        for name, lo, lo_ok, hi, hi_ok in bounds:
            lo_a, hi_a = np.array([lo], t), np.array([hi], t)
            arrays = {"x": R.bits(x), "x_ok": xv, "lo": R.bits(lo_a), "hi": R.bits(hi_a)}
            runs = []
            for skip in (1, 0):
                inner = pc.min_element_wise(to_arrow(x, xv, dt), to_scalar(hi_a, np.array([hi_ok]), dt), skip_nulls=bool(skip))
                res = pc.max_element_wise(inner, to_scalar(lo_a, np.array([lo_ok]), dt), skip_nulls=bool(skip))
                out, ok = from_arrow(res, dt)
                runs.append({"key": f"s{skip}", "skip_nulls": skip})
                arrays[f"s{skip}/out"], arrays[f"s{skip}/ok"] = out, ok
            st.add({"fn": "clip", "name": f"clip_{dt}_{name}", "dtype": dt, "n": N, "lo_ok": bool(lo_ok), "hi_ok": bool(hi_ok), "runs": runs}, **arrays)


def gen_replace(st, rng):
    for dt in R.ALL_DTYPES:
        for name, a_nulls, m_nulls, r_nulls, p_true, extra in (("plain", False, False, False, 0.4, 0), ("nulls", True, True, True, 0.4, 0),
                                                              ("longer", True, True, True, 0.6, 5), ("all_false", True, False, False, 0.0, 0),
                                                              ("all_true", False, False, True, 1.0, 0), ("mask_nulls", False, True, False, 0.5, 1)):
            a = values(dt, N, rng)
            av = rng.random(N) >= 0.2 if a_nulls else None
            mask = rng.random(N) < p_true
            mv = rng.random(N) >= 0.2 if m_nulls else None
            need = int((mask & (True if mv is None else mv)).sum())
            repl = values(dt, need + extra, rng)
            rv = rng.random(need + extra) >= 0.3 if r_nulls else None
            res = pc.replace_with_mask(to_arrow(a, av, dt), to_arrow(mask, mv, "bool"), to_arrow(repl, rv, dt))
            out, ok = from_arrow(res, dt)
            st.add({"fn": "replace_with_mask", "name": f"rwm_{dt}_{name}", "dtype": dt, "n": N, "m": need + extra, "need": need,
                    "has_valid": [av is not None, mv is not None, rv is not None]},
                   a=R.bits(a), a_ok=np.ones(N, bool) if av is None else av, mask=mask, mask_ok=np.ones(N, bool) if mv is None else mv,
                   repl=R.bits(repl), repl_ok=np.ones(need + extra, bool) if rv is None else rv, out=out, ok=ok)
    # the two refusals, with Arrow's text
    a, mask = np.arange(5, dtype=np.int64), np.array([True, False, True, True, False])
    errors = {}
    for name, m, r in (("short_repl", mask, np.arange(2, dtype=np.int64)), ("mask_length", mask[:4], np.arange(3, dtype=np.int64))):
        try:
            pc.replace_with_mask(pa.array(a), pa.array(m), pa.array(r))
            raise AssertionError(name)
        except pa.ArrowInvalid as e:
            errors[name] = str(e)
    st.add({"fn": "replace_with_mask_errors", "name": "rwm_errors", "dtype": "i64", "errors": errors})


def gen_nonzero(st, rng):
    for dt in R.NONZERO_DTYPES:
        for nulls in (False, True):
            a = values(dt, N, rng, 0.5)
            av = rng.random(N) >= 0.3 if nulls else None
            res = pc.indices_nonzero(to_arrow(a, av, dt))
            assert res.type == pa.uint64() and res.null_count == 0
            st.add({"fn": "indices_nonzero", "name": f"nonzero_{dt}_{int(nulls)}", "dtype": dt, "n": N, "has_valid": nulls},
                   a=R.bits(a), a_ok=np.ones(N, bool) if av is None else av, out=np.asarray(res.to_numpy(), np.uint64))
    errors = {}
    try:
        pc.indices_nonzero(pa.array([1], pa.timestamp("ns")))
    except pa.ArrowNotImplementedError as e:
        errors["ts"] = str(e)
    try:
        pc.min_element_wise(pa.array([True]), pa.array([False]))
    except pa.ArrowNotImplementedError as e:
        errors["minmax_bool"] = str(e)
    st.add({"fn": "not_implemented", "name": "not_implemented", "dtype": "ts", "errors": errors})


def gen_drop_null(st, rng):
    for C in (1, 3, 17):
        for vk in ("none", "sparse", "dense", "word", "all_null"):
            valid = validity(vk, C, N, rng)
            cols = [to_arrow(values("i64", N, rng), None if valid is None else valid[c], "i64") for c in range(C)]
            batch = pa.RecordBatch.from_arrays(cols + [pa.array(np.arange(N, dtype=np.int64))], [f"c{c}" for c in range(C)] + ["row"])
            kept = pc.drop_null(batch)
            st.add({"fn": "drop_null", "name": f"drop_null_c{C}_{vk}", "dtype": "i64", "C": C, "n": N, "has_valid": valid is not None},
                   valid=np.ones((C, N), bool) if valid is None else valid, rows=np.asarray(kept.column(C).to_numpy(), np.int64))


def generate():
    rng = np.random.default_rng(20261018)
    st = Store()
    gen_coalesce(st, rng)
    gen_minmax(st, rng)
    gen_clip(st, rng)
    gen_replace(st, rng)
    gen_nonzero(st, rng)
    gen_drop_null(st, rng)
    return st.done()


if __name__ == "__main__":
    store = generate()
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    m = json.loads(str(store["manifest"]))
    print(f"wrote {OUT}: {len(m['cases'])} cases, {size} bytes")
