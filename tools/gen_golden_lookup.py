"""Writes tests/golden/lookup_golden.npz from pyarrow 25.0.0 (arrow::compute is_in / index_in / index / min / max / dictionary_encode): run once
where pyarrow is installed.

    python tools/gen_golden_lookup.py

Every value travels as its bit image (uint64), so NaN payloads and signed zeros survive; the manifest lists the cases (tests/_lookup_ref.py
reads the file back)."""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lookup_ref as R  # noqa: E402

PA = {"i64": pa.int64(), "u64": pa.uint64(), "ts": pa.timestamp("ns"), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32()}
STORE = {"i64": pa.int64(), "u64": pa.uint64(), "ts": pa.int64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32()}


def to_arrow(a, valid, dt):
    arr = pa.array(np.ascontiguousarray(a), STORE[dt], mask=None if valid is None else ~np.asarray(valid, bool))
    return arr.view(PA[dt]) if dt == "ts" else arr


def to_numpy(arr, dt):
    """values of a (possibly null-holding) Arrow array as numpy of the case's dtype; nulls read as zero bits"""
    if dt == "ts":
        arr = arr.view(pa.int64())
    ok = ~np.asarray(arr.is_null().to_numpy(zero_copy_only=False), bool)
    buf = arr.buffers()[1]
    host = np.frombuffer(buf, R.NP_DTYPES[dt], count=len(arr), offset=arr.offset * np.dtype(R.NP_DTYPES[dt]).itemsize).copy() if len(arr) else np.zeros(0, R.NP_DTYPES[dt])
    host[~ok] = 0
    return host, ok


def special(dt):
    """values that are easy to get wrong, as an array of the dtype"""
    t = R.NP_DTYPES[dt]
    if dt in ("f64", "f32"):
        u = np.uint32 if dt == "f32" else np.uint64
        nan = np.array([np.nan], t).view(u)[0]
        sign = u(1) << u(t().itemsize * 8 - 1)
        b = np.array([np.array([1.0], t).view(u)[0], nan, nan + u(5), np.array([0.0], t).view(u)[0], sign, nan | sign, np.array([5.0], t).view(u)[0],
                      np.array([7.0], t).view(u)[0], np.array([np.inf], t).view(u)[0], np.array([-np.inf], t).view(u)[0], np.array([-2.5], t).view(u)[0]], u)
        return b.view(t)
    if dt == "u64":
        return np.array([1, 2**63, 2**64 - 1, 0, 2**63 + 5, 5, 7, 2**63 - 1], np.uint64)
    if dt == "i32":
        return np.array([1, -2**31, 2**31 - 1, 0, -1, 5, 7, -5], np.int32)
    return np.array([1, -2**63, 2**63 - 1, 0, -1, 5, 7, -5, 2**40], np.int64)


def main():
    rng = np.random.default_rng(20261019)
    arrays, cases = {}, []

    def store(key, a, valid):
        if key not in arrays:
            arrays[key] = R.bits(a)
            if valid is not None:
                arrays[key + "_ok"] = np.asarray(valid, bool)
        return key

    def add_set(name, dt, a, valid, s, svalid, skip):
        r_in = pc.is_in(to_arrow(a, valid, dt), value_set=to_arrow(s, svalid, dt), skip_nulls=bool(skip))
        r_ix = pc.index_in(to_arrow(a, valid, dt), value_set=to_arrow(s, svalid, dt), skip_nulls=bool(skip))
        assert r_in.null_count == 0 and r_ix.type == pa.int32()
        ok = ~np.asarray(r_ix.is_null().to_numpy(zero_copy_only=False), bool)
        arrays[name + "/is_in"] = np.asarray(r_in.to_numpy(zero_copy_only=False), bool)
        arrays[name + "/index_in"] = np.where(ok, np.asarray(r_ix.fill_null(0).to_numpy(zero_copy_only=False)), 0).astype(np.int32)
        arrays[name + "/index_in_ok"] = ok
        cases.append({"name": name, "kind": "set", "dtype": dt, "a": store(f"in/{name[:name.rindex('_skip')]}/a", a, valid), "set": store(f"in/{name[:name.rindex('_skip')]}/set", s, svalid),
                      "skip_nulls": int(skip)})

    def add_index(name, dt, key, a, valid, value):
        """value: a numpy scalar of the dtype, or None for the null scalar"""
        if value is None:
            sc = pa.scalar(None, PA[dt])
        else:
            sc = to_arrow(np.array([value], R.NP_DTYPES[dt]), None, dt)[0]
        row = pc.index(to_arrow(a, valid, dt), sc).as_py()
        cases.append({"name": name, "kind": "index", "dtype": dt, "a": store(key, a, valid), "value_null": int(value is None),
                      "value_bits": 0 if value is None else int(R.bits(np.array([value], R.NP_DTYPES[dt]))[0]), "row": int(row)})

    def add_argext(name, dt, a, valid):
        arr = to_arrow(a, valid, dt)
        rows = [int(pc.index(arr, pc.min(arr) if not mx else pc.max(arr)).as_py()) for mx in (0, 1)]
        cases.append({"name": name, "kind": "argext", "dtype": dt, "a": store(f"in/{name}/a", a, valid), "argmin": rows[0], "argmax": rows[1]})

    def add_dict(name, dt, a, valid):
        r = pc.dictionary_encode(to_arrow(a, valid, dt), null_encoding="mask")
        codes, ok = to_numpy(r.indices, "i32")
        d, dok = to_numpy(r.dictionary, dt)
        assert dok.all() and r.indices.type == pa.int32()
        arrays[name + "/codes"], arrays[name + "/codes_ok"], arrays[name + "/dict"] = codes, ok, R.bits(d)
        cases.append({"name": name, "kind": "dict", "dtype": dt, "a": store(f"in/{name}/a", a, valid)})

    for dt in R.LOOKUP_DTYPES:
        t = R.NP_DTYPES[dt]
        sp = special(dt)
        # ---- the issue's own example and its relatives: duplicates, a null in the set, payloads, both zeros
        a = np.concatenate([sp, sp[::-1], sp[:3]])
        valid = np.ones(len(a), bool)
        valid[[2, len(sp) + 1]] = False
        s = np.concatenate([sp[[1, 4]], sp[:1], sp[[6, 6, 7]]])           # [nan, -0.0, (null), 5, 5, 7]
        sv = np.ones(len(s), bool)
        sv[2] = False
        for skip in (0, 1):
            add_set(f"{dt}/sp_null_in_set_skip{skip}", dt, a, valid, s, sv, skip)
            add_set(f"{dt}/sp_no_null_in_set_skip{skip}", dt, a, valid, s, None, skip)
            add_set(f"{dt}/sp_no_validity_skip{skip}", dt, a, None, s, sv, skip)
            add_set(f"{dt}/sp_empty_set_skip{skip}", dt, a, valid, s[:0], None, skip)
            add_set(f"{dt}/sp_all_null_set_skip{skip}", dt, a, valid, s[:2], np.zeros(2, bool), skip)
            add_set(f"{dt}/sp_empty_input_skip{skip}", dt, a[:0], None, s, sv, skip)
        # ---- fuzzed: small range so that values repeat, specials sprinkled into set and input
        for n, m in ((1, 1), (63, 2), (65, 40), (700, 300)):
            pool = np.concatenate([sp, rng.integers(0, 50, 60).astype(t)])
            a = pool[rng.integers(0, len(pool), n)]
            s = pool[rng.integers(0, len(pool), m)]
            valid = rng.random(n) > 0.25
            sv = rng.random(m) > 0.2
            for skip in (0, 1):
                add_set(f"{dt}/fuzz_{n}_{m}_skip{skip}", dt, a, valid, s, sv, skip)
        # ---- index
        a = np.concatenate([sp, sp])
        valid = np.ones(len(a), bool)
        valid[[0, 3]] = False  # the first 1 and the first 0.0 / 0 are null: the match is the next row that is equal
        key = f"in/{dt}/index/a"
        for j, v in enumerate(sp):
            add_index(f"{dt}/index_sp{j}", dt, key, a, valid, v)
        add_index(f"{dt}/index_null", dt, key, a, valid, None)
        add_index(f"{dt}/index_absent", dt, key, a, valid, t(99))
        add_index(f"{dt}/index_empty", dt, f"in/{dt}/index/empty", a[:0], None, t(1))
        # ---- argmin / argmax
        zeros = np.array([3, 0, 0, 3], t)
        shapes = {"special": (np.concatenate([sp, sp]), None), "special_nulls": (np.concatenate([sp, sp]), rng.random(2 * len(sp)) > 0.4),
                  "empty": (sp[:0], None), "all_null": (sp, np.zeros(len(sp), bool)), "tie_first_last": (np.array([4, 9, 1, 9, 4, 1], t), None),
                  "one": (sp[:1], None), "fuzz": (rng.integers(0, 1000, 700).astype(t), rng.random(700) > 0.3)}
        if dt in ("f64", "f32"):
            nz = t(-0.0)
            shapes.update({"zeros_pos_first": (np.array([3, 0.0, nz, 3], t), None), "zeros_neg_first": (np.array([3, nz, 0.0, 3], t), None),
                           "zeros_low_pos_first": (np.array([-3, 0.0, nz, -3], t), None), "zeros_low_neg_first": (np.array([-3, nz, 0.0, -3], t), None),
                           "all_nan": (np.array([np.nan, np.nan, np.nan], t), None), "nan_then_number": (np.array([np.nan, np.nan, 2, 1, 2], t), None),
                           "nan_and_null": (np.array([np.nan, 5, np.nan], t), np.array([1, 0, 1], bool))})
        else:
            shapes["zeros"] = (zeros, None)
        for nm, (a, valid) in shapes.items():
            add_argext(f"{dt}/argext_{nm}", dt, a, valid)
        # ---- dictionary_encode
        a = np.concatenate([sp, sp[::-1]])
        valid = np.ones(len(a), bool)
        valid[[5, 9]] = False
        add_dict(f"{dt}/dict_special", dt, a, valid)
        add_dict(f"{dt}/dict_no_validity", dt, a, None)
        add_dict(f"{dt}/dict_null_first", dt, a, np.concatenate([[False], np.ones(len(a) - 1, bool)]))
        add_dict(f"{dt}/dict_all_null", dt, a, np.zeros(len(a), bool))
        add_dict(f"{dt}/dict_empty", dt, a[:0], None)
        pool = np.concatenate([sp, rng.integers(0, 40, 40).astype(t)])
        add_dict(f"{dt}/dict_fuzz", dt, pool[rng.integers(0, len(pool), 700)], rng.random(700) > 0.2)

    arrays["manifest"] = np.array(json.dumps({"arrow": pa.__version__, "cases": cases}))
    out = os.path.join(ROOT, "tests", "golden", "lookup_golden.npz")
    np.savez_compressed(out, **arrays)
    print(f"{len(cases)} cases -> {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
