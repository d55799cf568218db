"""Writes tests/golden/quantile_golden.npz from pyarrow 25.0.0 (arrow::compute::Quantile): run once where pyarrow is installed.

    python tools/gen_golden_quantile.py

Inputs are small-range values (they compress, and they tie), so the file stays far below 1 MiB."""
import json
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _quantile_ref as R  # noqa: E402

PA = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "i32": pa.int32(), "f32": pa.float32()}
LENGTHS = (0, 1, 2, 63, 64, 65, 4097)
SHAPES = ("none", "tenth", "ends", "all")


def make_input(dt, n, rng):
    if dt in ("f64", "f32"):
        a = (rng.integers(-4000, 4000, n) / 8.0).astype(R.NP_DTYPES[dt])
        a[a == 0] = 0.125  # never both zeros in a golden input: Arrow's pick between them is its nth_element's
        if n >= 63:
            a[rng.integers(0, n, 4)] = np.nan
            a[rng.integers(0, n)] = np.inf
            a[rng.integers(0, n)] = -np.inf
        return a
    if dt == "u64":
        return rng.integers(0, 5000, n).astype(np.uint64)
    return rng.integers(-2500, 2500, n).astype(R.NP_DTYPES[dt])


def make_valid(shape, n, rng):
    v = np.ones(n, bool)
    if shape == "tenth":
        v[rng.random(n) < 0.1] = False
    elif shape == "ends":
        v[:1] = False
        v[-1:] = False
    elif shape == "all":
        v[:] = False
    return v


def q_list(n_numbers):
    qs = [0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 0.999]
    m = n_numbers - 1
    if m >= 2:  # (n - 1) q exactly on an integer, and exactly on k + 0.5, where the product is exact
        for k in (1, m // 2, m - 1):
            for x in (k / m, (k + 0.5) / m):
                if 0 <= x <= 1 and np.float64(m) * np.float64(x) in (float(k), k + 0.5):
                    qs.append(float(x))
    return qs


def arrow_quantile(a, valid, dt, qs, interp, skip, min_count):
    arr = pa.array(a, PA[dt], mask=~valid)
    r = pc.quantile(arr, q=qs, interpolation=interp, skip_nulls=bool(skip), min_count=int(min_count))
    ok = np.array([x.is_valid for x in r], bool)
    vals = np.array([x.as_py() if x.is_valid else 0 for x in r], np.float64 if interp in ("linear", "midpoint") else R.NP_DTYPES[dt])
    return R.bits(vals), ok


def main():
    rng = np.random.default_rng(20251016)
    arrays, cases = {}, []
    all_bits, all_ok = [], []

    def expect(b, ok):
        """every expected result lives in ONE pair of arrays (thousands of tiny npz members would cost more than their data)"""
        off = sum(len(x) for x in all_bits)
        all_bits.append(np.asarray(b, np.uint64))
        all_ok.append(np.asarray(ok, bool))
        return [off, len(b)]

    def add(name, dt, a, valid, qs, interp, skip=1, min_count=0, in_name=None, valid_name=None):
        in_name = in_name or name + "/in"
        if in_name not in arrays:
            arrays[in_name] = a
        if valid_name is None and not valid.all():
            valid_name = name + "/valid"
        if valid_name and valid_name not in arrays:
            arrays[valid_name] = valid
        b, ok = arrow_quantile(a, valid, dt, qs, interp, skip, min_count)
        cases.append({"name": name, "expect": expect(b, ok), "kind": "column", "dtype": dt, "input": in_name, "valid": valid_name, "q": [float(x) for x in qs], "interpolation": interp,
                      "skip_nulls": int(skip), "min_count": int(min_count)})

    for dt in PA:
        for n in LENGTHS:
            for shape in SHAPES:
                if n == 0 and shape != "none":
                    continue
                a, valid = make_input(dt, n, rng), make_valid(shape, n, rng)
                numbers = int((valid & ~(np.isnan(a) if a.dtype.kind == "f" else np.zeros(n, bool))).sum())
                qs = q_list(numbers)
                base = f"q_{dt}_{shape}_{n}"
                for interp in R.INTERPOLATIONS:
                    for skip, mc, tag in ((1, 0, "s1m0"), (0, 0, "s0m0"), (1, 1, "s1m1"), (1, numbers + 1, "s1mN")):
                        add(f"{base}_{interp}_{tag}", dt, a, valid, qs, interp, skip, mc, in_name=base + "/in", valid_name=None if valid.all() else base + "/valid")
    allv = np.ones(2, bool)
    for interp in R.INTERPOLATIONS:
        add(f"sp_one_inf_{interp}", "f64", np.array([1.0, np.inf]), allv, [0.0, 0.5, 1.0], interp)
        add(f"sp_inf_inf_{interp}", "f64", np.array([-np.inf, np.inf]), allv, [0.0, 0.5, 1.0], interp)
        add(f"sp_big_i64_{interp}", "i64", np.array([2**62, 2**62 + 1], np.int64), allv, [0.0, 0.5, 1.0, 0.3], interp)
        add(f"sp_big_u64_{interp}", "u64", np.array([2**63 + 1, 2**64 - 1, 2**53 + 1], np.uint64), np.ones(3, bool), [0.0, 0.5, 1.0, 0.3, 0.75], interp)
        add(f"sp_huge_f64_{interp}", "f64", np.array([1e308, 1.7e308]), allv, [0.5, 0.25], interp)
        add(f"sp_subnormal_{interp}", "f64", np.array([5e-324, 5e-324, 1.5e-323]), np.ones(3, bool), [0.0, 0.5, 0.25, 0.75, 1.0], interp)
        add(f"sp_tie_even4_{interp}", "i64", np.array([4, 1, 3, 2], np.int64), np.ones(4, bool), [0.5], interp)
        add(f"sp_tie_even6_{interp}", "i64", np.array([6, 5, 4, 3, 2, 1], np.int64), np.ones(6, bool), [0.5, 0.1, 0.3, 0.7, 0.9], interp)
    # errors (q = NaN is not among them: Arrow 25 lets it through and returns NaN; this backend refuses it with the same text)
    for name, dt, a, qs, typ in (("err_q_high", "f64", [1.0, 2.0], [0.5, 1.5], None), ("err_q_low", "i64", [1, 2], [-0.1], None), ("err_q_empty", "f64", [1.0], [], None),
                                 ("err_timestamp", "ts", [1, 2], [0.5], pa.timestamp("ns")), ("err_bool", "bool", [True, False], [0.5], pa.bool_())):
        try:
            pc.quantile(pa.array(a, typ or PA[dt]), q=qs)
            raise SystemExit(name + ": no error")
        except (pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
            cases.append({"name": name, "kind": "error", "dtype": dt, "q": qs, "error": str(e).split("\n")[0],
                          "status": "invalid" if isinstance(e, pa.ArrowInvalid) else "not_implemented"})
    # grouped: per group one Arrow call over the group's rows (what the reference's GroupBy::quantile does), first-occurrence order
    for dt in ("f64", "i64", "u64"):
        for G, n in ((1, 300), (7, 500), (1000, 6000)):
            keys = rng.integers(0, G, n).astype(np.int64) * 3 - 5
            a, valid = make_input(dt, n, rng), make_valid("tenth", n, rng)
            ids, uniq = R.group_ids(keys)
            if G == 7:
                valid[ids == 2] = False  # a group that is all null
                if dt == "f64":
                    a[ids == 3] = np.nan  # a group that is all NaN
                keys = np.concatenate([keys, [10**9]])  # a single-row group
                a = np.concatenate([a, a[:1]])
                valid = np.concatenate([valid, [True]])
                ids, uniq = R.group_ids(keys)
            base = f"g_{dt}_{G}"
            arrays[base + "/keys"], arrays[base + "/in"], arrays[base + "/valid"] = keys, a, valid
            for interp in R.INTERPOLATIONS:
                for q in (0.5, 0.25, 1.0):
                    for skip, mc, tag in ((1, 0, "s1m0"), (0, 0, "s0m0"), (1, 3, "s1m3")):
                        name = f"{base}_{interp}_{q}_{tag}"
                        bb, oo = [], []
                        for g in range(len(uniq)):
                            rows = np.flatnonzero(ids == g)
                            b, ok = arrow_quantile(a[rows], valid[rows], dt, [q], interp, skip, mc)
                            bb.append(b[0])
                            oo.append(ok[0])
                        cases.append({"name": name, "expect": expect(bb, oo), "kind": "group", "dtype": dt, "keys": base + "/keys", "input": base + "/in", "valid": base + "/valid", "q": [q],
                                      "interpolation": interp, "skip_nulls": skip, "min_count": mc})
    arrays["expected_bits"], arrays["expected_ok"] = np.concatenate(all_bits), np.concatenate(all_ok)
    arrays["cases"] = np.frombuffer(json.dumps(cases).encode(), np.uint8)
    out = os.path.join(ROOT, "tests", "golden", "quantile_golden.npz")
    np.savez_compressed(out, **arrays)
    print(f"{out}: {len(cases)} cases, {os.path.getsize(out)} bytes (pyarrow {pa.__version__})")
    assert os.path.getsize(out) < 1 << 20


if __name__ == "__main__":
    main()
