"""Numpy restatement of Arrow C++ 25's exact `quantile` (sort + one interpolation formula), the reference of the GPU tests for inputs too
large to freeze.  tests/test_quantile_golden.py holds it against tests/golden/quantile_golden.npz (pyarrow 25.0.0) case by case."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantile_golden.npz")
INTERPOLATIONS = ("linear", "lower", "higher", "nearest", "midpoint")  # arrow::compute::QuantileOptions::Interpolation, same numbering
NP_DTYPES = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "f32": np.float32}


def bits(x):
    """the comparison image of a result array: float64 / float32 -> their bit patterns, integers -> int64 / uint64"""
    x = np.asarray(x)
    if x.dtype == np.float64:
        return x.view(np.uint64)
    if x.dtype == np.float32:
        return x.view(np.uint32).astype(np.uint64)
    return x.astype(np.uint64) if x.dtype == np.uint64 else x.astype(np.int64).view(np.uint64)


def check_q(qs):
    if len(qs) == 0:
        raise ValueError("Requires quantile argument")
    for q in qs:
        if not (0.0 <= q <= 1.0):  # (NaN included)
            raise ValueError("Quantile must be between 0 and 1")


def quantile(a, valid, qs, interpolation="linear", skip_nulls=True, min_count=0):
    """-> (results, is_valid, n): results float64 (linear / midpoint) or a's dtype; n = valid non-NaN values.
    -0.0 and 0.0 are equal in the order and keep their row order (a stable sort)."""
    check_q(qs)
    a = np.asarray(a)
    valid = np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)
    to_f64 = interpolation in ("linear", "midpoint")
    out = np.zeros(len(qs), np.float64 if to_f64 else a.dtype)
    v = a[valid]
    if v.dtype.kind == "f":
        v = v[~np.isnan(v)]
    n = len(v)
    if n == 0 or int(valid.sum()) < min_count or (not skip_nulls and not valid.all()):  # (min_count counts NaN rows too, as Arrow does)
        return out, np.zeros(len(qs), bool), n
    v = v[np.argsort(v, kind="stable")]
    with np.errstate(all="ignore"):
        for k, q in enumerate(qs):
            index = np.float64(n - 1) * np.float64(q)
            lo = int(index)
            f = index - np.float64(lo)
            hi = min(lo + 1, n - 1) if f != 0 else lo
            if to_f64:
                lower, higher = np.float64(v[lo]), np.float64(v[hi])
                if f == 0:
                    out[k] = lower
                elif interpolation == "linear":
                    out[k] = f * higher + (1 - f) * lower
                else:
                    out[k] = lower / 2 + higher / 2
            elif interpolation == "lower":
                out[k] = v[lo]
            elif interpolation == "higher":
                out[k] = v[hi]
            else:  # nearest: a tie goes to the even index
                out[k] = v[lo] if f < 0.5 else v[hi] if f > 0.5 else v[lo + (lo & 1)]
    return out, np.ones(len(qs), bool), n


def group_ids(keys):
    """dense group ids in first-occurrence order (int64 keys without nulls) -> (ids, unique keys)"""
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    return rank[inv], uniq[order]


def group_quantile(keys, a, valid, q, interpolation="linear", skip_nulls=True, min_count=0):
    """per group (first-occurrence order) the quantile of its rows -> (results [G], is_valid [G])"""
    ids, uniq = group_ids(np.asarray(keys))
    a = np.asarray(a)
    valid = np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)
    to_f64 = interpolation in ("linear", "midpoint")
    out = np.zeros(len(uniq), np.float64 if to_f64 else a.dtype)
    ok = np.zeros(len(uniq), bool)
    order = np.argsort(ids, kind="stable")
    cuts = np.searchsorted(ids[order], np.arange(len(uniq) + 1))
    for g in range(len(uniq)):
        rows = order[cuts[g]:cuts[g + 1]]
        r, k, _ = quantile(a[rows], valid[rows], [q], interpolation, skip_nulls, min_count)
        out[g], ok[g] = r[0], k[0]
    return out, ok


def same(got, got_valid, want_bits, want_valid):
    """bit-equal where valid; a NaN result is compared as "is NaN" """
    got, got_valid, want_valid = np.asarray(got), np.asarray(got_valid, bool), np.asarray(want_valid, bool)
    if not np.array_equal(got_valid, want_valid):
        return False
    gb, wb = bits(got)[want_valid], np.asarray(want_bits, np.uint64)[want_valid]
    if got.dtype.kind == "f":
        g = got[want_valid]
        w = wb.view(np.float64) if got.dtype == np.float64 else wb.astype(np.uint32).view(np.float32)
        nan = np.isnan(g)
        return bool(np.array_equal(nan, np.isnan(w)) and np.array_equal(gb[~nan], wb[~nan]))
    return bool(np.array_equal(gb, wb))


class QuantileGolden:
    def __init__(self, path=GOLDEN):
        self.z = np.load(path)
        self.cases = json.loads(bytes(self.z["cases"]).decode())
        self.bits, self.ok = self.z["expected_bits"], self.z["expected_ok"].astype(bool)

    def inputs(self, case):
        a = self.z[case["input"]]
        valid = self.z[case["valid"]] if case.get("valid") else np.ones(len(a), bool)
        return a, valid.astype(bool)

    def keys(self, case):
        return self.z[case["keys"]]

    def expected(self, case):
        """-> (bit patterns uint64, is_valid)"""
        off, n = case["expect"]
        return self.bits[off:off + n], self.ok[off:off + n]
