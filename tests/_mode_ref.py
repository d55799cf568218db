"""numpy restatement of the value-frequency rules of include/pdx/abi.h (Arrow C++ 25.0.0's `mode` and `value_counts`, is_unique, the per-group
mode), and the reader of tests/golden/mode_golden.npz (tools/gen_golden_mode.py).  test_mode_golden.py holds the restatement against the
golden on the CPU; the GPU tests use it for the shapes that are too large to freeze."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mode_golden.npz")
NP_DTYPES = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "f32": np.float32, "bool": np.bool_, "ts": np.int64}
MODE_DTYPES = ("i64", "u64", "f64", "i32", "f32", "bool")
N_ERROR = "ModeOptions::n must be strictly positive"
TS_ERROR = "Function 'mode' has no kernel matching input types (timestamp[ns])"


def bits(a):
    """the values' bit patterns as uint64 (bool: 0 / 1)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.astype(np.uint64)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).astype(np.uint64)


def canonical_nan(dtype):
    return np.array([0x7FC00000], np.uint32).view(np.float32)[0] if np.dtype(dtype) == np.float32 else np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def mode(a, valid=None, n=1, skip_nulls=True, min_count=0):
    """-> (modes: a's dtype, counts: int64), both of length k = min(n, distinct valid values), 0 for the empty results.  Ordered by count
    descending, ties by value ascending with NaN (one value, returned canonical) above +inf; -0.0 == 0.0 is one value, returned as the
    zero that comes first in row order."""
    if n <= 0:
        raise ValueError(N_ERROR)
    a = np.asarray(a)
    valid = np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)
    x = a[valid]
    if len(x) == 0 or (not skip_nulls and len(x) < len(a)) or len(x) < min_count:
        return np.zeros(0, a.dtype), np.zeros(0, np.int64)
    key = x
    if a.dtype.kind == "f":
        key = np.where(x == 0, a.dtype.type(0), x)  # both zeros share a key; np.unique folds the NaNs into one, behind +inf
    u, first, counts = np.unique(key, return_index=True, return_counts=True)
    order = np.lexsort((np.arange(len(u)), -counts))[: min(n, len(u))]
    modes = x[first[order]].copy()
    if a.dtype.kind == "f":
        modes[np.isnan(modes)] = canonical_nan(a.dtype)
    return modes, counts[order].astype(np.int64)


def value_counts(a, valid=None):
    """-> (values, value_valid, counts): the distinct bit patterns in first-occurrence order, a null as one entry where the first null is"""
    a = np.asarray(a)
    valid = np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)
    b = bits(a)
    key = np.where(valid, b, 0)
    pair = np.stack([(~valid).astype(np.uint64), key], 1)
    if len(a) == 0:
        return a[:0], np.zeros(0, bool), np.zeros(0, np.int64)
    _, first, counts = np.unique(pair, axis=0, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    rows = first[order]
    vals = a[rows].copy()
    vals[~valid[rows]] = 0
    return vals, valid[rows], counts[order].astype(np.int64)


def is_unique(a, valid=None):
    return len(value_counts(a, valid)[0]) == len(a)


def group_ids(keys, keys_valid=None):
    """first-occurrence group ids (a null key is its own group) -> (ids, number of groups)"""
    keys = np.asarray(keys)
    kv = np.ones(len(keys), bool) if keys_valid is None else np.asarray(keys_valid, bool)
    seen, ids = {}, np.zeros(len(keys), np.int64)
    for i, (k, ok) in enumerate(zip(keys.tolist(), kv.tolist())):
        ids[i] = seen.setdefault(k if ok else None, len(seen))
    return ids, len(seen)


def group_mode(ids, G, a, valid=None):
    """mode(n = 1, skip_nulls, min_count = 0) of every group's rows -> (modes, ok, counts); a group without a valid value: (0, False, 0)"""
    a = np.asarray(a)
    valid = np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)
    modes, ok, counts = np.zeros(G, a.dtype), np.zeros(G, bool), np.zeros(G, np.int64)
    order = np.argsort(ids, kind="stable")
    cuts = np.searchsorted(ids[order], np.arange(G + 1))
    for g in range(G):
        rows = order[cuts[g]:cuts[g + 1]]
        m, c = mode(a[rows], valid[rows])
        if len(m):
            modes[g], ok[g], counts[g] = m[0], True, c[0]
    return modes, ok, counts


def same_values(got, want, ignore_zero_sign=False):
    """bit for bit (a NaN by its bits); ignore_zero_sign: a zero equals the other zero"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    eq = bits(got) == bits(want)
    if ignore_zero_sign and got.dtype.kind == "f":
        eq |= (got == 0) & (want == 0)
    return bool(eq.all())


def holds_both_zeros(a, valid=None):
    a = np.asarray(a)
    if a.dtype.kind != "f":
        return False
    z = a[(np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)) & (a == 0)]
    return bool(len(z) and np.signbit(z).any() and not np.signbit(z).all())


class ModeGolden:
    def __init__(self, path=GOLDEN):
        self.z = np.load(path)
        self.cases = json.loads(bytes(self.z["cases"]).decode())
        self.by_name = {c["name"]: c for c in self.cases}

    def inputs(self, c):
        a = self.z[c["input"]]
        if c["dtype"] in ("f64", "f32"):  # stored as bits: NaN payloads survive
            a = a.view(NP_DTYPES[c["dtype"]])
        valid = self.z[c["valid"]] if c.get("valid") else np.ones(len(a), bool)
        return a, valid

    def keys(self, c):
        return self.z[c["keys"]]

    def expected(self, c):
        """-> (values in the case's dtype, ok, counts)"""
        off, n = c["expect"]
        b = self.z["expected_bits"][off:off + n]
        dt = np.dtype(NP_DTYPES[c["dtype"]])
        if dt == np.bool_:
            vals = b.astype(bool)
        else:
            vals = b.astype({4: np.uint32, 8: np.uint64}[dt.itemsize]).view(dt)
        return vals, self.z["expected_ok"][off:off + n], self.z["expected_counts"][off:off + n]
