"""numpy restatement of the lookup rules of include/pdx/abi.h (pdx_is_in / pdx_index_in / pdx_index / pdx_arg_extreme / pdx_dictionary_encode),
on bit patterns.  tests/test_lookup_golden.py holds it against tests/golden/lookup_golden.npz (Arrow C++ 25.0.0); the GPU tests lean on it for
the shapes the golden file does not hold.  No pyarrow, no GPU."""
import json
import os

import numpy as np

NP_DTYPES = {"i64": np.int64, "u64": np.uint64, "ts": np.int64, "f64": np.float64, "i32": np.int32, "f32": np.float32}
LOOKUP_DTYPES = list(NP_DTYPES)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookup_golden.npz")


def bits(a):
    """the bit image of every element, zero-extended to uint64"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def from_bits(b, dt):
    """inverse of bits() for the dtype name `dt`"""
    t = np.dtype(NP_DTYPES[dt])
    b = np.asarray(b, np.uint64)
    return (b.astype(np.uint32) if t.itemsize == 4 else b).view(t)


def _ok(valid, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid, bool)


def index_in(a, valid, s, svalid, skip_nulls):
    """-> (int32 positions, 0 under a null; bool validity): the position of the FIRST occurrence of a[i]'s bit pattern in s; a null row takes
    the position of s's first null when skip_nulls is false and s holds one."""
    ab, sb = bits(a), bits(s)
    aok, sok = _ok(valid, len(ab)), _ok(svalid, len(sb))
    out, ok = np.zeros(len(ab), np.int32), np.zeros(len(ab), bool)
    spos = np.flatnonzero(sok)
    if len(spos):
        u, first = np.unique(sb[spos], return_index=True)  # (the index of the first occurrence of every sorted unique value)
        j = np.minimum(np.searchsorted(u, ab), len(u) - 1)
        hit = aok & (u[j] == ab)
        out[hit], ok[hit] = spos[first[j[hit]]].astype(np.int32), True
    nulls = np.flatnonzero(~sok)
    if not skip_nulls and len(nulls):
        out[~aok], ok[~aok] = np.int32(nulls[0]), True
    return out, ok


def is_in(a, valid, s, svalid, skip_nulls):
    return index_in(a, valid, s, svalid, skip_nulls)[1]


def index(a, valid, value):
    """the first valid row with a[row] == value under IEEE ==; None (the null scalar), NaN and "not there" give -1"""
    a = np.asarray(a)
    if value is None or len(a) == 0:
        return -1
    with np.errstate(invalid="ignore"):
        hit = _ok(valid, len(a)) & (a == a.dtype.type(value))
    r = np.flatnonzero(hit)
    return int(r[0]) if len(r) else -1


def arg_extreme(a, valid, is_max):
    """index(min(a)) / index(max(a)): NaN is ignored unless every valid value is NaN (then the extreme is NaN and index finds nothing)"""
    a = np.asarray(a)
    take = _ok(valid, len(a)).copy()
    if a.dtype.kind == "f":
        take &= ~np.isnan(a)
    if not take.any():
        return -1
    m = a[take].max() if is_max else a[take].min()
    return int(np.flatnonzero(take & (a == m))[0])


def dictionary_encode(a, valid):
    """-> (int32 codes, 0 under a null; bool validity; dictionary as an array of a's dtype): distinct bit patterns of the valid rows in
    first-occurrence order, a null row gets a null code and takes no slot"""
    a = np.ascontiguousarray(a)
    ok = _ok(valid, len(a))
    rows = np.flatnonzero(ok)
    codes = np.zeros(len(a), np.int32)
    if not len(rows):
        return codes, ok, a[:0].copy()
    u, first, inv = np.unique(bits(a)[rows], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")  # sorted-unique slot -> rank by first occurrence
    rank = np.empty(len(u), np.int32)
    rank[order] = np.arange(len(u), dtype=np.int32)
    codes[rows] = rank[inv.reshape(-1)]
    return codes, ok, a[rows[first[order]]].copy()


class LookupGolden:
    """tests/golden/lookup_golden.npz: `manifest` (JSON: the cases) + arrays.  Values travel as bit images (uint64)."""

    def __init__(self, path=GOLDEN):
        self.z = np.load(path)
        self.cases = json.loads(str(self.z["manifest"]))["cases"]

    def column(self, c, key):
        """-> (values of the case's dtype, validity or None)"""
        v = from_bits(self.z[c[key]], c["dtype"])
        ok = self.z[c[key] + "_ok"] if c[key] + "_ok" in self.z.files else None
        return v, ok

    def arr(self, c, key):
        return self.z[c["name"] + "/" + key]
