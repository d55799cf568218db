"""numpy restatement of pdx_select_k and pdx_partition_nth (include/pdx/abi.h): a stable argsort on the order-preserving key image with
classes (number < NaN < null in both orders), sliced to k; the deterministic five-part layout of partition_nth and a checker of its contract.
tests/test_topk_golden.py holds select_k against tests/golden/topk_golden.npz (Arrow C++ 25.0.0: array_sort_indices(order)[:k]); the GPU tests
lean on it for the shapes the golden file does not hold.  No pyarrow, no GPU."""
import json
import os

import numpy as np

NP_DTYPES = {"i64": np.int64, "u64": np.uint64, "ts": np.int64, "f64": np.float64, "i32": np.int32, "f32": np.float32}
TOPK_DTYPES = list(NP_DTYPES)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_golden.npz")


def bits(a):
    """the bit image of every element, zero-extended to uint64"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def from_bits(b, dt):
    t = np.dtype(NP_DTYPES[dt])
    b = np.asarray(b, np.uint64)
    return (b.astype(np.uint32) if t.itemsize == 4 else b).view(t)


def keys_and_classes(a, valid):
    """-> (uint64 key whose unsigned order is the value's order, 0 outside class 0; class: 0 number, 1 NaN, 2 null).  -0.0 and 0.0 share
    a key."""
    a = np.ascontiguousarray(a)
    n, w = len(a), a.dtype.itemsize * 8
    sign = np.uint64(1) << np.uint64(w - 1)
    full = np.uint64((1 << w) - 1)
    u = bits(a)
    cls = np.zeros(n, np.int8)
    if a.dtype.kind == "f":
        cls[np.isnan(a)] = 1
        u = np.where(a == 0, np.uint64(0), u)
        key = np.where((u & sign) != 0, ~u & full, u | sign)
    elif a.dtype.kind == "i":
        key = u ^ sign
    else:
        key = u
    if valid is not None:
        cls[~np.asarray(valid, bool)] = 2
    return np.where(cls == 0, key, np.uint64(0)), cls


def argsort(a, valid, ascending=True):
    """pdx_argsort: stable in both orders, NaN rows behind the numbers, null rows behind the NaNs"""
    key, cls = keys_and_classes(a, valid)
    if not ascending:
        key = np.where(cls == 0, ~key, np.uint64(0))
    return np.lexsort((key, cls)).astype(np.uint64)  # (lexsort is stable; the last key is the primary one)


def select_k(a, valid, k, ascending=True):
    return argsort(a, valid, ascending)[: max(k, 0)]


def counts(a, valid):
    """-> (numbers, NaN rows, null rows)"""
    _, cls = keys_and_classes(a, valid)
    return int((cls == 0).sum()), int((cls == 1).sum()), int((cls == 2).sum())


def sorted_number_keys(a, valid):
    """the keys of the numbers in ascending order (what partition_nth and its checker look ranks up in; callers with many pivots share it)"""
    key, cls = keys_and_classes(a, valid)
    return np.sort(key[cls == 0])


def partition_nth(a, valid, pivot, sorted_keys=None):
    """the layout pdx_partition_nth writes: with T the key at rank min(pivot, numbers - 1), rows with key < T, == T, > T, NaN rows, null
    rows, each part in row order"""
    key, cls = keys_and_classes(a, valid)
    rows = np.arange(len(key), dtype=np.uint64)
    num = cls == 0
    m = int(num.sum())
    parts = []
    if m:
        t = (sorted_number_keys(a, valid) if sorted_keys is None else sorted_keys)[min(pivot, m - 1)]
        parts += [rows[num & (key < t)], rows[num & (key == t)], rows[num & (key > t)]]
    parts += [rows[cls == 1], rows[cls == 2]]
    return np.concatenate(parts) if parts else rows


def check_partition(a, valid, pivot, idx, sorted_keys=None):
    """asserts the contract of pdx_partition_nth on the indices `idx`"""
    key, cls = keys_and_classes(a, valid)
    n = len(key)
    idx = np.asarray(idx)
    assert idx.dtype == np.uint64 and len(idx) == n
    assert np.array_equal(np.sort(idx), np.arange(n, dtype=np.uint64)), "not a permutation"
    m, nan, _ = counts(a, valid)
    p = min(pivot, m)
    ix = idx.astype(np.int64)
    assert (cls[ix[:m]] == 0).all() and (cls[ix[m:m + nan]] == 1).all() and (cls[ix[m + nan:]] == 2).all(), "classes out of place"
    if 0 < p < m:
        assert key[ix[:p]].max() <= key[ix[p:m]].min(), "a number in front of the pivot is larger than one behind it"
    if pivot < m:
        want = (sorted_number_keys(a, valid) if sorted_keys is None else sorted_keys)[pivot]  # (the key pdx_argsort(col, 1) puts at that place)
        assert key[ix[pivot]] == want, "the pivot's place does not hold the value of that rank"


class TopkGolden:
    """tests/golden/topk_golden.npz: `manifest` (JSON: the cases) + arrays.  Values travel as bit images (uint64).  A case holds one column
    and, per order, the full array_sort_indices; its `ks` are the prefix lengths the issue lists."""

    def __init__(self, path=GOLDEN):
        self.z = np.load(path)
        m = json.loads(str(self.z["manifest"]))
        self.cases, self.arrow = m["cases"], m["arrow"]

    def column(self, c):
        v = from_bits(self.z[c["name"] + "/a"], c["dtype"])
        ok = self.z[c["name"] + "/a_ok"] if c["name"] + "/a_ok" in self.z.files else None
        return v, ok

    def want(self, c, ascending, k):
        """array_sort_indices(order)[:k]"""
        return self.z[c["name"] + ("/asc" if ascending else "/desc")][:k].astype(np.uint64)
