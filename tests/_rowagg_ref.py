"""Row-wise aggregates restated in numpy (no pyarrow, no GPU): what Arrow C++ 25's scalar aggregates return for the C cells of every row.

`row_aggregate` is the whole rule set of pdx_row_aggregate (include/pdx/abi.h); tests/test_rowagg_golden.py holds it against
tests/golden/rowagg_golden.npz (written by tools/gen_golden_rowagg.py from live pyarrow), tests/test_gpu_rowagg.py holds the kernel against
both.  Columns are the first axis everywhere: `a` is a (C, n) array, `valid` a (C, n) bool array or None."""
import json
import os

import numpy as np

KINDS = {"sum": 0, "mean": 1, "min": 2, "max": 3, "count": 4, "variance": 5, "stddev": 6, "product": 7, "first": 8, "last": 9, "all": 10, "any": 11,
         "count_null": 13}
NP_T = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "f32": np.float32, "ts": np.int64, "bool": np.bool_}
BITS_T = {"i64": np.uint64, "u64": np.uint64, "f64": np.uint64, "i32": np.uint32, "f32": np.uint32, "ts": np.uint64, "bool": np.bool_}
NUMERIC = ("i64", "u64", "f64", "i32", "f32")
# which kinds a dtype takes (include/pdx/abi.h at pdx_row_aggregate)
ACCEPTED = {
    "i64": ("sum", "mean", "min", "max", "count", "variance", "stddev", "product", "first", "last", "count_null"),
    "f64": ("sum", "mean", "min", "max", "count", "variance", "stddev", "product", "first", "last", "count_null"),
    "u64": ("sum", "mean", "min", "max", "count", "product", "first", "last", "count_null"),
    "i32": ("sum", "mean", "min", "max", "count", "product", "first", "last", "count_null"),
    "f32": ("sum", "mean", "min", "max", "count", "product", "first", "last", "count_null"),
    "ts": ("min", "max", "count", "first", "last", "count_null"),
    "bool": ("count", "all", "any", "count_null"),
}
# a NaN these return is compared as "is NaN": min / max, and the three that go through a GPU multiply / divide / sqrt
NAN_PAYLOAD_FREE = ("min", "max", "product", "variance", "stddev")

_QUIET = np.uint64(0x0008000000000000)
_DEFAULT_NAN = np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0]  # what x86 makes of inf - inf and of 0.0 / 0
_LEVELS = 12


def result_dtype(kind, dt):
    if kind in ("count", "count_null"):
        return "i64"
    if kind in ("all", "any"):
        return "bool"
    if kind in ("min", "max", "first", "last"):
        return dt
    if kind in ("sum", "product"):
        return "f64" if dt[0] == "f" else ("u64" if dt == "u64" else "i64")
    return "f64"


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _quiet(x):
    return (x.view(np.uint64) | _QUIET).view(np.float64)


def _nan_of(first, second):
    return np.where(np.isnan(first), _quiet(first), np.where(np.isnan(second), _quiet(second), _DEFAULT_NAN))


def _add(earlier, later, later_wins):
    """earlier + later; a NaN result carries the bits an x86 add gives it: its first operand's NaN, which is the earlier value inside a
    leaf and the later one in every merge of the tree (pandasarrow_amd/csrc/pairwise.hpp)"""
    with np.errstate(all="ignore"):
        r = earlier + later
    bad = np.isnan(r)
    if bad.any():
        fix = _nan_of(later, earlier) if later_wins else _nan_of(earlier, later)
        r = np.where(bad, fix, r)
    return r


def tree_sum(x, ok):
    """Arrow's pairwise sum of every row of x (C, n) float64 over the cells marked ok, in column order: sequential leaves of at most 16
    values that restart at every run of valid cells, merged through the binary counter, the leftovers folded from the lowest level up"""
    C, n = x.shape
    leaf, cnt = np.zeros(n), np.zeros(n, np.int64)
    s = [np.zeros(n) for _ in range(_LEVELS)]
    mask = np.zeros(n, np.int64)

    def push(rows):
        nonlocal leaf, cnt, mask
        if not rows.any():
            return
        carry, v = rows.copy(), leaf.copy()
        for lv in range(_LEVELS):
            m = _add(s[lv], v, True)
            taken = ((mask >> lv) & 1).astype(bool)
            s[lv] = np.where(carry, np.where(taken, 0.0, m), s[lv])
            v = np.where(carry & taken, m, v)
            carry = carry & taken
        mask = mask + rows
        leaf = np.where(rows, 0.0, leaf)
        cnt = np.where(rows, 0, cnt)

    for c in range(C):
        leaf = np.where(ok[c], _add(leaf, x[c], False), leaf)
        cnt = cnt + ok[c]
        push(np.where(ok[c], cnt == 16, cnt > 0))
    push(cnt > 0)
    root = np.where(mask > 0, np.floor(np.log2(np.maximum(mask, 1))).astype(np.int64), 0)
    r = s[0].copy()
    for lv in range(1, _LEVELS):
        m = _add(s[lv], s[lv - 1], True)
        s[lv] = np.where(lv <= root, m, s[lv])
        r = np.where(lv == root, s[lv], r)
    return r


def _mean_of(total, nv):
    with np.errstate(all="ignore"):
        q = total / np.maximum(nv, 1)
    return np.where(nv == 0, _DEFAULT_NAN, np.where(np.isnan(total), _quiet(total), q))


def row_values(kind, dt, a, valid, ddof=0):
    """-> (values of the result dtype, nv): the value of every row as if it were not null"""
    a = np.asarray(a)
    C, n = a.shape
    ok = np.ones((C, n), bool) if valid is None else np.asarray(valid, bool)
    nv = ok.sum(axis=0).astype(np.int64)
    if kind == "count":
        return nv, nv
    if kind == "count_null":
        return C - nv, nv
    if kind in ("all", "any"):
        b = a.astype(bool)
        return ((b | ~ok).all(axis=0) if kind == "all" else (b & ok).any(axis=0)), nv
    if kind in ("first", "last"):
        out = np.zeros(n, a.dtype)
        have = np.zeros(n, bool)
        for c in (range(C) if kind == "first" else range(C - 1, -1, -1)):
            take = ok[c] & ~have
            out = np.where(take, a[c], out)
            have |= take
        return out, nv
    if kind in ("min", "max"):
        is_f = a.dtype.kind == "f"
        cur_first, cur_last, have = np.zeros(n, a.dtype), np.zeros(n, a.dtype), np.zeros(n, bool)
        quiet_bit = None if not is_f else (np.uint64(1) << np.uint64(51) if a.dtype == np.float64 else np.uint32(1) << np.uint32(22))
        for c in range(C):
            use = ok[c] & ~np.isnan(a[c]) if is_f else ok[c]
            if is_f:  # a quiet NaN takes no part; a SIGNALLING one makes the running extreme NaN, and the next number replaces that (glibc's fmin)
                have &= ~(ok[c] & np.isnan(a[c]) & ((bits(a[c]) & quiet_bit) == 0))
            with np.errstate(all="ignore"):
                better = (a[c] < cur_first) if kind == "min" else (a[c] > cur_first)
                not_worse = ~(a[c] > cur_last) if kind == "min" else ~(a[c] < cur_last)
            cur_first = np.where(use & (~have | better), a[c], cur_first)
            cur_last = np.where(use & (~have | not_worse), a[c], cur_last)
            have |= use
        # of values that compare equal (0.0 / -0.0) the first wins, except float64's max in a row with nulls: the last (float32's keeps the first)
        out = np.where(nv < C, cur_last, cur_first) if kind == "max" and a.dtype == np.float64 else cur_first
        if is_f:
            out = np.where(have, out, np.nan).astype(a.dtype)
        return out, nv
    if kind in ("sum", "product") and a.dtype.kind in "iu":
        acc = np.full(n, 1 if kind == "product" else 0, np.uint64)
        wide = a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)
        with np.errstate(all="ignore"):
            for c in range(C):
                acc = np.where(ok[c], acc * wide[c] if kind == "product" else acc + wide[c], acc)
        return (acc if a.dtype == np.uint64 else acc.view(np.int64)), nv
    x = a.astype(np.float64)
    if kind == "product":
        acc = np.ones(n)
        with np.errstate(all="ignore"):
            for c in range(C):
                acc = np.where(ok[c], acc * x[c], acc)
        return acc, nv
    if kind in ("variance", "stddev") and a.dtype.kind in "iu":  # Arrow's first pass sums integers exactly (int128) and rounds once
        total = np.array([float(sum(int(a[c, r]) for c in range(C) if ok[c, r])) for r in range(n)], np.float64)
    else:
        total = tree_sum(x, ok)
    if kind == "sum":
        return total, nv
    mean = _mean_of(total, nv)
    if kind == "mean":
        return mean, nv
    with np.errstate(all="ignore"):
        d = x - np.where(nv == 0, 0.0, mean)[None, :]
        m2 = tree_sum(d * d, ok)
        var = np.where(nv > ddof, m2 / np.maximum(nv - ddof, 1), 0.0)
        return (var if kind == "variance" else np.sqrt(var)), nv


def row_validity(kind, a, valid, nv, skip_nulls, min_count, ddof=0):
    a = np.asarray(a)
    C, n = a.shape
    if kind in ("count", "count_null"):
        return np.ones(n, bool)
    ok = np.ones((C, n), bool) if valid is None else np.asarray(valid, bool)
    enough = nv >= min_count
    full = nv == C
    if kind in ("first", "last"):
        edge = ok[0] if kind == "first" else ok[C - 1]
        return enough & (nv > 0) & (edge if not skip_nulls else True)
    if kind in ("all", "any"):
        b = a.astype(bool)
        decided = (ok & ~b).any(axis=0) if kind == "all" else (ok & b).any(axis=0)
        return enough & (True if skip_nulls else (full | decided))
    r = enough & (True if skip_nulls else full)
    if kind in ("min", "max"):
        r = r & (nv > 0)
    if kind in ("variance", "stddev"):
        r = r & (nv > ddof)
    return r


def row_aggregate(kind, dt, a, valid, skip_nulls=True, min_count=0, ddof=0):
    """-> (values, valid): pdx_row_aggregate over the columns a[0], a[1], ..."""
    vals, nv = row_values(kind, dt, a, valid, ddof)
    return vals, row_validity(kind, a, valid, nv, skip_nulls, min_count, ddof)


def same_result(kind, got, got_valid, want, want_valid):
    """bit for bit on the non-null rows; a NaN of NAN_PAYLOAD_FREE kinds as "is NaN" -> list of offending rows"""
    got_valid = np.ones(len(want), bool) if got_valid is None else np.asarray(got_valid, bool)
    bad = list(np.flatnonzero(got_valid != want_valid))
    g, w = bits(np.asarray(got)), bits(np.asarray(want))
    assert g.dtype == w.dtype, (g.dtype, w.dtype)
    differ = want_valid & (g != w)
    if kind in NAN_PAYLOAD_FREE and np.asarray(want).dtype.kind == "f":
        differ &= ~(np.isnan(np.asarray(got)) & np.isnan(np.asarray(want)))
    return bad + list(np.flatnonzero(differ))


class RowaggGolden:
    """tests/golden/rowagg_golden.npz: per case a (C, n) matrix `a`, its validity, and per run (kind, skip_nulls, min_count, ddof) Arrow's
    result column as bits with its validity"""

    def __init__(self, path=None):
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowagg_golden.npz")
        self.z = np.load(path)
        m = json.loads(str(self.z["manifest"]))
        self.cases, self.index, self.arrow_version = m["cases"], m["arrays"], m["arrow_version"]

    def get(self, key):
        blob, start, count = self.index[key]
        return self.z[blob][start:start + count]

    def inputs(self, case):
        C, n, dt = case["C"], case["n"], case["dtype"]
        raw = self.get(case["name"] + "/a").reshape(C, n)
        a = raw if dt == "bool" else raw.view(NP_T[dt])
        return a, self.get(case["name"] + "/valid").reshape(C, n)

    def expected(self, case, run):
        rdt = result_dtype(run["kind"], case["dtype"])
        raw = self.get(f"{case['name']}/{run['key']}/out")
        return (raw if rdt == "bool" else raw.view(NP_T[rdt])), self.get(f"{case['name']}/{run['key']}/ok")
