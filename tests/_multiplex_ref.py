"""Selection / multiplexing and null-handling calls restated in numpy (no pyarrow, no GPU): what Arrow C++ 25's `coalesce`,
`min_element_wise` / `max_element_wise` (and the reference's clip nesting of them), `replace_with_mask`, `indices_nonzero` and the row
mask behind `drop_null` return.

These are the rule sets of pdx_coalesce, pdx_element_wise_minmax / pdx_clip, pdx_replace_with_mask, pdx_indices_nonzero and
pdx_all_valid_mask (include/pdx/abi.h).  tests/test_multiplex_golden.py holds them against tests/golden/multiplex_golden.npz (written by
tools/gen_golden_multiplex.py from live pyarrow), tests/test_gpu_multiplex.py holds the kernels against both.  Columns are the first axis:
`a` is a (C, n) array, `valid` a (C, n) bool array or None."""
import json
import os

import numpy as np

NP_T = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "f32": np.float32, "ts": np.int64, "bool": np.bool_}
ALL_DTYPES = tuple(NP_T)
MINMAX_DTYPES = ("i64", "u64", "f64", "i32", "f32", "ts")
NONZERO_DTYPES = ("i64", "u64", "f64", "i32", "f32", "bool")
ARROW_NAME = {"i64": "int64", "u64": "uint64", "f64": "double", "i32": "int32", "f32": "float", "ts": "timestamp[ns]", "bool": "bool"}


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _valid(valid, shape):
    return np.ones(shape, bool) if valid is None else np.asarray(valid, bool)


# ---------------------------------------------------------------- coalesce
def coalesce(a, valid):
    """-> (values, ok): per row the first valid cell in column order, bits untouched; null (value 0) when the row has none"""
    a = np.asarray(a)
    C, n = a.shape
    ok = _valid(valid, (C, n))
    out, have = np.zeros(n, a.dtype), np.zeros(n, bool)
    for c in range(C):
        take = ok[c] & ~have
        out = np.where(take, a[c], out)
        have |= take
    return out, have


# ---------------------------------------------------------------- min_element_wise / max_element_wise
def _signalling(x):
    if x.dtype == np.float64:
        return np.isnan(x) & ((bits(x) & np.uint64(1 << 51)) == 0)
    return np.isnan(x) & ((bits(x) & np.uint32(1 << 22)) == 0)


def _fold(is_max, acc, v, tie_later=False):
    """Arrow's Call(acc, v): std::min / std::max of integers; of floats the C library's fmin / fmax as they behave under Arrow 25 on x86-64:
    a signalling NaN on either side gives NaN; otherwise a NaN loses to the other side; of two values that compare equal (0.0 / -0.0)
    the accumulator (the earlier operand) stays unless `tie_later` says that the incoming value (the later one) does"""
    if acc.dtype.kind != "f":
        return np.maximum(acc, v) if is_max else np.minimum(acc, v)
    with np.errstate(all="ignore"):
        better = (v > acc) if is_max else (v < acc)
        worse = (v < acc) if is_max else (v > acc)
    r = np.where(better, v, np.where(worse, acc, np.where(tie_later, v, acc)))
    r = np.where(np.isnan(acc), v, np.where(np.isnan(v), acc, r))
    return np.where(_signalling(acc) | _signalling(v), np.array(np.nan, acc.dtype), r).astype(acc.dtype)


def _block_all_valid(ok):
    """per row: is every row of its 64-row block (counted from the array's first row; the last block may be shorter) valid?"""
    n = len(ok)
    out = np.zeros(n, bool)
    for b in range(0, n, 64):
        out[b:b + 64] = ok[b:b + 64].all()
    return out


def element_wise_minmax(is_max, operands, skip_nulls, n=None):
    """operands: [(values, valid | None, is_scalar)], values of length n (length 1 for a scalar).  Arrow folds the scalars first, in
    their order, then the arrays in theirs, each valid cell through Call(accumulator, cell); the accumulator starts as a quiet NaN
    (floats) or is taken from the first valid cell.  The first valid scalar is taken as it is (a signalling NaN stays signalling).
    Ties (0.0 / -0.0): the accumulator stays, except that a float32 ARRAY cell replaces it when the 64-row block of that array around the
    cell has no null (Arrow's loop over such a block is compiled differently from its loop over a block with nulls).
    -> (values, ok): ok = any operand valid (skip_nulls) / every operand valid."""
    arrays = [(np.asarray(v), ok) for v, ok, sc in operands if not sc]
    scalars = [(np.asarray(v), ok) for v, ok, sc in operands if sc]
    if n is None:
        n = len(arrays[0][0]) if arrays else 1
    dt = np.asarray(operands[0][0]).dtype
    is_f = dt.kind == "f"
    acc = np.full(n, np.nan if is_f else 0, dt)
    have = np.zeros(n, bool)
    every = np.ones(n, bool)
    first_scalar = True
    for v, ok in scalars:
        okb = bool(_valid(ok, (1,))[0])
        every &= okb
        if not okb:
            continue
        vv = np.full(n, v[0], dt)
        acc = vv if first_scalar else _fold(is_max, acc, vv)
        first_scalar = False
        have[:] = True
    for v, ok in arrays:
        okb = _valid(ok, (n,))
        every &= okb
        later = _block_all_valid(okb) if dt == np.float32 else False
        folded = _fold(is_max, acc, v, later) if is_f else np.where(have, _fold(is_max, acc, v), v)
        acc = np.where(okb, folded, acc)
        have |= okb
    good = have if skip_nulls else every
    return np.where(good, acc, np.zeros(1, dt)), good


def clip(x, x_valid, lo, lo_valid, hi, hi_valid, skip_nulls):
    """the reference's Series::clip: max_element_wise(min_element_wise(x, hi), lo), lo / hi scalars (values of length 1), the options
    applied by each level on its own"""
    inner, inner_ok = element_wise_minmax(False, [(x, x_valid, False), (hi, hi_valid, True)], skip_nulls)
    return element_wise_minmax(True, [(inner, inner_ok, False), (lo, lo_valid, True)], skip_nulls)


def same_minmax(got, got_valid, want, want_valid):
    """bit for bit on the non-null rows, except that a NaN result is compared as "is NaN" (the payload rule of min / max)
    -> list of offending rows"""
    got_valid = np.ones(len(want), bool) if got_valid is None else np.asarray(got_valid, bool)
    bad = list(np.flatnonzero(got_valid != want_valid))
    g, w = bits(np.asarray(got)), bits(np.asarray(want))
    assert g.dtype == w.dtype, (g.dtype, w.dtype)
    differ = want_valid & (g != w)
    if np.asarray(want).dtype.kind == "f":
        differ &= ~(np.isnan(np.asarray(got)) & np.isnan(np.asarray(want)))
    return bad + list(np.flatnonzero(differ))


def same_bits(got, got_valid, want, want_valid):
    """bit for bit on the non-null rows, validity everywhere -> list of offending rows"""
    got_valid = np.ones(len(want), bool) if got_valid is None else np.asarray(got_valid, bool)
    bad = list(np.flatnonzero(got_valid != want_valid))
    g, w = bits(np.asarray(got)), bits(np.asarray(want))
    assert g.dtype == w.dtype, (g.dtype, w.dtype)
    return bad + list(np.flatnonzero(want_valid & (g != w)))


# ---------------------------------------------------------------- replace_with_mask
class Invalid(ValueError):
    """Arrow's Status::Invalid"""


def replace_with_mask(a, a_valid, mask, mask_valid, repl, repl_valid):
    """-> (values, ok).  Row i with a valid true mask takes repl[k], k = the valid true mask rows before i (null where repl[k] is);
    a null mask row is null; every other row keeps a[i]."""
    a, mask, repl = np.asarray(a), np.asarray(mask, bool), np.asarray(repl)
    n = len(a)
    if len(mask) != n:
        raise Invalid(f"Mask must be of same length as array (expected {n} items but got {len(mask)} items)")
    mok = _valid(mask_valid, (n,))
    hit = mask & mok
    need = int(hit.sum())
    if len(repl) < need:
        raise Invalid(f"Replacement array must be of appropriate length (expected {need} items but got {len(repl)} items)")
    k = np.cumsum(hit) - hit
    rok = _valid(repl_valid, (len(repl),))
    out, ok = a.copy(), _valid(a_valid, (n,)).copy()
    out[hit] = repl[k[hit]]
    ok[hit] = rok[k[hit]]
    ok &= mok
    return np.where(ok, out, np.zeros(1, a.dtype)), ok


# ---------------------------------------------------------------- indices_nonzero, the drop_null row mask
def indices_nonzero(a, a_valid):
    """uint64 ascending rows that are valid and not zero: NaN counts, -0.0 does not; a bool counts when true"""
    a = np.asarray(a)
    return np.flatnonzero(_valid(a_valid, a.shape) & (a != 0)).astype(np.uint64)


def all_valid_mask(valids, n):
    """row i is kept by drop_null when every column is valid there; valids: one bool array or None per column"""
    keep = np.ones(n, bool)
    for v in valids:
        if v is not None:
            keep &= np.asarray(v, bool)
    return keep


def drop_na(cols, valids):
    """-> ([values], [valid]) of the rows all_valid_mask keeps"""
    keep = all_valid_mask(valids, len(cols[0]))
    return [np.asarray(c)[keep] for c in cols], keep


# ---------------------------------------------------------------- the golden file
class MultiplexGolden:
    """tests/golden/multiplex_golden.npz: a manifest of cases per function; every array a case names lives in one of a few typed blobs"""

    def __init__(self, path=None):
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiplex_golden.npz")
        self.z = np.load(path)
        m = json.loads(str(self.z["manifest"]))
        self.cases, self.index, self.arrow_version = m["cases"], m["arrays"], m["arrow_version"]

    def get(self, key, dt=None):
        blob, start, count = self.index[key]
        raw = self.z[blob][start:start + count]
        return raw if dt is None or dt == "bool" else raw.view(NP_T[dt])

    def of(self, fn):
        return [c for c in self.cases if c["fn"] == fn]
