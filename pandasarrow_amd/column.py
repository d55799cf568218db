"""Device-resident Arrow-layout columns and the thin Python calls into the C ABI.

A ``Column`` owns torch CUDA tensors (PyTorch is used only for device memory and streams): a contiguous
values buffer, an optional validity bitmap (1 bit/row, LSB first) and an element ``offset`` -- the fields
of ``arrow::ArrayData`` the reference's kernels read (src/ndframe.h:140-157).  Every operation below is one
call through ``libpdx_hip.so``; nothing is computed in Python/torch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

_TORCH_DT = {L.INT64: torch.int64, L.FLOAT64: torch.float64, L.UINT64: torch.int64, L.TIMESTAMP_NS: torch.int64, L.BOOL: torch.uint8,
             L.INT32: torch.int32, L.FLOAT32: torch.float32}
_HOST_DT = {L.FLOAT64: np.float64, L.UINT64: np.uint64, L.INT32: np.int32, L.FLOAT32: np.float32}  # (default: int64)


def _device():
    if not torch.cuda.is_available():
        raise L.PdxError(L.DEVICE, "no GPU visible: pandasarrow_amd runs on MI355X (gfx950) only; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bitmap_bytes(n):
    return (n + 7) // 8 + 16  # slack so kernels may store whole 64-bit words


def pack_bits_host(b, offset=0):
    b = np.asarray(b, dtype=bool)
    if offset:
        b = np.concatenate([np.zeros(offset, bool), b])
    bits = np.packbits(b, bitorder="little")
    return np.concatenate([bits, np.zeros(16, np.uint8)])


def unpack_bits_host(bits, n, offset=0):
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[offset:offset + n].astype(bool)


class Column:
    """One Arrow-layout column in HBM."""

    __slots__ = ("dtype", "length", "offset", "values", "validity", "null_count")

    def __init__(self, dtype, length, values, validity=None, offset=0, null_count=None):
        self.dtype = dtype
        self.length = int(length)
        self.offset = int(offset)
        self.values = values      # torch tensor (int64/float64, or uint8 bitmap for BOOL)
        self.validity = validity  # torch uint8 bitmap or None
        self.null_count = (0 if validity is None else -1) if null_count is None else int(null_count)

    # ---- construction -------------------------------------------------------------------------------------
    @staticmethod
    def from_numpy(a, valid=None, dtype=None, offset=0):
        """Host -> device.  ``offset`` prepends junk rows to exercise Arrow slice offsets.  A float32 array stays FLOAT32; an int32
        array widens to INT64 unless ``dtype=L.INT32`` asks for the native width."""
        a = np.asarray(a)
        dev = _device()
        if dtype is None:
            if a.dtype == np.bool_:
                dtype = L.BOOL
            elif a.dtype == np.float64:
                dtype = L.FLOAT64
            elif a.dtype == np.float32:
                dtype = L.FLOAT32
            elif a.dtype == np.uint64:
                dtype = L.UINT64
            elif a.dtype.kind in "iu":
                dtype = L.INT64
            elif a.dtype.kind == "M":
                dtype = L.TIMESTAMP_NS
                a = a.astype("datetime64[ns]").astype(np.int64)
            else:
                raise L.PdxError(L.INVALID, f"unsupported numpy dtype {a.dtype}")
        n = len(a)
        if dtype == L.BOOL:
            vals = torch.from_numpy(pack_bits_host(a.astype(bool), offset)).to(dev)
        else:
            host = a.astype(_HOST_DT.get(dtype, np.int64))
            if offset:
                host = np.concatenate([np.full(offset, 77, host.dtype), host])
            view = {L.FLOAT64: np.float64, L.INT32: np.int32, L.FLOAT32: np.float32}.get(dtype, np.int64)
            vals = torch.from_numpy(np.ascontiguousarray(host).view(view).copy()).to(dev)
        vbits = None
        if valid is not None:
            vbits = torch.from_numpy(pack_bits_host(valid, offset)).to(dev)
        return Column(dtype, n, vals, vbits, offset)

    @staticmethod
    def empty(dtype, n, with_validity=False):
        dev = _device()
        if dtype == L.BOOL:
            vals = torch.zeros(_bitmap_bytes(n), dtype=torch.uint8, device=dev)
        else:
            vals = torch.empty(max(n, 1), dtype=_TORCH_DT[dtype], device=dev)
        vb = torch.zeros(_bitmap_bytes(n), dtype=torch.uint8, device=dev) if with_validity else None
        return Column(dtype, n, vals, vb)

    # ---- host views ---------------------------------------------------------------------------------------
    def to_numpy(self):
        """-> (values ndarray, valid bool ndarray | None)."""
        torch.cuda.current_stream().synchronize()
        if self.dtype == L.BOOL:
            vals = unpack_bits_host(self.values.cpu().numpy(), self.length, self.offset)
        else:
            host = self.values[self.offset:self.offset + self.length].cpu().numpy()
            vals = host.view(np.uint64) if self.dtype == L.UINT64 else host
        valid = None
        if self.validity is not None:
            valid = unpack_bits_host(self.validity.cpu().numpy(), self.length, self.offset)
        return vals, valid

    # ---- ABI structs --------------------------------------------------------------------------------------
    def c(self):
        return L.PdxColumn(self.dtype, 0, self.length, self.offset, self.null_count,
                           None if self.validity is None else self.validity.data_ptr(), self.values.data_ptr())

    def mut(self):
        return L.PdxMutColumn(self.dtype, 0, self.length, -1, None if self.validity is None else self.validity.data_ptr(),
                              self.values.data_ptr())

    def _adopt(self, m):
        self.length = int(m.length)
        self.null_count = int(m.null_count)
        return self

    def has_nulls(self):
        return self.validity is not None and self.null_count != 0

    def slice(self, start, length):
        return Column(self.dtype, length, self.values, self.validity, self.offset + start, None if self.validity is not None else 0)


def _scalar_column(x, like_float):
    if isinstance(x, Column):
        return x
    if x is None:
        return Column.from_numpy(np.zeros(1, np.float64 if like_float else np.int64), valid=np.zeros(1, bool))
    if isinstance(x, (float, np.floating)):
        return Column.from_numpy(np.array([x], np.float64))
    return Column.from_numpy(np.array([x], np.int64))


_NARROW = (L.INT32, L.FLOAT32)


def promote_dtype(da, db):
    """Arrow's implicit numeric promotion (include/pdx/abi.h): float64 > float32 > int64 > int32."""
    for dt in (L.FLOAT64, L.FLOAT32, L.INT64):
        if dt in (da, db):
            return dt
    return L.INT32 if (da, db) == (L.INT32, L.INT32) else L.INT64


def _promoted(a, b):
    if a.dtype in _NARROW or b.dtype in _NARROW:
        return promote_dtype(a.dtype, b.dtype)
    return L.FLOAT64 if L.FLOAT64 in (a.dtype, b.dtype) else L.INT64


# ---------------------------------------------------------------- element-wise
def _scalar_sides(a, b, scalar):
    """-> (a column, b column, pdx_scalar_side, result length).  A non-Column operand on either side is a scalar: on the right
    `series op 2` (src/series.cpp:25-28), on the left `2 op series` (Scalar::operator op(Series), src/scalar.cpp:24-56)."""
    side = L.SCALAR_RHS if scalar is True else int(scalar)
    if not isinstance(a, Column):
        a, side = _scalar_column(a, b.dtype == L.FLOAT64), L.SCALAR_LHS
    elif not isinstance(b, Column):
        b, side = _scalar_column(b, a.dtype == L.FLOAT64), L.SCALAR_RHS
    return a, b, side, (b.length if side == L.SCALAR_LHS else a.length)


def binary(op, a, b, scalar=False) -> Column:
    lib = L.load()
    a, b, side, n = _scalar_sides(a, b, scalar)
    out = Column.empty(_promoted(a, b), n, with_validity=a.has_nulls() or b.has_nulls())
    ca, cb, m = a.c(), b.c(), out.mut()
    L.check(lib.pdx_binary(op, C.byref(ca), C.byref(cb), side, C.byref(m), _stream()))
    return out._adopt(m)


def compare(op, a, b, scalar=False) -> Column:
    lib = L.load()
    a, b, side, n = _scalar_sides(a, b, scalar)
    out = Column.empty(L.BOOL, n, with_validity=a.has_nulls() or b.has_nulls())
    ca, cb, m = a.c(), b.c(), out.mut()
    L.check(lib.pdx_compare(op, C.byref(ca), C.byref(cb), side, C.byref(m), _stream()))
    return out._adopt(m)


def logical(op, a: Column, b: Column) -> Column:
    lib = L.load()
    out = Column.empty(L.BOOL, a.length, with_validity=a.has_nulls() or b.has_nulls())
    ca, cb, m = a.c(), b.c(), out.mut()
    L.check(lib.pdx_logical(op, C.byref(ca), C.byref(cb), C.byref(m), _stream()))
    return out._adopt(m)


def invert(a: Column) -> Column:
    lib = L.load()
    out = Column.empty(L.BOOL, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(lib.pdx_invert(C.byref(ca), C.byref(m), _stream()))
    return out._adopt(m)


def null_column(dtype, n) -> Column:
    """n nulls of `dtype` (device-side zeros: values and validity)."""
    nbytes = _bitmap_bytes(n)
    vdt = _TORCH_DT.get(dtype, torch.int64)
    vals = torch.zeros(max(nbytes if dtype == L.BOOL else n, 1), dtype=vdt, device=_device())
    return Column(dtype, n, vals, torch.zeros(nbytes, dtype=torch.uint8, device=_device()), 0, n)


def if_else(cond: Column, a, b, b_scalar=False) -> Column:
    """cond ? a : b (pdx_if_else); a or b may be a python scalar / None (null scalar), or b a length-1 Column broadcast as the scalar
    (b_scalar=True)."""
    lib = L.load()
    like_float = any(isinstance(x, Column) and x.dtype == L.FLOAT64 for x in (a, b)) or any(isinstance(x, float) for x in (a, b))
    side = L.SCALAR_RHS if b_scalar else L.SCALAR_NONE
    if not isinstance(b, Column):
        b, side = _scalar_column(b, like_float), L.SCALAR_RHS
    elif not isinstance(a, Column):
        a, side = _scalar_column(a, like_float), L.SCALAR_LHS
    out = Column.empty(_promoted(a, b), cond.length, with_validity=cond.has_nulls() or a.has_nulls() or b.has_nulls())
    cc, ca, cb, m = cond.c(), a.c(), b.c(), out.mut()
    L.check(lib.pdx_if_else(C.byref(cc), C.byref(ca), C.byref(cb), side, C.byref(m), _stream()))
    return out._adopt(m)


def unary(op, a: Column) -> Column:
    """negate / abs / sign / sqrt / exp / bit_wise_not of one column (pdx_unary)."""
    lib = L.load()
    to_f64 = op in (L.SQRT, L.EXP)
    if a.dtype == L.FLOAT32:
        out_dt = L.FLOAT32
    elif a.dtype == L.INT32:
        out_dt = L.FLOAT64 if to_f64 else L.INT64 if op == L.SIGN else L.INT32
    else:
        out_dt = L.FLOAT64 if to_f64 else (L.INT64 if (op == L.SIGN and a.dtype != L.FLOAT64) else a.dtype)
    out = Column.empty(out_dt, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(lib.pdx_unary(int(op), C.byref(ca), C.byref(m), _stream()))
    return out._adopt(m)


def cast_f64(a: Column, checked=True) -> Column:
    """Cast(int64 -> float64) (pdx_cast_f64): checked = Arrow's safe cast (pd::concat's promotion), unchecked = static_cast per value."""
    out = Column.empty(L.FLOAT64, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(L.load().pdx_cast_f64(C.byref(ca), int(bool(checked)), C.byref(m), _stream()))
    return out._adopt(m)


def cast(a: Column, dtype) -> Column:
    """Arrow's safe Cast between numeric dtypes (pdx_cast): int32 -> int64 / float64, float32 -> float64, int32 / int64 -> float32
    (checked: +-2^24), int64 -> float64 (checked: +-2^53)."""
    out = Column.empty(dtype, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(L.load().pdx_cast(C.byref(ca), C.byref(m), _stream()))
    return out._adopt(m)


def power(a: Column, exponent: float) -> Column:
    lib = L.load()
    out = Column.empty(L.FLOAT64, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(lib.pdx_power(C.byref(ca), float(exponent), C.byref(m), _stream()))
    return out._adopt(m)


# ---------------------------------------------------------------- cumulative scans, fill_null, shift
def cumulative(op, a: Column, start, skip_nulls=True) -> Column:
    """cumulative_sum / prod / max / min (pdx_cumulative): the input's dtype; `start` goes through Arrow's safe cast to it."""
    out = Column.empty(a.dtype, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(L.load().pdx_cumulative(int(op), C.byref(ca), float(start), int(bool(skip_nulls)), C.byref(m), _stream()))
    return out._adopt(m)


def fill_null(a: Column, backward=False) -> Column:
    """fill_null_forward / fill_null_backward (pdx_fill_null)."""
    out = Column.empty(a.dtype, a.length, with_validity=a.has_nulls())
    ca, m = a.c(), out.mut()
    L.check(L.load().pdx_fill_null(int(bool(backward)), C.byref(ca), C.byref(m), _stream()))
    return out._adopt(m)


def shift(a: Column, periods, fill=None) -> Column:
    """out[i] = a[i - periods]; rows without a source take `fill` (None: null) (pdx_shift)."""
    s = None
    if fill is not None:
        s = L.PdxScalar(a.dtype, 1)
        if a.dtype in (L.FLOAT64, L.FLOAT32):
            s.v.f64 = float(fill)
        elif a.dtype == L.UINT64:
            s.v.u64 = int(fill)
        else:
            s.v.i64 = int(fill)
    out = Column.empty(a.dtype, a.length, with_validity=a.has_nulls() or (fill is None and periods != 0 and a.length > 0))
    ca, m = a.c(), out.mut()
    L.check(L.load().pdx_shift(C.byref(ca), int(periods), None if s is None else C.byref(s), C.byref(m), _stream()))
    return out._adopt(m)


# ---------------------------------------------------------------- aggregates
def aggregate(kind, a: Column):
    """-> (python value | None, count)."""
    lib = L.load()
    s = L.PdxScalar()
    ca = a.c()
    L.check(lib.pdx_aggregate(kind, C.byref(ca), C.byref(s), _stream()))
    if not s.is_valid:
        return None, int(s.count)
    if s.dtype in (L.FLOAT64, L.FLOAT32):  # (a float32 result is held widened)
        return float(s.v.f64), int(s.count)
    return int(s.v.i64), int(s.count)


def row_result_dtype(kind, dtype):
    """the dtype pdx_row_aggregate writes for `kind` over columns of `dtype` (include/pdx/abi.h)"""
    if kind in (L.AGG_COUNT, L.AGG_COUNT_NULL):
        return L.INT64
    if kind in (L.AGG_ALL, L.AGG_ANY):
        return L.BOOL
    if kind in (L.AGG_MIN, L.AGG_MAX, L.AGG_FIRST, L.AGG_LAST):
        return dtype
    if kind in (L.AGG_SUM, L.AGG_PRODUCT):
        return L.FLOAT64 if dtype in (L.FLOAT64, L.FLOAT32) else (L.UINT64 if dtype == L.UINT64 else L.INT64)
    return L.FLOAT64


def row_aggregate(kind, cols, skip_nulls=True, min_count=0, ddof=0) -> Column:
    """Arrow's scalar aggregate `kind` over the cells of every row of `cols` (one dtype, one length): one kernel launch (pdx_row_aggregate)."""
    if not cols:
        raise L.PdxError(L.INVALID, "row_aggregate: at least one column is required")
    out = Column.empty(row_result_dtype(kind, cols[0].dtype), cols[0].length, with_validity=kind not in (L.AGG_COUNT, L.AGG_COUNT_NULL))
    m = out.mut()
    L.check(L.load().pdx_row_aggregate(int(kind), _col_array(cols), len(cols), int(bool(skip_nulls)), int(min_count), int(ddof), C.byref(m), _stream()))
    return out._adopt(m)


INTERPOLATIONS = {"linear": L.INTERP_LINEAR, "lower": L.INTERP_LOWER, "higher": L.INTERP_HIGHER, "nearest": L.INTERP_NEAREST,
                  "midpoint": L.INTERP_MIDPOINT}


def interpolation_code(interpolation) -> int:
    if isinstance(interpolation, str):
        if interpolation not in INTERPOLATIONS:
            raise L.PdxError(L.INVALID, f"unknown interpolation {interpolation!r}")
        return INTERPOLATIONS[interpolation]
    return int(interpolation)


def quantile(a: Column, qs, interpolation=L.INTERP_LINEAR, skip_nulls=True, min_count=0):
    """Exact quantiles of one column; the ranks of all of them are located by one histogram read of it (pdx_quantile).  -> list of (python value | None, count)."""
    qs = [float(x) for x in qs]
    qarr = (C.c_double * max(len(qs), 1))(*qs)
    outs = (L.PdxScalar * max(len(qs), 1))()
    ca = a.c()
    L.check(L.load().pdx_quantile(C.byref(ca), qarr, len(qs), interpolation_code(interpolation), int(bool(skip_nulls)), int(min_count), outs, _stream()))
    res = []
    for s in outs[:len(qs)]:
        if not s.is_valid:
            res.append((None, int(s.count)))
        elif s.dtype in (L.FLOAT64, L.FLOAT32):  # (a float32 result is held widened)
            res.append((float(s.v.f64), int(s.count)))
        elif s.dtype == L.UINT64:
            res.append((int(s.v.u64), int(s.count)))
        else:
            res.append((int(s.v.i64), int(s.count)))
    return res


def mode(a: Column, n=1, skip_nulls=True, min_count=0):
    """The min(n, distinct values) most frequent valid values of a column, by count descending then value ascending (pdx_mode: Arrow's
    mode).  -> (modes Column of a's dtype, counts Column int64), both of the result's length (0: an empty result)."""
    cap = max(0, min(int(n), a.length))
    modes, counts = Column.empty(a.dtype, cap), Column.empty(L.INT64, cap)
    mm, mc, ca = modes.mut(), counts.mut(), a.c()
    L.check(L.load().pdx_mode(C.byref(ca), int(n), int(bool(skip_nulls)), int(min_count), C.byref(mm), C.byref(mc), _stream()))
    return modes._adopt(mm), counts._adopt(mc)


def mode_last_plan() -> dict:
    """The path this thread's last pdx_mode took: {'path': 'count' | 'sort' | 'bool' | 'empty', 'bins': ..., 'width': ..., 'runs': ...}."""
    buf = C.create_string_buffer(256)
    L.check(L.load().pdx_mode_last_plan(buf, 256))
    return dict(w.split("=", 1) for w in buf.value.decode().split() if "=" in w)


_DTYPE_NAMES = {L.INT64: "int64", L.FLOAT64: "float64", L.BOOL: "bool", L.UINT64: "uint64", L.TIMESTAMP_NS: "timestamp[ns]", L.INT32: "int32",
                L.FLOAT32: "float32"}


def _frequency_key(a: Column, what) -> Column:
    """the column as a group-by key: float64 as its bit pattern (distinct = distinct bits), bool as 0 / 1 (pdx_if_else)"""
    if a.dtype in _NARROW:
        raise L.PdxError(L.NOT_IMPLEMENTED, f"{what}: dtype {_DTYPE_NAMES[a.dtype]} is not supported (the group-by does not take 4-byte keys yet)")
    if a.dtype == L.FLOAT64:
        return Column(L.INT64, a.length, a.values, a.validity, a.offset, a.null_count)
    if a.dtype == L.BOOL:
        ones = Column(L.INT64, a.length, torch.ones(max(a.length, 1), dtype=torch.int64, device=_device()), None)
        return if_else(a, ones, 0)
    return a


def value_counts(a: Column):
    """The distinct values (distinct bit patterns; a null is one entry) in first-occurrence order and their row counts: pdx_groupby_create +
    pdx_groupby_unique_keys + pdx_groupby_sizes.  -> (values Column of a's dtype, counts Column int64)."""
    key = _frequency_key(a, "value_counts")
    if a.length == 0:
        return Column.empty(a.dtype, 0), Column.empty(L.INT64, 0)
    h = GroupByHandle.create(key)
    try:
        u, counts = h.unique_keys(), h.sizes()
    finally:
        h.close()
    nulls = u.length - int(aggregate(L.AGG_COUNT, u)[0])
    validity = u.validity if nulls else None
    if a.dtype == L.BOOL:  # (at most three entries)
        hv, hok = u.to_numpy()
        return Column.from_numpy(hv.astype(bool), None if not nulls else hok), counts
    values = u.values.view(torch.float64) if a.dtype == L.FLOAT64 else u.values  # (the key was the bit pattern)
    return Column(a.dtype, u.length, values, validity, u.offset, nulls), counts


def is_unique(a: Column) -> bool:
    """unique().size() == size(): a column with two nulls is not unique."""
    key = _frequency_key(a, "is_unique")
    if a.length == 0:
        return True
    h = GroupByHandle.create(key)
    try:
        return h.num_groups == a.length
    finally:
        h.close()


# ---------------------------------------------------------------- lookups (pdx_is_in ... pdx_dictionary_encode)
def is_in(a: Column, value_set: Column, skip_nulls=False) -> Column:
    """BOOL column without nulls: row i is set when a[i] is one of `value_set` (same dtype; matched by bit pattern) (pdx_is_in)"""
    out = Column.empty(L.BOOL, a.length)
    ca, cs, m = a.c(), value_set.c(), out.mut()
    L.check(L.load().pdx_is_in(C.byref(ca), C.byref(cs), int(bool(skip_nulls)), C.byref(m), _stream()))
    return out._adopt(m)


def index_in(a: Column, value_set: Column, skip_nulls=False) -> Column:
    """INT32 column: the position of a[i]'s first occurrence in `value_set`, null where there is none (pdx_index_in)"""
    out = Column.empty(L.INT32, a.length, with_validity=True)
    ca, cs, m = a.c(), value_set.c(), out.mut()
    L.check(L.load().pdx_index_in(C.byref(ca), C.byref(cs), int(bool(skip_nulls)), C.byref(m), _stream()))
    return out._adopt(m)


def lookup_last_plan() -> dict:
    """The plan of this thread's last is_in / index_in: {'plan': 'lds' | 'global' | 'empty', 'set_size': ..., 'slots': ...}."""
    buf = C.create_string_buffer(256)
    L.check(L.load().pdx_lookup_last_plan(buf, 256))
    return dict(w.split("=", 1) for w in buf.value.decode().split() if "=" in w)


def index(a: Column, value) -> int:
    """The first valid row with a[row] == value (IEEE ==), -1 when there is none; None is the null scalar (pdx_index)"""
    s = None
    if value is not None:
        s = L.PdxScalar(a.dtype, 1)
        if a.dtype in (L.FLOAT64, L.FLOAT32):
            s.v.f64 = float(value)
        elif a.dtype == L.UINT64:
            s.v.u64 = int(value)
        else:
            s.v.i64 = int(value)
    row = C.c_int64(-1)
    ca = a.c()
    L.check(L.load().pdx_index(C.byref(ca), None if s is None else C.byref(s), C.byref(row), _stream()))
    return int(row.value)


def arg_extreme(cols, is_max=False):
    """Per column the row of its smallest / largest valid value (the first on ties, NaN ignored), -1 when there is none: one launch for
    all columns, which may differ in dtype (pdx_arg_extreme).  -> list of int"""
    if not cols:
        return []
    rows = (C.c_int64 * len(cols))()
    L.check(L.load().pdx_arg_extreme(int(bool(is_max)), _col_array(cols), len(cols), rows, _stream()))
    return [int(r) for r in rows]


def dictionary_encode(a: Column):
    """-> (codes Column int32: null for a null row, dictionary Column of a's dtype: the distinct bit patterns in first-occurrence order)
    (pdx_dictionary_encode)"""
    codes, dic = Column.empty(L.INT32, a.length, with_validity=a.has_nulls()), Column.empty(a.dtype, a.length)
    ca, mc, md = a.c(), codes.mut(), dic.mut()
    L.check(L.load().pdx_dictionary_encode(C.byref(ca), C.byref(mc), C.byref(md), _stream()))
    return codes._adopt(mc), dic._adopt(md)


# ---------------------------------------------------------------- join
JOIN_HOW = {"inner": L.JOIN_INNER, "left": L.JOIN_LEFT, "outer": L.JOIN_OUTER, "semi": L.JOIN_SEMI, "anti": L.JOIN_ANTI}


class JoinHandle:
    """Owner of a pdx_join*: the matched key columns of two frames.  ``rows`` is the size of the result; ``indices()`` writes it as INT64
    take indices into the left and the right frame (include/pdx/abi.h, "join")."""

    def __init__(self, left_key: Column, right_key: Column, how):
        self.how = JOIN_HOW[how] if isinstance(how, str) else int(how)
        self._h = C.c_void_p()
        cl, cr = left_key.c(), right_key.c()
        L.check(L.load().pdx_join_create(C.byref(cl), C.byref(cr), self.how, _stream(), C.byref(self._h)))
        n = C.c_int64(0)
        L.check(L.load().pdx_join_rows(self._h, C.byref(n)))
        self.rows = int(n.value)

    def close(self):
        if self._h is not None and self._h.value:
            L.load().pdx_join_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def has_right(self):
        return self.how not in (L.JOIN_SEMI, L.JOIN_ANTI)

    def indices(self, out_left=None, out_right=None):
        """-> (left indices, right indices | None).  Without arguments the outputs are allocated at exactly ``rows`` rows, with the
        validity buffers the join kind requires; a caller's own columns are written in place (their length is the capacity)."""
        if out_left is None:
            out_left = Column.empty(L.INT64, self.rows, with_validity=self.how == L.JOIN_OUTER)
        if out_right is None and self.has_right:
            out_right = Column.empty(L.INT64, self.rows, with_validity=self.how != L.JOIN_INNER)
        ml = out_left.mut()
        mr = out_right.mut() if out_right is not None else None
        L.check(L.load().pdx_join_indices(self._h, C.byref(ml), None if mr is None else C.byref(mr), _stream()))
        out_left._adopt(ml)
        if out_right is not None:
            out_right._adopt(mr)
        return out_left, out_right

    def plan(self) -> dict:
        """{'plan': 'lds' | 'global' | 'empty', 'build_rows': ..., 'distinct': ..., 'out_rows': ...} (pdx_join_last_plan)"""
        buf = C.create_string_buffer(256)
        L.check(L.load().pdx_join_last_plan(self._h, buf, 256))
        return dict(w.split("=", 1) for w in buf.value.decode().split() if "=" in w)


def join_indices(left_key: Column, right_key: Column, how="inner"):
    """The take indices of `left_key` JOIN `right_key` -> (left indices, right indices | None for semi / anti) (pdx_join_create +
    pdx_join_indices).  A null key matches nothing; the row order is defined by include/pdx/abi.h."""
    h = JoinHandle(left_key, right_key, how)
    try:
        return h.indices()
    finally:
        h.close()


# ---------------------------------------------------------------- filter / take / concat
def _col_array(cols):
    arr = (L.PdxColumn * len(cols))(*[c.c() for c in cols])
    return arr


def _mut_array(cols):
    return (L.PdxMutColumn * len(cols))(*[c.mut() for c in cols])


def filter_count(mask: Column, emit_null=True) -> int:
    lib = L.load()
    out = C.c_int64(0)
    cm = mask.c()
    L.check(lib.pdx_filter_count(C.byref(cm), int(emit_null), C.byref(out), _stream()))
    return int(out.value)


def filter(cols, mask: Column, emit_null=True):
    lib = L.load()
    cm = mask.c()
    if cols and cols[0].length != mask.length:  # same check the kernel would make, before sizing outputs
        L.check(lib.pdx_filter(_col_array(cols), len(cols), C.byref(cm), int(emit_null), _mut_array(cols), _stream()))
    m = filter_count(mask, emit_null)
    nullable = mask.has_nulls() and emit_null
    outs = [Column.empty(c.dtype, m, with_validity=c.has_nulls() or nullable) for c in cols]
    marr = _mut_array(outs)
    L.check(lib.pdx_filter(_col_array(cols), len(cols), C.byref(cm), int(emit_null), marr, _stream()))
    return [o._adopt(marr[i]) for i, o in enumerate(outs)]


def take(cols, idx: Column):
    lib = L.load()
    outs = [Column.empty(c.dtype, idx.length, with_validity=c.has_nulls() or idx.has_nulls()) for c in cols]
    marr = _mut_array(outs)
    ci = idx.c()
    L.check(lib.pdx_take(_col_array(cols), len(cols), C.byref(ci), marr, _stream()))
    return [o._adopt(marr[i]) for i, o in enumerate(outs)]


def scatter(cols, idx: Column, outs):
    """outs[c][idx[j]] = cols[c][j] in place (distinct indices)."""
    lib = L.load()
    marr = _mut_array(outs)
    ci = idx.c()
    L.check(lib.pdx_scatter(_col_array(cols), len(cols), C.byref(ci), marr, _stream()))
    return outs


def concat(parts) -> Column:
    """Row concat; parts that mix a 4-byte dtype with another numeric one are first cast to the common type (pdx_cast)."""
    lib = L.load()
    if any(p.dtype in _NARROW for p in parts) and len({p.dtype for p in parts}) > 1:
        dt = parts[0].dtype
        for p in parts[1:]:
            dt = promote_dtype(dt, p.dtype)
        parts = [p if p.dtype == dt else cast(p, dt) for p in parts]
    total = sum(p.length for p in parts)
    out = Column.empty(parts[0].dtype, total, with_validity=any(p.has_nulls() for p in parts))
    m = out.mut()
    L.check(lib.pdx_concat(_col_array(parts), len(parts), C.byref(m), _stream()))
    return out._adopt(m)


# ---------------------------------------------------------------- selection / multiplexing, null handling
def coalesce(cols) -> Column:
    """per row the first non-null cell of `cols` (one dtype, one length), null when all are: one kernel launch (pdx_coalesce)"""
    if not cols:
        raise L.PdxError(L.INVALID, "coalesce: at least one column is required")
    out = Column.empty(cols[0].dtype, cols[0].length, with_validity=cols[0].has_nulls())
    m = out.mut()
    L.check(L.load().pdx_coalesce(_col_array(cols), len(cols), C.byref(m), _stream()))
    return out._adopt(m)


def element_wise_minmax(is_max, cols, skip_nulls=True) -> Column:
    """min_element_wise / max_element_wise of `cols` (one dtype; length n, or 1 = a broadcast scalar) (pdx_element_wise_minmax)"""
    if not cols:
        raise L.PdxError(L.INVALID, "element_wise_minmax: at least one operand is required")
    out = Column.empty(cols[0].dtype, max(c.length for c in cols), with_validity=any(c.has_nulls() for c in cols))
    m = out.mut()
    L.check(L.load().pdx_element_wise_minmax(int(bool(is_max)), _col_array(cols), len(cols), int(bool(skip_nulls)), C.byref(m), _stream()))
    return out._adopt(m)


def clip(x: Column, lo: Column, hi: Column, skip_nulls=True) -> Column:
    """max_element_wise(min_element_wise(x, hi), lo) in one read of x; lo / hi: columns of length 1, which may be null (pdx_clip)"""
    out = Column.empty(x.dtype, x.length, with_validity=x.has_nulls() or lo.has_nulls() or hi.has_nulls())
    cx, cl, ch, m = x.c(), lo.c(), hi.c(), out.mut()
    L.check(L.load().pdx_clip(C.byref(cx), C.byref(cl), C.byref(ch), int(bool(skip_nulls)), C.byref(m), _stream()))
    return out._adopt(m)


def replace_with_mask(a: Column, mask: Column, repl: Column) -> Column:
    """the rows of `a` where `mask` is true replaced by the values of `repl` in their order (pdx_replace_with_mask)"""
    out = Column.empty(a.dtype, a.length, with_validity=a.has_nulls() or mask.has_nulls() or repl.has_nulls())
    ca, cm, cr, m = a.c(), mask.c(), repl.c(), out.mut()
    L.check(L.load().pdx_replace_with_mask(C.byref(ca), C.byref(cm), C.byref(cr), C.byref(m), _stream()))
    return out._adopt(m)


def indices_nonzero(a: Column) -> Column:
    """uint64 ascending rows of `a` that are valid and not zero (pdx_indices_nonzero_count + pdx_indices_nonzero)"""
    lib = L.load()
    cnt = C.c_int64(0)
    ca = a.c()
    L.check(lib.pdx_indices_nonzero_count(C.byref(ca), C.byref(cnt), _stream()))
    out = Column.empty(L.UINT64, int(cnt.value))
    m = out.mut()
    L.check(lib.pdx_indices_nonzero(C.byref(ca), C.byref(m), _stream()))
    return out._adopt(m)


def all_valid_mask(cols) -> Column:
    """BOOL column without nulls: row i is set when every column of `cols` is valid there (pdx_all_valid_mask)"""
    if not cols:
        raise L.PdxError(L.INVALID, "all_valid_mask: at least one column is required")
    out = Column.empty(L.BOOL, cols[0].length)
    m = out.mut()
    L.check(L.load().pdx_all_valid_mask(_col_array(cols), len(cols), C.byref(m), _stream()))
    return out._adopt(m)


def drop_na(cols):
    """the rows at which every column of `cols` is valid: pdx_all_valid_mask, then one pdx_filter over all of them (16 columns a call)"""
    mask = all_valid_mask(cols)
    outs = []
    for c0 in range(0, len(cols), 16):
        outs += filter(cols[c0:c0 + 16], mask, emit_null=False)
    return outs


# ---------------------------------------------------------------- temporal rounding (DataFrame::downsample)
def round_temporal(ts: Column, multiple, unit, ceil=False, week_starts_monday=True, calendar_based_origin=False, nearest=False) -> Column:
    """floor_temporal / ceil_temporal / round_temporal (nearest) of a timestamp[ns] column (pdx_round_temporal)."""
    out = Column.empty(L.TIMESTAMP_NS, ts.length, with_validity=ts.has_nulls())
    m = out.mut()
    ct = ts.c()
    how = L.ROUND_NEAREST if nearest else int(bool(ceil))
    L.check(L.load().pdx_round_temporal(how, C.byref(ct), int(multiple), int(unit), int(bool(week_starts_monday)),
                                        int(bool(calendar_based_origin)), C.byref(m), _stream()))
    return out._adopt(m)


def temporal_component_dtype(comp):
    return L.BOOL if comp == L.TC_IS_LEAP_YEAR else L.FLOAT64 if comp == L.TC_SUBSECOND else L.INT64


def temporal_components(ts: Column, comps, week_options=None):
    """Calendar components of a timestamp[ns] column, all from ONE read of it (pdx_temporal_components): 1 .. 8 pdx_temporal_component
    codes -> list of Columns (int64; bool for is_leap_year; float64 for subsecond).  week_options: (week_starts_monday, count_from_zero,
    first_week_is_fully_in_year) for TC_WEEK."""
    comps = [int(c) for c in comps]
    outs = [Column.empty(temporal_component_dtype(c), ts.length, with_validity=ts.has_nulls()) for c in comps]
    marr = _mut_array(outs) if outs else None
    carr = (C.c_int * max(len(comps), 1))(*comps)
    wo = None if week_options is None else C.byref(L.PdxWeekOptions(*[int(bool(x)) for x in week_options]))
    ct = ts.c()
    L.check(L.load().pdx_temporal_components(C.byref(ct), carr, len(comps), wo, marr, _stream()))
    return [o._adopt(marr[i]) for i, o in enumerate(outs)]


def temporal_between(unit, a: Column, b: Column) -> Column:
    """<unit>s_between(a, b): unit boundaries crossed from a to b, int64 (pdx_temporal_between)."""
    out = Column.empty(L.INT64, a.length, with_validity=a.has_nulls() or b.has_nulls())
    m = out.mut()
    ca, cb = a.c(), b.c()
    L.check(L.load().pdx_temporal_between(int(unit), C.byref(ca), C.byref(cb), C.byref(m), _stream()))
    return out._adopt(m)


# ---------------------------------------------------------------- index alignment (Series::broadcast / reindex)
def index_union(a: Column, b: Column, sort=True) -> Column:
    """distinct labels of both indexes, sorted ascending or in first-occurrence order (pdx_index_union)."""
    out = Column.empty(a.dtype, a.length + b.length)
    m = out.mut()
    ca, cb = a.c(), b.c()
    L.check(L.load().pdx_index_union(C.byref(ca), C.byref(cb), int(bool(sort)), C.byref(m), _stream()))
    return out._adopt(m)


def index_intersection(a: Column, b: Column) -> Column:
    """labels of a that occur in b, one per distinct label, in a's (last-)position order (pdx_index_intersection)."""
    out = Column.empty(a.dtype, a.length)
    m = out.mut()
    ca, cb = a.c(), b.c()
    L.check(L.load().pdx_index_intersection(C.byref(ca), C.byref(cb), C.byref(m), _stream()))
    return out._adopt(m)


def argsort(a: Column, ascending=True) -> Column:
    """uint64 take indices of the stable sort of a (array_sort_indices: NaN behind the numbers, nulls last, in both orders)."""
    out = Column.empty(L.UINT64, a.length)
    m = out.mut()
    ca = a.c()
    L.check(L.load().pdx_argsort(C.byref(ca), int(bool(ascending)), C.byref(m), _stream()))
    return out._adopt(m)


def sort_indices(keys, descending=None, with_info=False):
    """uint64 take indices of the stable lexicographic sort by several key columns (pdx_sort_indices: Arrow's sort_indices; per key numbers
    < NaN < null in both orders).  descending: one flag per key (None: all ascending).  with_info: -> (indices, (rounds, key_bits, passes))."""
    keys = list(keys)
    n = keys[0].length if keys else 0
    out = Column.empty(L.UINT64, n)
    m = out.mut()
    desc = None if descending is None else (C.c_int * max(len(keys), 1))(*[int(bool(d)) for d in descending])
    info = L.PdxSortInfo()
    L.check(L.load().pdx_sort_indices(_col_array(keys) if keys else None, len(keys), desc, C.byref(m), C.byref(info), _stream()))
    out._adopt(m)
    return (out, (info.rounds, info.key_bits, info.passes)) if with_info else out


def select_k(a: Column, k: int, ascending=True) -> Column:
    """the first min(k, a.length) uint64 take indices of argsort(a, ascending), without sorting the column (pdx_select_k)"""
    out = Column.empty(L.UINT64, max(0, min(int(k), a.length)))
    m = out.mut()
    ca = a.c()
    L.check(L.load().pdx_select_k(C.byref(ca), int(k), int(bool(ascending)), C.byref(m), _stream()))
    return out._adopt(m)


def partition_nth(a: Column, pivot: int) -> Column:
    """uint64 indices that partition a around the value of rank `pivot`: smaller keys, equal keys, larger keys, NaN rows, null rows, each
    in row order (pdx_partition_nth; deterministic, not Arrow's std::nth_element order)"""
    out = Column.empty(L.UINT64, a.length)
    m = out.mut()
    ca = a.c()
    L.check(L.load().pdx_partition_nth(C.byref(ca), int(pivot), C.byref(m), _stream()))
    return out._adopt(m)


def select_k_last_plan() -> dict:
    """The plan of this thread's last select_k: {'plan': 'select' | 'sort' | 'empty', 'k': ..., 'rows': ..., 'levels': ...}."""
    buf = C.create_string_buffer(256)
    L.check(L.load().pdx_select_k_last_plan(buf, 256))
    return dict(w.split("=", 1) for w in buf.value.decode().split() if "=" in w)


def reindex_indices(old_index: Column, new_index: Column) -> Column:
    """int64 take indices (LAST position of every new label in old_index, null where absent)."""
    out = Column.empty(L.INT64, new_index.length, with_validity=True)
    m = out.mut()
    co, cn = old_index.c(), new_index.c()
    L.check(L.load().pdx_reindex_indices(C.byref(co), C.byref(cn), C.byref(m), _stream()))
    return out._adopt(m)


# ---------------------------------------------------------------- group-by / resample handles
_AGG_OUT_DT = {L.AGG_MEAN: lambda dt: L.FLOAT64, L.AGG_COUNT: lambda dt: L.INT64, L.AGG_SUM: lambda dt: {L.INT32: L.INT64, L.FLOAT32: L.FLOAT64}.get(dt, dt), L.AGG_MIN: lambda dt: dt,
               L.AGG_MAX: lambda dt: dt, L.AGG_VARIANCE: lambda dt: L.FLOAT64, L.AGG_STDDEV: lambda dt: L.FLOAT64,
               L.AGG_PRODUCT: lambda dt: dt, L.AGG_FIRST: lambda dt: dt, L.AGG_LAST: lambda dt: dt,
               L.AGG_ALL: lambda dt: L.BOOL, L.AGG_ANY: lambda dt: L.BOOL, L.AGG_COUNT_DISTINCT: lambda dt: L.INT64}


class GroupByHandle:
    """Owner of a pdx_groupby* (hash group-by or resample segments)."""

    def __init__(self, handle, key_dtype, keep_alive=None):
        self._h = handle
        self.key_dtype = key_dtype
        self._keep = keep_alive  # the resample handle reads the timestamp buffer lazily

    @staticmethod
    def create(key: Column):
        lib = L.load()
        h = C.c_void_p()
        ck = key.c()
        L.check(lib.pdx_groupby_create(C.byref(ck), _stream(), C.byref(h)))
        return GroupByHandle(h, key.dtype)

    @staticmethod
    def resample(ts: Column, freq_ns, closed_right=False, label_right=False, origin=L.ORIGIN_START_DAY, origin_custom_ns=0, offset_ns=0):
        lib = L.load()
        h = C.c_void_p()
        ct = ts.c()
        L.check(lib.pdx_resample_create(C.byref(ct), int(freq_ns), int(closed_right), int(label_right), int(origin), int(origin_custom_ns),
                                        int(offset_ns), _stream(), C.byref(h)))
        return GroupByHandle(h, L.TIMESTAMP_NS, keep_alive=ts)

    @staticmethod
    def downsample(ts: Column, multiple, unit, ceil=False, week_starts_monday=True, calendar_based_origin=False, label_shift_ns=0):
        """Groups of equal Ceil/FloorTemporal labels (+ label_shift_ns) of a timestamp index -- DataFrame::downsample's GroupBy."""
        lib = L.load()
        h = C.c_void_p()
        ct = ts.c()
        L.check(lib.pdx_downsample_create(C.byref(ct), int(multiple), int(unit), int(bool(ceil)), int(bool(week_starts_monday)),
                                          int(bool(calendar_based_origin)), int(label_shift_ns), _stream(), C.byref(h)))
        return GroupByHandle(h, L.TIMESTAMP_NS)

    def close(self):
        if self._h is not None and self._h.value:
            L.load().pdx_groupby_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_groups(self):
        return int(L.load().pdx_groupby_num_groups(self._h))

    @property
    def num_rows(self):
        return int(L.load().pdx_groupby_num_rows(self._h))

    def unique_keys(self) -> Column:
        out = Column.empty(self.key_dtype if self.key_dtype != L.BOOL else L.INT64, self.num_groups, with_validity=True)
        m = out.mut()
        L.check(L.load().pdx_groupby_unique_keys(self._h, C.byref(m), _stream()))
        return out._adopt(m)

    def group_ids(self) -> torch.Tensor:
        out = torch.empty(max(self.num_rows, 1), dtype=torch.int32, device=_device())
        L.check(L.load().pdx_groupby_group_ids(self._h, out.data_ptr(), _stream()))
        return out[: self.num_rows]

    def map_ids(self, mapping: torch.Tensor) -> Column:
        """per-row map[group_id(row)] (int64)."""
        out = Column.empty(L.INT64, self.num_rows)
        L.check(L.load().pdx_groupby_map_ids(self._h, mapping.data_ptr(), out.values.data_ptr(), _stream()))
        return out

    def first_rows(self) -> torch.Tensor:
        out = torch.empty(max(self.num_groups, 1), dtype=torch.int64, device=_device())
        L.check(L.load().pdx_groupby_first_rows(self._h, out.data_ptr(), _stream()))
        return out[: self.num_groups]

    def groupings(self):
        """Grouper::MakeGroupings: (rows int64 [n]: the rows of group 0, then group 1, ..., each ascending; offsets int64 [G + 1])."""
        rows = torch.empty(max(self.num_rows, 1), dtype=torch.int64, device=_device())
        off = torch.empty(self.num_groups + 1, dtype=torch.int64, device=_device())
        L.check(L.load().pdx_groupby_groupings(self._h, rows.data_ptr(), off.data_ptr(), _stream()))
        return rows[: self.num_rows], off

    def row_labels(self) -> torch.Tensor:
        out = torch.empty(max(self.num_rows, 1), dtype=torch.int64, device=_device())
        L.check(L.load().pdx_resample_row_labels(self._h, out.data_ptr(), _stream()))
        return out[: self.num_rows]

    def bind(self, values: Column):
        """Group `values` once and keep the layout (+ later the per-group sum / count / min / max) in the handle: the reference's
        GroupBy constructor does this for every column (processEach, src/dataframe.cpp:1539-1554).  The handle keeps the column alive."""
        cv = values.c()
        L.check(L.load().pdx_groupby_bind(self._h, C.byref(cv), _stream()))
        if not hasattr(self, "_bound"):
            self._bound = []
        self._bound.append(values)
        return self

    def unbind(self, values: Column | None = None):
        if values is None:
            L.check(L.load().pdx_groupby_unbind(self._h, None))
            self._bound = []
        else:
            cv = values.c()
            L.check(L.load().pdx_groupby_unbind(self._h, C.byref(cv)))
            self._bound = [b for b in getattr(self, "_bound", []) if b is not values]

    def bound_bytes(self) -> int:
        return int(L.load().pdx_groupby_bound_bytes(self._h))

    def bind_limit(self, max_bytes: int):
        L.check(L.load().pdx_groupby_bind_limit(self._h, int(max_bytes)))

    def last_plan(self) -> dict:
        """The path the last agg() took: {'slots': 'dense', 'sort': 'narrow:7+7', 'layout': 'fused', 'reducer': 'flr_reduce_dense', ...}."""
        buf = C.create_string_buffer(512)
        L.check(L.load().pdx_groupby_last_plan(self._h, buf, 512))
        return dict(w.split("=", 1) for w in buf.value.decode().split() if "=" in w)

    def agg(self, values: Column, kinds):
        """All `kinds` from one grouped pass.  -> list of Columns (G rows, group-id order)."""
        kinds = list(kinds)
        G = self.num_groups
        outs = [Column.empty(_AGG_OUT_DT[k](values.dtype), G, with_validity=k in (L.AGG_ALL, L.AGG_ANY) or (
            values.has_nulls() and k not in (L.AGG_COUNT, L.AGG_COUNT_DISTINCT))) for k in kinds]
        marr = _mut_array(outs)
        karr = (C.c_int * len(kinds))(*kinds)
        cv = values.c()
        L.check(L.load().pdx_groupby_agg(self._h, C.byref(cv), karr, len(kinds), marr, _stream()))
        return [o._adopt(marr[i]) for i, o in enumerate(outs)]

    def quantile(self, values: Column, qs, interpolation=L.INTERP_LINEAR, skip_nulls=True, min_count=0):
        """Per group the exact quantiles of its values (pdx_groupby_quantile).  -> list of Columns (G rows, group-id order), one per q."""
        qs = [float(x) for x in qs]
        interp = interpolation_code(interpolation)
        G = self.num_groups
        dt = L.FLOAT64 if interp in (L.INTERP_LINEAR, L.INTERP_MIDPOINT) else values.dtype
        outs = [Column.empty(dt, G, with_validity=True) for _ in qs]
        marr = _mut_array(outs) if outs else None
        qarr = (C.c_double * max(len(qs), 1))(*qs)
        cv = values.c()
        L.check(L.load().pdx_groupby_quantile(self._h, C.byref(cv), qarr, len(qs), interp, int(bool(skip_nulls)), int(min_count), marr, _stream()))
        return [o._adopt(marr[i]) for i, o in enumerate(outs)]


    def mode(self, values: Column):
        """Per group the most frequent valid value (ties: the smallest) and its count (pdx_groupby_mode).  -> (modes, counts), G rows each."""
        G = self.num_groups
        modes, counts = Column.empty(values.dtype, G, with_validity=True), Column.empty(L.INT64, G)
        mm, mc, cv = modes.mut(), counts.mut(), values.c()
        L.check(L.load().pdx_groupby_mode(self._h, C.byref(cv), C.byref(mm), C.byref(mc), _stream()))
        return modes._adopt(mm), counts._adopt(mc)

    def sizes(self) -> Column:
        """rows per group, group-id order (pdx_groupby_sizes)"""
        out = Column.empty(L.INT64, self.num_groups)
        L.check(L.load().pdx_groupby_sizes(self._h, out.values.data_ptr(), _stream()))
        return out


class GroupedValues:
    """Owner of a pdx_grouped*: one float64 column stably sorted by group (for the multi-GPU partial-tree exchange)."""

    def __init__(self, gb: GroupByHandle, values: Column):
        self._gb = gb  # keep the group-by handle alive
        self._h = C.c_void_p()
        cv = values.c()
        L.check(L.load().pdx_groupby_group_values(gb._h, C.byref(cv), _stream(), C.byref(self._h)))
        self.total = None

    def close(self):
        if self._h is not None and self._h.value:
            L.load().pdx_grouped_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self) -> torch.Tensor:
        out = torch.empty(max(self._gb.num_groups, 1), dtype=torch.int64, device=_device())
        L.check(L.load().pdx_grouped_counts(self._h, out.data_ptr(), _stream()))
        return out[: self._gb.num_groups]

    def partial_plan(self, prefix: torch.Tensor, order: torch.Tensor | None = None) -> int:
        self._prefix = prefix.contiguous()  # read again by partial_fill
        self._order = None if order is None else order.contiguous()
        total = C.c_int64(0)
        L.check(L.load().pdx_grouped_partial_plan(self._h, self._prefix.data_ptr(), None if self._order is None else self._order.data_ptr(),
                                                  C.byref(total), _stream()))
        self.total = int(total.value)
        return self.total

    def partial_fill(self, gid_map: torch.Tensor):
        """-> (rec_key int64[total], rec_val float64[total]) device tensors."""
        dev = _device()
        key = torch.empty(max(self.total, 1), dtype=torch.int64, device=dev)
        val = torch.empty(max(self.total, 1), dtype=torch.float64, device=dev)
        gm = gid_map.contiguous()
        L.check(L.load().pdx_grouped_partial_fill(self._h, gm.data_ptr(), key.data_ptr(), val.data_ptr(), _stream()))
        return key[: self.total], val[: self.total]


def replay_partials(rec_key: torch.Tensor, rec_val: torch.Tensor, gid_lo: int, n_own: int) -> torch.Tensor:
    out = torch.empty(max(n_own, 1), dtype=torch.float64, device=_device())
    rk, rv = rec_key.contiguous(), rec_val.contiguous()
    L.check(L.load().pdx_replay_partials(rk.data_ptr(), rv.data_ptr(), int(rk.numel()), int(gid_lo), int(n_own), out.data_ptr(), _stream()))
    return out[:n_own]


# ---------------------------------------------------------------- synthetic inputs (bench / tests)
def synth_keys(start, n, num_keys) -> Column:
    out = Column.empty(L.INT64, n)
    L.check(L.load().pdx_synth_keys(int(start), int(n), int(num_keys), out.values.data_ptr(), _stream()))
    return out


def synth_vals(start, n, seed_off=0) -> Column:
    out = Column.empty(L.FLOAT64, n)
    L.check(L.load().pdx_synth_vals(int(start), int(n), int(seed_off), out.values.data_ptr(), _stream()))
    return out


def synth_ts(start, n, t0_ns, step_ns) -> Column:
    out = Column.empty(L.TIMESTAMP_NS, n)
    L.check(L.load().pdx_synth_ts(int(start), int(n), int(t0_ns), int(step_ns), out.values.data_ptr(), _stream()))
    return out


# ---------------------------------------------------------------- Arrow IPC streams <-> device columns (pdx_ipc_*)
class _FrameMemory:
    """A window of device memory owned by a pdx_ipc_frame, exposed through the CUDA array interface so that a torch tensor can
    alias it without a copy (the tensor keeps this object, and through it the frame, alive)."""

    def __init__(self, frame, ptr, count, typestr):
        self._frame = frame
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class IpcFrame:
    """Owner of a pdx_ipc_frame*: the parsed schema / record batch of ONE Arrow IPC stream and, after load(), its device copy."""

    def __init__(self, blob):
        lib = L.load()
        self._blob = bytes(blob) if not isinstance(blob, (bytes, bytearray, memoryview)) else blob  # must outlive load()
        self._h = C.c_void_p()
        buf = (C.c_char * len(self._blob)).from_buffer_copy(self._blob) if not isinstance(self._blob, bytes) else self._blob
        self._buf = buf
        L.check(lib.pdx_ipc_open(buf, len(self._blob), C.byref(self._h)))
        self.names = [lib.pdx_ipc_column_name(self._h, i).decode() for i in range(lib.pdx_ipc_num_columns(self._h))]
        self.num_rows = int(lib.pdx_ipc_num_rows(self._h))
        self.metadata = {lib.pdx_ipc_metadata_key(self._h, i).decode(): lib.pdx_ipc_metadata_value(self._h, i).decode()
                         for i in range(lib.pdx_ipc_num_metadata(self._h))}

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                L.load().pdx_ipc_destroy(self._h)
            self._h = None
        except Exception:
            pass

    def schema(self):
        """[(name, pdx dtype, null_count)] without touching the GPU."""
        out = []
        for i, nm in enumerate(self.names):
            c = L.PdxColumn()
            L.check(L.load().pdx_ipc_column(self._h, i, C.byref(c)))
            out.append((nm, int(c.dtype), int(c.null_count)))
        return out

    def load(self):
        """One host->device copy of the record batch body (+ widening kernels for narrow types) -> {name: Column} aliasing it."""
        _device()
        L.check(L.load().pdx_ipc_load(self._h, _stream()))
        self._blob = self._buf = None
        cols = []
        n = self.num_rows
        for i, nm in enumerate(self.names):
            c = L.PdxColumn()
            L.check(L.load().pdx_ipc_column(self._h, i, C.byref(c)))
            if c.dtype == L.BOOL:
                vals = torch.as_tensor(_FrameMemory(self, c.values, (n + 7) // 8 + 8, "|u1"), device=_device())
            else:
                vals = torch.as_tensor(_FrameMemory(self, c.values, max(n, 1), "<f8" if c.dtype == L.FLOAT64 else "<i8"), device=_device())
            vb = None
            if c.validity:
                vb = torch.as_tensor(_FrameMemory(self, c.validity, (n + 7) // 8 + 8, "|u1"), device=_device())
            cols.append((nm, Column(int(c.dtype), n, vals, vb, 0, int(c.null_count))))
        return cols


class ParquetFile:
    """Owner of a pdx_parquet_file*: the parsed footer of ONE Parquet file and, after load(), its decoded device columns
    (DataFrame::readParquet, reference src/dataframe.cpp:646-683)."""

    def __init__(self, blob):
        lib = L.load()
        self._blob = blob if isinstance(blob, bytes) else bytes(blob)  # must outlive load()
        self._h = C.c_void_p()
        L.check(lib.pdx_parquet_open(self._blob, len(self._blob), C.byref(self._h)))
        self.names = [lib.pdx_parquet_column_name(self._h, i).decode() for i in range(lib.pdx_parquet_num_columns(self._h))]
        self.num_rows = int(lib.pdx_parquet_num_rows(self._h))
        self.metadata = {lib.pdx_parquet_metadata_key(self._h, i).decode("utf-8", "replace"): lib.pdx_parquet_metadata_value(self._h, i)
                         for i in range(lib.pdx_parquet_num_metadata(self._h))}

    def __del__(self):
        try:
            if self._h is not None and self._h.value:
                L.load().pdx_parquet_destroy(self._h)
            self._h = None
        except Exception:
            pass

    def schema(self):
        """[(name, pdx dtype, null_count from the chunk statistics or -1)] without touching the GPU."""
        out = []
        for i, nm in enumerate(self.names):
            c = L.PdxColumn()
            L.check(L.load().pdx_parquet_column(self._h, i, C.byref(c)))
            out.append((nm, int(c.dtype), int(c.null_count)))
        return out

    def load(self):
        """One host->device copy of the column chunks + the decode kernels -> [(name, Column)] aliasing the file object's memory."""
        _device()
        L.check(L.load().pdx_parquet_load(self._h, _stream()))
        self._blob = None
        cols = []
        n = self.num_rows
        for i, nm in enumerate(self.names):
            c = L.PdxColumn()
            L.check(L.load().pdx_parquet_column(self._h, i, C.byref(c)))
            if c.dtype == L.BOOL:
                vals = torch.as_tensor(_FrameMemory(self, c.values, (n + 7) // 8 + 8, "|u1"), device=_device())
            else:
                vals = torch.as_tensor(_FrameMemory(self, c.values, max(n, 1), "<f8" if c.dtype == L.FLOAT64 else "<i8"), device=_device())
            vb = None
            if c.validity:
                vb = torch.as_tensor(_FrameMemory(self, c.validity, (n + 7) // 8 + 8, "|u1"), device=_device())
            cols.append((nm, Column(int(c.dtype), n, vals, vb, 0, int(c.null_count))))
        return cols


def parquet_write(cols, names) -> bytes:
    """pdx_parquet_write of device columns -> the bytes of a Parquet file (one row group, PLAIN pages)."""
    lib = L.load()
    arr = _col_array(cols)
    cn = (C.c_char_p * len(names))(*[nm.encode() for nm in names])
    out, size = C.c_void_p(), C.c_size_t()
    L.check(lib.pdx_parquet_write(arr, cn, len(cols), 0, _stream(), C.byref(out), C.byref(size)))
    try:
        return C.string_at(out, size.value)
    finally:
        lib.pdx_parquet_free_blob(out)


def ipc_write(cols, names, metadata=None) -> bytes:
    """One schema + one record batch (+ custom metadata) + end-of-stream, the layout DataFrame::toBinary produces."""
    lib = L.load()
    arr = _col_array(cols)
    cn = (C.c_char_p * max(len(names), 1))(*[nm.encode() for nm in names])
    kv = [x.encode() for k, v in (metadata or {}).items() for x in (k, v)]
    ckv = (C.c_char_p * max(len(kv), 1))(*kv)
    out, size = C.c_void_p(), C.c_size_t()
    L.check(lib.pdx_ipc_write(arr, cn, len(cols), ckv, len(kv) // 2, 0, _stream(), C.byref(out), C.byref(size)))
    try:
        return C.string_at(out, size.value)
    finally:
        lib.pdx_ipc_free_blob(out)
