"""The element-wise operations of csrc/elementwise.hip restated in plain numpy (no GPU): pdx_binary, pdx_compare, pdx_if_else, pdx_unary,
pdx_power, pdx_cast, pdx_cast_f64, pdx_logical, pdx_invert.  Every function takes host arrays (an operand of length 1 is the broadcast
scalar) with an optional bool validity, computes in the promoted type (float64 > float32 > int64 > int32) and returns (values, valid),
or raises RefError with Arrow's message.  Values under a null result row are unspecified.  What is restated is what DESIGN and the
kernels document, and tests/golden/elementwise_golden.npz pins it against Arrow 25.0.0."""
import hashlib

import numpy as np

ADD, SUB, MUL, DIV, BIT_OR, BIT_AND, BIT_XOR, SHIFT_LEFT, SHIFT_RIGHT = range(9)
EQ, NE, LT, LE, GT, GE = range(6)
AND, OR = range(2)
NEGATE, ABS, SIGN, SQRT, EXP, BIT_NOT = range(6)

NP = {"i32": np.dtype(np.int32), "i64": np.dtype(np.int64), "f32": np.dtype(np.float32), "f64": np.dtype(np.float64), "u64": np.dtype(np.uint64),
      "bool": np.dtype(bool)}
NAME = {v: k for k, v in NP.items()}
DIGITS = {"f32": 24, "f64": 53}  # mantissa digits: the exact integer range of a float is +-2^digits
ARROW_TYPE_NAME = {"f32": "float", "f64": "double"}


class RefError(Exception):
    pass


def promote(ta, tb):
    for t in ("f64", "f32", "i64"):
        if t in (ta, tb):
            return t
    return "i32"


def is_float(t):
    return t in ("f32", "f64")


def checked(ti, to):
    """Arrow's safe cast of integer ti to float to is range-checked when to cannot hold every ti"""
    return is_float(to) and not is_float(ti) and NP[ti].itemsize * 8 > DIGITS[to]


def _bits_t(dt):
    return np.dtype(np.uint64 if dt.itemsize == 8 else np.uint32)


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(_bits_t(v.dtype))


def _quiet_bit(dt):
    return _bits_t(dt).type(1 << (np.finfo(dt).nmant - 1))


def quieted(v):
    return (bits(v) | _quiet_bit(v.dtype)).view(v.dtype)


def is_nan(v):
    """from the bits: exponent all ones, mantissa not zero"""
    b = bits(v)
    one = _bits_t(v.dtype).type(1)
    nm = np.finfo(v.dtype).nmant
    mant = b & ((one << _bits_t(v.dtype).type(nm)) - one)
    expo = (b >> _bits_t(v.dtype).type(nm)) & _bits_t(v.dtype).type((1 << (v.dtype.itemsize * 8 - 1 - nm)) - 1)
    return (expo == (1 << (v.dtype.itemsize * 8 - 1 - nm)) - 1) & (mant != 0)


def widen_f32(v):
    """float32 -> float64 as cvtss2sd does it: exact, a NaN keeps sign and payload (shifted up 29 bits) and comes out quiet"""
    v = np.ascontiguousarray(v, np.float32)
    nan = is_nan(v)
    with np.errstate(all="ignore"):
        out = np.where(nan, 0.0, v).astype(np.float64)
    b = bits(v).astype(np.uint64)
    nb = ((b >> np.uint64(31)) << np.uint64(63)) | np.uint64(0x7FF8000000000000) | ((b & np.uint64(0x7FFFFF)) << np.uint64(29))
    return np.where(nan, nb, bits(out)).view(np.float64)


def _valid(v, n):
    return np.ones(n, bool) if v is None else np.broadcast_to(np.asarray(v, bool), (n,))


def range_message(value, ti, to):
    lim = 1 << DIGITS[to]
    return f"Integer value {int(value)} not in range: {0 if ti == 'u64' else -lim} to {lim}"


def first_bad(a, valid, ti, to):
    """row of the first VALID value of a outside to's exact range, or -1"""
    if not checked(ti, to):
        return -1
    lim = 1 << DIGITS[to]
    a = np.asarray(a)
    bad = (a > lim) if ti == "u64" else ((a > lim) | (a < -lim))
    bad = bad & _valid(valid, len(a))
    return int(np.flatnonzero(bad)[0]) if bad.any() else -1


def checked_cast(a, valid, ti, to):
    """Arrow's implicit (safe) cast of one operand, whole"""
    a = np.asarray(a, NP[ti])
    if ti == to:
        return a
    row = first_bad(a, valid, ti, to)
    if row >= 0:
        raise RefError(range_message(a[row], ti, to))
    return plain_cast(a, ti, to)


def plain_cast(a, ti, to):
    if ti == "f32" and to == "f64":
        return widen_f32(a)
    return np.asarray(a, NP[ti]).astype(NP[to])  # int -> wider int: exact; int -> float: round to nearest even


def x86_nan(r, x, y):
    """compute, then select: a NaN result is the first NaN operand quieted, else the second one quieted, else (an invalid operation on
    numbers: inf - inf, 0 * inf, 0 / 0, inf / inf) the negative indefinite"""
    r, x, y = np.broadcast_arrays(r, x, y)
    dt = r.dtype
    indefinite = np.array(0xFFF8000000000000 if dt.itemsize == 8 else 0xFFC00000, _bits_t(dt))
    out = np.where(is_nan(x), bits(quieted(x)), np.where(is_nan(y), bits(quieted(y)), indefinite))
    return np.where(is_nan(r), out, bits(r)).astype(_bits_t(dt)).view(dt)


def _int_div(x, y, both_valid):
    dt = x.dtype
    zero = (y == 0) & both_valid
    if zero.any():
        raise RefError("divide by zero")
    skip = ~both_valid | (y == 0) | ((x == np.iinfo(dt).min) & (y == -1))
    ys = np.where(skip, dt.type(1), y)
    q = np.floor_divide(x, ys)
    q = q + (((x % ys) != 0) & ((x < 0) != (ys < 0)))  # floor -> truncation toward zero
    return np.where(skip, dt.type(0), q).astype(dt)


def binary(op, a, ta, av, b, tb, bv, side=0):
    """side 0: two arrays; 1: b is the scalar; 2: a is the scalar (and stays the LEFT operand)"""
    to = promote(ta, tb)
    n = len(b) if side == 2 else len(a)
    if op >= BIT_OR and is_float(to):
        raise RefError("pdx_binary: bit-wise operators and shifts have no kernel matching floating-point input types")
    x = np.broadcast_to(checked_cast(a, av, ta, to), (n,))
    y = np.broadcast_to(checked_cast(b, bv, tb, to), (n,))
    valid = _valid(av, n) & _valid(bv, n)
    dt = NP[to]
    if is_float(to):
        with np.errstate(all="ignore"):
            r = (x + y, x - y, x * y, x / y)[op]
        if side == 2 and op in (ADD, MUL):  # the array element counts as the first operand
            return x86_nan(r, y, x), valid
        return x86_nan(r, x, y), valid
    ut = np.dtype(np.uint64 if dt.itemsize == 8 else np.uint32)
    ux, uy = x.astype(dt).view(ut), y.astype(dt).view(ut)
    if op == ADD:
        r = (ux + uy).view(dt)
    elif op == SUB:
        r = (ux - uy).view(dt)
    elif op == MUL:
        r = (ux * uy).view(dt)
    elif op == DIV:
        r = _int_div(x.astype(dt), y.astype(dt), valid)
    elif op == BIT_OR:
        r = (ux | uy).view(dt)
    elif op == BIT_AND:
        r = (ux & uy).view(dt)
    elif op == BIT_XOR:
        r = (ux ^ uy).view(dt)
    else:
        digits = dt.itemsize * 8 - 1
        keep = (y < 0) | (y >= digits)
        sh = np.where(keep, 0, y).astype(ut)
        r = (ux << sh).view(dt) if op == SHIFT_LEFT else (x.astype(dt) >> sh.astype(dt))
        r = np.where(keep, x, r).astype(dt)
    return np.ascontiguousarray(r), valid


def compare(op, a, ta, av, b, tb, bv, side=0):
    tc = promote(ta, tb)
    n = len(b) if side == 2 else len(a)
    x = np.broadcast_to(checked_cast(a, av, ta, tc), (n,))
    y = np.broadcast_to(checked_cast(b, bv, tb, tc), (n,))
    with np.errstate(all="ignore"):
        r = (x == y, x != y, x < y, x <= y, x > y, x >= y)[op]
    return np.ascontiguousarray(r), _valid(av, n) & _valid(bv, n)


def if_else(cond, cv, a, ta, av, b, tb, bv, side=0):
    """cond ? a : b; both operands are cast whole, chosen or not; null where cond is null or the chosen operand is"""
    to = promote(ta, tb)
    n = len(cond)
    x = checked_cast(a, av, ta, to)  # (a first: only one operand of a pair can be a checked one)
    y = checked_cast(b, bv, tb, to)
    x, y = np.broadcast_to(x, (n,)), np.broadcast_to(y, (n,))
    cond = np.asarray(cond, bool)
    r = np.where(cond, bits(x) if is_float(to) else x, bits(y) if is_float(to) else y)
    r = r.astype(_bits_t(NP[to])).view(NP[to]) if is_float(to) else r.astype(NP[to])
    valid = _valid(cv, n) & np.where(cond, _valid(av, n), _valid(bv, n))
    return np.ascontiguousarray(r), valid


def unary_result_type(op, ti):
    if op in (SQRT, EXP):
        return "f32" if ti == "f32" else "f64"
    if op == SIGN and not is_float(ti):
        return "i64"  # Arrow's int8 (uint8 for uint64) has no dtype here: widened
    return ti


def unary(op, a, ti, av):
    a = np.asarray(a, NP[ti])
    n = len(a)
    valid = _valid(av, n)
    dt = NP[ti]
    if op == BIT_NOT:
        if is_float(ti):
            raise RefError(f"Function 'bit_wise_not' has no kernel matching input types ({ARROW_TYPE_NAME[ti]})")
        return ~a, valid
    if op == NEGATE:
        if is_float(ti):
            return (bits(a) ^ _bits_t(dt).type(1 << (dt.itemsize * 8 - 1))).view(dt), valid
        ut = np.dtype("u%d" % dt.itemsize)
        return (ut.type(0) - a.view(ut)).view(dt), valid
    if op == ABS:
        if is_float(ti):
            return (bits(a) & _bits_t(dt).type((1 << (dt.itemsize * 8 - 1)) - 1)).view(dt), valid
        if ti == "u64":
            return a.copy(), valid
        ut = np.dtype("u%d" % dt.itemsize)
        return np.where(a < 0, ut.type(0) - a.view(ut), a.view(ut)).astype(ut).view(dt), valid
    if op == SIGN:
        if is_float(ti):
            s = np.where(a > 0, dt.type(1), np.where(a < 0, dt.type(-1), dt.type(0))).astype(dt)
            return np.where(is_nan(a), bits(a), bits(s)).astype(_bits_t(dt)).view(dt), valid
        return ((a > 0).astype(np.int64) - (a < 0).astype(np.int64)), valid
    to = unary_result_type(op, ti)
    d = checked_cast(a, av, ti, to)
    with np.errstate(all="ignore"):
        if op == SQRT:
            r = np.sqrt(np.where(is_nan(d) | (d < 0), NP[to].type(0), d)).astype(NP[to])
            qnan = np.array(0x7FF8000000000000 if to == "f64" else 0x7FC00000, _bits_t(NP[to]))
            r = np.where(is_nan(d), bits(quieted(d)), np.where(d < 0, qnan, bits(r))).astype(_bits_t(NP[to])).view(NP[to])
            return r, valid
        return np.exp(d).astype(NP[to]), valid  # (libm: compared within LIBM_TOL_ULP)


def power(a, ti, av, exponent):
    d = checked_cast(a, av, ti, "f64")
    with np.errstate(all="ignore"):
        return np.power(d, np.float64(exponent)), _valid(av, len(d))  # (libm: compared within LIBM_TOL_ULP)


CASTS = (("i32", "i64"), ("i32", "f64"), ("i32", "f32"), ("i64", "f32"), ("i64", "f64"), ("f32", "f64"), ("i32", "i32"), ("i64", "i64"), ("f32", "f32"),
         ("f64", "f64"))  # what pdx_cast offers


def cast(a, ti, av, to, checked_=True):
    a = np.asarray(a, NP[ti])
    r = checked_cast(a, av, ti, to) if checked_ else plain_cast(a, ti, to)
    return np.ascontiguousarray(r).copy(), _valid(av, len(a))


def logical(op, a, av, b, bv):
    """non-Kleene and / or: null where either side is"""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return (a & b) if op == AND else (a | b), _valid(av, len(a)) & _valid(bv, len(a))


def invert(a, av):
    a = np.asarray(a, bool)
    return ~a, _valid(av, len(a))


LIBM = "libm"  # marks a result that is compared within LIBM_TOL_ULP instead of bit for bit


def float_class(v):
    """per value: 0 a positive number or +0, 1 a negative number or -0, 4 +inf, 5 -inf, 6 NaN -- what a libm result is pinned to bit for
    bit (a result that underflows sits within one ULP of zero, so zero is no class of its own)"""
    v = np.asarray(v)
    neg = np.signbit(v)
    return np.where(np.isnan(v), 6, np.where(np.isinf(v), 4 + neg, neg)).astype(np.uint8)


class StreamDigest:
    """64-bit blake2b over the result dtype, the validity bits and the value bytes with null rows zeroed (bool values: packed bits; a libm
    result: its float_class bytes).  Fed in row chunks that are multiples of 8 rows: every validity chunk first, then every value chunk"""

    def __init__(self, tname, libm=False):
        self.tname, self.libm = tname, libm
        self.h = hashlib.blake2b(digest_size=8)
        self.h.update(tname.encode())

    def valid(self, valid):
        self.h.update(np.packbits(np.asarray(valid, bool), bitorder="little").tobytes())

    def values(self, values, valid):
        values = np.ascontiguousarray(values)
        valid = np.asarray(valid, bool)
        assert values.dtype == NP[self.tname], (values.dtype, self.tname)
        if self.tname == "bool":
            self.h.update(np.packbits(values & valid, bitorder="little").tobytes())
        elif self.libm:
            self.h.update(np.where(valid, float_class(values), 0).astype(np.uint8).tobytes())
        else:
            raw = values.view(_bits_t(values.dtype)) if values.dtype.kind == "f" else values
            self.h.update(np.where(valid, raw, raw.dtype.type(0)).tobytes())

    def value(self):
        return int.from_bytes(self.h.digest(), "little")


def digest(values, valid, tname, libm=False):
    d = StreamDigest(tname, libm)
    d.valid(valid)
    d.values(values, valid)
    return d.value()


def ulp_distance(g, e):
    """distance in units of the last place between two finite float arrays of one dtype"""
    it = np.int64 if g.dtype.itemsize == 8 else np.int32
    gi, ei = g.view(it).astype(np.int64), e.view(it).astype(np.int64)
    top = np.int64(np.iinfo(it).min)
    gi = np.where(gi < 0, top - gi, gi)
    ei = np.where(ei < 0, top - ei, ei)
    return np.abs(gi - ei)
