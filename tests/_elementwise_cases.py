"""Inputs and recipes of the element-wise tests: pure functions of their arguments (numpy only).

A RECIPE is the tuple (family, op, ta, tb, side, n, oi, seed, kind); inputs(recipe) regenerates its operands and reference(recipe) the
expected result, so tests/golden/elementwise_golden.npz stores recipes and 64-bit digests, not arrays.

THE FRAME.  Every operand is a slice [off, off + n) of a larger buffer: `off` rows in front and TAIL rows behind hold POISON and their
validity bits are set, and so does every null row inside the slice (validity clear).  Poison is a NaN with a payload of its own or
+-1e300 (+-3e38) for floats, an integer outside the exact range where the operand goes through a checked cast, a zero where it is an
integer divisor, else INT_MIN / INT_MAX.  A value or a bit read one off then shows as a wrong value, a wrong null or a spurious error."""
import zlib

import numpy as np

import _elementwise_ref as R
from _nanbits_inputs import special_values

TAIL = 130
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1027, 4095, 4096, 4097, 4159, 4160, 4161, 8191, 8192,
         8193, 12353)
# (a, b): the first two take the 16-byte vector form for both widths, the others the row-per-lane form with one or both sides misaligned;
# all differ mod 8 and mod 64 between the operands
OFFSETS = ((0, 0), (68, 64), (1, 64), (64, 3), (67, 1))
COND_OFFSETS = (5, 0, 61, 64, 7)
T4 = ("i32", "i64", "f32", "f64")
PAIRS = tuple((a, b) for a in T4 for b in T4)
INT_PAIRS = tuple(p for p in PAIRS if not R.is_float(p[0]) and not R.is_float(p[1]))
CHECKED_PAIRS = tuple(p for p in PAIRS if R.checked(p[0], R.promote(*p)) or R.checked(p[1], R.promote(*p)))
UNARY_TYPES = ("i32", "i64", "u64", "f32", "f64")
POWER_TYPES = ("i64", "u64", "f64")
EXPONENTS = (2.0, 0.5, -1.0)
CAST_F64 = (("i64", 1), ("i64", 0), ("f64", 1), ("f64", 0))  # (input, checked)
FAMILIES = ("binary", "compare", "if_else", "unary", "power", "cast", "cast_f64", "logical", "invert")
KINDS = ("small", "three", "nullonly", "bounds", "scalar_valid", "scalar_null", "div_last", "div_mid", "div_nullonly", "large", "small_eqnan")
MODES = ("rand", "none", "rand", "rand", "allvalid", "rand", "rand", "none", "rand", "allnull")  # validity of an operand, cycled
ERROR_SIZES = (5, 1027, 4097, 2_097_157)
ERROR_OFFSETS = (1, 4)  # OFFSETS index: the vector form, the row form
GRID_CAP_ROWS = 2_097_152    # k_binary_n / k_unary_n / k_if_else_n: 2048 workgroups x 256 lanes x 4 rows
BITMAP_CAP_ROWS = 33_554_432  # k_compare_n (8192 waves x 4096 rows), k_validity_and / k_logical (524,288 threads x 64 rows)
UNROLL_SECOND_TRIP = 3_670_016  # 7 x 524,288: the 4x unrolled row loop of an 8-byte pair takes a second trip above it


class Operand:
    """buf[off : off + n] with validity vbuf[off : off + n] (None: no bitmap); the rest of buf / vbuf is the poisoned frame"""

    def __init__(self, t, buf, vbuf, off, n, voff=None):
        self.t, self.buf, self.vbuf, self.off, self.n = t, buf, vbuf, off, n
        self.voff = off if voff is None else voff  # (differs from off only in a mutant that reads the validity one bit off)

    @property
    def values(self):
        return self.buf[self.off:self.off + self.n]

    @property
    def valid(self):
        return None if self.vbuf is None else self.vbuf[self.voff:self.voff + self.n]


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(k).encode()) if isinstance(k, str) else int(k) for k in key])


def _float_nans(rng, k, dt):
    """quiet and signalling NaNs of both signs with distinct payloads"""
    if dt == np.float64:
        b = (rng.integers(1, 2**51, k).astype(np.uint64) | np.uint64(0x7FF0000000000000) | (rng.integers(0, 2, k).astype(np.uint64) << np.uint64(63))
             | (rng.integers(0, 2, k).astype(np.uint64) << np.uint64(51)))
        return b.view(np.float64)
    b = (rng.integers(1, 2**22, k).astype(np.uint32) | np.uint32(0x7F800000) | (rng.integers(0, 2, k).astype(np.uint32) << np.uint32(31))
         | (rng.integers(0, 2, k).astype(np.uint32) << np.uint32(22)))
    return b.view(np.float32)


def rand_values(t, n, rng, limit=None):
    """random values over many binades with the type's edge values mixed in; |v| <= limit for an integer that goes through a checked cast"""
    dt = R.NP[t]
    if t == "f64":
        v = special_values(rng, n, 0.08, 0.03)
        m = ~R.is_nan(v)  # (a multiplication would quiet the signalling NaNs)
        v[m] *= 2.0 ** rng.integers(-40, 40, n)[m]
    elif t == "f32":
        with np.errstate(all="ignore"):
            v = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32)
        m = rng.random(n) < 0.08
        v[m] = _float_nans(rng, int(m.sum()), np.float32)  # (signalling ones included: the narrow side of a mixed float pair)
    elif t == "u64":
        top = 63 if limit is None else int(limit).bit_length() - 1
        v = rng.integers(0, 2**top, n, dtype=np.uint64) >> rng.integers(0, top, n).astype(np.uint64)
        if limit is None:
            v = v << rng.integers(0, 2, n).astype(np.uint64)
    else:
        top = (dt.itemsize * 8 - 1) if limit is None else int(limit).bit_length() - 1
        mag = rng.integers(0, 2**top, n, dtype=np.int64) >> rng.integers(0, top, n)
        v = (mag * rng.choice(np.array([-1, 1]), n)).astype(dt)
    v = np.ascontiguousarray(v, dt)
    m = rng.random(n) < 0.12
    k = int(m.sum())
    if R.is_float(t):
        edge = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, np.finfo(dt).max, np.finfo(dt).tiny / 4, 3.0, 0.25], dt)
    elif t == "u64":
        edge = np.array([0, 1, 2**53 if limit else 2**64 - 1, 2**53 - 1 if limit else 2**63, 4, 9], dt)
    elif limit is None:
        edge = np.array([np.iinfo(dt).min, np.iinfo(dt).max, -1, 0, 1, 2], dt)
    else:
        edge = np.array([-limit, limit, -1, 0, limit - 1, 1 - limit], dt)  # the bounds themselves pass
    v[m] = edge[rng.integers(0, len(edge), k)]
    return v


def poison(t, m, rng, role):
    """role: 'range' (outside the exact range of the checked cast), 'zero' (an integer divisor), 'plain'"""
    dt = R.NP[t]
    if R.is_float(t):
        big = 1e300 if t == "f64" else 3e38
        nan = np.array([0x7FF400000BAD5EED], np.uint64).view(np.float64)[0] if t == "f64" else np.array([0x7FA5EED1], np.uint32).view(np.float32)[0]
        tab = np.array([nan, big, -big], dt)
    elif role == "zero":
        tab = np.array([0], dt)
    elif t == "u64":
        tab = np.array([2**53 + 1, 2**64 - 1, 2**63], dt)
    elif role == "range":
        lim = 2**53 if t == "i64" else 2**24
        tab = np.array([lim + 1, -lim - 1, np.iinfo(dt).max, np.iinfo(dt).min], dt)
    else:
        tab = np.array([np.iinfo(dt).min, np.iinfo(dt).max], dt)
    return tab[rng.integers(0, len(tab), m)]


def validity(mode, n, rng):
    if mode == "none":
        return None
    if mode == "allvalid":
        return np.ones(n, bool)
    if mode == "allnull":
        return np.zeros(n, bool)
    return rng.random(n) > 0.3


def framed(t, v, valid, off, rng, role):
    """-> Operand: v with poison under its nulls, inside a poisoned frame whose validity bits are set"""
    n = len(v)
    v = v.copy()
    if t == "bool":
        buf = np.concatenate([np.ones(off, bool), v, np.ones(TAIL, bool)])
    else:
        if valid is not None:
            v[~valid] = poison(t, int((~valid).sum()), rng, role)
        buf = np.concatenate([poison(t, off, rng, role), v, poison(t, TAIL, rng, role)])
    vbuf = None if valid is None else np.concatenate([np.ones(off, bool), valid, np.ones(TAIL, bool)])
    return Operand(t, buf, vbuf, off, n)


def _mode(n, oi, k):
    si = SIZES.index(n) if n in SIZES else n % 7
    return MODES[(si * 5 + oi + 3 * k * (1 + si % 3)) % len(MODES)]


def _role(t, to, divisor):
    if R.checked(t, to):
        return "range"
    return "zero" if divisor and not R.is_float(to) else "plain"


def _limit(t, to):
    return (1 << R.DIGITS[to]) if R.checked(t, to) else None


def _as_type(x, t, limit):
    """the number x as type t (an integer: NaN -> 0, clamped to the type's range, or to +-limit for a checked operand)"""
    if R.is_float(t):
        with np.errstate(all="ignore"):
            return R.NP[t].type(x)
    x = x.item()
    if isinstance(x, float):
        x = 0 if x != x else int(max(-2.0**62, min(2.0**62, x)))
    lim = limit or int(np.iinfo(R.NP[t]).max)
    return R.NP[t].type(max(-lim, min(lim, x)))


def _narrow_nan(x):
    """float64 NaNs as float32 NaNs: sign and the top 23 payload bits (kept a NaN)"""
    b = R.bits(np.ascontiguousarray(x, np.float64))
    m = ((b >> np.uint64(29)) & np.uint64(0x7FFFFF)).astype(np.uint32)
    m = np.where(m == 0, np.uint32(0x400000), m)
    return ((b >> np.uint64(63)).astype(np.uint32) << np.uint32(31) | np.uint32(0x7F800000) | m).view(np.float32)


def pair_inputs(family, opclass, ta, tb, side, n, oi, seed, modes=None, eqnan=False):
    """-> {'a': Operand, 'b': Operand [, 'cond': Operand]} for binary / compare / if_else"""
    rng = _rng(family, opclass, ta, tb, side, n, oi, seed)
    to = R.promote(ta, tb)
    na, nb = (1 if side == 2 else n), (1 if side == 1 else n)
    a = rand_values(ta, na, rng, _limit(ta, to))
    b = rand_values(tb, nb, rng, _limit(tb, to))
    if opclass == "bits":
        digits = R.NP[to].itemsize * 8 - 1
        amounts = np.array([-1, 0, 1, 5, digits - 1, digits, 64], R.NP[tb])
        m = rng.random(nb) < 0.8
        b[m] = amounts[rng.integers(0, len(amounts), int(m.sum()))]
    if side == 0:
        # rows where both sides hold the same number (the relations, x - x), and the invalid operations on numbers
        m = rng.random(n) < 0.15
        with np.errstate(all="ignore"):
            if R.is_float(ta) and not R.is_float(tb):
                a[m] = b[m].astype(R.NP[ta])
            elif opclass != "bits":
                b[m] = a[m].astype(R.NP[tb])
        if R.is_float(to):
            pairs = ((np.inf, np.inf), (np.inf, -np.inf), (0.0, np.inf), (np.inf, 0.0), (0.0, 0.0), (-0.0, 0.0), (-np.inf, -np.inf))
            pick = rng.integers(0, len(pairs), n)
            m = rng.random(n) < 0.08
            for k, (x, y) in enumerate(pairs):
                mk = m & (pick == k)
                a[mk] = x if R.is_float(ta) else 0
                b[mk] = y if R.is_float(tb) else 0
    elif opclass != "bits":  # rows that hold the scalar's number
        arr, sc, t = (a, b, ta) if side == 1 else (b, a, tb)
        m = rng.random(n) < 0.15
        arr[m] = _as_type(sc[0], t, _limit(t, to))
    if eqnan and R.is_float(ta) and R.is_float(tb):
        # both-NaN rows carry one payload (Arrow's own choice between two NaNs is not uniform in the rows its vector
        # loops leave over).  The scalar, else the narrower side, is the source; a float64 source first becomes representable in float32
        src_is_a = side == 2 or (side == 0 and R.NP[ta].itemsize <= R.NP[tb].itemsize)
        s, d, ts, td = (a, b, ta, tb) if src_is_a else (b, a, tb, ta)
        if ts == "f64" and td == "f32":
            m = R.is_nan(s)
            s[m] = R.widen_f32(_narrow_nan(s[m]))
        both = np.broadcast_to(R.is_nan(s), (n,)) & R.is_nan(d)
        sv = np.broadcast_to(s, (n,))[both]
        d[both] = sv if ts == td else R.widen_f32(sv) if ts == "f32" else _narrow_nan(sv)
    if family == "binary" and opclass == "arith" and not R.is_float(to):
        b[b == 0] = 7  # an integer divisor is zero only under a null
    modes = modes or (_mode(n, oi, 1), _mode(n, oi, 2))
    va, vb = validity(modes[0], na, rng), validity(modes[1], nb, rng)
    if side and (modes[1 if side == 1 else 0] == "allnull") and (n + oi) % 3:
        if side == 1:
            vb = np.ones(1, bool)  # (a null scalar makes every row null: kept to a third of these recipes)
        else:
            va = np.ones(1, bool)
    off = OFFSETS[oi]
    out = {"a": framed(ta, a, va, off[0], rng, _role(ta, to, False)),
           "b": framed(tb, b, vb, off[1], rng, _role(tb, to, family == "binary" and opclass == "arith"))}
    if family == "if_else":
        cond = rng.random(n) > 0.5
        out["cond"] = framed("bool", cond, validity(_mode(n, oi, 3) if _mode(n, oi, 3) != "allnull" or n % 2 else "rand", n, rng), COND_OFFSETS[oi], rng, "plain")
    return out


def one_input(family, t, n, oi, seed, to=None, mode=None, positive=False):
    """-> {'a': Operand} for unary / power / cast / cast_f64 / invert"""
    rng = _rng(family, t, to or "", n, oi, seed)
    if t == "bool":
        a = rng.random(n) > 0.5
    else:
        a = rand_values(t, n, rng, _limit(t, to) if to else None)
    return {"a": framed(t, a, validity(mode or _mode(n, oi, 1), n, rng), OFFSETS[oi][0], rng, _role(t, to, False) if to else "plain")}


def logical_inputs(n, oi, seed):
    rng = _rng("logical", n, oi, seed)
    off = OFFSETS[oi]
    return {"a": framed("bool", rng.random(n) > 0.5, validity(_mode(n, oi, 1), n, rng), off[0], rng, "plain"),
            "b": framed("bool", rng.random(n) > 0.5, validity(_mode(n, oi, 2), n, rng), off[1], rng, "plain")}


# ---------------------------------------------------------------- recipes
def opclass(family, op):
    return ("bits" if op >= R.BIT_OR else "arith") if family == "binary" else ""


def checked_operand(family, ta, tb):
    """-> ('a' | 'b' | None, the float type it is cast to)"""
    if family in ("binary", "compare", "if_else"):
        to = R.promote(ta, tb)
        return ("a", to) if R.checked(ta, to) else ("b", to) if R.checked(tb, to) else (None, to)
    if family == "unary":
        to = R.unary_result_type(R.SQRT, ta)
        return ("a", to) if R.checked(ta, to) else (None, to)
    if family == "power":
        return ("a", "f64") if R.checked(ta, "f64") else (None, "f64")
    if family in ("cast", "cast_f64"):
        to = tb if family == "cast" else "f64"
        return ("a", to) if R.checked(ta, to) else (None, to)
    return None, None


def error_rows(n):
    """three rows in different lanes, 4-row groups and workgroups; above the grid cap one in the second round and one in the n & 3 tail"""
    if n > GRID_CAP_ROWS:
        return 1_000_003, GRID_CAP_ROWS + 1, n - 1
    if n <= 5:
        return 1, 2, n - 1
    return n // 3, (2 * n) // 3 + 1, n - 1


def _out_of_range(t, to, k):
    lim = 1 << R.DIGITS[to]
    if t == "u64":
        return (lim + 2, 2**64 - 2 - k, 2**63 + 5, lim + 77)[k]  # (none of them a poison value)
    return (-lim - 2 - k, lim + 2, np.iinfo(R.NP[t]).min + 3, lim + 77)[k]


def inputs(recipe):
    family, op, ta, tb, side, n, oi, seed, kind = recipe
    if family in ("binary", "compare", "if_else"):
        modes = None if kind in ("small", "large", "small_eqnan") else ("rand", "rand")
        if kind == "large":
            modes = ("rand", "rand") if family == "compare" else ("rand", "none")
        ops = pair_inputs(family, opclass(family, op), ta, tb, side, n, oi, seed, modes, kind == "small_eqnan")
    elif family == "logical":
        ops = logical_inputs(n, oi, seed)
    elif family == "invert":
        ops = one_input(family, "bool", n, oi, seed)
    else:
        _, to = checked_operand(family, ta, tb)
        if family == "unary" and op not in (R.SQRT, R.EXP):
            to = None
        ops = one_input(family, ta, n, oi, seed, to, None if kind in ("small", "large") else "rand")
    if kind in ("small", "large", "small_eqnan"):
        return ops
    # ---- the error recipes: plant values in the frame built above
    who, to = checked_operand(family, ta, tb)
    if kind.startswith("div"):
        b = ops["b"]
        rows = {"div_last": [n - 1], "div_mid": [(n // 2) & ~3], "div_nullonly": []}[kind]
        a = ops["a"]
        for r in rows:
            b.buf[b.off + r] = 0
            b.vbuf[b.off + r] = True
            a.vbuf[a.off + (r if a.n > 1 else 0)] = True
        return ops
    x = ops[who]
    t = x.t
    if kind == "three":
        rows = sorted(set(error_rows(n)))
        first = rows[0]
        if first > 0:  # an out-of-range value under a null in front of the first valid one
            x.vbuf[x.off + first - 1] = False
            x.buf[x.off + first - 1] = _out_of_range(t, to, 3)
        for k, r in enumerate(rows):
            x.buf[x.off + r] = _out_of_range(t, to, k)
            x.vbuf[x.off + r] = True
    elif kind == "nullonly":
        x.vbuf[x.off] = False
        x.buf[x.off] = _out_of_range(t, to, 0)
    elif kind == "bounds":
        lim = 1 << R.DIGITS[to]
        for k, r in enumerate(sorted(set(error_rows(n)))):
            x.buf[x.off + r] = (lim, 0 if t == "u64" else -lim, lim)[k]
            x.vbuf[x.off + r] = True
    elif kind in ("scalar_valid", "scalar_null"):
        x.buf[x.off] = _out_of_range(t, to, 1)
        x.vbuf[x.off] = kind == "scalar_valid"
    return ops


def rows(ops, start, stop, n):
    """the operands of an n-row recipe restricted to rows [start, stop) of the result (a length-1 operand stays the scalar it is)"""
    return {k: x if x.n == 1 and n != 1 else Operand(x.t, x.buf, x.vbuf, x.off + start, stop - start, x.voff + start) for k, x in ops.items()}


def input_key(recipe):
    """recipes with equal keys have equal inputs (the ops of a class share them)"""
    family, op = recipe[:2]
    return (opclass(family, op) if family != "unary" else op in (R.SQRT, R.EXP),) + tuple(recipe[5:])


def result_type(recipe):
    """-> (result type name, whether it is a libm result)"""
    family, op, ta, tb = recipe[:4]
    if family in ("binary", "if_else"):
        return R.promote(ta, tb), False
    if family == "unary":
        return R.unary_result_type(op, ta), op == R.EXP
    if family in ("power", "cast_f64"):
        return "f64", family == "power"
    return (tb if family == "cast" else "bool"), False


def reference(recipe, ops=None, swap_lhs=False):
    """-> (values, valid, result type name, libm) or raises R.RefError"""
    family, op, ta, tb, side, n, oi, seed, kind = recipe
    ops = ops or inputs(recipe)
    if swap_lhs:  # (a mutant: scalar OP array computed as array OP scalar)
        b, a = ops["a"], ops["b"]
        v, ok = R.binary(op, a.values, tb, a.valid, b.values, ta, b.valid, 1)
        return v, ok, R.promote(ta, tb), False
    a = ops["a"]
    if family == "binary":
        v, ok = R.binary(op, a.values, ta, a.valid, ops["b"].values, tb, ops["b"].valid, side)
        return v, ok, R.promote(ta, tb), False
    if family == "compare":
        v, ok = R.compare(op, a.values, ta, a.valid, ops["b"].values, tb, ops["b"].valid, side)
        return v, ok, "bool", False
    if family == "if_else":
        c = ops["cond"]
        v, ok = R.if_else(c.values, c.valid, a.values, ta, a.valid, ops["b"].values, tb, ops["b"].valid, side)
        return v, ok, R.promote(ta, tb), False
    if family == "unary":
        v, ok = R.unary(op, a.values, ta, a.valid)
        return v, ok, R.unary_result_type(op, ta), op == R.EXP
    if family == "power":
        v, ok = R.power(a.values, ta, a.valid, EXPONENTS[op])
        return v, ok, "f64", True
    if family == "cast":
        v, ok = R.cast(a.values, ta, a.valid, tb)
        return v, ok, tb, False
    if family == "cast_f64":
        v, ok = R.cast(a.values, ta, a.valid, "f64", bool(op))
        return v, ok, "f64", False
    if family == "logical":
        v, ok = R.logical(op, a.values, a.valid, ops["b"].values, ops["b"].valid)
        return v, ok, "bool", False
    v, ok = R.invert(a.values, a.valid)
    return v, ok, "bool", False


def groups():
    """[(family, ta, tb, side)] : one GPU test each"""
    g = [(f, ta, tb, s) for f in ("binary", "compare", "if_else") for ta, tb in PAIRS for s in (0, 1, 2)]
    g += [("unary", t, "", 0) for t in UNARY_TYPES] + [("power", t, "", 0) for t in POWER_TYPES]
    g += [("cast", ti, to, 0) for ti, to in R.CASTS] + [("cast_f64", t, "", 0) for t in ("i64", "f64")]
    return g + [("logical", "", "", 0), ("invert", "", "", 0)]


def group_ops(family, ta, tb):
    if family == "binary":
        return list(range(R.ADD, R.DIV + 1)) + (list(range(R.BIT_OR, R.SHIFT_RIGHT + 1)) if (ta, tb) in INT_PAIRS else [])
    if family == "compare":
        return list(range(6))
    if family == "unary":
        return list(range(6))
    if family == "power":
        return list(range(len(EXPONENTS)))
    if family == "cast_f64":
        return [1, 0]
    if family == "logical":
        return [R.AND, R.OR]
    return [0]


def small_recipes(group):
    family, ta, tb, side = group
    return [(family, op, ta, tb, side, n, oi, 1, "small") for op in group_ops(family, ta, tb) for n in SIZES for oi in range(len(OFFSETS))]


def error_recipes(group):
    """the recipes that plant out-of-range values / zero divisors: errors, and their passing neighbours"""
    family, ta, tb, side = group
    who, to = checked_operand(family, ta, tb)
    out = []
    op = {"binary": R.ADD, "compare": R.LT, "if_else": 0, "unary": R.SQRT, "power": 0, "cast": 0, "cast_f64": 1}.get(family, 0)
    if who and family != "power":
        scalar_checked = (side == 1 and who == "b") or (side == 2 and who == "a")
        for n in ERROR_SIZES:
            for oi in ERROR_OFFSETS:
                if scalar_checked:
                    out += [(family, op, ta, tb, side, n, oi, 1, k) for k in ("scalar_valid", "scalar_null")]
                else:
                    out += [(family, op, ta, tb, side, n, oi, 1, k) for k in ("three", "nullonly", "bounds")]
    if family == "binary" and (ta, tb) in INT_PAIRS and side != 1:
        for n in ERROR_SIZES:
            for oi in ERROR_OFFSETS:
                out += [(family, R.DIV, ta, tb, side, n, oi, 1, k) for k in ("div_last", "div_mid", "div_nullonly")]
    return out


def large_recipes():
    """one op each, the pairs rotating; every one sits past a launch boundary of its kernel"""
    out = []
    rot = ((R.ADD, "f32", "f32"), (R.MUL, "i32", "f64"), (R.SUB, "f64", "f64"), (R.DIV, "i32", "i32"), (R.SUB, "f64", "f32"), (R.ADD, "i64", "i64"))
    k = 0
    for n in (GRID_CAP_ROWS - 1, GRID_CAP_ROWS, GRID_CAP_ROWS + 5):
        for oi in (1, 2):
            for width in range(3):  # a narrow pair, a mixed pair, an 8-byte pair
                op, ta, tb = rot[width + 3 * (k % 2)]
                out.append(("binary", op, ta, tb, 0, n, oi, 1, "large"))
            k += 1
    out += [("binary", R.MUL, "f64", "f64", 0, UNROLL_SECOND_TRIP + 3, 2, 1, "large"), ("binary", R.ADD, "i64", "i64", 0, 4_194_309, 2, 1, "large")]
    out += [("unary", R.NEGATE, "f32", "", 0, GRID_CAP_ROWS + 5, 1, 1, "large"), ("unary", R.SQRT, "i32", "", 0, GRID_CAP_ROWS + 5, 4, 1, "large"),
            ("if_else", 0, "i32", "f64", 0, GRID_CAP_ROWS + 5, 1, 1, "large"), ("if_else", 0, "f32", "f32", 1, GRID_CAP_ROWS + 5, 4, 1, "large")]
    big = BITMAP_CAP_ROWS + 4096 + 5
    out += [("compare", R.LT, "i32", "f32", 0, big, 1, 1, "large"), ("compare", R.GE, "f64", "i64", 0, big, 1, 1, "large"),
            ("compare", R.NE, "i32", "i32", 0, big, 4, 1, "large"),
            ("logical", R.AND, "", "", 0, BITMAP_CAP_ROWS + 65, 3, 1, "large"), ("invert", 0, "", "", 0, BITMAP_CAP_ROWS + 65, 2, 1, "large"),
            ("if_else", 0, "i32", "i32", 0, BITMAP_CAP_ROWS + 65, 1, 1, "large")]
    return out


def all_recipes():
    out = []
    for g in groups():
        out += small_recipes(g) + error_recipes(g)
    return out + large_recipes()


# ---------------------------------------------------------------- the mutation condition
# Wrong kernels, restated on the reference.  A recipe is kept only if every APPLICABLE one changes its digest or message.  Whether one
# applies is decided from the inputs by the rule next to it, never by trying it:
#   v{a,b,c}_{early,late}  the validity of a / b / the condition read one bit early / late.  Applies when the operand has a bitmap, the bit in
#                          front exists (offset > 0) and the shifted window differs from the true one at a row where every OTHER factor of
#                          the result's validity is set (binary / compare / logical: the other operand valid; if_else: the condition valid
#                          and choosing this operand, for the condition's own validity the chosen operand valid; one column: any row).
#   c_{early,late}         the condition bits read one row off: the shifted bits differ at a row where the condition is valid.
#   {a,b}_{early,late}     the values read one row off: the shifted values differ in bits at a row where the result is valid (if_else: and
#                          this operand is the chosen one).
#   tail_poison            the last n & 3 rows (bit-packed results: the last partial 64-row word) left as the prefill: such rows exist and one
#                          of them is valid.
#   valid_tail_poison      the last partial word of the result's validity left as the prefill (bitmap_prefill): n % 64 != 0.
#   ballot_swap1 / 2       compare: rows i and i ^ 1 (i ^ 2) swapped within whole 4-row groups: a valid row below n & ~3.
#   word_swap              compare: words k and k ^ 1 swapped: n >= 128 and a valid row below n & ~127.
#   bad_last / bad_second  the named value taken from the last / second offending valid row: the true outcome is a range error and that row
#                          exists and holds another value than the first.
#   null_bad_counted       an out-of-range value under a null counted: one lies in front of the first valid offending row (or there is none).
#   null_zero_counted      a zero divisor under a null counted: integer divide, a zero where not both sides are valid, no valid zero.
#   lhs_swapped            scalar-lhs subtract / divide computed as array OP scalar: a valid row exists.
#   nan_other              the NaN payload of the other operand: a float result with a valid row where both operands are NaN, bits differing.
#   wrap64                 int32 arithmetic done at 64 bits and truncated: differs only in the shift range and MIN / -1, so it applies to
#                          int32 shifts with a valid amount in [31, 63) and to int32 divide with a valid MIN / -1 row.
# When the true outcome is an error only bad_last / bad_second / null_bad_counted apply (a one-off read need not move the first bad row).
MUTANTS = ("va_early", "va_late", "vb_early", "vb_late", "vc_early", "vc_late", "c_early", "c_late", "a_early", "a_late", "b_early", "b_late",
           "tail_poison", "valid_tail_poison", "ballot_swap1", "ballot_swap2", "word_swap", "bad_last", "bad_second", "null_bad_counted",
           "null_zero_counted", "lhs_swapped", "nan_other", "wrap64")
PREFILL = 0xA5  # every byte of an output buffer before the call (a bit-packed buffer: PREFILL or its complement, see bitmap_prefill)


def bitmap_prefill(expected, mask, n):
    """the byte a bit-packed output is filled with before the call: of 0xA5 and 0x5A the one that differs from the expected bit at the first
    row of the last partial 64-row word that `mask` selects -- so a word left unwritten can never hold the right answer by accident"""
    rows = np.flatnonzero(mask[n & ~63:]) + (n & ~63)
    if not len(rows):
        return PREFILL
    r = int(rows[0])
    return PREFILL ^ 0xFF if bool(expected[r]) == bool(PREFILL >> (r & 7) & 1) else PREFILL


def prefill_bits(n, byte=PREFILL):
    return np.unpackbits(np.full((n + 7) // 8, byte, np.uint8), bitorder="little")[:n].astype(bool)


def prefill_values(dt, n):
    return np.full(n * dt.itemsize, PREFILL, np.uint8).view(dt)


def _shift(x, dval=0, dvalid=0):
    return Operand(x.t, x.buf, x.vbuf, x.off + dval, x.n, x.voff + dvalid)


def _window(x, n):
    v = x.valid
    return np.ones(n, bool) if v is None else np.broadcast_to(v, (n,))


def _others_set(recipe, ops, name, n):
    """rows where every factor of the result's validity other than operand `name`'s own is set"""
    family = recipe[0]
    if family in ("binary", "compare", "logical"):
        return _window(ops["b" if name == "a" else "a"], n)
    if family == "if_else":
        c, cv = ops["cond"].values, _window(ops["cond"], n)
        if name == "cond":
            return np.where(c, _window(ops["a"], n), _window(ops["b"], n))
        return cv & (c if name == "a" else ~c)
    return np.ones(n, bool)


def _raw(v):
    return R.bits(v) if v.dtype.kind == "f" else v


def mutant_outcomes(recipe, ops, want, outcome):
    """-> (bit mask of the applicable mutants, the set of applicable ones whose outcome equals `want`)"""
    family, op, ta, tb, side, n, oi, seed, kind = recipe
    live, same = 0, set()

    def consider(name, fn):
        nonlocal live
        live |= 1 << MUTANTS.index(name)
        if outcome(fn) == want:
            same.add(name)

    def with_ops(**repl):
        return lambda: reference(recipe, {**ops, **repl})

    who, to = checked_operand(family, ta, tb)
    if want[0] == "error":
        if "not in range" in want[1]:
            x = ops[who]
            lim = 1 << R.DIGITS[to]
            vals = x.values
            out = (vals > lim) if x.t == "u64" else ((vals > lim) | (vals < -lim))
            bad = np.flatnonzero(out & _window(x, x.n))
            for name, k in (("bad_last", -1), ("bad_second", 1)):
                if len(bad) > 1 and vals[bad[k]] != vals[bad[0]]:
                    consider(name, lambda k=k: (_ for _ in ()).throw(R.RefError(R.range_message(vals[bad[k]], x.t, to))))
            anyrow = np.flatnonzero(out)
            if len(anyrow) and anyrow[0] < bad[0]:
                consider("null_bad_counted", lambda: (_ for _ in ()).throw(R.RefError(R.range_message(vals[anyrow[0]], x.t, to))))
        return live, same
    v, ok, tname, libm = reference(recipe, ops)
    # ---- one-off reads of the inputs
    for name in ("a", "b", "cond"):
        if name not in ops:
            continue
        x = ops[name]
        others = _others_set(recipe, ops, name, n)
        for d, tag in ((-1, "early"), (1, "late")):
            if x.off + d < 0:
                continue
            if x.vbuf is not None:
                sh = _shift(x, dvalid=d)
                if (np.broadcast_to(sh.valid, (n,)) != _window(x, n))[others].any():
                    consider(f"v{name[0]}_{tag}", with_ops(**{name: sh}))
            sh = _shift(x, dval=d)
            differs = np.broadcast_to(_raw(sh.values) != _raw(x.values), (n,))
            if name == "cond":
                if (differs & _window(x, n)).any():
                    consider(f"c_{tag}", with_ops(cond=sh))
            else:
                chosen = ok if family != "if_else" else ok & (ops["cond"].values if name == "a" else ~ops["cond"].values)
                if (differs & chosen).any():
                    consider(f"{name}_{tag}", with_ops(**{name: sh}))
    # ---- rows of the output left unwritten
    packed = tname == "bool"
    t0 = (n & ~63) if packed else (n & ~3)
    if t0 < n and ok[t0:].any():
        def tail():
            w = v.copy()
            w[t0:] = prefill_bits(n, bitmap_prefill(v, ok, n))[t0:] if packed else prefill_values(w.dtype, n - t0)
            return w, ok, tname, libm
        consider("tail_poison", tail)
    if n & 63:
        def vtail():
            k = ok.copy()
            k[n & ~63:] = prefill_bits(n, bitmap_prefill(ok, np.ones(n, bool), n))[n & ~63:]
            return v, k, tname, libm
        consider("valid_tail_poison", vtail)
    if family == "compare":
        for name, x, lim in (("ballot_swap1", 1, n & ~3), ("ballot_swap2", 2, n & ~3), ("word_swap", 64, n & ~127)):
            if lim and ok[:lim].any():
                def swapped(x=x, lim=lim):
                    w = v.copy()
                    w[:lim] = v[np.arange(lim) ^ x]
                    return w, ok, tname, libm
                consider(name, swapped)
    if family == "binary":
        a, b = ops["a"], ops["b"]
        if op == R.DIV and not R.is_float(tname):
            both = _window(a, n) & _window(b, n)
            if (np.broadcast_to(b.values == 0, (n,)) & ~both).any():
                consider("null_zero_counted", lambda: (_ for _ in ()).throw(R.RefError("divide by zero")))
        if side == 2 and op in (R.SUB, R.DIV) and ok.any():
            consider("lhs_swapped", lambda: reference(recipe, ops, swap_lhs=True))
        if R.is_float(tname):
            x = np.broadcast_to(R.plain_cast(a.values, ta, tname), (n,))
            y = np.broadcast_to(R.plain_cast(b.values, tb, tname), (n,))
            if (ok & R.is_nan(x) & R.is_nan(y) & (R.bits(R.quieted(x)) != R.bits(R.quieted(y)))).any():
                def other():
                    w = v.copy()
                    first = y if (side == 2 and op in (R.ADD, R.MUL)) else x
                    second = x if first is y else y
                    m = R.is_nan(x) & R.is_nan(y)
                    w[m] = R.quieted(np.ascontiguousarray(second))[m]
                    return w, ok, tname, libm
                consider("nan_other", other)
        if tname == "i32" and op in (R.DIV, R.SHIFT_LEFT, R.SHIFT_RIGHT):
            x, y = np.broadcast_to(a.values, (n,)), np.broadcast_to(b.values, (n,))
            hit = ((x == np.iinfo(np.int32).min) & (y == -1)) if op == R.DIV else ((y >= 31) & (y < 63))
            if (hit & ok).any():
                def wide():
                    w, k = R.binary(op, a.values.astype(np.int64), "i64", a.valid, b.values.astype(np.int64), "i64", b.valid, side)
                    return w.astype(np.int32), k, tname, libm
                consider("wrap64", wide)
    return live, same
