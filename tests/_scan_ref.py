"""numpy restatement of the order-dependent column transforms (cumsum / cumprod / cummax / cummin, ffill / bfill, shift) with Arrow's
semantics, the loader of tests/golden/scan_golden.npz and the a-priori error bound of the float sum / product.  TEST INFRASTRUCTURE:
tests/test_scan_golden.py holds it against the frozen Arrow results on the CPU, tests/test_gpu_scan.py holds the GPU library against it."""
import json
import os
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_golden.npz")
NP_T = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "f32": np.float32, "ts": np.int64}
BITS_T = {"i64": np.uint64, "u64": np.uint64, "f64": np.uint64, "i32": np.uint32, "f32": np.uint32, "ts": np.uint64}


class ScanGolden:
    def __init__(self, store=None):
        z = np.load(GOLDEN) if store is None else store
        self.manifest = json.loads(str(z["manifest"]))
        self.blobs = {k: np.asarray(z[k]) for k in (z.files if store is None else z) if k != "manifest"}
        self.cases = self.manifest["cases"]

    def get(self, name, field):
        key = f"{name}/{field}"
        if key not in self.manifest["arrays"]:
            return None
        blob, first, count = self.manifest["arrays"][key]
        return self.blobs[blob][first:first + count]

    def inputs(self, case):
        """-> (typed values, valid | None)"""
        a = self.get(case["name"], "a")
        if case["dtype"] != "bool":
            a = a.view(NP_T[case["dtype"]])
        v = self.get(case["name"], "a_valid")
        return a, (None if v is None else v.astype(bool))

    def expected(self, case):
        """-> (result bits, valid)"""
        return self.get(case["name"], "out"), self.get(case["name"], "out_valid").astype(bool)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


class StartError(ValueError):
    pass


def cast_start(start, dtype):
    """Arrow's safe cast of the double `start` to the column's type"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        with np.errstate(over="ignore"):
            return dtype.type(start)
    info = np.iinfo(dtype)
    if not (start == start and info.min <= start <= info.max and float(int(start)) == start and info.min <= int(start) <= info.max):
        text = "nan" if start != start else "%f" % start
        raise StartError(f"Float value {text} was truncated converting to {dtype.name}")
    return dtype.type(int(start))


def _latest_zero_sign(x, m):
    """max / min keep the LATER operand on a tie: a running extreme of zero carries the sign of the latest zero seen"""
    zero = x == 0
    last = np.maximum.accumulate(np.where(zero, np.arange(len(x)), -1))
    at = m == 0
    out = m.copy()
    out[at] = x[last[at]]
    return out


def cumulative(op, a, valid, start, skip_nulls=True):
    """-> (values, valid).  op: "sum" | "prod" | "max" | "min".  Values under a null row are unspecified."""
    a = np.asarray(a)
    n = len(a)
    s = cast_start(float(start), a.dtype)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    is_f = a.dtype.kind == "f"
    with np.errstate(all="ignore"):
        if op in ("sum", "prod"):
            ident = (-0.0 if op == "sum" else 1.0) if is_f else (0 if op == "sum" else 1)
            work = a if is_f else a.view(BITS_T["i64" if a.dtype.itemsize == 8 else "i32"])  # integers wrap: accumulate unsigned
            first = np.array([s]).astype(a.dtype)
            first = first if is_f else first.view(work.dtype)
            x = np.concatenate([first, np.where(ok, work, work.dtype.type(ident))])
            r = (np.cumsum if op == "sum" else np.cumprod)(x, dtype=work.dtype)[1:]  # sequential, left to right, in the column's type
            r = r if is_f else r.view(a.dtype)
        else:
            if is_f:
                x = np.concatenate([np.array([s], a.dtype), np.where(ok, a, a.dtype.type(np.nan))])
                m = (np.fmax if op == "max" else np.fmin).accumulate(x)  # NaN is skipped
                r = _latest_zero_sign(x, m)[1:]
            else:
                info = np.iinfo(a.dtype)
                x = np.concatenate([np.array([s], a.dtype), np.where(ok, a, a.dtype.type(info.min if op == "max" else info.max))])
                r = (np.maximum if op == "max" else np.minimum).accumulate(x)[1:]
    out_valid = ok.copy() if skip_nulls else np.logical_and.accumulate(ok) if n else ok.copy()
    return r, out_valid


def fill_null(a, valid, backward=False):
    a = np.asarray(a)
    n = len(a)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    if backward:
        r, v = fill_null(a[::-1], ok[::-1])
        return r[::-1].copy(), v[::-1].copy()
    if n == 0:
        return a.copy(), ok.copy()
    last = np.maximum.accumulate(np.where(ok, np.arange(n), -1))
    return a[np.maximum(last, 0)], last >= 0


def shift(a, valid, periods, fill=None):
    a = np.asarray(a)
    n = len(a)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    r = np.full(n, 0 if fill is None else fill, a.dtype)
    v = np.full(n, fill is not None, bool)
    p = int(periods)
    if abs(p) < n:
        if p >= 0:
            r[p:], v[p:] = a[:n - p], ok[:n - p]
        else:
            r[:n + p], v[:n + p] = a[-p:], ok[-p:]
    return r, v


def same_special(got, want):
    """NaN, +inf and -inf in the same rows (a NaN's sign and payload are not compared)"""
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
            and np.array_equal(np.isneginf(got), np.isneginf(want)))


def _dyadic(x):
    """a finite float as (n, s): x == n / 2**s"""
    n, d = float(x).as_integer_ratio()
    return n, d.bit_length() - 1


def bound_violations(op, got, a, valid, start, rows=None):
    """Rows where a float running sum / product leaves the bound that holds for ANY order of evaluation (Higham, Accuracy and Stability of
    Numerical Algorithms, 4.2): |got_i - E_i| <= g(k_i - 1) * S_i, g(m) = m u / (1 - m u), k_i = valid terms up to row i with the start,
    S_i = |start| + sum |x_j| (sum) or |E_i| (product).  Exact arithmetic: every float is a dyadic rational, so E_i is kept as an integer
    times a power of two (the same numbers as fractions.Fraction would hold, without its gcd per operation).
    -> ([(row, error / (u * S_i))], largest error / (u * S_i)); rows whose result is finite, up to the first non-finite input."""
    a = np.asarray(a)
    p = 53 if a.dtype == np.float64 else 24
    ok = np.ones(len(a), bool) if valid is None else np.asarray(valid, bool)
    s0 = float(cast_start(float(start), a.dtype))
    if not np.isfinite(s0):
        return [], 0.0
    shift_ = 1200  # sums: everything on the grid 2**-1200 (finer than the smallest float64 subnormal)
    n0, e0 = _dyadic(s0)
    if op == "sum":
        exact = n0 << (shift_ - e0)
        mag = abs(exact)
    else:
        exact, exact_s = n0, e0
    k = 1
    want = None if rows is None else set(int(r) for r in rows)
    bad, worst = [], 0.0
    for i in range(len(a)):
        if ok[i]:
            if not np.isfinite(a[i]):  # no exact value behind a NaN / infinity: those rows are held by same_special
                break
            n, e = _dyadic(a[i])
            k += 1
            if op == "sum":
                x = n << (shift_ - e)
                exact += x
                mag += abs(x)
            else:
                exact *= n
                exact_s += e
        if not ok[i] or (want is not None and i not in want) or not np.isfinite(got[i]):
            continue
        g, gs = _dyadic(got[i])
        if op == "sum":
            err, scale = abs((g << (shift_ - gs)) - exact), mag
        elif exact_s >= gs:
            err, scale = abs((g << (exact_s - gs)) - exact), abs(exact)
        else:
            err, scale = abs(g - (exact << (gs - exact_s))), abs(exact << (gs - exact_s))
        ratio = ((err << (p + 16)) // scale) / 65536.0 if scale else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        if err * ((1 << p) - (k - 1)) > (k - 1) * scale:  # err > (k - 1) u / (1 - (k - 1) u) * scale
            bad.append((i, ratio))
    return bad, worst
