"""Multi-key sort: the restatement of Arrow's sort_indices that the GPU tests compare against, and the seeded case grid shared by the golden
generator (tools/gen_golden_multisort.py), the CPU check of the restatement (tests/test_multisort_golden.py) and the GPU tests.

Restatement: pc.sort_indices(table, sort_keys=[(name, order), ...]) with default null placement is a STABLE lexicographic sort; per key
first the class (numbers < NaN < null in BOTH orders), then the value (-0.0 == 0.0; descending reverses only the numbers); rows that tie
on every key keep their row order.  np.lexsort over (class, dense rank) pairs says exactly that.

A key column is (values ndarray, valid bool ndarray, kind) with kind in KINDS; "ts" values are int64 nanoseconds.  The inputs come from a
counter-based generator written out below (splitmix64 over the row number), so they do not depend on numpy's own generators; the golden
file pins a digest of every case's inputs next to Arrow's answer."""
import hashlib

import numpy as np

KINDS = ("f64", "i64", "u64", "ts", "i32", "f32")
NP_DTYPE = {"f64": np.float64, "i64": np.int64, "u64": np.uint64, "ts": np.int64, "i32": np.int32, "f32": np.float32}


# ---------------------------------------------------------------- the restatement
def key_class_rank(values, valid, descending):
    """-> (class, dense rank of the value among the numbers in the wanted order; 0 where the row is no number)"""
    values = np.asarray(values)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    if values.dtype.kind == "f":
        nan = np.isnan(values)
        x = np.where(nan | (values == 0), values.dtype.type(0), values)  # -0.0 == 0.0
    else:
        nan = np.zeros(len(values), bool)
        x = values
    cls = np.where(~valid, 2, np.where(nan, 1, 0))
    xs = np.where(cls == 0, x, x.dtype.type(0))
    u, inv = np.unique(xs, return_inverse=True)
    r = inv.reshape(-1).astype(np.int64)
    if descending:
        r = len(u) - 1 - r
    return cls, np.where(cls == 0, r, 0)


def sort_indices_ref(cols, descending):
    """cols: [(values, valid | None, ...)], descending: one flag per key -> the int64 row numbers in sorted order"""
    n = len(cols[0][0])
    if n == 0:
        return np.zeros(0, np.int64)
    ks = []
    for col, d in zip(reversed(list(cols)), reversed(list(descending))):  # np.lexsort: the LAST key is the primary one
        c, r = key_class_rank(col[0], col[1], d)
        ks += [r, c]
    return np.lexsort(ks).astype(np.int64)


# ---------------------------------------------------------------- the generator
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix(seed, stream, n):
    """n uint64 words: splitmix64 of (row number + a start that depends on seed and stream); uint64 arithmetic wraps"""
    start = (int(seed) * 0x9E3779B97F4A7C15 + int(stream) * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(start)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform(seed, stream, n):
    return (splitmix(seed, stream, n) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def pick(seed, stream, n, k):
    """n integers in [0, k)"""
    return (splitmix(seed, stream, n) % np.uint64(k)).astype(np.int64)


_WIDE = {
    "f64": np.array([-1e308, -1.5, -0.0, 0.0, 5e-324, 1e308], np.float64),
    "f32": np.array([-3e38, -1.5, -0.0, 0.0, 1e-45, 3e38], np.float32),  # 1e-45: the smallest float32 denormal
    "i64": np.array([-2**63, -1, 0, 1, 2**63 - 1, 12345], np.int64),
    "u64": np.array([0, 1, 2**63, 2**64 - 1, 7, 2**63 - 1], np.uint64),
    "ts": np.array([-2**63, 0, 1_600_000_000_000_000_000, 1_600_000_001_000_000_000, 2**63 - 1, 86_400_000_000_000], np.int64),
    "i32": np.array([-2**31, -1, 0, 1, 2**31 - 1, 77], np.int32),
}


def make_column(seed, stream, n, kind, nulls, wide=False, fine=False):
    """Few distinct values (so that later keys and the row order decide); floats carry NaN, -0.0 and inf; `wide`: values that span the
    whole range of the dtype; `fine`: more distinct values."""
    s = stream * 8
    if wide:
        v = _WIDE[kind][pick(seed, s, n, 6)]
    elif kind in ("f64", "f32"):
        v = ((pick(seed, s, n, 61) - 30) / 8.0 if fine else (pick(seed, s, n, 7) - 3).astype(np.float64)).astype(NP_DTYPE[kind])
    elif kind == "u64":
        v = pick(seed, s, n, 1000 if fine else 4).astype(np.uint64)
    elif kind == "ts":
        v = 1_700_000_000_000_000_000 + pick(seed, s, n, 86400 if fine else 5) * 1_000_000_000
    else:
        v = (pick(seed, s, n, 1000 if fine else 6) - 3).astype(NP_DTYPE[kind])
    v = np.ascontiguousarray(v, dtype=NP_DTYPE[kind])
    if kind in ("f64", "f32"):
        u = uniform(seed, s + 1, n)
        v[u < 0.10] = np.nan
        v[(u >= 0.10) & (u < 0.20)] = -0.0
        v[(u >= 0.20) & (u < 0.24)] = np.inf
        v[(u >= 0.24) & (u < 0.26)] = -np.inf
    valid = uniform(seed, s + 2, n) > 0.15 if nulls else np.ones(n, bool)
    return v, valid, kind


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + b"\0" + str(a.shape).encode() + b"\0" + a.tobytes())
    return h.hexdigest()


def case_digest(cols, descending):
    parts = []
    for v, valid, kind in cols:
        parts += [v, np.asarray(valid, bool), np.frombuffer(kind.encode(), np.uint8)]
    return digest(*parts, np.asarray(descending, bool))


GOLDEN_NS = (0, 1, 2, 17, 1000, 40003)
GOLDEN_KEYS = (1, 2, 3, 9)
FULL_OUTPUT_MAX_N = 1000  # the golden file keeps Arrow's whole answer up to this many rows and its digest for every case


def golden_cases():
    """-> [(name, cols, descending)]: n x number of keys x nulls x 3 trials over all six dtypes and mixed orders, plus one 16-key case"""
    out = []
    seed = 0
    for n in GOLDEN_NS:
        for nk in GOLDEN_KEYS:
            for nulls in (False, True):
                for trial in range(3):
                    seed += 1
                    kinds = pick(seed, 1000, nk, len(KINDS))
                    flags = pick(seed, 1001, nk, 2)
                    shape = pick(seed, 1002, nk, 8)
                    cols = [make_column(seed, k, n, KINDS[kinds[k]], nulls, wide=shape[k] == 0, fine=(k == nk - 1 or shape[k] == 1)) for k in range(nk)]
                    out.append((f"n{n}_k{nk}_{'nulls' if nulls else 'dense'}_t{trial}", cols, [bool(f) for f in flags]))
    seed += 1
    kinds = pick(seed, 1000, 16, len(KINDS))
    cols = [make_column(seed, k, 1000, KINDS[kinds[k]], True, wide=k in (3, 11), fine=k == 15) for k in range(16)]
    out.append(("n1000_k16_nulls", cols, [bool(f) for f in pick(seed, 1001, 16, 2)]))
    return out
