"""Validity patterns, values and poisoned columns for the nullable-sum tests (test_nullruns_golden.py, test_gpu_nullruns.py,
oracle/gen_golden_nullruns.py).  Pure functions of (name, n) / (dtype, n, seed): no RNG state; randomness comes from the counter-based
generators of the oracle (synth_keys / synth_vals), which the library has too.

The sizes below follow from the launch geometry of sum_nullable (pandasarrow_amd/csrc/aggregate.hip):
  segments of SEG_ROWS rows, tiles of TILE_ROWS rows (4 segments), scan blocks of SCAN_TILE segments, EMIT_WAVES segments per emit
  workgroup and CUS * WGS_PER_CU emit workgroups, NULL_TILE_WAVES tiles per workgroup of the state kernel on a grid of at most CUS * 8.
test_nullruns_golden.py::test_source_constants pins every one of them to the sources.
"""
import ctypes as C

import numpy as np

import oracle as orc

SEG_ROWS, TILE_ROWS, SCAN_TILE, EMIT_WAVES, NULL_TILE_WAVES, CUS, WGS_PER_CU, GRID_CAP_PER_CU = 1024, 4096, 2048, 2, 4, 256, 6, 8
SCAN_EDGE = SCAN_TILE * SEG_ROWS                             # 2,097,152 rows: the last size whose segment scans fit one block
ROUND_EDGE = CUS * WGS_PER_CU * EMIT_WAVES * SEG_ROWS        # 3,145,728 rows: every emit wave takes exactly one segment
STATE_EDGE = CUS * GRID_CAP_PER_CU * NULL_TILE_WAVES * TILE_ROWS  # 33,554,432 rows: one grid-stride round of the state kernel

PERIODS = (17, 33, 1013, 1025, 2049, 4097, 65537)
LARGE_ONLY = ("scan_edge", "round_edge")
PATTERNS = (["all_valid_bitmap", "early_null", "late_null", "last_row_null", "ends", "seg_first", "seg_last", "tile_first", "tile_last"]
            + [f"period_{p}" for p in PERIODS]
            + ["runs_1_40", "word_bit0", "word_bit63", "alt_words", "null_segments", "null_tiles", "null_head", "null_tail", "all_null",
               "one_valid_last", "one_valid_first", "one_valid_per_segment", "random8"] + list(LARGE_ONLY))
DTYPES = ("f64", "f32", "i64", "i32")
NP_T = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32}
SUM, MEAN, MIN, MAX, COUNT = 0, 1, 2, 3, 4
KINDS = (SUM, MEAN, MIN, MAX, COUNT)
TAIL_ROWS = 130  # poisoned rows (validity bits set) behind every column


def _nulls_at(n, rows):
    valid = np.ones(n, bool)
    rows = np.asarray(rows, np.int64)
    valid[rows[(rows >= 0) & (rows < n)]] = False
    return valid


def validity(name, n):
    """bool[n], True = valid.  Null rows outside [0, n) are dropped."""
    if name == "all_valid_bitmap":
        return np.ones(n, bool)
    if name == "early_null":
        return _nulls_at(n, [5])
    if name == "late_null":
        return _nulls_at(n, [n - 3])
    if name == "last_row_null":
        return _nulls_at(n, [n - 1])
    if name == "ends":
        return _nulls_at(n, [0, n - 1])
    if name == "scan_edge":
        return _nulls_at(n, [5, SCAN_EDGE - 1, SCAN_EDGE, SCAN_EDGE + 1])
    if name == "round_edge":
        return _nulls_at(n, [5, ROUND_EDGE - 1, ROUND_EDGE])
    if name.startswith("period_"):
        return _nulls_at(n, np.arange(0, n, int(name[7:])))
    i = np.arange(n, dtype=np.int64)
    if name in ("seg_first", "seg_last", "tile_first", "tile_last", "word_bit0", "word_bit63"):
        period = {"seg": SEG_ROWS, "tile": TILE_ROWS, "word": 64}[name.split("_")[0]]
        return i % period != (0 if name.endswith(("first", "bit0")) else period - 1)
    if name == "runs_1_40":  # valid runs of 1, 2, ..., 40 rows, one null behind each, then again from 1
        ends = np.cumsum(np.arange(1, 41) + 1) - 1
        return ~np.isin(i % int(ends[-1] + 1), ends)
    if name == "alt_words":
        return (i >> 6) % 2 == 0
    if name == "null_segments":
        return (i < 3 * SEG_ROWS + 7) | (i >= 5 * SEG_ROWS + 9)
    if name == "null_tiles":
        return (i < 2 * TILE_ROWS - 3) | (i >= 4 * TILE_ROWS + 5)
    if name == "null_head":
        return i >= n // 2
    if name == "null_tail":
        return i < n - n // 2
    if name == "all_null":
        return np.zeros(n, bool)
    if name == "one_valid_last":
        return i == n - 1
    if name == "one_valid_first":
        return i == 0
    if name == "one_valid_per_segment":
        return i % SEG_ROWS == (7 * (i // SEG_ROWS)) % SEG_ROWS
    if name == "random8":
        return orc.synth_keys(3, n, 12) != 0
    raise KeyError(name)


def values(dtype, n, seed):
    """Zero-mean values over 41 binades (the scaling by a power of two is exact): two groupings of the same rows rarely round alike.
    f32: the same rounded once; i64: round(value * 2^40), up to 2^59, so partial sums pass 2^53; i32: uniform in [-2^30, 2^30) --
    every partial sum of such a column is exact in float64, so that dtype checks the handling of validity only."""
    if dtype == "i32":
        return (orc.synth_keys(seed, n, 1 << 31) - (1 << 30)).astype(np.int32)
    v = np.ldexp(orc.synth_vals(0, n, seed) - 0.5, (orc.synth_keys(seed, n, 41) - 20).astype(np.int32))  # (value - 0.5) * 2^(key - 20)
    if dtype == "f32":
        return v.astype(np.float32)
    if dtype == "i64":
        return np.rint(v * 2.0 ** 40).astype(np.int64)
    return v


def poison(dtype, m, kind):
    """m values that must never be read: kind 0 = quiet NaN (integers: the minimum), kind 1 = the largest magnitudes with alternating sign"""
    t = NP_T[dtype]
    if dtype in ("i64", "i32"):
        lo, hi = np.iinfo(t).min, np.iinfo(t).max
        out = np.full(m, lo, t)
        if kind:
            out[1::2] = hi
        return out
    if not kind:
        return np.full(m, np.nan, t)
    out = np.full(m, 1e300 if dtype == "f64" else 3e38, t)
    out[1::2] *= -1
    return out


def poisoned(dtype, v, valid, kind):
    return np.where(valid, v, poison(dtype, len(v), kind)).astype(NP_T[dtype])


def column(K, L, torch, dtype, v, valid, offset=0, kind=0, misalign=0, null_count=-1):
    """A device Column that is a slice of a longer allocation: `offset` rows in front and TAIL_ROWS behind, all of them poison with their
    validity bits SET, and poison under every null row: a read outside [offset, offset + n) or of a null row shows in the result.
    misalign: the validity bytes start that many bytes past an 8-byte boundary (a byte-offset view of a larger uint8 tensor)."""
    n = len(v)
    host = poison(dtype, offset + n + TAIL_ROWS, kind)
    np.copyto(host[offset:offset + n], np.asarray(v, host.dtype), where=valid)
    bits = np.ones(offset + n + TAIL_ROWS, bool)
    bits[offset:offset + n] = valid
    packed = np.concatenate([np.packbits(bits, bitorder="little"), np.full(16, 0xFF, np.uint8)])
    dev = torch.device("cuda", torch.cuda.current_device())
    raw = torch.empty(len(packed) + 16, dtype=torch.uint8, device=dev)
    start = (-raw.data_ptr()) % 8 + misalign
    vb = raw[start:start + len(packed)]
    vb.copy_(torch.from_numpy(packed))
    assert vb.data_ptr() % 8 == misalign % 8
    code = {"f64": L.FLOAT64, "f32": L.FLOAT32, "i64": L.INT64, "i32": L.INT32}[dtype]
    return K.Column(code, n, torch.from_numpy(host).to(dev), vb, offset, null_count)


# ------------------------------------------------------------------ results as bit patterns
def encode(dtype, kind, value):
    """-> (is_null, uint64 bit pattern): float results (float32 extremes held widened) as float64 bits, integer results as int64"""
    if value is None:
        return True, 0
    if kind == MEAN or (dtype in ("f64", "f32") and kind != COUNT):
        return False, int(np.array([value], np.float64).view(np.uint64)[0])
    return False, int(np.array([int(value)], np.int64).view(np.uint64)[0])


def wide(dtype, v):
    """the column as the oracle takes it: float32 -> float64, int32 -> int64 (both exact)"""
    return np.asarray(v).astype(np.float64 if dtype in ("f64", "f32") else np.int64)


def oracle_results(dtype, v, valid):
    """the five aggregates from the CPU oracle -> (is_null bool[5], bits uint64[5]).  (The calls of oracle.agg, with the column widened
    and its bitmap packed once for all five: at 3e7 rows that is most of the time.)"""
    w, n = np.ascontiguousarray(wide(dtype, v)), len(v)
    lib, vb, cnt = orc.lib(), orc.pack_bits(valid), C.c_int64(0)
    isf = w.dtype == np.float64
    T = C.c_double if isf else C.c_int64
    s, m, lo, hi = T(0), C.c_double(0), T(0), T(0)
    args = (orc._p(w), orc._p(vb), orc._i64(0), orc._i64(n))
    (lib.orc_sum_f64 if isf else lib.orc_sum_i64)(*args, C.byref(s), C.byref(cnt))
    (lib.orc_mean_f64 if isf else lib.orc_mean_i64)(*args, C.byref(m), C.byref(cnt))
    (lib.orc_minmax_f64 if isf else lib.orc_minmax_i64)(*args, C.byref(lo), C.byref(hi), C.byref(cnt))
    count = int(lib.orc_count(orc._p(vb), orc._i64(0), orc._i64(n)))
    assert count == cnt.value
    res = [encode(dtype, k, x.value if count else None) for k, x in zip(KINDS, (s, m, lo, hi))] + [encode(dtype, COUNT, count)]
    return np.array([r[0] for r in res], bool), np.array([r[1] for r in res], np.uint64)


# ------------------------------------------------------------------ wrong groupings (the mutation condition)
MUTANT_ROWS = [k * m for m in (16, 64, SEG_ROWS, TILE_ROWS) for k in (1, 2, 3)] + [SCAN_EDGE, ROUND_EDGE]
N_MUTANTS = 1 + len(MUTANT_ROWS)  # [0]: the unshifted grid; [1 + j]: one more run split in front of row MUTANT_ROWS[j]


def mutant_sums(dtype, v, valid, which=None):
    """-> {mutant index: tree sum under that wrong grouping} for the mutants the pattern admits (restricted to `which` when given).
    (a) index 0: nulls replaced by 0.0 and summed dense (the leaves never restart).  (b) index 1 + j: one null row with value 0 inserted
    in front of row r = MUTANT_ROWS[j] (one valid run split in two), only where rows [r - 8, r + 8) are all valid."""
    n = len(v)
    w = np.asarray(v).astype(np.float64)
    out = {}
    if which is None or 0 in which:
        out[0] = orc.agg(SUM, np.where(valid, w, 0.0))[0]
    for j, r in enumerate(MUTANT_ROWS):
        if (which is not None and 1 + j not in which) or r < 8 or r + 8 > n or not valid[r - 8:r + 8].all():
            continue
        out[1 + j] = orc.agg(SUM, np.insert(w, r, 0.0), np.insert(valid, r, False))[0]
    return out


def f64_bits(x):
    return None if x is None else int(np.array([x], np.float64).view(np.uint64)[0])


def separated(dtype, v, valid, which=None):
    """-> {mutant index: True when the wrong grouping's result differs in bits from the true one}.  int64: the results compared are the
    means (tree sum / valid count), which is where pdx_aggregate uses the tree for that dtype."""
    w = np.asarray(v).astype(np.float64)
    true, cnt = orc.agg(SUM, w, valid)
    if not cnt:
        return {}
    div = float(cnt) if dtype == "i64" else 1.0
    return {k: f64_bits(s / div) != f64_bits(true / div) for k, s in mutant_sums(dtype, v, valid, which).items()}


# ------------------------------------------------------------------ which wrong groupings are groupings of their own
def _mix(a, b):
    """uint64 stand-in for the float add: 0 is the identity on both sides (as 0.0 is), but it is neither associative nor commutative and
    nothing is ever absorbed, so two groupings give the same result only if they are the same expression"""
    return a + b + a * b * (a - b)


def grouping_hash(valid, x):
    """Arrow's nullable sum (16-value leaves from every run's start, binary-counter merge, low-to-high fold: oracle/pdx_oracle.c pw_*)
    over uint64 x with _mix in place of the add; x must be 0 wherever a row is to count as absent"""
    idx = np.flatnonzero(valid)
    if not len(idx):
        return 0
    k = np.arange(len(idx))
    newrun = np.ones(len(idx), bool)
    newrun[1:] = idx[1:] != idx[:-1] + 1
    pos = k - np.maximum.accumulate(np.where(newrun, k, 0))  # position inside the run
    leaf_start = np.flatnonzero(pos % 16 == 0)
    leaf_len = np.diff(np.append(leaf_start, len(idx)))
    xs = x[idx]
    with np.errstate(over="ignore"):
        level = np.zeros(len(leaf_start), np.uint64)
        for q in range(16):
            m = leaf_len > q
            level[m] = _mix(level[m], xs[leaf_start[m] + q])
        left = []  # what the counter still holds at every level (0: nothing)
        while len(level) > 1:
            left.append(level[-1] if len(level) & 1 else np.uint64(0))
            level = level[:len(level) & ~1]
            level = _mix(level[0::2], level[1::2])
        levels = left + [level[0]]
        s = levels[0]
        for held in levels[1:]:  # fold low -> high: sum[i] = merge(sum[i], sum[i - 1])
            s = _mix(held, s)
    return int(s)


def required_mutants(valid, large_dense=True):
    """-> bit mask of the wrong groupings of mutant_sums that are groupings of their own, decided from the validity alone.
    (b) a split in front of row r is the same grouping exactly when r lies on a leaf edge of its run, (r - run start) % 16 == 0: the
    leaves and their order stay what they were.  (a) the dense grid is compared with the true one as expressions (grouping_hash on two
    assignments of odd 64-bit numbers): it is the same one when every run starts on a multiple of 16 and the all-null 16-row blocks
    between them do not move a leaf to another place in the tree, when there is one valid row, when the only nulls trail the last run.
    large_dense=False leaves (a) out above 1e6 rows (the CPU test: the expression evaluation of 3e7 rows takes seconds)."""
    n = len(valid)
    mask = 0
    if valid.any() and not valid.all() and (large_dense or n <= 1_000_000):
        for seed in (11, 12):
            x = orc.synth_keys(seed, n, 1 << 62).astype(np.uint64) * np.uint64(2) + np.uint64(1)
            if grouping_hash(valid, x) != grouping_hash(np.ones(n, bool), np.where(valid, x, np.uint64(0))):
                mask |= 1
    nulls = np.flatnonzero(~valid)
    for j, r in enumerate(MUTANT_ROWS):
        if r < 8 or r + 8 > n or not valid[r - 8:r + 8].all():
            continue
        p = np.searchsorted(nulls, r)
        start = int(nulls[p - 1]) + 1 if p else 0
        if (r - start) % 16:
            mask |= 1 << (1 + j)
    return mask
