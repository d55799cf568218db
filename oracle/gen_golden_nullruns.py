#!/usr/bin/env python3
"""Generate tests/golden/nullruns_golden.npz -- Arrow's sum / mean / min / max / count of nullable columns whose nulls are STRUCTURED
(tests/_nullruns.py): single nulls in long valid runs, nulls on word / segment / tile edges, whole null segments and tiles, at sizes on
both sides of every launch boundary of the nullable-sum kernels.

TEST INFRASTRUCTURE.  As gen_golden.py: pc.sum / mean / min / max / count on pa.array(v, mask=~valid), Arrow 25.0.0 through pyarrow.
The file stores RECIPES, not arrays: pattern, n, dtype, seed, poison kind and the five results as bit patterns; every input is
regenerated from tests/_nullruns.py.

Mutation condition (checked on the CPU oracle alone).  A float sum only pins the leaf grid if a wrong grid gives other bits.  For every
float64 / float32 / int64 case the oracle's result is also computed under the wrong groupings of _nullruns.mutant_sums -- (a) the
unshifted grid, (b) one extra run split at row k * 16 / 64 / 1024 / 4096 (k = 1, 2, 3), 2,097,152 and 3,145,728, where rows
[r - 8, r + 8) are valid -- and the seeds 1, 2, ... 199 are searched for the first one under which every one of them differs in bits
from the true result.  A wrong grouping that is the SAME expression as the true one can never differ and is not required; that is
decided from the validity alone (_nullruns.required_mutants): a split on a leaf edge of its run, (r - run start) % 16 == 0, leaves every
leaf and the tree as they were; the dense grid is compared with the true grouping as an expression (one valid row, nulls that only
trail the last run, runs that all start on multiples of 16 with no all-null block moving a leaf in the tree).  `mutants` is the bit
mask of the required ones.  A case with none is kept and counted in manifest["no_distinct_grouping"]: its other four results and its
validity handling are still checked.  A case whose required mutants no seed below 200 separates all at once is dropped and listed in
manifest["dropped"]; at most 5 % may be, and no pattern may lose all its sizes.  all_null, all_valid_bitmap and int32 (exact in float64
under every grouping) are exempt.

Run:  python oracle/gen_golden_nullruns.py [out.npz]          (a few minutes; the output is byte-identical from run to run)
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _nullruns as NR  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "nullruns_golden.npz")
SMALL_SIZES = [1, 15, 16, 17, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5123, 65553]
FAMILIES = ["small", "scan", "pass", "emit", "state", "child"]
MAX_SEED = 200


def case_list():
    """[(family, pattern, n, dtype)] in file order (the poison kind of a case is its position's parity)"""
    out = [("small", p, n, dt) for dt in NR.DTYPES for n in SMALL_SIZES for p in NR.PATTERNS if p not in NR.LARGE_ONLY]
    out += [("scan", p, n, dt) for dt in ("f64", "i64") for n in (NR.SCAN_EDGE, NR.SCAN_EDGE + 1)
            for p in ("early_null", "period_1025", "null_head", "scan_edge", "random8")]
    out += [("pass", p, 6_300_007, "f64") for p in ("early_null", "ends", "scan_edge", "round_edge")]
    out += [("emit", p, n, dt) for dt in ("f64", "f32") for n in (NR.ROUND_EDGE, NR.ROUND_EDGE + 1, 3_150_855)
            for p in ("early_null", "seg_last", "period_2049", "null_tiles", "round_edge", "random8")]
    out += [("state", p, NR.STATE_EDGE + 3 * NR.TILE_ROWS + 5, "f32") for p in ("early_null", "period_65537")]
    out += [("child", p, n, "f64") for n in (524_288, 524_289, 3_150_855) for p in ("early_null", "period_1025", "null_segments")]
    return out


_vals = {}


def values(dtype, n, seed):
    key = (dtype, n, seed)
    if key not in _vals:
        if n > 100_000 and len(_vals) > 8:
            _vals.clear()
        _vals[key] = NR.values(dtype, n, seed)
    return _vals[key]


_required = {}


def pick_seed(pattern, n, dtype, valid):
    """-> (seed | None when dropped, required-mutant bit mask)"""
    if dtype == "i32" or pattern in ("all_null", "all_valid_bitmap"):
        return 1, 0
    if (pattern, n) not in _required:
        _required[(pattern, n)] = NR.required_mutants(valid)
    mask = _required[(pattern, n)]
    live = [k for k in range(NR.N_MUTANTS) if mask >> k & 1]
    if not live:
        return 1, 0
    for s in range(1, MAX_SEED):
        sep = NR.separated(dtype, values(dtype, n, s), valid, which=live)
        if sorted(sep) == live and all(sep.values()):
            return s, mask
    return None, mask


def arrow_results(dtype, pv, valid):
    a = pa.array(pv, mask=~valid)
    res = []
    for kind, fn in zip(NR.KINDS, (pc.sum, pc.mean, pc.min, pc.max, pc.count)):
        res.append(NR.encode(dtype, kind, fn(a).as_py()))
    return np.array([r[0] for r in res], bool), np.array([r[1] for r in res], np.uint64)


def write_npz(path, store):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(store[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    cases = case_list()
    rows, dropped, vacuous = [], [], 0
    validities = {}
    for idx, (family, pattern, n, dtype) in enumerate(cases):
        if (pattern, n) not in validities:
            if n > 100_000:
                validities.clear()
            validities[(pattern, n)] = NR.validity(pattern, n)
        valid = validities[(pattern, n)]
        seed, mask = pick_seed(pattern, n, dtype, valid)
        if seed is None:
            dropped.append([family, pattern, n, dtype])
            print("dropped", family, pattern, n, dtype, hex(mask), flush=True)
            continue
        if not mask and dtype != "i32" and pattern not in ("all_null", "all_valid_bitmap"):
            vacuous += 1
        kind = idx & 1
        v = values(dtype, n, seed)
        isnull, bits = arrow_results(dtype, NR.poisoned(dtype, v, valid, kind), valid)
        onull, obits = NR.oracle_results(dtype, v, valid)
        assert np.array_equal(isnull, onull) and np.array_equal(bits, obits), f"oracle != arrow: {family} {pattern} n={n} {dtype} seed={seed}: {bits} vs {obits}"
        rows.append((FAMILIES.index(family), NR.PATTERNS.index(pattern), n, NR.DTYPES.index(dtype), seed, kind, mask, int(valid.sum()), isnull, bits))
        if n > 100_000:
            print(f"{family:6s} {pattern:14s} n={n:9d} {dtype} seed={seed} mutants={mask:#x}", flush=True)
    assert len(dropped) * 20 <= len(cases), f"{len(dropped)} of {len(cases)} cases dropped"
    kept = {NR.PATTERNS[r[1]] for r in rows}
    assert kept == set(NR.PATTERNS), sorted(set(NR.PATTERNS) - kept)
    store = {"family": np.array([r[0] for r in rows], np.int8), "pattern": np.array([r[1] for r in rows], np.int16),
             "n": np.array([r[2] for r in rows], np.int64), "dtype": np.array([r[3] for r in rows], np.int8),
             "seed": np.array([r[4] for r in rows], np.int16), "poison": np.array([r[5] for r in rows], np.int8),
             "mutants": np.array([r[6] for r in rows], np.uint32), "count": np.array([r[7] for r in rows], np.int64),
             "isnull": np.array([r[8] for r in rows], bool), "exp": np.array([r[9] for r in rows], np.uint64)}
    manifest = {"arrow_version": pa.__version__, "patterns": list(NR.PATTERNS), "dtypes": list(NR.DTYPES), "families": FAMILIES,
                "small_sizes": SMALL_SIZES, "mutant_rows": NR.MUTANT_ROWS, "generated": len(cases), "dropped": dropped,
                "no_distinct_grouping": vacuous,
                "cases": {f: [i for i, r in enumerate(rows) if r[0] == k] for k, f in enumerate(FAMILIES)}}
    store["manifest"] = np.array(json.dumps(manifest))
    write_npz(OUT, store)
    print(f"wrote {OUT}: {len(rows)} cases ({len(dropped)} dropped, {vacuous} without a distinct wrong grouping), {os.path.getsize(OUT)} bytes; "
          f"arrow {pa.__version__}")


if __name__ == "__main__":
    main()
