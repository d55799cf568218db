#!/usr/bin/env python3
"""Generate tests/golden/elementwise_golden.npz -- Arrow's answers for the element-wise family (add .. shift_right, equal .. greater_equal,
if_else, negate .. bit_wise_not, power, cast, and / or / invert) on every dtype pair, at every path edge of csrc/elementwise.hip.

TEST INFRASTRUCTURE.  Arrow 25.0.0 through pyarrow.compute, fed SLICED arrays (pa.array(frame).slice(off, n)) so that its own offset
handling is the one recorded.  The file stores RECIPES, not arrays (tests/_elementwise_cases.py regenerates every input): family, op,
pair, scalar side, n, offsets, seed, kind and either a 64-bit blake2b digest of the result (dtype, validity bits, value bytes with null
rows zeroed; tests/_elementwise_ref.digest) or Arrow's error message.  `sign` of an integer is recorded after widening Arrow's int8
result to int64.  exp / power are recorded as the class of every value (finite sign, zero sign, inf sign, NaN): the numbers follow the
host's libm and are compared within LIBM_TOL_ULP.

For every recipe the numpy reference (tests/_elementwise_ref.py) must give Arrow's digest or message -- the generator stops where it
does not: Arrow wins, the reference is what gets corrected.

Mutation condition (decided on the reference alone, tests/_elementwise_cases.mutants): every applicable wrong kernel must change the
digest or the message; the seeds 1 .. 49 are searched for the first one under which all of them do.  A recipe that none separates is
dropped and listed in manifest["dropped"]: at most 2 % may be, no (family, pair, side) may lose a size, no large recipe may go.

Run:  python oracle/gen_golden_elementwise.py [out.npz]      (several minutes; the output is byte-identical from run to run)
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
import _elementwise_cases as EC  # noqa: E402
import _elementwise_ref as R  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "elementwise_golden.npz")
PA_TYPE = {"i32": pa.int32(), "i64": pa.int64(), "f32": pa.float32(), "f64": pa.float64(), "u64": pa.uint64(), "bool": pa.bool_()}
BINARY = ["add", "subtract", "multiply", "divide", "bit_wise_or", "bit_wise_and", "bit_wise_xor", "shift_left", "shift_right"]
COMPARE = ["equal", "not_equal", "less", "less_equal", "greater", "greater_equal"]
UNARY = ["negate", "abs", "sign", "sqrt", "exp", "bit_wise_not"]
MAX_SEED = 50


def pa_operand(x):
    """the frame as an Arrow array, sliced; a length-1 operand as the scalar at that position"""
    arr = pa.array(x.buf, type=PA_TYPE[x.t], mask=None if x.vbuf is None else ~x.vbuf).slice(x.off, x.n)
    return arr


def pa_scalar(x):
    return pa_operand(x)[0]


def result_arrays(r, tname):
    """-> (values, valid) read from the result's buffers (no conversion may touch a NaN payload)"""
    n = len(r)
    vb, data = r.buffers()
    valid = np.ones(n, bool) if vb is None else np.unpackbits(np.frombuffer(vb, np.uint8), bitorder="little")[r.offset:r.offset + n].astype(bool)
    if pa.types.is_boolean(r.type):
        v = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")[r.offset:r.offset + n].astype(bool)
    else:
        v = np.frombuffer(data, r.type.to_pandas_dtype())[r.offset:r.offset + n]
        if v.dtype != R.NP[tname]:  # sign of an integer: Arrow's int8 / uint8 widened to int64
            assert tname == "i64" and v.dtype.itemsize == 1, (v.dtype, tname)
            v = v.astype(np.int64)
    return v, valid


def arrow(recipe, ops):
    """-> (values, valid) or raises pa.ArrowInvalid / pa.ArrowNotImplementedError"""
    family, op, ta, tb, side, n, oi, seed, kind = recipe
    a = ops["a"]
    if family in ("binary", "compare", "if_else"):
        x = pa_scalar(a) if side == 2 else pa_operand(a)
        y = pa_scalar(ops["b"]) if side == 1 else pa_operand(ops["b"])
        if family == "binary":
            return pc.call_function(BINARY[op], [x, y])
        if family == "compare":
            return pc.call_function(COMPARE[op], [x, y])
        return pc.if_else(pa_operand(ops["cond"]), x, y)
    x = pa_operand(a)
    if family == "unary":
        return pc.call_function(UNARY[op], [x])
    if family == "power":
        return pc.power(x, pa.scalar(EC.EXPONENTS[op], pa.float64()))
    if family == "cast":
        return pc.cast(x, PA_TYPE[tb])
    if family == "cast_f64":
        return pc.cast(x, pa.float64(), safe=bool(op))
    if family == "logical":
        return pc.call_function("and" if op == R.AND else "or", [x, pa_operand(ops["b"])])
    return pc.invert(x)


def outcome(fn):
    """-> ('ok', digest) | ('error', message)"""
    try:
        v, ok, tname, libm = fn()
    except (R.RefError, pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
        return "error", str(e).splitlines()[0]
    return "ok", R.digest(v, ok, tname, libm)


def record(recipe):
    """-> (seed, mutant mask, 'ok' | 'error', digest | message), seed None when no seed separates every applicable mutant"""
    family, op, ta, tb, side, n, oi, _, kind = recipe
    for seed in range(1, MAX_SEED):
        rec = recipe[:7] + (seed, kind)
        ops = EC.inputs(rec)
        want = outcome(lambda: EC.reference(rec, ops))
        live, same = EC.mutant_outcomes(rec, ops, want, outcome)
        if not same or n > 100_000:
            break
    else:
        return None, kind, live, None, same
    assert not same, (recipe, same)  # (a large recipe must separate at its first seed: change the generators, not the rule)

    def from_arrow():
        tname, libm = EC.result_type(rec)
        v, ok = result_arrays(arrow(rec, ops), tname)
        return v, ok, tname, libm

    got = outcome(from_arrow)
    if got != want and kind == "small" and family == "binary" and R.is_float(R.promote(ta, tb)) and got[0] == want[0] == "ok":
        to = R.promote(ta, tb)
        v, ok, _, _ = EC.reference(rec, ops)
        av, aok = result_arrays(arrow(rec, ops), to)
        both = np.broadcast_to(R.is_nan(R.plain_cast(ops["a"].values, ta, to)), (n,)) & np.broadcast_to(R.is_nan(R.plain_cast(ops["b"].values, tb, to)), (n,))
        differ = (R.bits(v) != R.bits(av)) & ok
        assert np.array_equal(ok, aok) and not (differ & ~both).any(), f"reference != arrow outside both-NaN rows: {rec}"
        # Arrow's own choice between two NaN operands is not the documented one here: the recipe gives both-NaN rows one payload
        return record(recipe[:8] + ("small_eqnan",))
    assert got == want, f"reference != arrow: {rec}: reference {want}, arrow {got}"
    return seed, kind, live, got[0], got[1]


def write_npz(path, store):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(store[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    recipes = EC.all_recipes()
    rows, dropped, messages = [], [], []
    import multiprocessing

    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:  # (order is kept: the output does not depend on the worker count)
        results = pool.map(record, recipes, chunksize=64)
    for i, (rec, (seed, kind, live, status, val)) in enumerate(zip(recipes, results)):
        rec = rec[:8] + (kind,)
        if seed is None:
            dropped.append([*map(lambda x: x if isinstance(x, str) else int(x), rec[:7]), rec[8], sorted(val)])
            continue
        if status == "error":
            if val not in messages:
                messages.append(val)
            rows.append(rec[:7] + (seed, rec[8], live, 0, messages.index(val)))
        else:
            rows.append(rec[:7] + (seed, rec[8], live, val, -1))
        if rec[5] > 100_000 or i % 5000 == 0:
            print(i, len(recipes), rec, status, flush=True)
    assert len(dropped) * 50 <= len(recipes), f"{len(dropped)} of {len(recipes)} recipes dropped"
    assert not any(d[7] == "large" for d in dropped), dropped
    kept = {(r[0], r[2], r[3], r[4], r[5]) for r in rows if r[8].startswith("small")}
    lost = {(r[0], r[2], r[3], r[4], r[5]) for r in recipes if r[8] == "small"} - kept
    assert not lost, sorted(lost)
    types = ["", "i32", "i64", "f32", "f64", "u64"]
    store = {"family": np.array([EC.FAMILIES.index(r[0]) for r in rows], np.int8), "op": np.array([r[1] for r in rows], np.int8),
             "ta": np.array([types.index(r[2]) for r in rows], np.int8), "tb": np.array([types.index(r[3]) for r in rows], np.int8),
             "side": np.array([r[4] for r in rows], np.int8), "n": np.array([r[5] for r in rows], np.int64),
             "oi": np.array([r[6] for r in rows], np.int8), "seed": np.array([r[7] for r in rows], np.int8),
             "kind": np.array([EC.KINDS.index(r[8]) for r in rows], np.int8), "mutants": np.array([r[9] for r in rows], np.uint32),
             "digest": np.array([r[10] for r in rows], np.uint64), "error": np.array([r[11] for r in rows], np.int16)}
    manifest = {"arrow_version": pa.__version__, "families": list(EC.FAMILIES), "kinds": list(EC.KINDS), "types": types, "messages": messages,
                "sizes": list(EC.SIZES), "offsets": [list(o) for o in EC.OFFSETS], "cond_offsets": list(EC.COND_OFFSETS),
                "mutants": list(EC.MUTANTS), "generated": len(recipes), "dropped": dropped,
                "nan_rule_exceptions": [[*map(lambda x: x if isinstance(x, str) else int(x), r[:8])] for r in rows if r[8] == "small_eqnan"]}
    store["manifest"] = np.array(json.dumps(manifest))
    write_npz(OUT, store)
    print(f"wrote {OUT}: {len(rows)} recipes ({len(dropped)} dropped of {len(recipes)}), {os.path.getsize(OUT)} bytes; arrow {pa.__version__}")


if __name__ == "__main__":
    main()
