"""CPU tests of the element-wise test kit: the numpy reference (tests/_elementwise_ref.py) against Arrow's recorded results
(tests/golden/elementwise_golden.npz, tests/golden/narrow_golden.npz) and against the C oracle on the 64-bit pairs; the mutation
condition of every recipe; and the launch constants of csrc/elementwise.hip that place the sizes."""
import json
import os
import re

import numpy as np
import pytest

import _elementwise_cases as EC
import _elementwise_ref as R
from conftest import ROOT
from test_gpu_round2 import LIBM_TOL_ULP

Z = np.load(os.path.join(ROOT, "tests", "golden", "elementwise_golden.npz"))
MANIFEST = json.loads(str(Z["manifest"]))


def _recipes():
    t, f, k = MANIFEST["types"], MANIFEST["families"], MANIFEST["kinds"]
    cols = [Z[x].tolist() for x in ("family", "op", "ta", "tb", "side", "n", "oi", "seed", "kind", "digest", "error", "mutants")]
    return [((f[a], b, t[c], t[d], e, n, oi, s, k[kd]), dg, er, mu) for a, b, c, d, e, n, oi, s, kd, dg, er, mu in zip(*cols)]


RECIPES = _recipes()
GROUPS = EC.groups()


def _outcome(fn):
    try:
        v, ok, tname, libm = fn()
    except R.RefError as e:
        return "error", str(e)
    return "ok", R.digest(v, ok, tname, libm)


def test_source_constants():
    """the constants that place the sizes of the recipes, read from the sources: one that moves fails here instead of moving an edge out
    from under the tests"""
    csrc = os.path.join(ROOT, "pandasarrow_amd", "csrc")
    common = open(os.path.join(csrc, "pdx_common.hpp")).read()
    ew = open(os.path.join(csrc, "elementwise.hip")).read()
    cus = int(re.search(r"constexpr int kCUs = (\d+);", common).group(1))
    mult = int(re.search(r"int grid_for\(int64_t work_items, int block, int items_per_thread = 1, int max_blocks = kCUs \* (\d+)\)", common).group(1))
    assert (cus, mult) == (256, 8)
    cap = cus * mult  # workgroups
    # k_binary_n, k_if_else_n (n) and k_unary_n (a->length): one workgroup of 256 lanes per 1024 rows
    assert len(re.findall(r"grid_for\(n, 256, 4\)", ew)) == 2 and len(re.findall(r"grid_for\(a->length, 256, 4\)", ew)) == 1
    assert ew.count("__launch_bounds__(256)") == 4
    threads = cap * 256
    assert threads == 524_288 and threads * 4 == EC.GRID_CAP_ROWS == 2_097_152
    # the vector loop: a 4-row group per thread and round, then n & 3 rows; thread 0's second round starts at GRID_CAP_ROWS
    assert "const int64_t n4 = vec ? (n >> 2) : 0;" in ew and "const int64_t n4 = kNarrow && vec ? (n >> 2) : 0;" in ew
    assert ew.count("int64_t i = (n4 << 2) + tid") == 2
    assert all(n > EC.GRID_CAP_ROWS + 3 for n in (EC.ERROR_SIZES[-1],)) and EC.ERROR_SIZES[-1] & 3
    # the row-per-lane form of an 8-byte pair: 4x unrolled while i + 3 * stride < n
    assert "if constexpr (sizeof(TA) == 8 && sizeof(TB) == 8) {" in ew and "for (; i + 3 * stride < n; i += 4 * stride) {" in ew
    assert 7 * threads == EC.UNROLL_SECOND_TRIP
    # k_compare_n: a wave owns 4096-row tiles, four waves per workgroup, at most cap * 4 waves
    assert "const int64_t ntiles = (n + 4095) >> 12;" in ew and "const int64_t base = t << 12;" in ew
    assert "grid_for(((n + 4095) >> 12) * 64, 256)" in ew
    assert ew.count("base + 4096 <= n") == 2 and "constexpr bool kNarrow = sizeof(TA) == 4 || sizeof(TB) == 4;" in ew
    assert cap * 4 * 4096 == EC.BITMAP_CAP_ROWS == 33_554_432
    # the bitmap kernels: one thread per 64-row word
    assert ew.count("grid_for(nwords, 256)") == 2 and ew.count("int64_t nwords = (n + 63) >> 6;") == 4
    assert threads * 64 == EC.BITMAP_CAP_ROWS
    assert "for (int64_t w = tid; w < ((n + 63) >> 6); w += stride) {" in ew  # (k_if_else_n's validity half: the 4-rows-per-thread grid)
    # alignment: every array operand and the output; the scalar side is not looked at
    assert "const int vec = aligned16(out) && (scalar == 2 || aligned16(pa)) && (scalar == 1 || aligned16(pb));" in ew
    assert "const int vec = aligned16(pa) && (scalar || aligned16(pb));" in ew
    assert "const int vec = aligned16(in) && aligned16(out->values);" in ew
    for a, b in EC.OFFSETS[:2]:
        assert a % 4 == 0 and b % 4 == 0
    for a, b in EC.OFFSETS[2:]:
        assert a % 2 or b % 2
    for o in EC.OFFSETS[1:]:  # (all but the (0, 0) pair differ mod 8 and mod 64 between the operands)
        assert (o[0] - o[1]) % 8 and (o[0] - o[1]) % 64
    assert tuple(MANIFEST["sizes"]) == EC.SIZES and [tuple(o) for o in MANIFEST["offsets"]] == list(EC.OFFSETS)


def test_manifest():
    assert MANIFEST["arrow_version"] == "25.0.0"
    assert MANIFEST["mutants"] == list(EC.MUTANTS)
    dropped = MANIFEST["dropped"]
    print(f"{len(dropped)} of {MANIFEST['generated']} recipes dropped; NaN-rule exceptions: {MANIFEST['nan_rule_exceptions']}")
    assert len(dropped) * 50 <= MANIFEST["generated"] and len(dropped) + len(RECIPES) == MANIFEST["generated"]
    assert not any(d[7] == "large" for d in dropped)
    want = EC.all_recipes()
    kept = {(r[0][0], r[0][2], r[0][3], r[0][4], r[0][5]) for r in RECIPES}
    assert {(r[0], r[2], r[3], r[4], r[5]) for r in want} == kept  # no (family, pair, scalar side) lost a size
    gone = {tuple(d[:7]) for d in dropped}
    assert [r[:7] for r in want if r[:7] not in gone] == [r[0][:7] for r in RECIPES]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "elementwise_golden.npz")) < 1_000_000


@pytest.mark.parametrize("group", GROUPS + [("large",)], ids=["-".join(map(str, g)).rstrip("-0") or "x" for g in GROUPS] + ["large"])
def test_reference_reproduces_recipes_and_mutants_differ(group):
    """the reference gives Arrow's digest or message for every recipe, and every applicable wrong kernel (EC.MUTANTS) gives another"""
    if group == ("large",):
        mine = [r for r in RECIPES if r[0][8] == "large"]
    else:
        mine = [r for r in RECIPES if (r[0][0], r[0][2], r[0][3], r[0][4]) == group and r[0][8] != "large"]
    assert mine
    cache = {}
    for rec, digest, err, mask in mine:
        key = EC.input_key(rec)
        ops = cache.get(key) or EC.inputs(rec)
        if rec[5] < 100_000:
            cache[key] = ops  # (the ops of a class share their inputs)
        got = _outcome(lambda: EC.reference(rec, ops))
        want = ("ok", digest) if err < 0 else ("error", MANIFEST["messages"][err])
        assert got == want, rec
        live, same = EC.mutant_outcomes(rec, ops, want, _outcome)
        assert live == mask and not same, (rec, live, mask, same)


NARROW = np.load(os.path.join(ROOT, "tests", "golden", "narrow_golden.npz"))
NARROW_CASES = json.loads(str(NARROW["manifest"]))["cases"]


def _same(case, got, ok, ev, eok, ulp=0):
    assert np.array_equal(ok, eok), case
    assert got.dtype == ev.dtype or ev.dtype == np.int8, (case, got.dtype, ev.dtype)
    g, e = got[ok], ev[ok].astype(got.dtype)
    if ulp:
        cg, ce = R.float_class(g), R.float_class(e)
        assert np.array_equal(cg, ce), case
        fin = ce < 2
        assert (R.ulp_distance(g[fin], e[fin]) <= ulp).all(), case
    else:
        assert np.array_equal(EC._raw(g), EC._raw(e)), (case, g, e)


@pytest.mark.parametrize("kind", ["binary", "compare", "if_else", "unary", "cast"])
def test_reference_reproduces_narrow_golden(kind):
    names = sorted(k for k, c in NARROW_CASES.items() if c["kind"] == kind)
    assert names
    for case in names:
        c = NARROW_CASES[case]
        a, av = NARROW[f"{case}/a"], NARROW[f"{case}/a_valid"]

        def run():
            if kind == "unary":
                return R.unary(c["op"], a, c["a"], av)
            if kind == "cast":
                return R.cast(a, c["a"], av, c["to"])
            b, bv = NARROW[f"{case}/b"], NARROW[f"{case}/b_valid"]
            if kind == "binary":
                return R.binary(c["op"], a, c["a"], av, b, c["b"], bv, c["side"])
            if kind == "compare":
                return R.compare(c["op"], a, c["a"], av, b, c["b"], bv, c["side"])
            return R.if_else(NARROW[f"{case}/cond"], NARROW[f"{case}/cond_valid"], a, c["a"], av, b, c["b"], bv, c["side"])

        if c["error"]:
            with pytest.raises(R.RefError) as ei:
                run()
            assert str(ei.value) == c["error"], case
            continue
        got, ok = run()
        _same(case, got, ok, NARROW[f"{case}/out"], NARROW[f"{case}/out_valid"], ulp=LIBM_TOL_ULP if kind == "unary" and c["op"] == R.EXP else 0)


@pytest.mark.parametrize("family", ["binary", "compare", "if_else", "unary"])
def test_reference_agrees_with_the_oracle_on_the_64_bit_pairs(family):
    """the C restatement (oracle/pdx_oracle.c) knows int64 / uint64 / float64: both restatements give the same bits at the small sizes"""
    import oracle as orc

    ran = 0
    for rec, digest, err, _ in RECIPES:
        fam, op, ta, tb, side, n, oi, seed, kind = rec
        if fam != family or kind != "small" or err >= 0 or oi not in (0, 4) or ta == "i32" or ta == "f32" or tb in ("i32", "f32"):
            continue
        ops = EC.inputs(rec)
        want, ok, tname, libm = EC.reference(rec, ops)
        a = ops["a"]
        if family == "unary":
            got, gok = orc.unary(op, a.values, a.valid), (np.ones(n, bool) if a.valid is None else a.valid)
        else:
            b = ops["b"]
            x = a.values[0] if side == 2 else a.values
            y = b.values[0] if side == 1 else b.values
            if family == "if_else":
                c = ops["cond"]
                if (side == 2 and a.valid is not None and not a.valid[0]) or (side == 1 and b.valid is not None and not b.valid[0]):
                    continue  # (the oracle spells a null scalar as None and then takes int64: only the typed form is compared)
                got, gok = orc.if_else(c.values, x, y, c.valid, a.valid, b.valid)
            else:
                got, gok = (orc.binary if family == "binary" else orc.compare)(op, x, y, a.valid, b.valid)
                gok = np.ones(n, bool) if gok is None else gok
        assert np.array_equal(gok, ok), rec
        got = np.asarray(got)
        if family == "binary" and tname == "f64":
            # where both operands are NaN the C oracle returns what its own compiler's x + y returns (for a scalar lhs the scalar's payload,
            # Arrow the array's): Arrow wins, the reference follows it, and such a row is compared as a NaN only
            both = np.broadcast_to(R.is_nan(R.plain_cast(a.values, ta, "f64")), (n,)) & np.broadcast_to(R.is_nan(R.plain_cast(b.values, tb, "f64")), (n,))
            assert R.is_nan(got)[both & ok].all(), rec
            ok = ok & ~both
        _same(rec, got, ok, want, ok, ulp=LIBM_TOL_ULP if libm else 0)
        ran += 1
    assert ran > 100
