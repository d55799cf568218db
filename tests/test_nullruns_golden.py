"""CPU: the oracle equals Arrow C++ 25 on every recipe of tests/golden/nullruns_golden.npz (oracle/gen_golden_nullruns.py) -- sum / mean /
min / max / count of columns with STRUCTURED nulls at sizes around every launch boundary of the nullable-sum kernels -- bit for bit; the
recipes still tell a wrong leaf grid from the right one (the mutation condition, re-checked here from the recipes alone); and the
constants those sizes were derived from still have their values in the sources.  No pyarrow, no GPU."""
import os
import re

import numpy as np
import pytest

import _nullruns as NR
from conftest import ROOT, Golden

GOLD = Golden("nullruns_golden.npz")
M = GOLD.manifest
Z = {k: GOLD.z[k] for k in ("family", "pattern", "n", "dtype", "seed", "poison", "mutants", "count", "isnull", "exp")}


def recipe(i):
    return (M["patterns"][Z["pattern"][i]], int(Z["n"][i]), M["dtypes"][Z["dtype"][i]], int(Z["seed"][i]), int(Z["poison"][i]))


def _groups():
    """the cases in chunks of one family (the small ones: one dtype of one family)"""
    out = []
    for fam in M["families"]:
        ids = GOLD.cases(fam)
        for dt in (M["dtypes"] if fam == "small" else [None]):
            out.append(pytest.param([i for i in ids if dt is None or M["dtypes"][Z["dtype"][i]] == dt], id=fam + ("" if dt is None else "-" + dt)))
    return out


def test_golden_covers_what_the_generator_promises():
    assert M["arrow_version"].startswith("25.")
    assert M["patterns"] == list(NR.PATTERNS) and M["dtypes"] == list(NR.DTYPES) and M["mutant_rows"] == NR.MUTANT_ROWS
    total = len(Z["n"])
    assert total + len(M["dropped"]) == M["generated"] and len(M["dropped"]) * 20 <= M["generated"], M["dropped"]
    assert {M["patterns"][p] for p in Z["pattern"]} == set(NR.PATTERNS)  # no pattern lost all its sizes
    dropped = {tuple(d) for d in M["dropped"]}

    def have(fam):
        return {recipe(i)[:3] for i in GOLD.cases(fam)} | {d[1:] for d in dropped if d[0] == fam}

    small = [p for p in NR.PATTERNS if p not in NR.LARGE_ONLY]
    assert have("small") == {(p, n, dt) for p in small for n in (1, 15, 16, 17, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5123, 65553) for dt in NR.DTYPES}
    assert have("scan") == {(p, n, dt) for p in ("early_null", "period_1025", "null_head", "scan_edge", "random8") for n in (2_097_152, 2_097_153)
                            for dt in ("f64", "i64")}
    assert have("pass") == {(p, 6_300_007, "f64") for p in ("early_null", "ends", "scan_edge", "round_edge")}
    assert have("emit") == {(p, n, dt) for p in ("early_null", "seg_last", "period_2049", "null_tiles", "round_edge", "random8")
                            for n in (3_145_728, 3_145_729, 3_150_855) for dt in ("f64", "f32")}
    assert have("state") == {(p, 33_554_432 + 3 * 4096 + 5, "f32") for p in ("early_null", "period_65537")}
    assert have("child") == {(p, n, "f64") for p in ("early_null", "period_1025", "null_segments") for n in (524_288, 524_289, 3_150_855)}
    # every large case with a long valid run keeps the unshifted grid AND at least one run split among its required mutants
    for fam in M["families"][1:]:
        for i in GOLD.cases(fam):
            if recipe(i)[0] in ("early_null", "ends", "scan_edge", "round_edge", "period_1025", "period_2049", "period_65537", "null_tiles", "null_segments"):
                assert Z["mutants"][i] & 1 and Z["mutants"][i] >> 1, recipe(i)
    # poison: NaN in the even-numbered cases, the huge values in the odd ones -- both kinds occur in every family
    for fam in M["families"]:
        assert {int(Z["poison"][i]) for i in GOLD.cases(fam)} == {0, 1}, fam


@pytest.mark.parametrize("ids", _groups())
def test_oracle_equals_arrow(ids):
    """all five kinds; the oracle never sees the poison (it gets the clean values): Arrow got the poisoned ones"""
    for i in ids:
        pattern, n, dtype, seed, _ = recipe(i)
        valid = NR.validity(pattern, n)
        isnull, bits = NR.oracle_results(dtype, NR.values(dtype, n, seed), valid)
        assert int(valid.sum()) == int(Z["count"][i]), recipe(i)
        assert np.array_equal(isnull, Z["isnull"][i]) and np.array_equal(bits[~isnull], Z["exp"][i][~isnull]), (recipe(i), bits, Z["exp"][i])


_required = {}


@pytest.mark.parametrize("ids", _groups())
def test_mutation_condition(ids):
    """under the recorded seed every required wrong grouping (the unshifted grid, one more run split) gives other bits than the right one;
    which ones are required is decided again here from the validity alone (above 1e6 rows: the run splits only, the expression
    comparison of the dense grid takes seconds there), so the recorded mask cannot quietly lose a grouping of its own"""
    for i in ids:
        pattern, n, dtype, seed, _ = recipe(i)
        which = [k for k in range(NR.N_MUTANTS) if int(Z["mutants"][i]) >> k & 1]
        if dtype == "i32" or pattern in ("all_null", "all_valid_bitmap"):
            assert not which
            continue
        valid = NR.validity(pattern, n)
        if (pattern, n) not in _required:
            _required[(pattern, n)] = NR.required_mutants(valid, large_dense=False)
        assert int(Z["mutants"][i]) | (n > 1_000_000) == _required[(pattern, n)] | (n > 1_000_000), recipe(i)
        if not which:
            continue
        sep = NR.separated(dtype, NR.values(dtype, n, seed), valid, which=which)
        assert sorted(sep) == which and all(sep.values()), (recipe(i), sep)


def test_mutation_condition_has_teeth():
    """most cases do pin the grid: those without a distinct wrong grouping are the tiny and the (nearly) empty ones"""
    pinned = np.count_nonzero(Z["mutants"])
    checked = sum(1 for i in range(len(Z["n"])) if recipe(i)[2] != "i32" and recipe(i)[0] not in ("all_null", "all_valid_bitmap"))
    assert pinned + M["no_distinct_grouping"] == checked
    for i in range(len(Z["n"])):
        pattern, n, dtype, _, _ = recipe(i)
        if dtype != "i32" and n >= 1023 and pattern in ("early_null", "seg_first", "period_17", "period_33", "period_1013",
                                                       "runs_1_40", "word_bit0", "random8"):
            assert Z["mutants"][i] & 1, recipe(i)


def _constants(*files):
    """every `constexpr int[64_t] NAME = <product / sum / shift of numbers and earlier names>;` of the given sources"""
    env = {}
    for f in files:
        with open(os.path.join(ROOT, "pandasarrow_amd", "csrc", f)) as fh:
            text = fh.read()
        for name, expr in re.findall(r"constexpr\s+(?:int|int64_t)\s+(\w+)\s*=\s*([^;]+);", text):
            expr = expr.replace("(int64_t)", "")
            if re.fullmatch(r"[\w\s*+()<-]+", expr) and all(t.isdigit() or t in env for t in re.findall(r"\w+", expr)):
                env[name] = eval(expr, {"__builtins__": {}}, dict(env))  # noqa: S307 (numbers, names above, * + << only)
    return env


def test_source_constants():
    """the sizes of the golden file sit on the launch boundaries of sum_nullable only while these hold: a constant that moves must fail
    here, not quietly move a boundary out from under the sizes"""
    c = _constants("pdx_common.hpp", "scan.hpp", "aggregate.hip", "gb_seg_reduce.hpp")
    assert (c["kSegRows"], c["kLeafElems"], c["kScanTile"], c["kEmitWaves"], c["kNullTileWaves"], c["kCUs"]) == (
        NR.SEG_ROWS, NR.TILE_ROWS, NR.SCAN_TILE, NR.EMIT_WAVES, NR.NULL_TILE_WAVES, NR.CUS)
    assert c["kHugeNullable"] == 1 << 22  # the group size beyond which the group-by hands a nullable group to these kernels
    with open(os.path.join(ROOT, "pandasarrow_amd", "csrc", "aggregate.hip")) as fh:
        agg = fh.read()
    with open(os.path.join(ROOT, "pandasarrow_amd", "csrc", "pdx_common.hpp")) as fh:
        common = fh.read()
    # the emit launch: min(segments / kEmitWaves, kCUs * wgs_per_cu), wgs_per_cu = 6 unless the diagnostic knob says otherwise
    assert re.search(r'getenv\("PDX_NULLSUM_WGS_PER_CU"\);\s*return e && atoi\(e\) > 0 \? atoi\(e\) : (\d+);', agg).group(1) == str(NR.WGS_PER_CU)
    assert "ceil_div(ceil_div(n, kSegRows), kEmitWaves), (int64_t)kCUs * wgs_per_cu)" in agg
    # the state kernel's grid cap and the scans over 4 segments per tile
    assert f"hipLaunchKernelGGL(k_null_seg_state, dim3(std::min<unsigned>(grid, kCUs * {NR.GRID_CAP_PER_CU}))" in agg
    assert "nseg = ntiles * 4;" in agg and "ceil_div(ntiles, kNullTileWaves)" in agg
    assert f"int max_blocks = kCUs * {NR.GRID_CAP_PER_CU})" in common
    assert (NR.SCAN_EDGE, NR.ROUND_EDGE, NR.STATE_EDGE) == (2_097_152, 3_145_728, 33_554_432)
