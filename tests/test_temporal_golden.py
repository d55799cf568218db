"""CPU-only: tests/_temporal_ref.py (plain numpy / datetime) equals Arrow C++ 25's temporal kernels bit for bit on
tests/golden/temporal_golden.npz (tools/gen_golden_temporal.py).  This checks both the golden file and the reference the GPU tests
use for inputs the file does not hold."""
import os

import numpy as np
import pytest

import _temporal_ref as R
from conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "temporal_golden.npz"))
ROUND_CASES = sorted({k.split("_", 2)[2] for k in G.files if k.startswith("round_")})


def same_bits(got, exp):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    assert np.array_equal(got.view(np.uint8), exp.view(np.uint8))


def test_golden_file_holds_every_kernel_and_edge():
    assert all("comp_" + c in G.files for c in R.COMPONENTS if c != "week")
    assert all(f"week_{a}{b}{c}" in G.files for a in (0, 1) for b in (0, 1) for c in (0, 1))
    assert all("between_" + u in G.files for u in R.BETWEEN_UNITS)
    assert {c.split("_")[0] for c in ROUND_CASES} == set(R.UNITS[:10])
    ts = G["ts"]
    for t in (-1, 0, 1, np.iinfo(np.int64).max, np.iinfo(np.int64).min + 1):
        assert t in ts
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "temporal_golden.npz")) < 600 * 1024


@pytest.mark.parametrize("name", [c for c in R.COMPONENTS if c != "week"])
def test_component(name):
    same_bits(R.component(name, G["ts"]), G["comp_" + name])


@pytest.mark.parametrize("opts", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])
def test_week_options(opts):
    same_bits(R.week(G["ts"], *map(bool, opts)), G["week_%d%d%d" % opts])


def test_named_weeks_are_week_options():
    same_bits(G["week_100"], G["comp_iso_week"])
    same_bits(G["week_000"], G["comp_us_week"])


def test_iso_calendar_is_the_single_components():
    same_bits(np.stack([R.component(c, G["ts"]) for c in ("iso_year", "iso_week", "iso_day_of_week")], axis=1), G["isocal"])


def test_known_instants():
    """-1 ns is 1969-12-31 23:59:59.999999999, a Wednesday in ISO week 1 of 1970."""
    one = np.array([-1], np.int64)
    got = {c: R.component(c, one)[0] for c in R.COMPONENTS}
    assert (got["year"], got["month"], got["day"], got["hour"], got["minute"], got["second"]) == (1969, 12, 31, 23, 59, 59)
    assert (got["millisecond"], got["microsecond"], got["nanosecond"], got["subsecond"]) == (999, 999, 999, 0.999999999)
    assert (got["day_of_week"], got["iso_day_of_week"], got["iso_year"], got["iso_week"], got["day_of_year"]) == (2, 3, 1970, 1, 365)


@pytest.mark.parametrize("unit", R.BETWEEN_UNITS)
def test_between(unit):
    same_bits(R.between(unit, G["ts"], G["b_ts"]), G["between_" + unit])


@pytest.mark.parametrize("case", ROUND_CASES)
def test_round(case):
    unit, mult, wsm, cbo = case.split("_")
    mult, wsm, cbo = int(mult), bool(int(wsm)), bool(int(cbo))
    ts = G["r_ts"]
    f, c, r = (G[f"round_{how}_{case}"] for how in ("floor", "ceil", "round"))
    same_bits(R.nearest(ts, f, c), r)  # the tie rule, for every option set (calendar origins included)
    if not cbo:
        same_bits(R.floor_temporal(ts, mult, unit, wsm), f)
        same_bits(R.ceil_temporal(ts, mult, unit, wsm), c)
        same_bits(R.round_temporal(ts, mult, unit, wsm), r)


def test_round_ties_present():
    """the file holds exact ties (t - floor == ceil - t) for the fixed units and shows them going up"""
    ts = G["r_ts"]
    for unit in ("second", "minute", "hour", "day", "week"):
        f, c, r = (G[f"round_{how}_{unit}_1_1_0"] for how in ("floor", "ceil", "round"))
        tie = (ts - f == c - ts) & (c > f)
        assert tie.any(), unit
        assert np.array_equal(r[tie], c[tie])
