"""Writes tests/golden/temporal_golden.npz: the output of every Arrow temporal kernel the dt accessor covers, from pyarrow 25
(Arrow C++ 25.0.0), on edge instants and a few thousand random ones.  Run on a machine with pyarrow: python tools/gen_golden_temporal.py

Arrays:  ts / b_ts (int64 ns): the operands of the components and of *_between (same length)
         comp_<name>, week_<monday><from_zero><fully_in_year>, isocal (n x 3), between_<unit>
         r_ts: the rounding operand (no instants so close to the ends of the range that a ceil would overflow)
         round_<floor|ceil|round>_<unit>_<multiple>_<monday>_<calendar_origin>"""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import _temporal_ref as R  # noqa: E402  (names only: the component and unit lists)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "temporal_golden.npz")
DAY = R.NS_DAY


def ns(s):
    return int(np.datetime64(s, "ns").astype(np.int64))


def edge_instants(january_sweep=True):
    e = [-1, 0, 1]
    for s in ("2019-12-31T23:59:59.999999999", "2020-01-01", "2020-02-29T23:59:59.999999999", "2020-03-01", "2021-06-30T23:59:59.999999999",
              "2021-07-01", "2021-07-01T12:59:59.999999999", "2021-07-01T13:00", "1969-12-31T23:00", "1969-12-31T22:59:59.999999999",
              "1970-01-01T00:59:59.999999999", "1970-01-01T01:00"):
        e.append(ns(s))
    for s in ("2000-02-29", "2000-02-29T23:59:59.999999999", "2000-03-01", "1900-02-28", "1900-02-28T23:59:59.999999999", "1900-03-01",
              "2100-02-28", "2100-02-28T23:59:59.999999999", "2100-03-01", "2000-12-31", "1900-12-31", "2024-12-31", "2023-12-31"):
        e.append(ns(s))
    for s in ("2018-12-31", "2020-12-31", "2021-01-03", "2024-12-30", "2026-01-01", "2015-12-31", "2016-01-03", "2010-01-03"):  # ISO edges
        e += [ns(s), ns(s) + DAY - 1]
    for y in range(1995, 2031) if january_sweep else (2017, 2023):  # the Sundays (and the days next to them) around 1 January, and the first week of every year
        j = ns(f"{y}-01-01")
        e += [j + k * DAY for k in range(-8, 9)]
    for s in ("1969-12-31T23:59:59.5", "1969-07-20T20:17:40.123456789", "1901-12-13T20:45:52.000000001", "1800-01-01T00:00:00.999999999",
              "1677-09-22T00:00:00.000000001", "1969-12-31T23:59:59.000000001"):  # before the epoch, with a sub-second part
        e.append(ns(s))
    lo, hi = np.iinfo(np.int64).min + 1, np.iinfo(np.int64).max  # (min itself is NaT in numpy)
    e += [lo, lo + 1, lo + DAY, ns("1677-09-22"), ns("1677-12-31T23:59:59"), hi, hi - 1, hi - DAY, ns("2262-04-11"), ns("2262-01-01")]
    return e


def main():
    rng = np.random.default_rng(20251017)
    lo, hi = np.iinfo(np.int64).min + 1, np.iinfo(np.int64).max
    ts = np.array(edge_instants() + list(rng.integers(lo, hi, 2400, endpoint=True)), np.int64)
    b_ts = np.concatenate([ts[7:], ts[:7]])  # pairs across the whole range ...
    near = rng.integers(0, len(ts), 1200)  # ... and pairs a few hours / days / months apart
    b_ts[near] = np.clip(ts[near].astype(object) + rng.integers(-400 * DAY, 400 * DAY, len(near)).astype(object), lo, hi).astype(np.int64)
    wraps = np.array([abs(int(y) - int(x)) >= 2**63 for x, y in zip(ts, b_ts)])  # a difference past int64 is outside the contract
    b_ts[wraps] = ts[wraps] // 2
    T, B = pa.array(ts, pa.timestamp("ns")), pa.array(b_ts, pa.timestamp("ns"))
    out = {"ts": ts, "b_ts": b_ts}
    for name in R.COMPONENTS:
        if name == "iso_day_of_week":  # Arrow has it as the third field of iso_calendar only
            out["comp_" + name] = pc.iso_calendar(T).field("iso_day_of_week").to_numpy()
        elif name != "week":
            out["comp_" + name] = getattr(pc, name)(T).to_numpy(zero_copy_only=False)
    for wsm in (0, 1):
        for cfz in (0, 1):
            for full in (0, 1):
                out[f"week_{wsm}{cfz}{full}"] = pc.week(T, week_starts_monday=bool(wsm), count_from_zero=bool(cfz),
                                                        first_week_is_fully_in_year=bool(full)).to_numpy()
    # (year_month_day is not recorded: the struct kernel of this pyarrow build returns corrupt month / day children past a few rows and
    # can crash; its fields are by definition the year / month / day kernels above, which is what the fused call is held to)
    iso = pc.iso_calendar(T)
    out["isocal"] = np.stack([iso.field(k).to_numpy() for k in ("iso_year", "iso_week", "iso_day_of_week")], axis=1)
    for unit in R.BETWEEN_UNITS:
        out["between_" + unit] = getattr(pc, unit + "s_between")(T, B).to_numpy()

    # rounding: instants within 1700 .. 2250, the edges that lie there, and exact ties of every unit
    r = [t for t in edge_instants(january_sweep=False) if ns("1700-01-01") < t < ns("2250-01-01")]
    r += list(rng.integers(ns("1700-01-01"), ns("2250-01-01"), 200))
    for base in (ns("2021-03-01"), ns("1969-12-29"), ns("1955-11-07")):  # (Mondays / a first of the month: origins of every unit)
        for u in ("microsecond", "millisecond", "second", "minute", "hour", "day", "week"):
            h = R.UNIT_NS[u] // 2
            r += [base + h, base + h - 1, base + h + 1, base + 3 * R.UNIT_NS[u] + h, base - h, base + R.UNIT_NS[u] * 5 // 2]
    r += [ns("2021-02-15"), ns("2021-02-14T23:59:59.999999999"), ns("2021-03-16T12:00"), ns("2021-03-16T11:59:59.999999999"),  # month ties
          ns("2021-02-15T00:00:00.000000001"), ns("2021-05-16T12:00"), ns("2021-08-16"), ns("2021-02-14T12:00"), ns("1969-11-16")]
    r_ts = np.array(r, np.int64)
    out["r_ts"] = r_ts
    RT = pa.array(r_ts, pa.timestamp("ns"))
    fns = {"floor": pc.floor_temporal, "ceil": pc.ceil_temporal, "round": pc.round_temporal}
    cases = [(u, 1, 1, 0) for u in R.UNITS[:10]] + [(u, m, 1, 0) for u, m in zip(R.UNITS[:10], (7, 250, 5, 15, 5, 6, 3, 2, 5, 2))]
    cases += [("week", 1, 0, 0), ("week", 2, 0, 0), ("hour", 5, 1, 1), ("day", 3, 1, 1), ("week", 2, 1, 1), ("week", 2, 0, 1), ("month", 5, 1, 1),
              ("quarter", 3, 1, 1), ("minute", 7, 1, 1)]
    for unit, mult, wsm, cbo in cases:
        for how, fn in fns.items():
            got = fn(RT, multiple=mult, unit=unit, week_starts_monday=bool(wsm), calendar_based_origin=bool(cbo))
            out[f"round_{how}_{unit}_{mult}_{wsm}_{cbo}"] = got.cast(pa.int64()).to_numpy()
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT) / 1024:.0f} KiB, pyarrow {pa.__version__}")


if __name__ == "__main__":
    main()
