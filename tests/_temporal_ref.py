"""Plain Python / numpy restatement of Arrow's temporal kernels on timestamp[ns] (no time zone): the calendar components, the
*_between family and floor / ceil / round_temporal.  Independent of the library (numpy's datetime64 fields, datetime.date.isocalendar)
and of pyarrow, so it runs wherever the tests run; tests/test_temporal_golden.py holds it to Arrow C++ 25's own output bit for bit
(tests/golden/temporal_golden.npz), and tests/test_gpu_temporal.py then uses it as the reference for inputs the golden file does not hold."""
import datetime

import numpy as np

NS_DAY = 86400 * 10**9
COMPONENTS = ["year", "month", "day", "day_of_week", "day_of_year", "hour", "minute", "second", "millisecond", "microsecond", "nanosecond",
              "quarter", "iso_week", "iso_year", "iso_day_of_week", "us_week", "us_year", "week", "is_leap_year", "subsecond"]  # pdx_temporal_component order
UNIT_NS = {"nanosecond": 1, "microsecond": 10**3, "millisecond": 10**6, "second": 10**9, "minute": 60 * 10**9, "hour": 3600 * 10**9,
           "day": NS_DAY, "week": 7 * NS_DAY}
UNITS = ["nanosecond", "microsecond", "millisecond", "second", "minute", "hour", "day", "week", "month", "quarter", "year"]  # pdx_calendar_unit order
BETWEEN_UNITS = [u for u in UNITS if u != "month"]
_EPOCH_ORD = datetime.date(1970, 1, 1).toordinal()


def _i64(a):
    return np.asarray(a).astype(np.int64)


def _fields(ts):
    t = _i64(ts)
    day = (t // NS_DAY).view("M8[D]")  # (numpy's own ns -> D conversion overflows within a day of the int64 minimum)
    return t, day, day.astype("M8[M]"), day.astype("M8[Y]")


def _per_day(daynum, fn):
    """fn(datetime.date) -> tuple of ints, evaluated once per distinct day."""
    u, inv = np.unique(daynum, return_inverse=True)
    vals = np.array([fn(datetime.date.fromordinal(int(d) + _EPOCH_ORD)) for d in u], dtype=np.int64).reshape(len(u), -1)
    return vals[inv]


def _week_year(d, week_starts_monday, count_from_zero, first_week_is_fully_in_year):
    """Arrow's Week functor on one date -> (year of the week, week number)."""
    def start_of(y):
        if first_week_is_fully_in_year:  # the first Monday / Sunday of the year
            s = datetime.date(y, 1, 1)
            want = 0 if week_starts_monday else 6  # date.weekday(): Monday = 0
            return s + datetime.timedelta((want - s.weekday()) % 7)
        s = datetime.date(y - 1, 12, 31)  # four days after the last Thursday / Wednesday of the December before
        want = 3 if week_starts_monday else 2
        return s - datetime.timedelta((s.weekday() - want) % 7) + datetime.timedelta(4)

    y = (d if first_week_is_fully_in_year or count_from_zero else d + datetime.timedelta(3)).year  # counting from zero stays in d's own year
    start = start_of(y)
    if not count_from_zero and d < start:
        y -= 1
        start = start_of(y)
    return y, (d - start).days // 7 + 1


def week(ts, week_starts_monday=True, count_from_zero=False, first_week_is_fully_in_year=False):
    t, day, _, _ = _fields(ts)
    return _per_day(_i64(day), lambda d: _week_year(d, week_starts_monday, count_from_zero, first_week_is_fully_in_year))[:, 1]


def component(name, ts, week_options=(True, False, False)):
    """One component: int64, bool (is_leap_year) or float64 (subsecond) ndarray."""
    t, day, mon, yr = _fields(ts)
    daynum = _i64(day)
    tod = t - daynum * NS_DAY
    year = _i64(yr) + 1970
    if name == "year":
        return year
    if name == "month":
        return _i64(mon) % 12 + 1
    if name == "quarter":
        return _i64(mon) % 12 // 3 + 1
    if name == "day":
        return _i64(day - mon.astype("M8[D]")) + 1
    if name == "day_of_year":
        return _i64(day - yr.astype("M8[D]")) + 1
    if name == "day_of_week":  # Arrow's default DayOfWeekOptions: Monday = 0
        return (daynum + 3) % 7
    if name == "iso_day_of_week":
        return (daynum + 3) % 7 + 1
    if name == "is_leap_year":
        return (year % 4 == 0) & ((year % 100 != 0) | (year % 400 == 0))
    if name == "hour":
        return tod // (3600 * 10**9)
    if name == "minute":
        return tod // (60 * 10**9) % 60
    if name == "second":
        return tod // 10**9 % 60
    if name == "millisecond":
        return tod // 10**6 % 1000
    if name == "microsecond":
        return tod // 10**3 % 1000
    if name == "nanosecond":
        return tod % 1000
    if name == "subsecond":
        return (tod % 10**9).astype(np.float64) / 1e9
    if name in ("iso_year", "iso_week"):
        return _per_day(daynum, lambda d: tuple(d.isocalendar()))[:, 0 if name == "iso_year" else 1]
    if name in ("us_year", "us_week"):  # the week (from Sunday) belongs to the year of its Wednesday
        wed = daynum - (daynum + 4) % 7 + 3
        wy = wed.view("M8[D]").astype("M8[Y]")
        return _i64(wy) + 1970 if name == "us_year" else _i64(wed.view("M8[D]") - wy.astype("M8[D]")) // 7 + 1
    if name == "week":
        return week(ts, *week_options)
    raise KeyError(name)


def between(unit, a, b):
    """Arrow's <unit>s_between(a, b): unit boundaries crossed from a to b."""
    def index(ts):
        t, day, mon, yr = _fields(ts)
        if unit == "year":
            return _i64(yr)
        if unit == "quarter":
            return _i64(mon) // 3
        if unit == "week":  # weeks start on Monday; 1970-01-01 was a Thursday
            return (_i64(day) + 3) // 7
        return t // UNIT_NS[unit]
    return index(b) - index(a)


def floor_temporal(ts, multiple, unit, week_starts_monday=True):
    """floor_temporal with the multiples counted from the epoch (calendar_based_origin = false)."""
    t, _, mon, _ = _fields(ts)
    if unit in ("month", "quarter"):
        k = multiple * (3 if unit == "quarter" else 1)
        return _i64((_i64(mon) // k * k).view("M8[M]").astype("M8[ns]"))
    p = multiple * UNIT_NS[unit]
    org = (3 if week_starts_monday else 4) * NS_DAY if unit == "week" else 0
    return (t + org) // p * p - org


def ceil_temporal(ts, multiple, unit, week_starts_monday=True):
    t = _i64(ts)
    f = floor_temporal(ts, multiple, unit, week_starts_monday)
    if unit in ("month", "quarter"):
        k = multiple * (3 if unit == "quarter" else 1)
        return _i64((_i64(f.view("M8[ns]").astype("M8[M]")) + k).view("M8[M]").astype("M8[ns]"))
    return np.where(f >= t, f, f + multiple * UNIT_NS[unit])


def nearest(ts, f, c):
    """round_temporal from the floor and the ceil under the same options: the ceil on a tie."""
    t = _i64(ts)
    return np.where(t - f >= c - t, c, f)


def round_temporal(ts, multiple, unit, week_starts_monday=True):
    return nearest(ts, floor_temporal(ts, multiple, unit, week_starts_monday), ceil_temporal(ts, multiple, unit, week_starts_monday))
