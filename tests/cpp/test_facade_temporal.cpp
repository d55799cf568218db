// test_facade_temporal.cpp -- Series::dt() through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> C ABI -> HIP kernels): the known answers
// of the reference's "Test DateTimeLike" (tests/series_indexing_test.cpp:247-341) restated on the same four instants, the *_between
// family on the operands of its (commented-out) "between functions" case, rounding, nulls and the refusals.  Built with g++ (host code
// only) and run on the GPU box by tests/test_gpu_cpp_temporal.py.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "pdx.hpp"

static int g_checks = 0, g_failed = 0;
#define REQUIRE(cond)                                                              \
  do {                                                                             \
    ++g_checks;                                                                    \
    if (!(cond)) {                                                                 \
      ++g_failed;                                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);                \
    }                                                                              \
  } while (0)
#define REQUIRE_THROWS(expr)                                                       \
  do {                                                                             \
    ++g_checks;                                                                    \
    bool threw = false;                                                            \
    try { (void)(expr); } catch (const std::runtime_error&) { threw = true; }      \
    if (!threw) {                                                                  \
      ++g_failed;                                                                  \
      std::printf("FAILED %s:%d  expected std::runtime_error: %s\n", __FILE__, __LINE__, #expr); \
    }                                                                              \
  } while (0)
using namespace pd;
using I64 = std::vector<int64_t>;
using Flags = std::vector<bool>;

static const int64_t kSec = 1000000000LL, kHour = 3600 * kSec, kDay = 24 * kHour;
static const int64_t k2022 = 18993 * kDay;  // 2022-01-01T00:00:00 (a Saturday)

static Series stamps(const I64& v) {
  Array a = Array::Make(v);
  a.dtype = PDX_TIMESTAMP_NS;
  return Series(a);
}

// "2022-01-01T01:00:00" .. "2022-01-04T01:00:00"
static void test_components() {
  Series s = stamps({k2022 + kHour, k2022 + kDay + kHour, k2022 + 2 * kDay + kHour, k2022 + 3 * kDay + kHour});
  DateTimeLike dt = s.dt();
  REQUIRE((dt.day().values<int64_t>() == I64{1, 2, 3, 4}));
  REQUIRE((dt.day_of_week().values<int64_t>() == I64{5, 6, 0, 1}));
  REQUIRE((dt.day_of_year().values<int64_t>() == I64{1, 2, 3, 4}));
  REQUIRE((dt.hour().values<int64_t>() == I64{1, 1, 1, 1}));
  REQUIRE_THROWS(dt.is_dst());
  REQUIRE((dt.iso_week().values<int64_t>() == I64{52, 52, 1, 1}));
  REQUIRE((dt.iso_year().values<int64_t>() == I64{2021, 2021, 2022, 2022}));
  DataFrame iso = dt.iso_calendar();
  REQUIRE((iso.m_names == std::vector<std::string>{"iso_year", "iso_week", "iso_day_of_week"}));
  REQUIRE((iso["iso_year"].values<int64_t>() == I64{2021, 2021, 2022, 2022}));
  REQUIRE((iso["iso_week"].values<int64_t>() == I64{52, 52, 1, 1}));
  REQUIRE((iso["iso_day_of_week"].values<int64_t>() == I64{6, 7, 1, 2}));
  REQUIRE((dt.is_leap_year().values<bool>() == Flags{false, false, false, false}));
  REQUIRE((dt.microsecond().values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((dt.millisecond().values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((dt.minute().values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((dt.month().values<int64_t>() == I64{1, 1, 1, 1}));
  REQUIRE((dt.nanosecond().values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((dt.quarter().values<int64_t>() == I64{1, 1, 1, 1}));
  REQUIRE((dt.second().values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((dt.subsecond().values<double>() == std::vector<double>{0, 0, 0, 0}));
  REQUIRE((dt.us_week().values<int64_t>() == I64{52, 1, 1, 1}));
  REQUIRE((dt.us_year().values<int64_t>() == I64{2021, 2022, 2022, 2022}));
  REQUIRE((dt.year().values<int64_t>() == I64{2022, 2022, 2022, 2022}));
  DataFrame ymd = dt.year_month_day();  // (the reference's commented-out expectation: 2022 / 1 / 1)
  REQUIRE((ymd.m_names == std::vector<std::string>{"year", "month", "day"}));
  REQUIRE((ymd["year"].values<int64_t>() == I64{2022, 2022, 2022, 2022}));
  REQUIRE((ymd["month"].values<int64_t>() == I64{1, 1, 1, 1}));
  REQUIRE((ymd["day"].values<int64_t>() == I64{1, 2, 3, 4}));
  REQUIRE((dt.week().values<int64_t>() == I64{52, 52, 1, 1}));
  REQUIRE((dt.week(true, true, false).values<int64_t>() == I64{0, 0, 1, 1}));
  REQUIRE((dt.week(false, false, true).values<int64_t>() == I64{52, 1, 1, 1}));
}

// one nanosecond before the epoch: 1969-12-31 23:59:59.999999999, a leap-year check, an int64 Series through the cast, an index kept
static void test_floor_toward_minus_infinity_and_index() {
  Series idx(I64{10, 20, 30});
  Series s(Array::Make(I64{-1, 951782400 * kSec, 0}), idx.m_array, "t");  // -1 ns, 2000-02-29, the epoch (int64: dt() casts)
  DateTimeLike dt = s.dt();
  REQUIRE((dt.year().values<int64_t>() == I64{1969, 2000, 1970}));
  REQUIRE((dt.month().values<int64_t>() == I64{12, 2, 1}));
  REQUIRE((dt.day().values<int64_t>() == I64{31, 29, 1}));
  REQUIRE((dt.hour().values<int64_t>() == I64{23, 0, 0}));
  REQUIRE((dt.nanosecond().values<int64_t>() == I64{999, 0, 0}));
  REQUIRE((dt.subsecond().values<double>() == std::vector<double>{0.999999999, 0, 0}));
  REQUIRE((dt.is_leap_year().values<bool>() == Flags{false, true, false}));
  REQUIRE((dt.day_of_year().values<int64_t>() == I64{365, 60, 1}));
  Series y = dt.year();
  REQUIRE(y.m_index.has_value() && (y.m_index->values_as<int64_t>() == I64{10, 20, 30}));
  REQUIRE(y.name().empty());
  REQUIRE_THROWS(Series(std::vector<double>{1.5}).dt());
  REQUIRE_THROWS(Series(Flags{true}).dt());
}

// the operands of the reference's "between functions" case: midnight and noon of 2022-01-01 .. 04, then pairs that cross boundaries
static void test_between() {
  Series a = stamps({k2022, k2022 + kDay, k2022 + 2 * kDay, k2022 + 3 * kDay});
  Series b = stamps({k2022 + 12 * kHour, k2022 + kDay + 12 * kHour, k2022 + 2 * kDay + 12 * kHour, k2022 + 3 * kDay + 12 * kHour});
  DateTimeLike d = a.dt();
  REQUIRE((d.days_between(b).values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((d.hours_between(b).values<int64_t>() == I64{12, 12, 12, 12}));
  REQUIRE((d.minutes_between(b).values<int64_t>() == I64{720, 720, 720, 720}));
  REQUIRE((d.seconds_between(b).values<int64_t>() == I64{43200, 43200, 43200, 43200}));
  REQUIRE((d.milliseconds_between(b).values<int64_t>() == I64{43200000, 43200000, 43200000, 43200000}));
  REQUIRE((d.microseconds_between(b).values<int64_t>() == I64{43200000000LL, 43200000000LL, 43200000000LL, 43200000000LL}));
  REQUIRE((d.nanoseconds_between(b).values<int64_t>() == I64{12 * kHour, 12 * kHour, 12 * kHour, 12 * kHour}));
  REQUIRE((d.weeks_between(b).values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((d.years_between(b).values<int64_t>() == I64{0, 0, 0, 0}));
  REQUIRE((d.quarters_between(b).values<int64_t>() == I64{0, 0, 0, 0}));
  // boundaries crossed, not elapsed time: 2 ns apart across the new year 2021 -> 2022 (a Friday night); Sunday -> Monday; backwards
  Series p = stamps({k2022 - 1, k2022 + kDay, k2022 + kDay});
  Series q = stamps({k2022 + 1, k2022 + 2 * kDay, k2022 - 90 * kDay});
  DateTimeLike pd_ = p.dt();
  REQUIRE((pd_.years_between(q).values<int64_t>() == I64{1, 0, -1}));
  REQUIRE((pd_.quarters_between(q).values<int64_t>() == I64{1, 0, -1}));
  REQUIRE((pd_.days_between(q).values<int64_t>() == I64{1, 1, -91}));
  REQUIRE((pd_.hours_between(q).values<int64_t>() == I64{1, 24, -91 * 24}));
  REQUIRE((pd_.weeks_between(q).values<int64_t>() == I64{0, 1, -13}));
  REQUIRE((pd_.nanoseconds_between(q).values<int64_t>() == I64{2, kDay, -91 * kDay}));
  // null where either side is null; unequal lengths and the interval kernels throw
  const Flags va{true, false, true}, vb{true, true, false};
  Array na = Array::Make(I64{k2022, k2022, k2022}, &va);
  na.dtype = PDX_TIMESTAMP_NS;
  Array nb = Array::Make(I64{k2022 + kDay, k2022 + kDay, k2022 + kDay}, &vb);
  nb.dtype = PDX_TIMESTAMP_NS;
  Series nd = Series(na).dt().days_between(Series(nb));
  REQUIRE((nd.m_array.valid_flags() == Flags{true, false, false}));
  REQUIRE(nd.values<int64_t>()[0] == 1);
  REQUIRE_THROWS(d.days_between(p));
  REQUIRE_THROWS(d.day_time_interval_between(b));
  REQUIRE_THROWS(d.month_interval_between(b));
  REQUIRE_THROWS(d.month_day_nano_interval_between(b));
}

static void test_round() {
  // 2022-01-01 11:59:59.999999999, 12:00 (a tie: up), 2022-01-02 00:00 (on the boundary), 2022-01-16 12:00 (a month tie: up)
  Series s = stamps({k2022 + 12 * kHour - 1, k2022 + 12 * kHour, k2022 + kDay, k2022 + 15 * kDay + 12 * kHour});
  DateTimeLike dt = s.dt();
  REQUIRE((dt.floor().values<int64_t>() == I64{k2022, k2022, k2022 + kDay, k2022 + 15 * kDay}));
  REQUIRE((dt.ceil().values<int64_t>() == I64{k2022 + kDay, k2022 + kDay, k2022 + kDay, k2022 + 16 * kDay}));
  REQUIRE((dt.round().values<int64_t>() == I64{k2022, k2022 + kDay, k2022 + kDay, k2022 + 16 * kDay}));
  REQUIRE(dt.round().dtype() == PDX_TIMESTAMP_NS);
  REQUIRE((dt.round(1, CalendarUnit::MONTH).values<int64_t>() == I64{k2022, k2022, k2022, k2022 + 31 * kDay}));
  REQUIRE((dt.round(6, CalendarUnit::HOUR).values<int64_t>() == I64{k2022 + 12 * kHour, k2022 + 12 * kHour, k2022 + kDay, k2022 + 15 * kDay + 12 * kHour}));
  REQUIRE((dt.floor(1, CalendarUnit::WEEK).values<int64_t>() == I64{k2022 - 5 * kDay, k2022 - 5 * kDay, k2022 - 5 * kDay, k2022 + 9 * kDay}));
  REQUIRE((dt.floor(1, CalendarUnit::WEEK, false).values<int64_t>() == I64{k2022 - 6 * kDay, k2022 - 6 * kDay, k2022 + kDay, k2022 + 15 * kDay}));
  REQUIRE_THROWS(dt.ceil(1, CalendarUnit::DAY, true, true));
  try {  // the refusals carry Arrow's NotImplemented prefix, an invalid argument does not
    (void)dt.is_dst();
  } catch (const std::runtime_error& e) {
    REQUIRE(std::string(e.what()).rfind("NotImplemented: DateTimeLike::is_dst", 0) == 0);
  }
  try {
    (void)dt.round(1, CalendarUnit::DAY, true, true);
  } catch (const std::runtime_error& e) {
    REQUIRE(std::string(e.what()).rfind("NotImplemented: DateTimeLike::round", 0) == 0);
  }
  REQUIRE_THROWS(dt.round(1, CalendarUnit::YEAR));
  const Flags vn{true, false};
  Array n = Array::Make(I64{k2022 + 1, 0}, &vn);
  n.dtype = PDX_TIMESTAMP_NS;
  Series r = Series(n).dt().round(1, CalendarUnit::HOUR);
  REQUIRE((r.m_array.valid_flags() == Flags{true, false}));
  REQUIRE(r.values<int64_t>()[0] == k2022);
  Series h = Series(n).dt().hour();
  REQUIRE((h.m_array.valid_flags() == Flags{true, false}));
  Series e = stamps({});
  REQUIRE(e.dt().year().size() == 0 && e.dt().round().size() == 0 && e.dt().days_between(e).size() == 0);
}

int main() {
  ThrowOnFailure(pdx_init(0));
  test_components();
  test_floor_toward_minus_infinity_and_index();
  test_between();
  test_round();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
