// temporal_round.hpp -- Arrow's floor_temporal / ceil_temporal / round_temporal on one int64 nanosecond timestamp, as device functions
// shared by pdx_round_temporal (temporal.hip: the rounded column) and pdx_downsample_create (groupby.hip: runs of equal rounded labels
// without materialising the column), and the calendar fields behind pdx_temporal_components / pdx_temporal_between.  Semantics and their
// pinning: see temporal.hip.
#pragma once
#include "pdx_common.hpp"

namespace pdx {

constexpr long long kNsPerDay = 86400000000000LL;

struct RoundParams {
  long long u;       // unit in ns (fixed units), 7 days for week
  long long up;      // next larger unit in ns (calendar origin of the fixed units below day)
  long long p;       // multiple * u
  long long mult;    // multiple (months for month / quarter: multiple * 3 for quarters)
  long long week_org;  // 3 days (weeks start Monday) or 4 days (Sunday)
  int week_target;   // weekday of the anchor in the previous December: 4 = Thursday, 3 = Wednesday (0 = Sunday)
  double inv_u, inv_up, inv_p;  // reciprocals of u / up / p (0 where the divisor is unused)
};

// floor division toward -inf for b > 0 (generic form: a 64-bit hardware-less division, ~100 instructions)
__device__ __forceinline__ long long fdiv(long long a, long long b) {
  long long q = a / b;
  return (a % b < 0) ? q - 1 : q;
}
// The same for a divisor known on the host (inv = 1.0 / b): estimate the quotient in double precision, then correct it with the
// exact int64 remainder.  |estimate - a / b| <= |a / b| * 2^-51 + 1: at most one unit off for real timestamps and b >= 1 us (the
// common rules), so ONE conditional step settles it; a small divisor (rules like "7n": b < 1000 against |a| ~ 1e18) can leave the
// estimate hundreds of units off -- that case takes one exact 64-bit division of the (small) remainder instead of a loop of unit steps.
// The 64-bit division this replaces made the rounding kernels ALU bound (3.6 ms per 1e9 rows at 16 B/row).
__device__ __forceinline__ long long fdiv_c(long long a, long long b, double inv) {
  if (b == 1) return a;
  long long q = (long long)__builtin_floor((double)a * inv);
  long long r = (long long)((unsigned long long)a - (unsigned long long)q * (unsigned long long)b);
  if (r < 0) {
    --q;
    r += b;
  } else if (r >= b) {
    ++q;
    r -= b;
  }
  if (r < 0 || r >= b) {  // rare: still outside [0, b) -- floor-divide the remainder exactly
    long long adj = r / b;
    if (r % b < 0) --adj;
    q += adj;
  }
  return q;
}
// truncating division (C++ operator/) by a host-known divisor
__device__ __forceinline__ long long tdiv_c(long long a, long long b, double inv) {
  const long long q = fdiv_c(a, b, inv);
  return (a < 0 && q * b != a) ? q + 1 : q;
}

// days since 1970-01-01 <-> proleptic Gregorian civil date (H. Hinnant's algorithms, the ones Arrow's vendored date.h uses)
__device__ __forceinline__ void civil_from_days(long long z, long long* y, int* m) {
  z += 719468;
  const long long era = (z >= 0 ? z : z - 146096) / 146097;
  const long long doe = z - era * 146097;
  const long long yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const long long doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const long long mp = (5 * doy + 2) / 153;
  *m = (int)(mp < 10 ? mp + 3 : mp - 9);
  *y = yoe + era * 400 + (*m <= 2);
}
__device__ __forceinline__ long long days_from_civil(long long y, int m, int d) {
  y -= m <= 2;
  const long long era = (y >= 0 ? y : y - 399) / 400;
  const long long yoe = y - era * 400;
  const long long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const long long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

// MODE: 0 = fixed unit, multiple == 1      1 = fixed unit, multiples since the epoch      2 = fixed unit below day, calendar origin
//       3 = day, calendar origin (1st of the month)    4 = week, multiple == 1    5 = week, multiples since the epoch
//       6 = week, calendar origin          7 = month / quarter, multiple == 1 month       8 = months since 1970-01
//       9 = months since January of the year
template <int MODE>
__device__ __forceinline__ long long floor_one(long long t, const RoundParams& q) {
  if constexpr (MODE == 0) {
    return fdiv_c(t, q.u, q.inv_u) * q.u;
  } else if constexpr (MODE == 1) {
    return fdiv_c(t, q.p, q.inv_p) * q.p;  // floor(floor(t / u) / mult) == floor(t / (u * mult))
  } else if constexpr (MODE == 2) {
    const long long origin = fdiv_c(t, q.up, q.inv_up) * q.up;
    return fdiv_c(t - origin, q.p, q.inv_p) * q.p + origin;  // (t >= origin: truncation == floor)
  } else if constexpr (MODE == 3) {
    long long y;
    int m;
    civil_from_days(fdiv(t, kNsPerDay), &y, &m);
    const long long origin = days_from_civil(y, m, 1) * kNsPerDay;
    return fdiv_c(t - origin, q.p, q.inv_p) * q.p + origin;  // (t >= origin)
  } else if constexpr (MODE == 4) {
    return fdiv_c(t + q.week_org, q.u, q.inv_u) * q.u - q.week_org;
  } else if constexpr (MODE == 5) {
    return fdiv_c(t + q.week_org, q.p, q.inv_p) * q.p - q.week_org;
  } else if constexpr (MODE == 6) {
    const long long tt = t + q.week_org;
    long long y;
    int m;
    civil_from_days(fdiv(tt, kNsPerDay), &y, &m);
    const long long dec31 = days_from_civil(y - 1, 12, 31);
    const long long wd = ((dec31 + 4) % 7 + 7) % 7;  // 0 = Sunday (1970-01-01 was a Thursday)
    const long long last = dec31 - (((wd - q.week_target) % 7 + 7) % 7);
    const long long start = (last + 4) * kNsPerDay;  // date.h: (mon - thu) counts 4 days modulo 7
    return tdiv_c(tt - start, q.p, q.inv_p) * q.p + start;  // truncating, like the C++ it restates: tt may precede start by a few days
  } else {
    long long y;
    int m;
    civil_from_days(fdiv(t, kNsPerDay), &y, &m);
    if constexpr (MODE == 7) return days_from_civil(y, m, 1) * kNsPerDay;
    if constexpr (MODE == 9) return days_from_civil(y, 1 + (int)((m - 1) / q.mult * q.mult), 1) * kNsPerDay;
    const long long tm = fdiv((y - 1970) * 12 + m - 1, q.mult) * q.mult;
    const long long yy = fdiv(tm, 12);
    return days_from_civil(1970 + yy, (int)(tm - yy * 12) + 1, 1) * kNsPerDay;
  }
}

// the ceil that belongs to the floor f of t
template <int MODE>
__device__ __forceinline__ long long ceil_of_floor(long long t, long long f, const RoundParams& q) {
  if constexpr (MODE <= 6) return f >= t ? f : f + q.p;
  long long y;
  int m;
  civil_from_days(fdiv(f, kNsPerDay), &y, &m);
  const long long tm = y * 12 + m - 1 + q.mult;
  const long long yy = fdiv(tm, 12);
  return days_from_civil(yy, (int)(tm - yy * 12) + 1, 1) * kNsPerDay;
}

template <int MODE, bool CEIL>
__device__ __forceinline__ long long round_one(long long t, const RoundParams& q) {
  const long long f = floor_one<MODE>(t, q);
  if constexpr (!CEIL) return f;
  return ceil_of_floor<MODE>(t, f, q);
}

// round_temporal: of the floor f and the ceil c the nearer one, the ceil on a tie (t - f >= c - t)
template <int MODE>
__device__ __forceinline__ long long nearest_one(long long t, const RoundParams& q) {
  const long long f = floor_one<MODE>(t, q);
  const long long c = ceil_of_floor<MODE>(t, f, q);
  return (t - f >= c - t) ? c : f;
}

// RoundTemporalOptions -> kernel parameters and MODE; returns a PDX_* code (message through fail()).
inline int make_round_params(int64_t multiple, int unit, int week_starts_monday, int calendar_based_origin, RoundParams* out, int* mode_out,
                             const char* who) {
  if (unit < PDX_UNIT_NANOSECOND || unit > PDX_UNIT_QUARTER)
    return fail(unit == PDX_UNIT_QUARTER + 1 ? PDX_NOT_IMPLEMENTED : PDX_INVALID, std::string(who) + ": unit must be nanosecond .. quarter");
  if (multiple < 1) return fail(PDX_INVALID, std::string(who) + ": multiple must be >= 1");
  static const long long unit_ns[8] = {1LL, 1000LL, 1000000LL, 1000000000LL, 60000000000LL, 3600000000000LL, kNsPerDay, 7 * kNsPerDay};
  RoundParams q{};
  int mode;
  if (unit <= PDX_UNIT_WEEK) {
    q.u = unit_ns[unit];
    if (multiple > INT64_MAX / q.u) return fail(PDX_INVALID, std::string(who) + ": multiple x unit overflows int64 nanoseconds");
    q.p = multiple * q.u;
    q.mult = multiple;
    if (unit <= PDX_UNIT_DAY) {
      q.up = unit < PDX_UNIT_DAY ? unit_ns[unit + 1] : 0;
      mode = multiple == 1 ? 0 : !calendar_based_origin ? 1 : unit == PDX_UNIT_DAY ? 3 : 2;
    } else {
      q.week_org = (week_starts_monday ? 3 : 4) * kNsPerDay;
      q.week_target = week_starts_monday ? 4 : 3;
      mode = multiple == 1 ? 4 : !calendar_based_origin ? 5 : 6;
    }
    q.inv_u = 1.0 / (double)q.u;
    q.inv_p = 1.0 / (double)q.p;
    q.inv_up = q.up ? 1.0 / (double)q.up : 0.0;
  } else {
    if (multiple > (1 << 24)) return fail(PDX_INVALID, std::string(who) + ": multiple too large for a calendar unit");
    q.mult = multiple * (unit == PDX_UNIT_QUARTER ? 3 : 1);
    mode = q.mult == 1 ? 7 : calendar_based_origin ? 9 : 8;
  }
  *out = q;
  *mode_out = mode;
  return PDX_OK;
}

// ---------------------------------------------------------------- calendar fields of one timestamp (pdx_temporal_components / _between)
// Every int64 nanosecond timestamp lies within +-106752 days of the epoch (1677-09-21 .. 2262-04-11), so all day arithmetic fits 32 bits
// and the shifted day number below is positive: unsigned divisions by constants, no sign fix-ups.
constexpr unsigned kTfTod = 1, kTfCivil = 2, kTfIso = 4, kTfUs = 8, kTfWeek = 16;  // field families (what a component needs)

struct WeekOpts {  // arrow::compute::WeekOptions
  int week_starts_monday, count_from_zero, first_week_is_fully_in_year;
};

struct TemporalFields {
  int days;                            // floor(t / 1 day)
  int dow;                             // 0 = Monday .. 6 = Sunday
  int y, m, d, doy;                    // civil date, doy: 1 = 1 January
  bool leap;
  int hour, minute, second, ms, us, ns;
  unsigned subns;                      // nanoseconds since the last whole second
  int iso_y, iso_w, us_y, us_w, week;
};

__device__ __forceinline__ int floor_days(long long t) { return (int)fdiv_c(t, kNsPerDay, 1.0 / (double)kNsPerDay); }
__device__ __forceinline__ bool leap_year(int y) { return (y % 4 == 0) && (y % 100 != 0 || y % 400 == 0); }
__device__ __forceinline__ int weekday_sun0(int z) { return (int)((unsigned)(z + 4 + 7 * 20000) % 7u); }  // 1970-01-01 was a Thursday

// civil_from_days with the day of the month, the day of the year and the leap flag (same algorithm, 32-bit, z + 719468 > 0)
__device__ __forceinline__ void civil_fields(int z, int* y, int* m, int* d, int* doy_jan, bool* leap) {
  const unsigned zz = (unsigned)(z + 719468);
  const unsigned era = zz / 146097u;
  const unsigned doe = zz - era * 146097u;
  const unsigned yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
  const unsigned doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);  // 0 = 1 March
  const unsigned mp = (5u * doy + 2u) / 153u;
  *d = (int)(doy - (153u * mp + 2u) / 5u + 1u);
  *m = (int)(mp < 10u ? mp + 3u : mp - 9u);
  *y = (int)(yoe + era * 400u) + (*m <= 2);
  *leap = leap_year(*y);
  *doy_jan = *m > 2 ? (int)doy + 60 + (int)*leap : (int)doy - 305;
}

// Arrow's Week / ISOWeek / USWeek / ISOYear / USYear (scalar_temporal_unary.cc) on day numbers.  The year is that of z + 3 days (the
// week's middle day) or of z itself (first_week_is_fully_in_year or count_from_zero); week 1 starts on the first Monday / Sunday of that year, or four days
// after the last Thursday / Wednesday of the December before; a day before that start belongs to the year before unless count_from_zero,
// where it is week 0.
__device__ __forceinline__ int week_start(int jan1, bool monday, bool full) {
  if (full) return jan1 + (int)((unsigned)((monday ? 1 : 0) - weekday_sun0(jan1) + 7) % 7u);
  const int dec31 = jan1 - 1;
  return dec31 - (int)((unsigned)(weekday_sun0(dec31) - (monday ? 4 : 3) + 7) % 7u) + 4;
}
__device__ __forceinline__ void week_of(int z, bool monday, bool from_zero, bool full, int* year, int* week) {
  const int zo = z + (full || from_zero ? 0 : 3);
  int y, m, d, doy;
  bool leap;
  civil_fields(zo, &y, &m, &d, &doy, &leap);
  int jan1 = zo - (doy - 1);
  int start = week_start(jan1, monday, full);
  if (!from_zero && z < start) {
    --y;
    jan1 -= 365 + (int)leap_year(y);
    start = week_start(jan1, monday, full);
  }
  *year = y;
  *week = (z - start + 7) / 7;  // floor((z - start) / 7) + 1: z - start >= -6
}

template <unsigned FAM>
__device__ __forceinline__ TemporalFields temporal_fields(long long t, const WeekOpts& w) {
  TemporalFields f{};
  f.days = floor_days(t);
  f.dow = (int)((unsigned)(f.days + 3 + 7 * 20000) % 7u);
  if constexpr (FAM & kTfTod) {  // one floor division (above), then remainders of a 47-bit and a 30-bit unsigned number
    // (unsigned: days * 1 day lies below INT64_MIN for the first, partial day of the range; the difference is in [0, 1 day) modulo 2^64)
    const unsigned long long tod = (unsigned long long)t - (unsigned long long)(long long)f.days * (unsigned long long)kNsPerDay;
    const unsigned secs = (unsigned)(tod / 1000000000ull);
    f.subns = (unsigned)(tod - (unsigned long long)secs * 1000000000ull);
    f.hour = (int)(secs / 3600u);
    f.minute = (int)(secs / 60u % 60u);
    f.second = (int)(secs % 60u);
    f.ms = (int)(f.subns / 1000000u);
    f.us = (int)(f.subns / 1000u % 1000u);
    f.ns = (int)(f.subns % 1000u);
  }
  if constexpr (FAM & kTfCivil) civil_fields(f.days, &f.y, &f.m, &f.d, &f.doy, &f.leap);
  if constexpr (FAM & kTfIso) week_of(f.days, true, false, false, &f.iso_y, &f.iso_w);
  if constexpr (FAM & kTfUs) week_of(f.days, false, false, false, &f.us_y, &f.us_w);
  if constexpr (FAM & kTfWeek) {
    int y;
    week_of(f.days, w.week_starts_monday != 0, w.count_from_zero != 0, w.first_week_is_fully_in_year != 0, &y, &f.week);
  }
  return f;
}

constexpr unsigned temporal_family(int c) {
  switch (c) {
    case PDX_TC_YEAR: case PDX_TC_MONTH: case PDX_TC_DAY: case PDX_TC_DAY_OF_YEAR: case PDX_TC_QUARTER: case PDX_TC_IS_LEAP_YEAR: return kTfCivil;
    case PDX_TC_HOUR: case PDX_TC_MINUTE: case PDX_TC_SECOND: case PDX_TC_MILLISECOND: case PDX_TC_MICROSECOND: case PDX_TC_NANOSECOND:
    case PDX_TC_SUBSECOND: return kTfTod;
    case PDX_TC_ISO_WEEK: case PDX_TC_ISO_YEAR: return kTfIso;
    case PDX_TC_US_WEEK: case PDX_TC_US_YEAR: return kTfUs;
    case PDX_TC_WEEK: return kTfWeek;
    default: return 0;  // DAY_OF_WEEK, ISO_DAY_OF_WEEK: the day number alone
  }
}

}  // namespace pdx
