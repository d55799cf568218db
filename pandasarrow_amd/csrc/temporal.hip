// temporal.hip -- floor_temporal / ceil_temporal / round_temporal, the calendar components and the *_between kernels on timestamp[ns]
// columns for gfx950 (the second half of this file: the dt accessor).
//
// Replaces arrow::compute::FloorTemporal / CeilTemporal(m_index, RoundTemporalOptions(multiple, unit, week_starts_monday,
// ceil_is_strictly_greater = false, calendar_based_origin)) in DataFrame::downsample (reference src/dataframe.cpp:1265-1290):
// the binned index that the Resampler's GroupBy is then keyed on.  One HBM-bound stream: 8 B read + 8 B write per row
// (16 B/row), grid-stride over coalesced 8-byte lanes, 4 rows in flight per thread; all the calendar work is integer
// arithmetic in registers.  Semantics restate Arrow C++ 25.0.0 (pinned by the vectors in tests/golden/arrow_golden_r2.npz): floors go toward -inf, a calendar origin is the floor to the next larger unit (day: the
// 1st of the month; week: the Monday/Sunday after the last Thursday/Wednesday of the previous December), month / quarter are
// counted in calendar months, ceil = floor when floor >= t, else floor + multiple x unit (month / quarter: always floor +
// multiple -- Arrow ignores ceil_is_strictly_greater there).
#include "pdx_common.hpp"
#include "temporal_round.hpp"

namespace pdx {

int launch_validity_and(const pdx_column* a, const pdx_column* b, int b_is_scalar, int64_t n, uint8_t* out, hipStream_t st);  // elementwise.hip

namespace {

template <int MODE, bool CEIL>
__global__ void __launch_bounds__(256) k_round_temporal(const long long* __restrict__ ts, long long* __restrict__ out, int64_t n, RoundParams q) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    long long t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = ts[i + k * stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[i + k * stride] = round_one<MODE, CEIL>(t[k], q);
  }
  for (; i < n; i += stride) out[i] = round_one<MODE, CEIL>(ts[i], q);
}

// round to nearest: the same stream, floor and ceil of a row share the floor's arithmetic
template <int MODE>
__global__ void __launch_bounds__(256) k_round_nearest(const long long* __restrict__ ts, long long* __restrict__ out, int64_t n, RoundParams q) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    long long t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = ts[i + k * stride];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[i + k * stride] = nearest_one<MODE>(t[k], q);
  }
  for (; i < n; i += stride) out[i] = nearest_one<MODE>(ts[i], q);
}

template <int MODE>
void launch_mode(int how, const long long* ts, long long* out, int64_t n, const RoundParams& q, hipStream_t st) {
  dim3 grid(grid_for(n, 256, 4)), block(256);
  if (how == PDX_ROUND_NEAREST) hipLaunchKernelGGL((k_round_nearest<MODE>), grid, block, 0, st, ts, out, n, q);
  else if (how != PDX_ROUND_FLOOR) hipLaunchKernelGGL((k_round_temporal<MODE, true>), grid, block, 0, st, ts, out, n, q);
  else hipLaunchKernelGGL((k_round_temporal<MODE, false>), grid, block, 0, st, ts, out, n, q);
}

// ---------------------------------------------------------------- calendar components (pdx_temporal_components)
// Built as one stream like k_round_temporal (whether each instantiation reaches that kernel's rate: DESIGN section 13): 8 B read + 8 B
// (1/8 B for a bool) written per row and output; a wave owns 64 consecutive
// rows of each of its four strided batches, so a bool output is one ballot and one 64-bit store per wave and batch (no byte is shared
// between waves).  The fields of a row (temporal_round.hpp) are computed once, whatever the number of outputs that use them, and only
// the families the list needs: the list is either a template parameter pack (every single component, the year_month_day and
// iso_calendar triples: unused fields fold away) or, for any other list, kernel arguments held in scalar registers -- the switch that
// picks a field is wave uniform and sits outside the loop over the four rows in flight; FAM names the field families to compute.
struct ComponentArgs {
  void* out[8];
  int comp[8];
  int nc;
  WeekOpts w;
};

template <int R, bool FULL>
__device__ __forceinline__ void emit_component(int comp, void* outp, const TemporalFields (&f)[R], int64_t base, int lane, int64_t stride, int64_t n) {
  if (comp == PDX_TC_IS_LEAP_YEAR) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int64_t b = base + k * stride;
      const uint64_t bal = __ballot((FULL || b + lane < n) && f[k].leap);
      if (lane == 0) {
        if (FULL || n - b >= 64) {
          static_cast<uint64_t*>(outp)[b >> 6] = bal;
        } else {
          for (int q = 0; q < (int)((n - b + 7) >> 3); ++q) static_cast<uint8_t*>(outp)[(b >> 3) + q] = (uint8_t)(bal >> (8 * q));
        }
      }
    }
  } else if (comp == PDX_TC_SUBSECOND) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int64_t row = base + k * stride + lane;
      if (FULL || row < n) static_cast<double*>(outp)[row] = (double)f[k].subns / 1000000000.0;
    }
  } else {
    long long v[R];
#define PDX_TC_CASE(NAME, EXPR)                 \
  case NAME:                                    \
    _Pragma("unroll") for (int k = 0; k < R; ++k) v[k] = (EXPR); \
    break;
    switch (comp) {
      PDX_TC_CASE(PDX_TC_YEAR, f[k].y)
      PDX_TC_CASE(PDX_TC_MONTH, f[k].m)
      PDX_TC_CASE(PDX_TC_DAY, f[k].d)
      PDX_TC_CASE(PDX_TC_DAY_OF_WEEK, f[k].dow)
      PDX_TC_CASE(PDX_TC_DAY_OF_YEAR, f[k].doy)
      PDX_TC_CASE(PDX_TC_HOUR, f[k].hour)
      PDX_TC_CASE(PDX_TC_MINUTE, f[k].minute)
      PDX_TC_CASE(PDX_TC_SECOND, f[k].second)
      PDX_TC_CASE(PDX_TC_MILLISECOND, f[k].ms)
      PDX_TC_CASE(PDX_TC_MICROSECOND, f[k].us)
      PDX_TC_CASE(PDX_TC_NANOSECOND, f[k].ns)
      PDX_TC_CASE(PDX_TC_QUARTER, (f[k].m + 2) / 3)
      PDX_TC_CASE(PDX_TC_ISO_WEEK, f[k].iso_w)
      PDX_TC_CASE(PDX_TC_ISO_YEAR, f[k].iso_y)
      PDX_TC_CASE(PDX_TC_ISO_DAY_OF_WEEK, f[k].dow + 1)
      PDX_TC_CASE(PDX_TC_US_WEEK, f[k].us_w)
      PDX_TC_CASE(PDX_TC_US_YEAR, f[k].us_y)
      default:
        _Pragma("unroll") for (int k = 0; k < R; ++k) v[k] = f[k].week;
        break;
    }
#undef PDX_TC_CASE
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int64_t row = base + k * stride + lane;
      if (FULL || row < n) static_cast<long long*>(outp)[row] = v[k];
    }
  }
}

// R rows of this lane: base + k * stride + lane.  CS empty: the list comes from the arguments.
template <unsigned FAM, int R, bool FULL, int... CS>
__device__ __forceinline__ void components_step(const long long* __restrict__ ts, int64_t base, int lane, int64_t stride, int64_t n, const ComponentArgs& a) {
  long long t[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int64_t row = base + k * stride + lane;
    t[k] = (FULL || row < n) ? ts[row] : 0;
  }
  TemporalFields f[R];
#pragma unroll
  for (int k = 0; k < R; ++k) f[k] = temporal_fields<FAM>(t[k], a.w);
  if constexpr (sizeof...(CS) > 0) {
    int c = 0;
    ((emit_component<R, FULL>(CS, a.out[c], f, base, lane, stride, n), ++c), ...);
  } else {
    for (int c = 0; c < a.nc; ++c) emit_component<R, FULL>(a.comp[c], a.out[c], f, base, lane, stride, n);
  }
}

template <unsigned FAM, int... CS>
__device__ __forceinline__ void components_body(const long long* __restrict__ ts, int64_t n, const ComponentArgs& a) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;  // a multiple of 256: every batch of a wave starts on a 64-row word
  int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
  for (; base + 3 * stride + 64 <= n; base += 4 * stride) components_step<FAM, 4, true, CS...>(ts, base, lane, stride, n, a);
  for (; base < n; base += stride) components_step<FAM, 1, false, CS...>(ts, base, lane, stride, n, a);
}

template <int... CS>
__global__ void __launch_bounds__(256) k_components(const long long* __restrict__ ts, int64_t n, ComponentArgs a) {
  components_body<(temporal_family(CS) | ...), CS...>(ts, n, a);
}
// any other list.  FAM bit 0: time of day, bit 1: civil date, bit 2: the ISO / US / WEEK numbering
template <unsigned FAM3>
__global__ void __launch_bounds__(256) k_components_list(const long long* __restrict__ ts, int64_t n, ComponentArgs a) {
  components_body<((FAM3 & 1) ? kTfTod : 0) | ((FAM3 & 2) ? kTfCivil : 0) | ((FAM3 & 4) ? (kTfIso | kTfUs | kTfWeek) : 0)>(ts, n, a);
}

template <int... CS>
void launch_components(const long long* ts, int64_t n, const ComponentArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_components<CS...>), dim3(grid_for(n, 256, 4)), dim3(256), 0, st, ts, n, a);
}
template <unsigned FAM3>
void launch_components_list(const long long* ts, int64_t n, const ComponentArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_components_list<FAM3>), dim3(grid_for(n, 256, 4)), dim3(256), 0, st, ts, n, a);
}

// ---------------------------------------------------------------- *_between (pdx_temporal_between): 16 B read + 8 B written per row
template <int UNIT>
__device__ __forceinline__ long long unit_index(long long t) {
  if constexpr (UNIT == PDX_UNIT_NANOSECOND) return t;
  else if constexpr (UNIT == PDX_UNIT_MICROSECOND) return fdiv_c(t, 1000LL, 1.0 / 1000.0);
  else if constexpr (UNIT == PDX_UNIT_MILLISECOND) return fdiv_c(t, 1000000LL, 1.0 / 1000000.0);
  else if constexpr (UNIT == PDX_UNIT_SECOND) return fdiv_c(t, 1000000000LL, 1.0 / 1000000000.0);
  else if constexpr (UNIT == PDX_UNIT_MINUTE) return fdiv_c(t, 60000000000LL, 1.0 / 60000000000.0);
  else if constexpr (UNIT == PDX_UNIT_HOUR) return fdiv_c(t, 3600000000000LL, 1.0 / 3600000000000.0);
  else if constexpr (UNIT == PDX_UNIT_DAY) return floor_days(t);
  else if constexpr (UNIT == PDX_UNIT_WEEK) return (long long)((unsigned)(floor_days(t) + 3 + 7 * 20000) / 7u);  // weeks start on Monday
  else {
    int y, m, d, doy;
    bool leap;
    civil_fields(floor_days(t), &y, &m, &d, &doy, &leap);
    return UNIT == PDX_UNIT_YEAR ? (long long)y : (long long)y * 4 + (m - 1) / 3;
  }
}
template <int UNIT>
__global__ void __launch_bounds__(256) k_between(const long long* __restrict__ a, const long long* __restrict__ b, long long* __restrict__ out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    long long x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = a[i + k * stride];
      y[k] = b[i + k * stride];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[i + k * stride] = unit_index<UNIT>(y[k]) - unit_index<UNIT>(x[k]);
  }
  for (; i < n; i += stride) out[i] = unit_index<UNIT>(b[i]) - unit_index<UNIT>(a[i]);
}
template <int UNIT>
void launch_between(const long long* a, const long long* b, long long* out, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL((k_between<UNIT>), dim3(grid_for(n, 256, 4)), dim3(256), 0, st, a, b, out, n);
}

}  // namespace
}  // namespace pdx

using namespace pdx;

extern "C" {

int pdx_round_temporal(int ceil_mode, const pdx_column* ts, int64_t multiple, int unit, int week_starts_monday, int calendar_based_origin,
                       pdx_mut_column* out, void* stream) {
  PDX_TRY(check_column(ts, "pdx_round_temporal"));
  if (ts->dtype != PDX_TIMESTAMP_NS) return fail(PDX_INVALID, "pdx_round_temporal: input must be PDX_TIMESTAMP_NS");
  RoundParams q{};
  int mode = 0;
  PDX_TRY(make_round_params(multiple, unit, week_starts_monday, calendar_based_origin, &q, &mode, "pdx_round_temporal"));
  if (!out || out->length < ts->length || out->dtype != PDX_TIMESTAMP_NS)
    return fail(PDX_INVALID, "pdx_round_temporal: output must be PDX_TIMESTAMP_NS of the input length");
  const bool has_nulls = validity_or_null(ts) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_round_temporal: input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  const int64_t n = ts->length;
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, "pdx_round_temporal: null output buffer");
  const long long* in = static_cast<const long long*>(ts->values) + ts->offset;
  long long* o = static_cast<long long*>(out->values);
  {
    PDX_PROFILE("round_temporal", st);
    switch (mode) {
      case 0: launch_mode<0>(ceil_mode, in, o, n, q, st); break;
      case 1: launch_mode<1>(ceil_mode, in, o, n, q, st); break;
      case 2: launch_mode<2>(ceil_mode, in, o, n, q, st); break;
      case 3: launch_mode<3>(ceil_mode, in, o, n, q, st); break;
      case 4: launch_mode<4>(ceil_mode, in, o, n, q, st); break;
      case 5: launch_mode<5>(ceil_mode, in, o, n, q, st); break;
      case 6: launch_mode<6>(ceil_mode, in, o, n, q, st); break;
      case 7: launch_mode<7>(ceil_mode, in, o, n, q, st); break;
      case 8: launch_mode<8>(ceil_mode, in, o, n, q, st); break;
      default: launch_mode<9>(ceil_mode, in, o, n, q, st); break;
    }
    PDX_LAUNCH_CHECK();
  }
  if (out->validity) PDX_TRY(launch_validity_and(ts, nullptr, 0, n, static_cast<uint8_t*>(out->validity), st));
  return PDX_OK;
}

int pdx_temporal_components(const pdx_column* ts, const int* components, int nc, const pdx_week_options* week_opts, pdx_mut_column* outs,
                            void* stream) {
  static const char* who = "pdx_temporal_components";
  PDX_TRY(check_column(ts, who));
  if (ts->dtype != PDX_TIMESTAMP_NS) return fail(PDX_INVALID, std::string(who) + ": input must be PDX_TIMESTAMP_NS");
  if (nc < 1 || nc > 8) return fail(PDX_INVALID, std::string(who) + ": between 1 and 8 components per call");
  if (!components || !outs) return fail(PDX_INVALID, std::string(who) + ": null component list or outputs");
  const bool has_nulls = validity_or_null(ts) != nullptr;
  const int64_t n = ts->length;
  ComponentArgs a{};
  a.nc = nc;
  a.w = week_opts ? WeekOpts{week_opts->week_starts_monday, week_opts->count_from_zero, week_opts->first_week_is_fully_in_year} : WeekOpts{1, 0, 0};
  unsigned fam = 0;
  for (int c = 0; c < nc; ++c) {
    const int comp = components[c];
    if (comp < PDX_TC_YEAR || comp > PDX_TC_SUBSECOND) return fail(PDX_INVALID, std::string(who) + ": unknown component " + std::to_string(comp));
    const int want = comp == PDX_TC_IS_LEAP_YEAR ? PDX_BOOL : comp == PDX_TC_SUBSECOND ? PDX_FLOAT64 : PDX_INT64;
    if (outs[c].dtype != want || outs[c].length < n)
      return fail(PDX_INVALID, std::string(who) + ": output " + std::to_string(c) + " must be " + dtype_name(want) + " of the input length");
    if (has_nulls && !outs[c].validity) return fail(PDX_INVALID, std::string(who) + ": input carries nulls but output " + std::to_string(c) + " has no validity buffer");
    if (n > 0 && !outs[c].values) return fail(PDX_INVALID, std::string(who) + ": null output buffer");
    if (want == PDX_BOOL && (reinterpret_cast<uintptr_t>(outs[c].values) & 7))  // the kernel stores whole 64-row words
      return fail(PDX_INVALID, std::string(who) + ": the values buffer of a PDX_BOOL output must be 8-byte aligned");
    for (int e = 0; e < c; ++e)
      if (outs[e].values == outs[c].values && n > 0) return fail(PDX_INVALID, std::string(who) + ": two outputs share a buffer");
    a.comp[c] = comp;
    a.out[c] = outs[c].values;
    fam |= temporal_family(comp);
  }
  hipStream_t st = as_stream(stream);
  for (int c = 0; c < nc; ++c) {
    outs[c].length = n;
    outs[c].null_count = has_nulls ? -1 : 0;
  }
  if (n == 0) return PDX_OK;
  const long long* in = static_cast<const long long*>(ts->values) + ts->offset;
  {
    PDX_PROFILE("temporal_components", st);
    const int* cs = components;
    if (nc == 1) {
      switch (cs[0]) {
        case PDX_TC_YEAR: launch_components<PDX_TC_YEAR>(in, n, a, st); break;
        case PDX_TC_MONTH: launch_components<PDX_TC_MONTH>(in, n, a, st); break;
        case PDX_TC_DAY: launch_components<PDX_TC_DAY>(in, n, a, st); break;
        case PDX_TC_DAY_OF_WEEK: launch_components<PDX_TC_DAY_OF_WEEK>(in, n, a, st); break;
        case PDX_TC_DAY_OF_YEAR: launch_components<PDX_TC_DAY_OF_YEAR>(in, n, a, st); break;
        case PDX_TC_HOUR: launch_components<PDX_TC_HOUR>(in, n, a, st); break;
        case PDX_TC_MINUTE: launch_components<PDX_TC_MINUTE>(in, n, a, st); break;
        case PDX_TC_SECOND: launch_components<PDX_TC_SECOND>(in, n, a, st); break;
        case PDX_TC_MILLISECOND: launch_components<PDX_TC_MILLISECOND>(in, n, a, st); break;
        case PDX_TC_MICROSECOND: launch_components<PDX_TC_MICROSECOND>(in, n, a, st); break;
        case PDX_TC_NANOSECOND: launch_components<PDX_TC_NANOSECOND>(in, n, a, st); break;
        case PDX_TC_QUARTER: launch_components<PDX_TC_QUARTER>(in, n, a, st); break;
        case PDX_TC_ISO_WEEK: launch_components<PDX_TC_ISO_WEEK>(in, n, a, st); break;
        case PDX_TC_ISO_YEAR: launch_components<PDX_TC_ISO_YEAR>(in, n, a, st); break;
        case PDX_TC_ISO_DAY_OF_WEEK: launch_components<PDX_TC_ISO_DAY_OF_WEEK>(in, n, a, st); break;
        case PDX_TC_US_WEEK: launch_components<PDX_TC_US_WEEK>(in, n, a, st); break;
        case PDX_TC_US_YEAR: launch_components<PDX_TC_US_YEAR>(in, n, a, st); break;
        case PDX_TC_WEEK: launch_components<PDX_TC_WEEK>(in, n, a, st); break;
        case PDX_TC_IS_LEAP_YEAR: launch_components<PDX_TC_IS_LEAP_YEAR>(in, n, a, st); break;
        default: launch_components<PDX_TC_SUBSECOND>(in, n, a, st); break;
      }
    } else if (nc == 3 && cs[0] == PDX_TC_YEAR && cs[1] == PDX_TC_MONTH && cs[2] == PDX_TC_DAY) {
      launch_components<PDX_TC_YEAR, PDX_TC_MONTH, PDX_TC_DAY>(in, n, a, st);
    } else if (nc == 3 && cs[0] == PDX_TC_ISO_YEAR && cs[1] == PDX_TC_ISO_WEEK && cs[2] == PDX_TC_ISO_DAY_OF_WEEK) {
      launch_components<PDX_TC_ISO_YEAR, PDX_TC_ISO_WEEK, PDX_TC_ISO_DAY_OF_WEEK>(in, n, a, st);
    } else {
      const unsigned fam3 = ((fam & kTfTod) ? 1u : 0u) | ((fam & kTfCivil) ? 2u : 0u) | ((fam & (kTfIso | kTfUs | kTfWeek)) ? 4u : 0u);
      switch (fam3) {
        case 0: launch_components_list<0>(in, n, a, st); break;
        case 1: launch_components_list<1>(in, n, a, st); break;
        case 2: launch_components_list<2>(in, n, a, st); break;
        case 3: launch_components_list<3>(in, n, a, st); break;
        case 4: launch_components_list<4>(in, n, a, st); break;
        case 5: launch_components_list<5>(in, n, a, st); break;
        case 6: launch_components_list<6>(in, n, a, st); break;
        default: launch_components_list<7>(in, n, a, st); break;
      }
    }
    PDX_LAUNCH_CHECK();
  }
  for (int c = 0; c < nc; ++c)
    if (outs[c].validity) PDX_TRY(launch_validity_and(ts, nullptr, 0, n, static_cast<uint8_t*>(outs[c].validity), st));
  return PDX_OK;
}

int pdx_temporal_between(int unit, const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream) {
  static const char* who = "pdx_temporal_between";
  PDX_TRY(check_column(a, who));
  PDX_TRY(check_column(b, who));
  if (a->dtype != PDX_TIMESTAMP_NS || b->dtype != PDX_TIMESTAMP_NS) return fail(PDX_INVALID, std::string(who) + ": inputs must be PDX_TIMESTAMP_NS");
  if (unit < PDX_UNIT_NANOSECOND || unit > PDX_UNIT_YEAR || unit == PDX_UNIT_MONTH)
    return fail(PDX_INVALID, std::string(who) + ": unit must be a pdx_calendar_unit other than month");
  if (a->length != b->length) return fail(PDX_INVALID, "Array arguments must all be the same length");
  const int64_t n = a->length;
  if (!out || out->dtype != PDX_INT64 || out->length < n) return fail(PDX_INVALID, std::string(who) + ": output must be PDX_INT64 of the input length");
  const bool has_nulls = validity_or_null(a) != nullptr || validity_or_null(b) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, std::string(who) + ": an input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, std::string(who) + ": null output buffer");
  const long long* pa = static_cast<const long long*>(a->values) + a->offset;
  const long long* pb = static_cast<const long long*>(b->values) + b->offset;
  long long* o = static_cast<long long*>(out->values);
  {
    PDX_PROFILE("temporal_between", st);
    switch (unit) {
      case PDX_UNIT_NANOSECOND: launch_between<PDX_UNIT_NANOSECOND>(pa, pb, o, n, st); break;
      case PDX_UNIT_MICROSECOND: launch_between<PDX_UNIT_MICROSECOND>(pa, pb, o, n, st); break;
      case PDX_UNIT_MILLISECOND: launch_between<PDX_UNIT_MILLISECOND>(pa, pb, o, n, st); break;
      case PDX_UNIT_SECOND: launch_between<PDX_UNIT_SECOND>(pa, pb, o, n, st); break;
      case PDX_UNIT_MINUTE: launch_between<PDX_UNIT_MINUTE>(pa, pb, o, n, st); break;
      case PDX_UNIT_HOUR: launch_between<PDX_UNIT_HOUR>(pa, pb, o, n, st); break;
      case PDX_UNIT_DAY: launch_between<PDX_UNIT_DAY>(pa, pb, o, n, st); break;
      case PDX_UNIT_WEEK: launch_between<PDX_UNIT_WEEK>(pa, pb, o, n, st); break;
      case PDX_UNIT_QUARTER: launch_between<PDX_UNIT_QUARTER>(pa, pb, o, n, st); break;
      default: launch_between<PDX_UNIT_YEAR>(pa, pb, o, n, st); break;
    }
    PDX_LAUNCH_CHECK();
  }
  if (out->validity) PDX_TRY(launch_validity_and(a, b, 0, n, static_cast<uint8_t*>(out->validity), st));
  return PDX_OK;
}

}  // extern "C"
