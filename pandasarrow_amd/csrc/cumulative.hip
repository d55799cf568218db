// cumulative.hip -- pdx_cumulative (cumsum / cumprod / cummax / cummin), pdx_fill_null (ffill / bfill), pdx_shift.
// The scans are cum_scan.hpp's Scan<T, Op>; shift is one pass of its own (a row per lane, validity by ballot).  The null counter, its
// read-back and the wave's null count are colview.hpp's.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "colview.hpp"
#include "cum_scan.hpp"

namespace pdx {

// tiles per chunk of the chunked three-phase scan.  PDX_SCAN_CHUNK_ROWS (read once): > 0 rows (rounded up to whole tiles), 0 or unset =
// the plain form (one chunk).  Chunks of 64 MiB of input, meant to serve the second read from the Infinity Cache, measured slower than
// the plain form at 1e9 rows, so the plain form is the default.
static int64_t scan_chunk_tiles() {
  static const int64_t env_rows = [] {
    const char* e = getenv("PDX_SCAN_CHUNK_ROWS");
    return e && e[0] ? atoll(e) : -1ll;
  }();
  return env_rows > 0 ? ceil_div(env_rows, kCumTile) : 0;
}

// the checks the three entry points share
static int check_io(const pdx_column* a, const pdx_mut_column* out, const char* who, bool timestamp_ok) {
  PDX_TRY(check_column(a, who, true));
  const int dt = a->dtype;
  const bool ok = dt == PDX_INT64 || dt == PDX_UINT64 || dt == PDX_FLOAT64 || is_narrow(dt) || (timestamp_ok && dt == PDX_TIMESTAMP_NS);
  if (!ok) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": dtype " + dtype_name(dt) + " is not supported");
  if (!out) return fail(PDX_INVALID, std::string(who) + ": null output");
  if (out->dtype != dt || out->length < a->length) return fail(PDX_INVALID, std::string(who) + ": output dtype / length do not match the input");
  if (a->length > 0 && !out->values) return fail(PDX_INVALID, std::string(who) + ": null output buffer");
  if (a->length > 0 && out->values == a->values) return fail(PDX_INVALID, std::string(who) + ": in-place operation (out aliases the input) is not supported");
  return PDX_OK;
}

static CumArgs scan_args(const pdx_column* a, pdx_mut_column* out, int rev, int skip, unsigned long long* nulls) {
  CumArgs c;
  const size_t w = (size_t)dtype_bytes(a->dtype);
  c.in = static_cast<const char*>(a->values) + (size_t)a->offset * w;
  c.valid = validity_or_null(a);
  c.voff = a->offset;
  c.n = a->length;
  c.padded = round_up(a->length, kCumItems);
  c.rev = rev;
  c.vec = aligned16(c.in) && aligned16(out->values);
  c.skip = skip;
  c.out = out->values;
  c.ovalid = static_cast<uint8_t*>(out->validity);
  c.nulls = nulls;
  c.tile_nulls = nullptr;
  return c;
}

// Arrow's safe cast of the double `start` to the column's type: "Float value %f was truncated converting to <type>"
template <typename T>
static int cast_start(double start, const char* type_name, T* out) {
  constexpr double kLo = std::numeric_limits<T>::is_signed ? -(double)(1ull << (sizeof(T) * 8 - 2)) * 2.0 : 0.0;
  constexpr double kHi = (double)(1ull << (sizeof(T) * 8 - 2)) * (std::numeric_limits<T>::is_signed ? 2.0 : 4.0);  // exclusive
  if (!(start >= kLo && start < kHi) || (double)(T)start != start) {
    char buf[400];
    snprintf(buf, sizeof(buf), "Float value %f was truncated converting to %s", start, type_name);
    return fail(PDX_INVALID, buf);
  }
  *out = (T)start;
  return PDX_OK;
}

template <typename T> struct WrapType { using type = T; };
template <> struct WrapType<int64_t> { using type = uint64_t; };
template <> struct WrapType<int32_t> { using type = uint32_t; };

template <typename T, typename Op>
static int run_cumulative(const pdx_column* a, T start, int skip, pdx_mut_column* out, unsigned long long* nulls, Scratch& s, hipStream_t st) {
  const CumArgs c = scan_args(a, out, 0, skip, nulls);
  return cum_scan_launch<T, Op>(c, CumElem<T>{start, 1}, scan_chunk_tiles(), s, st);
}
template <typename T>
static int run_cumulative_op(int op, const pdx_column* a, T start, int skip, pdx_mut_column* out, unsigned long long* nulls, Scratch& s, hipStream_t st) {
  // sum / product of integers wrap: computed unsigned
  using U = typename WrapType<T>::type;
  switch (op) {
    case PDX_CUM_SUM: return run_cumulative<U, CumSum>(a, (U)start, skip, out, nulls, s, st);
    case PDX_CUM_PROD: return run_cumulative<U, CumProd>(a, (U)start, skip, out, nulls, s, st);
    case PDX_CUM_MAX: return run_cumulative<T, CumMax>(a, start, skip, out, nulls, s, st);
    default: return run_cumulative<T, CumMin>(a, start, skip, out, nulls, s, st);
  }
}

// ---------------------------------------------------------------- shift: out[i] = a[i - periods], or the fill
template <typename T>
__global__ void __launch_bounds__(256) k_shift(const T* __restrict__ in, const uint8_t* __restrict__ valid, int64_t voff, int64_t n, int64_t periods, T fillv,
                                               int fill_valid, T* __restrict__ out, uint8_t* __restrict__ ovalid, unsigned long long* __restrict__ nulls) {
  const int lane = threadIdx.x & 63;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long nc = 0;
  for (int64_t w = wave; w < nwords; w += nwaves) {
    const int64_t i = (w << 6) + lane, s = i - periods;
    const bool in_out = i < n, from_a = in_out && s >= 0 && s < n;
    bool ok = false;
    if (in_out) {
      out[i] = from_a ? in[s] : fillv;
      ok = from_a ? (!valid || bit_get(valid, voff + s)) : fill_valid != 0;
    }
    if (ovalid) {
      const unsigned long long word = __ballot(ok);  // (the last byte is written whole: not colview.hpp's tail-preserving store)
      if (lane < 8 && (w << 6) + lane * 8 < n) ovalid[(w << 3) + lane] = (uint8_t)(word >> (8 * lane));
      if (in_out && !ok) ++nc;
    }
  }
  if (ovalid) wave_add_nulls(nulls, lane, nc);
}

}  // namespace pdx

using namespace pdx;

extern "C" {

int pdx_cumulative(int op, const pdx_column* a, double start, int skip_nulls, pdx_mut_column* out, void* stream) {
  static const char* const kNames[] = {"cumulative_sum", "cumulative_prod", "cumulative_max", "cumulative_min"};
  if (op < PDX_CUM_SUM || op > PDX_CUM_MIN) return fail(PDX_INVALID, "pdx_cumulative: unknown op");
  if (a && (a->dtype == PDX_TIMESTAMP_NS || a->dtype == PDX_BOOL))
    return fail(PDX_NOT_IMPLEMENTED, std::string("Function '") + kNames[op] + "' has no kernel matching input types (" +
                                         (a->dtype == PDX_BOOL ? "bool" : "timestamp[ns]") + ")");
  PDX_TRY(check_io(a, out, "pdx_cumulative", false));
  // the start value in the column's type, checked before anything is launched
  int64_t si = 0;
  uint64_t su = 0;
  int32_t s32 = 0;
  switch (a->dtype) {
    case PDX_INT64: PDX_TRY(cast_start<int64_t>(start, "int64", &si)); break;
    case PDX_UINT64: PDX_TRY(cast_start<uint64_t>(start, "uint64", &su)); break;
    case PDX_INT32: PDX_TRY(cast_start<int32_t>(start, "int32", &s32)); break;
    default: break;  // float64: as is; float32: rounded to nearest
  }
  const bool has_nulls = validity_or_null(a) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_cumulative: input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  const int64_t n = a->length;
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  Scratch s;
  unsigned long long* nulls = nullptr;
  if (out->validity) PDX_TRY(open_null_counter(s, st, &nulls));  // only an output with a bitmap has a counter
  const int skip = skip_nulls != 0;
  switch (a->dtype) {
    case PDX_INT64: PDX_TRY(run_cumulative_op<int64_t>(op, a, si, skip, out, nulls, s, st)); break;
    case PDX_UINT64: PDX_TRY(run_cumulative_op<uint64_t>(op, a, su, skip, out, nulls, s, st)); break;
    case PDX_INT32: PDX_TRY(run_cumulative_op<int32_t>(op, a, s32, skip, out, nulls, s, st)); break;
    case PDX_FLOAT32: PDX_TRY(run_cumulative_op<float>(op, a, (float)start, skip, out, nulls, s, st)); break;
    default: PDX_TRY(run_cumulative_op<double>(op, a, start, skip, out, nulls, s, st)); break;
  }
  if (has_nulls) PDX_TRY(read_back(&out->null_count, nulls, sizeof(out->null_count), st));  // the one case that synchronises
  return PDX_OK;
}

int pdx_fill_null(int backward, const pdx_column* a, pdx_mut_column* out, void* stream) {
  if (a && a->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, "pdx_fill_null: dtype bool is not supported");
  PDX_TRY(check_io(a, out, "pdx_fill_null", true));
  const bool has_nulls = validity_or_null(a) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_fill_null: input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  const int64_t n = a->length;
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  Scratch s;
  unsigned long long* nulls = nullptr;
  if (out->validity) PDX_TRY(open_null_counter(s, st, &nulls));  // only an output with a bitmap has a counter
  const CumArgs c = scan_args(a, out, backward != 0, 0, nulls);
  if (dtype_bytes(a->dtype) == 4) PDX_TRY((cum_scan_launch<uint32_t, CumLatest>(c, CumElem<uint32_t>{0u, 0}, scan_chunk_tiles(), s, st)));
  else PDX_TRY((cum_scan_launch<uint64_t, CumLatest>(c, CumElem<uint64_t>{0ull, 0}, scan_chunk_tiles(), s, st)));
  if (has_nulls) PDX_TRY(read_back(&out->null_count, nulls, sizeof(out->null_count), st));
  return PDX_OK;
}

int pdx_shift(const pdx_column* a, int64_t periods, const pdx_scalar* fill, pdx_mut_column* out, void* stream) {
  if (a && a->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, "pdx_shift: dtype bool is not supported");
  PDX_TRY(check_io(a, out, "pdx_shift", true));
  if (fill && fill->dtype != a->dtype)
    return fail(PDX_INVALID, std::string("pdx_shift: fill value of dtype ") + dtype_name(fill->dtype) + " for a column of dtype " + dtype_name(a->dtype));
  const int64_t n = a->length;
  const bool fill_valid = fill && fill->is_valid;
  const int64_t mag = periods < 0 ? (periods == INT64_MIN ? INT64_MAX : -periods) : periods;
  const int64_t fills = mag < n ? mag : n;
  const bool has_nulls = validity_or_null(a) != nullptr;
  const bool may_null = (has_nulls && fills < n) || (!fill_valid && fills > 0);
  if (may_null && !out->validity) return fail(PDX_INVALID, "pdx_shift: the result can hold nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  Scratch s;
  unsigned long long* nulls = nullptr;
  if (out->validity) PDX_TRY(open_null_counter(s, st, &nulls));  // only an output with a bitmap has a counter
  const int64_t p = periods > n ? n : periods < -n ? -n : periods;  // |periods| >= length: a column of fills
  const dim3 grid(grid_for(n, 256, 4)), block(256);
  uint8_t* ov = static_cast<uint8_t*>(out->validity);
  if (dtype_bytes(a->dtype) == 4) {
    uint32_t fv = 0;
    if (fill_valid) {
      if (a->dtype == PDX_INT32) fv = (uint32_t)(int32_t)fill->v.i64;
      else {
        const float f = (float)fill->v.f64;
        memcpy(&fv, &f, 4);
      }
    }
    hipLaunchKernelGGL((k_shift<uint32_t>), grid, block, 0, st, static_cast<const uint32_t*>(a->values) + a->offset, validity_or_null(a), a->offset, n, p, fv,
                       (int)fill_valid, static_cast<uint32_t*>(out->values), ov, nulls);
  } else {
    const uint64_t fv = fill_valid ? fill->v.u64 : 0ull;
    hipLaunchKernelGGL((k_shift<uint64_t>), grid, block, 0, st, static_cast<const uint64_t*>(a->values) + a->offset, validity_or_null(a), a->offset, n, p, fv,
                       (int)fill_valid, static_cast<uint64_t*>(out->values), ov, nulls);
  }
  PDX_LAUNCH_CHECK();
  // known on the host unless rows of a column with nulls are kept: only then does the call synchronise
  if (fills == n || !has_nulls) out->null_count = fill_valid ? 0 : fills;
  else PDX_TRY(read_back(&out->null_count, nulls, sizeof(out->null_count), st));
  return PDX_OK;
}

}  // extern "C"
