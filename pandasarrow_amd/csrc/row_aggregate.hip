// row_aggregate.hip -- pdx_row_aggregate: for every row, Arrow's scalar aggregate over that row's cells across C columns
// (DataFrame::sum / mean / min / max / ... (AxisType::Columns), reference src/dataframe.cpp:136-229).
//
// Shape: a lane owns a row, a wave owns 64 consecutive rows.  A column read is one contiguous 512-byte (256 for 4-byte values) access
// per wave; the column loop runs inside the lane, kRowU column loads issued before the first is consumed.  The columns come as a device
// table (ColView) that every wave reads with uniform loads, as it reads one 64-bit validity word per column.  Output validity is one
// ballot per wave.  Every input byte is read once (twice for variance / stddev, whose second pass re-reads the row); no scratch but
// the table and the null counter.  The table, the bitmap windows and stores and the null counting are colview.hpp's.
//
// Bit parity with Arrow C++ 25: the fp64 sum of a row is pairwise.hpp's tree in column order (16-value leaves restarting at every run
// of valid cells, binary-counter merge, the NaN rule of each site), held per lane in registers (RowTree); variance is the two passes
// of gb_more_aggs.hpp through the same tree; min / max are a running fmin / fmax with minmax.hpp's tie rules (see RowMinMax).
#include <limits.h>
#include <math.h>
#include <string.h>
#include <string>
#include <vector>
#include "colview.hpp"
#include "pairwise.hpp"

namespace pdx {

constexpr int kRowU = 8;             // column loads in flight per lane
constexpr int kRowMaxCols = 2046;    // RowTree<10> holds the 1023 leaves of 2046 alternating cells (multiplex.hip's kMxMaxCols follows it)

struct RowOpts {
  int kind, skip, min_count, ddof;  // min_count clamped to [0, C + 1] by the host
};
struct RowOut {
  void* values;
  uint8_t* valid;              // nullptr: the caller knows that no row is null
  unsigned long long* nulls;   // nullptr: the host knows the count
};

// the null rule every kind but count shares: ScalarAggregateOptions{skip_nulls, min_count} against nv valid cells of C
__device__ __forceinline__ bool row_has_result(const RowOpts& p, int nv, int C) { return (p.skip || nv == C) && nv >= p.min_count; }

// Arrow's SumArray for one row, fed a cell at a time: the open leaf, and the binary counter as L registers (level l holds a node over
// 2^l leaves while bit l of mask is set, 0.0 otherwise -- so the counter's `sum[cur] += x` is one merge whether the level is taken or not).
template <int L>
struct RowTree {
  double leaf, s[L];
  int cnt;
  uint32_t mask;
  __device__ __forceinline__ void init() {
    leaf = 0.0;
    cnt = 0;
    mask = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) s[l] = 0.0;
  }
  __device__ __forceinline__ void push(double x) {
    bool carry = true;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const double m = pw_merge(s[l], x);
      const bool taken = (mask >> l) & 1u;
      s[l] = carry ? (taken ? 0.0 : m) : s[l];
      x = carry && taken ? m : x;
      carry = carry && taken;
    }
    ++mask;
  }
  __device__ __forceinline__ void add(double x, bool ok) {
    if (ok) {
      leaf = pw_leaf_add(leaf, x);
      ++cnt;
    }
    if (ok ? cnt == 16 : cnt > 0) {
      push(leaf);
      leaf = 0.0;
      cnt = 0;
    }
  }
  __device__ __forceinline__ double finish() {
    if (cnt > 0) push(leaf);
    const int root = mask ? 31 - __clz((int)mask) : 0;
    double r = s[0];
#pragma unroll
    for (int l = 1; l < L; ++l) {
      const double m = pw_merge(s[l], s[l - 1]);
      s[l] = l <= root ? m : s[l];
      r = l == root ? s[l] : r;
    }
    return r;
  }
};
// C <= 16 cells without nulls are one leaf: the chain alone (the counter's 0.0 + leaf changes no bit of it)
template <>
struct RowTree<0> {
  double leaf;
  __device__ __forceinline__ void init() { leaf = 0.0; }
  __device__ __forceinline__ void add(double x, bool) { leaf = pw_leaf_add(leaf, x); }
  __device__ __forceinline__ double finish() { return leaf; }
};

// ---------------------------------------------------------------- the per-kind state of a lane.  add() sees the cells in column order.
template <typename T, int L>
struct RowSumTree {  // sum (float32 / float64) and mean (every numeric dtype) -> float64
  using Out = double;
  static constexpr int kPasses = 1;
  RowTree<L> t;
  int nv;
  __device__ __forceinline__ void init(const RowOpts&) { t.init(); nv = 0; }
  __device__ __forceinline__ void next_pass() {}
  __device__ __forceinline__ void add(T v, bool ok, int, int) { t.add((double)v, ok); nv += ok; }
  __device__ __forceinline__ bool finish(const RowOpts& p, int C, Out& r) {
    const double sum = t.finish();
    if (p.kind == PDX_AGG_SUM) r = sum;
    else r = nv ? pw_mean(sum, (double)nv) : __longlong_as_double((long long)0xFFF8000000000000ull);  // x86's 0.0 / 0
    return row_has_result(p, nv, C);
  }
};
template <typename T>
struct RowSumInt {  // int64 / uint64 / int32 -> 64 bits, wrapping
  using Out = uint64_t;
  static constexpr int kPasses = 1;
  uint64_t acc;
  int nv;
  bool prod;
  __device__ __forceinline__ void init(const RowOpts& p) { acc = p.kind == PDX_AGG_PRODUCT ? 1ull : 0ull; nv = 0; prod = p.kind == PDX_AGG_PRODUCT; }
  __device__ __forceinline__ void next_pass() {}
  __device__ __forceinline__ void add(T v, bool ok, int, int) {
    const uint64_t x = (uint64_t)(long long)v;  // (int32 sign-extends; uint64 passes through)
    if (ok) acc = prod ? acc * x : acc + x;
    nv += ok;
  }
  __device__ __forceinline__ bool finish(const RowOpts& p, int C, Out& r) {
    r = acc;
    return row_has_result(p, nv, C);
  }
};
template <typename T>
struct RowProductF {  // float32 / float64 -> float64: one multiply per valid cell in column order
  using Out = double;
  static constexpr int kPasses = 1;
  double acc;
  int nv;
  __device__ __forceinline__ void init(const RowOpts&) { acc = 1.0; nv = 0; }
  __device__ __forceinline__ void next_pass() {}
  __device__ __forceinline__ void add(T v, bool ok, int, int) {
    if (ok) acc = acc * (double)v;
    nv += ok;
  }
  __device__ __forceinline__ bool finish(const RowOpts& p, int C, Out& r) {
    r = acc;
    return row_has_result(p, nv, C);
  }
};
template <typename T> struct RowBits { using type = uint64_t; };
template <> struct RowBits<int32_t> { using type = uint32_t; };
template <> struct RowBits<float> { using type = uint32_t; };
template <typename T>
__device__ __forceinline__ typename RowBits<T>::type row_bits_of(T v) {
  typename RowBits<T>::type b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}
// Arrow's min / max, a running fmin / fmax over the valid cells: a quiet NaN cell takes no part; a SIGNALLING one makes the running extreme
// NaN, which the next number replaces (glibc's fmin / fmax, measured against Arrow 25: min([5, sNaN, 7]) is 7) -- so the result is NaN when
// no number follows the last signalling NaN, or every valid cell is NaN.  Between cells that compare equal (0.0 / -0.0) min keeps the
// first; max keeps the first, except float64 in a row with a null cell: the last (minmax.hpp; float32's fmaxf keeps the first there too).
template <typename T> __device__ __forceinline__ bool row_signalling(T) { return false; }
template <> __device__ __forceinline__ bool row_signalling<double>(double v) { return v != v && !(__double_as_longlong(v) & 0x0008000000000000ll); }
template <> __device__ __forceinline__ bool row_signalling<float>(float v) { return v != v && !(__float_as_uint(v) & 0x00400000u); }
template <typename T>
struct RowMinMax {
  using Out = typename RowBits<T>::type;
  static constexpr int kPasses = 1;
  T lo, hi_first, hi_last;
  bool have;
  int nv;
  __device__ __forceinline__ void init(const RowOpts&) { lo = hi_first = hi_last = T(0); have = false; nv = 0; }
  __device__ __forceinline__ void next_pass() {}
  __device__ __forceinline__ void add(T v, bool ok, int, int) {
    nv += ok;
    if (ok && v == v) {
      if (!have || v < lo) lo = v;
      if (!have || v > hi_first) hi_first = v;
      if (!have || !(v < hi_last)) hi_last = v;
      have = true;
    } else if (ok && row_signalling(v)) {
      have = false;
    }
  }
  __device__ __forceinline__ bool finish(const RowOpts& p, int C, Out& r) {
    T x = p.kind == PDX_AGG_MIN ? lo : (__is_same(T, double) && nv < C ? hi_last : hi_first);
    if constexpr (__is_same(T, double) || __is_same(T, float)) {
      if (!have) x = (T)__longlong_as_double(0x7FF8000000000000ll);  // every valid cell is NaN
    }
    r = row_bits_of(x);
    return nv > 0 && row_has_result(p, nv, C);
  }
};
// first / last: with skip_nulls the first / last valid cell, without it the first / last cell (null when that cell is null)
template <typename B>
struct RowFirstLast {
  using Out = B;
  static constexpr int kPasses = 1;
  B val;
  bool have, edge_ok, last;
  int nv;
  __device__ __forceinline__ void init(const RowOpts& p) { val = 0; have = false; edge_ok = false; nv = 0; last = p.kind == PDX_AGG_LAST; }
  __device__ __forceinline__ void next_pass() {}
  __device__ __forceinline__ void add(B v, bool ok, int col, int C) {
    nv += ok;
    if (ok && (last || !have)) { val = v; have = true; }
    if (col == (last ? C - 1 : 0)) edge_ok = ok;
  }
  __device__ __forceinline__ bool finish(const RowOpts& p, int C, Out& r) {
    r = val;
    return have && nv >= p.min_count && (p.skip || edge_ok);
  }
};
// variance / stddev of float64 / int64 cells: mean = tree sum / count, then the tree sum of (x - mean)^2, over (count - ddof)
// (int64: Arrow sums the first pass exactly, in 128 bits, and rounds once -- here a 64-bit sum with its carries, converted by hand)
__device__ __forceinline__ double row_i128_to_double(long long hi, unsigned long long lo) {
  const bool neg = hi < 0;
  if (neg) {  // magnitude
    lo = ~lo + 1ull;
    hi = ~hi + (lo == 0ull);
  }
  double r;
  if (hi == 0) {
    r = (double)lo;
  } else {  // the top 64 bits, the bits below them folded into a sticky bit: one rounding, then an exact scale
    const int sh = __clzll(hi);
    unsigned long long top = sh ? ((unsigned long long)hi << sh) | (lo >> (64 - sh)) : (unsigned long long)hi;
    if (sh ? (lo << sh) != 0ull : lo != 0ull) top |= 1ull;
    r = ldexp((double)top, 64 - sh);
  }
  return neg ? -r : r;
}
template <typename T, int L>
struct RowVar {
  using Out = double;
  static constexpr int kPasses = 2;
  static constexpr bool kInt = !__is_same(T, double);
  RowTree<L> t;
  int nv;
  double mean;
  bool second;
  long long hi;
  unsigned long long lo;
  __device__ __forceinline__ void init(const RowOpts&) { t.init(); nv = 0; mean = 0.0; second = false; hi = 0; lo = 0; }
  __device__ __forceinline__ void next_pass() {
    const double sum = kInt ? row_i128_to_double(hi, lo) : t.finish();
    mean = nv ? pw_mean(sum, (double)nv) : 0.0;
    t.init();
    second = true;
  }
  __device__ __forceinline__ void add(T v, bool ok, int, int) {
    double x = (double)v;
    if (second) {
      const double d = x - mean;
      x = d * d;
    } else {
      nv += ok;
      if constexpr (kInt) {
        if (ok) {
          const unsigned long long u = (unsigned long long)v, s = lo + u;
          hi += (long long)(s < lo) - (long long)(v < 0);
          lo = s;
        }
        return;
      }
    }
    t.add(x, ok);
  }
  __device__ __forceinline__ bool finish(const RowOpts& p, int C, Out& r) {
    const double m2 = t.finish();
    const double var = nv > p.ddof ? m2 / (double)(nv - p.ddof) : 0.0;
    r = p.kind == PDX_AGG_VARIANCE ? var : sqrt(var);
    return nv > p.ddof && row_has_result(p, nv, C);
  }
};

template <typename R>
__device__ __forceinline__ void row_emit(const RowOut& o, int64_t w, int64_t n, int lane, bool in, bool ok, R r, unsigned long long& nc) {
  if (in) static_cast<R*>(o.values)[(w << 6) + lane] = ok ? r : R(0);
  if (o.valid) {
    store_bits_wave(o.valid, w, n, __ballot(ok), lane);
    if (in && !ok) ++nc;
  }
}

template <typename T, typename Op>
__global__ void __launch_bounds__(256) k_row_agg(const ColView* __restrict__ tab, int ncols, int64_t n, RowOpts p, RowOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t nwords = (n + 63) >> 6, nwaves = (int64_t)(gridDim.x * blockDim.x) >> 6;
  unsigned long long nc = 0;
  for (int64_t w = first_word_of_wave(); w < nwords; w += nwaves) {
    const int64_t base = w << 6, i = base + lane;
    const bool in = i < n;
    const int nbits = n - base < 64 ? (int)(n - base) : 64;
    Op op;
    op.init(p);
    for (int pass = 0; pass < Op::kPasses; ++pass) {
      if (pass) op.next_pass();
      for (int c0 = 0; c0 < ncols; c0 += kRowU) {
        T v[kRowU];
        uint64_t vw[kRowU];
#pragma unroll
        for (int u = 0; u < kRowU; ++u) {
          v[u] = T(0);
          vw[u] = 0;
          if (c0 + u < ncols) {
            const ColView e = tab[c0 + u];
            vw[u] = e.valid ? load_bits64_uniform(e.valid, e.voff + base, nbits) : ~0ull;
            if (in) v[u] = ((const __attribute__((address_space(1))) T*)e.values)[i];  // (a global load, not a flat one: the table hides the address space)
          }
        }
#pragma unroll
        for (int u = 0; u < kRowU; ++u)
          if (c0 + u < ncols) op.add(v[u], in && ((vw[u] >> lane) & 1ull), c0 + u, ncols);
      }
    }
    typename Op::Out r;
    const bool ok = op.finish(p, ncols, r) && in;
    row_emit(o, w, n, lane, in, ok, r, nc);
  }
  if (o.nulls) wave_add_nulls(o.nulls, lane, nc);
}

// count / count_null: the validity words alone -> int64, never null
__global__ void __launch_bounds__(256) k_row_count(const ColView* __restrict__ tab, int ncols, int64_t n, int only_null, long long* __restrict__ out,
                                                   uint8_t* __restrict__ ovalid) {
  const int lane = threadIdx.x & 63;
  const int64_t nwords = (n + 63) >> 6, nwaves = (int64_t)(gridDim.x * blockDim.x) >> 6;
  for (int64_t w = first_word_of_wave(); w < nwords; w += nwaves) {
    const int64_t base = w << 6, i = base + lane;
    const int nbits = n - base < 64 ? (int)(n - base) : 64;
    int nv = 0;
    for (int c = 0; c < ncols; ++c) {
      const ColView e = tab[c];
      const uint64_t vw = e.valid ? load_bits64_uniform(e.valid, e.voff + base, nbits) : ~0ull;
      nv += (int)((vw >> lane) & 1ull);
    }
    if (i < n) out[i] = only_null ? ncols - nv : nv;
    if (ovalid) store_bits_wave(ovalid, w, n, ~0ull, lane);
  }
}

// all / any of bit-packed cells: a value word and a validity word per column and wave.  skip_nulls: over the valid cells (none: all is
// true, any false); otherwise a null cell makes the row null unless a valid cell already decides it (a false for all, a true for any).
__global__ void __launch_bounds__(256) k_row_all_any(const ColView* __restrict__ tab, int ncols, int64_t n, RowOpts p, RowOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t nwords = (n + 63) >> 6, nwaves = (int64_t)(gridDim.x * blockDim.x) >> 6;
  const bool is_all = p.kind == PDX_AGG_ALL;
  unsigned long long nc = 0;
  for (int64_t w = first_word_of_wave(); w < nwords; w += nwaves) {
    const int64_t base = w << 6;
    const bool in = base + lane < n;
    const int nbits = n - base < 64 ? (int)(n - base) : 64;
    uint64_t seen_true = 0, seen_false = 0, full = ~0ull;  // per row: a valid true cell, a valid false cell, no null cell
    int nv = 0;
    for (int c = 0; c < ncols; ++c) {
      const ColView e = tab[c];
      const uint64_t vw = e.valid ? load_bits64_uniform(e.valid, e.voff + base, nbits) : ~0ull;
      const uint64_t bw = load_bits64_uniform(static_cast<const uint8_t*>(e.values), e.boff + base, nbits);
      seen_true |= vw & bw;
      seen_false |= vw & ~bw;
      full &= vw;
      nv += (int)((vw >> lane) & 1ull);
    }
    const uint64_t value = is_all ? ~seen_false : seen_true;
    const uint64_t decided = is_all ? seen_false : seen_true;
    const bool ok = in && nv >= p.min_count && (p.skip || (((full | decided) >> lane) & 1ull));
    store_bits_wave(static_cast<uint8_t*>(o.values), w, n, value & __ballot(ok), lane);
    if (o.valid) {
      store_bits_wave(o.valid, w, n, __ballot(ok), lane);
      if (in && !ok) ++nc;
    }
  }
  if (o.nulls) wave_add_nulls(o.nulls, lane, nc);
}

// ---------------------------------------------------------------- host side
static const char* row_kind_name(int kind) {
  static const char* const kNames[] = {"sum", "mean", "min", "max", "count", "variance", "stddev", "product", "first", "last", "all", "any", "count_distinct", "count"};
  return kNames[kind];
}

template <typename T, typename Op>
static void row_launch(const ColView* tab, int C, int64_t n, const RowOpts& p, const RowOut& o, hipStream_t st) {
  // rows per thread 1: a lane's state is a row; the grid strides over 64-row words
  hipLaunchKernelGGL((k_row_agg<T, Op>), dim3(grid_for(n, 256)), dim3(256), 0, st, tab, C, n, p, o);
}
// the counter depth a row can need: up to ceil(C / 2) leaves when cells can be null (alternating), ceil(C / 16) otherwise
static int row_tree_levels(int C, bool any_validity) {
  if (!any_validity && C <= 16) return 0;
  const int leaves = any_validity ? (C + 1) / 2 : (C + 15) / 16;
  return leaves < 16 ? 4 : leaves < 128 ? 7 : 10;
}
template <typename T, template <typename, int> class Op>
static void row_launch_tree(int levels, const ColView* tab, int C, int64_t n, const RowOpts& p, const RowOut& o, hipStream_t st) {
  switch (levels) {
    case 0: return row_launch<T, Op<T, 0>>(tab, C, n, p, o, st);
    case 4: return row_launch<T, Op<T, 4>>(tab, C, n, p, o, st);
    case 7: return row_launch<T, Op<T, 7>>(tab, C, n, p, o, st);
    default: return row_launch<T, Op<T, 10>>(tab, C, n, p, o, st);
  }
}

}  // namespace pdx

using namespace pdx;

extern "C" int pdx_row_aggregate(int kind, const pdx_column* cols, int ncols, int skip_nulls, int64_t min_count, int ddof, pdx_mut_column* out,
                                 void* stream) {
  const char* who = "pdx_row_aggregate";
  if (kind == PDX_AGG_COUNT_DISTINCT) return fail(PDX_NOT_IMPLEMENTED, "pdx_row_aggregate: count_distinct over a row is not implemented");
  if (kind < PDX_AGG_SUM || kind > PDX_AGG_COUNT_NULL) return fail(PDX_INVALID, "pdx_row_aggregate: unknown kind");
  if (!cols || ncols <= 0) return fail(PDX_INVALID, "pdx_row_aggregate: at least one column is required");
  if (ncols > kRowMaxCols) return fail(PDX_INVALID, "pdx_row_aggregate: more than " + std::to_string(kRowMaxCols) + " columns");
  for (int c = 0; c < ncols; ++c) PDX_TRY(check_column(&cols[c], who, true));
  const int dt = cols[0].dtype;
  const int64_t n = cols[0].length;
  const int C = ncols;
  bool any_validity = false;
  for (int c = 0; c < C; ++c) {
    if (cols[c].dtype != dt)
      return fail(PDX_INVALID, std::string(who) + ": column " + std::to_string(c) + " is " + dtype_name(cols[c].dtype) + ", column 0 " + dtype_name(dt) +
                                   " (the cells of a row must share one type)");
    if (cols[c].length != n) return fail(PDX_INVALID, std::string(who) + ": Array arguments must all be the same length");
    any_validity = any_validity || validity_or_null(&cols[c]) != nullptr;
  }
  // which (kind, dtype) pairs Arrow has a kernel for, narrowed to what this library carries
  const bool is_count = kind == PDX_AGG_COUNT || kind == PDX_AGG_COUNT_NULL;
  const bool is_var = kind == PDX_AGG_VARIANCE || kind == PDX_AGG_STDDEV;
  const bool is_bool_kind = kind == PDX_AGG_ALL || kind == PDX_AGG_ANY;
  const bool keeps_dtype = kind == PDX_AGG_MIN || kind == PDX_AGG_MAX || kind == PDX_AGG_FIRST || kind == PDX_AGG_LAST;
  bool accepted;
  switch (dt) {
    case PDX_BOOL: accepted = is_bool_kind || is_count; break;
    case PDX_TIMESTAMP_NS: accepted = keeps_dtype || is_count; break;
    case PDX_INT64: case PDX_FLOAT64: accepted = !is_bool_kind; break;
    case PDX_UINT64: case PDX_INT32: case PDX_FLOAT32: accepted = !is_bool_kind && !is_var; break;  // (variance: what pdx_groupby_agg accepts)
    default: return fail(PDX_INVALID, std::string(who) + ": unknown dtype");
  }
  if (!accepted)
    return fail(PDX_NOT_IMPLEMENTED, std::string("Function '") + row_kind_name(kind) + "' has no kernel matching input types (" + arrow_dtype_name(dt) + ")");
  const bool is_f = dt == PDX_FLOAT64 || dt == PDX_FLOAT32;
  int want;
  if (is_count) want = PDX_INT64;
  else if (is_bool_kind) want = PDX_BOOL;
  else if (keeps_dtype) want = dt;
  else if (kind == PDX_AGG_SUM || kind == PDX_AGG_PRODUCT) want = is_f ? PDX_FLOAT64 : dt == PDX_UINT64 ? PDX_UINT64 : PDX_INT64;
  else want = PDX_FLOAT64;
  PDX_TRY(check_out(who, out, want, n));
  RowOpts p;
  p.kind = kind;
  p.skip = skip_nulls != 0;
  p.min_count = (int)(min_count < 0 ? 0 : min_count > C + 1 ? C + 1 : min_count);
  p.ddof = ddof;
  // can a row be null?  Without a bitmap on any column every row has C valid cells and the answer is one for all rows.
  const bool all_valid_null = !is_count && (C < p.min_count || (is_var && (int64_t)C <= (int64_t)ddof));
  bool may_null;
  if (is_count) may_null = false;
  else if (!any_validity) may_null = all_valid_null;
  else may_null = all_valid_null || !(kind == PDX_AGG_SUM || kind == PDX_AGG_MEAN || kind == PDX_AGG_PRODUCT || is_bool_kind) || !p.skip || p.min_count > 0;
  if (may_null && !out->validity) return fail(PDX_INVALID, std::string(who) + ": the result can hold nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;

  Scratch s;
  std::vector<ColView> host;
  for (int c = 0; c < C; ++c) host.push_back(col_view(cols[c]));
  const ColView* tab;
  PDX_TRY(upload_views(s, host, st, &tab));
  RowOut o;
  o.values = out->values;
  o.valid = static_cast<uint8_t*>(out->validity);
  o.nulls = nullptr;
  const bool count_on_device = may_null && any_validity && !all_valid_null;
  if (count_on_device) PDX_TRY(open_null_counter(s, st, &o.nulls));
  const dim3 grid(grid_for(n, 256)), block(256);
  if (is_count) {
    hipLaunchKernelGGL(k_row_count, grid, block, 0, st, tab, C, n, (int)(kind == PDX_AGG_COUNT_NULL), static_cast<long long*>(out->values),
                       static_cast<uint8_t*>(out->validity));
  } else if (is_bool_kind) {
    hipLaunchKernelGGL(k_row_all_any, grid, block, 0, st, tab, C, n, p, o);
  } else if (keeps_dtype && (kind == PDX_AGG_FIRST || kind == PDX_AGG_LAST)) {
    if (dtype_bytes(dt) == 4) row_launch<uint32_t, RowFirstLast<uint32_t>>(tab, C, n, p, o, st);
    else row_launch<uint64_t, RowFirstLast<uint64_t>>(tab, C, n, p, o, st);
  } else if (keeps_dtype) {
    switch (dt) {
      case PDX_FLOAT64: row_launch<double, RowMinMax<double>>(tab, C, n, p, o, st); break;
      case PDX_FLOAT32: row_launch<float, RowMinMax<float>>(tab, C, n, p, o, st); break;
      case PDX_UINT64: row_launch<uint64_t, RowMinMax<uint64_t>>(tab, C, n, p, o, st); break;
      case PDX_INT32: row_launch<int32_t, RowMinMax<int32_t>>(tab, C, n, p, o, st); break;
      default: row_launch<int64_t, RowMinMax<int64_t>>(tab, C, n, p, o, st); break;
    }
  } else if (is_var) {
    const int lv = row_tree_levels(C, any_validity);
    if (dt == PDX_FLOAT64) row_launch_tree<double, RowVar>(lv, tab, C, n, p, o, st);
    else row_launch_tree<int64_t, RowVar>(lv, tab, C, n, p, o, st);
  } else if (kind == PDX_AGG_MEAN || (kind == PDX_AGG_SUM && is_f)) {
    const int lv = row_tree_levels(C, any_validity);
    switch (dt) {
      case PDX_FLOAT64: row_launch_tree<double, RowSumTree>(lv, tab, C, n, p, o, st); break;
      case PDX_FLOAT32: row_launch_tree<float, RowSumTree>(lv, tab, C, n, p, o, st); break;
      case PDX_UINT64: row_launch_tree<uint64_t, RowSumTree>(lv, tab, C, n, p, o, st); break;
      case PDX_INT32: row_launch_tree<int32_t, RowSumTree>(lv, tab, C, n, p, o, st); break;
      default: row_launch_tree<int64_t, RowSumTree>(lv, tab, C, n, p, o, st); break;
    }
  } else if (is_f) {  // product of floats
    if (dt == PDX_FLOAT64) row_launch<double, RowProductF<double>>(tab, C, n, p, o, st);
    else row_launch<float, RowProductF<float>>(tab, C, n, p, o, st);
  } else {  // integer sum / product
    switch (dt) {
      case PDX_UINT64: row_launch<uint64_t, RowSumInt<uint64_t>>(tab, C, n, p, o, st); break;
      case PDX_INT32: row_launch<int32_t, RowSumInt<int32_t>>(tab, C, n, p, o, st); break;
      default: row_launch<int64_t, RowSumInt<int64_t>>(tab, C, n, p, o, st); break;
    }
  }
  PDX_LAUNCH_CHECK();
  // the null count is known on the host unless rows differ, i.e. a column brings a bitmap: only then is it read back (the one host wait)
  if (all_valid_null) out->null_count = n;
  else if (count_on_device) PDX_TRY(read_back(&out->null_count, o.nulls, sizeof(out->null_count), st));
  return PDX_OK;
}
