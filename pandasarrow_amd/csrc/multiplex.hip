// multiplex.hip -- selection / multiplexing and null handling: pdx_coalesce, pdx_element_wise_minmax / pdx_clip, pdx_replace_with_mask,
// pdx_indices_nonzero(_count) and pdx_all_valid_mask (the row mask of drop_null).
//
// Replaces (reference file:line)
//   DataFrame::coalesce() / coalesce(columns)   : CallFunction("coalesce", columns)                       src/dataframe.cpp:1210-1225
//   Series::clip(x, min, max, skipNull)         : MaxElementWise({MinElementWise({x, max}), min})        src/series.cpp:874-880
//   Series::replace_with_mask(cond, other)      : ReplaceWithMask(array, cond, other)                    src/series.cpp:752-761
//   Series::drop_na / DataFrame::drop_na        : "drop_null" / DropNull(batch + index)                  src/series.cpp:363, src/dataframe.cpp:1244-1252
//   Series::indices_nonzero                     : "indices_nonzero"                                      src/series.cpp:365
//
// Shapes.  coalesce and min / max: a lane owns a row (four consecutive rows of a 4-byte coalesce whose streams start on 16 bytes), a wave
// 64 (256) consecutive rows; the columns come as a device table (colview.hpp's ColView) read with uniform loads, as the 64-bit validity words are.  coalesce keeps
// the rows of its words that still lack a value as wave-uniform masks: a column is loaded only by the lanes it gives a value to, and the
// column loop ends when no row is pending -- a frame whose first column is mostly valid moves about one column.  clip folds both levels
// of the nesting over one read of x.  replace_with_mask is compact.hpp's two passes: valid-true mask rows per tile, scanned, then a pass
// that ranks within the tile (ballot + popcount) and gathers from the replacement.  indices_nonzero is compact.hpp with a predicate.
// all_valid_mask ANDs the bitmaps at their own bit offsets, one 64-bit word per lane.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "colview.hpp"
#include "compact.hpp"

namespace pdx {

constexpr int kMxMaxCols = 2046;  // as pdx_row_aggregate (row_aggregate.hip's kRowMaxCols)
constexpr int kMxU = 4;           // column loads in flight per lane

template <typename B>
using MxV4 = B __attribute__((ext_vector_type(4)));  // 16 bytes of a 4-byte stream
// the R bits of this lane's rows (R * lane ... R * lane + R - 1 of the wave's 64 R rows) out of R wave-uniform words
template <int R>
__device__ __forceinline__ uint32_t mx_lane_bits(const uint64_t (&w)[R], int lane) {
  if constexpr (R == 1) {
    return (uint32_t)((w[0] >> lane) & 1ull);
  } else {
    static_assert(R == 4, "one row or four rows per lane");
    const int j = lane >> 4;
    const uint64_t x = j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3];
    return (uint32_t)((x >> ((lane & 15) * 4)) & 0xFull);
  }
}

// ---------------------------------------------------------------- coalesce
// pend: the rows of the wave's words that no column has given a value yet.  A column takes `pend & its validity word`; only the lanes
// with a bit there load from it.  Values travel as bits (B = uint32_t / uint64_t), so NaN payloads and -0.0 survive.
template <typename B, int R>
__global__ void __launch_bounds__(256) k_coalesce(const ColView* __restrict__ tab, int ncols, int64_t n, B* __restrict__ out, uint8_t* __restrict__ ovalid,
                                                  unsigned long long* __restrict__ nulls) {
  const int lane = threadIdx.x & 63;
  constexpr int64_t kRows = 64 * R;
  const int64_t ngroups = (n + kRows - 1) / kRows, nwaves = (int64_t)(gridDim.x * blockDim.x) >> 6;
  unsigned long long nc = 0;  // (wave-uniform)
  for (int64_t g = first_word_of_wave(); g < ngroups; g += nwaves) {
    const int64_t base = g * kRows;
    const bool full = base + kRows <= n;
    uint64_t inr[R], pend[R];
    int nbits[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t rem = n - (base + 64 * j);
      nbits[j] = rem >= 64 ? 64 : rem > 0 ? (int)rem : 0;
      inr[j] = in_range_mask(rem);
      pend[j] = inr[j];
    }
    B val[R];
#pragma unroll
    for (int k = 0; k < R; ++k) val[k] = B(0);
    for (int c0 = 0; c0 < ncols; c0 += kMxU) {
      uint32_t nib[kMxU];
      B v[kMxU][R];
#pragma unroll
      for (int u = 0; u < kMxU; ++u) {
        nib[u] = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) v[u][k] = B(0);
        if (c0 + u < ncols) {
          const ColView e = tab[c0 + u];
          uint64_t take[R];
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const uint64_t vw = !nbits[j] ? 0ull : e.valid ? load_bits64_uniform(e.valid, e.voff + base + 64 * j, nbits[j]) : ~0ull;
            take[j] = pend[j] & vw;
            pend[j] &= ~vw;
          }
          nib[u] = mx_lane_bits<R>(take, lane);
          if (nib[u]) {
            const __attribute__((address_space(1))) B* src = (const __attribute__((address_space(1))) B*)e.values + base + R * lane;
            if constexpr (R == 4) {
              if (full) {
                const MxV4<B> x = *reinterpret_cast<const __attribute__((address_space(1))) MxV4<B>*>(src);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[u][k] = x[k];
              } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                  if ((nib[u] >> k) & 1u) v[u][k] = src[k];
              }
            } else {
              v[u][0] = src[0];
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kMxU; ++u)
#pragma unroll
        for (int k = 0; k < R; ++k)
          if ((nib[u] >> k) & 1u) val[k] = v[u][k];
      uint64_t left = 0;
#pragma unroll
      for (int j = 0; j < R; ++j) left |= pend[j];
      if (!left) break;
    }
    if constexpr (R == 4) {
      if (full) {
        MxV4<B> x;
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = val[k];
        *reinterpret_cast<MxV4<B>*>(out + base + 4 * lane) = x;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (base + 4 * lane + k < n) out[base + 4 * lane + k] = val[k];
      }
    } else {
      if (base + lane < n) out[base + lane] = val[0];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (!nbits[j]) continue;
      if (ovalid) store_bits_wave(ovalid, g * R + j, n, inr[j] & ~pend[j], lane);
      nc += (unsigned long long)__popcll(pend[j]);
    }
  }
  if (nulls && lane == 0 && nc) atomicAdd(nulls, nc);
}
// bit-packed cells: a thread owns a 64-row word of every column
__global__ void __launch_bounds__(256) k_coalesce_bool(const ColView* __restrict__ tab, int ncols, int64_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ ovalid,
                                                       unsigned long long* __restrict__ nulls) {
  const int64_t nwords = (n + 63) >> 6, stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long nc = 0;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    const int64_t base = w << 6;
    const uint64_t inr = in_range_mask(n - base);
    uint64_t pend = inr, val = 0;
    for (int c = 0; c < ncols && pend; ++c) {
      const ColView e = tab[c];
      const uint64_t vw = e.valid ? load_bits64(e.valid, e.voff + base, e.voff + n) : ~0ull;
      const uint64_t take = pend & vw;
      if (take) val |= take & load_bits64(static_cast<const uint8_t*>(e.values), e.boff + base, e.boff + n);
      pend &= ~vw;
    }
    store_bits_word(out, w, n, val);
    if (ovalid) store_bits_word(ovalid, w, n, inr & ~pend);
    nc += (unsigned long long)__popcll(pend);
  }
  if (nulls) wave_add_nulls(nulls, threadIdx.x & 63, nc);
}

// ---------------------------------------------------------------- min_element_wise / max_element_wise, clip
// Arrow folds every valid cell of a row through Call(accumulator, cell), the scalars first, then the arrays.  Integers: std::min /
// std::max.  Floats: fmin / fmax as they behave under Arrow 25 on x86-64 (tests/golden/multiplex_golden.npz): the accumulator starts as a
// quiet NaN; a signalling NaN on either side gives NaN; otherwise a NaN loses to the other side; of two values that compare equal
// (0.0 / -0.0) the accumulator stays -- except that a float32 ARRAY cell replaces it when the 64-row block of that array around the cell
// holds no null (Arrow's loop over an all-valid block is compiled differently from its loop over a block with nulls; a wave's word IS
// that block).  The first valid scalar becomes the accumulator as it is.
template <typename T>
constexpr bool mx_is_float() { return __is_same(T, double) || __is_same(T, float); }
template <typename T> __device__ __forceinline__ bool mx_signalling(T) { return false; }
template <> __device__ __forceinline__ bool mx_signalling<double>(double v) { return v != v && !(__double_as_longlong(v) & 0x0008000000000000ll); }
template <> __device__ __forceinline__ bool mx_signalling<float>(float v) { return v != v && !(__float_as_uint(v) & 0x00400000u); }
template <typename T>
__device__ __forceinline__ T mx_quiet_nan() {
  if constexpr (__is_same(T, double)) return __longlong_as_double(0x7FF8000000000000ll);
  else if constexpr (__is_same(T, float)) return __uint_as_float(0x7FC00000u);
  else return T(0);
}
template <typename T>
__device__ __forceinline__ T mx_fold(bool is_max, T acc, T v, bool tie_later) {
  if constexpr (mx_is_float<T>()) {
    if (mx_signalling(acc) || mx_signalling(v)) return mx_quiet_nan<T>();
    if (acc != acc) return v;
    if (v != v) return acc;
    const bool better = is_max ? v > acc : v < acc, worse = is_max ? v < acc : v > acc;
    return better ? v : worse ? acc : tie_later ? v : acc;
  } else {
    return is_max ? (v > acc ? v : acc) : (v < acc ? v : acc);
  }
}
template <typename T>
struct MxAcc {
  T acc;
  bool have, every;
  __device__ __forceinline__ void init() { acc = mx_quiet_nan<T>(); have = false; every = true; }
  __device__ __forceinline__ void scalar(bool is_max, T v, bool ok) {
    every = every && ok;
    if (ok) acc = have ? mx_fold(is_max, acc, v, false) : v;
    have = have || ok;
  }
  __device__ __forceinline__ void cell(bool is_max, T v, bool ok, bool block_full) {
    every = every && ok;
    if (ok) acc = (mx_is_float<T>() || have) ? mx_fold(is_max, acc, v, __is_same(T, float) && block_full) : v;
    have = have || ok;
  }
  __device__ __forceinline__ bool good(bool skip) const { return skip ? have : every; }
};

// tab: the nscalar broadcast operands (one value each), then the arrays.  CLIP: tab = {x, hi, lo}: max(min(x, hi), lo), each level with
// the options on its own, over one read of x.
template <typename T, bool CLIP>
__global__ void __launch_bounds__(256) k_minmax(const ColView* __restrict__ tab, int nscalar, int ncols, int64_t n, int is_max_i, int skip_i, T* __restrict__ out,
                                                uint8_t* __restrict__ ovalid, unsigned long long* __restrict__ nulls) {
  const int lane = threadIdx.x & 63;
  const bool is_max = is_max_i != 0, skip = skip_i != 0;
  const int64_t nwords = (n + 63) >> 6, nwaves = (int64_t)(gridDim.x * blockDim.x) >> 6;
  MxAcc<T> s0;
  s0.init();
  T hi = T(0), lo = T(0);
  bool hi_ok = false, lo_ok = false;
  if constexpr (CLIP) {
    const ColView eh = tab[1], el = tab[2];
    hi = static_cast<const T*>(eh.values)[0];
    lo = static_cast<const T*>(el.values)[0];
    hi_ok = !eh.valid || bit_get(eh.valid, eh.voff);
    lo_ok = !el.valid || bit_get(el.valid, el.voff);
  } else {
    for (int s = 0; s < nscalar; ++s) {
      const ColView e = tab[s];
      s0.scalar(is_max, static_cast<const T*>(e.values)[0], !e.valid || bit_get(e.valid, e.voff));
    }
  }
  unsigned long long nc = 0;
  for (int64_t w = first_word_of_wave(); w < nwords; w += nwaves) {
    const int64_t base = w << 6, i = base + lane;
    const bool in = i < n;
    const int nbits = n - base < 64 ? (int)(n - base) : 64;
    const uint64_t inr = in_range_mask(nbits);
    T r;
    bool ok;
    if constexpr (CLIP) {
      const ColView e = tab[0];
      const uint64_t vw = e.valid ? load_bits64_uniform(e.valid, e.voff + base, nbits) : ~0ull;
      const T x = in ? ((const __attribute__((address_space(1))) T*)e.values)[i] : T(0);
      MxAcc<T> a, b;
      a.init();
      a.scalar(false, hi, hi_ok);
      a.cell(false, x, in && ((vw >> lane) & 1ull), (vw & inr) == inr);
      b.init();
      b.scalar(true, lo, lo_ok);
      const bool inner_ok = in && a.good(skip);
      b.cell(true, a.acc, inner_ok, __ballot(inner_ok) == inr);
      ok = in && b.good(skip);
      r = b.acc;
    } else {
      MxAcc<T> a = s0;
      for (int c0 = nscalar; c0 < ncols; c0 += kMxU) {
        T v[kMxU];
        uint64_t vw[kMxU];
#pragma unroll
        for (int u = 0; u < kMxU; ++u) {
          v[u] = T(0);
          vw[u] = 0;
          if (c0 + u < ncols) {
            const ColView e = tab[c0 + u];
            vw[u] = e.valid ? load_bits64_uniform(e.valid, e.voff + base, nbits) : ~0ull;
            if (in) v[u] = ((const __attribute__((address_space(1))) T*)e.values)[i];
          }
        }
#pragma unroll
        for (int u = 0; u < kMxU; ++u)
          if (c0 + u < ncols) a.cell(is_max, v[u], in && ((vw[u] >> lane) & 1ull), (vw[u] & inr) == inr);
      }
      ok = in && a.good(skip);
      r = a.acc;
    }
    if (in) out[i] = ok ? r : T(0);
    if (ovalid) {
      store_bits_wave(ovalid, w, n, __ballot(ok), lane);
      if (in && !ok) ++nc;
    }
  }
  if (nulls) wave_add_nulls(nulls, lane, nc);
}

// ---------------------------------------------------------------- replace_with_mask
struct RwmArgs {
  const void* a;          // element offset applied (PDX_BOOL: the bitmap's base, bit offset aoff)
  const uint8_t* avalid;
  int64_t aoff;
  const uint8_t* mask;
  const uint8_t* mvalid;
  int64_t moff;
  const void* repl;       // as a
  const uint8_t* rvalid;
  int64_t roff, rlen;
  void* out;
  uint8_t* ovalid;
  int64_t n;
};
struct RwmHit {  // a valid true mask row
  const uint8_t* mask;
  const uint8_t* mvalid;
  int64_t off;
  __device__ bool operator()(int64_t i) const { return (!mvalid || bit_get(mvalid, off + i)) && bit_get(mask, off + i); }
};
// compact.hpp's tile: a workgroup owns kCompactTile rows, a wave 16 steps of 64; block_offsets[blockIdx.x] = the hits before the tile.
// A hit whose rank is not below rlen (a replacement that is too short: the host fails the call after this launch) reads nothing.
template <typename B, bool BOOL>
__global__ void __launch_bounds__(kCompactBlock) k_replace_with_mask(RwmArgs p, const int64_t* __restrict__ block_offsets, unsigned long long* __restrict__ nulls) {
  __shared__ int wave_tot[4];
  __shared__ unsigned int wave_nulls[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t base = (int64_t)blockIdx.x * kCompactTile + wave * (64 * kCompactItems);
  auto hits_of = [&](int64_t i0, int nb, uint64_t& mv) -> uint64_t {
    mv = (p.mvalid ? load_bits64_uniform(p.mvalid, p.moff + i0, nb) : ~0ull) & in_range_mask(nb);
    return load_bits64_uniform(p.mask, p.moff + i0, nb) & mv;
  };
  int cnt = 0;
  for (int s = 0; s < kCompactItems; ++s) {
    const int64_t i0 = base + s * 64;
    if (i0 >= p.n) break;
    uint64_t mv;
    cnt += __popcll(hits_of(i0, p.n - i0 < 64 ? (int)(p.n - i0) : 64, mv));
  }
  if (lane == 0) wave_tot[wave] = cnt;
  __syncthreads();
  int64_t pos = block_offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos += wave_tot[w];
  const uint64_t lt = (1ull << lane) - 1ull;
  unsigned int nc = 0;
  for (int s = 0; s < kCompactItems; ++s) {
    const int64_t i0 = base + s * 64;
    if (i0 >= p.n) break;
    const int nb = p.n - i0 < 64 ? (int)(p.n - i0) : 64;
    uint64_t mv;
    const uint64_t hit = hits_of(i0, nb, mv);
    const uint64_t keep_ok = (p.avalid ? load_bits64_uniform(p.avalid, p.aoff + i0, nb) : ~0ull) & mv;
    const int64_t i = i0 + lane;
    const bool in = lane < nb, mine = (hit >> lane) & 1ull;
    const int64_t k = pos + __popcll(hit & lt);
    const bool kin = mine && k < p.rlen;
    const bool ok = in && (mine ? (kin && (!p.rvalid || bit_get(p.rvalid, p.roff + k))) : (bool)((keep_ok >> lane) & 1ull));
    if constexpr (BOOL) {
      const uint64_t abits = load_bits64_uniform(static_cast<const uint8_t*>(p.a), p.aoff + i0, nb);
      const bool bit = mine ? (kin && bit_get(static_cast<const uint8_t*>(p.repl), p.roff + k)) : (bool)((abits >> lane) & 1ull);
      store_bits_wave(static_cast<uint8_t*>(p.out), i0 >> 6, p.n, __ballot(ok && bit), lane);
    } else {
      B v = B(0);
      if (ok) v = mine ? static_cast<const B*>(p.repl)[k] : static_cast<const B*>(p.a)[i];
      if (in) static_cast<B*>(p.out)[i] = v;
    }
    if (p.ovalid) store_bits_wave(p.ovalid, i0 >> 6, p.n, __ballot(ok), lane);
    nc += (unsigned int)(nb - __popcll(__ballot(ok)));
    pos += __popcll(hit);
  }
  if (!nulls) return;  // (uniform for the launch)
  if (lane == 0) wave_nulls[wave] = nc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = wave_nulls[0] + wave_nulls[1] + wave_nulls[2] + wave_nulls[3];
    if (t) atomicAdd(nulls, (unsigned long long)t);
  }
}

// ---------------------------------------------------------------- indices_nonzero
template <typename T>
struct NonZero {  // a valid row that is not zero: NaN counts, -0.0 does not
  const T* v;     // element offset applied
  const uint8_t* valid;
  int64_t off;
  __device__ bool operator()(int64_t i) const { return (!valid || bit_get(valid, off + i)) && v[i] != T(0); }
};
struct NonZeroBool {
  const uint8_t* bits;
  const uint8_t* valid;
  int64_t off;
  __device__ bool operator()(int64_t i) const { return (!valid || bit_get(valid, off + i)) && bit_get(bits, off + i); }
};
struct RowIdEmit {
  uint64_t* out;
  __device__ void operator()(int64_t pos, int64_t i) const { out[pos] = (uint64_t)i; }
};

// ---------------------------------------------------------------- all_valid_mask: tab holds the columns that bring a bitmap
__global__ void __launch_bounds__(256) k_all_valid(const ColView* __restrict__ tab, int ncols, int64_t n, uint8_t* __restrict__ out) {
  const int64_t nwords = (n + 63) >> 6, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    const int64_t base = w << 6;
    uint64_t r = in_range_mask(n - base);
    for (int c = 0; c < ncols; ++c) r &= load_bits64(tab[c].valid, tab[c].voff + base, tab[c].voff + n);
    store_bits_word(out, w, n, r);
  }
}

// ---------------------------------------------------------------- host side
static bool mx_known_dtype(int dt) { return dt >= PDX_INT64 && dt <= PDX_FLOAT32; }

template <typename T>
static void mx_launch_minmax(bool clip, const ColView* tab, int nscalar, int C, int64_t n, int is_max, int skip, pdx_mut_column* out, unsigned long long* nulls,
                             hipStream_t st) {
  const dim3 grid(grid_for(n, 256)), block(256);
  T* o = static_cast<T*>(out->values);
  uint8_t* ov = static_cast<uint8_t*>(out->validity);
  if (clip) hipLaunchKernelGGL((k_minmax<T, true>), grid, block, 0, st, tab, nscalar, C, n, is_max, skip, o, ov, nulls);
  else hipLaunchKernelGGL((k_minmax<T, false>), grid, block, 0, st, tab, nscalar, C, n, is_max, skip, o, ov, nulls);
}
// scalars: the operands that are broadcast, in their order; arrays: the others.  clip: arrays = {x}, scalars = {hi, lo}.
static int mx_minmax(const char* who, bool clip, int is_max, const std::vector<const pdx_column*>& scalars, const std::vector<const pdx_column*>& arrays, int64_t n,
                     int skip_nulls, pdx_mut_column* out, void* stream) {
  const int dt = arrays[0]->dtype;
  if (!mx_known_dtype(dt)) return fail(PDX_INVALID, std::string(who) + ": unknown dtype");
  for (const pdx_column* c : scalars)
    if (c->dtype != dt) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": operands are " + dtype_name(dt) + " and " + dtype_name(c->dtype) + " (promote to one type first)");
  for (const pdx_column* c : arrays)
    if (c->dtype != dt) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": operands are " + dtype_name(dt) + " and " + dtype_name(c->dtype) + " (promote to one type first)");
  if (dt == PDX_BOOL) {
    std::string types = "bool";
    for (size_t k = 1; k < (clip ? 2 : scalars.size() + arrays.size()); ++k) types += ", bool";
    return fail(PDX_NOT_IMPLEMENTED, std::string("Function '") + (is_max && !clip ? "max_element_wise" : "min_element_wise") + "' has no kernel matching input types (" + types + ")");
  }
  PDX_TRY(check_out(who, out, dt, n));
  // can a row be null?  skip_nulls: only when every operand can be; otherwise as soon as one can.  (A scalar with a bitmap and
  // null_count != 0 may be null: its bit is on the device.)
  bool any_v = false, all_v = true;
  for (const std::vector<const pdx_column*>* group : {&scalars, &arrays})
    for (const pdx_column* c : *group) {
      if (validity_or_null(c)) any_v = true;
      else all_v = false;
    }
  const bool may_null = skip_nulls ? all_v : any_v;
  if (may_null && !out->validity) return fail(PDX_INVALID, std::string(who) + ": the result can hold nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  std::vector<ColView> host;
  if (clip) {
    host = {col_view(*arrays[0]), col_view(*scalars[0]), col_view(*scalars[1])};
  } else {
    for (const pdx_column* c : scalars) host.push_back(col_view(*c));
    for (const pdx_column* c : arrays) host.push_back(col_view(*c));
  }
  Scratch s;
  const ColView* tab;
  unsigned long long* nulls = nullptr;
  PDX_TRY(upload_views(s, host, st, &tab));
  if (may_null) PDX_TRY(open_null_counter(s, st, &nulls));
  const int ns = clip ? 0 : (int)scalars.size(), C = (int)host.size();
  switch (dt) {
    case PDX_FLOAT64: mx_launch_minmax<double>(clip, tab, ns, C, n, is_max, skip_nulls, out, nulls, st); break;
    case PDX_FLOAT32: mx_launch_minmax<float>(clip, tab, ns, C, n, is_max, skip_nulls, out, nulls, st); break;
    case PDX_UINT64: mx_launch_minmax<uint64_t>(clip, tab, ns, C, n, is_max, skip_nulls, out, nulls, st); break;
    case PDX_INT32: mx_launch_minmax<int32_t>(clip, tab, ns, C, n, is_max, skip_nulls, out, nulls, st); break;
    default: mx_launch_minmax<int64_t>(clip, tab, ns, C, n, is_max, skip_nulls, out, nulls, st); break;
  }
  PDX_LAUNCH_CHECK();
  if (may_null) return read_back(&out->null_count, nulls, sizeof(out->null_count), st);
  return PDX_OK;
}

template <typename Pred>
static int mx_nonzero(const char* who, int64_t n, Pred pred, int64_t* out_count, pdx_mut_column* out, hipStream_t st) {
  Scratch s;
  if (out_count) return count_if(n, pred, out_count, s, st);
  PDX_TRY(check_out(who, out, PDX_UINT64, 0));
  int64_t m = 0;
  const int64_t nblocks = ceil_div(n, kCompactTile);
  int64_t* counts = nullptr;
  if (n > 0) {
    counts = s.get<int64_t>((size_t)nblocks);
    int64_t* total = s.get<int64_t>(1);
    PDX_SCRATCH_CHECK(s);
    hipLaunchKernelGGL((k_compact_count<Pred>), dim3((unsigned)nblocks), dim3(kCompactBlock), 0, st, n, pred, counts);
    PDX_TRY((device_exclusive_scan<int64_t, SumOp>(counts, counts, nblocks, total, s, st)));
    PDX_HIP(hipMemcpyAsync(&m, total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PDX_HIP(hipStreamSynchronize(st));
  }
  if (out->length < m) return fail(PDX_INVALID, std::string(who) + ": output too small (" + std::to_string(m) + " rows are not zero)");
  if (m > 0 && !out->values) return fail(PDX_INVALID, std::string(who) + ": null output buffer");
  if (m > 0) {
    RowIdEmit emit{static_cast<uint64_t*>(out->values)};
    hipLaunchKernelGGL((k_compact_write<Pred, RowIdEmit>), dim3((unsigned)nblocks), dim3(kCompactBlock), 0, st, n, pred, emit, counts);
    PDX_LAUNCH_CHECK();
  }
  out->length = m;
  out->null_count = 0;
  return PDX_OK;
}
static int mx_nonzero_any(const char* who, const pdx_column* a, int64_t* out_count, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_column(a, who, true));
  if (!out_count && !out) return fail(PDX_INVALID, std::string(who) + ": null output");
  if (!mx_known_dtype(a->dtype)) return fail(PDX_INVALID, std::string(who) + ": unknown dtype");
  if (a->dtype == PDX_TIMESTAMP_NS) return fail(PDX_NOT_IMPLEMENTED, "Function 'indices_nonzero' has no kernel matching input types (timestamp[ns])");
  hipStream_t st = as_stream(stream);
  const uint8_t* v = validity_or_null(a);
  const int64_t n = a->length;
  switch (a->dtype) {
    case PDX_BOOL: return mx_nonzero(who, n, NonZeroBool{static_cast<const uint8_t*>(a->values), v, a->offset}, out_count, out, st);
    case PDX_FLOAT64: return mx_nonzero(who, n, NonZero<double>{static_cast<const double*>(a->values) + a->offset, v, a->offset}, out_count, out, st);
    case PDX_FLOAT32: return mx_nonzero(who, n, NonZero<float>{static_cast<const float*>(a->values) + a->offset, v, a->offset}, out_count, out, st);
    case PDX_INT32: return mx_nonzero(who, n, NonZero<int32_t>{static_cast<const int32_t*>(a->values) + a->offset, v, a->offset}, out_count, out, st);
    default: return mx_nonzero(who, n, NonZero<int64_t>{static_cast<const int64_t*>(a->values) + a->offset, v, a->offset}, out_count, out, st);
  }
}

}  // namespace pdx

using namespace pdx;

extern "C" {

int pdx_coalesce(const pdx_column* cols, int ncols, pdx_mut_column* out, void* stream) {
  const char* who = "pdx_coalesce";
  if (!cols || ncols <= 0) return fail(PDX_INVALID, "pdx_coalesce: at least one column is required");
  if (ncols > kMxMaxCols) return fail(PDX_INVALID, "pdx_coalesce: more than " + std::to_string(kMxMaxCols) + " columns");
  for (int c = 0; c < ncols; ++c) PDX_TRY(check_column(&cols[c], who, true));
  const int dt = cols[0].dtype;
  const int64_t n = cols[0].length;
  if (!mx_known_dtype(dt)) return fail(PDX_INVALID, "pdx_coalesce: unknown dtype");
  for (int c = 1; c < ncols; ++c) {
    if (cols[c].dtype != dt)
      return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": column " + std::to_string(c) + " is " + dtype_name(cols[c].dtype) + ", column 0 " + dtype_name(dt) +
                                           " (cast to one type first)");
    if (cols[c].length != n) return fail(PDX_INVALID, std::string(who) + ": Array arguments must all be the same length");
  }
  PDX_TRY(check_out(who, out, dt, n));
  const bool may_null = validity_or_null(&cols[0]) != nullptr;
  if (may_null && !out->validity) return fail(PDX_INVALID, std::string(who) + ": the result can hold nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  // the columns behind the first one without a bitmap never give a value
  std::vector<ColView> host;
  bool vec = is_narrow(dt) && aligned16(out->values);
  for (int c = 0; c < ncols; ++c) {
    host.push_back(col_view(cols[c]));
    vec = vec && aligned16(host.back().values);
    if (!host.back().valid) break;
  }
  const bool count = host.back().valid != nullptr;  // (a column without a bitmap leaves no row null)
  Scratch s;
  const ColView* tab;
  unsigned long long* nulls = nullptr;
  PDX_TRY(upload_views(s, host, st, &tab));
  if (count) PDX_TRY(open_null_counter(s, st, &nulls));
  const int C = (int)host.size();
  uint8_t* ov = static_cast<uint8_t*>(out->validity);
  if (dt == PDX_BOOL) {
    hipLaunchKernelGGL(k_coalesce_bool, dim3(grid_for((n + 63) >> 6, 256)), dim3(256), 0, st, tab, C, n, static_cast<uint8_t*>(out->values), ov, nulls);
  } else if (is_narrow(dt)) {
    if (vec) hipLaunchKernelGGL((k_coalesce<uint32_t, 4>), dim3(grid_for(ceil_div(n, 256) * 64, 256)), dim3(256), 0, st, tab, C, n, static_cast<uint32_t*>(out->values), ov, nulls);
    else hipLaunchKernelGGL((k_coalesce<uint32_t, 1>), dim3(grid_for(n, 256)), dim3(256), 0, st, tab, C, n, static_cast<uint32_t*>(out->values), ov, nulls);
  } else {
    hipLaunchKernelGGL((k_coalesce<uint64_t, 1>), dim3(grid_for(n, 256)), dim3(256), 0, st, tab, C, n, static_cast<uint64_t*>(out->values), ov, nulls);
  }
  PDX_LAUNCH_CHECK();
  if (count) return read_back(&out->null_count, nulls, sizeof(out->null_count), st);
  return PDX_OK;
}

int pdx_element_wise_minmax(int is_max, const pdx_column* cols, int ncols, int skip_nulls, pdx_mut_column* out, void* stream) {
  const char* who = "pdx_element_wise_minmax";
  if (!cols || ncols <= 0) return fail(PDX_INVALID, "pdx_element_wise_minmax: at least one operand is required");
  if (ncols > kMxMaxCols) return fail(PDX_INVALID, "pdx_element_wise_minmax: more than " + std::to_string(kMxMaxCols) + " operands");
  int64_t n = 0;
  for (int c = 0; c < ncols; ++c) {
    PDX_TRY(check_column(&cols[c], who, true));
    n = std::max(n, cols[c].length);
  }
  std::vector<const pdx_column*> scalars, arrays;
  for (int c = 0; c < ncols; ++c) {
    if (cols[c].length == n) arrays.push_back(&cols[c]);
    else if (cols[c].length == 1) scalars.push_back(&cols[c]);
    else return fail(PDX_INVALID, std::string(who) + ": Array arguments must all be the same length");
  }
  return mx_minmax(who, false, is_max != 0, scalars, arrays, n, skip_nulls != 0, out, stream);
}

int pdx_clip(const pdx_column* x, const pdx_column* lo, const pdx_column* hi, int skip_nulls, pdx_mut_column* out, void* stream) {
  const char* who = "pdx_clip";
  PDX_TRY(check_column(x, who, true));
  PDX_TRY(check_column(lo, who, true));
  PDX_TRY(check_column(hi, who, true));
  if (lo->length != 1 || hi->length != 1) return fail(PDX_INVALID, "pdx_clip: lo and hi are columns of length 1 (scalars)");
  return mx_minmax(who, true, 0, {hi, lo}, {x}, x->length, skip_nulls != 0, out, stream);
}

int pdx_replace_with_mask(const pdx_column* a, const pdx_column* mask, const pdx_column* repl, pdx_mut_column* out, void* stream) {
  const char* who = "pdx_replace_with_mask";
  PDX_TRY(check_column(a, who, true));
  PDX_TRY(check_column(mask, who, true));
  PDX_TRY(check_column(repl, who, true));
  if (!mx_known_dtype(a->dtype)) return fail(PDX_INVALID, "pdx_replace_with_mask: unknown dtype");
  if (mask->dtype != PDX_BOOL)
    return fail(PDX_INVALID, std::string("Function 'replace_with_mask' has no kernel matching input types (") + arrow_dtype_name(a->dtype) + ", " + arrow_dtype_name(mask->dtype) +
                                 ", " + arrow_dtype_name(repl->dtype) + ")");
  if (repl->dtype != a->dtype)
    return fail(PDX_INVALID, std::string("Function 'replace_with_mask' has no kernel matching input types (") + arrow_dtype_name(a->dtype) + ", bool, " +
                                 arrow_dtype_name(repl->dtype) + ")");
  const int64_t n = a->length;
  if (mask->length != n)
    return fail(PDX_INVALID, "Mask must be of same length as array (expected " + std::to_string(n) + " items but got " + std::to_string(mask->length) + " items)");
  PDX_TRY(check_out(who, out, a->dtype, n));
  const bool may_null = validity_or_null(a) || validity_or_null(mask) || validity_or_null(repl);
  if (may_null && !out->validity) return fail(PDX_INVALID, std::string(who) + ": the result can hold nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    out->length = 0;
    out->null_count = 0;
    return PDX_OK;
  }
  const int dt = a->dtype;
  const size_t w = (size_t)dtype_bytes(dt);
  RwmArgs p;
  p.a = dt == PDX_BOOL ? a->values : static_cast<const void*>(static_cast<const char*>(a->values) + (size_t)a->offset * w);
  p.avalid = validity_or_null(a);
  p.aoff = a->offset;
  p.mask = static_cast<const uint8_t*>(mask->values);
  p.mvalid = validity_or_null(mask);
  p.moff = mask->offset;
  p.repl = dt == PDX_BOOL || !repl->values ? repl->values : static_cast<const void*>(static_cast<const char*>(repl->values) + (size_t)repl->offset * w);
  p.rvalid = validity_or_null(repl);
  p.roff = repl->offset;
  p.rlen = repl->length;
  p.out = out->values;
  p.ovalid = static_cast<uint8_t*>(out->validity);
  p.n = n;
  Scratch s;
  const int64_t nblocks = ceil_div(n, kCompactTile);
  int64_t* counts = s.get<int64_t>((size_t)nblocks);
  int64_t* total = s.get<int64_t>(1);
  unsigned long long* nulls = may_null ? s.get<unsigned long long>(1) : nullptr;
  PDX_SCRATCH_CHECK(s);
  if (nulls) PDX_HIP(hipMemsetAsync(nulls, 0, sizeof(unsigned long long), st));
  RwmHit pred{p.mask, p.mvalid, p.moff};
  hipLaunchKernelGGL((k_compact_count<RwmHit>), dim3((unsigned)nblocks), dim3(kCompactBlock), 0, st, n, pred, counts);
  PDX_TRY((device_exclusive_scan<int64_t, SumOp>(counts, counts, nblocks, total, s, st)));
  const dim3 grid((unsigned)nblocks), block(kCompactBlock);
  if (dt == PDX_BOOL) hipLaunchKernelGGL((k_replace_with_mask<uint32_t, true>), grid, block, 0, st, p, counts, nulls);
  else if (w == 4) hipLaunchKernelGGL((k_replace_with_mask<uint32_t, false>), grid, block, 0, st, p, counts, nulls);
  else hipLaunchKernelGGL((k_replace_with_mask<uint64_t, false>), grid, block, 0, st, p, counts, nulls);
  PDX_LAUNCH_CHECK();
  // the one host wait: the number of valid true mask rows (the length check) and, with it, the null count
  int64_t need = 0;
  unsigned long long hn = 0;
  PDX_HIP(hipMemcpyAsync(&need, total, sizeof(need), hipMemcpyDeviceToHost, st));
  if (nulls) PDX_HIP(hipMemcpyAsync(&hn, nulls, sizeof(hn), hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));
  if (repl->length < need)
    return fail(PDX_INVALID, "Replacement array must be of appropriate length (expected " + std::to_string(need) + " items but got " + std::to_string(repl->length) +
                                 " items)");
  out->length = n;
  out->null_count = (int64_t)hn;
  return PDX_OK;
}

int pdx_indices_nonzero_count(const pdx_column* a, int64_t* out_count, void* stream) {
  if (!out_count) return fail(PDX_INVALID, "pdx_indices_nonzero_count: null output");
  return mx_nonzero_any("pdx_indices_nonzero_count", a, out_count, nullptr, stream);
}

int pdx_indices_nonzero(const pdx_column* a, pdx_mut_column* out, void* stream) {
  if (!out) return fail(PDX_INVALID, "pdx_indices_nonzero: null output");
  return mx_nonzero_any("pdx_indices_nonzero", a, nullptr, out, stream);
}

int pdx_all_valid_mask(const pdx_column* cols, int ncols, pdx_mut_column* out_mask, void* stream) {
  const char* who = "pdx_all_valid_mask";
  if (!cols || ncols <= 0) return fail(PDX_INVALID, "pdx_all_valid_mask: at least one column is required");
  if (ncols > kMxMaxCols) return fail(PDX_INVALID, "pdx_all_valid_mask: more than " + std::to_string(kMxMaxCols) + " columns");
  const int64_t n = cols[0].length;
  std::vector<ColView> host;
  for (int c = 0; c < ncols; ++c) {
    PDX_TRY(check_column(&cols[c], who, true));
    if (cols[c].length != n) return fail(PDX_INVALID, std::string(who) + ": all columns must have the same length");
    if (validity_or_null(&cols[c])) host.push_back(col_view(cols[c]));
  }
  PDX_TRY(check_out(who, out_mask, PDX_BOOL, n));
  hipStream_t st = as_stream(stream);
  out_mask->length = n;
  out_mask->null_count = 0;
  if (n == 0) return PDX_OK;
  Scratch s;
  const ColView* tab;
  PDX_TRY(upload_views(s, host, st, &tab));
  hipLaunchKernelGGL(k_all_valid, dim3(grid_for((n + 63) >> 6, 256)), dim3(256), 0, st, tab, (int)host.size(), n, static_cast<uint8_t*>(out_mask->values));
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

}  // extern "C"
