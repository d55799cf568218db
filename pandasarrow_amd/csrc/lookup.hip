// lookup.hip -- "where is this value" and "is this value one of those" for gfx950: pdx_is_in / pdx_index_in (Arrow's is_in / index_in under
// SetLookupOptions{value_set, skip_nulls}; reference src/series.cpp:632-640), pdx_index (Arrow's index; src/ndframe.h:276-282),
// pdx_arg_extreme (index(min()) / index(max()): NDFrame::argmin / argmax, Series / DataFrame::idxMin / idxMax, src/series.cpp:164-172,
// src/dataframe.cpp:496-512) and pdx_dictionary_encode (src/series.cpp:341).
//
// Set lookup.  Values are matched by their bit image (uint64 / uint32): 0.0 and -0.0, and NaNs of different sign or payload, are different
// values, as in Arrow's memo table.  Build: the value set goes into an open-addressing table (linear probing, splitmix64 of the bit image)
// of slots = the power of two >= 2 * set size, so the load factor stays <= 0.5; a slot holds the FIRST position of its value in the set
// (atomicCAS claims a slot, atomicMin lowers the position of a duplicate), null entries stay out and the first of them is remembered.
// Probe, two plans behind one kernel template:
//   lds     set size <= kLkLdsMaxEntries (PDX_LOOKUP_LDS_MAX lowers it): every workgroup copies keys + positions into LDS (12 B a slot, at
//           most 4096 slots = 48 KB: three workgroups stay resident on a CU's 160 KB), then streams its rows
//   global  larger sets: the same loop over the table where it was built (L2 / Infinity Cache resident up to some 1e7 entries)
// A wave takes tiles of 64 * VEC rows; with VEC = 2 every lane loads its two neighbouring rows in one 16-byte (8-byte for the 4-byte dtypes)
// load, and the two ballots are interleaved bit by bit -- on the scalar unit -- into the two 64-row words of the packed output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "colview.hpp"
#include "lookup_table.hpp"

namespace pdx {

// (the table itself -- constants, k_lk_insert, k_lk_keys, k_lk_widen -- lives in lookup_table.hpp, shared with join.hip)
static thread_local std::string g_lookup_plan = "plan=empty set_size=0 slots=0";

template <typename U>
struct LkVec2 {
  typedef U type __attribute__((ext_vector_type(2)));
};

// the two rows i, i + 1 of a lane (i even): one vector load where the pointer allows it and both rows exist
template <typename U>
__device__ __forceinline__ void lk_load2(const U* __restrict__ p, int64_t i, int64_t n, bool vec, U* x0, U* x1) {
  if (vec && i + 1 < n) {
    const typename LkVec2<U>::type v = *reinterpret_cast<const typename LkVec2<U>::type*>(p + i);
    *x0 = v.x;
    *x1 = v.y;
  } else {
    *x0 = i < n ? p[i] : U(0);
    *x1 = i + 1 < n ? p[i + 1] : U(0);
  }
}
// the validity of the 64 rows from row i0 + 64 * w of a tile (bits of rows >= n are clear); all operands wave-uniform
__device__ __forceinline__ uint64_t lk_valid_word(const uint8_t* valid, int64_t voff, int64_t i0, int64_t n, int w) {
  const int64_t rem = n - i0 - 64 * (int64_t)w;
  if (rem <= 0) return 0ull;
  const uint64_t in = in_range_mask(rem);
  return valid ? (load_bits64_uniform(valid, voff + i0 + 64 * (int64_t)w, (int)(rem < 64 ? rem : 64)) & in) : in;
}

// ---------------------------------------------------------------- probe
struct LkProbe {
  const void* vals;          // element offset applied
  const uint8_t* valid;      // nullptr: every row is valid
  int64_t voff, n;
  const void* keys;          // [mask + 1]
  const uint32_t* pos;       // [mask + 1]
  uint32_t mask;
  int match_null;            // a null row takes the position of the set's first null (skip_nulls == 0)
  const uint32_t* first_null;
  uint8_t* out_bits;         // is_in: the packed values; index_in: the validity
  int32_t* out_idx;          // index_in only
  unsigned long long* nulls; // index_in only
  int vec;                   // VEC == 2: the lanes' pairs may be loaded (and the index pairs stored) as one vector
};

extern __shared__ __attribute__((aligned(16))) unsigned char lk_smem[];

template <typename U, int VEC, bool LDS, bool INDEX>
__global__ void __launch_bounds__(kLkBlock) k_lk_probe(const LkProbe a) {
  const U* __restrict__ gkeys = static_cast<const U*>(a.keys);
  const uint32_t* __restrict__ gpos = a.pos;
  const uint32_t mask = a.mask;
  U* skeys = reinterpret_cast<U*>(lk_smem);
  uint32_t* spos = reinterpret_cast<uint32_t*>(lk_smem + ((size_t)mask + 1) * sizeof(U));
  if constexpr (LDS) {
    for (uint32_t h = threadIdx.x; h <= mask; h += kLkBlock) {
      skeys[h] = gkeys[h];
      spos[h] = gpos[h];
    }
    __syncthreads();
  }
  // the position of k in the set, -1 when it is not there; at most mask + 1 steps whatever the table holds
  auto probe = [&](U k) -> int32_t {
    uint32_t h = (uint32_t)splitmix64((uint64_t)k) & mask;
    for (uint64_t step = 0; step <= (uint64_t)mask; ++step) {
      uint32_t p;
      U key;
      if constexpr (LDS) {
        p = spos[h];
        key = skeys[h];
      } else {
        p = gpos[h];
        key = gkeys[h];
      }
      if (p == kLkEmpty) return -1;
      if (key == k) return (int32_t)p;
      h = (h + 1) & mask;
    }
    return -1;
  };
  const U* __restrict__ v = static_cast<const U*>(a.vals);
  const int64_t n = a.n;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int32_t null_pos = -1;
  if (a.match_null) {
    const uint32_t fn = *a.first_null;
    null_pos = fn == kLkEmpty ? -1 : (int32_t)fn;
  }
  constexpr int ROWS = 64 * VEC;
  const int64_t tiles = (n + ROWS - 1) / ROWS;
  const int64_t stride = (int64_t)gridDim.x * kLkWaves;
  unsigned long long nc = 0;
  for (int64_t t = (int64_t)blockIdx.x * kLkWaves + wave; t < tiles; t += stride) {  // (t is the same in all lanes: whole waves reach the ballots)
    const int64_t i0 = t * ROWS;
    uint64_t vb[VEC];
#pragma unroll
    for (int w = 0; w < VEC; ++w) vb[w] = lk_valid_word(a.valid, a.voff, i0, n, w);
    const int64_t i = i0 + (int64_t)lane * VEC;
    U x[VEC];
    if constexpr (VEC == 2) lk_load2<U>(v, i, n, a.vec != 0, &x[0], &x[1]);
    else x[0] = i < n ? v[i] : U(0);
    int32_t p[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int r = lane * VEC + e;  // the row inside the tile
      const bool ok = (vb[r >> 6] >> (r & 63)) & 1ull;
      p[e] = ok ? probe(x[e]) : (i + e < n ? null_pos : -1);
      if (i + e < n && p[e] < 0) ++nc;
    }
    if constexpr (VEC == 1) {
      const uint64_t word = __ballot(p[0] >= 0);
      store_bits_wave(a.out_bits, t, n, word, lane);
      if constexpr (INDEX) {
        if (i < n) a.out_idx[i] = p[0] < 0 ? 0 : p[0];
      }
    } else {
      const uint64_t b0 = __ballot(p[0] >= 0), b1 = __ballot(p[1] >= 0);
      store_bits_wave(a.out_bits, 2 * t, n, lk_spread(b0) | (lk_spread(b1) << 1), lane);
      store_bits_wave(a.out_bits, 2 * t + 1, n, lk_spread(b0 >> 32) | (lk_spread(b1 >> 32) << 1), lane);
      if constexpr (INDEX) {
        const int32_t o0 = p[0] < 0 ? 0 : p[0], o1 = p[1] < 0 ? 0 : p[1];
        if (a.vec && i + 1 < n) {
          typename LkVec2<int32_t>::type o;
          o.x = o0;
          o.y = o1;
          *reinterpret_cast<typename LkVec2<int32_t>::type*>(a.out_idx + i) = o;
        } else {
          if (i < n) a.out_idx[i] = o0;
          if (i + 1 < n) a.out_idx[i + 1] = o1;
        }
      }
    }
  }
  if constexpr (INDEX) wave_add_nulls(a.nulls, lane, nc);
}

// ---------------------------------------------------------------- index: the first row == value
template <typename T>
__global__ void __launch_bounds__(kLkBlock) k_lk_index(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, int64_t n, T value,
                                                       unsigned long long* __restrict__ best /* ~0: none yet */) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t tiles = (n + 63) >> 6, stride = (int64_t)gridDim.x * kLkWaves;
  for (int64_t t = (int64_t)blockIdx.x * kLkWaves + wave; t < tiles; t += stride) {
    const int64_t i0 = t << 6;
    // a match before this tile is already known: the wave's later tiles lie behind it too (a stale read costs one tile, never a result)
    // (lane 0 reads, the wave shares its value: all lanes leave together, the ballot below always sees a whole wave)
    unsigned long long seen = 0;
    if (lane == 0) seen = __atomic_load_n(best, __ATOMIC_RELAXED);
    const uint32_t seen_lo = __builtin_amdgcn_readfirstlane((uint32_t)seen), seen_hi = __builtin_amdgcn_readfirstlane((uint32_t)(seen >> 32));
    if ((unsigned long long)i0 >= (((unsigned long long)seen_hi << 32) | seen_lo)) break;
    const uint64_t vb = lk_valid_word(valid, voff, i0, n, 0);
    const bool hit = ((vb >> lane) & 1ull) ? v[i0 + lane] == value : false;
    const unsigned long long m = __ballot(hit);
    if (m) {
      if (lane == 0) atomicMin(best, (unsigned long long)(i0 + __ffsll((long long)m) - 1));
      break;
    }
  }
}

// ---------------------------------------------------------------- arg_extreme: index(min()) / index(max()) of every column, one read
struct AxCol {
  const void* values;  // element offset applied
  const uint8_t* valid;
  int64_t voff, n;
  int32_t dtype, vec;
};
struct AxPair {  // the smaller pair wins: key first (the value in an order-preserving unsigned image, inverted for max), then the row
  unsigned long long key;
  long long row;
};
constexpr long long kAxNoRow = 0x7FFFFFFFFFFFFFFFll;
__device__ __forceinline__ bool ax_less(const AxPair& x, const AxPair& y) { return x.key < y.key || (x.key == y.key && x.row < y.row); }

// the order-preserving image of a value; false: the value takes no part (NaN).  The two zeros share one image: they tie, the first row wins.
template <typename T>
__device__ __forceinline__ bool ax_key(T x, unsigned long long* key);
template <> __device__ __forceinline__ bool ax_key<int64_t>(int64_t x, unsigned long long* key) {
  *key = (unsigned long long)x ^ 0x8000000000000000ull;
  return true;
}
template <> __device__ __forceinline__ bool ax_key<uint64_t>(uint64_t x, unsigned long long* key) {
  *key = x;
  return true;
}
template <> __device__ __forceinline__ bool ax_key<int32_t>(int32_t x, unsigned long long* key) { return ax_key<int64_t>((int64_t)x, key); }
template <> __device__ __forceinline__ bool ax_key<double>(double x, unsigned long long* key) {
  if (x != x) return false;
  if (x == 0.0) x = 0.0;
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  *key = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return true;
}
template <> __device__ __forceinline__ bool ax_key<float>(float x, unsigned long long* key) { return ax_key<double>((double)x, key); }  // (exact)

template <typename T>
__device__ __forceinline__ AxPair ax_scan(const AxCol& c, int is_max, int lane, int wave) {
  const T* __restrict__ v = static_cast<const T*>(c.values);
  const int64_t n = c.n, tiles = (n + 127) >> 7, stride = (int64_t)gridDim.x * kLkWaves;
  AxPair best{~0ull, kAxNoRow};
  for (int64_t t = (int64_t)blockIdx.x * kLkWaves + wave; t < tiles; t += stride) {
    const int64_t i0 = t << 7, i = i0 + 2 * lane;
    const uint64_t vb0 = lk_valid_word(c.valid, c.voff, i0, n, 0), vb1 = lk_valid_word(c.valid, c.voff, i0, n, 1);
    T x[2];
    lk_load2<T>(v, i, n, c.vec != 0, &x[0], &x[1]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = 2 * lane + e;
      const bool ok = ((r < 64 ? vb0 : vb1) >> (r & 63)) & 1ull;
      unsigned long long k;
      if (ok && ax_key<T>(x[e], &k)) {
        if (is_max) k = ~k;
        if (k < best.key || best.row == kAxNoRow) best = AxPair{k, (long long)(i + e)};  // (a lane's rows ascend: the first of equals stays)
      }
    }
  }
  return best;
}

__global__ void __launch_bounds__(kLkBlock) k_ax_partial(const AxCol* __restrict__ cols, int is_max, AxPair* __restrict__ part /* [ncols][gridDim.x] */) {
  __shared__ AxPair ws[kLkWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const AxCol c = cols[blockIdx.y];
  AxPair best;
  switch (c.dtype) {  // (the same in the whole workgroup)
    case PDX_FLOAT64: best = ax_scan<double>(c, is_max, lane, wave); break;
    case PDX_UINT64: best = ax_scan<uint64_t>(c, is_max, lane, wave); break;
    case PDX_INT32: best = ax_scan<int32_t>(c, is_max, lane, wave); break;
    case PDX_FLOAT32: best = ax_scan<float>(c, is_max, lane, wave); break;
    default: best = ax_scan<int64_t>(c, is_max, lane, wave); break;  // int64, timestamp[ns]
  }
  for (int d = 32; d > 0; d >>= 1) {
    AxPair o;
    o.key = __shfl_down(best.key, d, 64);
    o.row = __shfl_down(best.row, d, 64);
    if (ax_less(o, best)) best = o;
  }
  if (lane == 0) ws[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kLkWaves; ++w)
      if (ax_less(ws[w], best)) best = ws[w];
    part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = best;
  }
}
__global__ void __launch_bounds__(64) k_ax_final(const AxPair* __restrict__ part, int nparts, long long* __restrict__ out_rows) {
  const int lane = threadIdx.x;
  AxPair best{~0ull, kAxNoRow};
  for (int j = lane; j < nparts; j += 64) {
    const AxPair o = part[(size_t)blockIdx.x * nparts + j];
    if (ax_less(o, best)) best = o;
  }
  for (int d = 32; d > 0; d >>= 1) {
    AxPair o;
    o.key = __shfl_down(best.key, d, 64);
    o.row = __shfl_down(best.row, d, 64);
    if (ax_less(o, best)) best = o;
  }
  if (lane == 0) out_rows[blockIdx.x] = best.row == kAxNoRow ? -1ll : best.row;
}

// ---------------------------------------------------------------- dictionary_encode (over the group-by handle)
// ctl[1] = the id of the null key's group (it stays ~0 without one)
__global__ void k_lk_null_group(const uint8_t* __restrict__ uvalid, int64_t G, unsigned long long* __restrict__ ctl) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += stride)
    if (!bit_get(uvalid, g)) ctl[1] = (unsigned long long)g;
}
// codes: the group ids with the null group taken out of the numbering; a row of the null group is null.  ctl[0] counts them.
__global__ void __launch_bounds__(kLkBlock) k_lk_codes(const uint32_t* __restrict__ ids, int64_t n, unsigned long long* __restrict__ ctl, int32_t* __restrict__ codes,
                                                       uint8_t* __restrict__ out_valid /* may be nullptr */) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned long long gnull = ctl[1];
  const int64_t tiles = (n + 63) >> 6, stride = (int64_t)gridDim.x * kLkWaves;
  unsigned long long nc = 0;
  for (int64_t t = (int64_t)blockIdx.x * kLkWaves + wave; t < tiles; t += stride) {
    const int64_t i = (t << 6) + lane;
    bool ok = false;
    if (i < n) {
      const unsigned long long g = ids[i];
      ok = g != gnull;
      codes[i] = ok ? (int32_t)(g - (g > gnull ? 1 : 0)) : 0;
      if (!ok) ++nc;
    }
    const uint64_t word = __ballot(ok);
    if (out_valid) store_bits_wave(out_valid, t, n, word, lane);
  }
  wave_add_nulls(&ctl[0], lane, nc);
}
template <typename U>
__global__ void k_lk_dict(const unsigned long long* __restrict__ uniq, int64_t G, const unsigned long long* __restrict__ ctl, U* __restrict__ dict) {
  const unsigned long long gnull = ctl[1];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += stride)
    if ((unsigned long long)g != gnull) dict[g - ((unsigned long long)g > gnull ? 1 : 0)] = (U)uniq[g];
}

// ---------------------------------------------------------------- host
static bool lookup_dtype(int dt) { return is_int_like(dt) || dt == PDX_FLOAT64 || is_narrow(dt); }

template <typename U, bool INDEX>
static int lookup_launch(bool lds, int vec2, size_t shmem, int grid, hipStream_t st, const LkProbe& args) {
  if (lds) {
    if (vec2) hipLaunchKernelGGL((k_lk_probe<U, 2, true, INDEX>), dim3(grid), dim3(kLkBlock), shmem, st, args);
    else hipLaunchKernelGGL((k_lk_probe<U, 1, true, INDEX>), dim3(grid), dim3(kLkBlock), shmem, st, args);
  } else {
    if (vec2) hipLaunchKernelGGL((k_lk_probe<U, 2, false, INDEX>), dim3(grid), dim3(kLkBlock), 0, st, args);
    else hipLaunchKernelGGL((k_lk_probe<U, 1, false, INDEX>), dim3(grid), dim3(kLkBlock), 0, st, args);
  }
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

template <typename U, bool INDEX>
static int lookup_typed(const pdx_column* a, const pdx_column* vs, int skip_nulls, pdx_mut_column* out, hipStream_t st) {
  const int64_t n = a->length, m = vs->length;
  uint64_t slots = 2;
  while (slots < 2 * (uint64_t)m) slots <<= 1;
  const bool lds = m <= lookup_lds_max();
  g_lookup_plan = std::string("plan=") + (m == 0 ? "empty" : lds ? "lds" : "global") + " set_size=" + std::to_string(m) + " slots=" + std::to_string(slots);
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  Scratch s;
  PDX_PROFILE(INDEX ? "index_in" : "is_in", st);
  uint32_t* pos = s.get<uint32_t>((size_t)slots + 1);  // [slots] = the position of the set's first null
  U* keys = s.get<U>((size_t)slots);
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemsetAsync(pos, 0xFF, sizeof(uint32_t) * ((size_t)slots + 1), st));
  const uint32_t mask = (uint32_t)(slots - 1);
  const U* set = static_cast<const U*>(vs->values) + vs->offset;
  if (m > 0) hipLaunchKernelGGL(k_lk_insert<U>, dim3(grid_for(m, 256, 4)), dim3(256), 0, st, set, validity_or_null(vs), vs->offset, m, pos, mask, pos + slots);
  hipLaunchKernelGGL(k_lk_keys<U>, dim3(grid_for((int64_t)slots, 256, 4)), dim3(256), 0, st, set, pos, slots, keys);
  PDX_LAUNCH_CHECK();
  LkProbe args{};
  args.vals = static_cast<const U*>(a->values) + a->offset;
  args.valid = validity_or_null(a);
  args.voff = a->offset;
  args.n = n;
  args.keys = keys;
  args.pos = pos;
  args.mask = mask;
  args.match_null = skip_nulls ? 0 : 1;
  args.first_null = pos + slots;
  args.out_bits = static_cast<uint8_t*>(INDEX ? out->validity : out->values);
  args.out_idx = INDEX ? static_cast<int32_t*>(out->values) : nullptr;
  args.nulls = nullptr;
  if (INDEX) PDX_TRY(open_null_counter(s, st, &args.nulls));
  const uintptr_t pv = reinterpret_cast<uintptr_t>(args.vals);
  args.vec = (pv % (2 * sizeof(U)) == 0) && (!INDEX || reinterpret_cast<uintptr_t>(args.out_idx) % 8 == 0);
  const size_t shmem = lds ? (size_t)slots * (sizeof(U) + sizeof(uint32_t)) : 0;
  // lds: as many workgroups as stay resident (each one copies the table once), every wave strides over the tiles
  const int resident = lds ? (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) / std::max<size_t>(shmem, 1))) : 8;
  const int grid = grid_for(n, kLkBlock, args.vec ? 2 : 1, kCUs * resident);
  PDX_TRY((lookup_launch<U, INDEX>(lds, args.vec, shmem, grid, st, args)));
  if (INDEX) {
    unsigned long long hn = 0;
    PDX_TRY(read_back(&hn, args.nulls, sizeof(hn), st));
    out->null_count = (int64_t)hn;
  }
  return PDX_OK;
}

template <bool INDEX>
static int lookup_entry(const char* who, const pdx_column* a, const pdx_column* vs, int skip_nulls, pdx_mut_column* out, void* stream) {
  if (!a || !vs) return fail(PDX_INVALID, std::string(who) + ": null column");
  if (a->dtype == PDX_BOOL || vs->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": dtype bool is not supported");
  if (!lookup_dtype(a->dtype) || !lookup_dtype(vs->dtype)) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": unsupported dtype");
  PDX_TRY(check_column(a, who, true));
  PDX_TRY(check_column(vs, who, true));
  if (a->dtype != vs->dtype)
    return fail(PDX_INVALID, std::string(who) + ": the value set is " + dtype_name(vs->dtype) + ", the input " + dtype_name(a->dtype) + " (cast the set first)");
  if (vs->length > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": more than 2^31-1 entries in the value set are not supported");
  PDX_TRY(check_out(who, out, INDEX ? PDX_INT32 : PDX_BOOL, a->length));
  if (INDEX && a->length > 0 && !out->validity) return fail(PDX_INVALID, std::string(who) + ": the output needs a validity buffer (a row without a match is null)");
  hipStream_t st = as_stream(stream);
  return is_narrow(a->dtype) ? lookup_typed<uint32_t, INDEX>(a, vs, skip_nulls, out, st) : lookup_typed<uint64_t, INDEX>(a, vs, skip_nulls, out, st);
}

template <typename T>
static int index_typed(const pdx_column* a, T value, int64_t* out_row, hipStream_t st) {
  Scratch s;
  PDX_PROFILE("index", st);
  unsigned long long* best = s.get<unsigned long long>(1);
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemsetAsync(best, 0xFF, sizeof(*best), st));
  hipLaunchKernelGGL(k_lk_index<T>, dim3(grid_for(a->length, kLkBlock, 1)), dim3(kLkBlock), 0, st, static_cast<const T*>(a->values) + a->offset, validity_or_null(a),
                     a->offset, a->length, value, best);
  PDX_LAUNCH_CHECK();
  unsigned long long h = 0;
  PDX_TRY(read_back(&h, best, sizeof(h), st));
  *out_row = h == ~0ull ? -1 : (int64_t)h;
  return PDX_OK;
}

}  // namespace pdx

using namespace pdx;

extern "C" int pdx_is_in(const pdx_column* a, const pdx_column* value_set, int skip_nulls, pdx_mut_column* out, void* stream) {
  return lookup_entry<false>("pdx_is_in", a, value_set, skip_nulls, out, stream);
}

extern "C" int pdx_index_in(const pdx_column* a, const pdx_column* value_set, int skip_nulls, pdx_mut_column* out, void* stream) {
  return lookup_entry<true>("pdx_index_in", a, value_set, skip_nulls, out, stream);
}

extern "C" int pdx_lookup_last_plan(char* buf, size_t buf_len) {
  if (!buf || !buf_len) return fail(PDX_INVALID, "pdx_lookup_last_plan: null buffer");
  snprintf(buf, buf_len, "%s", g_lookup_plan.c_str());
  return PDX_OK;
}

extern "C" int pdx_index(const pdx_column* a, const pdx_scalar* value, int64_t* out_row, void* stream) {
  if (!a || !out_row) return fail(PDX_INVALID, "pdx_index: null argument");
  if (a->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, "pdx_index: dtype bool is not supported");
  if (!lookup_dtype(a->dtype)) return fail(PDX_NOT_IMPLEMENTED, "pdx_index: unsupported dtype");
  PDX_TRY(check_column(a, "pdx_index", true));
  if (value && value->dtype != a->dtype)
    return fail(PDX_INVALID, std::string("pdx_index: the value is ") + dtype_name(value->dtype) + ", the column " + dtype_name(a->dtype));
  hipStream_t st = as_stream(stream);
  *out_row = -1;
  if (!value || !value->is_valid || a->length == 0) return PDX_OK;  // (a null never equals anything)
  switch (a->dtype) {
    case PDX_FLOAT64: return value->v.f64 != value->v.f64 ? PDX_OK : index_typed<double>(a, value->v.f64, out_row, st);
    // a 4-byte column holds only values of its own width: a scalar that does not round-trip equals no row
    case PDX_FLOAT32: return (double)(float)value->v.f64 != value->v.f64 ? PDX_OK : index_typed<float>(a, (float)value->v.f64, out_row, st);
    case PDX_INT32: return (int64_t)(int32_t)value->v.i64 != value->v.i64 ? PDX_OK : index_typed<uint32_t>(a, (uint32_t)(int32_t)value->v.i64, out_row, st);
    default: return index_typed<uint64_t>(a, value->v.u64, out_row, st);  // int64, uint64, timestamp[ns]: equal values are equal bits
  }
}

extern "C" int pdx_arg_extreme(int is_max, const pdx_column* cols, int ncols, int64_t* out_rows, void* stream) {
  if (!cols || !out_rows) return fail(PDX_INVALID, "pdx_arg_extreme: null argument");
  if (ncols < 1 || ncols > 65535) return fail(PDX_INVALID, "pdx_arg_extreme: 1 .. 65535 columns a call");
  int64_t nmax = 0;
  for (int c = 0; c < ncols; ++c) {
    if (cols[c].dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, "pdx_arg_extreme: dtype bool is not supported");
    if (!lookup_dtype(cols[c].dtype)) return fail(PDX_NOT_IMPLEMENTED, "pdx_arg_extreme: unsupported dtype");
    PDX_TRY(check_column(&cols[c], "pdx_arg_extreme", true));
    nmax = std::max(nmax, cols[c].length);
  }
  hipStream_t st = as_stream(stream);
  for (int c = 0; c < ncols; ++c) out_rows[c] = -1;
  if (nmax == 0) return PDX_OK;
  std::vector<AxCol> host((size_t)ncols);
  for (int c = 0; c < ncols; ++c) {
    const ColView e = col_view(cols[c]);
    const uintptr_t pv = reinterpret_cast<uintptr_t>(e.values);
    host[c] = AxCol{e.values, e.valid, e.voff, cols[c].length, cols[c].dtype, pv % (size_t)(2 * dtype_bytes(cols[c].dtype)) == 0 ? 1 : 0};
  }
  Scratch s;
  PDX_PROFILE("arg_extreme", st);
  // the whole device a call, shared by the columns; a partial per workgroup
  const int grid = grid_for(nmax, kLkBlock, 8, std::max(1, (kCUs * 8) / ncols));
  AxCol* tab = s.get<AxCol>((size_t)ncols);
  AxPair* part = s.get<AxPair>((size_t)ncols * (size_t)grid);
  long long* rows = s.get<long long>((size_t)ncols);
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemcpyAsync(tab, host.data(), sizeof(AxCol) * (size_t)ncols, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ax_partial, dim3(grid, ncols), dim3(kLkBlock), 0, st, tab, is_max ? 1 : 0, part);
  hipLaunchKernelGGL(k_ax_final, dim3(ncols), dim3(64), 0, st, part, grid, rows);
  PDX_LAUNCH_CHECK();
  std::vector<long long> hrows((size_t)ncols);
  PDX_TRY(read_back(hrows.data(), rows, sizeof(long long) * (size_t)ncols, st));  // (also keeps `host` alive until the table has been copied)
  for (int c = 0; c < ncols; ++c) out_rows[c] = (int64_t)hrows[c];
  return PDX_OK;
}

extern "C" int pdx_dictionary_encode(const pdx_column* a, pdx_mut_column* out_codes, pdx_mut_column* out_dict, void* stream) {
  if (!a) return fail(PDX_INVALID, "pdx_dictionary_encode: null column");
  if (a->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, "pdx_dictionary_encode: dtype bool is not supported");
  if (!lookup_dtype(a->dtype)) return fail(PDX_NOT_IMPLEMENTED, "pdx_dictionary_encode: unsupported dtype");
  PDX_TRY(check_column(a, "pdx_dictionary_encode", true));
  const int64_t n = a->length;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_dictionary_encode: more than 2^31-1 rows per call is not supported yet (the group-by handle's row limit)");
  PDX_TRY(check_out("pdx_dictionary_encode", out_codes, PDX_INT32, n));
  PDX_TRY(check_out("pdx_dictionary_encode", out_dict, a->dtype, n));
  const uint8_t* valid = validity_or_null(a);
  if (n > 0 && valid && !out_codes->validity) return fail(PDX_INVALID, "pdx_dictionary_encode: the codes need a validity buffer (a null row gets a null code)");
  hipStream_t st = as_stream(stream);
  out_codes->length = n;
  out_codes->null_count = 0;
  out_dict->length = 0;
  out_dict->null_count = 0;
  if (n == 0) return PDX_OK;
  Scratch s;
  // the 8-byte bit image as the key: float64 as it stands; a 4-byte column zero-extended, placed so that the validity keeps its bit offset
  pdx_column key = *a;
  key.dtype = a->dtype == PDX_UINT64 || a->dtype == PDX_TIMESTAMP_NS ? a->dtype : is_narrow(a->dtype) ? PDX_UINT64 : PDX_INT64;
  if (is_narrow(a->dtype)) {
    const int64_t off7 = a->offset & 7;
    unsigned long long* wide = s.get<unsigned long long>((size_t)(n + off7));
    PDX_SCRATCH_CHECK(s);
    hipLaunchKernelGGL(k_lk_widen, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, static_cast<const uint32_t*>(a->values) + a->offset, n, wide + off7);
    PDX_LAUNCH_CHECK();
    key.values = wide;
    key.offset = off7;
    key.validity = a->validity ? static_cast<const uint8_t*>(a->validity) + (a->offset >> 3) : nullptr;
  }
  pdx_groupby* gb = nullptr;
  PDX_TRY(pdx_groupby_create(&key, stream, &gb));
  struct Closer {
    pdx_groupby* g;
    ~Closer() { pdx_groupby_destroy(g); }
  } closer{gb};
  const int64_t G = pdx_groupby_num_groups(gb);
  if (G <= 0 || G > n) return fail(PDX_DEVICE, "pdx_dictionary_encode: the group-by returned an impossible group count");
  uint32_t* ids = s.get<uint32_t>((size_t)n);
  unsigned long long* uniq = s.get<unsigned long long>((size_t)G);
  uint8_t* uvalid = s.get<uint8_t>((size_t)((G + 7) / 8 + 8));
  unsigned long long* ctl = s.get<unsigned long long>(2);  // [0] null rows, [1] the null group's id
  PDX_SCRATCH_CHECK(s);
  PDX_TRY(pdx_groupby_group_ids(gb, ids, stream));
  pdx_mut_column um{};
  um.dtype = key.dtype;
  um.length = G;
  um.values = uniq;
  um.validity = uvalid;
  PDX_TRY(pdx_groupby_unique_keys(gb, &um, stream));
  note_stream(st);
  PDX_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned long long), st));
  PDX_HIP(hipMemsetAsync(ctl + 1, 0xFF, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_lk_null_group, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, uvalid, G, ctl);
  hipLaunchKernelGGL(k_lk_codes, dim3(grid_for(n, kLkBlock, 4)), dim3(kLkBlock), 0, st, ids, n, ctl, static_cast<int32_t*>(out_codes->values),
                     static_cast<uint8_t*>(out_codes->validity));
  if (is_narrow(a->dtype)) hipLaunchKernelGGL(k_lk_dict<uint32_t>, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, uniq, G, ctl, static_cast<uint32_t*>(out_dict->values));
  else hipLaunchKernelGGL(k_lk_dict<unsigned long long>, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, uniq, G, ctl, static_cast<unsigned long long*>(out_dict->values));
  PDX_LAUNCH_CHECK();
  unsigned long long h[2];
  PDX_TRY(read_back(h, ctl, sizeof(h), st));
  out_codes->null_count = (int64_t)h[0];
  out_dict->length = G - (h[1] != ~0ull ? 1 : 0);
  return PDX_OK;
}
