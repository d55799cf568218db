// cum_scan.hpp -- value-carrying prefix scans for gfx950: Scan<T, Op> behind pdx_cumulative / pdx_fill_null (cumulative.hip).
//
// An element is (value, flag).  A null row is part of the element, not a second pass:
//   cumulative, skip_nulls     : a null row carries the operator's identity, flag = 1; the output row is null where the input is
//   cumulative, not skip_nulls : flag = the row's validity, combined by AND: the inclusive flag is the prefix-AND, rows behind the first
//                                null are null
//   fill ("latest valid")      : flag = the row's validity; combine keeps the later operand when it is valid
// Every operator is associative but NOT commutative (Arrow's max / min keep the later operand on a tie, signed zeros): operand order
// is kept everywhere.
//
// Three phases, no workgroup waits on another one: k_cum_reduce (one aggregate per tile), the scan of the aggregates (k_cum_groups: a wave
// per group of 64 tiles, any number of workgroups; k_cum_chain: one workgroup, a wave per SUPERGROUP of 64 groups and a sequential chain
// over the supergroups: 120 steps at 1e9 rows), k_cum_apply (per tile, with its carry-in).  The column is walked in one go by default;
// PDX_SCAN_CHUNK_ROWS walks it in chunks of tiles (reduce / scan / apply per chunk), which measured slower.
//
// The evaluation tree is a function of the row index relative to the slice's first row alone (never of an address, the launch shape or
// the chunk length), which is what makes the floating-point sum / product deterministic:
//   row i lives in tile i / 2048, thread (i % 2048) / 8, item i % 8 (blocked: a thread owns 8 consecutive rows = one validity byte)
//   result(i) = ((((S[sg] (+) W2[g - 1]) (+) W1[t - 1]) (+) X[thread]) (+) item_0 (+) ... (+) item_k      (left to right)
//     X      exclusive scan of the 256 thread aggregates of the tile: Hillis-Steele over the 64 lanes of a wave, the waves before it
//            folded in left to right
//     W1[t]  inclusive Hillis-Steele scan of the tile aggregates inside tile t's GROUP g = t / 64 (left out when t is the group's first)
//     W2[g]  the same over the group aggregates W1[64 g + 63] inside g's SUPERGROUP sg = g / 64 (left out when g is its first)
//     S[sg]  carry into supergroup sg: S[0] = start, S[sg + 1] = S[sg] (+) W2[64 sg + 63], a sequential chain
// A chunk boundary may cut a group or a supergroup: the aggregates stay in scratch for the whole call, the cut one is scanned again from
// the same values.
// Validity: the issue's sketch reads 64 rows per wave and writes the output bitmap by ballot; with the blocked layout a thread's 8 rows ARE one
// output byte, so the input bits are two byte loads per thread and the output byte has one owner (no ballot, no read-modify-write).
#pragma once
#include <limits>
#include "pdx_common.hpp"

namespace pdx {

constexpr int kCumBlock = 256;
constexpr int kCumItems = 8;  // rows per thread: one byte of validity, 64 bytes (32 for 4-byte values) of data
constexpr int kCumTile = kCumBlock * kCumItems;
constexpr int kCumGroup = 64;  // tiles per group, groups per supergroup: one wave scans 64 aggregates

template <typename T>
struct CumElem {
  T v;
  int f;
};

template <typename T>
constexpr bool cum_is_fp() { return __is_same(T, double) || __is_same(T, float); }

// integers are instantiated unsigned for sum / product: wrapping, the same bits as Arrow's unchecked signed arithmetic
struct CumSum {
  static constexpr bool kFill = false;
  template <typename T>
  __host__ __device__ static T identity() {
    if constexpr (cum_is_fp<T>()) return T(-0.0);  // x + -0.0 == x for every x, -0.0 and 0.0 included
    else return T(0);
  }
  template <typename T>
  __device__ __forceinline__ static T ap(T a, T b) { return a + b; }
};
struct CumProd {
  static constexpr bool kFill = false;
  template <typename T>
  __host__ __device__ static T identity() { return T(1); }
  template <typename T>
  __device__ __forceinline__ static T ap(T a, T b) { return a * b; }
};
// Arrow's Maximum / Minimum: a NaN operand is skipped (so NaN is the identity), the LATER operand wins a tie
struct CumMax {
  static constexpr bool kFill = false;
  template <typename T>
  __host__ __device__ static T identity() {
    if constexpr (cum_is_fp<T>()) return std::numeric_limits<T>::quiet_NaN();
    else return std::numeric_limits<T>::lowest();
  }
  template <typename T>
  __device__ __forceinline__ static T ap(T a, T b) {
    if constexpr (cum_is_fp<T>()) {
      if (a != a) return b;
      if (b != b) return a;
    }
    return a > b ? a : b;
  }
};
struct CumMin {
  static constexpr bool kFill = false;
  template <typename T>
  __host__ __device__ static T identity() {
    if constexpr (cum_is_fp<T>()) return std::numeric_limits<T>::quiet_NaN();
    else return std::numeric_limits<T>::max();
  }
  template <typename T>
  __device__ __forceinline__ static T ap(T a, T b) {
    if constexpr (cum_is_fp<T>()) {
      if (a != a) return b;
      if (b != b) return a;
    }
    return a < b ? a : b;
  }
};
// fill_null_forward: the latest valid row (values are moved as bits: T is unsigned)
struct CumLatest {
  static constexpr bool kFill = true;
  template <typename T>
  __host__ __device__ static T identity() { return T(0); }
};

template <typename T, typename Op>
__device__ __forceinline__ CumElem<T> cum_comb(CumElem<T> a, CumElem<T> b) {
  if constexpr (Op::kFill) return CumElem<T>{b.f ? b.v : a.v, a.f | b.f};
  else return CumElem<T>{Op::template ap<T>(a.v, b.v), a.f & b.f};
}
template <typename T, typename Op>
__host__ __device__ __forceinline__ CumElem<T> cum_identity() { return CumElem<T>{Op::template identity<T>(), Op::kFill ? 0 : 1}; }

template <typename T>
__device__ __forceinline__ CumElem<T> cum_shfl_up(CumElem<T> e, int d) {
  CumElem<T> r;
  if constexpr (sizeof(T) == 8) {
    // moved as bits: the shuffle has no overload for every 8-byte type used here
    unsigned long long u = __builtin_bit_cast(unsigned long long, e.v);
    r.v = __builtin_bit_cast(T, __shfl_up(u, d, 64));
  } else {
    unsigned u = __builtin_bit_cast(unsigned, e.v);
    r.v = __builtin_bit_cast(T, __shfl_up(u, d, 64));
  }
  r.f = __shfl_up(e.f, d, 64);
  return r;
}
template <typename T, typename Op>
__device__ __forceinline__ CumElem<T> cum_wave_inclusive(CumElem<T> x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    CumElem<T> y = cum_shfl_up(x, d);
    if (lane >= d) x = cum_comb<T, Op>(y, x);
  }
  return x;
}
// exclusive scan of one element per thread over the 256 threads of a tile, and the tile's aggregate
template <typename T, typename Op>
__device__ __forceinline__ CumElem<T> cum_block_exclusive(CumElem<T> x, CumElem<T>* total, CumElem<T>* smem /* 4 */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  CumElem<T> inc = cum_wave_inclusive<T, Op>(x);
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  CumElem<T> pre = cum_identity<T, Op>(), tot = cum_identity<T, Op>();
#pragma unroll
  for (int w = 0; w < kCumBlock / 64; ++w) {
    CumElem<T> v = smem[w];
    if (w < wave) pre = cum_comb<T, Op>(pre, v);
    tot = cum_comb<T, Op>(tot, v);
  }
  __syncthreads();
  CumElem<T> exc = cum_shfl_up(inc, 1);
  if (lane == 0) exc = cum_identity<T, Op>();
  *total = tot;
  return cum_comb<T, Op>(pre, exc);
}

template <typename T>
struct alignas(16) CumVec {
  T v[16 / sizeof(T)];
};

struct CumArgs {
  const void* in;         // first row of the slice
  const uint8_t* valid;   // or null
  int64_t voff;           // bit offset of the slice's first row in `valid`
  int64_t n;              // rows
  int64_t padded;         // n rounded up to 8: a backward scan's logical row r is physical row padded - 1 - r
  int rev;                // bfill: scan from the end
  int vec;                // in and out start on 16 bytes
  int skip;               // cumulative: skip_nulls
  void* out;
  uint8_t* ovalid;        // or null
  unsigned long long* nulls;  // null rows written (only counted when ovalid)
  unsigned* tile_nulls;       // ... per tile (scratch), summed into *nulls by k_cum_sum_nulls: no same-address atomics
};

// the thread's 8 rows in LOGICAL order; pb = first physical row of the 8 (a multiple of 8), cnt = how many of them exist
template <typename T, typename Op>
__device__ __forceinline__ void cum_load(const CumArgs& a, int64_t r0, CumElem<T> (&e)[kCumItems], unsigned& bits, int64_t& pb, int& cnt) {
  const T* in = static_cast<const T*>(a.in);
  T x[kCumItems];
  bits = 0;
  cnt = 0;
  pb = a.rev ? a.padded - kCumItems - r0 : r0;
  if (r0 < a.padded) {
    const int64_t left = a.n - pb;
    cnt = left < kCumItems ? (int)left : kCumItems;
    if (a.vec && cnt == kCumItems) {
      constexpr int kPer = 16 / sizeof(T);
#pragma unroll
      for (int q = 0; q < kCumItems / kPer; ++q) {
        const CumVec<T> v = *reinterpret_cast<const CumVec<T>*>(in + pb + q * kPer);
#pragma unroll
        for (int k = 0; k < kPer; ++k) x[q * kPer + k] = v.v[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCumItems; ++k) x[k] = k < cnt ? in[pb + k] : T(0);
    }
    const unsigned mask = (1u << cnt) - 1u;
    bits = mask;
    if (a.valid) {
      const int64_t pos = a.voff + pb, byte = pos >> 3;
      const int sh = (int)(pos & 7);
      unsigned w = a.valid[byte];
      if (((pos + cnt - 1) >> 3) > byte) w |= (unsigned)a.valid[byte + 1] << 8;
      bits = (w >> sh) & mask;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kCumItems; ++k) x[k] = T(0);
  }
  if (a.rev) bits = __brev(bits) >> 24;
#pragma unroll
  for (int k = 0; k < kCumItems; ++k) {
    const T xv = a.rev ? x[kCumItems - 1 - k] : x[k];
    const int ok = (bits >> k) & 1;
    if constexpr (Op::kFill) e[k] = CumElem<T>{xv, ok};
    else e[k] = CumElem<T>{ok ? xv : Op::template identity<T>(), a.skip ? 1 : ok};
  }
}

template <typename T, typename Op>
__global__ void __launch_bounds__(kCumBlock) k_cum_reduce(CumArgs a, int64_t tile0, CumElem<T>* __restrict__ agg) {
  __shared__ CumElem<T> smem[kCumBlock / 64];
  const int64_t tile = tile0 + blockIdx.x;
  CumElem<T> e[kCumItems];
  unsigned bits;
  int64_t pb;
  int cnt;
  cum_load<T, Op>(a, tile * kCumTile + (int64_t)threadIdx.x * kCumItems, e, bits, pb, cnt);
  CumElem<T> acc = e[0];
#pragma unroll
  for (int k = 1; k < kCumItems; ++k) acc = cum_comb<T, Op>(acc, e[k]);
  CumElem<T> total;
  (void)cum_block_exclusive<T, Op>(acc, &total, smem);
  if (threadIdx.x == 0) agg[tile] = total;
}

// tiles [t0, t1) have fresh aggregates: W1 for every group they touch, a wave per group (any number of workgroups)
template <typename T, typename Op>
__global__ void __launch_bounds__(kCumBlock) k_cum_groups(const CumElem<T>* __restrict__ agg, CumElem<T>* __restrict__ w1, int64_t g0, int64_t g1, int64_t t1) {
  const int lane = threadIdx.x & 63;
  const int64_t g = g0 + (int64_t)blockIdx.x * (kCumBlock / 64) + (threadIdx.x >> 6);
  if (g > g1) return;
  const int64_t t = g * kCumGroup + lane;
  CumElem<T> x = t < t1 ? agg[t] : cum_identity<T, Op>();
  x = cum_wave_inclusive<T, Op>(x);
  if (t < t1) w1[t] = x;
}
// one workgroup: W2 for every supergroup the groups [g0, g1] touch (only complete groups have an aggregate), S behind every supergroup
// they complete
template <typename T, typename Op>
__global__ void __launch_bounds__(kCumBlock) k_cum_chain(const CumElem<T>* __restrict__ w1, CumElem<T>* __restrict__ w2, CumElem<T>* __restrict__ scarry,
                                                         int64_t g0, int64_t g1, int64_t t0, int64_t t1, CumElem<T> start) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s0 = g0 / kCumGroup, s1 = g1 / kCumGroup;
  const int64_t gdone = t1 / kCumGroup;  // groups [0, gdone) are complete
  if (threadIdx.x == 0 && t0 == 0) scarry[0] = start;
  for (int64_t sg = s0 + wave; sg <= s1; sg += kCumBlock / 64) {
    const int64_t g = sg * kCumGroup + lane;
    CumElem<T> x = g < gdone ? w1[g * kCumGroup + kCumGroup - 1] : cum_identity<T, Op>();
    x = cum_wave_inclusive<T, Op>(x);
    if (g < gdone) w2[g] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    CumElem<T> c = scarry[s0];
    for (int64_t sg = s0; sg <= s1; ++sg) {
      const int64_t last = sg * kCumGroup + kCumGroup - 1;
      if (last >= gdone) break;
      c = cum_comb<T, Op>(c, w2[last]);
      scarry[sg + 1] = c;
    }
  }
}

__global__ void __launch_bounds__(kCumBlock) k_cum_sum_nulls(const unsigned* __restrict__ tile_nulls, int64_t tiles, unsigned long long* __restrict__ nulls) {
  __shared__ unsigned long long part[kCumBlock / 64];
  unsigned long long nc = 0;
  for (int64_t t = threadIdx.x; t < tiles; t += kCumBlock) nc += tile_nulls[t];
  for (int d = 32; d > 0; d >>= 1) nc += __shfl_down(nc, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = nc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (int w = 0; w < kCumBlock / 64; ++w) tot += part[w];
    *nulls = tot;
  }
}

template <typename T, typename Op>
__global__ void __launch_bounds__(kCumBlock) k_cum_apply(CumArgs a, int64_t tile0, const CumElem<T>* __restrict__ w1, const CumElem<T>* __restrict__ w2,
                                                         const CumElem<T>* __restrict__ scarry) {
  __shared__ CumElem<T> smem[kCumBlock / 64];
  __shared__ unsigned wave_nulls[kCumBlock / 64];
  const int64_t tile = tile0 + blockIdx.x;
  CumElem<T> e[kCumItems];
  unsigned bits;
  int64_t pb;
  int cnt;
  cum_load<T, Op>(a, tile * kCumTile + (int64_t)threadIdx.x * kCumItems, e, bits, pb, cnt);
  CumElem<T> acc = e[0];
#pragma unroll
  for (int k = 1; k < kCumItems; ++k) acc = cum_comb<T, Op>(acc, e[k]);
  CumElem<T> total;
  const CumElem<T> exc = cum_block_exclusive<T, Op>(acc, &total, smem);
  const int64_t group = tile / kCumGroup;
  CumElem<T> run = scarry[group / kCumGroup];
  if (group % kCumGroup) run = cum_comb<T, Op>(run, w2[group - 1]);
  if (tile % kCumGroup) run = cum_comb<T, Op>(run, w1[tile - 1]);
  run = cum_comb<T, Op>(run, exc);
  T r[kCumItems];
  unsigned obits = 0;
#pragma unroll
  for (int k = 0; k < kCumItems; ++k) {
    run = cum_comb<T, Op>(run, e[k]);
    r[k] = run.v;
    const unsigned ok = Op::kFill ? (unsigned)run.f : (((bits >> k) & 1u) & (unsigned)run.f);
    obits |= ok << k;
  }
  unsigned nc = 0;
  if (cnt > 0) {
    T* out = static_cast<T*>(a.out);
    T p[kCumItems];
#pragma unroll
    for (int k = 0; k < kCumItems; ++k) p[k] = a.rev ? r[kCumItems - 1 - k] : r[k];
    if (a.rev) obits = __brev(obits) >> 24;
    obits &= (1u << cnt) - 1u;
    if (a.vec && cnt == kCumItems) {
      constexpr int kPer = 16 / sizeof(T);
#pragma unroll
      for (int q = 0; q < kCumItems / kPer; ++q) {
        CumVec<T> v;
#pragma unroll
        for (int k = 0; k < kPer; ++k) v.v[k] = p[q * kPer + k];
        *reinterpret_cast<CumVec<T>*>(out + pb + q * kPer) = v;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kCumItems; ++k)
        if (k < cnt) out[pb + k] = p[k];
    }
    if (a.ovalid) {
      a.ovalid[pb >> 3] = (uint8_t)obits;  // the thread's 8 rows are exactly one byte of the output bitmap (its offset is 0)
      nc = (unsigned)(cnt - __popc(obits));
    }
  }
  if (a.ovalid) {  // the tile's null rows go to its own scratch word: one same-address atomic per wave measured 20 ms at 1e9 rows
    for (int d = 32; d > 0; d >>= 1) nc += __shfl_down(nc, d, 64);
    if ((threadIdx.x & 63) == 0) wave_nulls[threadIdx.x >> 6] = nc;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tot = 0;
      for (int w = 0; w < kCumBlock / 64; ++w) tot += wave_nulls[w];
      a.tile_nulls[tile] = tot;
    }
  }
}

// the whole scan: chunk_tiles tiles per round of reduce / scan of the aggregates / apply (< 1: one round, the plain three-phase form)
template <typename T, typename Op>
int cum_scan_launch(CumArgs a, CumElem<T> start, int64_t chunk_tiles, Scratch& s, hipStream_t st) {
  const int64_t tiles = ceil_div(a.padded, kCumTile);
  if (tiles <= 0) return PDX_OK;
  const int64_t groups = ceil_div(tiles, kCumGroup);
  CumElem<T>* agg = s.get<CumElem<T>>((size_t)tiles);
  CumElem<T>* w1 = s.get<CumElem<T>>((size_t)tiles);
  CumElem<T>* w2 = s.get<CumElem<T>>((size_t)groups);
  CumElem<T>* scarry = s.get<CumElem<T>>((size_t)(groups / kCumGroup + 2));
  a.tile_nulls = a.ovalid ? s.get<unsigned>((size_t)tiles) : nullptr;
  PDX_SCRATCH_CHECK(s);
  if (chunk_tiles < 1) chunk_tiles = tiles;
  if (chunk_tiles > (1 << 30)) chunk_tiles = 1 << 30;  // one launch's grid
  for (int64_t t0 = 0; t0 < tiles; t0 += chunk_tiles) {
    const int64_t t1 = t0 + chunk_tiles < tiles ? t0 + chunk_tiles : tiles;
    const int64_t g0 = t0 / kCumGroup, g1 = (t1 - 1) / kCumGroup;
    const dim3 grid((unsigned)(t1 - t0)), block(kCumBlock);
    hipLaunchKernelGGL((k_cum_reduce<T, Op>), grid, block, 0, st, a, t0, agg);
    hipLaunchKernelGGL((k_cum_groups<T, Op>), dim3((unsigned)ceil_div(g1 - g0 + 1, kCumBlock / 64)), block, 0, st, agg, w1, g0, g1, t1);
    hipLaunchKernelGGL((k_cum_chain<T, Op>), dim3(1), block, 0, st, w1, w2, scarry, g0, g1, t0, t1, start);
    hipLaunchKernelGGL((k_cum_apply<T, Op>), grid, block, 0, st, a, t0, w1, w2, scarry);
  }
  if (a.ovalid) hipLaunchKernelGGL(k_cum_sum_nulls, dim3(1), dim3(kCumBlock), 0, st, a.tile_nulls, tiles, a.nulls);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

}  // namespace pdx
