// quantile.hpp -- order-preserving keys and the level descriptors of the radix select behind pdx_quantile (quantile.hip).
//
// A value becomes an unsigned key whose unsigned order is the value's order (the image pdx_argsort sorts on, align.hip sort_image; a
// 32-bit twin serves the 4-byte dtypes): -0.0 and 0.0 share one key, NaN and null rows have no key and take no part.
#pragma once
#include "pdx_common.hpp"

namespace pdx {

constexpr int kQBits = 11;             // digit width of one select level: 2048 bins, 8 KB of LDS counters per workgroup
constexpr int kQBins = 1 << kQBits;
constexpr int kQBlock = 256;
constexpr int kQMaxTargets = 128;      // ranks resolved by one run over the column: lo and lo + 1 of 64 quantiles
constexpr int kQSmall = 4096;          // a bucket of at most this many rows is finished by one workgroup's LDS sort

template <typename T> struct QKey;
template <> struct QKey<double> {
  using K = uint64_t;
  static __host__ __device__ __forceinline__ bool key(double x, K* k) {
    if (x != x) return false;
    K u;
    if (x == 0.0) u = 0;
    else __builtin_memcpy(&u, &x, 8);
    *k = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return true;
  }
  static double value(K k) {
    const K u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
  }
  static constexpr K kZero = 0x8000000000000000ull;
  static constexpr bool kFloat = true;
};
template <> struct QKey<float> {
  using K = uint32_t;
  static __host__ __device__ __forceinline__ bool key(float x, K* k) {
    if (x != x) return false;
    K u;
    if (x == 0.0f) u = 0;
    else __builtin_memcpy(&u, &x, 4);
    *k = (u >> 31) ? ~u : (u | 0x80000000u);
    return true;
  }
  static float value(K k) {
    const K u = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
  }
  static constexpr K kZero = 0x80000000u;
  static constexpr bool kFloat = true;
};
template <> struct QKey<int64_t> {
  using K = uint64_t;
  static __host__ __device__ __forceinline__ bool key(int64_t x, K* k) {
    *k = (K)x ^ 0x8000000000000000ull;
    return true;
  }
  static int64_t value(K k) { return (int64_t)(k ^ 0x8000000000000000ull); }
  static constexpr K kZero = 0;
  static constexpr bool kFloat = false;
};
template <> struct QKey<uint64_t> {
  using K = uint64_t;
  static __host__ __device__ __forceinline__ bool key(uint64_t x, K* k) {
    *k = x;
    return true;
  }
  static uint64_t value(K k) { return k; }
  static constexpr K kZero = 0;
  static constexpr bool kFloat = false;
};
template <> struct QKey<int32_t> {
  using K = uint32_t;
  static __host__ __device__ __forceinline__ bool key(int32_t x, K* k) {
    *k = (K)x ^ 0x80000000u;
    return true;
  }
  static int32_t value(K k) { return (int32_t)(k ^ 0x80000000u); }
  static constexpr K kZero = 0;
  static constexpr bool kFloat = false;
};

// One segment of a level: level 0 has one (the column itself, typed values + validity); later levels read compacted keys.  The
// workgroups of a level form one flat grid; segment s owns the workgroups [first_block, first_block + nblocks), each `chunk` rows.
struct QSeg {
  const void* src;
  uint64_t size;
  uint64_t chunk;
  uint32_t first_block, nblocks;
  uint32_t sel_begin, sel_end;  // this segment's entries in the level's QSel list (the buckets that are compacted)
};
// one bucket of a segment that is copied out for the next level
struct QSel {
  void* dst;
  uint64_t base_index;  // where this bucket's per-workgroup output offsets start in the offsets array
  uint32_t seg, digit;
};
// one rank asked of a small (sorted in LDS) segment
struct QPick {
  const void* src;
  uint64_t size, rank;
};
struct QPicked {
  uint64_t key, nth_equal;  // the key of that rank, and how many equal keys precede it inside the segment
};

}  // namespace pdx
