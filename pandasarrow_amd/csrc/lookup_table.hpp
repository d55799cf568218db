// lookup_table.hpp -- the open-addressing value -> position table shared by the set lookups (lookup.hip) and the hash join (join.hip).
//
// Linear probing over slots = the power of two >= 2 * entries (load factor <= 0.5), splitmix64 of the value's bit image.  A slot of pos[]
// holds the FIRST position of its value in the set (atomicCAS claims a slot, atomicMin lowers the position of a duplicate), kLkEmpty when
// it is free; null entries stay out and the first of them is remembered.  k_lk_keys then copies the values beside the positions, so that a
// probe reads the table alone -- from LDS (up to kLkLdsMaxEntries entries, 12 B a slot) or from where it was built.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include "pdx_common.hpp"

namespace pdx {

constexpr int kLkBlock = 256;
constexpr int kLkWaves = kLkBlock / 64;
constexpr int64_t kLkLdsMaxEntries = 2048;  // 4096 slots * (8 + 4) B = 48 KB of LDS per workgroup
constexpr uint32_t kLkEmpty = 0xFFFFFFFFu;  // a slot without a value (positions are < 2^31 - 1)

// bits 0..31 of x moved to the even bit positions of a 64-bit word (wave-uniform operands: scalar instructions)
__device__ __forceinline__ uint64_t lk_spread(uint64_t x) {
  x &= 0xFFFFFFFFull;
  x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
  x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
  x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// the number of slots for m entries
inline uint64_t lk_slots_for(int64_t m) {
  uint64_t slots = 2;
  while (slots < 2 * (uint64_t)m) slots <<= 1;
  return slots;
}

// the largest set that is probed from LDS: kLkLdsMaxEntries, lowered by PDX_LOOKUP_LDS_MAX
inline int64_t lookup_lds_max() {
  int64_t lim = kLkLdsMaxEntries;
  if (const char* e = getenv("PDX_LOOKUP_LDS_MAX")) {
    char* end = nullptr;
    const long long x = strtoll(e, &end, 10);
    if (end != e) lim = std::min<int64_t>(kLkLdsMaxEntries, std::max<long long>(0, x));  // (never above what the LDS holds)
  }
  return lim;
}

// ---------------------------------------------------------------- build
template <typename U>
__global__ void __launch_bounds__(256) k_lk_insert(const U* __restrict__ set, const uint8_t* __restrict__ valid, int64_t voff, int64_t m, uint32_t* __restrict__ pos,
                                                   uint32_t mask, uint32_t* __restrict__ first_null) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    if (valid && !bit_get(valid, voff + j)) {
      atomicMin(first_null, (uint32_t)j);
      continue;
    }
    const U k = set[j];
    uint32_t h = (uint32_t)splitmix64((uint64_t)k) & mask;
    for (uint64_t step = 0; step <= (uint64_t)mask; ++step) {  // (an empty slot exists: at most half of them are taken)
      const uint32_t p = atomicCAS(&pos[h], kLkEmpty, (uint32_t)j);
      if (p == kLkEmpty) break;
      if (set[p] == k) {  // (p < m: only positions are ever stored)
        atomicMin(&pos[h], (uint32_t)j);
        break;
      }
      h = (h + 1) & mask;
    }
  }
}
template <typename U>
__global__ void __launch_bounds__(256) k_lk_keys(const U* __restrict__ set, const uint32_t* __restrict__ pos, uint64_t slots, U* __restrict__ keys) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < slots; h += stride) {
    const uint32_t p = pos[h];
    keys[h] = p == kLkEmpty ? U(0) : set[p];
  }
}

// the position of k in a table (keys / pos: LDS or global pointers), -1 when it is not there; at most mask + 1 steps whatever the table holds
template <typename U>
__device__ __forceinline__ int32_t lk_find(const U* keys, const uint32_t* pos, uint32_t mask, U k) {
  uint32_t h = (uint32_t)splitmix64((uint64_t)k) & mask;
  for (uint64_t step = 0; step <= (uint64_t)mask; ++step) {
    const uint32_t p = pos[h];
    if (p == kLkEmpty) return -1;
    if (keys[h] == k) return (int32_t)p;
    h = (h + 1) & mask;
  }
  return -1;
}

// a 4-byte column as the 8-byte key the group-by takes: the bit image, zero-extended
__global__ inline void k_lk_widen(const uint32_t* __restrict__ v, int64_t n, unsigned long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (unsigned long long)v[i];
}

}  // namespace pdx
