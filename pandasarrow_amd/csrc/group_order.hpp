// group_order.hpp -- the (group, value, row) order shared by pdx_groupby_quantile (quantile.hip) and pdx_groupby_mode (mode.hip):
// pdx_argsort of the values (numbers ascending, then NaN, then nulls; stable), then one stable radix sort of that row list by group id.
// Also the ok-bytes -> validity-bits kernel both use for their per-group results.
#pragma once
#include "pdx_common.hpp"
#include "radix_sort.hpp"

namespace pdx {

__global__ inline void k_go_gather(const unsigned long long* __restrict__ order, const uint32_t* __restrict__ gids, int64_t n, uint32_t* __restrict__ keys,
                                   uint32_t* __restrict__ rows) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t r = (uint32_t)order[i];
    rows[i] = r;
    keys[i] = gids[r];
  }
}
// ok bytes -> validity bits (+ the number of nulls)
__global__ inline void k_go_pack(const uint8_t* __restrict__ ok, int64_t G, uint8_t* __restrict__ bits, unsigned long long* __restrict__ nulls) {
  const int64_t nbytes = (G + 7) >> 3, stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long c = 0;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbytes; b += stride) {
    unsigned byte = 0;
    for (int j = 0; j < 8; ++j) {
      const int64_t g = b * 8 + j;
      if (g < G) {
        if (ok[g]) byte |= 1u << j;
        else ++c;
      }
    }
    if (bits) bits[b] = (uint8_t)byte;
  }
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(nulls, c);
}

// *keys: the group id of every position, *rows: its row; both n entries living in `s`; groups ascending, inside a group the values ascending
// with NaN and then nulls behind them, equal values in row order
inline int build_group_value_order(pdx_groupby* gb, const pdx_column* values, const uint32_t** keys, const uint32_t** rows, Scratch& s, void* stream,
                                   hipStream_t st) {
  const int64_t n = values->length, G = pdx_groupby_num_groups(gb);
  unsigned long long* order = s.get<unsigned long long>((size_t)n);
  uint32_t* gids = s.get<uint32_t>((size_t)n);
  uint32_t* k0 = s.get<uint32_t>((size_t)n);
  uint32_t* v0 = s.get<uint32_t>((size_t)n);
  uint32_t* k1 = s.get<uint32_t>((size_t)n);
  uint32_t* v1 = s.get<uint32_t>((size_t)n);
  uint32_t* k2 = s.get<uint32_t>((size_t)n);
  uint32_t* v2 = s.get<uint32_t>((size_t)n);
  PDX_SCRATCH_CHECK(s);
  pdx_mut_column om{};
  om.dtype = PDX_UINT64;
  om.length = n;
  om.values = order;
  PDX_TRY(pdx_argsort(values, 1, &om, stream));
  PDX_TRY(pdx_groupby_group_ids(gb, gids, stream));
  note_stream(st);
  hipLaunchKernelGGL(k_go_gather, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, order, gids, n, k0, v0);
  PDX_LAUNCH_CHECK();
  *keys = k0;
  *rows = v0;
  if (G > 1) {
    int bits = 1;
    while (bits < 32 && ((uint64_t)(G - 1) >> bits)) ++bits;
    PDX_TRY((radix_sort_pairs<uint32_t>(k0, v0, k1, v1, k2, v2, n, bits, keys, rows, true, s, st)));
  }
  return PDX_OK;
}

}  // namespace pdx
