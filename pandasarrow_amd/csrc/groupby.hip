// groupby.hip -- hash group-by with sum/mean/min/max/count, and the resample front-end, for gfx950.
//
// Replaces (reference file:line)
//   GroupBy::makeGroups  src/dataframe.cpp:1571-1600   Grouper::Make/Consume/GetUniques  -> pdx_groupby_create
//   processIndex/processEach (MakeGroupings + ApplyGroupings of every column, 1539-1569)  -> deferred, per aggregated
//                                                                                            column, to pdx_groupby_agg
//   GROUPBY_AGG / GROUPBY_NUMERIC_AGG  src/pd_core_macros.h:5-147 (one CallFunction per group)  -> pdx_groupby_agg
//   GroupBy::group / MakeSubDataFrame / apply (src/group_by.h:38-77: walk the per-group arrays)  -> pdx_groupby_groupings
//   pd::resample / makeGroupInfo / generate_bins_dt64 / GroupInfo::downsample
//        src/resample.h:19-43,91-122  src/resample.cpp:11-83,85-178,202-295               -> pdx_resample_create
//
// Data path for N rows, G groups (all arrays in HBM; DESIGN.md section 3 has the kernel-by-kernel accounting):
//   1. key -> slot.  Dense integer key domain (span < min(2^26, 4N)): slot = key - min, or its residue form key & (2^b - 1) built
//      in ONE speculative pass together with the exact min/max, first rows through an LDS-resident "seen" bitmap
//      (k_dense_slots*, k_sample_key_range).  General keys: hash -> stable partition of (key, row id) by the low 8 hash bits
//      (k_hash_bucket_hist + radix scatter; a second level for very many groups) -> one workgroup per bucket builds the
//      bucket's table region in LDS (k_hash_probe_lds; skewed buckets: head rows there, the rest in chunks against an LDS
//      snapshot, k_hash_probe_lds_tail; k_hash_probe_part is the memory-side fallback).  Tiny inputs: one global
//      open-addressing table (k_hash_insert).  Host side: gb_create.hpp, one builder per path (try_dense_speculative,
//      try_dense_exact, build_hash_partitioned, build_hash_global), each returning a SlotDomain.
//   2. occupied slots are compacted (slot order) and sorted by first_row -> dense gid in FIRST-OCCURRENCE order (finish_group_ids).
//   3. per aggregated column: stable LSD radix sort of (slot, value) by slot (radix_sort.hpp) -> every group's values
//      contiguous IN ROW ORDER.  For sum/mean/min/max/count (and variance) the last 6 slot bits are not sorted: k_flr_reduce
//      ranks each 2560-row tile by them in LDS, stages the rows by 16-value leaf, sums one leaf per thread and pushes the leaves
//      through Arrow's binary counter with one lane per group (k_flr_wave: one wave per run, for nullable values / min / max).
//      Dense slots + values without nulls: narrowing sort (the key shrinks 4 -> 2 -> 1 byte as digits are consumed; run and
//      group starts come from the scatter offsets, k_level_starts).  Runs longer than 2^19 rows (hot keys) are skipped by the
//      fused kernels and reduced from a side form of the layout (build_side, gb_layout.hpp).
//      Host side: gb_layout.hpp, build_layout over one function per path, each ending in seal_fused / seal_full.
//   4. classic reducers on fully sorted values (skewed keys, small inputs, resample, product/first/last): k_seg_reduce (one wave
//      per group, 16-value leaves + shuffle tree + counter), k_seg_reduce_mid (batches of short groups per wave),
//      k_seg_reduce_sub + k_seg_combine_big (many waves per long group), k_seg_reduce_nullable.
//      Host side of 3. and 4.: gb_agg.hpp, one function per stage of pdx_groupby_agg.
// All fp64 sums reproduce Arrow's pairwise summation bit for bit.  Algorithmic bytes: 16 B/row (8 key + 8 value).
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <memory>
#include <vector>
#include "compact.hpp"
#include "minmax.hpp"
#include "pairwise.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"
#include "temporal_round.hpp"

namespace pdx {
#include "gb_hash_build.hpp"
#include "gb_dense_slots.hpp"
#include "gb_group_ids.hpp"
#include "gb_seg_reduce.hpp"
#include "gb_resample_kernels.hpp"

}  // namespace pdx

using namespace pdx;

#include "gb_handle.hpp"

// the 4-byte logical slots of a hash-partitioned handle, rebuilt from the 2-byte region indexes the LDS build wrote (on demand)
static int ensure_slot_part(pdx_groupby* gb, hipStream_t st) {
  if (!gb->slot_part || gb->slot_part_ready) return PDX_OK;
  hipLaunchKernelGGL(k_slot_part_from_idx16, dim3(grid_for(gb->n, 256, 8)), dim3(256), 0, st, gb->idx16_part, gb->part_off, gb->n, gb->slot_part);
  PDX_LAUNCH_CHECK();
  gb->slot_part_ready = true;
  return PDX_OK;
}

// the original row of every partitioned row (no null keys: the hash build's partition moves the keys alone and finds the groups' first rows
// from positions; the few callers that want every row's origin -- group ids per row, validity flags of nullable values, the memory-side /
// split / skewed-bucket forms of the build -- replay the partition with the row number as the payload)
static int ensure_rows_part(pdx_groupby* gb, hipStream_t st) {
  if (gb->rows_part || !gb->bucket8) return PDX_OK;
  gb->rows_part = gb->own<uint32_t>((size_t)gb->n);
  if (!gb->rows_part) return PDX_OOM;
  return radix_scatter_iota<kPartBits, uint8_t>(gb->bucket8, nullptr, gb->rows_part, gb->n, 0, false, gb->part_off, nullptr, 0, st);
}

namespace pdx {
#include "gb_sort_values.hpp"
#include "gb_flr_reduce.hpp"
#include "gb_more_aggs.hpp"

}  // namespace pdx

// Groups = runs of equal labels over the rows as they stand (segments mode).  *done = false when the labels descend somewhere in
// both integer orders (the caller then builds a dictionary); otherwise the handle is complete.
template <typename LabelFn>
static int build_label_runs(pdx_groupby* gb, int64_t n, LabelFn fn, long long shift, Scratch& s, hipStream_t st, bool* done) {
  *done = false;
  const int64_t nblocks = ceil_div(n, (int64_t)kRunTile), nwaves = ceil_div(n, (int64_t)kRunWaveRows);
  unsigned int* flags = s.get<unsigned int>(2);
  unsigned long long* marks = s.get<unsigned long long>((size_t)((n + 63) >> 6));
  int64_t* offsets = s.get<int64_t>((size_t)nwaves);  // run starts in front of every 1024-row slice
  int64_t* total = s.get<int64_t>(1);
  PDX_SCRATCH_CHECK(s);
  unsigned int hflags[2] = {0, 0};
  int64_t G = 0;
  {
    PDX_PROFILE("label_runs", st);
    PDX_HIP(hipMemsetAsync(flags, 0, sizeof(hflags), st));
    hipLaunchKernelGGL((k_label_run_count<LabelFn, LabelFn::kBatch>), dim3((unsigned)nblocks), dim3(kRunBlock), 0, st, n, fn, marks, offsets, flags);
    PDX_TRY((device_exclusive_scan<int64_t, SumOp>(offsets, offsets, nwaves, total, s, st)));
    PDX_LAUNCH_CHECK();
  }
  PDX_HIP(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, st));
  PDX_HIP(hipMemcpyAsync(&G, total, sizeof(G), hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));
  if (hflags[0] && hflags[1]) return PDX_OK;
  gb->mode = 1;
  gb->G = G;
  gb->seg_start = gb->own<uint32_t>((size_t)G + 1);
  gb->uniques = gb->own<int64_t>((size_t)G);
  gb->first_rows = gb->own<int64_t>((size_t)G);
  gb->unique_ok = gb->own<uint8_t>((size_t)G);
  gb->gid_of_occ = gb->own<uint32_t>((size_t)G);
  if (!gb->seg_start || !gb->uniques || !gb->first_rows || !gb->unique_ok || !gb->gid_of_occ) return PDX_OOM;
  {
    PDX_PROFILE("label_runs", st);
    hipLaunchKernelGGL((k_label_run_write<RunEmit<LabelFn>>), dim3((unsigned)nblocks), dim3(kRunBlock), 0, st, n, marks,
                       RunEmit<LabelFn>{fn, shift, gb->seg_start, gb->uniques, gb->first_rows, gb->gid_of_occ}, offsets, nwaves, total);
    hipLaunchKernelGGL(k_set_last, dim3(1), dim3(64), 0, st, gb->seg_start, G, (uint32_t)n);
    PDX_HIP(hipMemsetAsync(gb->unique_ok, 1, (size_t)G, st));
    PDX_LAUNCH_CHECK();
  }
  PDX_HIP(hipStreamSynchronize(st));
  *done = true;
  return PDX_OK;
}

template <int MODE, bool CEIL>
struct RoundLabel {
  static constexpr int kBatch = 4;
  const long long* ts;
  RoundParams q;
  __device__ long long operator()(int64_t i) const { return round_one<MODE, CEIL>(ts[i], q); }
};
__global__ void k_shift_labels(int64_t* __restrict__ labels, int64_t G, long long shift) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += stride)
    labels[i] = (long long)((unsigned long long)labels[i] + (unsigned long long)shift);
}

// one pinned word per host thread: the target of small device-to-host reads that must not block the launches queued behind them
// (a copy into pageable memory is staged and waits; pinned memory makes hipMemcpyAsync + an event a real overlap)
static unsigned int* hmax_pinned() {
  static thread_local unsigned int* p = nullptr;
  if (!p) {
    void* q = nullptr;
    if (hipHostMalloc(&q, 64, hipHostMallocPortable) != hipSuccess) {
      (void)hipGetLastError();
      q = new unsigned int[16];
    }
    p = static_cast<unsigned int*>(q);
  }
  return p;
}

namespace pdx {
#include "gb_layout.hpp"
#include "gb_acc.hpp"
#include "gb_create.hpp"
}  // namespace pdx

extern "C" {

int pdx_groupby_create(const pdx_column* key, void* stream, pdx_groupby** out) {
  PDX_TRY(check_column(key, "pdx_groupby_create"));
  if (!out) return fail(PDX_INVALID, "pdx_groupby_create: null output");
  if (!is_int_like(key->dtype)) return fail(PDX_NOT_IMPLEMENTED, "pdx_groupby_create: key must be int64/uint64/timestamp");
  const int64_t n = key->length;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_groupby_create: more than 2^31-1 rows per call is not supported yet");
  hipStream_t st = as_stream(stream);
  std::unique_ptr<pdx_groupby> owner(new pdx_groupby());  // released into *out on success
  owner->stream = st;
  pdx_groupby* gb = owner.get();
  gb->n = n;
  gb->key_dtype = key->dtype;
  *out = nullptr;
  if (n == 0) {
    *out = owner.release();
    return PDX_OK;
  }
  Scratch s;
  const CreateTuning t = CreateTuning::read();
  const CreateCtx c{gb, static_cast<const long long*>(key->values) + key->offset, validity_or_null(key), key->offset, n, s, st, t, s.get<HashCtl>(1)};
  if (s.failed) return PDX_OOM;
  // both samples in one host round trip: sortedness (the runs path) and the key range (the speculative dense build)
  const bool want_sorted_sample = t.sorted && n >= 2 && !c.valid;
  const bool want_range_sample = t.dense && t.dense_speculate && t.dense_lds && n >= ((int64_t)1 << 23);
  KeySample sample;
  PDX_TRY(sample_keys(c, want_sorted_sample, want_range_sample, &sample));
  if (sample.maybe_sorted) {
    bool done = false;
    PDX_TRY(build_label_runs(gb, n, KeyLabel{c.keys}, 0, s, st, &done));
    if (done) {
      *out = owner.release();
      return PDX_OK;
    }
  }
  // key -> slot: dense slots when the keys span a small integer range (speculatively, then on the exact range), else a hash table
  SlotDomain d;
  KeyRangeFacts range;
  range.not_dense = !t.dense;
  if (want_range_sample) PDX_TRY(try_dense_speculative(c, sample.range, &d, &range));
  if (!gb->dense && !range.not_dense) PDX_TRY(try_dense_exact(c, &d, &range));
  if (!gb->dense) {
    const bool use_partition = t.partition != 0 && (n >= ((int64_t)1 << 18) || t.partition == 2);
    PDX_TRY(use_partition ? build_hash_partitioned(c, &d) : build_hash_global(c, &d));
  }
  PDX_TRY(finish_group_ids(c, d));
  hipError_t e = hipGetLastError();
  // no drain of the stream: everything the caller can read on the host (G) is known; later calls are ordered by the stream / the event
  if (e == hipSuccess) e = hipEventCreateWithFlags(&gb->ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(gb->ready, st);
  if (e != hipSuccess) return hip_fail(e, "pdx_groupby_create");
  gb->create_stream = st;
  *out = owner.release();
  return PDX_OK;
}

int pdx_groupby_destroy(pdx_groupby* gb) {
  delete gb;
  return PDX_OK;
}
int64_t pdx_groupby_num_groups(const pdx_groupby* gb) { return gb ? gb->G : -1; }
int64_t pdx_groupby_num_rows(const pdx_groupby* gb) { return gb ? gb->n : -1; }

int pdx_groupby_unique_keys(const pdx_groupby* gb, pdx_mut_column* out, void* stream) {
  if (!gb || !out) return fail(PDX_INVALID, "pdx_groupby_unique_keys: null argument");
  if (out->length < gb->G) return fail(PDX_INVALID, "pdx_groupby_unique_keys: output too small");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);  // ordered behind the handle's creation; frees of its blocks are ordered behind this stream
  out->length = gb->G;
  out->null_count = -1;
  if (gb->G == 0) return PDX_OK;
  PDX_HIP(hipMemcpyAsync(out->values, gb->uniques, (size_t)gb->G * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  if (out->validity) {
    hipLaunchKernelGGL(k_pack_bytes, dim3(grid_for((gb->G + 7) / 8, 256)), dim3(256), 0, st, gb->unique_ok, gb->G,
                       static_cast<uint8_t*>(out->validity));
    PDX_LAUNCH_CHECK();
  }
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

int pdx_groupby_first_rows(const pdx_groupby* gb, int64_t* out_rows, void* stream) {
  if (!gb || !out_rows) return fail(PDX_INVALID, "pdx_groupby_first_rows: null argument");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);  // ordered behind the handle's creation; frees of its blocks are ordered behind this stream
  if (gb->G) PDX_HIP(hipMemcpyAsync(out_rows, gb->first_rows, (size_t)gb->G * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

int pdx_groupby_group_ids(pdx_groupby* gb, uint32_t* out_ids, void* stream) {
  if (!gb || !out_ids) return fail(PDX_INVALID, "pdx_groupby_group_ids: null argument");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);  // ordered behind the handle's creation; frees of its blocks are ordered behind this stream
  if (gb->n == 0) return PDX_OK;
  if (gb->mode == 0 && gb->slot_part) PDX_TRY(ensure_slot_part(gb, st));
  if (gb->mode == 0 && gb->slot_part) PDX_TRY(ensure_rows_part(gb, st));
  if (gb->mode == 0 && gb->slot_part)
    hipLaunchKernelGGL(k_part_row_gids, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, st, gb->gid_of_slot, gb->slot_part, gb->rows_part, gb->n,
                       (const int64_t*)nullptr, out_ids, (int64_t*)nullptr);
  else if (gb->mode == 0)
    hipLaunchKernelGGL(k_row_gids, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, st, gb->gid_of_slot, gb->slot_of_row, gb->n, out_ids);
  else
    hipLaunchKernelGGL(k_seg_row_ids, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, st, gb->seg_start, gb->G, gb->n, out_ids);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

int pdx_groupby_map_ids(pdx_groupby* gb, const int64_t* map, int64_t* out, void* stream) {
  if (!gb || !map || !out) return fail(PDX_INVALID, "pdx_groupby_map_ids: null argument");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);  // ordered behind the handle's creation; frees of its blocks are ordered behind this stream
  if (gb->n == 0) return PDX_OK;
  if (gb->mode == 0 && gb->slot_part) PDX_TRY(ensure_slot_part(gb, st));
  if (gb->mode == 0 && gb->slot_part) PDX_TRY(ensure_rows_part(gb, st));
  if (gb->mode == 0 && gb->slot_part)
    hipLaunchKernelGGL(k_part_row_gids, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, st, gb->gid_of_slot, gb->slot_part, gb->rows_part, gb->n, map,
                       (uint32_t*)nullptr, out);
  else
    hipLaunchKernelGGL(k_map_ids, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, st, gb->mode == 0 ? gb->gid_of_slot : nullptr, gb->slot_of_row,
                       gb->seg_start, gb->G, gb->n, map, out);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

}  // extern "C"

namespace pdx {
// offsets[g] = first position of group id g in the sorted ids (g = G: n); rows[i] widened to int64
__global__ void k_groupings_finish(const uint32_t* __restrict__ sorted_ids, const uint32_t* __restrict__ rows32, int64_t n, int64_t G,
                                   int64_t* __restrict__ out_rows, int64_t* __restrict__ out_offsets) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + G + 1; i += stride) {
    if (i < n) {
      out_rows[i] = (int64_t)rows32[i];
      continue;
    }
    const int64_t g = i - n;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)sorted_ids[mid] < g) lo = mid + 1;
      else hi = mid;
    }
    out_offsets[g] = lo;
  }
}
__global__ void k_iota_rows(uint32_t* __restrict__ p, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = (uint32_t)i;
}
}  // namespace pdx

namespace pdx {
// the rows of `gb` stably sorted by group id: *ks the sorted ids, *vs their rows (both n entries, living in `s`)
static int sort_rows_by_group(pdx_groupby* gb, const uint32_t** ks, const uint32_t** vs, Scratch& s, void* stream, hipStream_t st) {
  const int64_t n = gb->n, G = gb->G;
  uint32_t* ids = s.get<uint32_t>((size_t)n);
  uint32_t* rows = s.get<uint32_t>((size_t)n);
  uint32_t* k0 = s.get<uint32_t>((size_t)n);
  uint32_t* k1 = s.get<uint32_t>((size_t)n);
  uint32_t* v0 = s.get<uint32_t>((size_t)n);
  uint32_t* v1 = s.get<uint32_t>((size_t)n);
  PDX_SCRATCH_CHECK(s);
  PDX_TRY(pdx_groupby_group_ids(gb, ids, stream));
  hipLaunchKernelGGL(k_iota_rows, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, rows, n);
  PDX_LAUNCH_CHECK();
  *ks = ids;
  *vs = rows;
  if (gb->mode == 0 && G > 1) {  // (segments mode: the rows are grouped as they stand)
    const int bits = std::max(1, ilog2((uint64_t)G));
    PDX_TRY((radix_sort_pairs<uint32_t>(ids, rows, k0, v0, k1, v1, n, bits, ks, vs, true, s, st)));
  }
  return PDX_OK;
}
__global__ void k_seg_sizes(const uint32_t* __restrict__ seg_start, int64_t G, long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += stride) out[g] = (long long)seg_start[g + 1] - (long long)seg_start[g];
}
// sizes[g] = the distance between the first positions of the ids g and g + 1 in the sorted ids
__global__ void k_sorted_id_sizes(const uint32_t* __restrict__ sorted_ids, int64_t n, int64_t G, long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += stride) {
    int64_t bound[2];
    for (int k = 0; k < 2; ++k) {
      int64_t lo = 0, hi = n;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sorted_ids[mid] < g + k) lo = mid + 1;
        else hi = mid;
      }
      bound[k] = lo;
    }
    out[g] = bound[1] - bound[0];
  }
}
}  // namespace pdx

extern "C" {
// Grouper::MakeGroupings (src/dataframe.cpp:1546, 1562): the rows of every group, ascending, groups in group-id order
int pdx_groupby_groupings(pdx_groupby* gb, int64_t* out_rows, int64_t* out_offsets, void* stream) {
  if (!gb || !out_rows || !out_offsets) return fail(PDX_INVALID, "pdx_groupby_groupings: null argument");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);
  const int64_t n = gb->n, G = gb->G;
  if (n == 0) {
    PDX_HIP(hipMemsetAsync(out_offsets, 0, sizeof(int64_t) * (size_t)(G + 1), st));
    PDX_HIP(hipStreamSynchronize(st));
    return PDX_OK;
  }
  Scratch s;
  const uint32_t* ks = nullptr;
  const uint32_t* vs = nullptr;
  PDX_TRY(sort_rows_by_group(gb, &ks, &vs, s, stream, st));
  hipLaunchKernelGGL(k_groupings_finish, dim3(grid_for(n + G + 1, 256, 4)), dim3(256), 0, st, ks, vs, n, G, out_rows, out_offsets);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

// Rows per group, group-id order.  The handle keeps them once known (the COUNT of a column without nulls leaves them there and reads them
// from there): from the segment boundaries (resample / downsample / sorted keys); else through that same COUNT -- the LDS accumulators of
// gb_acc.hpp over the handle's slots, which reads no value column; else (few rows, or slots that do not fit LDS) from the rows sorted by
// group id, as pdx_groupby_groupings sorts them.
int pdx_groupby_sizes(pdx_groupby* gb, int64_t* out_sizes, void* stream) {
  if (!gb || !out_sizes) return fail(PDX_INVALID, "pdx_groupby_sizes: null argument");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);
  const int64_t n = gb->n, G = gb->G;
  if (G == 0) return PDX_OK;
  Scratch s;
  if (!gb->sizes_ready) {
    long long* sizes = acc_sizes_cache(gb);
    if (!sizes) return PDX_OOM;
    const AccTuning at = AccTuning::read();
    const AccGeom ag = acc_geometry(gb, false, kAccCnt, false, at);
    if (gb->mode != 0 && gb->seg_start) {
      hipLaunchKernelGGL(k_seg_sizes, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, gb->seg_start, G, sizes);
      PDX_LAUNCH_CHECK();
      gb->sizes_ready = true;
    } else if (ag.ok) {
      pdx_column rows_only{};  // a column without nulls: COUNT touches the handle's slots alone, never the values
      rows_only.dtype = PDX_INT64;
      rows_only.length = n;
      rows_only.values = gb->uniques;
      SegOut oo{};
      oo.count = s.get<long long>((size_t)G);
      PDX_SCRATCH_CHECK(s);
      PDX_TRY(reduce_acc(gb, ag, &rows_only, oo, nullptr, at, s, st, nullptr));  // (leaves the counts in gb->sizes)
    } else if (n == 0) {
      PDX_HIP(hipMemsetAsync(sizes, 0, (size_t)G * sizeof(long long), st));
      gb->sizes_ready = true;
    } else {
      const uint32_t* ks = nullptr;
      const uint32_t* vs = nullptr;
      PDX_TRY(sort_rows_by_group(gb, &ks, &vs, s, stream, st));
      hipLaunchKernelGGL(k_sorted_id_sizes, dim3(grid_for(G, 256)), dim3(256), 0, st, ks, n, G, sizes);
      PDX_LAUNCH_CHECK();
      gb->sizes_ready = true;
    }
  }
  PDX_HIP(hipMemcpyAsync(out_sizes, gb->sizes, (size_t)G * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- bound columns: layouts (and cached results) kept in the handle
namespace pdx {
static GroupedLayout* find_bound(pdx_groupby* gb, const pdx_column* values) {
  const void* vv = validity_or_null(values);
  for (auto& b : gb->bound)
    if (b->values == values->values && b->offset == values->offset && b->dtype == values->dtype && b->validity == vv) {
      b->last_use = ++gb->use_clock;
      return b.get();
    }
  return nullptr;
}
static size_t bind_limit_bytes(const pdx_groupby* gb) {
  if (gb->bind_limit) return gb->bind_limit;
  if (const char* e = getenv("PDX_BIND_MAX_BYTES")) return (size_t)atoll(e);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return (size_t)64 << 30;
  }
  return total_b / 4;
}
// least recently used layouts go first until the bound set fits the limit (the newest one always stays)
static void enforce_bind_limit(pdx_groupby* gb, const GroupedLayout* keep) {
  const size_t limit = bind_limit_bytes(gb);
  for (;;) {
    size_t total = 0;
    for (auto& b : gb->bound) total += b->bytes;
    if (total <= limit || gb->bound.size() <= 1) return;
    size_t victim = gb->bound.size();
    for (size_t i = 0; i < gb->bound.size(); ++i)
      if (gb->bound[i].get() != keep && (victim == gb->bound.size() || gb->bound[i]->last_use < gb->bound[victim]->last_use)) victim = i;
    if (victim == gb->bound.size()) return;
    gb->bound[victim]->stream = gb->stream;
    gb->bound.erase(gb->bound.begin() + (long)victim);
  }
}

#include "gb_agg.hpp"
}  // namespace pdx

extern "C" {

int pdx_groupby_bind(pdx_groupby* gb, const pdx_column* values, void* stream) {
  if (!gb) return fail(PDX_INVALID, "pdx_groupby_bind: null handle");
  PDX_TRY(check_column(values, "pdx_groupby_bind"));
  if (values->length != gb->n) return fail(PDX_INVALID, "pdx_groupby_bind: values length differs from the grouped key length");
  if (values->dtype != PDX_FLOAT64 && values->dtype != PDX_INT64)
    return fail(PDX_NOT_IMPLEMENTED, "pdx_groupby_bind: values must be int64 or float64 (boolean columns are order-free: nothing to keep)");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);
  if (find_bound(gb, values)) return PDX_OK;
  std::unique_ptr<GroupedLayout> L(new GroupedLayout());
  L->bound = true;
  L->last_use = ++gb->use_clock;
  // registration only: the first pdx_groupby_agg of the column builds the layout ITS kinds need (the fused form for the standard
  // kinds, the fully sorted form for product / first / last), later calls reuse it
  L->values = values->values;
  L->validity = validity_or_null(values);
  L->offset = values->offset;
  L->dtype = values->dtype;
  L->stream = st;
  gb->bound.push_back(std::move(L));
  enforce_bind_limit(gb, gb->bound.back().get());
  return PDX_OK;
}
int pdx_groupby_unbind(pdx_groupby* gb, const pdx_column* values) {
  if (!gb) return fail(PDX_INVALID, "pdx_groupby_unbind: null handle");
  for (auto& b : gb->bound) b->stream = gb->stream;
  if (!values) {
    gb->bound.clear();
    return PDX_OK;
  }
  const void* vv = validity_or_null(values);
  for (size_t i = 0; i < gb->bound.size(); ++i)
    if (gb->bound[i]->values == values->values && gb->bound[i]->offset == values->offset && gb->bound[i]->dtype == values->dtype &&
        gb->bound[i]->validity == vv) {
      gb->bound.erase(gb->bound.begin() + (long)i);
      break;
    }
  return PDX_OK;
}
int pdx_groupby_bind_limit(pdx_groupby* gb, size_t max_bytes) {
  if (!gb) return fail(PDX_INVALID, "pdx_groupby_bind_limit: null handle");
  gb->bind_limit = max_bytes;
  enforce_bind_limit(gb, nullptr);
  return PDX_OK;
}
int64_t pdx_groupby_bound_bytes(const pdx_groupby* gb) {
  if (!gb) return -1;
  size_t total = 0;
  for (auto& b : gb->bound) total += b->bytes;
  return (int64_t)total;
}
int pdx_groupby_last_plan(const pdx_groupby* gb, char* buf, size_t buf_len) {
  if (!gb || !buf || buf_len == 0) return fail(PDX_INVALID, "pdx_groupby_last_plan: null argument");
  if (gb->last_plan.size() + 1 > buf_len) return fail(PDX_INVALID, "pdx_groupby_last_plan: buffer too small");
  memcpy(buf, gb->last_plan.c_str(), gb->last_plan.size() + 1);
  return PDX_OK;
}

// Stage 1: the grouped layout of the value column (build_layout, gb_layout.hpp; a bound column brings its own); stage 2: the reducers
// over it (gb_agg.hpp).  Outputs are valid on return.
int pdx_groupby_agg(pdx_groupby* gb, const pdx_column* values, const int* kinds, int nk, pdx_mut_column* outs, void* stream) {
  if (!gb || !kinds || !outs || nk <= 0) return fail(PDX_INVALID, "pdx_groupby_agg: null argument");
  PDX_TRY(check_column(values, "pdx_groupby_agg"));
  if (values->length != gb->n) return fail(PDX_INVALID, "pdx_groupby_agg: values length differs from the grouped key length");
  // all / any / count_distinct (and boolean values) are order-free: they live in groupby_extra.hip and come back here for the
  // standard kinds named in the same request
  bool extra = values->dtype == PDX_BOOL;
  for (int k = 0; k < nk; ++k) extra = extra || kinds[k] == PDX_AGG_ALL || kinds[k] == PDX_AGG_ANY || kinds[k] == PDX_AGG_COUNT_DISTINCT;
  if (extra) return groupby_agg_extra(gb, values, kinds, nk, outs, stream);
  if (values->dtype != PDX_FLOAT64 && values->dtype != PDX_INT64) return fail(PDX_NOT_IMPLEMENTED, "pdx_groupby_agg: values must be int64 or float64");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);  // ordered behind the handle's creation; frees of its blocks are ordered behind this stream
  AggRequest rq;
  PDX_TRY(parse_agg_request(gb, values, kinds, nk, outs, &rq));
  if (gb->G == 0) return PDX_OK;
  const AggTuning t = AggTuning::read();
  const AccTuning at = AccTuning::read();
  GroupedLayout local;
  GroupedLayout* bound = find_bound(gb, values);
  Scratch s;  // (declared after `local`: scratch goes back to the pool first)
  AggCtx c{gb, values, validity_or_null(values), bound ? *bound : local, t, at, s, st, bound != nullptr};
  const size_t bytes_before = c.L.bytes;
  PDX_TRY(choose_reducer(c, rq));
  if (rq.want_std5) PDX_TRY(c.bound ? agg_std_bound(c, rq) : agg_std_unbound(c, rq));
  if (rq.var_out || rq.std_out) PDX_TRY(agg_variance(c, rq));
  if (rq.prod_out || rq.first_out || rq.last_out) PDX_TRY(agg_product_first_last(c, rq));
  gb->last_plan = compose_plan(c);
  if (c.bound && c.L.bytes != bytes_before) enforce_bind_limit(gb, &c.L);
  PDX_HIP(hipStreamSynchronize(st));  // outputs are valid on return; scratch and a local layout go back to the pool on exit
  return PDX_OK;
}


// adjustDatesAnchored + date_range (src/resample.cpp:85-178, src/core.cpp:308-331), tz == "": the first bin edge and the number of bins
// of an axis whose smallest / largest timestamps are tmin / tmax.  Host arithmetic only (also used by the sharded resample, where
// every rank must bin on the WHOLE axis' grid).
int pdx_resample_grid(int64_t tmin, int64_t tmax, int64_t freq_ns, int closed_right, int origin_type, int64_t origin_custom_ns, int64_t offset_ns,
                      int64_t* first_edge, int64_t* num_bins) {
  if (!first_edge || !num_bins) return fail(PDX_INVALID, "pdx_resample_grid: null output");
  if (freq_ns <= 0) return fail(PDX_INVALID, "FREQ must be positive");
  auto floor_div = [](long long a, long long b) { long long q = a / b, r = a % b; return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q; };
  const long long day = 86400000000000LL;
  long long first = tmin, last = tmax, origin = 0;
  switch (origin_type & ~PDX_ORIGIN_SHARD) {
    case PDX_ORIGIN_EPOCH: origin = 0; break;
    case PDX_ORIGIN_START_DAY: origin = floor_div(first, day) * day; break;
    case PDX_ORIGIN_START: origin = first; break;
    case PDX_ORIGIN_END: origin = last; break;
    case PDX_ORIGIN_END_DAY: origin = floor_div(last, day) * day; break;
    default: origin = origin_custom_ns; break;
  }
  origin += offset_ns;
  long long foffset = (first - origin) % freq_ns, loffset = (last - origin) % freq_ns;
  if (closed_right) {
    if (foffset > 0) first -= foffset; else first -= freq_ns;
    if (loffset > 0) last += freq_ns - loffset;
  } else {
    if (foffset > 0) first -= foffset;
    if (loffset > 0) last += freq_ns - loffset; else last += freq_ns;
  }
  if (first >= last) return fail(PDX_INVALID, "start date has to be less than end date");
  long long nedges = (last - first) / freq_ns + 1;  // date_range: first + k*freq <= last (src/core.cpp:308-331)
  long long last_edge = first + (nedges - 1) * freq_ns;
  if (tmin < first) return fail(PDX_INVALID, "Values falls before first bin");
  if (tmax > last_edge) return fail(PDX_INVALID, "Values falls after last bin");
  *first_edge = first;
  *num_bins = nedges - 1;
  return PDX_OK;
}

int pdx_resample_create(const pdx_column* ts, int64_t freq_ns, int closed_right, int label_right, int origin_type,
                        int64_t origin_custom_ns, int64_t offset_ns, void* stream, pdx_groupby** out) {
  PDX_TRY(check_column(ts, "pdx_resample_create"));
  if (!out) return fail(PDX_INVALID, "pdx_resample_create: null output");
  if (ts->dtype != PDX_TIMESTAMP_NS && ts->dtype != PDX_INT64) return fail(PDX_INVALID, "axis must be a TimestampArray");
  if (validity_or_null(ts)) return fail(PDX_NOT_IMPLEMENTED, "pdx_resample_create: null timestamps are not supported");
  if (freq_ns <= 0) return fail(PDX_INVALID, "FREQ must be positive");
  const int64_t n = ts->length;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_resample_create: more than 2^31-1 rows per call is not supported yet");
  hipStream_t st = as_stream(stream);
  std::unique_ptr<pdx_groupby> owner(new pdx_groupby());  // released into *out on success
  owner->stream = st;
  pdx_groupby* gb = owner.get();
  gb->mode = 1;
  gb->resample = true;
  gb->n = n;
  gb->key_dtype = PDX_TIMESTAMP_NS;
  *out = nullptr;
  if (n == 0) {
    *out = owner.release();
    return PDX_OK;
  }
  Scratch s;
  const long long* t = static_cast<const long long*>(ts->values) + ts->offset;
  unsigned int* bad = s.get<unsigned int>(1);
  if (s.failed) return PDX_OOM;
  hipMemsetAsync(bad, 0, sizeof(unsigned int), st);
  {
    PDX_PROFILE("resample_check_sorted", st);
    hipLaunchKernelGGL(k_check_sorted, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, t, n, bad);
  }
  // sorted input: MinMax (src/resample.cpp:223) is the first and the last timestamp
  long long mn = 0, mx = 0;
  unsigned int hbad = 0;
  int rc = PDX_OK;
  {
    hipError_t e = hipMemcpyAsync(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&mn, t, sizeof(mn), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&mx, t + (n - 1), sizeof(mx), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = hip_fail(e, "pdx_resample_create");
  }
  if (rc != PDX_OK) return rc;
  if (hbad) return fail(PDX_INVALID, "pdx_resample_create: timestamps must be sorted ascending");
  const bool is_shard = (origin_type & PDX_ORIGIN_SHARD) != 0;
  origin_type &= ~PDX_ORIGIN_SHARD;
  int64_t first_edge = 0, num_bins = 0;
  PDX_TRY(pdx_resample_grid(mn, mx, freq_ns, closed_right, origin_type, origin_custom_ns, offset_ns, &first_edge, &num_bins));
  const long long first = first_edge, nbins = num_bins;
  if (n < nbins && !is_shard) return fail(PDX_INVALID, "upSampling is not implemented.");  // GroupInfo::upsampling, src/resample.h:14-17
  gb->bin = BinParams{t, first, freq_ns, 1.0 / (double)freq_ns, closed_right};
  gb->label_base = first + (label_right ? freq_ns : 0);
  // non-empty bins: boundaries where the bin index changes (timestamps are sorted)
  int64_t maxg = std::min<int64_t>(n, nbins);
  gb->seg_start = gb->own<uint32_t>((size_t)maxg + 1);
  gb->uniques = gb->own<int64_t>((size_t)maxg);
  gb->first_rows = gb->own<int64_t>((size_t)maxg);
  gb->unique_ok = gb->own<uint8_t>((size_t)maxg);
  if (!gb->seg_start || !gb->uniques || !gb->first_rows || !gb->unique_ok) return PDX_OOM;
  int64_t G = 0;
  {
    PDX_PROFILE("resample_bins", st);
    if (nbins * 16 <= n) {
      // many rows per bin: binary-search every edge (nbins * log n reads) instead of evaluating the bin of every row
      uint32_t* lb = s.get<uint32_t>((size_t)nbins + 1);
      if (s.failed) return PDX_OOM;
      hipLaunchKernelGGL(k_bin_lower_bounds, dim3(grid_for(nbins + 1, 256)), dim3(256), 0, st, gb->bin, n, (int64_t)nbins, mn, mx, lb);
      rc = compact_indices((int64_t)nbins, NonEmptyBinPred{lb}, NonEmptyBinEmit{lb, gb->label_base, freq_ns, gb->seg_start, gb->uniques, gb->first_rows},
                           &G, s, st);
    } else {
      rc = compact_indices(n, BinStartPred{gb->bin}, BinStartEmit{gb->bin, gb->label_base, gb->seg_start, gb->uniques, gb->first_rows}, &G, s, st);
    }
  }
  if (rc != PDX_OK) return rc;
  gb->G = G;
  hipLaunchKernelGGL(k_set_last, dim3(1), dim3(64), 0, st, gb->seg_start, G, (uint32_t)n);
  hipMemsetAsync(gb->unique_ok, 1, (size_t)G, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "pdx_resample_create");
  *out = owner.release();
  return PDX_OK;
}

// DataFrame::downsample (reference src/dataframe.cpp:1265-1290): Ceil/FloorTemporal of the index, optionally one day less, then a
// GroupBy keyed on the rounded index.  On a sorted axis the rounded labels are (almost always) non-decreasing, so the groups are
// runs of equal labels: ONE pass over the timestamps rounds each row in registers, marks the run starts and proves the order --
// the rounded column is never written or hashed (8 B/row instead of 16 + the dictionary build).  Anything else (nulls, an unsorted
// axis, a calendar-origin ceil that steps back at an origin) goes through pdx_round_temporal + pdx_groupby_create as before.
int pdx_downsample_create(const pdx_column* ts, int64_t multiple, int unit, int ceil_mode, int week_starts_monday, int calendar_based_origin,
                          int64_t label_shift_ns, void* stream, pdx_groupby** out) {
  PDX_TRY(check_column(ts, "pdx_downsample_create"));
  if (!out) return fail(PDX_INVALID, "pdx_downsample_create: null output");
  if (ts->dtype != PDX_TIMESTAMP_NS) return fail(PDX_INVALID, "pdx_downsample_create: index must be PDX_TIMESTAMP_NS");
  RoundParams q{};
  int mode = 0;
  PDX_TRY(make_round_params(multiple, unit, week_starts_monday, calendar_based_origin, &q, &mode, "pdx_downsample_create"));
  const int64_t n = ts->length;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_downsample_create: more than 2^31-1 rows per call is not supported yet");
  hipStream_t st = as_stream(stream);
  *out = nullptr;
  if (CreateTuning::read().sorted && n >= 1 && !validity_or_null(ts)) {
    std::unique_ptr<pdx_groupby> owner(new pdx_groupby());
    owner->stream = st;
    pdx_groupby* gb = owner.get();
    gb->n = n;
    gb->key_dtype = PDX_TIMESTAMP_NS;
    Scratch s;
    const long long* t = static_cast<const long long*>(ts->values) + ts->offset;
    bool done = false;
    int rc = PDX_OK;
    rc = with_digit_bits<0, 9>(mode, [&](auto m) {  // (the rounding mode is a template parameter too)
      return ceil_mode ? build_label_runs(gb, n, RoundLabel<m(), true>{t, q}, label_shift_ns, s, st, &done)
                       : build_label_runs(gb, n, RoundLabel<m(), false>{t, q}, label_shift_ns, s, st, &done);
    });
    if (rc != PDX_OK) return rc;
    if (done) {
      *out = owner.release();
      return PDX_OK;
    }
  }
  // the general way: the rounded column, then a dictionary of it (first-occurrence order; nulls form their own group)
  const bool has_nulls = validity_or_null(ts) != nullptr;
  void* binned_vals = pool_alloc((size_t)(n ? n : 1) * sizeof(int64_t));
  void* binned_valid = has_nulls ? pool_alloc((size_t)(n + 7) / 8 + 8) : nullptr;
  if (!binned_vals || (has_nulls && !binned_valid)) {
    if (binned_vals) pool_free(binned_vals);
    if (binned_valid) pool_free(binned_valid);
    return PDX_OOM;
  }
  pdx_mut_column mb{};
  mb.dtype = PDX_TIMESTAMP_NS;
  mb.length = n;
  mb.values = binned_vals;
  mb.validity = binned_valid;
  int rc = pdx_round_temporal(ceil_mode, ts, multiple, unit, week_starts_monday, calendar_based_origin, &mb, stream);
  if (rc == PDX_OK) {
    pdx_column cb{};
    cb.dtype = PDX_TIMESTAMP_NS;
    cb.length = n;
    cb.values = binned_vals;
    cb.validity = binned_valid;
    cb.offset = 0;
    cb.null_count = has_nulls ? -1 : 0;
    rc = pdx_groupby_create(&cb, stream, out);
  }
  if (rc == PDX_OK && *out && label_shift_ns != 0 && (*out)->G > 0) {
    hipLaunchKernelGGL(k_shift_labels, dim3(grid_for((*out)->G, 256)), dim3(256), 0, st, (*out)->uniques, (*out)->G, (long long)label_shift_ns);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = fail(PDX_DEVICE, "pdx_downsample_create: label shift failed");
  }
  {
    StreamNote note(st);
    pool_free(binned_vals);
    if (binned_valid) pool_free(binned_valid);
  }
  if (rc != PDX_OK && *out) {
    pdx_groupby_destroy(*out);
    *out = nullptr;
  }
  return rc;
}

int pdx_resample_row_labels(pdx_groupby* gb, int64_t* out_labels, void* stream) {
  if (!gb || !out_labels) return fail(PDX_INVALID, "pdx_resample_row_labels: null argument");
  if (!gb->resample) return fail(PDX_INVALID, "pdx_resample_row_labels: handle was not created by pdx_resample_create");
  hipStream_t st = as_stream(stream);
  gb->use_on(st);  // ordered behind the handle's creation; frees of its blocks are ordered behind this stream
  if (gb->n) hipLaunchKernelGGL(k_row_labels, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, st, gb->bin, gb->label_base, gb->n, out_labels);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

}  // extern "C"

#include "gb_partial_tree.hpp"

#ifdef PDX_FLR_TIMING
// diagnostic build only: read (and clear) the dense fused kernel's per-phase cycle sums
extern "C" int pdx_debug_flr_cycles(unsigned long long* out24, int reset) {
  if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(pdx::g_flr_cycles), sizeof(unsigned long long) * 24) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[24] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(pdx::g_flr_cycles), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
#endif
