// quantile.hip -- exact quantiles for gfx950: pdx_quantile (whole column, radix select) and pdx_groupby_quantile.
//
// Replaces CallFunction("quantile", {array}, QuantileOptions{q, interpolation, skip_nulls, min_count}) reached from NDFrame::quantile
// (reference src/ndframe.h:259-263, src/ndframe.cpp:202-212), DataFrame::describe (src/dataframe.cpp:983-1030) and, per group,
// GroupBy::quantile (src/group_by.h:123-124, src/dataframe.cpp:1867-1931).
//
// Whole column: a quantile needs the values at ranks lo and lo + 1 of the sorted valid non-NaN values, not the order of the rest.
//   level 0  k_q_hist     one streaming read of the column: value -> order-preserving key (quantile.hpp), 2048-bin LDS histogram of the
//                         key's top 11 bits per workgroup (hot digits counted once per wave), written as per-workgroup partials;
//                         smallest / largest key and valid rows by one atomic per workgroup;
//            k_q_fold     partials -> one 64-bit histogram (a few dozen adds per bin and slice, no per-wave global atomics)
//            host         n = sum of the bins; every rank of every q is located in its bin: one histogram read serves all of them
//            k_q_offsets  per selected bin: exclusive scan of the workgroups' partial counts = where each workgroup writes
//            k_q_compact  second read: the keys of the selected bins are copied out, one segment per bin
//   level k  the same three steps over the segments (flat grid over all of them) on the next 11 key bits.
// A bin of at most 4096 keys is finished by one workgroup (bitonic sort in LDS, k_q_small); a segment whose smallest and largest key
// are equal is finished at once; a bin that holds its whole segment is not copied (the next level reads the same keys); after the
// last digit every key of a bin is known.  So at most 6 (32-bit keys: 3) levels are taken for ANY input, and every row count is 64 bits.
// The interpolation runs on the host from the (at most two) selected values per q, with Arrow's expressions (-ffp-contract=off).
//
// Group form: pdx_argsort of the values (numbers ascending, then NaN, then nulls; stable), one stable radix sort of that row list by group
// id, then one lane per group counts the group's numbers by bisection and interpolates with unfused multiplies and adds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#include "colview.hpp"
#include "group_order.hpp"
#include "quantile.hpp"
#include "radix_sort.hpp"

namespace pdx {

// ---------------------------------------------------------------- device helpers
template <typename T, bool L0>
__device__ __forceinline__ bool q_load(const void* src, uint64_t i, const uint8_t* valid, int64_t voff, typename QKey<T>::K* k, bool* row_valid) {
  if constexpr (L0) {
    *row_valid = !valid || bit_get(valid, voff + (int64_t)i);
    if (!*row_valid) return false;
    return QKey<T>::key(static_cast<const T*>(src)[i], k);
  } else {
    *row_valid = true;
    *k = static_cast<const typename QKey<T>::K*>(src)[i];
    return true;
  }
}
__device__ __forceinline__ int q_find_seg(const QSeg* segs, int nseg, uint32_t block) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {  // the last segment whose first workgroup is <= block
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_block <= block) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// wave_hist_add (radix_sort.hpp) for a wave whose lanes take part or not from step to step: every lane calls it, so the candidate digit
// stays the same in all of them
__device__ __forceinline__ void q_hist_add(uint32_t* h, uint32_t d, bool ok, uint32_t& cand, int lane) {
  const unsigned long long m = __ballot(ok && d == cand);
  const int shared = __popcll(m);
  if (shared >= 8) {
    if (ok) {
      if (d != cand) atomicAdd(&h[d], 1u);
      else if (lane == __ffsll((long long)m) - 1) atomicAdd(&h[d], (uint32_t)shared);
    }
  } else {
    if (ok) atomicAdd(&h[d], 1u);
    const unsigned long long a = __ballot(ok);
    if (a) cand = (uint32_t)__shfl((int)d, __ffsll((long long)a) - 1, 64);
  }
}

constexpr int kQUnroll = 4;

template <typename T, bool L0>
__global__ void __launch_bounds__(kQBlock) k_q_hist(const QSeg* __restrict__ segs, int nseg, const uint8_t* __restrict__ valid, int64_t voff, int shift,
                                                    uint32_t mask, uint32_t* __restrict__ partial /* [blocks][kQBins] */,
                                                    unsigned long long* __restrict__ seg_minmax /* [2 nseg] */,
                                                    unsigned long long* __restrict__ valid_total) {
  using K = typename QKey<T>::K;
  __shared__ uint32_t h[kQBins];
  __shared__ unsigned long long red[3][kQBlock / 64];
  for (int d = threadIdx.x; d < kQBins; d += kQBlock) h[d] = 0;
  __syncthreads();
  const int seg = q_find_seg(segs, nseg, blockIdx.x);
  const QSeg sg = segs[seg];
  const uint64_t begin = (uint64_t)(blockIdx.x - sg.first_block) * sg.chunk;
  const uint64_t end = begin + sg.chunk < sg.size ? begin + sg.chunk : sg.size;
  const int lane = threadIdx.x & 63;
  uint32_t cand = 0xFFFFFFFFu;
  unsigned long long mn = ~0ull, mx = 0ull, vc = 0;
  for (uint64_t i0 = begin; i0 < end; i0 += (uint64_t)kQBlock * kQUnroll) {  // (uniform trip count: q_hist_add is called by whole waves)
    K k[kQUnroll];
    bool ok[kQUnroll];
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      const uint64_t i = i0 + (uint64_t)u * kQBlock + threadIdx.x;
      bool rv = false;
      k[u] = 0;
      ok[u] = i < end && q_load<T, L0>(sg.src, i, valid, voff, &k[u], &rv);
      if (L0 && i < end && rv) ++vc;
    }
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      q_hist_add(h, (uint32_t)(k[u] >> shift) & mask, ok[u], cand, lane);
      if (ok[u]) {
        mn = (unsigned long long)k[u] < mn ? (unsigned long long)k[u] : mn;
        mx = (unsigned long long)k[u] > mx ? (unsigned long long)k[u] : mx;
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long omn = __shfl_down(mn, d, 64), omx = __shfl_down(mx, d, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    vc += __shfl_down(vc, d, 64);
  }
  if (lane == 0) {
    red[0][threadIdx.x >> 6] = mn;
    red[1][threadIdx.x >> 6] = mx;
    red[2][threadIdx.x >> 6] = vc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // one atomic per WORKGROUP and address (<= ~2048 per segment)
    for (int w = 1; w < kQBlock / 64; ++w) {
      mn = red[0][w] < mn ? red[0][w] : mn;
      mx = red[1][w] > mx ? red[1][w] : mx;
      vc += red[2][w];
    }
    if (mn <= mx) {
      atomicMin(&seg_minmax[2 * seg], mn);
      atomicMax(&seg_minmax[2 * seg + 1], mx);
    }
    if (L0 && vc) atomicAdd(valid_total, vc);
  }
  for (int d = threadIdx.x; d < kQBins; d += kQBlock) partial[(uint64_t)blockIdx.x * kQBins + d] = h[d];
}

constexpr int kQFoldSlice = 32;  // workgroup partials summed by one thread before its one atomic per bin
__global__ void __launch_bounds__(kQBlock) k_q_fold(const QSeg* __restrict__ segs, int nseg, const uint32_t* __restrict__ partial, uint32_t total_blocks,
                                                    unsigned long long* __restrict__ hist /* [nseg][kQBins] */) {
  const uint32_t bin = blockIdx.x * kQBlock + threadIdx.x;
  const uint32_t b0 = blockIdx.y * kQFoldSlice;
  const uint32_t b1 = b0 + kQFoldSlice < total_blocks ? b0 + kQFoldSlice : total_blocks;
  int seg = q_find_seg(segs, nseg, b0);
  unsigned long long acc = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    while (b >= segs[seg].first_block + segs[seg].nblocks) {
      if (acc) atomicAdd(&hist[(uint64_t)seg * kQBins + bin], acc);
      acc = 0;
      ++seg;
    }
    acc += partial[(uint64_t)b * kQBins + bin];
  }
  if (acc) atomicAdd(&hist[(uint64_t)seg * kQBins + bin], acc);
}

// offsets[sel.base_index + b] = rows of the selected bin in the segment's workgroups before workgroup b
__global__ void __launch_bounds__(kQBlock) k_q_offsets(const QSeg* __restrict__ segs, const QSel* __restrict__ sels, const uint32_t* __restrict__ partial,
                                                       unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long wsum[kQBlock / 64];
  __shared__ unsigned long long carry_s;
  const QSel sel = sels[blockIdx.x];
  const QSeg sg = segs[sel.seg];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < sg.nblocks; b0 += kQBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const unsigned long long v = b < sg.nblocks ? partial[(uint64_t)(sg.first_block + b) * kQBins + sel.digit] : 0ull;
    unsigned long long inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (b < sg.nblocks) offsets[sel.base_index + b] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == kQBlock - 1) carry_s = before + inc;
    __syncthreads();
  }
}

template <typename T, bool L0>
__global__ void __launch_bounds__(kQBlock) k_q_compact(const QSeg* __restrict__ segs, int nseg, const uint8_t* __restrict__ valid, int64_t voff, int shift,
                                                       uint32_t mask, const QSel* __restrict__ sels, const unsigned long long* __restrict__ offsets) {
  using K = typename QKey<T>::K;
  __shared__ int16_t slot_of[kQBins];
  __shared__ uint32_t cursor[kQMaxTargets];
  __shared__ unsigned long long base[kQMaxTargets];
  __shared__ K* dst[kQMaxTargets];
  const int seg = q_find_seg(segs, nseg, blockIdx.x);
  const QSeg sg = segs[seg];
  const int nsel = (int)(sg.sel_end - sg.sel_begin);
  if (nsel == 0) return;  // nothing of this segment is copied (finished, or handed on as it stands)
  const uint32_t local = blockIdx.x - sg.first_block;
  for (int d = threadIdx.x; d < kQBins; d += kQBlock) slot_of[d] = -1;
  __syncthreads();
  for (int j = threadIdx.x; j < nsel; j += kQBlock) {
    const QSel sel = sels[sg.sel_begin + j];
    slot_of[sel.digit] = (int16_t)j;
    cursor[j] = 0;
    base[j] = offsets[sel.base_index + local];
    dst[j] = static_cast<K*>(sel.dst);
  }
  __syncthreads();
  const uint64_t begin = (uint64_t)local * sg.chunk;
  const uint64_t end = begin + sg.chunk < sg.size ? begin + sg.chunk : sg.size;
  const int lane = threadIdx.x & 63;
  const unsigned long long lt_mask = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (uint64_t i0 = begin; i0 < end; i0 += (uint64_t)kQBlock * kQUnroll) {
    K k[kQUnroll];
    int sl[kQUnroll];
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      const uint64_t i = i0 + (uint64_t)u * kQBlock + threadIdx.x;
      bool rv;
      k[u] = 0;
      const bool ok = i < end && q_load<T, L0>(sg.src, i, valid, voff, &k[u], &rv);
      sl[u] = ok ? (int)slot_of[(uint32_t)(k[u] >> shift) & mask] : -1;
    }
#pragma unroll
    for (int u = 0; u < kQUnroll; ++u) {
      // the lanes of a wave that go to the same bin take their places with ONE LDS add (a hot bin is most of the wave)
      bool pending = sl[u] >= 0;
      unsigned long long m = __ballot(pending);
      while (m) {
        const int leader = __ffsll((long long)m) - 1;
        const int lsl = __shfl(sl[u], leader, 64);
        const unsigned long long same = __ballot(pending && sl[u] == lsl);
        uint32_t pos = 0;
        if (lane == leader) pos = atomicAdd(&cursor[lsl], (uint32_t)__popcll(same));
        pos = (uint32_t)__shfl((int)pos, leader, 64);
        if (pending && sl[u] == lsl) {
          dst[lsl][base[lsl] + pos + (uint32_t)__popcll(same & lt_mask)] = k[u];
          pending = false;
        }
        m = __ballot(pending);
      }
    }
  }
}

// one workgroup sorts one small segment in LDS and reads off one rank
template <typename K>
__global__ void __launch_bounds__(kQBlock) k_q_small(const QPick* __restrict__ picks, QPicked* __restrict__ out) {
  __shared__ K s[kQSmall];
  const QPick p = picks[blockIdx.x];
  const K* src = static_cast<const K*>(p.src);
  const int m = (int)p.size;
  int P = 1;
  while (P < m) P <<= 1;
  for (int i = threadIdx.x; i < P; i += kQBlock) s[i] = i < m ? src[i] : (K)~(K)0;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += kQBlock) {
        const int x = i ^ j;
        if (x > i) {
          const K a = s[i], b = s[x];
          if ((a > b) == ((i & k) == 0)) {
            s[i] = b;
            s[x] = a;
          }
        }
      }
      __syncthreads();
    }
  if (threadIdx.x == 0) {
    const K key = s[p.rank];
    int lo = 0, hi = (int)p.rank;  // first position that holds `key`
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    out[blockIdx.x].key = (uint64_t)key;
    out[blockIdx.x].nth_equal = p.rank - (uint64_t)lo;
  }
}

// ---- which zero: -0.0 and 0.0 share a key; the result is the zero that comes first in pdx_argsort's stable order = row order
template <typename T>
__global__ void __launch_bounds__(kQBlock) k_q_zero_count(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, uint64_t n, uint64_t chunk,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long ws[kQBlock / 64];
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  const uint64_t end = begin + chunk < n ? begin + chunk : n;
  unsigned long long c = 0;
  for (uint64_t i = begin + threadIdx.x; i < end; i += kQBlock)
    if ((!valid || bit_get(valid, voff + (int64_t)i)) && v[i] == T(0)) ++c;
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
// workgroup p: the sign of the j-th zero (row order) of the rows [begin, end), which hold more than j zeros
struct QZeroPick {
  uint64_t begin, end, j;
};
template <typename T>
__global__ void __launch_bounds__(kQBlock) k_q_zero_pick(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff,
                                                         const QZeroPick* __restrict__ picks, uint32_t* __restrict__ negative) {
  __shared__ unsigned long long cnt[kQBlock];
  __shared__ int who;
  __shared__ unsigned long long rest;
  const uint64_t begin = picks[blockIdx.x].begin, end = picks[blockIdx.x].end, j = picks[blockIdx.x].j;
  const uint64_t per = (end - begin + kQBlock - 1) / kQBlock;
  const uint64_t b = begin + per * threadIdx.x < end ? begin + per * threadIdx.x : end;
  const uint64_t e = b + per < end ? b + per : end;
  unsigned long long c = 0;
  for (uint64_t i = b; i < e; ++i)
    if ((!valid || bit_get(valid, voff + (int64_t)i)) && v[i] == T(0)) ++c;
  cnt[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long r = j;
    int t = 0;
    while (t < kQBlock - 1 && r >= cnt[t]) r -= cnt[t++];
    who = t;
    rest = r;
  }
  __syncthreads();
  if ((int)threadIdx.x == who) {
    unsigned long long r = rest;
    for (uint64_t i = b; i < e; ++i)
      if ((!valid || bit_get(valid, voff + (int64_t)i)) && v[i] == T(0)) {
        if (r == 0) {
          negative[blockIdx.x] = __builtin_signbit((double)v[i]) ? 1u : 0u;
          return;
        }
        --r;
      }
  }
}

// ---------------------------------------------------------------- host: the select
template <typename K>
struct QTarget {
  uint64_t global_rank;
  int seg;        // index into the current level's segments (or -1: waiting for a small pick / done)
  uint64_t rank;  // inside that segment
  bool done;
  K key;
  uint64_t nth_equal;
  bool negative_zero;
};
template <typename K>
struct QHostSeg {
  const void* src;      // nullptr while the segment waits for the level's output buffer (in_newest)
  uint64_t size;
  K prefix;
  uint64_t out_offset;  // in_newest: where the segment starts in that buffer, in keys
  bool in_newest;
};

// Level 0 over the column, then whatever levels the ranks need.  make_ranks(n, valid_rows) is called once n is known (after the first
// histogram) and returns the distinct ranks wanted (an empty list ends the run); out: key, place among equal keys, sign of a zero.
template <typename T, typename MakeRanks>
static int q_select(const pdx_column* a, MakeRanks make_ranks, std::vector<QTarget<typename QKey<T>::K>>* out, hipStream_t st) {
  using K = typename QKey<T>::K;
  constexpr int kKeyBits = (int)sizeof(K) * 8;
  Scratch s;
  const uint8_t* valid = validity_or_null(a);
  const int64_t voff = a->offset;
  const T* values = static_cast<const T*>(a->values) + a->offset;
  std::vector<QHostSeg<K>> cur{{values, (uint64_t)a->length, (K)0, 0, false}};
  std::vector<QTarget<K>>& tg = *out;
  tg.clear();
  std::vector<QPick> picks;
  std::vector<int> pick_target;
  std::vector<uint64_t> pick_offset;  // where a pick's segment starts in the output buffer of the level that made it
  size_t picks_placed = 0;            // picks [0, picks_placed) already point into their buffers
  int shift = kKeyBits;
  bool level0 = true;
  PDX_PROFILE("quantile_select", st);
  while (!cur.empty()) {
    const int w = shift < kQBits ? shift : kQBits;
    shift -= w;
    const uint32_t mask = (1u << w) - 1u;
    const int nseg = (int)cur.size();
    std::vector<QSeg> hs((size_t)nseg);
    uint64_t total_blocks = 0;
    for (int i = 0; i < nseg; ++i) {
      QSeg& g = hs[i];
      g.src = cur[i].src;
      g.size = cur[i].size;
      g.chunk = std::max<uint64_t>(65536, (g.size + 2047) / 2048);
      g.nblocks = (uint32_t)((g.size + g.chunk - 1) / g.chunk);
      g.first_block = (uint32_t)total_blocks;
      g.sel_begin = g.sel_end = 0;
      total_blocks += g.nblocks;
    }
    QSeg* dsegs = s.get<QSeg>((size_t)nseg);
    uint32_t* partial = s.get<uint32_t>((size_t)total_blocks * kQBins);
    unsigned long long* hist = s.get<unsigned long long>((size_t)nseg * kQBins + 2 * (size_t)nseg + 1);
    PDX_SCRATCH_CHECK(s);
    unsigned long long* minmax = hist + (size_t)nseg * kQBins;
    unsigned long long* valid_total = minmax + 2 * (size_t)nseg;
    std::vector<unsigned long long> hh((size_t)nseg * kQBins + 2 * (size_t)nseg + 1, 0ull);
    for (int i = 0; i < nseg; ++i) hh[(size_t)nseg * kQBins + 2 * i] = ~0ull;
    PDX_HIP(hipMemcpyAsync(dsegs, hs.data(), sizeof(QSeg) * (size_t)nseg, hipMemcpyHostToDevice, st));
    PDX_HIP(hipMemcpyAsync(hist, hh.data(), sizeof(unsigned long long) * hh.size(), hipMemcpyHostToDevice, st));
    if (level0)
      hipLaunchKernelGGL((k_q_hist<T, true>), dim3((unsigned)total_blocks), dim3(kQBlock), 0, st, dsegs, nseg, valid, voff, shift, mask, partial, minmax, valid_total);
    else
      hipLaunchKernelGGL((k_q_hist<T, false>), dim3((unsigned)total_blocks), dim3(kQBlock), 0, st, dsegs, nseg, valid, voff, shift, mask, partial, minmax,
                         valid_total);
    hipLaunchKernelGGL(k_q_fold, dim3(kQBins / kQBlock, (unsigned)((total_blocks + kQFoldSlice - 1) / kQFoldSlice)), dim3(kQBlock), 0, st, dsegs, nseg, partial,
                       (uint32_t)total_blocks, hist);
    PDX_LAUNCH_CHECK();
    PDX_TRY(read_back(hh.data(), hist, sizeof(unsigned long long) * hh.size(), st));
    const unsigned long long* hmm = hh.data() + (size_t)nseg * kQBins;  // [2 sg], [2 sg + 1]: smallest / largest key of segment sg
    const size_t valid_total_index = (size_t)nseg * kQBins + 2 * (size_t)nseg;
    if (level0) {
      uint64_t n = 0;
      for (int d = 0; d < kQBins; ++d) n += hh[d];
      const uint64_t valid_rows = valid ? hh[valid_total_index] : (uint64_t)a->length;
      std::vector<uint64_t> ranks = make_ranks(n, valid_rows);
      if (ranks.empty()) return PDX_OK;
      if ((int)ranks.size() > kQMaxTargets) return fail(PDX_INVALID, "internal: too many ranks in one select");
      for (uint64_t r : ranks) tg.push_back(QTarget<K>{r, 0, r, false, (K)0, 0, false});
    }
    // every pending rank: its bin in its segment
    std::vector<QHostSeg<K>> next;
    std::vector<QSel> sels;
    std::vector<std::pair<int, uint64_t>> sel_out;  // per sel: (next segment or -1 for a small one, rows)
    uint64_t out_rows = 0, offsets_len = 0;
    for (int sgi = 0; sgi < nseg; ++sgi) {
      hs[sgi].sel_begin = (uint32_t)sels.size();
      const unsigned long long* h = hh.data() + (size_t)sgi * kQBins;
      std::map<uint32_t, int> bin_next;   // digit -> index in `next` (handed on or copied, large)
      std::map<uint32_t, uint64_t> bin_small;  // digit -> offset of its copy in this level's output (small)
      for (size_t t = 0; t < tg.size(); ++t) {
        QTarget<K>& x = tg[t];
        if (x.done || x.seg != sgi) continue;
        if (hmm[2 * sgi] == hmm[2 * sgi + 1]) {  // one distinct key in the whole segment
          x.done = true;
          x.key = (K)hmm[2 * sgi];
          x.nth_equal = x.rank;
          x.seg = -1;
          continue;
        }
        uint64_t cum = 0;
        uint32_t d = 0;
        for (; d < (uint32_t)kQBins; ++d) {
          if (x.rank < cum + h[d]) break;
          cum += h[d];
        }
        if (d == (uint32_t)kQBins) return fail(PDX_DEVICE, "pdx_quantile: a rank lies beyond its histogram");
        const uint64_t cnt = h[d], rank_in = x.rank - cum;
        const K prefix = (K)(cur[sgi].prefix | ((K)d << shift));
        if (shift == 0) {  // the last digit: the key is known
          x.done = true;
          x.key = prefix;
          x.nth_equal = rank_in;
          x.seg = -1;
          continue;
        }
        x.rank = rank_in;
        if (cnt <= (uint64_t)kQSmall) {
          auto it = bin_small.find(d);
          if (it == bin_small.end()) {
            it = bin_small.emplace(d, out_rows).first;
            sels.push_back(QSel{nullptr, offsets_len, (uint32_t)sgi, d});
            sel_out.emplace_back(-1, out_rows);
            out_rows += cnt;
            offsets_len += hs[sgi].nblocks;
          }
          x.seg = -1;
          picks.push_back(QPick{nullptr, cnt, rank_in});  // (src: once this level's output buffer exists)
          pick_target.push_back((int)t);
          pick_offset.push_back(it->second);
          continue;
        }
        auto it = bin_next.find(d);
        if (it == bin_next.end()) {
          it = bin_next.emplace(d, (int)next.size()).first;
          if (!level0 && cnt == cur[sgi].size) {
            next.push_back(QHostSeg<K>{cur[sgi].src, cnt, prefix, 0, false});  // the bin IS the segment: read it again, copy nothing
          } else {
            next.push_back(QHostSeg<K>{nullptr, cnt, prefix, out_rows, true});
            sels.push_back(QSel{nullptr, offsets_len, (uint32_t)sgi, d});
            sel_out.emplace_back(it->second, out_rows);
            out_rows += cnt;
            offsets_len += hs[sgi].nblocks;
          }
        }
        x.seg = it->second;
      }
      hs[sgi].sel_end = (uint32_t)sels.size();
      if ((int)(hs[sgi].sel_end - hs[sgi].sel_begin) > kQMaxTargets) return fail(PDX_INVALID, "internal: too many bins selected in one segment");
    }
    if (!sels.empty()) {
      K* outbuf = s.get<K>((size_t)out_rows);
      QSel* dsels = s.get<QSel>(sels.size());
      unsigned long long* offsets = s.get<unsigned long long>((size_t)offsets_len);
      PDX_SCRATCH_CHECK(s);
      for (size_t j = 0; j < sels.size(); ++j) sels[j].dst = outbuf + sel_out[j].second;
      for (auto& ns : next)
        if (ns.in_newest) {
          ns.src = outbuf + ns.out_offset;
          ns.in_newest = false;
        }
      for (; picks_placed < picks.size(); ++picks_placed) picks[picks_placed].src = outbuf + pick_offset[picks_placed];
      PDX_HIP(hipMemcpyAsync(dsegs, hs.data(), sizeof(QSeg) * (size_t)nseg, hipMemcpyHostToDevice, st));
      PDX_HIP(hipMemcpyAsync(dsels, sels.data(), sizeof(QSel) * sels.size(), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_q_offsets, dim3((unsigned)sels.size()), dim3(kQBlock), 0, st, dsegs, dsels, partial, offsets);
      if (level0)
        hipLaunchKernelGGL((k_q_compact<T, true>), dim3((unsigned)total_blocks), dim3(kQBlock), 0, st, dsegs, nseg, valid, voff, shift, mask, dsels, offsets);
      else
        hipLaunchKernelGGL((k_q_compact<T, false>), dim3((unsigned)total_blocks), dim3(kQBlock), 0, st, dsegs, nseg, valid, voff, shift, mask, dsels, offsets);
      PDX_LAUNCH_CHECK();
      // (hs / sels are pageable host memory: the copies above have been staged by the time the calls return)
    }
    // PDX_QUANTILE_TRACE=1 (diagnostic, tools/bench_quantile.py --trace): what this level read, kept and copied
    static const bool trace = [] { const char* e = getenv("PDX_QUANTILE_TRACE"); return e && atoi(e) > 0; }();
    if (trace) {
      uint64_t rows_in = 0, rows_on = 0;
      for (auto& c : cur) rows_in += c.size;
      for (auto& c : next) rows_on += c.size;
      fprintf(stderr, "pdx_quantile level shift=%d bits=%d: %d segment(s) %llu rows read, %zu bin(s) %llu rows copied, %zu segment(s) %llu rows go on, %zu small pick(s)\n",
              shift, w, nseg, (unsigned long long)rows_in, sels.size(), (unsigned long long)out_rows, next.size(), (unsigned long long)rows_on, picks.size());
    }
    cur.swap(next);
    level0 = false;
  }
  if (!picks.empty()) {
    QPick* dp = s.get<QPick>(picks.size());
    QPicked* dr = s.get<QPicked>(picks.size());
    PDX_SCRATCH_CHECK(s);
    std::vector<QPicked> hr(picks.size());
    PDX_HIP(hipMemcpyAsync(dp, picks.data(), sizeof(QPick) * picks.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_q_small<K>, dim3((unsigned)picks.size()), dim3(kQBlock), 0, st, dp, dr);
    PDX_LAUNCH_CHECK();
    PDX_TRY(read_back(hr.data(), dr, sizeof(QPicked) * picks.size(), st));
    for (size_t j = 0; j < picks.size(); ++j) {
      QTarget<K>& x = tg[(size_t)pick_target[j]];
      x.done = true;
      x.key = (K)hr[j].key;
      x.nth_equal = hr[j].nth_equal;
    }
  }
  for (auto& x : tg)
    if (!x.done) return fail(PDX_DEVICE, "pdx_quantile: a rank was left unresolved");
  if constexpr (QKey<T>::kFloat) {
    bool any_zero = false;
    for (auto& x : tg) any_zero = any_zero || x.key == QKey<T>::kZero;
    if (any_zero) {
      const uint64_t n = (uint64_t)a->length;
      const uint64_t chunk = std::max<uint64_t>(65536, (n + 2047) / 2048);
      const unsigned nb = (unsigned)((n + chunk - 1) / chunk);
      unsigned long long* counts = s.get<unsigned long long>(nb);
      PDX_SCRATCH_CHECK(s);
      hipLaunchKernelGGL(k_q_zero_count<T>, dim3(nb), dim3(kQBlock), 0, st, values, valid, voff, n, chunk, counts);
      PDX_LAUNCH_CHECK();
      std::vector<unsigned long long> hc(nb);
      PDX_TRY(read_back(hc.data(), counts, sizeof(unsigned long long) * nb, st));
      std::vector<QZeroPick> zp;  // every zero target: one launch, one copy back
      std::vector<size_t> zp_target;
      for (size_t t = 0; t < tg.size(); ++t) {
        if (tg[t].key != QKey<T>::kZero) continue;
        uint64_t j = tg[t].nth_equal;
        unsigned b = 0;
        while (b + 1 < nb && j >= hc[b]) j -= hc[b++];
        if (j >= hc[b]) return fail(PDX_DEVICE, "pdx_quantile: zero ranks do not add up");
        const uint64_t begin = (uint64_t)b * chunk;
        zp.push_back(QZeroPick{begin, std::min<uint64_t>(begin + chunk, n), j});
        zp_target.push_back(t);
      }
      QZeroPick* dzp = s.get<QZeroPick>(zp.size());
      uint32_t* neg = s.get<uint32_t>(zp.size());
      PDX_SCRATCH_CHECK(s);
      std::vector<uint32_t> hn(zp.size(), 0u);
      PDX_HIP(hipMemcpyAsync(dzp, zp.data(), sizeof(QZeroPick) * zp.size(), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_q_zero_pick<T>, dim3((unsigned)zp.size()), dim3(kQBlock), 0, st, values, valid, voff, dzp, neg);
      PDX_LAUNCH_CHECK();
      PDX_TRY(read_back(hn.data(), neg, sizeof(uint32_t) * zp.size(), st));
      for (size_t k = 0; k < zp.size(); ++k) tg[zp_target[k]].negative_zero = hn[k] != 0;
    }
  }
  return PDX_OK;
}

// ---------------------------------------------------------------- host: Arrow's interpolation (arrow/compute/kernels/aggregate_quantile.cc)
struct QRank {
  uint64_t lo, hi;
  double f;
};
static QRank q_rank(uint64_t n, double q) {
  const double index = (double)(n - 1) * q;
  QRank r;
  r.lo = (uint64_t)index;
  r.f = index - (double)r.lo;
  r.hi = r.f != 0.0 ? r.lo + 1 : r.lo;
  if (r.hi > n - 1) r.hi = n - 1;
  return r;
}
// the data point LOWER / HIGHER / NEAREST return
static uint64_t q_point(const QRank& r, int interp) {
  if (interp == PDX_INTERP_LOWER) return r.lo;
  if (interp == PDX_INTERP_HIGHER) return r.hi;
  if (r.f < 0.5) return r.lo;
  if (r.f > 0.5) return r.hi;
  return r.lo + (r.lo & 1);  // a tie goes to the even index
}

template <typename T>
static void q_store(pdx_scalar* o, int dtype, T v) {
  o->dtype = dtype;
  if (dtype == PDX_FLOAT64 || dtype == PDX_FLOAT32) o->v.f64 = (double)v;
  else if (dtype == PDX_UINT64) o->v.u64 = (uint64_t)v;
  else o->v.i64 = (int64_t)v;
}

template <typename T>
static int quantile_typed(const pdx_column* a, const double* q, int nq, int interp, int skip_nulls, int64_t min_count, pdx_scalar* outs, hipStream_t st) {
  using K = typename QKey<T>::K;
  const bool to_f64 = interp == PDX_INTERP_LINEAR || interp == PDX_INTERP_MIDPOINT;
  for (int k = 0; k < nq; ++k) {
    outs[k].dtype = to_f64 ? (int)PDX_FLOAT64 : a->dtype;
    outs[k].is_valid = 0;
    outs[k].v.i64 = 0;
    outs[k].count = 0;
  }
  for (int q0 = 0; q0 < nq; q0 += kQMaxTargets / 2) {  // (more than 64 quantiles: the column is read once per 64)
    const int qn = std::min(nq - q0, kQMaxTargets / 2);
    uint64_t n = 0;
    std::vector<QRank> rk((size_t)qn);
    std::vector<QTarget<K>> tg;
    auto make_ranks = [&](uint64_t n_numbers, uint64_t valid_rows) {
      n = n_numbers;
      std::vector<uint64_t> ranks;
      const bool has_null = valid_rows < (uint64_t)a->length;
      if (n == 0 || (int64_t)valid_rows < min_count || (!skip_nulls && has_null)) return ranks;  // (null result; the count is still reported)
      for (int k = 0; k < qn; ++k) {
        rk[k] = q_rank(n, q[q0 + k]);
        ranks.push_back(rk[k].lo);
        ranks.push_back(rk[k].hi);
      }
      std::sort(ranks.begin(), ranks.end());
      ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
      return ranks;
    };
    if (a->length > 0) PDX_TRY((q_select<T>(a, make_ranks, &tg, st)));
    for (int k = 0; k < qn; ++k) outs[q0 + k].count = (int64_t)n;
    if (tg.empty()) continue;
    auto value_at = [&](uint64_t rank) -> T {
      for (auto& x : tg)
        if (x.global_rank == rank) {
          T v = QKey<T>::value(x.key);
          if (QKey<T>::kFloat && x.negative_zero) v = -v;
          return v;
        }
      return T(0);
    };
    for (int k = 0; k < qn; ++k) {
      pdx_scalar* o = &outs[q0 + k];
      const QRank& r = rk[k];
      o->is_valid = 1;
      if (interp == PDX_INTERP_LINEAR || interp == PDX_INTERP_MIDPOINT) {
        const double lower = (double)value_at(r.lo);
        o->dtype = PDX_FLOAT64;
        if (r.f == 0.0) {
          o->v.f64 = lower;
        } else {
          const double higher = (double)value_at(r.hi);
          if (interp == PDX_INTERP_LINEAR) {
            const double x = r.f * higher, y = (1 - r.f) * lower;
            o->v.f64 = x + y;
          } else {
            const double x = lower / 2, y = higher / 2;
            o->v.f64 = x + y;
          }
        }
      } else {
        q_store<T>(o, a->dtype, value_at(q_point(r, interp)));
      }
    }
  }
  return PDX_OK;
}

static int q_check_args(const char* what, const pdx_column* a, const double* q, int nq, int interp) {
  if (!a) return fail(PDX_INVALID, std::string(what) + ": null column");
  if (a->dtype == PDX_TIMESTAMP_NS) return fail(PDX_NOT_IMPLEMENTED, "Function 'quantile' has no kernel matching input types (timestamp[ns])");
  if (a->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, "Function 'quantile' has no kernel matching input types (bool)");
  if (nq <= 0 || !q) return fail(PDX_INVALID, "Requires quantile argument");
  for (int k = 0; k < nq; ++k)
    if (!(q[k] >= 0.0 && q[k] <= 1.0)) return fail(PDX_INVALID, "Quantile must be between 0 and 1");
  if (interp < PDX_INTERP_LINEAR || interp > PDX_INTERP_MIDPOINT) return fail(PDX_INVALID, std::string(what) + ": unknown interpolation");
  return PDX_OK;
}

// ---------------------------------------------------------------- group form
struct GQOuts {
  void* values[kQMaxTargets / 2];
  double q[kQMaxTargets / 2];
};
template <typename T>
__device__ __forceinline__ bool gq_number(const T* v, const uint8_t* valid, int64_t voff, uint32_t row) {
  if (valid && !bit_get(valid, voff + row)) return false;
  const T x = v[row];
  return x == x;
}
// one lane per group: rows [start, end) of the group in (value, row) order with NaN and nulls behind
template <typename T>
__global__ void __launch_bounds__(256) k_gq_pick(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, const uint32_t* __restrict__ keys,
                                                 const uint32_t* __restrict__ rows, int64_t n, int64_t G, GQOuts o, int nq, int interp, int skip_nulls,
                                                 int64_t min_count, uint8_t* __restrict__ ok /* [nq][G] */) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {  // first position whose group id is >= g
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)keys[mid] < g) lo = mid + 1;
    else hi = mid;
  }
  const int64_t start = lo;
  hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)keys[mid] <= g) lo = mid + 1;
    else hi = mid;
  }
  const int64_t end = lo;
  lo = start;
  hi = end;
  while (lo < hi) {  // first row of the group that is not a number
    const int64_t mid = (lo + hi) >> 1;
    if (gq_number(v, valid, voff, rows[mid])) lo = mid + 1;
    else hi = mid;
  }
  const int64_t cnt = lo - start;
  hi = end;
  while (valid && lo < hi) {  // first null row of the group (behind the NaN rows)
    const int64_t mid = (lo + hi) >> 1;
    if (bit_get(valid, voff + rows[mid])) lo = mid + 1;
    else hi = mid;
  }
  const int64_t non_null = valid ? lo - start : end - start;
  const bool has_null = non_null < end - start;
  const bool is_null = cnt == 0 || non_null < min_count || (!skip_nulls && has_null);
  const bool to_f64 = interp == PDX_INTERP_LINEAR || interp == PDX_INTERP_MIDPOINT;
  for (int k = 0; k < nq; ++k) {
    ok[(int64_t)k * G + g] = is_null ? 0 : 1;
    if (is_null) {
      if (to_f64) static_cast<double*>(o.values[k])[g] = 0.0;
      else static_cast<T*>(o.values[k])[g] = T(0);
      continue;
    }
    const double index = __dmul_rn((double)(cnt - 1), o.q[k]);
    const uint64_t l = (uint64_t)index;
    const double f = __dsub_rn(index, (double)l);
    uint64_t h = f != 0.0 ? l + 1 : l;
    if (h > (uint64_t)(cnt - 1)) h = (uint64_t)(cnt - 1);
    if (to_f64) {
      const double lower = (double)v[rows[start + (int64_t)l]];
      double r = lower;
      if (f != 0.0) {
        const double higher = (double)v[rows[start + (int64_t)h]];
        if (interp == PDX_INTERP_LINEAR) r = __dadd_rn(__dmul_rn(f, higher), __dmul_rn(__dsub_rn(1.0, f), lower));
        else r = __dadd_rn(__ddiv_rn(lower, 2.0), __ddiv_rn(higher, 2.0));
      }
      static_cast<double*>(o.values[k])[g] = r;
    } else {
      uint64_t p;
      if (interp == PDX_INTERP_LOWER) p = l;
      else if (interp == PDX_INTERP_HIGHER) p = h;
      else p = f < 0.5 ? l : f > 0.5 ? h : l + (l & 1);
      static_cast<T*>(o.values[k])[g] = v[rows[start + (int64_t)p]];
    }
  }
}
template <typename T>
static int groupby_quantile_typed(pdx_groupby* gb, const pdx_column* values, const double* q, int nq, int interp, int skip_nulls, int64_t min_count,
                                  pdx_mut_column* outs, void* stream, hipStream_t st) {
  const int64_t n = values->length, G = pdx_groupby_num_groups(gb);
  Scratch s;
  uint8_t* ok = s.get<uint8_t>((size_t)G * (size_t)nq);
  unsigned long long* nulls = s.get<unsigned long long>((size_t)nq);
  PDX_SCRATCH_CHECK(s);
  const uint32_t* ks = nullptr;
  const uint32_t* vs = nullptr;
  PDX_TRY(build_group_value_order(gb, values, &ks, &vs, s, stream, st));
  PDX_HIP(hipMemsetAsync(nulls, 0, sizeof(unsigned long long) * (size_t)nq, st));
  const T* v = static_cast<const T*>(values->values) + values->offset;
  const uint8_t* valid = validity_or_null(values);
  for (int k0i = 0; k0i < nq; k0i += kQMaxTargets / 2) {
    const int kn = std::min(nq - k0i, kQMaxTargets / 2);
    GQOuts o;
    for (int k = 0; k < kn; ++k) {
      o.values[k] = outs[k0i + k].values;
      o.q[k] = q[k0i + k];
    }
    hipLaunchKernelGGL(k_gq_pick<T>, dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, st, v, valid, values->offset, ks, vs, n, G, o, kn, interp, skip_nulls, min_count,
                       ok + (size_t)k0i * (size_t)G);
  }
  for (int k = 0; k < nq; ++k)
    hipLaunchKernelGGL(k_go_pack, dim3(grid_for((G + 7) / 8, 256)), dim3(256), 0, st, ok + (size_t)k * (size_t)G, G, static_cast<uint8_t*>(outs[k].validity),
                       nulls + k);
  PDX_LAUNCH_CHECK();
  std::vector<unsigned long long> hn((size_t)nq);
  PDX_TRY(read_back(hn.data(), nulls, sizeof(unsigned long long) * (size_t)nq, st));
  for (int k = 0; k < nq; ++k) {
    outs[k].length = G;
    outs[k].null_count = (int64_t)hn[k];
    if (hn[k] && !outs[k].validity) return fail(PDX_INVALID, "pdx_groupby_quantile: a group result is null and the output has no validity buffer");
  }
  return PDX_OK;
}

}  // namespace pdx

using namespace pdx;

extern "C" int pdx_quantile(const pdx_column* a, const double* q, int nq, int interpolation, int skip_nulls, int64_t min_count, pdx_scalar* outs,
                            void* stream) {
  PDX_TRY(q_check_args("pdx_quantile", a, q, nq, interpolation));
  PDX_TRY(check_column(a, "pdx_quantile", true));
  if (!outs) return fail(PDX_INVALID, "pdx_quantile: null output");
  hipStream_t st = as_stream(stream);
  switch (a->dtype) {
    case PDX_FLOAT64: return quantile_typed<double>(a, q, nq, interpolation, skip_nulls, min_count, outs, st);
    case PDX_INT64: return quantile_typed<int64_t>(a, q, nq, interpolation, skip_nulls, min_count, outs, st);
    case PDX_UINT64: return quantile_typed<uint64_t>(a, q, nq, interpolation, skip_nulls, min_count, outs, st);
    case PDX_FLOAT32: return quantile_typed<float>(a, q, nq, interpolation, skip_nulls, min_count, outs, st);
    case PDX_INT32: return quantile_typed<int32_t>(a, q, nq, interpolation, skip_nulls, min_count, outs, st);
    default: return fail(PDX_NOT_IMPLEMENTED, "pdx_quantile: unsupported dtype");
  }
}

extern "C" int pdx_groupby_quantile(pdx_groupby* gb, const pdx_column* values, const double* q, int nq, int interpolation, int skip_nulls, int64_t min_count,
                                    pdx_mut_column* outs, void* stream) {
  if (!gb) return fail(PDX_INVALID, "pdx_groupby_quantile: null handle");
  PDX_TRY(q_check_args("pdx_groupby_quantile", values, q, nq, interpolation));
  PDX_TRY(check_column(values, "pdx_groupby_quantile"));
  if (!outs) return fail(PDX_INVALID, "pdx_groupby_quantile: null output");
  const int64_t n = pdx_groupby_num_rows(gb), G = pdx_groupby_num_groups(gb);
  if (values->length != n) return fail(PDX_INVALID, "pdx_groupby_quantile: values and keys differ in length");
  const bool to_f64 = interpolation == PDX_INTERP_LINEAR || interpolation == PDX_INTERP_MIDPOINT;
  for (int k = 0; k < nq; ++k) {
    if (outs[k].dtype != (to_f64 ? (int)PDX_FLOAT64 : values->dtype)) return fail(PDX_INVALID, "pdx_groupby_quantile: wrong output dtype");
    if (outs[k].length < G || (G && !outs[k].values)) return fail(PDX_INVALID, "pdx_groupby_quantile: output too small");
  }
  hipStream_t st = as_stream(stream);
  if (G == 0 || n == 0) {
    for (int k = 0; k < nq; ++k) {
      outs[k].length = G;
      outs[k].null_count = 0;
    }
    return PDX_OK;
  }
  switch (values->dtype) {
    case PDX_FLOAT64: return groupby_quantile_typed<double>(gb, values, q, nq, interpolation, skip_nulls, min_count, outs, stream, st);
    case PDX_INT64: return groupby_quantile_typed<int64_t>(gb, values, q, nq, interpolation, skip_nulls, min_count, outs, stream, st);
    case PDX_UINT64: return groupby_quantile_typed<uint64_t>(gb, values, q, nq, interpolation, skip_nulls, min_count, outs, stream, st);
    default: return fail(PDX_NOT_IMPLEMENTED, "pdx_groupby_quantile: unsupported dtype");
  }
}
