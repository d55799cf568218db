// radix_select.hpp -- the 11-bit radix select shared by pdx_quantile (quantile.hip) and pdx_select_k / pdx_partition_nth (select_k.hip):
// the kernels of one level (histogram, fold, offsets, compaction), the small LDS finish and the host loop q_select that locates any
// ranks of a column's numbers.  The algorithm is described at the top of quantile.hip; the keys and level descriptors are quantile.hpp's.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>
#include "colview.hpp"
#include "quantile.hpp"

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
static __global__ void __launch_bounds__(kQBlock) k_q_fold(const QSeg* __restrict__ segs, int nseg, const uint32_t* __restrict__ partial, uint32_t total_blocks,
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
static __global__ void __launch_bounds__(kQBlock) k_q_offsets(const QSeg* __restrict__ segs, const QSel* __restrict__ sels, const uint32_t* __restrict__ partial,
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
// zero_sign = false: a caller that only wants keys skips the two reads that tell -0.0 from 0.0; levels (optional): histogram levels run.
template <typename T, typename MakeRanks>
static int q_select(const pdx_column* a, MakeRanks make_ranks, std::vector<QTarget<typename QKey<T>::K>>* out, hipStream_t st, bool zero_sign = true,
                    int* levels = nullptr) {
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
    if (levels) ++*levels;
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
    for (auto& x : tg) any_zero = any_zero || (zero_sign && x.key == QKey<T>::kZero);
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

}  // namespace pdx
