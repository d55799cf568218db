// select_k.hip -- top-k and partition without a full sort for gfx950: pdx_select_k (Series::n_largest / n_smallest) and
// pdx_partition_nth (Series::nth_element).
//
// Replaces sort + Slice at the reference's src/series.cpp:1211-1229 (n_largest / n_smallest) and CallFunction("partition_nth_indices")
// at src/series.cpp:973-976.  pdx_select_k writes the first min(k, n) entries of pdx_argsort(col, ascending), bit for bit:
//   select   q_select (radix_select.hpp, the select of pdx_quantile) locates the key T at the k-th place among the numbers and returns
//            the number and valid-row counts (-> NaN and null counts);
//   count    k_sk_count: one streaming read; every WAVE owns a contiguous quarter of its workgroup's chunk and counts its rows in front
//            of T, equal to T, behind T, NaN and null (one ballot + popcount per class and 64 rows, no atomics);
//   scan     k_sk_scan: exclusive scan of those counts over the waves, per class, and the totals;
//   emit     k_sk_emit: second read; the rows in front of T and the first r = k - total_front ties become (key, row) pairs, placed in
//            row order by ballot + popcount from the wave's scanned offset; when k exceeds the numbers the first NaN rows and then the
//            first null rows go straight behind them in the output.  A wave with nothing to give returns before it reads a row, so for
//            a small k the second read touches only the few sub-chunks that hold a candidate;
//   sort     the at most k pairs: one workgroup in LDS up to 4096 (k_sk_small), else the stable LSD radix sort of radix_sort.hpp.  The
//            keys are complemented for descending, so a stable ascending sort is the stable descending order.
// pdx_partition_nth runs the same select, count and scan and then one scatter read (k_sk_emit<.., true>); it sorts nothing.
// Every row count is 64 bits; row ids fit 32 bits (at most 2^31-1 rows per call).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "colview.hpp"
#include "quantile.hpp"
#include "radix_select.hpp"
#include "radix_sort.hpp"

namespace pdx {

static thread_local std::string g_select_k_plan = "plan=none k=0 rows=0 levels=0";

// Above this fraction of the rows (k > rows >> kSkCrossoverShift) pdx_select_k sorts the whole column instead.  Measured (tools/bench_topk.py,
// 1e8 rows): the select plan beats the sort plan at every k / n of the sweep up to 0.5 (4.42 against 6.08 ms float64, 2.47
// against 3.70 ms int32); nothing was measured between 0.5 and 1, so the largest measured fraction, 1/2, is the constant.
constexpr int kSkCrossoverShift = 1;

constexpr int kSkBlock = 256;
constexpr int kSkWaves = kSkBlock / 64;
constexpr int kSkUnroll = 4;
constexpr int kSkSmall = 4096;  // pairs finished by one workgroup in LDS
enum { kSkFront = 0, kSkEqual = 1, kSkBack = 2, kSkNan = 3, kSkNull = 4, kSkClasses = 5 };

// a row's class against the threshold key t; *key: its ascending key (classes front / equal / back only)
template <typename T>
__device__ __forceinline__ int sk_class(T v, bool row_valid, typename QKey<T>::K t, bool descending, typename QKey<T>::K* key) {
  if (!row_valid) return kSkNull;
  typename QKey<T>::K k = 0;
  if (!QKey<T>::key(v, &k)) return kSkNan;
  *key = k;
  if (k == t) return kSkEqual;
  return ((k < t) != descending) ? kSkFront : kSkBack;
}
// the rows [*begin, *end) of this wave: a quarter of the workgroup's chunk (chunk is a multiple of 256), wave-uniform
__device__ __forceinline__ uint32_t sk_unit(uint64_t n, uint64_t chunk, uint64_t* begin, uint64_t* end) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t sub = chunk / kSkWaves;
  const uint64_t b = (uint64_t)blockIdx.x * chunk + (uint64_t)wave * sub;
  *begin = b < n ? b : n;
  *end = b + sub < n ? b + sub : n;
  return blockIdx.x * kSkWaves + wave;
}
// validity of the 64 rows from row0 on (row0 < end; wave-uniform): scalar loads
__device__ __forceinline__ uint64_t sk_valid_word(const uint8_t* valid, int64_t voff, uint64_t row0, uint64_t end) {
  if (!valid) return ~0ull;
  const uint64_t rem = end - row0;
  return load_bits64_uniform(valid, voff + (int64_t)row0, rem < 64 ? (int)rem : 64);
}

template <typename T>
__global__ void __launch_bounds__(kSkBlock) k_sk_count(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, uint64_t n, uint64_t chunk,
                                                       typename QKey<T>::K t, int descending, unsigned long long* __restrict__ counts /* [units][5] */) {
  using K = typename QKey<T>::K;
  uint64_t begin, end;
  const uint32_t unit = sk_unit(n, chunk, &begin, &end);
  const int lane = threadIdx.x & 63;
  uint32_t c[kSkClasses] = {0, 0, 0, 0, 0};
  for (uint64_t i0 = begin; i0 < end; i0 += 64 * kSkUnroll) {
    int cls[kSkUnroll];
#pragma unroll
    for (int u = 0; u < kSkUnroll; ++u) {
      const uint64_t row0 = i0 + (uint64_t)u * 64, i = row0 + lane;
      cls[u] = -1;
      if (row0 < end) {
        const uint64_t w = sk_valid_word(valid, voff, row0, end);
        K key;
        if (i < end) cls[u] = sk_class<T>(v[i], (w >> lane) & 1, t, descending != 0, &key);
      }
    }
#pragma unroll
    for (int u = 0; u < kSkUnroll; ++u)
#pragma unroll
      for (int q = 0; q < kSkClasses; ++q) c[q] += (uint32_t)__popcll(__ballot(cls[u] == q));
  }
  if (lane < kSkClasses) {
    uint32_t mine = c[0];
#pragma unroll
    for (int q = 1; q < kSkClasses; ++q) mine = lane == q ? c[q] : mine;
    counts[(uint64_t)unit * kSkClasses + lane] = mine;
  }
}

// workgroup q (one wave): counts[u][q] -> rows of class q in the units before u; counts[units][q] = the total
__global__ void __launch_bounds__(64) k_sk_scan(unsigned long long* __restrict__ counts, uint32_t units) {
  const int q = blockIdx.x, lane = threadIdx.x;
  unsigned long long carry = 0;
  for (uint32_t u0 = 0; u0 < units; u0 += 64) {
    const uint32_t u = u0 + lane;
    const unsigned long long x = u < units ? counts[(uint64_t)u * kSkClasses + q] : 0ull;
    unsigned long long inc = x;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (u < units) counts[(uint64_t)u * kSkClasses + q] = carry + inc - x;
    carry += __shfl(inc, 63, 64);
  }
  if (lane == 0) counts[(uint64_t)units * kSkClasses + q] = carry;
}

// where the emit read writes.  Top-k: pairs (lo, pay) -- 8-byte keys: lo = the low key half, pay = high key half << 32 | row (the
// element of the 64-bit sort, align.hip); 4-byte keys: lo = the key, pay = the row -- and NaN / null rows straight into `out`.
// Partition: every row into `out`.
template <typename P>
struct SkOut {
  uint32_t* lo;
  P* pay;
  unsigned long long* out;
  uint64_t k_num;      // numbers wanted = pairs
  uint64_t want_nan;   // NaN rows wanted behind them
  uint64_t want_null;  // null rows wanted behind those
};

template <typename T, bool PARTITION>
__global__ void __launch_bounds__(kSkBlock) k_sk_emit(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, uint64_t n, uint64_t chunk,
                                                      typename QKey<T>::K t, int descending, const unsigned long long* __restrict__ offs /* [units + 1][5] */,
                                                      uint32_t units, SkOut<typename std::conditional<sizeof(typename QKey<T>::K) == 8, unsigned long long, uint32_t>::type> o) {
  using K = typename QKey<T>::K;
  uint64_t begin, end;
  const uint32_t unit = sk_unit(n, chunk, &begin, &end);
  if (begin >= end) return;
  const int lane = threadIdx.x & 63;
  const unsigned long long lt_mask = lane ? (~0ull >> (64 - lane)) : 0ull;
  const unsigned long long* tot = offs + (uint64_t)units * kSkClasses;
  unsigned long long at[kSkClasses];  // this wave's next place per class (wave-uniform)
#pragma unroll
  for (int q = 0; q < kSkClasses; ++q) at[q] = offs[(uint64_t)unit * kSkClasses + q];
  const unsigned long long total_front = tot[kSkFront], total_equal = tot[kSkEqual], total_back = tot[kSkBack], total_nan = tot[kSkNan];
  unsigned long long ties = 0;  // top-k: ties kept
  unsigned long long base[kSkClasses] = {0, 0, 0, 0, 0};
  if constexpr (PARTITION) {
    base[kSkEqual] = total_front;
    base[kSkBack] = total_front + total_equal;
    base[kSkNan] = base[kSkBack] + total_back;
    base[kSkNull] = base[kSkNan] + total_nan;
  } else {
    ties = total_front < o.k_num ? o.k_num - total_front : 0;  // (total_front < k_num by the choice of T)
    const unsigned long long front_here = offs[(uint64_t)(unit + 1) * kSkClasses + kSkFront] - at[kSkFront];  // (row `units` holds the totals)
    if (front_here == 0 && at[kSkEqual] >= ties && at[kSkNan] >= o.want_nan && at[kSkNull] >= o.want_null) return;  // nothing of this wave is kept
  }
  for (uint64_t i0 = begin; i0 < end; i0 += 64 * kSkUnroll) {
    int cls[kSkUnroll];
    K key[kSkUnroll];
#pragma unroll
    for (int u = 0; u < kSkUnroll; ++u) {
      const uint64_t row0 = i0 + (uint64_t)u * 64, i = row0 + lane;
      cls[u] = -1;
      key[u] = 0;
      if (row0 < end) {
        const uint64_t w = sk_valid_word(valid, voff, row0, end);
        if (i < end) cls[u] = sk_class<T>(v[i], (w >> lane) & 1, t, descending != 0, &key[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kSkUnroll; ++u) {
      const uint64_t i = i0 + (uint64_t)u * 64 + lane;
      unsigned long long place = 0;
#pragma unroll
      for (int q = 0; q < kSkClasses; ++q) {
        const unsigned long long m = __ballot(cls[u] == q);
        if (cls[u] == q) place = at[q] + (unsigned long long)__popcll(m & lt_mask);
        at[q] += (unsigned long long)__popcll(m);
      }
      if (cls[u] < 0) continue;
      if constexpr (PARTITION) {
        const unsigned long long dst = base[cls[u]] + place;
        if (dst < n) o.out[dst] = i;  // (always: the five totals add up to n)
      } else {
        if (cls[u] == kSkFront || (cls[u] == kSkEqual && place < ties)) {
          const unsigned long long p = cls[u] == kSkFront ? place : total_front + place;
          const K sk = descending ? (K)~key[u] : key[u];
          if (p >= o.k_num) continue;  // (never: front rows + kept ties == k_num)
          if constexpr (sizeof(K) == 8) {
            o.lo[p] = (uint32_t)sk;
            o.pay[p] = (sk & 0xFFFFFFFF00000000ull) | i;
          } else {
            o.lo[p] = sk;
            o.pay[p] = (uint32_t)i;
          }
        } else if (cls[u] == kSkNan && place < o.want_nan) {
          o.out[o.k_num + place] = i;
        } else if (cls[u] == kSkNull && place < o.want_null) {
          o.out[o.k_num + o.want_nan + place] = i;
        }
      }
    }
  }
}

// one workgroup sorts the m <= 4096 pairs by (key, row) in LDS (rows are distinct, so the bitonic network gives the stable order)
template <typename K, typename P>
__global__ void __launch_bounds__(kSkBlock) k_sk_small(const uint32_t* __restrict__ lo, const P* __restrict__ pay, int m, unsigned long long* __restrict__ out) {
  __shared__ K sk[kSkSmall];
  __shared__ uint32_t sr[kSkSmall];
  int P2 = 1;
  while (P2 < m) P2 <<= 1;
  for (int i = threadIdx.x; i < P2; i += kSkBlock) {
    K k = (K)~(K)0;
    uint32_t r = 0xFFFFFFFFu;
    if (i < m) {
      if constexpr (sizeof(K) == 8) {
        k = (K)((pay[i] & 0xFFFFFFFF00000000ull) | lo[i]);
        r = (uint32_t)pay[i];
      } else {
        k = lo[i];
        r = pay[i];
      }
    }
    sk[i] = k;
    sr[i] = r;
  }
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P2; i += kSkBlock) {
        const int x = i ^ j;
        if (x > i) {
          const K a = sk[i], b = sk[x];
          const uint32_t ra = sr[i], rb = sr[x];
          const bool gt = a > b || (a == b && ra > rb);
          if (gt == ((i & k) == 0)) {
            sk[i] = b;
            sk[x] = a;
            sr[i] = rb;
            sr[x] = ra;
          }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < m; i += kSkBlock) out[i] = sr[i];
}
template <typename P>
__global__ void k_sk_rows_out(const P* __restrict__ pay, int64_t m, unsigned long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) out[i] = (unsigned long long)pay[i] & 0xFFFFFFFFull;
}

// ---------------------------------------------------------------- host
struct SkCounts {
  uint64_t numbers, nans, nulls;
  int levels;
};
// the key at `rank_of(numbers)` among the numbers of a (no select when the column has none), and the class counts
template <typename T, typename RankOf>
static int sk_threshold(const pdx_column* a, RankOf rank_of, typename QKey<T>::K* t, SkCounts* c, hipStream_t st) {
  using K = typename QKey<T>::K;
  std::vector<QTarget<K>> tg;
  uint64_t numbers = 0, valid_rows = 0;
  auto make_ranks = [&](uint64_t n_numbers, uint64_t n_valid) {
    numbers = n_numbers;
    valid_rows = n_valid;
    std::vector<uint64_t> ranks;
    if (numbers) ranks.push_back(rank_of(numbers));
    return ranks;
  };
  c->levels = 0;
  PDX_TRY((q_select<T>(a, make_ranks, &tg, st, false, &c->levels)));
  c->numbers = numbers;
  c->nans = valid_rows - numbers;
  c->nulls = (uint64_t)a->length - valid_rows;
  *t = tg.empty() ? (K)0 : tg[0].key;
  return PDX_OK;
}

struct SkGrid {
  uint64_t chunk;
  uint32_t nblocks, units;
};
static SkGrid sk_grid(uint64_t n) {
  SkGrid g;
  g.chunk = (uint64_t)round_up((int64_t)std::max<uint64_t>(65536, (n + 2047) / 2048), kSkBlock);
  g.nblocks = (uint32_t)((n + g.chunk - 1) / g.chunk);
  g.units = g.nblocks * kSkWaves;
  return g;
}
// count + scan: offs[u][q] = rows of class q in front of wave u, offs[units][q] = all of them
template <typename T>
static int sk_offsets(const pdx_column* a, typename QKey<T>::K t, int descending, const SkGrid& g, Scratch& s, hipStream_t st, unsigned long long** offs) {
  *offs = s.get<unsigned long long>((size_t)(g.units + 1) * kSkClasses);
  PDX_SCRATCH_CHECK(s);
  const T* v = static_cast<const T*>(a->values) + a->offset;
  hipLaunchKernelGGL(k_sk_count<T>, dim3(g.nblocks), dim3(kSkBlock), 0, st, v, validity_or_null(a), a->offset, (uint64_t)a->length, g.chunk, t, descending, *offs);
  hipLaunchKernelGGL(k_sk_scan, dim3(kSkClasses), dim3(64), 0, st, *offs, g.units);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// the m > 4096 pairs in key order: rows to out
static int sk_sort_pairs(uint32_t* lo, unsigned long long* pay, int64_t m, unsigned long long* out, Scratch& s, hipStream_t st) {
  const int64_t ntiles = ceil_div(m, kSortTile), nchunks = ceil_div(ntiles, kColChunk);
  uint32_t* lo1 = s.get<uint32_t>((size_t)m);
  unsigned long long* pay1 = s.get<unsigned long long>((size_t)m);
  uint32_t* hist = s.get<uint32_t>((size_t)ntiles << 8);
  uint32_t* chunk = s.get<uint32_t>((size_t)(nchunks + 1) << 8);
  PDX_SCRATCH_CHECK(s);
  const uint32_t* kin = lo;
  const unsigned long long* vin = pay;
  for (int d = 0; d < 8; ++d) {  // four passes on the low key half carry the element along, four take their digit from its high half
    unsigned long long* vout = vin == pay ? pay1 : pay;
    if (d < 4) {
      uint32_t* kout = kin == lo ? lo1 : lo;
      PDX_TRY((radix_pass_dispatch<uint64_t>(8, kin, reinterpret_cast<const uint64_t*>(vin), kout, reinterpret_cast<uint64_t*>(vout), m, 8 * d, d != 3, hist, chunk, st)));
      if (d != 3) kin = kout;
    } else {
      PDX_TRY((radix_pass_payload_hi<8>(reinterpret_cast<const uint64_t*>(vin), reinterpret_cast<uint64_t*>(vout), m, 8 * (d - 4), hist, chunk, st)));
    }
    vin = vout;
  }
  hipLaunchKernelGGL(k_sk_rows_out<unsigned long long>, dim3(grid_for(m, 256, 4)), dim3(256), 0, st, vin, m, out);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}
static int sk_sort_pairs(uint32_t* lo, uint32_t* rows, int64_t m, unsigned long long* out, Scratch& s, hipStream_t st) {
  uint32_t* k0 = s.get<uint32_t>((size_t)m);
  uint32_t* v0 = s.get<uint32_t>((size_t)m);
  uint32_t* k1 = s.get<uint32_t>((size_t)m);
  uint32_t* v1 = s.get<uint32_t>((size_t)m);
  PDX_SCRATCH_CHECK(s);
  const uint32_t* ks = nullptr;
  const uint32_t* vs = nullptr;
  PDX_TRY((radix_sort_pairs<uint32_t>(lo, rows, k0, v0, k1, v1, m, 32, &ks, &vs, false, s, st)));
  hipLaunchKernelGGL(k_sk_rows_out<uint32_t>, dim3(grid_for(m, 256, 4)), dim3(256), 0, st, vs, m, out);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

template <typename T>
static int select_k_typed(const pdx_column* a, uint64_t k, int ascending, unsigned long long* out, int* levels, hipStream_t st) {
  using K = typename QKey<T>::K;
  using P = typename std::conditional<sizeof(K) == 8, unsigned long long, uint32_t>::type;
  PDX_PROFILE("select_k", st);
  const int descending = ascending ? 0 : 1;
  K t = 0;
  SkCounts c{};
  auto rank_of = [&](uint64_t numbers) {
    const uint64_t k_num = std::min(k, numbers);
    return descending ? numbers - k_num : k_num - 1;
  };
  PDX_TRY((sk_threshold<T>(a, rank_of, &t, &c, st)));
  *levels = c.levels;
  Scratch s;
  SkOut<P> o{};
  o.out = out;
  o.k_num = std::min(k, c.numbers);
  o.want_nan = std::min(k - o.k_num, c.nans);
  o.want_null = std::min(k - o.k_num - o.want_nan, c.nulls);
  o.lo = s.get<uint32_t>((size_t)o.k_num);
  o.pay = s.get<P>((size_t)o.k_num);
  PDX_SCRATCH_CHECK(s);
  const SkGrid g = sk_grid((uint64_t)a->length);
  unsigned long long* offs = nullptr;
  PDX_TRY((sk_offsets<T>(a, t, descending, g, s, st, &offs)));
  const T* v = static_cast<const T*>(a->values) + a->offset;
  hipLaunchKernelGGL((k_sk_emit<T, false>), dim3(g.nblocks), dim3(kSkBlock), 0, st, v, validity_or_null(a), a->offset, (uint64_t)a->length, g.chunk, t, descending,
                     offs, g.units, o);
  PDX_LAUNCH_CHECK();
  if (o.k_num == 0) return PDX_OK;
  if (o.k_num <= (uint64_t)kSkSmall) {
    hipLaunchKernelGGL((k_sk_small<K, P>), dim3(1), dim3(kSkBlock), 0, st, o.lo, o.pay, (int)o.k_num, out);
    PDX_LAUNCH_CHECK();
    return PDX_OK;
  }
  return sk_sort_pairs(o.lo, o.pay, (int64_t)o.k_num, out, s, st);
}

template <typename T>
static int partition_nth_typed(const pdx_column* a, uint64_t pivot, unsigned long long* out, hipStream_t st) {
  using K = typename QKey<T>::K;
  using P = typename std::conditional<sizeof(K) == 8, unsigned long long, uint32_t>::type;
  PDX_PROFILE("partition_nth", st);
  K t = 0;
  SkCounts c{};
  auto rank_of = [&](uint64_t numbers) { return std::min(pivot, numbers - 1); };  // (a pivot among the NaN / null rows: the largest key)
  PDX_TRY((sk_threshold<T>(a, rank_of, &t, &c, st)));
  Scratch s;
  SkOut<P> o{};
  o.out = out;
  const SkGrid g = sk_grid((uint64_t)a->length);
  unsigned long long* offs = nullptr;
  PDX_TRY((sk_offsets<T>(a, t, 0, g, s, st, &offs)));
  const T* v = static_cast<const T*>(a->values) + a->offset;
  hipLaunchKernelGGL((k_sk_emit<T, true>), dim3(g.nblocks), dim3(kSkBlock), 0, st, v, validity_or_null(a), a->offset, (uint64_t)a->length, g.chunk, t, 0, offs,
                     g.units, o);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

static int sk_check(const char* who, const pdx_column* col, pdx_mut_column* out, int64_t rows_out) {
  if (!col) return fail(PDX_INVALID, std::string(who) + ": null column");
  if (col->dtype == PDX_BOOL) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": dtype bool is not supported");
  PDX_TRY(check_column(col, who, true));
  if (col->length > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": more than 2^31-1 rows per call is not supported yet");
  return check_out(who, out, PDX_UINT64, rows_out);
}

enum { kSkPlanAuto = 0, kSkPlanSelect = 1, kSkPlanSort = 2 };
static int select_k_forced_plan() {  // read per call: a test exercises both plans at small sizes
  const char* e = getenv("PDX_SELECT_K_PLAN");
  if (!e) return kSkPlanAuto;
  if (!strcmp(e, "select")) return kSkPlanSelect;
  if (!strcmp(e, "sort")) return kSkPlanSort;
  return kSkPlanAuto;
}

}  // namespace pdx

using namespace pdx;

extern "C" int pdx_select_k(const pdx_column* col, int64_t k, int ascending, pdx_mut_column* out, void* stream) {
  if (k < 0) return fail(PDX_INVALID, "pdx_select_k: k must not be negative");
  const int64_t n = col ? col->length : 0, rows_out = std::min(k, n);
  PDX_TRY(sk_check("pdx_select_k", col, out, rows_out));
  hipStream_t st = as_stream(stream);
  const bool can_select = k > 0 && k < n;
  const int forced = select_k_forced_plan();
  const bool empty = k == 0 || n == 0;
  const bool select = !empty && can_select && (forced == kSkPlanSelect || (forced != kSkPlanSort && k <= (n >> kSkCrossoverShift)));
  int levels = 0;
  out->length = rows_out;
  out->null_count = 0;
  if (empty) {
    g_select_k_plan = "plan=empty k=" + std::to_string(k) + " rows=" + std::to_string(n) + " levels=0";
    return PDX_OK;
  }
  unsigned long long* outp = static_cast<unsigned long long*>(out->values);
  if (select) {
    int rc = PDX_NOT_IMPLEMENTED;
    switch (col->dtype) {
      case PDX_FLOAT64: rc = select_k_typed<double>(col, (uint64_t)k, ascending, outp, &levels, st); break;
      case PDX_INT64:
      case PDX_TIMESTAMP_NS: rc = select_k_typed<int64_t>(col, (uint64_t)k, ascending, outp, &levels, st); break;
      case PDX_UINT64: rc = select_k_typed<uint64_t>(col, (uint64_t)k, ascending, outp, &levels, st); break;
      case PDX_FLOAT32: rc = select_k_typed<float>(col, (uint64_t)k, ascending, outp, &levels, st); break;
      case PDX_INT32: rc = select_k_typed<int32_t>(col, (uint64_t)k, ascending, outp, &levels, st); break;
      default: return fail(PDX_NOT_IMPLEMENTED, "pdx_select_k: unsupported dtype");
    }
    PDX_TRY(rc);
    PDX_HIP(hipStreamSynchronize(st));
  } else {  // one full single-key sort, the first k indices copied out
    Scratch s;
    const int desc = ascending ? 0 : 1;
    pdx_mut_column all{};
    all.dtype = PDX_UINT64;
    all.length = n;
    all.values = outp;
    if (rows_out < n) {
      all.values = s.get<unsigned long long>((size_t)n);
      PDX_SCRATCH_CHECK(s);
    }
    PDX_TRY(pdx_sort_indices(col, 1, &desc, &all, nullptr, stream));
    if (rows_out < n) {
      PDX_HIP(hipMemcpyAsync(outp, all.values, sizeof(unsigned long long) * (size_t)rows_out, hipMemcpyDeviceToDevice, st));
      PDX_HIP(hipStreamSynchronize(st));
    }
  }
  g_select_k_plan = std::string("plan=") + (select ? "select" : "sort") + " k=" + std::to_string(k) + " rows=" + std::to_string(n) + " levels=" + std::to_string(levels);
  return PDX_OK;
}

extern "C" int pdx_partition_nth(const pdx_column* col, int64_t pivot, pdx_mut_column* out, void* stream) {
  if (pivot < 0) return fail(PDX_INVALID, "pdx_partition_nth: the pivot must not be negative");
  const int64_t n = col ? col->length : 0;
  PDX_TRY(sk_check("pdx_partition_nth", col, out, n));
  if (pivot > n) return fail(PDX_INVALID, "pdx_partition_nth: the pivot lies beyond the column");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  unsigned long long* outp = static_cast<unsigned long long*>(out->values);
  int rc = PDX_NOT_IMPLEMENTED;
  switch (col->dtype) {
    case PDX_FLOAT64: rc = partition_nth_typed<double>(col, (uint64_t)pivot, outp, st); break;
    case PDX_INT64:
    case PDX_TIMESTAMP_NS: rc = partition_nth_typed<int64_t>(col, (uint64_t)pivot, outp, st); break;
    case PDX_UINT64: rc = partition_nth_typed<uint64_t>(col, (uint64_t)pivot, outp, st); break;
    case PDX_FLOAT32: rc = partition_nth_typed<float>(col, (uint64_t)pivot, outp, st); break;
    case PDX_INT32: rc = partition_nth_typed<int32_t>(col, (uint64_t)pivot, outp, st); break;
    default: return fail(PDX_NOT_IMPLEMENTED, "pdx_partition_nth: unsupported dtype");
  }
  PDX_TRY(rc);
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

extern "C" int pdx_select_k_last_plan(char* buf, size_t buf_len) {
  if (!buf || !buf_len) return fail(PDX_INVALID, "pdx_select_k_last_plan: null buffer");
  snprintf(buf, buf_len, "%s", g_select_k_plan.c_str());
  return PDX_OK;
}
