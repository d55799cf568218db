// mode.hip -- value frequencies for gfx950: pdx_mode (the n most frequent values of a column) and pdx_groupby_mode.
//
// Replaces CallFunction("mode", {array}, ModeOptions{n, skip_nulls, min_count}) reached from NDFrame::mode (reference src/ndframe.h:63-66,
// 255, src/ndframe.cpp:177-197) and, per group, what GroupBy::mode intends (src/group_by.h:126-127, src/dataframe.cpp:1808-1865).
//
// Whole column, two paths behind one first read (k_mode_scan: valid rows, and for the integer dtypes the smallest / largest value):
//   counting  bool, and integers whose max - min + 1 <= kModeBins: a second read builds a workgroup-private uint32 histogram in LDS
//             (k_mode_hist; the lanes of a wave that share the wave's hot bin are counted by one ballot) and adds its non-zero bins to
//             one global 64-bit histogram.  A candidate is a bin, its position the bin index.
//   sort      everything else: the stable sort of the column (numbers ascending, NaN behind them, nulls last; -0.0 == 0.0 keep their
//             row order), k_mode_mark flags the first row of every run of equal values (all NaNs are equal), the flagged positions are
//             compacted (compact.hpp).  A candidate is a run, its position the run's start in the sorted order.
// Top n, shared: key = (count << 32) | ~position, so the largest key is the most frequent value and, among equals, the smallest one
// (NaN last).  n == 1 is one max-reduction (k_mode_top, which also counts the candidates that hold rows); n > 1 is one stable radix
// sort of the candidates by (largest count - count): they are generated in position order, so ties keep ascending positions.
//
// Group form: the (group, value, row) order of pdx_groupby_quantile, the same run flags with the group id as a second break, the runs
// compacted, then one 64-bit atomic max per run into its group's slot.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "colview.hpp"
#include "compact.hpp"
#include "group_order.hpp"
#include "minmax.hpp"
#include "quantile.hpp"
#include "radix_sort.hpp"

namespace pdx {

constexpr int kModeBins = 8192;  // widest value range the counting path takes: 32 KB of LDS counters per workgroup (measured against 4096 and
                                 // 16384 words)
constexpr int kModeBlock = 256;
constexpr int kModeMaxBlocks = kCUs * 4;

static thread_local std::string g_mode_plan;

template <typename T>
__device__ __forceinline__ T mode_unkey(unsigned long long k);
template <> __device__ __forceinline__ int64_t mode_unkey<int64_t>(unsigned long long k) { return (int64_t)(k ^ 0x8000000000000000ull); }
template <> __device__ __forceinline__ uint64_t mode_unkey<uint64_t>(unsigned long long k) { return k; }
template <> __device__ __forceinline__ int32_t mode_unkey<int32_t>(unsigned long long k) { return (int32_t)((uint32_t)k ^ 0x80000000u); }
template <> __device__ __forceinline__ double mode_unkey<double>(unsigned long long) { return 0.0; }  // (floats never take the counting path:
template <> __device__ __forceinline__ float mode_unkey<float>(unsigned long long) { return 0.0f; }  //  k_mode_emit's other branch is theirs)

template <typename T>
__device__ __forceinline__ bool mode_equal(T x, T y) { return x == y || (x != x && y != y); }
template <typename T>
__device__ __forceinline__ T mode_canonical(T x) {
  if constexpr (QKey<T>::kFloat) {
    if (x != x) {
      if constexpr (sizeof(T) == 8) return __longlong_as_double(0x7ff8000000000000ll);
      else return __int_as_float(0x7fc00000);
    }
  }
  return x;
}

// ---------------------------------------------------------------- first read: valid rows; integers: smallest / largest key
struct ModeScan {
  unsigned long long kmin, kmax, valid;
  long long any;  // >= 0: kmin / kmax are set
};
template <typename T>
__global__ void __launch_bounds__(kModeBlock) k_mode_scan(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                          ModeScan* __restrict__ part /* [gridDim.x] */) {
  using K = typename QKey<T>::K;
  __shared__ ModeScan ws[kModeBlock / 64];
  Extreme<unsigned long long> e;
  e.init();
  unsigned long long vc = 0;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kModeBlock;
  for (int64_t i0 = ((int64_t)blockIdx.x * (kModeBlock / 64) + (threadIdx.x >> 6)) * 64; i0 < n; i0 += stride) {
    const uint64_t bits = valid ? load_bits64(valid, voff + i0, voff + n) : ~0ull;  // one 64-bit window per wave step
    const int64_t i = i0 + lane;
    if (i < n && ((bits >> lane) & 1ull)) {
      ++vc;
      if constexpr (!QKey<T>::kFloat) {
        K k;
        QKey<T>::key(v[i], &k);
        e.add((unsigned long long)k, (long long)i);
      }
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long omin = __shfl_down(e.vmin, d, 64), omax = __shfl_down(e.vmax, d, 64);
    const long long ormin = __shfl_down(e.rmin, d, 64), ormax = __shfl_down(e.rmax, d, 64);
    e.merge(omin, ormin, omax, ormax);
    vc += __shfl_down(vc, d, 64);
  }
  if (lane == 0) ws[threadIdx.x >> 6] = ModeScan{e.vmin, e.vmax, vc, e.rmin};
  __syncthreads();
  if (threadIdx.x == 0) {
    ModeScan r = ws[0];
    for (int w = 1; w < kModeBlock / 64; ++w) {
      const ModeScan o = ws[w];
      r.valid += o.valid;
      if (o.any >= 0) {
        if (r.any < 0 || o.kmin < r.kmin) r.kmin = o.kmin;
        if (r.any < 0 || o.kmax > r.kmax) r.kmax = o.kmax;
        r.any = 0;
      }
    }
    part[blockIdx.x] = r;
  }
}

// bool: the valid rows and the valid true rows, one 64-bit window of both bitmaps per lane and step
__global__ void __launch_bounds__(kModeBlock) k_mode_bool(const uint8_t* __restrict__ vals, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                          unsigned long long* __restrict__ out /* [0] true, [1] valid */) {
  unsigned long long t = 0, c = 0;
  const int64_t nwin = (n + 63) >> 6, stride = (int64_t)gridDim.x * kModeBlock;
  for (int64_t w = (int64_t)blockIdx.x * kModeBlock + threadIdx.x; w < nwin; w += stride) {
    const int64_t remain = n - w * 64;
    const uint64_t in = remain >= 64 ? ~0ull : ((1ull << remain) - 1ull);
    const uint64_t vb = valid ? load_bits64(valid, off + w * 64, off + n) : in;
    const uint64_t xb = load_bits64(vals, off + w * 64, off + n);
    t += (unsigned long long)__popcll(xb & vb);
    c += (unsigned long long)__popcll(vb);
  }
  for (int d = 32; d > 0; d >>= 1) {
    t += __shfl_down(t, d, 64);
    c += __shfl_down(c, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (t) atomicAdd(&out[0], t);
    if (c) atomicAdd(&out[1], c);
  }
}
// the (at most two) bool results: value bits 0 .. k-1 of the packed output and the int64 counts; nothing beyond them is written
__global__ void k_mode_emit_bool(uint8_t* __restrict__ out_bits, long long* __restrict__ out_counts, int k, int v0, int v1, long long c0, long long c1) {
  if (threadIdx.x || blockIdx.x) return;
  uint8_t b = out_bits[0];
  if (k > 0) {
    b = (uint8_t)((b & ~1u) | (v0 ? 1u : 0u));
    out_counts[0] = c0;
  }
  if (k > 1) {
    b = (uint8_t)((b & ~2u) | (v1 ? 2u : 0u));
    out_counts[1] = c1;
  }
  out_bits[0] = b;
}

// ---------------------------------------------------------------- counting path
template <typename T>
__global__ void __launch_bounds__(kModeBlock) k_mode_hist(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                          unsigned long long kmin, unsigned long long* __restrict__ ghist /* [kModeBins] */) {
  constexpr int BINS = kModeBins;
  using K = typename QKey<T>::K;
  __shared__ uint32_t h[BINS];
  for (int d = threadIdx.x; d < BINS; d += kModeBlock) h[d] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kModeBlock;
  uint32_t cand = 0xFFFFFFFFu;
  // (i0 is the same in all lanes of a wave: whole waves take every step, as the ballots below need)
  for (int64_t i0 = ((int64_t)blockIdx.x * (kModeBlock / 64) + (threadIdx.x >> 6)) * 64; i0 < n; i0 += stride) {
    const uint64_t bits = valid ? load_bits64(valid, voff + i0, voff + n) : ~0ull;
    const int64_t i = i0 + lane;
    const bool ok = i < n && ((bits >> lane) & 1ull);
    uint32_t d = 0;
    if (ok) {
      K k;
      QKey<T>::key(v[i], &k);
      d = (uint32_t)((unsigned long long)k - kmin);
      if (d >= (uint32_t)BINS) d = BINS - 1;  // (cannot happen: kmin / kmax come from the same rows; keeps a stray index inside LDS)
    }
    // the lanes that share the wave's candidate bin are counted from one ballot by their first lane (a mode column has a hot value, and LDS
    // atomics on one word serialise): 0.62 instead of 0.76 ms on a single-value column of 1e8 rows, 3 - 4 % slower on evenly spread values
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
  __syncthreads();
  for (int d = threadIdx.x; d < BINS; d += kModeBlock) {
    const uint32_t c = h[d];
    if (c) atomicAdd(&ghist[d], (unsigned long long)c);
  }
}
__global__ void k_mode_bins_to_counts(const unsigned long long* __restrict__ ghist, int64_t R, uint32_t* __restrict__ cnt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += stride) cnt[j] = (uint32_t)ghist[j];
}

// ---------------------------------------------------------------- sort path
// flag[i] = 1 when position i of the sorted order starts a run (i < V: the null tail is cut off by the caller)
template <typename T>
__global__ void k_mode_mark(const T* __restrict__ v, const unsigned long long* __restrict__ order, int64_t V, uint8_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride)
    flag[i] = (i == 0 || !mode_equal(v[order[i]], v[order[i - 1]])) ? 1 : 0;
}
struct FlagPred {
  const uint8_t* flag;
  __device__ bool operator()(int64_t i) const { return flag[i] != 0; }
};
struct StartEmit {
  uint32_t* starts;
  __device__ void operator()(int64_t pos, int64_t i) const { starts[pos] = (uint32_t)i; }
};
__global__ void k_mode_run_counts(const uint32_t* __restrict__ starts, int64_t R, int64_t V, uint32_t* __restrict__ cnt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += stride)
    cnt[j] = (uint32_t)((j + 1 < R ? (int64_t)starts[j + 1] : V) - (int64_t)starts[j]);
}

// ---------------------------------------------------------------- top n over R candidates (count, position)
__global__ void __launch_bounds__(256) k_mode_top(const uint32_t* __restrict__ cnt, int64_t R, unsigned long long* __restrict__ res /* [0] best key, [1] candidates with rows */) {
  unsigned long long best = 0, nz = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += stride) {
    const uint32_t c = cnt[j];
    if (c) {
      ++nz;
      const unsigned long long key = ((unsigned long long)c << 32) | (unsigned long long)(uint32_t)~(uint32_t)j;
      best = key > best ? key : best;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_down(best, d, 64);
    best = o > best ? o : best;
    nz += __shfl_down(nz, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && nz) {
    atomicMax(&res[0], best);
    atomicAdd(&res[1], nz);
  }
}
__global__ void k_mode_sort_keys(const uint32_t* __restrict__ cnt, int64_t R, uint32_t maxc, uint32_t* __restrict__ keys, uint32_t* __restrict__ pos) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += stride) {
    keys[j] = maxc - cnt[j];  // (an empty bin gets the largest key and sorts behind every candidate)
    pos[j] = (uint32_t)j;
  }
}
// winner i: position winners[i] (or pos0 when there is one winner); counting path (order == nullptr): the value is kmin + position
template <typename T>
__global__ void k_mode_emit(const T* __restrict__ v, const unsigned long long* __restrict__ order, const uint32_t* __restrict__ starts,
                            const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ winners, uint32_t pos0, unsigned long long kmin, int64_t k,
                            T* __restrict__ out_modes, long long* __restrict__ out_counts) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += stride) {
    const uint32_t p = winners ? winners[i] : pos0;
    out_counts[i] = (long long)cnt[p];
    out_modes[i] = order ? mode_canonical(v[order[starts[p]]]) : mode_unkey<T>(kmin + p);
  }
}

static void mode_done(pdx_mut_column* out_modes, pdx_mut_column* out_counts, int64_t k) {
  out_modes->length = out_counts->length = k;
  out_modes->null_count = out_counts->null_count = 0;
}

// cnt[R] (device) -> the k = min(n, candidates with rows) winners written to the outputs
template <typename T>
static int mode_top_emit(const T* v, const unsigned long long* order, const uint32_t* starts, const uint32_t* cnt, int64_t R, unsigned long long kmin, int64_t n_want,
                         pdx_mut_column* out_modes, pdx_mut_column* out_counts, Scratch& s, hipStream_t st) {
  unsigned long long* res = s.get<unsigned long long>(2);
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemsetAsync(res, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_mode_top, dim3(grid_for(R, 256, 4)), dim3(256), 0, st, cnt, R, res);
  PDX_LAUNCH_CHECK();
  unsigned long long hres[2];
  PDX_TRY(read_back(hres, res, sizeof(hres), st));
  const int64_t k = std::min<int64_t>(n_want, (int64_t)hres[1]);
  if (k <= 0) return fail(PDX_DEVICE, "pdx_mode: no candidate although a valid row exists");
  const uint32_t maxc = (uint32_t)(hres[0] >> 32);
  const uint32_t* winners = nullptr;
  if (k > 1) {
    uint32_t* kin = s.get<uint32_t>((size_t)R);
    uint32_t* pin = s.get<uint32_t>((size_t)R);
    uint32_t* k0 = s.get<uint32_t>((size_t)R);
    uint32_t* p0 = s.get<uint32_t>((size_t)R);
    uint32_t* k1 = s.get<uint32_t>((size_t)R);
    uint32_t* p1 = s.get<uint32_t>((size_t)R);
    PDX_SCRATCH_CHECK(s);
    hipLaunchKernelGGL(k_mode_sort_keys, dim3(grid_for(R, 256, 4)), dim3(256), 0, st, cnt, R, maxc, kin, pin);
    PDX_LAUNCH_CHECK();
    int bits = 1;
    while (bits < 31 && ((uint64_t)maxc >> bits)) ++bits;
    const uint32_t* ks = kin;
    PDX_TRY((radix_sort_pairs<uint32_t>(kin, pin, k0, p0, k1, p1, R, bits, &ks, &winners, false, s, st)));
  }
  hipLaunchKernelGGL(k_mode_emit<T>, dim3(grid_for(k, 256)), dim3(256), 0, st, v, order, starts, cnt, winners, (uint32_t)~(uint32_t)hres[0], kmin, k,
                     static_cast<T*>(out_modes->values), static_cast<long long*>(out_counts->values));
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  mode_done(out_modes, out_counts, k);
  return PDX_OK;
}

template <typename T>
static int mode_typed(const pdx_column* a, int64_t n_want, int skip_nulls, int64_t min_count, pdx_mut_column* out_modes, pdx_mut_column* out_counts, void* stream,
                      hipStream_t st) {
  const int64_t n = a->length;
  const T* v = static_cast<const T*>(a->values) + a->offset;
  const uint8_t* valid = validity_or_null(a);
  Scratch s;
  PDX_PROFILE("mode", st);
  // ---- first read
  const int grid = grid_for(n, kModeBlock, 16, kModeMaxBlocks);
  ModeScan* part = s.get<ModeScan>((size_t)grid);
  PDX_SCRATCH_CHECK(s);
  hipLaunchKernelGGL(k_mode_scan<T>, dim3(grid), dim3(kModeBlock), 0, st, v, valid, a->offset, n, part);
  PDX_LAUNCH_CHECK();
  std::vector<ModeScan> hp((size_t)grid);
  PDX_TRY(read_back(hp.data(), part, sizeof(ModeScan) * (size_t)grid, st));
  unsigned long long kmin = ~0ull, kmax = 0;
  int64_t V = 0;
  bool any = false;
  for (const ModeScan& p : hp) {
    V += (int64_t)p.valid;
    if (p.any >= 0) {
      kmin = std::min(kmin, p.kmin);
      kmax = std::max(kmax, p.kmax);
      any = true;
    }
  }
  if (V == 0 || V < min_count || (!skip_nulls && V < n)) {
    g_mode_plan = "path=empty";
    mode_done(out_modes, out_counts, 0);
    return PDX_OK;
  }
  // ---- counting path: the width in unsigned 64-bit arithmetic (kmax - kmin < kModeBins, never kmax - kmin + 1: INT64_MIN beside INT64_MAX)
  if constexpr (!QKey<T>::kFloat) if (any && kmax - kmin < (unsigned long long)kModeBins) {
    const int64_t R = (int64_t)(kmax - kmin) + 1;
    unsigned long long* ghist = s.get<unsigned long long>((size_t)kModeBins);
    uint32_t* cnt = s.get<uint32_t>((size_t)kModeBins);
    PDX_SCRATCH_CHECK(s);
    PDX_HIP(hipMemsetAsync(ghist, 0, sizeof(unsigned long long) * (size_t)kModeBins, st));
    hipLaunchKernelGGL(k_mode_hist<T>, dim3(grid_for(n, kModeBlock, 16, kModeMaxBlocks)), dim3(kModeBlock), 0, st, v, valid, a->offset, n, kmin, ghist);
    hipLaunchKernelGGL(k_mode_bins_to_counts, dim3(grid_for(R, 256)), dim3(256), 0, st, ghist, R, cnt);
    PDX_LAUNCH_CHECK();
    g_mode_plan = "path=count bins=" + std::to_string(kModeBins) + " width=" + std::to_string(R);
    return mode_top_emit<T>(v, nullptr, nullptr, cnt, R, kmin, n_want, out_modes, out_counts, s, st);
  }
  // ---- sort path
  unsigned long long* order = s.get<unsigned long long>((size_t)n);
  uint8_t* flag = s.get<uint8_t>((size_t)V);
  uint32_t* starts = s.get<uint32_t>((size_t)V);
  PDX_SCRATCH_CHECK(s);
  pdx_mut_column om{};
  om.dtype = PDX_UINT64;
  om.length = n;
  om.values = order;
  if (sizeof(T) == 8) PDX_TRY(pdx_argsort(a, 1, &om, stream));
  else PDX_TRY(pdx_sort_indices(a, 1, nullptr, &om, nullptr, stream));
  note_stream(st);
  hipLaunchKernelGGL(k_mode_mark<T>, dim3(grid_for(V, 256, 4)), dim3(256), 0, st, v, order, V, flag);
  PDX_LAUNCH_CHECK();
  int64_t R = 0;
  PDX_TRY(compact_indices(V, FlagPred{flag}, StartEmit{starts}, &R, s, st));
  if (R <= 0) return fail(PDX_DEVICE, "pdx_mode: no run although a valid row exists");
  uint32_t* cnt = s.get<uint32_t>((size_t)R);
  PDX_SCRATCH_CHECK(s);
  hipLaunchKernelGGL(k_mode_run_counts, dim3(grid_for(R, 256, 4)), dim3(256), 0, st, starts, R, V, cnt);
  PDX_LAUNCH_CHECK();
  g_mode_plan = "path=sort runs=" + std::to_string(R);
  return mode_top_emit<T>(v, order, starts, cnt, R, 0ull, n_want, out_modes, out_counts, s, st);
}

static int mode_bool(const pdx_column* a, int64_t n_want, int skip_nulls, int64_t min_count, pdx_mut_column* out_modes, pdx_mut_column* out_counts, hipStream_t st) {
  const int64_t n = a->length;
  Scratch s;
  unsigned long long* res = s.get<unsigned long long>(2);
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemsetAsync(res, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_mode_bool, dim3(grid_for((n + 63) / 64, kModeBlock)), dim3(kModeBlock), 0, st, static_cast<const uint8_t*>(a->values), validity_or_null(a),
                     a->offset, n, res);
  PDX_LAUNCH_CHECK();
  unsigned long long h[2];
  PDX_TRY(read_back(h, res, sizeof(h), st));
  const int64_t V = (int64_t)h[1], t = (int64_t)h[0], f = V - t;
  if (V == 0 || V < min_count || (!skip_nulls && V < n)) {
    g_mode_plan = "path=empty";
    mode_done(out_modes, out_counts, 0);
    return PDX_OK;
  }
  int vals[2] = {0, 1};
  long long cs[2] = {f, t};
  if (t > f) {  // (a tie: false < true)
    std::swap(vals[0], vals[1]);
    std::swap(cs[0], cs[1]);
  }
  const int k = (int)std::min<int64_t>(n_want, (f > 0) + (t > 0));
  hipLaunchKernelGGL(k_mode_emit_bool, dim3(1), dim3(64), 0, st, static_cast<uint8_t*>(out_modes->values), static_cast<long long*>(out_counts->values), k, vals[0],
                     vals[1], cs[0], cs[1]);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  g_mode_plan = "path=bool";
  mode_done(out_modes, out_counts, k);
  return PDX_OK;
}

// ---------------------------------------------------------------- group form
// (group, value, row) order, nulls at each group's tail: a run breaks where the group id, the validity or the value changes
template <typename T>
__global__ void k_gm_mark(const T* __restrict__ v, const uint8_t* __restrict__ valid, int64_t voff, const uint32_t* __restrict__ keys,
                          const uint32_t* __restrict__ rows, int64_t n, uint8_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    bool start = i == 0;
    if (!start) {
      const uint32_t r = rows[i], p = rows[i - 1];
      const bool ok = !valid || bit_get(valid, voff + r), okp = !valid || bit_get(valid, voff + p);
      start = keys[i] != keys[i - 1] || ok != okp || (ok && !mode_equal(v[r], v[p]));
    }
    flag[i] = start ? 1 : 0;
  }
}
// one 64-bit max per run of valid rows into its group's slot: the most rows, then the lowest position (= the smallest value, NaN last)
__global__ void k_gm_best(const uint8_t* __restrict__ valid, int64_t voff, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ rows,
                          const uint32_t* __restrict__ starts, int64_t R, int64_t n, unsigned long long* __restrict__ best /* [G], zeroed */) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += stride) {
    const int64_t s = starts[j], e = j + 1 < R ? (int64_t)starts[j + 1] : n;
    if (valid && !bit_get(valid, voff + rows[s])) continue;
    atomicMax(&best[keys[s]], ((unsigned long long)(e - s) << 32) | (unsigned long long)(uint32_t)~(uint32_t)s);
  }
}
template <typename T>
__global__ void k_gm_emit(const T* __restrict__ v, const uint32_t* __restrict__ rows, const unsigned long long* __restrict__ best, int64_t G,
                          T* __restrict__ out_modes, long long* __restrict__ out_counts, uint8_t* __restrict__ ok) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += stride) {
    const unsigned long long b = best[g];
    ok[g] = b ? 1 : 0;
    out_counts[g] = (long long)(b >> 32);
    out_modes[g] = b ? mode_canonical(v[rows[(uint32_t)~(uint32_t)b]]) : T(0);
  }
}
template <typename T>
static int groupby_mode_typed(pdx_groupby* gb, const pdx_column* values, pdx_mut_column* out_modes, pdx_mut_column* out_counts, void* stream, hipStream_t st) {
  const int64_t n = values->length, G = pdx_groupby_num_groups(gb);
  Scratch s;
  uint8_t* flag = s.get<uint8_t>((size_t)n);
  uint32_t* starts = s.get<uint32_t>((size_t)n);
  unsigned long long* best = s.get<unsigned long long>((size_t)G);
  uint8_t* ok = s.get<uint8_t>((size_t)G);
  unsigned long long* nulls = s.get<unsigned long long>(1);
  PDX_SCRATCH_CHECK(s);
  const uint32_t* ks = nullptr;
  const uint32_t* vs = nullptr;
  PDX_TRY(build_group_value_order(gb, values, &ks, &vs, s, stream, st));
  PDX_PROFILE("groupby_mode", st);
  const T* v = static_cast<const T*>(values->values) + values->offset;
  const uint8_t* valid = validity_or_null(values);
  hipLaunchKernelGGL(k_gm_mark<T>, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, v, valid, values->offset, ks, vs, n, flag);
  PDX_LAUNCH_CHECK();
  int64_t R = 0;
  PDX_TRY(compact_indices(n, FlagPred{flag}, StartEmit{starts}, &R, s, st));
  PDX_HIP(hipMemsetAsync(best, 0, sizeof(unsigned long long) * (size_t)G, st));
  PDX_HIP(hipMemsetAsync(nulls, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_gm_best, dim3(grid_for(R, 256, 4)), dim3(256), 0, st, valid, values->offset, ks, vs, starts, R, n, best);
  hipLaunchKernelGGL(k_gm_emit<T>, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, v, vs, best, G, static_cast<T*>(out_modes->values),
                     static_cast<long long*>(out_counts->values), ok);
  hipLaunchKernelGGL(k_go_pack, dim3(grid_for((G + 7) / 8, 256)), dim3(256), 0, st, ok, G, static_cast<uint8_t*>(out_modes->validity), nulls);
  PDX_LAUNCH_CHECK();
  unsigned long long hn = 0;
  PDX_TRY(read_back(&hn, nulls, sizeof(hn), st));
  if (hn && !out_modes->validity) {  // (known only now: the rows have been written, so the outputs are handed back empty)
    out_modes->length = out_counts->length = 0;
    out_modes->null_count = out_counts->null_count = -1;
    return fail(PDX_INVALID, "pdx_groupby_mode: a group has no valid value and the output has no validity buffer");
  }
  out_modes->length = out_counts->length = G;
  out_modes->null_count = (int64_t)hn;
  out_counts->null_count = 0;
  return PDX_OK;
}

}  // namespace pdx

using namespace pdx;

extern "C" int pdx_mode(const pdx_column* a, int64_t n, int skip_nulls, int64_t min_count, pdx_mut_column* out_modes, pdx_mut_column* out_counts, void* stream) {
  if (!a) return fail(PDX_INVALID, "pdx_mode: null column");
  if (a->dtype == PDX_TIMESTAMP_NS) return fail(PDX_NOT_IMPLEMENTED, "Function 'mode' has no kernel matching input types (timestamp[ns])");
  if (n <= 0) return fail(PDX_INVALID, "ModeOptions::n must be strictly positive");
  PDX_TRY(check_column(a, "pdx_mode", true));
  if (!out_modes || !out_counts) return fail(PDX_INVALID, "pdx_mode: null output");
  if (a->length > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_mode: more than 2^31-1 rows per call is not supported yet");
  if (out_modes->dtype != a->dtype) return fail(PDX_INVALID, "pdx_mode: the modes have the input's dtype");
  if (out_counts->dtype != PDX_INT64) return fail(PDX_INVALID, "pdx_mode: the counts are int64");
  const int64_t cap = std::min<int64_t>(n, a->length);
  if (out_modes->length < cap || out_counts->length < cap || (cap && (!out_modes->values || !out_counts->values)))
    return fail(PDX_INVALID, "pdx_mode: output too small");
  hipStream_t st = as_stream(stream);
  if (a->length == 0) {
    g_mode_plan = "path=empty";
    mode_done(out_modes, out_counts, 0);
    return PDX_OK;
  }
  switch (a->dtype) {
    case PDX_BOOL: return mode_bool(a, n, skip_nulls, min_count, out_modes, out_counts, st);
    case PDX_FLOAT64: return mode_typed<double>(a, n, skip_nulls, min_count, out_modes, out_counts, stream, st);
    case PDX_INT64: return mode_typed<int64_t>(a, n, skip_nulls, min_count, out_modes, out_counts, stream, st);
    case PDX_UINT64: return mode_typed<uint64_t>(a, n, skip_nulls, min_count, out_modes, out_counts, stream, st);
    case PDX_FLOAT32: return mode_typed<float>(a, n, skip_nulls, min_count, out_modes, out_counts, stream, st);
    case PDX_INT32: return mode_typed<int32_t>(a, n, skip_nulls, min_count, out_modes, out_counts, stream, st);
    default: return fail(PDX_NOT_IMPLEMENTED, "pdx_mode: unsupported dtype");
  }
}

extern "C" int pdx_mode_last_plan(char* buf, size_t buf_len) {
  if (!buf || !buf_len) return fail(PDX_INVALID, "pdx_mode_last_plan: null buffer");
  snprintf(buf, buf_len, "%s", g_mode_plan.c_str());
  return PDX_OK;
}

extern "C" int pdx_groupby_mode(pdx_groupby* gb, const pdx_column* values, pdx_mut_column* out_modes, pdx_mut_column* out_counts, void* stream) {
  if (!gb) return fail(PDX_INVALID, "pdx_groupby_mode: null handle");
  if (!values) return fail(PDX_INVALID, "pdx_groupby_mode: null column");
  if (values->dtype != PDX_INT64 && values->dtype != PDX_UINT64 && values->dtype != PDX_FLOAT64)
    return fail(PDX_NOT_IMPLEMENTED, std::string("pdx_groupby_mode: dtype ") + dtype_name(values->dtype) + " is not supported");
  PDX_TRY(check_column(values, "pdx_groupby_mode"));
  if (!out_modes || !out_counts) return fail(PDX_INVALID, "pdx_groupby_mode: null output");
  const int64_t n = pdx_groupby_num_rows(gb), G = pdx_groupby_num_groups(gb);
  if (values->length != n) return fail(PDX_INVALID, "pdx_groupby_mode: values and keys differ in length");
  if (out_modes->dtype != values->dtype) return fail(PDX_INVALID, "pdx_groupby_mode: the modes have the values' dtype");
  if (out_counts->dtype != PDX_INT64) return fail(PDX_INVALID, "pdx_groupby_mode: the counts are int64");
  if (out_modes->length < G || out_counts->length < G || (G && (!out_modes->values || !out_counts->values)))
    return fail(PDX_INVALID, "pdx_groupby_mode: output too small");
  hipStream_t st = as_stream(stream);
  if (G == 0) {  // (a handle over no rows has no groups)
    out_modes->length = out_counts->length = 0;
    out_modes->null_count = out_counts->null_count = 0;
    return PDX_OK;
  }
  switch (values->dtype) {
    case PDX_FLOAT64: return groupby_mode_typed<double>(gb, values, out_modes, out_counts, stream, st);
    case PDX_INT64: return groupby_mode_typed<int64_t>(gb, values, out_modes, out_counts, stream, st);
    default: return groupby_mode_typed<uint64_t>(gb, values, out_modes, out_counts, stream, st);
  }
}
