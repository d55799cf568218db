// align.hip -- index alignment for binary operations on UNEQUAL indexes (the first caller-side "next" row).
//
// Reference: Series::broadcast (src/series.cpp:212-227) = Concatenate(index_a, index_b) -> Unique -> array_sort_indices
// (ascending) -> Take, then Series::reindex (src/series.cpp:1255-1309) of both operands onto that index: a host
// std::unordered_map<int64, int64> built with insert_or_assign (so the LAST position of a duplicated label wins) and one
// GetScalar/AppendScalar per new label; labels that are absent become null.
//
// Device form: both steps are the group-by dictionary (csrc/groupby.hip) applied to a concatenation.
//   union   : uniques of concat(a, b) (first-occurrence dictionary), then a stable LSD radix sort of the 64-bit labels
//             (sort_packed64 below: eight 8-bit passes over (low key half, high key half | row) elements, constant digits skipped)
//   reindex : group ids of concat(reverse(old), new); a new label is present iff its group's first row lies in the reversed old
//             part, and that first row is the LAST position of the label in the old index.  Output = take indices with a
//             validity bitmap (absent -> null); values then go through pdx_take, whose null indices yield null rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "compact.hpp"
#include "pdx/abi.h"
#include "pdx_common.hpp"
#include "radix_sort.hpp"

namespace pdx {

__global__ void k_concat2_i64(const long long* __restrict__ a, int64_t na, int reverse_a, const long long* __restrict__ b, int64_t nb,
                              long long* __restrict__ out) {
  const int64_t n = na + nb, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = i < na ? a[reverse_a ? na - 1 - i : i] : b[i - na];
}
__global__ void k_gather_labels(const long long* __restrict__ labels, const uint32_t* __restrict__ perm, int64_t n, long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = labels[perm[i]];
}
__global__ void k_reindex_emit(const uint32_t* __restrict__ gids, const int64_t* __restrict__ first_rows, int64_t n_old, int64_t n_new,
                               long long* __restrict__ out_idx, uint8_t* __restrict__ ok) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_new; j += stride) {
    const int64_t f = first_rows[gids[n_old + j]];
    const bool present = f < n_old;
    out_idx[j] = present ? n_old - 1 - f : 0;
    ok[j] = present;
  }
}

// ---- 64-bit stable sort with row numbers.  An element is (lo: low 32 key bits, pay: high 32 key bits << 32 | row): four LSD passes on
// `lo` carry the payload along, four more take their digit from the payload's own high half (k_radix_scatter PAYLOAD_DIGIT), so
// the keys are never gathered through a permutation (the three-round form did: k_label_chunk read keys[perm[i]], ten 16 B/row
// passes + four random gathers = 13.5 ms per 1e8 rows).  Digits that are equal in every key (OR == AND over the column) are skipped.

// the order-preserving unsigned image of a value (ascending: as is, descending: complemented) and its class (0 number, 1 NaN,
// 2 null): numbers first, then NaNs, then nulls in BOTH orders, as Arrow's array_sort_indices places them
__device__ __forceinline__ unsigned long long sort_image(unsigned long long u, bool is_null, int dtype, int descending, int* cls) {
  *cls = 0;
  if (is_null) {
    *cls = 2;
    return 0;
  }
  if (dtype == PDX_FLOAT64) {
    const double x = __longlong_as_double((long long)u);
    if (x != x) {
      *cls = 1;
      return 0;
    }
    if (x == 0.0) u = 0;  // -0.0 and 0.0 compare equal: one key, so the stable sort keeps their row order
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  } else if (dtype != PDX_UINT64) {
    u ^= 0x8000000000000000ull;  // int64 / timestamp
  }
  return descending ? ~u : u;
}
struct SortStats {
  unsigned long long bits_or, bits_and;  // over the keys of class 0
  unsigned long long others;             // rows of class 1 / 2
};
__device__ __forceinline__ void sort_stats_flush(SortStats* st, unsigned long long o, unsigned long long a, unsigned long long others) {
  for (int d = 32; d >= 1; d >>= 1) {
    o |= __shfl_xor(o, d, 64);
    a &= __shfl_xor(a, d, 64);
    others += __shfl_xor(others, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicOr(&st->bits_or, o);
    atomicAnd(&st->bits_and, a);
    if (others) atomicAdd(&st->others, others);
  }
}
// every row: class byte (cls8 != nullptr) and -- when lo / pay are given -- the packed element at the row's own position
__global__ void k_sort_pack(const unsigned long long* __restrict__ v, const uint8_t* __restrict__ valid, int64_t off, int64_t n, int dtype, int descending,
                            unsigned long long flip, uint8_t* __restrict__ cls8, uint32_t* __restrict__ lo, unsigned long long* __restrict__ pay,
                            SortStats* __restrict__ stats) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long o = 0, a = ~0ull, others = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int c;
    const unsigned long long u = sort_image(v[i] ^ flip, valid && !bit_get(valid, off + i), dtype, descending, &c);
    if (cls8) cls8[i] = (uint8_t)c;
    if (c == 0) {
      o |= u;
      a &= u;
      if (lo) {
        lo[i] = (uint32_t)u;
        pay[i] = (u & 0xFFFFFFFF00000000ull) | (unsigned long long)i;
      }
    } else {
      ++others;
    }
  }
  sort_stats_flush(stats, o, a, others);
}
struct ClassPred {
  const uint8_t* cls8;
  int c;
  __device__ bool operator()(int64_t i) const { return cls8[i] == c; }
};
struct PackEmit {  // the numbers, compacted in row order
  const unsigned long long* v;
  int dtype, descending;
  uint32_t* lo;
  unsigned long long* pay;
  __device__ void operator()(int64_t pos, int64_t i) const {
    int c;
    const unsigned long long u = sort_image(v[i], false, dtype, descending, &c);
    lo[pos] = (uint32_t)u;
    pay[pos] = (u & 0xFFFFFFFF00000000ull) | (unsigned long long)i;
  }
};
struct RowEmit {  // NaN / null rows behind the numbers, in row order
  unsigned long long* out;
  int64_t base;
  __device__ void operator()(int64_t pos, int64_t i) const { out[base + pos] = (unsigned long long)i; }
};
__global__ void k_pay_rows_u64(const unsigned long long* __restrict__ pay, int64_t n, unsigned long long* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = pay[i] & 0xFFFFFFFFull;
}
__global__ void k_pay_rows_u32(const unsigned long long* __restrict__ pay, int64_t n, uint32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (uint32_t)pay[i];
}
// Sorts the n packed elements (lo0, pay0) by their 64-bit key; `varying` = key bits that differ somewhere.  *sorted points at the
// payloads in key order (one of the ping-pong buffers).  This form works in buffers of the caller's: lo1 / pay1 hold n elements, hist
// ntiles << 8 and chunk (nchunks + 1) << 8 counters; *passes (optional) grows by the radix passes issued.
static int sort_packed64_in(uint32_t* lo0, unsigned long long* pay0, uint32_t* lo1, unsigned long long* pay1, uint32_t* hist, uint32_t* chunk, int64_t n,
                            unsigned long long varying, hipStream_t st, const unsigned long long** sorted, int* passes) {
  const uint32_t* kin = lo0;
  const unsigned long long* vin = pay0;
  int last_lo = -1;
  for (int d = 0; d < 4; ++d)
    if ((varying >> (8 * d)) & 0xFFull) last_lo = d;
  for (int d = 0; d < 8; ++d) {
    if (!((varying >> (8 * d)) & 0xFFull)) continue;
    unsigned long long* vout = vin == pay0 ? pay1 : pay0;
    if (d < 4) {
      uint32_t* kout = kin == lo0 ? lo1 : lo0;
      PDX_TRY((radix_pass_dispatch<uint64_t>(8, kin, reinterpret_cast<const uint64_t*>(vin), kout, reinterpret_cast<uint64_t*>(vout), n, 8 * d, d != last_lo,
                                             hist, chunk, st)));
      if (d != last_lo) kin = kout;
    } else {
      PDX_TRY((radix_pass_payload_hi<8>(reinterpret_cast<const uint64_t*>(vin), reinterpret_cast<uint64_t*>(vout), n, 8 * (d - 4), hist, chunk, st)));
    }
    if (passes) ++*passes;
    vin = vout;
  }
  *sorted = vin;
  return PDX_OK;
}
static int sort_packed64(uint32_t* lo0, unsigned long long* pay0, int64_t n, unsigned long long varying, Scratch& s, hipStream_t st,
                         const unsigned long long** sorted) {
  *sorted = pay0;
  if (n <= 1 || varying == 0) return PDX_OK;
  const int64_t ntiles = ceil_div(n, kSortTile), nchunks = ceil_div(ntiles, kColChunk);
  uint32_t* lo1 = s.get<uint32_t>((size_t)n);
  unsigned long long* pay1 = s.get<unsigned long long>((size_t)n);
  uint32_t* hist = s.get<uint32_t>((size_t)ntiles << 8);
  uint32_t* chunk = s.get<uint32_t>((size_t)(nchunks + 1) << 8);
  PDX_SCRATCH_CHECK(s);
  return sort_packed64_in(lo0, pay0, lo1, pay1, hist, chunk, n, varying, st, sorted, nullptr);
}
// perm[i] = index of the i-th smallest label (labels ^ flip in unsigned order), stable
static int argsort_labels64(const long long* labels, int64_t n, unsigned long long flip, uint32_t* perm, Scratch& s, hipStream_t st) {
  uint32_t* lo = s.get<uint32_t>((size_t)n);
  unsigned long long* pay = s.get<unsigned long long>((size_t)n);
  SortStats* stats = s.get<SortStats>(1);
  PDX_SCRATCH_CHECK(s);
  const SortStats init{0ull, ~0ull, 0ull};
  SortStats h{};
  PDX_HIP(hipMemcpyAsync(stats, &init, sizeof(init), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_sort_pack, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, reinterpret_cast<const unsigned long long*>(labels), (const uint8_t*)nullptr,
                     (int64_t)0, n, (int)PDX_UINT64, 0, flip, (uint8_t*)nullptr, lo, pay, stats);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipMemcpyAsync(&h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));
  const unsigned long long* sorted = nullptr;
  PDX_TRY(sort_packed64(lo, pay, n, h.bits_or ^ h.bits_and, s, st, &sorted));
  hipLaunchKernelGGL(k_pay_rows_u32, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, sorted, n, perm);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

static int check_index(const pdx_column* c, const char* what) {
  PDX_TRY(check_column(c, what));
  if (!is_int_like(c->dtype)) return fail(PDX_NOT_IMPLEMENTED, std::string(what) + ": index must be int64 / uint64 / timestamp[ns]");
  if (validity_or_null(c)) return fail(PDX_NOT_IMPLEMENTED, std::string(what) + ": null index labels are not supported");
  return PDX_OK;
}
struct GroupByOwner {  // RAII for the internal dictionary handle
  pdx_groupby* h = nullptr;
  ~GroupByOwner() {
    if (h) pdx_groupby_destroy(h);
  }
};

__global__ void k_mark_groups(const uint32_t* __restrict__ gids, int64_t from, int64_t n, uint8_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = from + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) flag[gids[i]] = 1;
}
// groups are numbered by first occurrence in concat(reverse(a), b): walking them backwards walks a's LAST positions upwards
struct IntersectPred {
  const int64_t* first_rows;
  const uint8_t* in_b;
  int64_t G, n_a;
  __device__ bool operator()(int64_t i) const {
    const int64_t g = G - 1 - i;
    return first_rows[g] < n_a && in_b[g];
  }
};
struct IntersectEmit {
  const int64_t* first_rows;
  const long long* a;
  int64_t G, n_a;
  long long* out;
  __device__ void operator()(int64_t pos, int64_t i) const { out[pos] = a[n_a - 1 - first_rows[G - 1 - i]]; }
};

// ---- multi-key sort (pdx_sort_indices): range-compressed composite keys.  Per key column the ascending sort_image minus the column's
// minimum needs only bit_length(max - min) bits; a 2-bit class field (0 number, 1 NaN, 2 null) above it, present only where the column
// has a NaN / null row, places those rows as Arrow's sort_indices does.  The fields of several keys concatenated are ONE 64-bit key of
// sort_packed64; keys wider than a word sort as an LSD chain of such rounds, least significant fields first (stable passes: the chain
// is the lexicographic order, full ties keep their row order).
struct SortKeyStats {
  unsigned long long min, max;    // of the ascending image over the rows of class 0 (~0 / 0 when there is none)
  unsigned long long nans, nulls;
};
struct SortKeyDesc {  // one key column as a round reads it; wave-uniform (kernel argument)
  const void* v;         // values + offset
  const uint8_t* valid;  // bitmap or nullptr
  long long off;         // bit offset into valid
  unsigned long long base;  // value field = img - base (ascending: the minimum) or base - img (descending: the maximum)
  int dtype, descending;
  int vshift, vwidth;  // value field: position in the round's key, width (0: not in this round)
  int cshift;          // class field position (-1: not in this round)
  int pad;
};
struct SortKeyDescs {
  SortKeyDesc k[PDX_SORT_MAX_KEYS];
  int n;
};
// the ascending image and class of row `row`; 4-byte keys widen here: int32 sign-extends, float32 converts to double (exact: order, NaN and
// the -0 rule carry over)
__device__ __forceinline__ unsigned long long sort_key_image(const SortKeyDesc& d, int64_t row, bool need_value, int* cls) {
  const bool is_null = d.valid && !bit_get(d.valid, d.off + row);
  unsigned long long u = 0;
  int dt = d.dtype;
  if (need_value) {
    if (dt == PDX_INT32) {
      u = (unsigned long long)(long long)static_cast<const int32_t*>(d.v)[row];
      dt = PDX_INT64;
    } else if (dt == PDX_FLOAT32) {
      u = (unsigned long long)__double_as_longlong((double)static_cast<const float*>(d.v)[row]);
      dt = PDX_FLOAT64;
    } else {
      u = static_cast<const unsigned long long*>(d.v)[row];
    }
  } else {
    dt = PDX_UINT64;  // only the class is wanted and only a null makes one here
  }
  return sort_image(u, is_null, dt, 0, cls);
}
// grid.y = key: every key column is read once; per wave one 64-bit atomic per statistic
__global__ void k_sort_key_stats(const SortKeyDescs keys, int64_t n, SortKeyStats* __restrict__ stats) {
  const SortKeyDesc& d = keys.k[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long mn = ~0ull, mx = 0ull, nans = 0, nulls = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int c;
    const unsigned long long u = sort_key_image(d, i, true, &c);
    if (c == 0) {
      mn = u < mn ? u : mn;
      mx = u > mx ? u : mx;
    }
    nans += c == 1;
    nulls += c == 2;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long omn = __shfl_xor(mn, s, 64), omx = __shfl_xor(mx, s, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    nans += __shfl_xor(nans, s, 64);
    nulls += __shfl_xor(nulls, s, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    SortKeyStats* st = stats + blockIdx.y;
    if (mn <= mx) {
      atomicMin(&st->min, mn);
      atomicMax(&st->max, mx);
    }
    if (nans) atomicAdd(&st->nans, nans);
    if (nulls) atomicAdd(&st->nulls, nulls);
  }
}
// one round: the (lo, pay) element of sort_packed64 at position i for the row at position i of the previous round's order (prev ==
// nullptr: row i itself).  The loop over the fields is wave-uniform; a row that is no number has value field 0.
__global__ void k_sort_compose(const SortKeyDescs keys, const unsigned long long* __restrict__ prev, int64_t n, uint32_t* __restrict__ lo,
                               unsigned long long* __restrict__ pay) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long row = prev ? (prev[i] & 0xFFFFFFFFull) : (unsigned long long)i;
    unsigned long long key = 0;
    for (int f = 0; f < keys.n; ++f) {
      const SortKeyDesc& d = keys.k[f];
      int c;
      const unsigned long long u = sort_key_image(d, (int64_t)row, d.vwidth > 0 || d.dtype == PDX_FLOAT64 || d.dtype == PDX_FLOAT32, &c);
      if (d.vwidth > 0) key |= (c == 0 ? (d.descending ? d.base - u : u - d.base) : 0ull) << d.vshift;
      if (d.cshift >= 0) key |= (unsigned long long)c << d.cshift;
    }
    lo[i] = (uint32_t)key;
    pay[i] = (key & 0xFFFFFFFF00000000ull) | row;
  }
}

}  // namespace pdx

using namespace pdx;

extern "C" {

int pdx_index_union(const pdx_column* a, const pdx_column* b, int sort, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_index(a, "pdx_index_union"));
  PDX_TRY(check_index(b, "pdx_index_union"));
  if (!out) return fail(PDX_INVALID, "pdx_index_union: null output");
  if (a->dtype != b->dtype) return fail(PDX_INVALID, "type(NewIndex) != type(CurrentIndex).");
  const int64_t na = a->length, nb = b->length, n = na + nb;
  if (out->dtype != a->dtype) return fail(PDX_INVALID, "pdx_index_union: output dtype must be the index dtype");
  if (out->length < n || (n && !out->values)) return fail(PDX_INVALID, "pdx_index_union: output must hold a.length + b.length labels");
  out->length = 0;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_index_union: more than 2^31-1 labels per call is not supported yet");
  hipStream_t st = as_stream(stream);
  Scratch s;
  long long* cat = s.get<long long>((size_t)n);
  PDX_SCRATCH_CHECK(s);
  hipLaunchKernelGGL(k_concat2_i64, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, static_cast<const long long*>(a->values) + a->offset, na, 0,
                     static_cast<const long long*>(b->values) + b->offset, nb, cat);
  PDX_LAUNCH_CHECK();
  // Unique (first-occurrence dictionary)
  pdx_column cc{};
  cc.dtype = a->dtype;
  cc.length = n;
  cc.values = cat;
  GroupByOwner gb;
  PDX_TRY(pdx_groupby_create(&cc, stream, &gb.h));
  const int64_t G = pdx_groupby_num_groups(gb.h);
  long long* uniq = s.get<long long>((size_t)G);
  uint8_t* uniq_ok = s.get<uint8_t>((size_t)(G + 7) / 8 + 8);
  PDX_SCRATCH_CHECK(s);
  pdx_mut_column um{};
  um.dtype = a->dtype;
  um.length = G;
  um.values = uniq;
  um.validity = uniq_ok;
  PDX_TRY(pdx_groupby_unique_keys(gb.h, &um, stream));
  if (!sort) {  // Series::union_ (src/series.cpp:782-798): Unique(Concatenate) as is, first-occurrence order
    PDX_HIP(hipMemcpyAsync(out->values, uniq, (size_t)G * sizeof(long long), hipMemcpyDeviceToDevice, st));
    if (out->validity) PDX_HIP(hipMemsetAsync(out->validity, 0xFF, (size_t)((G + 7) / 8), st));
    PDX_HIP(hipStreamSynchronize(st));
    out->length = G;
    return PDX_OK;
  }
  // array_sort_indices ascending + Take: stable LSD sort of the 64-bit labels, three rounds through the 32-bit pair sort
  uint32_t* perm = s.get<uint32_t>((size_t)G);
  PDX_SCRATCH_CHECK(s);
  const unsigned long long flip = a->dtype == PDX_UINT64 ? 0ull : 0x8000000000000000ull;
  PDX_TRY(argsort_labels64(uniq, G, flip, perm, s, st));
  hipLaunchKernelGGL(k_gather_labels, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, uniq, perm, G, static_cast<long long*>(out->values));
  PDX_LAUNCH_CHECK();
  if (out->validity) PDX_HIP(hipMemsetAsync(out->validity, 0xFF, (size_t)((G + 7) / 8), st));
  PDX_HIP(hipStreamSynchronize(st));
  out->length = G;
  return PDX_OK;
}

int pdx_argsort(const pdx_column* col, int ascending, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_column(col, "pdx_argsort"));
  if (!out) return fail(PDX_INVALID, "pdx_argsort: null output");
  if (col->dtype != PDX_INT64 && col->dtype != PDX_UINT64 && col->dtype != PDX_FLOAT64 && col->dtype != PDX_TIMESTAMP_NS)
    return fail(PDX_NOT_IMPLEMENTED, "pdx_argsort: int64 / uint64 / float64 / timestamp[ns] columns only");
  const int64_t n = col->length;
  if (out->dtype != PDX_UINT64) return fail(PDX_INVALID, "pdx_argsort: the indices are uint64");
  if (out->length < n || (n && !out->values)) return fail(PDX_INVALID, "pdx_argsort: output too small");
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_argsort: more than 2^31-1 rows per call is not supported yet");
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  hipStream_t st = as_stream(stream);
  Scratch s;
  const uint8_t* valid = validity_or_null(col);
  const bool classes = valid || col->dtype == PDX_FLOAT64;  // NaNs / nulls go behind the numbers, in row order
  const unsigned long long* v = static_cast<const unsigned long long*>(col->values) + col->offset;
  unsigned long long* outp = static_cast<unsigned long long*>(out->values);
  uint32_t* lo = s.get<uint32_t>((size_t)n);
  unsigned long long* pay = s.get<unsigned long long>((size_t)n);
  uint8_t* cls8 = classes ? s.get<uint8_t>((size_t)n) : nullptr;
  SortStats* stats = s.get<SortStats>(1);
  PDX_SCRATCH_CHECK(s);
  const SortStats init{0ull, ~0ull, 0ull};
  SortStats h{};
  PDX_HIP(hipMemcpyAsync(stats, &init, sizeof(init), hipMemcpyHostToDevice, st));
  // one pass: class bytes, the packed elements at their own positions (all that is needed when every row is a number), key statistics
  hipLaunchKernelGGL(k_sort_pack, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, v, valid, col->offset, n, col->dtype, ascending ? 0 : 1, 0ull, cls8, lo, pay,
                     stats);
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipMemcpyAsync(&h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));
  int64_t n0 = n;
  if (h.others) {  // numbers compacted to the front (row order), NaN rows, then null rows straight into the output
    int64_t n1 = 0, n2 = 0;
    PDX_TRY(compact_indices(n, ClassPred{cls8, 0}, PackEmit{v, col->dtype, ascending ? 0 : 1, lo, pay}, &n0, s, st));
    PDX_TRY(compact_indices(n, ClassPred{cls8, 1}, RowEmit{outp, n0}, &n1, s, st));
    PDX_TRY(compact_indices(n, ClassPred{cls8, 2}, RowEmit{outp, n0 + n1}, &n2, s, st));
    if (n0 + n1 + n2 != n) return fail(PDX_DEVICE, "pdx_argsort: class counts do not add up");
  }
  const unsigned long long* sorted = nullptr;
  PDX_TRY(sort_packed64(lo, pay, n0, h.bits_or ^ h.bits_and, s, st, &sorted));
  if (n0) hipLaunchKernelGGL(k_pay_rows_u64, dim3(grid_for(n0, 256, 4)), dim3(256), 0, st, sorted, n0, outp);
  PDX_LAUNCH_CHECK();
  if (out->validity) PDX_HIP(hipMemsetAsync(out->validity, 0xFF, (size_t)((n + 7) / 8), st));
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

int pdx_sort_indices(const pdx_column* keys, int nkeys, const int* descending, pdx_mut_column* out, pdx_sort_info* info, void* stream) {
  if (info) *info = pdx_sort_info{0, 0, 0, 0};
  if (nkeys < 1 || nkeys > PDX_SORT_MAX_KEYS) return fail(PDX_INVALID, "pdx_sort_indices: between 1 and " + std::to_string(PDX_SORT_MAX_KEYS) + " sort keys");
  if (!keys) return fail(PDX_INVALID, "pdx_sort_indices: null keys");
  if (!out) return fail(PDX_INVALID, "pdx_sort_indices: null output");
  for (int k = 0; k < nkeys; ++k) {
    const int dt = keys[k].dtype;
    if (dt != PDX_INT64 && dt != PDX_UINT64 && dt != PDX_FLOAT64 && dt != PDX_TIMESTAMP_NS && dt != PDX_INT32 && dt != PDX_FLOAT32)
      return fail(PDX_NOT_IMPLEMENTED, "pdx_sort_indices: int64 / uint64 / float64 / timestamp[ns] / int32 / float32 keys only");
    if (keys[k].length < 0 || keys[k].offset < 0) return fail(PDX_INVALID, "pdx_sort_indices: negative length/offset");
    if (keys[k].length != keys[0].length) return fail(PDX_INVALID, "pdx_sort_indices: all keys must have the same length");
  }
  const int64_t n = keys[0].length;
  if (out->dtype != PDX_UINT64) return fail(PDX_INVALID, "pdx_sort_indices: the indices are uint64");
  if (out->length < n) return fail(PDX_INVALID, "pdx_sort_indices: output too small");
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_sort_indices: more than 2^31-1 rows per call is not supported yet");
  for (int k = 0; k < nkeys; ++k) PDX_TRY(check_column(keys + k, "pdx_sort_indices", true));
  if (n && !out->values) return fail(PDX_INVALID, "pdx_sort_indices: output too small");
  out->length = n;
  out->null_count = 0;
  if (n == 0) return PDX_OK;
  hipStream_t st = as_stream(stream);
  Scratch s;
  const int64_t ntiles = ceil_div(n, kSortTile), nchunks = ceil_div(ntiles, kColChunk);
  unsigned long long* pays[3];
  for (auto& p : pays) p = s.get<unsigned long long>((size_t)n);
  uint32_t* lo0 = s.get<uint32_t>((size_t)n);
  uint32_t* lo1 = s.get<uint32_t>((size_t)n);
  uint32_t* hist = s.get<uint32_t>((size_t)ntiles << 8);
  uint32_t* chunk = s.get<uint32_t>((size_t)(nchunks + 1) << 8);
  SortKeyStats* stats = s.get<SortKeyStats>((size_t)nkeys);
  PDX_SCRATCH_CHECK(s);

  SortKeyDescs all{};
  all.n = nkeys;
  for (int k = 0; k < nkeys; ++k) {
    SortKeyDesc& d = all.k[k];
    d.v = static_cast<const char*>(keys[k].values) + keys[k].offset * dtype_bytes(keys[k].dtype);
    d.valid = validity_or_null(keys + k);
    d.off = keys[k].offset;
    d.dtype = keys[k].dtype;
    d.descending = descending && descending[k];
    d.cshift = -1;
  }
  SortKeyStats h[PDX_SORT_MAX_KEYS];
  for (int k = 0; k < nkeys; ++k) h[k] = SortKeyStats{~0ull, 0ull, 0ull, 0ull};
  PDX_HIP(hipMemcpyAsync(stats, h, sizeof(SortKeyStats) * (size_t)nkeys, hipMemcpyHostToDevice, st));
  {
    PDX_PROFILE("sort_key_stats", st);
    hipLaunchKernelGGL(k_sort_key_stats, dim3(grid_for(n, 256, 4), nkeys), dim3(256), 0, st, all, n, stats);
  }
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipMemcpyAsync(h, stats, sizeof(SortKeyStats) * (size_t)nkeys, hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));

  // the plan: fields from the least significant (the last key's value field) to the most significant (the first key's class field), packed
  // greedily into rounds of at most 64 bits; a field is never split and a field of width 0 takes no part
  struct Field {
    int key, width;
    bool is_class;
  };
  Field fields[2 * PDX_SORT_MAX_KEYS];
  int nfields = 0, key_bits = 0;
  for (int k = nkeys - 1; k >= 0; --k) {
    if ((int64_t)(h[k].nans + h[k].nulls) > n || (h[k].min > h[k].max && (int64_t)(h[k].nans + h[k].nulls) != n))
      return fail(PDX_DEVICE, "pdx_sort_indices: key statistics do not add up");
    const unsigned long long range = h[k].min <= h[k].max ? h[k].max - h[k].min : 0ull;
    const int w = range ? 64 - __builtin_clzll(range) : 0;
    all.k[k].base = all.k[k].descending ? h[k].max : h[k].min;
    if (w) fields[nfields++] = Field{k, w, false};
    if (h[k].nans + h[k].nulls) fields[nfields++] = Field{k, 2, true};
    key_bits += w + ((h[k].nans + h[k].nulls) ? 2 : 0);
  }
  const unsigned long long* sorted = nullptr;
  int rounds = 0, passes = 0;
  for (int f = 0; f < nfields || rounds == 0;) {  // (no field at all: one compose of key 0 numbers the rows)
    SortKeyDescs rd{};
    int bits = 0;
    int slot_of_key[PDX_SORT_MAX_KEYS];
    for (int& x : slot_of_key) x = -1;
    for (; f < nfields && bits + fields[f].width <= 64; ++f) {
      int& slot = slot_of_key[fields[f].key];
      if (slot < 0) {
        slot = rd.n++;
        rd.k[slot] = all.k[fields[f].key];
      }
      if (fields[f].is_class) {
        rd.k[slot].cshift = bits;
      } else {
        rd.k[slot].vshift = bits;
        rd.k[slot].vwidth = fields[f].width;
      }
      bits += fields[f].width;
    }
    unsigned long long* in = pays[0] == sorted ? pays[1] : pays[0];
    unsigned long long* tmp = pays[2] == in || pays[2] == sorted ? (pays[1] == in || pays[1] == sorted ? pays[0] : pays[1]) : pays[2];
    {
      PDX_PROFILE("sort_compose", st);
      hipLaunchKernelGGL(k_sort_compose, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, rd, sorted, n, lo0, in);
    }
    PDX_LAUNCH_CHECK();
    sorted = in;
    if (bits == 0) break;
    ++rounds;
    if (n > 1) PDX_TRY(sort_packed64_in(lo0, in, lo1, tmp, hist, chunk, n, bits == 64 ? ~0ull : (1ull << bits) - 1ull, st, &sorted, &passes));
  }
  hipLaunchKernelGGL(k_pay_rows_u64, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, sorted, n, static_cast<unsigned long long*>(out->values));
  PDX_LAUNCH_CHECK();
  if (out->validity) PDX_HIP(hipMemsetAsync(out->validity, 0xFF, (size_t)((n + 7) / 8), st));
  PDX_HIP(hipStreamSynchronize(st));
  if (info) *info = pdx_sort_info{rounds, key_bits, passes, 0};
  return PDX_OK;
}

int pdx_reindex_indices(const pdx_column* old_index, const pdx_column* new_index, pdx_mut_column* out_idx, void* stream) {
  PDX_TRY(check_index(old_index, "pdx_reindex_indices"));
  PDX_TRY(check_index(new_index, "pdx_reindex_indices"));
  if (!out_idx) return fail(PDX_INVALID, "pdx_reindex_indices: null output");
  if (old_index->dtype != new_index->dtype) return fail(PDX_INVALID, "type(NewIndex) != type(CurrentIndex).");
  const int64_t n_old = old_index->length, n_new = new_index->length, n = n_old + n_new;
  if (out_idx->dtype != PDX_INT64) return fail(PDX_INVALID, "pdx_reindex_indices: output must be int64 take indices");
  if (out_idx->length < n_new || (n_new && (!out_idx->values || !out_idx->validity)))
    return fail(PDX_INVALID, "pdx_reindex_indices: output needs new_index.length indices and a validity buffer");
  out_idx->length = n_new;
  out_idx->null_count = -1;
  if (n_new == 0) return PDX_OK;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_reindex_indices: more than 2^31-1 labels per call is not supported yet");
  hipStream_t st = as_stream(stream);
  Scratch s;
  long long* cat = s.get<long long>((size_t)n);
  uint32_t* gids = s.get<uint32_t>((size_t)n);
  uint8_t* ok = s.get<uint8_t>((size_t)n_new);
  PDX_SCRATCH_CHECK(s);
  hipLaunchKernelGGL(k_concat2_i64, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, static_cast<const long long*>(old_index->values) + old_index->offset,
                     n_old, 1, static_cast<const long long*>(new_index->values) + new_index->offset, n_new, cat);
  PDX_LAUNCH_CHECK();
  pdx_column cc{};
  cc.dtype = old_index->dtype;
  cc.length = n;
  cc.values = cat;
  GroupByOwner gb;
  PDX_TRY(pdx_groupby_create(&cc, stream, &gb.h));
  const int64_t G = pdx_groupby_num_groups(gb.h);
  int64_t* first_rows = s.get<int64_t>((size_t)G);
  PDX_SCRATCH_CHECK(s);
  PDX_TRY(pdx_groupby_group_ids(gb.h, gids, stream));
  PDX_TRY(pdx_groupby_first_rows(gb.h, first_rows, stream));
  hipLaunchKernelGGL(k_reindex_emit, dim3(grid_for(n_new, 256, 4)), dim3(256), 0, st, gids, first_rows, n_old, n_new,
                     static_cast<long long*>(out_idx->values), ok);
  hipLaunchKernelGGL(k_pack_bytes, dim3(grid_for((n_new + 7) / 8, 256)), dim3(256), 0, st, ok, n_new, static_cast<uint8_t*>(out_idx->validity));
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(st));
  return PDX_OK;
}

int pdx_index_intersection(const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_index(a, "pdx_index_intersection"));
  PDX_TRY(check_index(b, "pdx_index_intersection"));
  if (!out) return fail(PDX_INVALID, "pdx_index_intersection: null output");
  if (a->dtype != b->dtype) return fail(PDX_INVALID, "type(NewIndex) != type(CurrentIndex).");
  const int64_t na = a->length, nb = b->length, n = na + nb;
  if (out->dtype != a->dtype) return fail(PDX_INVALID, "pdx_index_intersection: output dtype must be the index dtype");
  if (out->length < na || (na && !out->values)) return fail(PDX_INVALID, "pdx_index_intersection: output must hold a.length labels");
  out->length = 0;
  out->null_count = 0;
  if (na == 0 || nb == 0) return PDX_OK;
  if (n > 0x7FFFFFFFll) return fail(PDX_NOT_IMPLEMENTED, "pdx_index_intersection: more than 2^31-1 labels per call is not supported yet");
  hipStream_t st = as_stream(stream);
  Scratch s;
  long long* cat = s.get<long long>((size_t)n);
  uint32_t* gids = s.get<uint32_t>((size_t)n);
  PDX_SCRATCH_CHECK(s);
  const long long* av = static_cast<const long long*>(a->values) + a->offset;
  hipLaunchKernelGGL(k_concat2_i64, dim3(grid_for(n, 256, 4)), dim3(256), 0, st, av, na, 1, static_cast<const long long*>(b->values) + b->offset, nb, cat);
  PDX_LAUNCH_CHECK();
  pdx_column cc{};
  cc.dtype = a->dtype;
  cc.length = n;
  cc.values = cat;
  GroupByOwner gb;
  PDX_TRY(pdx_groupby_create(&cc, stream, &gb.h));
  const int64_t G = pdx_groupby_num_groups(gb.h);
  int64_t* first_rows = s.get<int64_t>((size_t)G);
  uint8_t* in_b = s.get<uint8_t>((size_t)G);
  PDX_SCRATCH_CHECK(s);
  PDX_TRY(pdx_groupby_group_ids(gb.h, gids, stream));
  PDX_TRY(pdx_groupby_first_rows(gb.h, first_rows, stream));
  PDX_HIP(hipMemsetAsync(in_b, 0, (size_t)G, st));
  hipLaunchKernelGGL(k_mark_groups, dim3(grid_for(nb, 256, 4)), dim3(256), 0, st, gids, na, n, in_b);
  PDX_LAUNCH_CHECK();
  int64_t m = 0;
  PDX_TRY(compact_indices(G, IntersectPred{first_rows, in_b, G, na}, IntersectEmit{first_rows, av, G, na, static_cast<long long*>(out->values)}, &m, s, st));
  if (out->validity) PDX_HIP(hipMemsetAsync(out->validity, 0xFF, (size_t)((m + 7) / 8), st));
  PDX_HIP(hipStreamSynchronize(st));
  out->length = m;
  return PDX_OK;
}

}  // extern "C"
