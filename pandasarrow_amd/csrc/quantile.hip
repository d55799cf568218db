// quantile.hip -- exact quantiles for gfx950: pdx_quantile (whole column, radix select) and pdx_groupby_quantile.
//
// Replaces CallFunction("quantile", {array}, QuantileOptions{q, interpolation, skip_nulls, min_count}) reached from NDFrame::quantile
// (reference src/ndframe.h:259-263, src/ndframe.cpp:202-212), DataFrame::describe (src/dataframe.cpp:983-1030) and, per group,
// GroupBy::quantile (src/group_by.h:123-124, src/dataframe.cpp:1867-1931).
//
// (The select itself -- the level kernels and the host loop q_select -- lives in radix_select.hpp, shared with select_k.hip.)
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
#include <algorithm>
#include <vector>
#include "colview.hpp"
#include "group_order.hpp"
#include "quantile.hpp"
#include "radix_select.hpp"
#include "radix_sort.hpp"

namespace pdx {

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
