// gb_agg.hpp -- part of groupby.hip (namespace pdx): stage 2 of pdx_groupby_agg, the reducers over a GroupedLayout, one function per path.
//
//   parse_agg_request        the kinds and output columns of a call -> AggRequest (checks, length / null_count of every output)
//   choose_reducer           LDS accumulators (gb_acc.hpp, no layout) or a layout (build_layout, gb_layout.hpp), fused or full
//   reduce_std               the five standard kinds from one reduce: reduce_acc / reduce_fused / reduce_full
//   agg_std_bound / _unbound ... through a bound column's per-group cache (cache_alloc, then copies) / straight into the outputs
//   agg_variance, agg_product_first_last, compose_plan (what pdx_groupby_last_plan reports)
// Every stage works on one AggCtx: ONE Scratch per pdx_groupby_agg call, released when the driver returns.
#pragma once

struct AggRequest {
  const int* kinds = nullptr;
  int nk = 0;
  pdx_mut_column* outs = nullptr;
  SegOut o{};
  bool want_pw = false, want_mm = false, want_is = false, want_std5 = false;
  // the "next" kinds (variance, stddev, product, first, last) run after the five standard ones on the same grouped values
  double *var_out = nullptr, *std_out = nullptr;
  void *prod_out = nullptr, *first_out = nullptr, *last_out = nullptr;
  bool is_f = true;
  bool std_only() const { return (want_std5 || var_out || std_out) && !prod_out && !first_out && !last_out; }  // (variance: two more fused passes)
};

// What every stage works on: the handle, the value column of the call, its layout (the bound one or the call's own) and the reducer chosen
struct AggCtx {
  pdx_groupby* gb;
  const pdx_column* values;
  const uint8_t* vvalid;  // the column's validity bitmap or nullptr
  GroupedLayout& L;
  const AggTuning& t;
  const AccTuning& at;
  Scratch& s;
  hipStream_t st;
  bool bound;  // the layout is kept in the handle (pdx_groupby_bind)
  AccGeom ag{};
  bool use_acc = false, use_fused = false;
  std::string reducer, acc_plan, cache_note;  // the words of the plan the stages leave behind
};

static int parse_agg_request(const pdx_groupby* gb, const pdx_column* values, const int* kinds, int nk, pdx_mut_column* outs, AggRequest* rq) {
  const int64_t G = gb->G;
  const bool is_f = values->dtype == PDX_FLOAT64;
  rq->kinds = kinds;
  rq->nk = nk;
  rq->outs = outs;
  rq->is_f = is_f;
  SegOut& o = rq->o;
  for (int k = 0; k < nk; ++k) {
    pdx_mut_column* oc = &outs[k];
    if (oc->length < G) return fail(PDX_INVALID, "pdx_groupby_agg: output too small");
    if (G && !oc->values) return fail(PDX_INVALID, "pdx_groupby_agg: null output buffer");
    int want_dt;
    bool needs_validity = validity_or_null(values) != nullptr;
    switch (kinds[k]) {
      case PDX_AGG_SUM:
        want_dt = is_f ? PDX_FLOAT64 : PDX_INT64;
        if (is_f) { o.sum_f = static_cast<double*>(oc->values); rq->want_pw = true; }
        else { o.sum_i = static_cast<long long*>(oc->values); rq->want_is = true; }
        rq->want_std5 = true;
        break;
      case PDX_AGG_MEAN: want_dt = PDX_FLOAT64; o.mean = static_cast<double*>(oc->values); rq->want_pw = true; rq->want_std5 = true; break;
      case PDX_AGG_MIN: want_dt = values->dtype; o.vmin = oc->values; rq->want_mm = true; rq->want_std5 = true; break;
      case PDX_AGG_MAX: want_dt = values->dtype; o.vmax = oc->values; rq->want_mm = true; rq->want_std5 = true; break;
      case PDX_AGG_COUNT: want_dt = PDX_INT64; o.count = static_cast<long long*>(oc->values); needs_validity = false; rq->want_std5 = true; break;
      case PDX_AGG_VARIANCE: want_dt = PDX_FLOAT64; rq->var_out = static_cast<double*>(oc->values); break;
      case PDX_AGG_STDDEV: want_dt = PDX_FLOAT64; rq->std_out = static_cast<double*>(oc->values); break;
      case PDX_AGG_PRODUCT: want_dt = values->dtype; rq->prod_out = oc->values; break;
      case PDX_AGG_FIRST: want_dt = values->dtype; rq->first_out = oc->values; break;
      case PDX_AGG_LAST: want_dt = values->dtype; rq->last_out = oc->values; break;
      default: return fail(PDX_INVALID, "pdx_groupby_agg: unknown aggregate kind");
    }
    if (oc->dtype != want_dt) return fail(PDX_INVALID, "pdx_groupby_agg: output dtype does not match the aggregate's result type");
    if (needs_validity && !oc->validity)
      return fail(PDX_INVALID, "pdx_groupby_agg: values carry nulls but an output has no validity buffer");
    oc->length = G;
    oc->null_count = needs_validity ? -1 : 0;
  }
  return PDX_OK;
}

// one segmented reduce of `vals` (float64 or int64 per f64) over `G` segments of `nrows` grouped rows into `oo`; nullable: the null flag of
// every grouped row is bit 31 of flag_keys (or read in place from row_valid, segments mode); ok_bytes: 1 = the group has a valid value
static int reduce_segments(bool nullable, const uint32_t* flag_keys, const uint8_t* row_valid, int64_t valid_off, const uint32_t* seg_start, int64_t G,
                           int64_t nrows, const void* vals, bool f64, const SegOut& oo, bool pw, bool mm, bool is, const uint32_t* oidx, uint8_t* ok_bytes,
                           Scratch& s, hipStream_t st) {
  PDX_PROFILE("seg_reduce", st);
  const int64_t n = nrows;
  if (!nullable) {
    if (f64) return launch_seg_reduce_dense<double>(static_cast<const double*>(vals), seg_start, G, oidx, oo, pw, mm, is, n, s, st);
    return launch_seg_reduce_dense<long long>(static_cast<const long long*>(vals), seg_start, G, oidx, oo, pw, mm, is, n, s, st);
  }
  const int grid = (int)std::min<int64_t>(ceil_div(G, kSegWaves), (int64_t)kCUs * 8);
  if (f64)
    hipLaunchKernelGGL((k_seg_reduce_nullable<double>), dim3(grid), dim3(kSegWaves * 64), 0, st, static_cast<const double*>(vals), flag_keys, row_valid,
                       valid_off, seg_start, G, oidx, oo, ok_bytes);
  else
    hipLaunchKernelGGL((k_seg_reduce_nullable<long long>), dim3(grid), dim3(kSegWaves * 64), 0, st, static_cast<const long long*>(vals), flag_keys,
                       row_valid, valid_off, seg_start, G, oidx, oo, ok_bytes);
  PDX_LAUNCH_CHECK();
  return reduce_huge_nullable_groups(vals, f64 ? PDX_FLOAT64 : PDX_INT64, flag_keys, row_valid, valid_off, seg_start, G, oidx, n, oo, ok_bytes, s, st);
}
// ... over a full layout; vals == the layout's own values or an array in the same order
static int reduce_full(const pdx_groupby* gb, const GroupedLayout& L, const void* vals, bool f64, const SegOut& oo, bool pw, bool mm, bool is,
                       const uint32_t* oidx, uint8_t* ok_bytes, Scratch& s, hipStream_t st) {
  return reduce_segments(L.validity != nullptr, L.flag_keys, L.row_valid, L.offset, L.seg_start, gb->G, gb->n, vals, f64, oo, pw, mm, is, oidx, ok_bytes, s, st);
}
// ... over the side form of a fused layout (the rows of its long runs): EVERY group's outputs are written -- zeros / nulls for the groups
// outside the long runs -- so it runs before the fused kernel, which then writes the groups of the runs it walks
static int reduce_side(const pdx_groupby* gb, const GroupedLayout& L, const SegOut& oo, bool pw, bool mm, bool is, uint8_t* ok_bytes, const double* sqmean,
                       Scratch& s, hipStream_t st) {
  const bool is_f = L.dtype == PDX_FLOAT64, nullable = L.validity != nullptr;
  const void* vals = L.side_vals;
  bool f64 = is_f;
  if (sqmean) {  // second pass of variance: (x - mean of x's group)^2, summed over the same valid runs
    double* d = s.get<double>((size_t)L.side_rows);
    PDX_SCRATCH_CHECK(s);
    PDX_PROFILE("seg_sqdev", st);
    const int grid = (int)std::min<int64_t>(ceil_div(gb->G, 4), (int64_t)kCUs * 16);
    if (is_f) hipLaunchKernelGGL((k_seg_sqdev<double>), dim3(grid), dim3(256), 0, st, reinterpret_cast<const double*>(L.side_vals), L.side_seg, gb->G, sqmean, d, gb->gid_of_occ);
    else hipLaunchKernelGGL((k_seg_sqdev<long long>), dim3(grid), dim3(256), 0, st, reinterpret_cast<const long long*>(L.side_vals), L.side_seg, gb->G, sqmean, d, gb->gid_of_occ);
    PDX_LAUNCH_CHECK();
    vals = d;
    f64 = true;
  }
  return reduce_segments(nullable, L.side_keys, nullptr, 0, L.side_seg, gb->G, L.side_rows, vals, f64, oo, pw, mm, is, gb->gid_of_occ, ok_bytes, s, st);
}

// A run-time flag as a template argument of a kernel: f(std::true_type{}) or f(std::false_type{})
template <typename F>
static void with_flag(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
// The rows of a fused layout as typed pointers: f(keys, vals), keys = its top-digit bytes (narrowing sort) or its 4-byte slots, vals =
// its doubles or int64s
template <typename F>
static void with_fused_rows(const GroupedLayout& L, F&& f) {
  auto with_keys = [&](auto* vals) {
    if (L.keys8) f(L.keys8, vals);
    else f(L.fkeys, vals);
  };
  if (L.dtype == PDX_FLOAT64) with_keys(reinterpret_cast<const double*>(L.fvals));
  else with_keys(reinterpret_cast<const long long*>(L.fvals));
}
template <typename P>
using pointee_t = std::remove_const_t<std::remove_pointer_t<P>>;

// The fused last digit: rank by the top 6 slot bits + Arrow's leaf / counter recurrence in one pass over a fused layout.
// ok_bytes (nullable values): 1 = the group has a valid value; sqmean: second pass of variance.
static int reduce_fused(const pdx_groupby* gb, const GroupedLayout& L, const AggTuning& t, const SegOut& oo, bool pw, bool mm, bool is, uint8_t* okbytes,
                        const double* sqmean, Scratch& s, hipStream_t st, std::string* reducer) {
  if (L.side_rows) PDX_TRY(reduce_side(gb, L, oo, pw, mm, is, okbytes, sqmean, s, st));
  const unsigned int max_run = L.max_run ? L.max_run : 0xFFFFFFFFu;
  PDX_PROFILE("fused_last_digit_reduce", st);
  const bool nullable = L.validity != nullptr;
  const int64_t nruns = L.nruns, n = gb->n;
  const int low_bits = L.low_bits;
  const uint32_t* run_start = L.run_start;
  const bool dense = pw && !mm && !is && !nullable;
  // (values with nulls, sum / mean / count: the thread-per-leaf form is opt-in, PDX_FLR_NULL_PW=1 -- measured 11.3 ms against
  //  10.7 ms of the literal per-lane replay at 5 % nulls: its per-group walk over the leaf markers is as serial as the replay)
  const bool nullpw = pw && !mm && !is && nullable && t.null_pw;
  // one WAVE per run (flr_wave.hpp) for everything but the dense sum / mean / count: nullable values, min / max and int64 sums
  // were a per-lane replay by wave 0 alone in the workgroup-per-run kernel (5 % nulls: 10.7 -> 4.9 ms per 1e9 rows); the dense
  // fast path of k_flr_reduce (thread per leaf) is still ahead of the wave form (3.0 vs 3.3 ms).  PDX_FLR_WAVE=1 / 0 force either.
  const bool wave_form = !nullpw && (t.wave_force >= 0 ? t.wave_force != 0 : !dense);
  if (reducer) *reducer = wave_form ? "flr_wave" : (nullpw ? "flr_reduce_nullpw" : (dense ? "flr_reduce_dense" : "flr_reduce"));
  if (wave_form) {
    const int wgrid = (int)std::min<int64_t>(nruns, (int64_t)kCUs * t.fw_wgs_per_cu);
    const bool pw_only = pw && !mm && !is;
    // counter levels: a group cannot outgrow its run, and a leaf holds 16 rows unless nulls cut it short
    const uint64_t max_leaves = nullable ? (uint64_t)L.hmax + 1 : (uint64_t)L.hmax / 16 + 2;
    const int fw_levels = std::max(2, ilog2(max_leaves + 1));  // 2^levels > leaves: level index <= levels - 1
    const size_t fw_lds = (size_t)fw_lds_bytes(nullable, fw_levels);
    with_fused_rows(L, [&](auto* keys, auto* vals) {
      with_flag(nullable, [&](auto nn) {
        with_flag(pw_only, [&](auto pp) {
          hipLaunchKernelGGL((k_flr_wave<pointee_t<decltype(vals)>, pointee_t<decltype(keys)>, decltype(nn)::value, decltype(pp)::value>), dim3(wgrid), dim3(64),
                             fw_lds, st, keys, vals, n, run_start, nruns, low_bits, gb->gid_of_slot, oo, okbytes, (int)pw, (int)mm, (int)is, sqmean, fw_levels,
                             max_run);
        });
      });
    });
  } else {
    const int grid = (int)std::min<int64_t>(nruns, (int64_t)kCUs * t.flr_wgs_per_cu);
    with_fused_rows(L, [&](auto* keys, auto* vals) {
      auto launch = [&](auto dense_pw, auto null_pw) {
        hipLaunchKernelGGL((k_flr_reduce<pointee_t<decltype(vals)>, decltype(dense_pw)::value, pointee_t<decltype(keys)>, decltype(null_pw)::value>), dim3(grid),
                           dim3(kSortBlock), 0, st, keys, vals, run_start, nruns, low_bits, gb->gid_of_slot, oo, okbytes, (int)pw, (int)mm, (int)is,
                           nullable ? 1 : 0, sqmean, max_run);
      };
      // (no kernel is both: the dense form is for values without nulls, the thread-per-leaf form for values with nulls)
      if (nullpw) launch(std::false_type{}, std::true_type{});
      else with_flag(dense, [&](auto dense_pw) { launch(dense_pw, std::false_type{}); });
    });
  }
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

__global__ void k_mean_from_cache(const double* __restrict__ sum, const long long* __restrict__ cnt, int64_t G, double* __restrict__ out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < G; i += stride) out[i] = cnt[i] ? pw_mean(sum[i], (double)cnt[i]) : 0.0;
}

// Which reducer serves the request, and stage 1 (the grouped layout) where that reducer needs one the column does not have yet
static int choose_reducer(AggCtx& c, const AggRequest& rq) {
  GroupedLayout& L = c.L;
  const SegOut& o = rq.o;
  const bool std_only = rq.std_only();
  // count / min / max / int64 sum do not depend on the order of a group's rows: when nothing else is asked for and no sorted layout of
  // the column exists yet, they skip the value sort (gb_acc.hpp: one partition pass + accumulators in LDS)
  const bool order_free = rq.want_std5 && !rq.want_pw && !rq.var_out && !rq.std_out && !rq.prod_out && !rq.first_out && !rq.last_out;
  // (a BOUND column's int64 sum keeps the sorted layout: gb.sum(c) is usually followed by gb.mean(c), which needs it -- Arrow's int64 mean
  //  is the pairwise sum of the doubles -- and the layout then serves both; min / max / count of a bound column do skip the sort)
  if (order_free && !(c.bound && rq.want_is) && !L.fused && !L.full)
    c.ag = acc_geometry(c.gb, c.vvalid != nullptr, (o.vmin ? kAccMin : 0u) | (o.vmax ? kAccMax : 0u) | (o.sum_i ? kAccSum : 0u) | (o.count ? kAccCnt : 0u),
                        rq.is_f, c.at);
  c.use_acc = c.ag.ok;
  if (!c.use_acc && ((!L.fused && !L.full) || (!std_only && !L.full))) PDX_TRY(build_layout(c.gb, c.values, std_only, c.t, L, c.st));
  c.use_fused = std_only && L.fused;
  return PDX_OK;
}

// the five standard kinds from one reduce into `oo`
static int reduce_std(AggCtx& c, const AggRequest& rq, const SegOut& oo, bool pw, bool mm, bool is, uint8_t* okb) {
  if (c.use_acc) {
    c.reducer = "lds_acc";
    return reduce_acc(c.gb, c.ag, c.values, oo, okb, c.at, c.s, c.st, &c.acc_plan);
  }
  if (c.use_fused) return reduce_fused(c.gb, c.L, c.t, oo, pw, mm, is, okb, nullptr, c.s, c.st, &c.reducer);
  c.reducer = c.vvalid ? "seg_reduce_nullable" : "seg_reduce";
  return reduce_full(c.gb, c.L, c.L.vals_sorted, rq.is_f, oo, pw, mm, is, c.L.out_index, okb, c.s, c.st);
}

// The validity bitmaps of the outputs whose kind is in `served`, in request order: packed from the kind's ok-bytes (1 = the group has a
// valid value), all ones where it has none.  The caller checks the launches.
struct KindOk {
  int kind;
  const uint8_t* ok_bytes;
};
static void pack_validity(const AggCtx& c, const AggRequest& rq, std::initializer_list<KindOk> served) {
  const int64_t G = c.gb->G;
  for (int k = 0; k < rq.nk; ++k)
    for (const KindOk& ko : served) {
      uint8_t* bits = static_cast<uint8_t*>(rq.outs[k].validity);
      if (ko.kind != rq.kinds[k] || !bits) continue;
      if (!ko.ok_bytes) hipMemsetAsync(bits, 0xFF, (size_t)((G + 7) / 8), c.st);
      else hipLaunchKernelGGL(k_pack_bytes, dim3(grid_for((G + 7) / 8, 256)), dim3(256), 0, c.st, ko.ok_bytes, G, bits);
    }
}
static void pack_validity_std(const AggCtx& c, const AggRequest& rq, const uint8_t* okb) {  // (a count is never null)
  pack_validity(c, rq, {{PDX_AGG_SUM, okb}, {PDX_AGG_MEAN, okb}, {PDX_AGG_MIN, okb}, {PDX_AGG_MAX, okb}, {PDX_AGG_COUNT, nullptr}});
}

// the per-group cache of a bound column: allocates what a fill needs and the layout does not have yet (PDX_OOM if any allocation failed)
// and points the fill's outputs `f` at it
static int cache_alloc(AggCtx& c, bool cnt, bool sum, bool isum, bool mm, SegOut* f) {
  GroupedLayout& L = c.L;
  const size_t G = (size_t)c.gb->G;
  if (cnt && !L.c_count) L.c_count = L.own<long long>(G);
  if (c.vvalid && !L.c_ok) L.c_ok = L.own<uint8_t>(G);
  if (sum && !L.c_sum) L.c_sum = L.own<double>(G);
  if (isum && !L.c_isum) L.c_isum = L.own<long long>(G);
  if (mm && !L.c_min) {
    L.c_min = L.own<uint64_t>(G);
    L.c_max = L.own<uint64_t>(G);
  }
  if ((cnt && !L.c_count) || (c.vvalid && !L.c_ok) || (sum && !L.c_sum) || (isum && !L.c_isum) || (mm && (!L.c_min || !L.c_max))) return PDX_OOM;
  if (cnt) f->count = L.c_count;
  if (sum) f->sum_f = L.c_sum;
  if (isum) f->sum_i = L.c_isum;
  if (mm) f->vmin = L.c_min;
  if (mm) f->vmax = L.c_max;
  return PDX_OK;
}

// The five standard kinds of a bound column, which keeps its per-group sum / count (/ min / max): sum(); mean(); count() as three calls
// cost one reduce
static int agg_std_bound(AggCtx& c, const AggRequest& rq) {
  GroupedLayout& L = c.L;
  const SegOut& o = rq.o;
  const int64_t G = c.gb->G;
  const bool is_f = rq.is_f;
  const bool have_cnt = L.have_pw || L.have_count, have_isum = L.have_pw || L.have_is;
  const bool need_sumfam = (rq.want_pw && !L.have_pw) || (rq.want_is && !have_isum) || (o.count && !have_cnt), need_mm = rq.want_mm && !L.have_mm;
  SegOut f{};
  if (c.use_acc && (need_sumfam || need_mm)) {
    // order-free kinds of a bound column: only what is asked for is computed and kept
    const bool need_is = rq.want_is && !have_isum, need_cnt = o.count && !have_cnt;
    PDX_TRY(cache_alloc(c, need_cnt, false, need_is, need_mm, &f));
    PDX_TRY(reduce_std(c, rq, f, false, need_mm, need_is, L.c_ok));
    L.have_count = L.have_count || need_cnt;
    L.have_is = L.have_is || need_is;
    L.have_mm = L.have_mm || need_mm;
    c.cache_note = " cache=fill";
  } else if (need_sumfam || need_mm) {
    // from a sorted layout: the count is always kept, and the whole sum family (pairwise sum, count, int64 sum) comes from one reduce
    PDX_TRY(cache_alloc(c, true, need_sumfam, need_sumfam && !is_f, need_mm, &f));
    PDX_TRY(reduce_std(c, rq, f, need_sumfam, need_mm, need_sumfam && !is_f, L.c_ok));
    L.have_pw = L.have_pw || need_sumfam;
    L.have_mm = L.have_mm || need_mm;
    c.cache_note = " cache=fill";
  } else {
    c.cache_note = " cache=hit";
    c.reducer = "none";
  }
  const size_t gb8 = (size_t)G * 8;
  if (o.sum_f) PDX_HIP(hipMemcpyAsync(o.sum_f, L.c_sum, gb8, hipMemcpyDeviceToDevice, c.st));
  if (o.sum_i) PDX_HIP(hipMemcpyAsync(o.sum_i, L.c_isum, gb8, hipMemcpyDeviceToDevice, c.st));
  if (o.count) PDX_HIP(hipMemcpyAsync(o.count, L.c_count, gb8, hipMemcpyDeviceToDevice, c.st));
  if (o.vmin) PDX_HIP(hipMemcpyAsync(o.vmin, L.c_min, gb8, hipMemcpyDeviceToDevice, c.st));
  if (o.vmax) PDX_HIP(hipMemcpyAsync(o.vmax, L.c_max, gb8, hipMemcpyDeviceToDevice, c.st));
  if (o.mean) hipLaunchKernelGGL(k_mean_from_cache, dim3(grid_for(G, 256)), dim3(256), 0, c.st, L.c_sum, L.c_count, G, o.mean);
  pack_validity_std(c, rq, L.c_ok);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// ... of any other column: straight into the outputs
static int agg_std_unbound(AggCtx& c, const AggRequest& rq) {
  uint8_t* okb = c.vvalid ? c.s.get<uint8_t>((size_t)c.gb->G) : nullptr;
  PDX_SCRATCH_CHECK(c.s);
  PDX_TRY(reduce_std(c, rq, rq.o, rq.want_pw, rq.want_mm, rq.want_is, okb));
  pack_validity_std(c, rq, okb);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// Variance / stddev: Arrow's two passes: mean = pairwise sum / count, then the pairwise sum of (x - mean)^2 over the same valid runs
static int agg_variance(AggCtx& c, const AggRequest& rq) {
  pdx_groupby* gb = c.gb;
  GroupedLayout& L = c.L;
  Scratch& s = c.s;
  hipStream_t st = c.st;
  const int64_t G = gb->G;
  double* m2 = s.get<double>((size_t)G);
  long long* cnt_g = s.get<long long>((size_t)G);
  uint8_t* ok2 = c.vvalid ? s.get<uint8_t>((size_t)G) : nullptr;
  uint8_t* ok1 = c.vvalid ? s.get<uint8_t>((size_t)G) : nullptr;
  double* mean_g = s.get<double>((size_t)G);
  PDX_SCRATCH_CHECK(s);
  SegOut o1{}, o2{};
  o1.mean = mean_g;
  o2.sum_f = m2;
  o2.count = cnt_g;
  if (c.use_fused) {
    // on the same partially sorted rows: per-group mean (group-id order), then the squared deviations formed inside the kernel
    PDX_TRY(reduce_fused(gb, L, c.t, o1, true, false, false, ok1, nullptr, s, st, &c.reducer));
    PDX_TRY(reduce_fused(gb, L, c.t, o2, true, false, false, ok2, mean_g, s, st, nullptr));
  } else {
    if (c.reducer.empty()) c.reducer = c.vvalid ? "seg_reduce_nullable" : "seg_reduce";
    double* d = s.get<double>((size_t)gb->n);
    PDX_SCRATCH_CHECK(s);
    PDX_TRY(reduce_full(gb, L, L.vals_sorted, rq.is_f, o1, true, false, false, nullptr, ok1, s, st));  // segment order
    {
      PDX_PROFILE("seg_sqdev", st);
      const int grid = (int)std::min<int64_t>(ceil_div(G, 4), (int64_t)kCUs * 16);
      if (rq.is_f) hipLaunchKernelGGL((k_seg_sqdev<double>), dim3(grid), dim3(256), 0, st, static_cast<const double*>(L.vals_sorted), L.seg_start, G, mean_g, d);
      else hipLaunchKernelGGL((k_seg_sqdev<long long>), dim3(grid), dim3(256), 0, st, static_cast<const long long*>(L.vals_sorted), L.seg_start, G, mean_g, d);
      PDX_LAUNCH_CHECK();
    }
    PDX_TRY(reduce_full(gb, L, d, true, o2, true, false, false, L.out_index, ok2, s, st));
  }
  hipLaunchKernelGGL(k_var_finish, dim3(grid_for(G, 256)), dim3(256), 0, st, m2, cnt_g, G, rq.var_out, rq.std_out);
  pack_validity(c, rq, {{PDX_AGG_VARIANCE, ok2}, {PDX_AGG_STDDEV, ok2}});
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// product / first / last: one kernel over the full layout
static int agg_product_first_last(AggCtx& c, const AggRequest& rq) {
  const GroupedLayout& L = c.L;
  hipStream_t st = c.st;
  const int64_t G = c.gb->G;
  uint8_t* pok = (c.vvalid && rq.prod_out) ? c.s.get<uint8_t>((size_t)G) : nullptr;
  uint8_t* fok = (c.vvalid && rq.first_out) ? c.s.get<uint8_t>((size_t)G) : nullptr;
  uint8_t* lok = (c.vvalid && rq.last_out) ? c.s.get<uint8_t>((size_t)G) : nullptr;
  PDX_SCRATCH_CHECK(c.s);
  {
    PDX_PROFILE("seg_product_first_last", st);
    const int pf_grid = (int)std::min<int64_t>(ceil_div(G, 4), (int64_t)kCUs * 16);
    if (rq.is_f)
      hipLaunchKernelGGL((k_seg_product_first_last<double>), dim3(pf_grid), dim3(256), 0, st, static_cast<const double*>(L.vals_sorted), L.flag_keys,
                         L.row_valid, c.values->offset, L.seg_start, G, L.out_index, static_cast<double*>(rq.prod_out), pok, static_cast<double*>(rq.first_out),
                         fok, static_cast<double*>(rq.last_out), lok);
    else
      hipLaunchKernelGGL((k_seg_product_first_last<long long>), dim3(pf_grid), dim3(256), 0, st, static_cast<const long long*>(L.vals_sorted),
                         L.flag_keys, L.row_valid, c.values->offset, L.seg_start, G, L.out_index, static_cast<long long*>(rq.prod_out), pok,
                         static_cast<long long*>(rq.first_out), fok, static_cast<long long*>(rq.last_out), lok);
  }
  pack_validity(c, rq, {{PDX_AGG_PRODUCT, pok}, {PDX_AGG_FIRST, fok}, {PDX_AGG_LAST, lok}});
  PDX_LAUNCH_CHECK();
  if (c.reducer.empty() || c.reducer == "none") c.reducer = "seg_product_first_last";
  return PDX_OK;
}

// what pdx_groupby_last_plan reports: the layout's own words (or the accumulators'), then the reducer and the cache
static std::string compose_plan(const AggCtx& c) {
  const char* bound = c.bound ? " bound=1" : " bound=0";
  if (c.use_acc)
    return (c.acc_plan.empty() ? std::string("slots=") + slots_name(c.gb) + " sort=none layout=none reducer=none" : c.acc_plan) + bound + c.cache_note;
  return (c.use_fused ? c.L.plan_fused : c.L.plan_full) + " reducer=" + c.reducer + bound + c.cache_note;
}
