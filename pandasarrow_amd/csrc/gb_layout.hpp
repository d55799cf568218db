// gb_layout.hpp -- part of groupby.hip: the grouped layout of ONE value column (GroupedLayout, gb_handle.hpp) and how it is built.
//
// Reference: GroupBy's constructor materialises every column's per-group arrays once (processEach, src/dataframe.cpp:1539-1554:
// Grouper::MakeGroupings + ApplyGroupings) and sum() / mean() / count() reuse them (src/group_by.h:85-139).  Here the same
// split: build_layout sorts the values by slot (stage 1), the reducers in gb_agg.hpp consume the layout (stage 2); a bound column
// (pdx_groupby_bind) keeps its layout in the handle, so the reference's call pattern gb.sum(c); gb.mean(c); gb.count(c) sorts once.
#pragma once

// Diagnostic switches of pdx_groupby_agg, read once per call (tests flip them inside one process).  Defaults are the product path;
// pdx_groupby_last_plan reports the path a call actually took, so a test can assert it instead of trusting the thresholds.
struct AggTuning {
  bool fused = true;        // PDX_FUSED_LAST_DIGIT=0: never fuse the last digit into the reduce
  bool fused_hash = true;   // PDX_FUSED_LAST_DIGIT_HASH=0: not on hash-partitioned slots
  bool narrow = true;       // PDX_SORT_NARROW=0: 4-byte slots through every pass
  bool null_pw = false;     // PDX_FLR_NULL_PW=1: thread-per-leaf form for nullable sum / mean / count
  int64_t min_rows = (int64_t)1 << 22;  // PDX_FUSED_LAST_DIGIT_MIN_ROWS
  // PDX_FUSED_LAST_DIGIT_MIN_RUN: a run is one workgroup's sequential work (1e8 groups: 119-row runs).  Was 8192 until round 4: the
  // 1e6-key query at an 8-GPU shard's size (1.25e8 rows: 7629-row runs) fell just below it and took the classic full sort, 4.18 ms
  // against 2.69 ms fused; fused also wins at 5e7 / 2e7 / 3e7 rows (tools/sweep_min_run.sh: 2.25 -> 1.61, 1.60 -> 1.28, 1.46 -> 1.07 ms)
  int64_t min_run = 1024;
  int min_low = 10;         // PDX_FUSED_LAST_DIGIT_MIN_LOW_BITS
  int flr_wgs_per_cu = 24;  // PDX_FLR_WGS_PER_CU
  int fw_wgs_per_cu = 48;   // PDX_FLR_WAVE_WGS_PER_CU
  int wave_force = -1;      // PDX_FLR_WAVE=0 / 1: force the workgroup / wave form of the fused kernel
  bool hybrid = true;       // PDX_FLR_HYBRID=0: any run over the limit sends the whole column down the classic path
  unsigned int max_run = 1u << 19;  // PDX_FLR_MAX_RUN (<= 2^19): rows of the longest run the fused kernels take
  static AggTuning read() {
    AggTuning t;
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    auto on = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
    t.fused = !off("PDX_FUSED_LAST_DIGIT");
    t.fused_hash = !off("PDX_FUSED_LAST_DIGIT_HASH");
    t.narrow = !off("PDX_SORT_NARROW");
    t.null_pw = on("PDX_FLR_NULL_PW");
    if (const char* e = getenv("PDX_FUSED_LAST_DIGIT_MIN_ROWS")) t.min_rows = atoll(e);
    if (const char* e = getenv("PDX_FUSED_LAST_DIGIT_MIN_RUN")) t.min_run = atoll(e);
    if (const char* e = getenv("PDX_FUSED_LAST_DIGIT_MIN_LOW_BITS")) t.min_low = atoi(e);
    if (const char* e = getenv("PDX_FLR_WGS_PER_CU")) if (atoi(e) > 0) t.flr_wgs_per_cu = atoi(e);
    if (const char* e = getenv("PDX_FLR_WAVE_WGS_PER_CU")) if (atoi(e) > 0) t.fw_wgs_per_cu = atoi(e);
    if (const char* e = getenv("PDX_FLR_WAVE")) t.wave_force = e[0] != '0' ? 1 : 0;
    t.hybrid = !off("PDX_FLR_HYBRID");
    if (const char* e = getenv("PDX_FLR_MAX_RUN")) if (atoll(e) >= 64 && atoll(e) <= (1ll << 19)) t.max_run = (unsigned int)atoll(e);
    return t;
  }
};

constexpr unsigned int kFlrMaxRun = 1u << 19;  // a run is walked by ONE workgroup / wave (and sizes their counter levels): longer runs
                                               // (skewed keys) go through the side form below, or the whole column takes the classic path

// Which sort feeds the fused last digit on this handle (all false: full sort + classic reducers)
struct FusedPlan {
  bool flr = false, narrow = false, narrow_part = false;
  int low_bits = 0, eff_bits = 0, part = 0, mid_bits = 0;
  SortPlan low_plan{};
};
static FusedPlan plan_fused(const pdx_groupby* gb, bool nullable, const AggTuning& t) {
  FusedPlan p;
  const int64_t n = gb->n;
  p.part = gb->slot_part ? gb->part_bits : 0;
  // partitioned hash slots: the table itself is a power of two; only the two special slots (null key, INT64_MIN key) need one
  // more bit, so without them the top digit is drawn from the table's own bits (all 64 values used)
  p.eff_bits = (gb->slot_part && !gb->special_slots) ? gb->slot_bits - 1 : gb->slot_bits;
  p.low_bits = p.eff_bits - kFlrBits;
  p.mid_bits = p.low_bits - p.part;
  if (p.low_bits < 0) return p;
  // (hash-partitioned slots: only without the special slots -- with them the top digit is half empty and the runs half as long,
  //  measured slower than the classic path)
  p.flr = t.fused && n >= t.min_rows && p.low_bits - p.part >= 4 && p.low_bits >= t.min_low && p.low_bits <= 26 &&
          (!gb->slot_part || (t.fused_hash && !gb->special_slots)) && (n >> p.low_bits) >= t.min_run;
  if (p.flr && !gb->slot_part && gb->pass0_off)  // the stored pass-0 offsets belong to the first digit of the FULL plan
    p.flr = make_sort_plan(gb->slot_bits, sort_max_bits()).bits[0] == make_sort_plan(p.low_bits, sort_max_bits()).bits[0];
  if (!p.flr) return p;
  // Narrowing sort (dense slots, two passes below the fused digit): a digit that has been sorted on is dropped from the key, so
  // pass 0 writes 2-byte keys, pass 1 reads them and writes the top digit alone in a byte, which is all the fused kernel reads:
  // 12 B/row less traffic than carrying the 4-byte slot through.  Run starts then come from the scatter offsets (k_level_starts)
  // instead of a search in the sorted slots.  (values with nulls: the null flag rides in the narrow key's top bit, read from the
  // validity bitmap by pass 0 itself)
  p.low_plan = make_sort_plan(p.low_bits, sort_max_bits());
  p.narrow = t.narrow && !gb->slot_part && gb->pass0_off && p.low_plan.npasses == 2 && gb->slot_bits - p.low_plan.bits[0] <= (nullable ? 15 : 16) &&
             p.low_plan.bits[0] <= 8 && p.low_plan.bits[1] <= 8 && p.eff_bits == gb->slot_bits;
  // The same for the hash-partitioned layout (LDS build, one level, values without nulls): the value partition by bucket plays
  // pass 0, the build left every row's 13-bit index inside its bucket's region as a 2-byte key (idx16_part), so the one sort pass
  // below the fused digit reads 2-byte keys and writes the top digit alone: 8 B/row less than carrying the 4-byte logical slot.
  p.narrow_part = t.narrow && gb->slot_part && gb->idx16_part && !gb->digit2 && !nullable && p.part == kPartBits && p.mid_bits >= 4 && p.mid_bits <= 8 &&
                  p.eff_bits - p.part <= 16;
  return p;
}

static const char* slots_name(const pdx_groupby* gb) {
  if (gb->mode != 0) return gb->resample ? "bins" : "runs";
  if (gb->dense) return "dense";
  if (gb->slot_part) return gb->digit2 ? "hash_part2" : (gb->idx16_part ? "hash_lds" : "hash_part");
  return "hash_global";
}

// frees every block the layout took since `mark` except the ones named (a sort's ping-pong partners, partition copies)
static void keep_only(GroupedLayout& L, size_t mark, std::initializer_list<const void*> keep) {
  std::vector<void*> drop;
  for (size_t i = mark; i < L.owned.size(); ++i) {
    bool k = false;
    for (const void* q : keep) k = k || q == L.owned[i];
    if (!k) drop.push_back(L.owned[i]);
  }
  for (void* q : drop) L.disown(q);
}

// What every piece of build_layout works on: the handle, the value column of the call and the layout under construction.  ONE Scratch
// per build_layout call, released when the driver returns: k16, nhist, nchunk and dmax are read by kernels that a later piece enqueues.
struct LayoutCtx {
  pdx_groupby* gb;
  const pdx_column* values;
  const uint8_t* vvalid;  // the column's validity bitmap or nullptr
  const uint64_t* vin;    // row 0 of its values
  const AggTuning& t;
  GroupedLayout& L;
  Scratch& s;
  hipStream_t st;
};

// The runs of a column sorted by its low slot bits, as k_run_max_len counts them
struct RunStats {
  unsigned int hmax = 0, n_long = 0, rows_long = 0;  // longest run, runs over the limit, their rows
  // a few long runs (one key with a large share of the rows is enough to make one) are reduced from a side form, the rest by the
  // fused kernels; many or very long ones: the whole column takes the classic path
  bool side_ok(const AggTuning& t, int64_t n) const { return t.hybrid && n_long > 0 && n_long <= (unsigned int)kMaxLongRuns && (int64_t)rows_long <= n / 4; }
};

// What sort_narrow_to_runs / sort_lsd_to_runs return: the rows stably sorted by the low `low_bits` slot bits.  Every block named here
// is owned by the layout except dmax, nhist and nchunk (scratch of the build_layout call).
struct SortedRuns {
  int low_bits = 0;
  int64_t nruns = 0;
  unsigned int max_run = 0;                      // rows of the longest run the fused kernels take
  uint32_t* run_start = nullptr;                 // nruns + 1
  unsigned int* dmax = nullptr;                  // the three words of RunStats on the device
  const uint8_t* keys8 = nullptr;                // narrowing sort: the top digit of every row (else nullptr)
  const uint32_t* fkeys = nullptr;               // 4-byte LSD: the slot of every row (else nullptr)
  const uint64_t* vals = nullptr;
  uint64_t* spare = nullptr;                     // narrowing sort: the values as pass 0 left them, free as the target of one more pass
  uint32_t *nhist = nullptr, *nchunk = nullptr;  // narrowing sort: the offsets scratch of its passes
  RunStats stats;
  std::string sort_desc;
};

// (A') of GroupedLayout as build_side returns it (all zero: no run is over the limit)
struct SideForm {
  int64_t rows = 0;
  int runs = 0;
  const uint64_t* vals = nullptr;
  const uint32_t *keys = nullptr, *seg = nullptr;
};

// seal_fused / seal_full: the only places that set L.fused / L.full, the field groups (A), (A'), (B) of GroupedLayout and its plan strings
static int seal_fused(const LayoutCtx& c, const SortedRuns& r, const SideForm& side) {
  GroupedLayout& L = c.L;
  L.fused = true;
  L.keys8 = r.keys8;
  L.fkeys = r.fkeys;
  L.fvals = r.vals;
  if (r.spare) L.disown(r.spare);
  L.low_bits = r.low_bits;
  L.nruns = r.nruns;
  L.hmax = std::min(r.stats.hmax, r.max_run);  // (rows of the longest run the fused kernels walk)
  L.max_run = r.max_run;
  L.run_start = r.run_start;
  L.side_rows = side.rows;
  L.side_runs = side.runs;
  L.side_vals = side.vals;
  L.side_keys = side.keys;
  L.side_seg = side.seg;
  L.plan_fused = std::string("slots=") + slots_name(c.gb) + " sort=" + r.sort_desc + " layout=fused" + (side.rows ? " side=" + std::to_string(side.runs) : std::string());
  return PDX_OK;
}
static int seal_full(const LayoutCtx& c, const void* vals_sorted, const uint32_t* flag_keys, const uint32_t* seg_start, const uint32_t* out_index,
                     const uint8_t* row_valid, const std::string& sort_desc, bool skew) {
  GroupedLayout& L = c.L;
  L.full = true;
  L.vals_sorted = vals_sorted;
  L.flag_keys = flag_keys;
  L.seg_start = seg_start;
  L.out_index = out_index;
  L.row_valid = row_valid;
  L.plan_full = std::string("slots=") + slots_name(c.gb) + " sort=" + sort_desc + " layout=full" + (skew ? " skew=1" : "");
  return PDX_OK;
}

// segments: the rows are grouped as they stand
static int layout_segments(const LayoutCtx& c) { return seal_full(c, c.vin, nullptr, c.gb->seg_start, nullptr, c.vvalid, "none", false); }

// The side form of a fused layout: the rows of the (few) runs longer than r.max_run, gathered with their full slots, sorted by the top
// digit (one pass: within a digit they are in run order already, so the result is in slot order) and cut into segments for all G
// groups.  `keys` = the runs' top-digit bytes or 4-byte slots.
template <typename KT>
static int build_side(const LayoutCtx& c, const SortedRuns& r, const KT* keys, SideForm* out) {
  pdx_groupby* gb = c.gb;
  GroupedLayout& L = c.L;
  Scratch& s = c.s;
  hipStream_t st = c.st;
  PDX_PROFILE("side_layout", st);
  const int64_t G = gb->G, m = (int64_t)r.stats.rows_long;
  const int n_long = (int)r.stats.n_long;
  uint32_t* unordered = s.get<uint32_t>(kMaxLongRuns);
  uint32_t* list = s.get<uint32_t>(kMaxLongRuns);
  uint32_t* off = s.get<uint32_t>(kMaxLongRuns + 1);
  unsigned int* cnt = s.get<unsigned int>(1);
  uint32_t* k_in = s.get<uint32_t>((size_t)m);
  uint64_t* v_in = s.get<uint64_t>((size_t)m);
  PDX_SCRATCH_CHECK(s);
  uint32_t* k_out = L.own<uint32_t>((size_t)m);
  uint64_t* v_out = L.own<uint64_t>((size_t)m);
  uint32_t* seg = L.own<uint32_t>((size_t)G + 1);
  if (!k_out || !v_out || !seg) return PDX_OOM;
  PDX_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned int), st));
  hipLaunchKernelGGL(k_long_runs_append, dim3(grid_for(r.nruns, 256)), dim3(256), 0, st, r.run_start, r.nruns, r.max_run, (unsigned int)kMaxLongRuns, unordered, cnt);
  hipLaunchKernelGGL(k_long_runs_order, dim3(1), dim3(256), 0, st, unordered, n_long, r.run_start, list, off);
  hipLaunchKernelGGL((k_side_gather<KT>), dim3(grid_for(m, 256, 4)), dim3(256), 0, st, keys, r.vals, r.run_start, list, off, n_long, r.low_bits, m, k_in, v_in);
  PDX_LAUNCH_CHECK();
  const uint32_t* ks = nullptr;
  const uint64_t* vs = nullptr;
  PDX_TRY((radix_sort_pairs<uint64_t>(k_in, v_in, k_out, v_out, k_out, v_out, m, kFlrBits, &ks, &vs, true, s, st, r.low_bits)));
  hipLaunchKernelGGL(k_seg_starts, dim3(grid_for(G + 1, 256)), dim3(256), 0, st, ks, m, gb->occ_slot, G, seg);
  PDX_LAUNCH_CHECK();
  *out = SideForm{m, n_long, vs, nullptr, seg};
  if (c.vvalid) out->keys = ks;
  else L.disown(k_out);
  return PDX_OK;
}

// both sorts to runs begin here: the run starts (kept by a fused layout) and the device words of RunStats
static int begin_runs(const LayoutCtx& c, const FusedPlan& fp, SortedRuns* r) {
  r->low_bits = fp.low_bits;
  r->nruns = (int64_t)1 << fp.low_bits;
  r->max_run = std::min(c.t.max_run, kFlrMaxRun);
  r->run_start = c.L.own<uint32_t>((size_t)r->nruns + 1);
  r->dmax = c.s.get<unsigned int>(3);
  if (!r->run_start) return PDX_OOM;
  PDX_SCRATCH_CHECK(c.s);
  return PDX_OK;
}

// The narrowing sort (fp.narrow: dense slots, two passes; fp.narrow_part: the hash partition plays pass 0) up to the run statistics.
// Returns with pass 1's scatter enqueued and the statistics read back; every block of both passes is still owned.
static int sort_narrow_to_runs(const LayoutCtx& c, const FusedPlan& fp, SortedRuns* r) {
  pdx_groupby* gb = c.gb;
  GroupedLayout& L = c.L;
  Scratch& s = c.s;
  hipStream_t st = c.st;
  const int64_t n = gb->n;
  PDX_TRY(begin_runs(c, fp, r));
  const int b0 = fp.narrow ? fp.low_plan.bits[0] : kPartBits, b1 = fp.narrow ? fp.low_plan.bits[1] : fp.mid_bits;
  r->sort_desc = std::string(fp.narrow ? "narrow:" : "narrow_part:") + std::to_string(b0) + "+" + std::to_string(b1);
  const int64_t ntiles = ceil_div(n, kSortTile), nchunks = ceil_div(ntiles, kColChunk);
  uint16_t* k16 = fp.narrow ? s.get<uint16_t>((size_t)n) : gb->idx16_part;
  const uint32_t* prev_off = fp.narrow ? gb->pass0_off : gb->part_off;  // (row 0 = where every first digit's rows begin in the input of pass 1)
  uint8_t* k8 = L.own<uint8_t>((size_t)n);
  uint64_t* nv0 = L.own<uint64_t>((size_t)n);
  uint64_t* nv1 = L.own<uint64_t>((size_t)n);
  uint32_t* nhist = s.get<uint32_t>((size_t)ntiles << 8);
  uint32_t* nchunk = s.get<uint32_t>((size_t)(nchunks + 1) << 8);
  if (!k8 || !nv0 || !nv1) return PDX_OOM;
  PDX_SCRATCH_CHECK(s);
  int rcn = PDX_OK;
  if (fp.narrow_part) rcn = radix_scatter_only<kPartBits, uint64_t, uint8_t>(gb->bucket8, c.vin, nullptr, nv0, n, 0, false, gb->part_off, st);
  else
    rcn = with_digit_bits<4, 8>(b0, [&](auto b) {
      return c.vvalid ? radix_scatter_narrow<b(), uint64_t, uint32_t, uint16_t, true>(gb->slot_of_row, c.vin, k16, nv0, n, gb->pass0_off, st, c.vvalid, c.values->offset)
                      : radix_scatter_narrow<b(), uint64_t, uint32_t, uint16_t>(gb->slot_of_row, c.vin, k16, nv0, n, gb->pass0_off, st);
    });
  PDX_TRY(rcn);
  // pass 1 in two halves: its offsets first -- the run starts and the longest run (the host needs that number to choose the
  // reducer) follow from them alone -- then the scatter, which runs while the host reads the number back
  rcn = with_digit_bits<4, 8>(b1, [&](auto b) { return radix_offsets<b(), uint16_t>(k16, n, 0, nhist, nchunk, true, st); });
  PDX_TRY(rcn);
  struct EventGuard {  // the event must not outlive an early return
    hipEvent_t ev = nullptr;
    ~EventGuard() { if (ev) (void)hipEventDestroy(ev); }
  } hmax_ready;
  {
    PDX_PROFILE("run_starts", st);
    // (row 0 of the pass-0 offsets = where every first digit's rows begin in the input of pass 1)
    hipLaunchKernelGGL((k_level_starts<uint16_t>), dim3(1u << b0), dim3(256), 0, st, k16, n, prev_off, (int64_t)1 << b0, b0, b1, nhist, r->run_start);
    PDX_HIP(hipMemsetAsync(r->dmax, 0, 3 * sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_run_max_len, dim3(grid_for(r->nruns, 256)), dim3(256), 0, st, r->run_start, r->nruns, r->dmax, r->max_run);
    PDX_LAUNCH_CHECK();
    PDX_HIP(hipMemcpyAsync(hmax_pinned(), r->dmax, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    PDX_HIP(hipEventCreateWithFlags(&hmax_ready.ev, hipEventDisableTiming));
    PDX_HIP(hipEventRecord(hmax_ready.ev, st));
  }
  rcn = with_digit_bits<4, 8>(b1, [&](auto b) {
    return c.vvalid ? radix_scatter_narrow<b(), uint64_t, uint16_t, uint8_t, true>(k16, nv0, k8, nv1, n, nhist, st)
                    : radix_scatter_narrow<b(), uint64_t, uint16_t, uint8_t>(k16, nv0, k8, nv1, n, nhist, st);
  });
  PDX_TRY(rcn);
  const hipError_t ew = hipEventSynchronize(hmax_ready.ev);
  if (ew != hipSuccess) return hip_fail(ew, "pdx_groupby_agg");
  r->stats = RunStats{hmax_pinned()[0], hmax_pinned()[1], hmax_pinned()[2]};
  r->keys8 = k8;
  r->vals = nv1;
  r->spare = nv0;
  r->nhist = nhist;
  r->nchunk = nchunk;
  return PDX_OK;
}

// The narrowing sort on skewed keys: the fused kernel is skipped.  Finish the sort with the one pass that is left (on the byte digits)
// and take the group offsets from its scatter offsets: one more level of k_level_starts gives the start of every slot's rows
static int finish_narrow_skewed(const LayoutCtx& c, const SortedRuns& r) {
  pdx_groupby* gb = c.gb;
  GroupedLayout& L = c.L;
  hipStream_t st = c.st;
  const int64_t n = gb->n, G = gb->G;
  uint32_t* ss_narrow = L.own<uint32_t>((size_t)G + 1);
  uint32_t* slot_start = c.s.get<uint32_t>(((size_t)r.nruns << kFlrBits) + 1);
  if (!ss_narrow) return PDX_OOM;
  PDX_SCRATCH_CHECK(c.s);
  PDX_TRY((radix_offsets<kFlrBits, uint8_t>(r.keys8, n, 0, r.nhist, r.nchunk, true, st)));
  const uint32_t* fkeys = nullptr;
  if (c.vvalid) {  // the classic nullable reducers read the null flag from bit 31 of a 4-byte key per grouped row: write flags only
    uint32_t* fk = L.own<uint32_t>((size_t)n);
    if (!fk) return PDX_OOM;
    PDX_TRY((radix_scatter_narrow<kFlrBits, uint64_t, uint8_t, uint32_t, true>(r.keys8, r.vals, fk, r.spare, n, r.nhist, st)));
    fkeys = fk;
  } else {
    PDX_TRY((radix_scatter_narrow<kFlrBits, uint64_t, uint8_t, uint8_t>(r.keys8, r.vals, (uint8_t*)nullptr, r.spare, n, r.nhist, st)));
  }
  {
    PDX_PROFILE("seg_starts", st);
    hipLaunchKernelGGL((k_level_starts<uint8_t>), dim3((unsigned)std::min<int64_t>(r.nruns, 65536)), dim3(256), 0, st, r.keys8, n, r.run_start, r.nruns,
                       r.low_bits, kFlrBits, r.nhist, slot_start);
    hipLaunchKernelGGL(k_seg_starts_from_slots, dim3(grid_for(G + 1, 256)), dim3(256), 0, st, slot_start, n, gb->occ_slot, G, ss_narrow);
  }
  PDX_LAUNCH_CHECK();
  L.disown(r.keys8);  // what is kept of the sort: the values of the last pass, the group offsets, the flag keys
  L.disown(r.vals);
  L.disown(r.run_start);
  return seal_full(c, r.spare, fkeys, ss_narrow, gb->gid_of_occ, nullptr, r.sort_desc, true);
}

// 4-byte slots sorted by the low bits only (LSD passes that skip the top digit), run starts by a search in the sorted slots
static int sort_lsd_to_runs(const LayoutCtx& c, const FusedPlan& fp, SortedRuns* r) {
  pdx_groupby* gb = c.gb;
  GroupedLayout& L = c.L;
  hipStream_t st = c.st;
  PDX_TRY(begin_runs(c, fp, r));
  r->sort_desc = "lsd:skip" + std::to_string(gb->slot_bits - r->low_bits);
  const size_t mark = L.owned.size();
  PDX_TRY(sort_values_by_slot(gb, c.vin, c.vvalid, c.values->offset, [&](size_t bytes) { return (void*)L.own<uint8_t>(bytes); }, c.s, st, &r->fkeys, &r->vals,
                              gb->slot_bits - r->low_bits));
  keep_only(L, mark, {r->fkeys, r->vals});
  {
    PDX_PROFILE("run_starts", st);
    PDX_HIP(hipMemsetAsync(r->dmax, 0, 3 * sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_run_starts, dim3(grid_for(r->nruns + 1, 256)), dim3(256), 0, st, r->fkeys, gb->n, r->low_bits, r->nruns, r->run_start, r->dmax);
    hipLaunchKernelGGL(k_run_max_len, dim3(grid_for(r->nruns, 256)), dim3(256), 0, st, r->run_start, r->nruns, r->dmax, r->max_run);
    PDX_LAUNCH_CHECK();
    unsigned int h3[3] = {0, 0, 0};
    PDX_HIP(hipMemcpyAsync(h3, r->dmax, sizeof(h3), hipMemcpyDeviceToHost, st));
    PDX_HIP(hipStreamSynchronize(st));
    r->stats = RunStats{h3[0], h3[1], h3[2]};
  }
  return PDX_OK;
}

// The tail of every sort by the whole slot: group offsets by a search in the sorted slots, which then stay only as null flags
static int finish_sorted_slots(const LayoutCtx& c, const uint32_t* keys_sorted, const uint64_t* vs, const std::string& sort_desc, bool skew) {
  pdx_groupby* gb = c.gb;
  const int64_t G = gb->G;
  uint32_t* ss = c.L.own<uint32_t>((size_t)G + 1);
  if (!ss) return PDX_OOM;
  {
    PDX_PROFILE("seg_starts", c.st);
    hipLaunchKernelGGL(k_seg_starts, dim3(grid_for(G + 1, 256)), dim3(256), 0, c.st, keys_sorted, gb->n, gb->occ_slot, G, ss);
  }
  PDX_LAUNCH_CHECK();
  if (!c.vvalid && keys_sorted != gb->slot_of_row) c.L.disown(keys_sorted);  // the sorted slots were only needed for the group offsets
  return seal_full(c, vs, c.vvalid ? keys_sorted : nullptr, ss, gb->gid_of_occ, nullptr, sort_desc, skew);
}

// 4-byte LSD on skewed keys: the fused kernel is skipped (a run longer than 2^19 rows): finish the sort with the one pass that is left
static int finish_partial_lsd(const LayoutCtx& c, const SortedRuns& r) {
  GroupedLayout& L = c.L;
  const int64_t n = c.gb->n;
  L.disown(r.run_start);
  uint32_t* k2 = L.own<uint32_t>((size_t)n);
  uint64_t* v2 = L.own<uint64_t>((size_t)n);
  if (!k2 || !v2) return PDX_OOM;
  const uint32_t* ks2 = nullptr;
  const uint64_t* vs2 = nullptr;
  PDX_TRY((radix_sort_pairs<uint64_t>(r.fkeys, r.vals, k2, v2, k2, v2, n, kFlrBits, &ks2, &vs2, true, c.s, c.st, r.low_bits)));
  L.disown(r.fkeys);
  L.disown(r.vals);
  return finish_sorted_slots(c, ks2, vs2, r.sort_desc + "+finish", true);
}

// one group: the rows are grouped as they stand (no sort); null flags, if any, still go into a key per row
static int layout_single_group(const LayoutCtx& c) {
  pdx_groupby* gb = c.gb;
  const uint32_t* keys = gb->slot_of_row;
  if (c.vvalid) {
    uint32_t* fk1 = c.L.own<uint32_t>((size_t)gb->n);
    if (!fk1) return PDX_OOM;
    hipLaunchKernelGGL(k_flag_keys, dim3(grid_for(gb->n, 256, 4)), dim3(256), 0, c.st, gb->slot_of_row, c.vvalid, c.values->offset, gb->n, fk1);
    keys = fk1;
  }
  return finish_sorted_slots(c, keys, c.vin, "none", false);
}

// full form: stable sort of (slot, value) by slot, each group's values contiguous in row order
static int layout_full_sort(const LayoutCtx& c) {
  GroupedLayout& L = c.L;
  const uint32_t* keys_sorted = nullptr;
  const uint64_t* vs = nullptr;
  const size_t mark = L.owned.size();  // (a bound layout's older fused form lies below the mark)
  PDX_TRY(sort_values_by_slot(c.gb, c.vin, c.vvalid, c.values->offset, [&](size_t bytes) { return (void*)L.own<uint8_t>(bytes); }, c.s, c.st, &keys_sorted, &vs));
  keep_only(L, mark, {keys_sorted, vs});
  return finish_sorted_slots(c, keys_sorted, vs, "lsd", false);
}

// Stage 1 of pdx_groupby_agg for one column.  allow_fused: the request can be served by the fused last-digit kernels (the five
// standard kinds, variance, stddev); the layout then stops LOW of the top 6 slot bits when the handle qualifies (L.fused), unless a
// run turns out longer than kFlrMaxRun (skewed keys), in which case the sort is finished here (L.full).  Otherwise a full sort.
static int build_layout(pdx_groupby* gb, const pdx_column* values, bool allow_fused, const AggTuning& t, GroupedLayout& L, hipStream_t st) {
  L.values = values->values;
  L.validity = validity_or_null(values);
  L.offset = values->offset;
  L.dtype = values->dtype;
  L.stream = st;
  Scratch s;
  const LayoutCtx c{gb, values, validity_or_null(values), static_cast<const uint64_t*>(values->values) + values->offset, t, L, s, st};
  if (gb->mode != 0) return layout_segments(c);
  const FusedPlan fp = allow_fused && !L.fused ? plan_fused(gb, c.vvalid != nullptr, t) : FusedPlan{};
  if (!fp.flr) return gb->G == 1 && gb->slot_of_row ? layout_single_group(c) : layout_full_sort(c);
  SortedRuns r;
  const bool narrow = fp.narrow || fp.narrow_part;
  PDX_TRY(narrow ? sort_narrow_to_runs(c, fp, &r) : sort_lsd_to_runs(c, fp, &r));
  if (r.stats.hmax <= r.max_run) return seal_fused(c, r, SideForm{});
  if (!r.stats.side_ok(t, gb->n)) return narrow ? finish_narrow_skewed(c, r) : finish_partial_lsd(c, r);
  SideForm side;
  PDX_TRY(narrow ? build_side(c, r, r.keys8, &side) : build_side(c, r, r.fkeys, &side));
  return seal_fused(c, r, side);
}
