// gb_create.hpp -- part of groupby.hip (namespace pdx): the host side of pdx_groupby_create, one builder per key -> slot path.
//
//   sample_keys             one host round trip: can the keys be sorted (-> build_label_runs, groupby.hip), how wide is their window
//   try_dense_speculative   residue-form dense slots and the exact min/max in ONE pass; rolled back when the window was guessed too narrow
//   try_dense_exact         min/max pass, then slot = key - min
//   build_dense_domain      the slot / first-row kernels of both
//   build_hash_partitioned  general keys: partition by hash bucket, one table region per bucket (LDS or memory side), retry loop
//   build_hash_global       small inputs: one open-addressing table
//   finish_group_ids        every path: occupied slots compacted, group ids in first-occurrence order
// A builder describes its slots in a SlotDomain, which finish_group_ids consumes; the handle's own fields (slot_of_row, slot_part,
// part_off, ...) are filled by the builder that owns them.  Diagnostic switches: CreateTuning, read once per call.
#pragma once

// Diagnostic switches of pdx_groupby_create, read once per call (tests flip them inside one process).  Defaults are the product path.
struct CreateTuning {
  bool sorted = true;           // PDX_GROUPBY_SORTED=0: keys that arrive grouped are not taken as runs (pdx_downsample_create too)
  bool dense = true;            // PDX_GROUPBY_DENSE=0: never dense slots, always a hash table
  bool dense_lds = true;        // PDX_DENSE_LDS=0: the dense tail keeps its seen-bitmap in memory (and nothing is built speculatively)
  bool dense_speculate = true;  // PDX_DENSE_SPECULATE=0: the exact min/max pass first, no speculative dense build
  int speculate_bits = 20;      // PDX_DENSE_SPECULATE_BITS: widest key window the speculative build tries
  int64_t prefix_per_slot = 0;  // PDX_DENSE_PREFIX_PER_SLOT (> 0): rows per slot through the full first-row protocol; 0 = by size
  int partition = 1;            // PDX_HASH_PARTITION=0: global table at any size, =2: partitioned at any size, else partitioned from 2^18 rows
  bool hash_rows = false;       // PDX_HASH_ROWS=1: row ids ride through the partition even without null keys
  bool hash_lds = true;         // PDX_HASH_LDS=0: memory-side probe only (and no second partition level)
  int64_t head_rows = 0;        // PDX_HASH_HEAD_ROWS (>= 1, rounded up to 4 probe blocks): a bucket's rows the LDS build takes itself; 0 = by size
  bool hash_split = true;       // PDX_HASH_SPLIT=0: no second partition level
  bool hash_debug = false;      // PDX_HASH_DEBUG (set at all): one stderr line per build attempt
  static CreateTuning read() {
    CreateTuning t;
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    t.sorted = !off("PDX_GROUPBY_SORTED");
    t.dense = !off("PDX_GROUPBY_DENSE");
    t.dense_lds = !off("PDX_DENSE_LDS");
    t.dense_speculate = !off("PDX_DENSE_SPECULATE");
    if (const char* e = getenv("PDX_DENSE_SPECULATE_BITS")) t.speculate_bits = atoi(e);
    if (const char* e = getenv("PDX_DENSE_PREFIX_PER_SLOT")) if (atoi(e) > 0) t.prefix_per_slot = atoi(e);
    if (const char* e = getenv("PDX_HASH_PARTITION")) t.partition = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
    if (const char* e = getenv("PDX_HASH_ROWS")) t.hash_rows = e[0] == '1';
    t.hash_lds = !off("PDX_HASH_LDS");
    if (const char* e = getenv("PDX_HASH_HEAD_ROWS")) t.head_rows = std::max<int64_t>(atoll(e), 1);
    t.hash_split = !off("PDX_HASH_SPLIT");
    t.hash_debug = getenv("PDX_HASH_DEBUG") != nullptr;
    return t;
  }
};

// What every builder works on: the handle under construction and the key column of the call.
struct CreateCtx {
  pdx_groupby* gb;
  const long long* keys;  // row 0 of the key column
  const uint8_t* valid;   // its validity bitmap or nullptr
  int64_t key_off;        // bit of row 0 in `valid`
  int64_t n;
  Scratch& s;
  hipStream_t st;
  const CreateTuning& t;
  HashCtl* ctl;           // one device HashCtl: what a hash build attempt reports back
};

// What a builder returns and finish_group_ids consumes.
//   dense slots:        dense_first (first row of every slot), null_slot, nslots; slot = key - dense_min (dense_mask == 0) or
//                       key & dense_mask (the speculative build; dense_min is then the exact minimum).  table, region stay 0.
//   partitioned table:  table, region (slots per bucket: logical slot = (index in region << part_bits) | bucket), null_slot = capacity,
//                       nslots = capacity + 2 (the null key and the INT64_MIN key live past the table).  The dense fields stay 0.
//   global table:       the same with region == 0.
struct SlotDomain {
  Slot* table = nullptr;
  unsigned int* dense_first = nullptr;
  long long dense_min = 0;
  unsigned int dense_mask = 0, null_slot = 0, region = 0;
  int64_t nslots = 0;
};

// The hash table of one build attempt: returned to the pool on every exit until the handle takes it (owned.push_back + release()).
struct PoolFree {
  void operator()(void* p) const { pool_free(p); }
};
using TableBlock = std::unique_ptr<Slot, PoolFree>;
static Slot* alloc_table(unsigned int cap) { return static_cast<Slot*>(pool_alloc(((size_t)cap + 2) * sizeof(Slot))); }

constexpr KeyRange kNoKeys{0x7FFFFFFFFFFFFFFFll, (long long)0x8000000000000000ull, 0, 0};
static void widen_range(KeyRange& r, const KeyRange& w) {
  if (!w.any) return;
  r.vmin = std::min(r.vmin, w.vmin);
  r.vmax = std::max(r.vmax, w.vmax);
  r.any = 1;
}

struct KeySample {
  bool maybe_sorted = false;  // no sampled pair of neighbours rules the runs path out
  KeyRange range = kNoKeys;   // hull of the sampled valid keys (want_range only)
};
// ---- keys that arrive grouped (non-decreasing, no nulls: a sorted id column, a time index rounded to calendar bins): the groups
// are the runs of equal keys where they stand -- no dictionary, and no value sort in pdx_groupby_agg (segments mode, as resample).
// 65536 sampled neighbour pairs rule the path out for anything else at the price of one small kernel; the counting pass of the
// run-start compaction then proves the order over all rows (a sample that lied costs that one pass: the builders below take over).
// The key-range sample of the speculative dense build shares the host round trip.
static int sample_keys(const CreateCtx& c, bool want_sorted, bool want_range, KeySample* out) {
  if (!want_sorted && !want_range) return PDX_OK;
  KeyRange hsv[64];
  unsigned int hflags[4] = {0, 0, 0, 4u};
  unsigned int* flags = c.s.get<unsigned int>(4);
  KeyRange* dsample = c.s.get<KeyRange>(64);
  if (c.s.failed) return PDX_OOM;
  if (want_sorted) {
    PDX_HIP(hipMemsetAsync(flags, 0, 4 * sizeof(unsigned int), c.st));
    hipLaunchKernelGGL(k_sample_descents, dim3(64), dim3(1024), 0, c.st, c.keys, c.valid, c.key_off, c.n, flags + 3);
    PDX_HIP(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, c.st));
  }
  if (want_range) {
    hipLaunchKernelGGL(k_sample_key_range, dim3(64), dim3(1024), 0, c.st, c.keys, c.valid, c.key_off, c.n, dsample);
    PDX_HIP(hipMemcpyAsync(hsv, dsample, sizeof(hsv), hipMemcpyDeviceToHost, c.st));
  }
  PDX_LAUNCH_CHECK();
  PDX_HIP(hipStreamSynchronize(c.st));
  out->maybe_sorted = want_sorted && !(hflags[3] & 4u) && (hflags[3] & 3u) != 3u;
  if (want_range)
    for (const KeyRange& w : hsv) widen_range(out->range, w);
  return PDX_OK;
}

// rows that go through the full first-row protocol before the tail's bitmap is taken: a slot unseen by then costs one global atomic per
// later row of its key.  16 rows per slot leave e^-16 of uniformly spread keys unseen; below 2^29 rows 8 per slot (e^-8 = 3e-4 of the
// slots, a few 10^4 atomics) -- the prefix pass is the slow one (60 Grows/s: a random read of first[] per row) and at an 8-GPU shard's
// size 16 per slot was 13 % of the rows, 0.28 ms of a 0.84 ms create.
// From 2^29 rows on, domains whose bitmap fits the LDS tail (<= 2^20 slots) take 4 per slot: an unseen slot there costs a read of the
// cache-resident first[] per later row and an atomic only for the first of them.  Measured at 1e9 rows / 1e6 keys, the slot kernels
// per step over five alternated runs each: 16 -> 2.51-2.57 ms, 8 -> 2.46-2.52 ms, 4 -> 2.37-2.45 ms (at 1e5 keys the 2^22-row floor
// below decides and the three are the same 2.35 ms).  Larger domains (global bitmap, first[] not cache resident) keep 16.
static int64_t dense_prefix_rows(const CreateCtx& c, int64_t nslots) {
  int64_t per_slot = c.t.prefix_per_slot;
  if (per_slot <= 0) per_slot = c.n < ((int64_t)1 << 29) ? 8 : ((nslots + 31) >> 5) <= kDenseLdsWords ? 4 : 16;
  const int64_t prefix = std::min<int64_t>(c.n, std::max<int64_t>((int64_t)1 << 22, per_slot * nslots));
  return std::min<int64_t>(c.n, round_up(prefix, kSortTile));
}

// Builds slot_of_row, first[] and (when the first sort digit is 4..8 bits wide) the scanned pass-0 offsets for the dense domain
// described by (mn, mask, null_slot, nslots).  range_out != nullptr: also the exact key range, computed by the same pass.
static int build_dense_domain(const CreateCtx& c, long long mn, unsigned int mask, unsigned int null_slot, int64_t nslots, KeyRange* range_out,
                              unsigned int** first_out) {
  pdx_groupby* gb = c.gb;
  hipStream_t st = c.st;
  const int64_t n = c.n;
  unsigned int* dense_first = *first_out = c.s.get<unsigned int>((size_t)nslots);
  if (c.s.failed) return PDX_OOM;
  hipMemsetAsync(dense_first, 0xFF, (size_t)nslots * sizeof(unsigned int), st);
  // prefix with the full first-row protocol, then the bitmap-filtered tail; the tail kernel is tile shaped and also emits the
  // per-tile histogram of the first sort digit
  const int64_t ntiles = ceil_div(n, kSortTile), nchunks = ceil_div(ntiles, kColChunk);
  const int bits0 = make_sort_plan(ilog2((uint64_t)nslots), sort_max_bits()).bits[0];
  const int64_t prefix = dense_prefix_rows(c, nslots);
  const bool fuse = bits0 >= 4 && bits0 <= 8;
  const int64_t nwords = (nslots + 31) >> 5;
  const int64_t tile_first_tail = prefix / kSortTile;
  const bool lds_bitmap = fuse && c.t.dense_lds && prefix < n && nwords <= kDenseLdsWords && ntiles - tile_first_tail >= 256;
  if (range_out && !(fuse && prefix < n)) return fail(PDX_DEVICE, "dense_build: fused key range needs the histogram tail");
  uint32_t* chunk_sum = nullptr;
  if (fuse) {
    gb->pass0_off = gb->own<uint32_t>((size_t)ntiles << bits0);
    chunk_sum = c.s.get<uint32_t>((size_t)(nchunks + 1) << bits0);  // + digit totals row
    if (!gb->pass0_off || c.s.failed) return PDX_OOM;
  }
  KeyRange* wg_range = nullptr;
  long long *tile_min = nullptr, *tile_max = nullptr;
  if (range_out) {
    wg_range = c.s.get<KeyRange>((size_t)kCUs);
    if (c.s.failed) return PDX_OOM;
    if (!lds_bitmap) {  // the global-bitmap tail writes one (min, max) per tile
      tile_min = c.s.get<long long>((size_t)ntiles);
      tile_max = c.s.get<long long>((size_t)ntiles);
      if (c.s.failed) return PDX_OOM;
    }
  }
  {
    PDX_PROFILE("dense_slots", st);
    // (a tail that walks all tiles from 0 rewrites every slot: the prefix then leaves slot_of_row alone)
    if (prefix < n && fuse && (lds_bitmap || range_out))
      hipLaunchKernelGGL(k_dense_slots<false>, dim3(grid_for(prefix, 256, 8)), dim3(256), 0, st, c.keys, c.valid, c.key_off, prefix, mn, mask, null_slot,
                         dense_first, gb->slot_of_row);
    else
      hipLaunchKernelGGL(k_dense_slots<true>, dim3(grid_for(prefix, 256, 8)), dim3(256), 0, st, c.keys, c.valid, c.key_off, prefix, mn, mask, null_slot,
                         dense_first, gb->slot_of_row);
    if (prefix < n) {
      uint32_t* seen = c.s.get<uint32_t>((size_t)nwords);
      if (c.s.failed) return PDX_OOM;
      hipLaunchKernelGGL(k_seen_bitmap, dim3(grid_for(nwords, 256)), dim3(256), 0, st, dense_first, nslots, seen);
      const unsigned tail_tiles = (unsigned)(ntiles - tile_first_tail);
      if (!fuse)
        hipLaunchKernelGGL(k_dense_slots_tail, dim3(grid_for(n - prefix, 256, 8)), dim3(256), 0, st, c.keys, c.valid, c.key_off, prefix, n, mn, mask,
                           null_slot, seen, dense_first, gb->slot_of_row);
      else
        with_digit_bits<4, 8>(bits0, [&](auto b) {
          // the LDS tail walks ALL tiles (slots, histogram and key range of the prefix rows too; first-row tracking from `prefix` on)
          if (lds_bitmap)
            hipLaunchKernelGGL((k_dense_slots_tail_hist_lds<b()>), dim3(kCUs), dim3(kDenseLdsBlock), 0, st, c.keys, c.valid, c.key_off, (int64_t)0, ntiles, n,
                               mn, mask, null_slot, seen, (int)nwords, prefix, dense_first, gb->slot_of_row, gb->pass0_off, wg_range);
          else if (range_out)  // all tiles: slots, histogram and key range of the prefix rows too
            hipLaunchKernelGGL((k_dense_slots_tail_hist<b()>), dim3((unsigned)ntiles), dim3(kSortBlock), 0, st, c.keys, c.valid, c.key_off, (int64_t)0, n, mn,
                               mask, null_slot, seen, prefix, dense_first, gb->slot_of_row, gb->pass0_off, tile_min, tile_max);
          else
            hipLaunchKernelGGL((k_dense_slots_tail_hist<b()>), dim3(tail_tiles), dim3(kSortBlock), 0, st, c.keys, c.valid, c.key_off, tile_first_tail, n, mn,
                               mask, null_slot, seen, prefix, dense_first, gb->slot_of_row, gb->pass0_off, (long long*)nullptr, (long long*)nullptr);
        });
    }
  }
  PDX_LAUNCH_CHECK();
  if (fuse) {
    if (!lds_bitmap && !range_out)  // histogram of the prefix tiles (the prefix is a whole number of tiles unless it is the whole input)
      with_digit_bits<4, 8>(bits0, [&](auto b) {
        hipLaunchKernelGGL((k_radix_hist<b()>), dim3((unsigned)ceil_div(prefix, kSortTile)), dim3(kSortBlock), 0, st, gb->slot_of_row, prefix, 0, gb->pass0_off);
      });
    PDX_TRY(radix_scan_dispatch(bits0, gb->pass0_off, ntiles, chunk_sum, true, st));
  }
  if (range_out && !lds_bitmap) {
    long long lo = 0, hi = 0, dummy = 0;
    PDX_TRY(minmax_i64_host(tile_min, ntiles, &lo, &dummy, c.s, st));
    PDX_TRY(minmax_i64_host(tile_max, ntiles, &dummy, &hi, c.s, st));
    *range_out = KeyRange{lo, hi, lo <= hi ? 1 : 0, 0};
  } else if (range_out) {
    std::vector<KeyRange> h((size_t)kCUs);
    PDX_HIP(hipMemcpyAsync(h.data(), wg_range, sizeof(KeyRange) * kCUs, hipMemcpyDeviceToHost, st));
    PDX_HIP(hipStreamSynchronize(st));
    *range_out = kNoKeys;
    for (const KeyRange& w : h) widen_range(*range_out, w);
  }
  return PDX_OK;
}

// What the dense attempts learn about the key range on their way
struct KeyRangeFacts {
  MinMaxPartial<long long> mm;  // exact minimum / maximum of the valid keys (rmin < 0: every key is null), once have_mm
  bool have_mm = false;
  bool not_dense = false;       // settled without the exact range: dense slots are switched off, or the sample alone is too wide
};

// slots may span this many keys: min(2^26, 4 n)
static unsigned long long dense_limit(int64_t n) { return std::min<unsigned long long>(1ull << 26, (unsigned long long)n * 4 + 1024); }

// ---- speculative single pass: guess the width of the key window from a sample, build the residue-form dense domain and the
// exact min/max together (saves the separate 8 B/row min/max pass), accept when the exact span fits the guessed width
static int try_dense_speculative(const CreateCtx& c, const KeyRange& hs, SlotDomain* d, KeyRangeFacts* f) {
  pdx_groupby* gb = c.gb;
  const int64_t n = c.n;
  const unsigned long long dense_lim = dense_limit(n);
  int b = 64;
  if (hs.any) {
    const unsigned long long span_s = (unsigned long long)hs.vmax - (unsigned long long)hs.vmin;
    b = 4;
    while (b < 64 && (span_s >> b)) ++b;  // smallest width (>= 4 bits) with sample span < 2^b
    // the sample range lies inside the exact range: a sample already too wide for the dense domain settles the question
    // without the full min/max pass
    if (span_s >= dense_lim) f->not_dense = true;
  }
  // Only windows of <= 20 bits (LDS-resident bitmap).  Wider windows work too (global bitmap, tile min/max in the same pass) but
  // do not pay: the power-of-two residue domain makes the bitmap up to 2x larger than key - min and costs more than the
  // saved min/max pass (measured at 1e7 keys: 42.6 vs 39.7 ms).
  if (!(b <= c.t.speculate_bits && b <= 26 && (1ull << b) <= dense_lim && (int64_t)16 * (((int64_t)1 << b) + 1) + 2 * kSortTile < n)) return PDX_OK;
  const unsigned int mask = (1u << b) - 1, null_slot = 1u << b;
  const int64_t nslots = (int64_t)null_slot + (c.valid ? 1 : 0);
  const size_t mark = gb->owned.size();  // the attempt's blocks are the ones the handle takes from here on
  gb->slot_of_row = gb->own<uint32_t>((size_t)n);
  if (!gb->slot_of_row) return PDX_OOM;
  KeyRange exact;
  unsigned int* first = nullptr;
  PDX_TRY(build_dense_domain(c, 0, mask, null_slot, nslots, &exact, &first));
  f->mm.vmin = exact.vmin;
  f->mm.vmax = exact.vmax;
  f->mm.rmin = f->mm.rmax = exact.any ? 0 : -1;
  f->have_mm = true;
  if (exact.any && (unsigned long long)exact.vmax - (unsigned long long)exact.vmin <= mask) {
    gb->dense = 1;
    d->dense_first = first;
    d->dense_min = exact.vmin;
    d->dense_mask = mask;
    d->null_slot = null_slot;
    d->nslots = nslots;
    return PDX_OK;
  }
  // the window is wider than the sample suggested (or there is no valid key at all): the caller redoes it on the exact range
  while (gb->owned.size() > mark) {
    pool_free(gb->owned.back());
    gb->owned.pop_back();
  }
  gb->slot_of_row = nullptr;
  gb->pass0_off = nullptr;
  return PDX_OK;
}

// ---- dense-domain fast path: valid keys span a small integer range -> slot = key - min, no table.  Leaves gb->dense == 0 when the
// range is too wide.
static int try_dense_exact(const CreateCtx& c, SlotDomain* d, KeyRangeFacts* f) {
  pdx_groupby* gb = c.gb;
  if (!f->have_mm) {
    PDX_TRY(minmax_keys_host(c.keys, c.valid, c.key_off, c.n, &f->mm, c.s, c.st));
    f->have_mm = true;
  }
  if (f->mm.rmin >= 0) {
    const unsigned long long span = (unsigned long long)f->mm.vmax - (unsigned long long)f->mm.vmin;  // range - 1
    if (span >= dense_limit(c.n)) return PDX_OK;
    d->dense_min = f->mm.vmin;
    d->null_slot = (unsigned int)span + 1;
    d->nslots = (int64_t)d->null_slot + 1;
  } else {  // every key is null: one group
    d->null_slot = 0;
    d->nslots = 1;
  }
  gb->dense = 1;
  gb->slot_of_row = gb->own<uint32_t>((size_t)c.n);
  if (!gb->slot_of_row) return PDX_OOM;
  return build_dense_domain(c, d->dense_min, 0, d->null_slot, d->nslots, nullptr, &d->dense_first);
}

// State of the partitioned hash build between its attempts
struct HashPartition {
  int64_t ntiles = 0, nchunks = 0;
  long long* keys_part = nullptr;       // the keys in partition order
  unsigned int pb = kPartBits;          // hash bits the rows are currently partitioned by
  uint32_t* bucket_starts = nullptr;    // starts of the 2^pb buckets after a second partition level
  bool idx16_written = false;           // by the attempt that succeeded (the LDS build at the first partition level)
  bool lds_failed_at_pb = false;
};

// ---- general keys, partitioned build: hash -> stable partition by the low 8 hash bits (== first LSD pass of the sort by slot)
static int partition_by_bucket(const CreateCtx& c, HashPartition* hp) {
  pdx_groupby* gb = c.gb;
  hipStream_t st = c.st;
  const int64_t n = c.n;
  const int64_t ntiles = hp->ntiles = ceil_div(n, kSortTile), nchunks = hp->nchunks = ceil_div(ntiles, kColChunk);
  gb->bucket8 = gb->own<uint8_t>((size_t)n);
  gb->part_off = gb->own<uint32_t>((size_t)ntiles << kPartBits);
  gb->slot_part = gb->own<uint32_t>((size_t)n);
  // row ids ride through the partition only when there are null keys (their flag is bit 31 of the row id); otherwise on demand
  const bool rows_in_partition = c.valid != nullptr || c.t.hash_rows;
  if (rows_in_partition) gb->rows_part = gb->own<uint32_t>((size_t)n);
  gb->idx16_part = gb->own<uint16_t>((size_t)n);
  uint32_t* chunk_sum = c.s.get<uint32_t>((size_t)(nchunks + 1) << kPartBits);  // + digit totals row
  long long* keys_part = hp->keys_part = c.s.get<long long>((size_t)n);
  if (c.s.failed || !gb->bucket8 || !gb->part_off || !gb->slot_part || (rows_in_partition && !gb->rows_part) || !gb->idx16_part) return PDX_OOM;
  {
    // one pass over the keys: bucket byte per row (kept: it is the digit of the value partition of every later aggregation)
    // + the partition histogram
    PDX_PROFILE("hash_bucket_hist", st);
    hipLaunchKernelGGL(k_hash_bucket_hist, dim3((unsigned)ntiles), dim3(kSortBlock), 0, st, c.keys, c.valid, c.key_off, n, gb->bucket8, gb->part_off);
  }
  PDX_TRY(radix_scan_only<kPartBits>(gb->part_off, ntiles, chunk_sum, true, st));
  if (rows_in_partition)  // keys and row ids in ONE scatter (they used to be two kernels ranking the same bucket bytes: 5.0 + 2.5 ms per 1e9 rows)
    return radix_scatter_with_rows<kPartBits>(gb->bucket8, reinterpret_cast<const uint64_t*>(c.keys), reinterpret_cast<uint64_t*>(keys_part), gb->rows_part, n,
                                              gb->part_off, c.valid, c.key_off, st);
  // the keys alone: 17 instead of 21 B/row, and the pass of the value partition (4 waves per SIMD)
  return radix_scatter_only<kPartBits, uint64_t, uint8_t>(gb->bucket8, reinterpret_cast<const uint64_t*>(c.keys), nullptr, reinterpret_cast<uint64_t*>(keys_part), n, 0,
                                                          false, gb->part_off, st);
}

// One attempt with a table region per bucket in LDS (k_hash_probe_lds): one workgroup per bucket.
// bucket starts: the offsets row of tile 0 of the partition pass, or the searched starts after a second level
// skewed buckets (longer than 1.5x the average and 2^20 rows): head rows here, the rest in chunks (k_hash_probe_lds_tail)
static int probe_lds(const CreateCtx& c, HashPartition* hp, Slot* table, unsigned int cap, unsigned int region) {
  pdx_groupby* gb = c.gb;
  hipStream_t st = c.st;
  const int64_t n = c.n;
  const unsigned int pb = hp->pb;
  PDX_PROFILE("hash_probe_lds", st);
  const uint32_t* boff = hp->bucket_starts ? hp->bucket_starts : gb->part_off;
  const size_t nb = (size_t)1 << pb;
  int64_t head_rows = std::max<int64_t>((int64_t)1 << 20, (n >> pb) + (n >> (pb + 1)));
  if (c.t.head_rows) head_rows = c.t.head_rows;
  head_rows = (head_rows + 4 * kProbeBlock - 1) / (4 * kProbeBlock) * (4 * kProbeBlock);
  std::vector<TailChunk> chunks;
  if (n > head_rows) {
    std::vector<uint32_t> hoff(nb);
    PDX_HIP(hipMemcpyAsync(hoff.data(), boff, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PDX_HIP(hipStreamSynchronize(st));
    for (size_t bi = 0; bi < nb; ++bi) {
      const int64_t bs = hoff[bi], be = bi + 1 < nb ? (int64_t)hoff[bi + 1] : n;
      for (int64_t c0 = bs + head_rows; c0 < be; c0 += kTailChunkRows)
        chunks.push_back(TailChunk{(uint32_t)bi, (uint32_t)c0, (uint32_t)std::min<int64_t>(c0 + kTailChunkRows, be)});
    }
  }
  uint16_t* idx16 = pb == (unsigned)kPartBits ? gb->idx16_part : nullptr;
  hp->idx16_written = idx16 != nullptr;
  if (!chunks.empty() || pb != (unsigned)kPartBits) PDX_TRY(ensure_rows_part(gb, st));  // (the tail kernel tracks first rows per row)
  const bool first_as_pos = !c.valid && !gb->rows_part;
  if (c.valid)
    hipLaunchKernelGGL((k_hash_probe_lds<true>), dim3(1u << pb), dim3(kProbeBlock), 0, st, hp->keys_part, gb->rows_part, boff, n, table, cap, region,
                       gb->slot_part, c.ctl, pb, head_rows, idx16);
  else  // no null keys: rows_part is not read per row (first rows as positions), and with idx16 the 4-byte slot is not written
    hipLaunchKernelGGL((k_hash_probe_lds<false>), dim3(1u << pb), dim3(kProbeBlock), 0, st, hp->keys_part, gb->rows_part, boff, n, table, cap, region,
                       gb->slot_part, c.ctl, pb, head_rows, idx16);
  if (first_as_pos)
    hipLaunchKernelGGL(k_first_rows_from_pos, dim3((unsigned)(((int64_t)cap + 2 + 255) / 256)), dim3(256), 0, st, table, cap, region, gb->part_off,
                       hp->ntiles, gb->bucket8, n);
  if (!chunks.empty()) {
    TailChunk* dchunks = c.s.get<TailChunk>(chunks.size());
    if (c.s.failed) return PDX_OOM;
    PDX_HIP(hipMemcpyAsync(dchunks, chunks.data(), chunks.size() * sizeof(TailChunk), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hash_probe_lds_tail, dim3((unsigned)chunks.size()), dim3(kProbeBlock), 0, st, hp->keys_part, gb->rows_part, dchunks, table, cap,
                       region, gb->slot_part, c.ctl, pb, idx16);
    PDX_HIP(hipStreamSynchronize(st));  // `chunks` (pageable host memory) must outlive the copy
  }
  return PDX_OK;
}

// One attempt with the table in memory (k_hash_probe_part): regions too large for LDS, or a skewed bucket that outgrew it
static int probe_part(const CreateCtx& c, HashPartition* hp, Slot* table, unsigned int cap, unsigned int region, unsigned int limit) {
  pdx_groupby* gb = c.gb;
  hp->idx16_written = false;
  PDX_TRY(ensure_rows_part(gb, c.st));
  PDX_PROFILE("hash_probe_part", c.st);
  constexpr unsigned int kWindowBits = 16;  // 2^16 slots = 1 MB per bucket window; about two buckets are active at a time
  const unsigned int nsweeps = region > (1u << kWindowBits) ? region >> kWindowBits : 1u;
  for (unsigned int sw = 0; sw < nsweeps; ++sw)
    hipLaunchKernelGGL((k_hash_probe_part<4>), dim3((unsigned int)ceil_div(c.n, 1024 * kProbeTiles)), dim3(256), 0, c.st, hp->keys_part, gb->rows_part, c.n, table,
                       cap, region, limit, gb->slot_part, c.ctl, nsweeps > 1 ? kWindowBits : 31u, sw, hp->pb);
  return PDX_OK;
}

// the LDS attempt saw d distinct keys in its first r rows (an exact pair, taken after every bucket's first 4096 rows): the cardinality
// K that predicts, d = K (1 - exp(-r / K)) for uniformly mixed keys, and from it the groups among all n rows.  Too few repeats to tell
// means "more groups than the sample can resolve": min(n, 2^28) keys.  0: the attempt took no sample.
static double estimate_groups(unsigned long long rows_seen, unsigned long long est_distinct, int64_t n) {
  if (!rows_seen) return 0.0;
  const double d = (double)est_distinct, r = (double)rows_seen;
  if (!(r - d > 0.001 * r && r - d >= 512.0)) return std::min((double)n, 268435456.0);
  double lo = d, hi = 1e18;  // bisection on K
  for (int it = 0; it < 200; ++it) {
    double mid = std::sqrt(lo * hi);
    if (mid * -std::expm1(-r / mid) < d) lo = mid;
    else hi = mid;
  }
  return std::min((double)n, hi * -std::expm1(-(double)n / hi));
}

// Very many groups: instead of a table that falls out of the L2 (every probe and atomic then goes to memory: 1.4 s per 1e9
// rows measured), split the buckets by a second partition level until a bucket's table (<= 8192 slots at <= ~35 % load)
// fits in LDS again.  The second level is one more stable scatter of (key, row) by the next hash bits; the logical slot id
// keeps the (index << pb) | bucket form with pb = 8 + extra, so the later sort by slot just sees a longer partitioned prefix.
// Digit width of that level for `groups` groups, 0 when even 8 more bits leave the buckets too full.
static int split_bits(double groups) {
  int extra = 4;
  while (extra < 8 && groups / (double)((uint64_t)1 << (kPartBits + extra)) > 2800.0) ++extra;  // ~35 % load when there is room ...
  return groups / (double)((uint64_t)1 << (kPartBits + extra)) <= 4200.0 ? extra : 0;           // ... up to ~51 % at the last level (2.7e8 groups)
}
static int split_buckets(const CreateCtx& c, HashPartition* hp, int extra) {
  pdx_groupby* gb = c.gb;
  hipStream_t st = c.st;
  const int64_t n = c.n;
  PDX_TRY(ensure_rows_part(gb, st));
  gb->digit2 = gb->own<uint8_t>((size_t)n);
  gb->part_off2 = gb->own<uint32_t>((size_t)hp->ntiles << extra);
  uint32_t* chunk_sum2 = c.s.get<uint32_t>((size_t)(hp->nchunks + 1) << extra);
  long long* keys_part2 = c.s.get<long long>((size_t)n);
  uint32_t* rows_part2 = gb->own<uint32_t>((size_t)n);
  hp->bucket_starts = c.s.get<uint32_t>(((size_t)1 << (kPartBits + extra)) + 1);
  if (c.s.failed || !gb->digit2 || !gb->part_off2 || !rows_part2) return PDX_OOM;
  {
    PDX_PROFILE("hash_bucket_hist", st);
    with_digit_bits<4, 8>(extra, [&](auto b) {
      hipLaunchKernelGGL((k_hash_digit_hist<b()>), dim3((unsigned)hp->ntiles), dim3(kSortBlock), 0, st, hp->keys_part, gb->rows_part, n, kPartBits, gb->digit2,
                         gb->part_off2);
    });
  }
  int rc2 = radix_scan_dispatch(extra, gb->part_off2, hp->ntiles, chunk_sum2, true, st);
  if (rc2 == PDX_OK)
    rc2 = with_digit_bits<4, 8>(extra, [&](auto b) {
      PDX_TRY((radix_scatter_only<b(), uint64_t, uint8_t>(gb->digit2, reinterpret_cast<const uint64_t*>(hp->keys_part), nullptr,
                                                          reinterpret_cast<uint64_t*>(keys_part2), n, 0, false, gb->part_off2, st)));
      return radix_scatter_only<b(), uint32_t, uint8_t>(gb->digit2, gb->rows_part, nullptr, rows_part2, n, 0, false, gb->part_off2, st);
    });
  if (rc2 != PDX_OK) return rc2;
  hp->keys_part = keys_part2;
  gb->rows_part = rows_part2;  // (the first-level array stays owned by the handle until it is destroyed)
  hp->pb = kPartBits + extra;
  gb->digit2_bits = extra;
  hipLaunchKernelGGL(k_bucket_starts, dim3(grid_for((int64_t)1 << hp->pb, 256)), dim3(256), 0, st, hp->keys_part, gb->rows_part, n, hp->pb, hp->bucket_starts);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// General keys, from 2^18 rows: partition, then attempts until a table holds every key at <= 70 % load.  Each round: one attempt (LDS or
// memory side) -> read HashCtl -> accept, split the buckets by a second level, or grow the table.
static int build_hash_partitioned(const CreateCtx& c, SlotDomain* d) {
  pdx_groupby* gb = c.gb;
  hipStream_t st = c.st;
  const int64_t n = c.n;
  HashPartition hp;
  PDX_TRY(partition_by_bucket(c, &hp));
  const uint64_t want = std::max<uint64_t>(next_pow2((uint64_t)n * 2), 1u << 16);
  unsigned int cap = (unsigned int)std::min<uint64_t>(want, 1u << 21);
  unsigned int region = 0;
  TableBlock table;
  for (;;) {
    table.reset(alloc_table(cap));
    if (!table) return PDX_OOM;
    region = cap >> hp.pb;
    hipLaunchKernelGGL(k_table_init, dim3(grid_for((int64_t)cap + 2, 256, 4)), dim3(256), 0, st, table.get(), (int64_t)cap + 2);
    hipMemsetAsync(c.ctl, 0, sizeof(HashCtl), st);
    const unsigned int limit = (unsigned int)((uint64_t)cap * 7 / 10);
    const bool use_lds = region <= (unsigned)kLdsRegionMax && c.t.hash_lds && !hp.lds_failed_at_pb;
    PDX_TRY(use_lds ? probe_lds(c, &hp, table.get(), cap, region) : probe_part(c, &hp, table.get(), cap, region, limit));
    HashCtl h;
    hipError_t e = hipMemcpyAsync(&h, c.ctl, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "k_hash_probe_part");
    if (c.t.hash_debug)
      fprintf(stderr, "[pdx] hash build attempt: pb=%u cap=%u region=%u lds=%d inserted=%u overflow=%u rows_seen=%llu distinct_seen=%llu\n", hp.pb, cap,
              region, (int)use_lds, h.inserted, h.overflow, (unsigned long long)h.rows_seen, (unsigned long long)h.est_distinct);
    if (!h.overflow && h.inserted <= limit) break;
    table.reset();  // the rejected attempt's table goes back before anything else is allocated
    if (cap >= want * 4 || cap >= (1u << 30)) return fail(PDX_DEVICE, "pdx_groupby_create: hash table overflow at maximum capacity");
    if (use_lds && hp.pb > (unsigned)kPartBits) hp.lds_failed_at_pb = true;  // a skewed bucket outgrew LDS even after the split: memory-side build
    uint64_t next = (uint64_t)cap * 8;
    const double groups = estimate_groups(h.rows_seen, h.est_distinct, n);
    if (h.rows_seen) next = std::max<uint64_t>(next, next_pow2((uint64_t)(groups / 0.4) + 1));  // aim at <= 40 % load: the estimate is noisy
    const int extra = c.t.hash_split && hp.pb == (unsigned)kPartBits && groups > 0.0 && next > (1u << 21) && c.t.hash_lds ? split_bits(groups) : 0;
    if (extra) {
      PDX_TRY(split_buckets(c, &hp, extra));
      cap = (unsigned int)kLdsRegionMax << hp.pb;
    } else {
      cap = (unsigned int)std::min<uint64_t>(std::max<uint64_t>(next, (uint64_t)cap * 2), std::max<uint64_t>(want * 4, 1u << 16));
    }
  }
  gb->part_bits = (int)hp.pb;
  if (!hp.idx16_written) gb->idx16_part = nullptr;  // (the block stays owned by the handle; nothing reads it)
  gb->slot_part_ready = !hp.idx16_written;          // the LDS build at the first level writes the 2-byte region indexes only
  gb->owned.push_back(table.get());
  d->table = table.release();
  Slot sp[2];
  PDX_HIP(hipMemcpyAsync(sp, d->table + cap, sizeof(sp), hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));
  gb->special_slots = sp[0].first != kNoRow || sp[1].first != kNoRow;
  d->region = region;
  d->null_slot = cap;
  d->nslots = (int64_t)cap + 2;
  return PDX_OK;
}

// Small inputs (or PDX_HASH_PARTITION=0): one open-addressing table over the rows as they stand.
// table capacity: start at min(2^21, pow2 >= 2n) and grow x8 whenever more than 70 % of the slots fill up
static int build_hash_global(const CreateCtx& c, SlotDomain* d) {
  pdx_groupby* gb = c.gb;
  hipStream_t st = c.st;
  const int64_t n = c.n;
  gb->slot_of_row = gb->own<uint32_t>((size_t)n);
  if (!gb->slot_of_row) return PDX_OOM;
  const uint64_t want = next_pow2((uint64_t)n * 2);
  unsigned int cap = (unsigned int)std::min<uint64_t>(want, 1u << 21);
  TableBlock table;
  for (;;) {
    table.reset(alloc_table(cap));
    if (!table) return PDX_OOM;
    hipLaunchKernelGGL(k_table_init, dim3(grid_for((int64_t)cap + 2, 256, 4)), dim3(256), 0, st, table.get(), (int64_t)cap + 2);
    hipMemsetAsync(c.ctl, 0, sizeof(HashCtl), st);
    unsigned int limit = (unsigned int)((uint64_t)cap * 7 / 10);
    if (cap >= want) limit = cap;  // a table of >= 2n slots can never overflow
    {
      PDX_PROFILE("hash_insert", st);
      hipLaunchKernelGGL(k_hash_insert, dim3(grid_for(n, 256, 8)), dim3(256), 0, st, c.keys, c.valid, c.key_off, n, table.get(), cap, limit, gb->slot_of_row, c.ctl);
    }
    HashCtl h;
    hipError_t e = hipMemcpyAsync(&h, c.ctl, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "k_hash_insert");
    if (!h.overflow) break;
    table.reset();  // the rejected attempt's table goes back before anything else is allocated
    if (cap >= want) return fail(PDX_DEVICE, "pdx_groupby_create: hash table overflow at maximum capacity");
    cap = (unsigned int)std::min<uint64_t>((uint64_t)cap * 8, want);
  }
  gb->owned.push_back(table.get());
  d->table = table.release();
  d->null_slot = cap;
  d->nslots = (int64_t)cap + 2;
  return PDX_OK;
}

// Every path: the occupied slots of `d` compacted in slot order, then dense group ids in FIRST-OCCURRENCE order with the groups' keys
// and first rows.  Sets gb->G.
static int finish_group_ids(const CreateCtx& c, const SlotDomain& d) {
  pdx_groupby* gb = c.gb;
  Scratch& s = c.s;
  hipStream_t st = c.st;
  const int64_t n = c.n, nslots = d.nslots;
  gb->nslots = nslots;
  gb->slot_bits = ilog2((uint64_t)nslots);
  gb->gid_of_slot = gb->own<uint32_t>((size_t)nslots);
  // occupied slots in slot order
  uint32_t* occ_slot_tmp = s.get<uint32_t>((size_t)std::min<int64_t>(nslots, n + 2));
  uint32_t* occ_first_tmp = s.get<uint32_t>((size_t)std::min<int64_t>(nslots, n + 2));
  if (s.failed || !gb->gid_of_slot) return PDX_OOM;
  int64_t G = 0;
  PDX_TRY(compact_indices(nslots, OccPred{d.table, d.dense_first, d.region, d.null_slot},
                          OccEmit{d.table, d.dense_first, d.region, d.null_slot, occ_slot_tmp, occ_first_tmp}, &G, s, st));
  gb->G = G;
  gb->occ_slot = gb->own<uint32_t>((size_t)G);
  gb->gid_of_occ = gb->own<uint32_t>((size_t)G);
  gb->uniques = gb->own<int64_t>((size_t)G);
  gb->unique_ok = gb->own<uint8_t>((size_t)G);
  gb->first_rows = gb->own<int64_t>((size_t)G);
  if (s.failed || !gb->occ_slot || !gb->gid_of_occ || !gb->uniques || !gb->unique_ok || !gb->first_rows) return PDX_OOM;
  hipMemcpyAsync(gb->occ_slot, occ_slot_tmp, (size_t)G * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
  // order groups by first occurrence: gid = rank of the group's first row among all first rows (bit map + block prefix, no sort).
  // Nearly every row its own group: the random bit sets / word reads of the map cost more than sorting the (first row, slot)
  // pairs (measured at 1.5e8 groups of 2.5e8 rows, pdx_reindex_indices: 65 ms with the map -- 5.6 ms of bit sets, > 10 ms of rank
  // reads -- against 54 ms with the sort)
  const bool rank_by_sort = G > ((int64_t)1 << 22) && G * 8 > n;
  const int g = grid_for(G, 256);
  if (rank_by_sort) {
    uint32_t* k0 = s.get<uint32_t>((size_t)G);
    uint32_t* v0 = s.get<uint32_t>((size_t)G);
    uint32_t* k1 = s.get<uint32_t>((size_t)G);
    uint32_t* v1 = s.get<uint32_t>((size_t)G);
    PDX_SCRATCH_CHECK(s);
    const uint32_t *ks = nullptr, *vs = nullptr;  // sort (first_row -> slot); first rows are distinct so any order of ties is moot
    PDX_TRY(radix_sort_pairs<uint32_t>(occ_first_tmp, occ_slot_tmp, k0, v0, k1, v1, G, ilog2((uint64_t)n + 1) < 31 ? ilog2((uint64_t)n + 1) : 31, &ks, &vs, true,
                                       s, st));
    hipLaunchKernelGGL(k_assign_gids, dim3(g), dim3(256), 0, st, d.table, d.dense_min, d.dense_mask, gb->gid_of_slot, ks, vs, G, d.null_slot, gb->uniques,
                       gb->unique_ok, gb->first_rows, d.region);
    hipLaunchKernelGGL(k_gid_of_occ, dim3(g), dim3(256), 0, st, gb->gid_of_slot, gb->occ_slot, G, gb->gid_of_occ);
  } else {
    const int64_t nwords = (n + 63) >> 6, nrb = ceil_div(nwords, (int64_t)kRankWords);
    unsigned long long* bits = s.get<unsigned long long>((size_t)nwords);
    int64_t* block_pre = s.get<int64_t>((size_t)nrb);
    PDX_SCRATCH_CHECK(s);
    PDX_HIP(hipMemsetAsync(bits, 0, (size_t)nwords * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_mark_first_rows, dim3(g), dim3(256), 0, st, occ_first_tmp, G, bits);
    hipLaunchKernelGGL(k_rank_block_counts, dim3(grid_for(nrb * kRankWords, 256)), dim3(256), 0, st, bits, nwords, nrb, block_pre);
    PDX_TRY((device_exclusive_scan<int64_t, SumOp>(block_pre, block_pre, nrb, (int64_t*)nullptr, s, st)));
    hipLaunchKernelGGL(k_assign_gids_ranked, dim3(g), dim3(256), 0, st, d.table, d.dense_min, d.dense_mask, gb->gid_of_slot, occ_first_tmp, occ_slot_tmp, G, bits,
                       block_pre, d.null_slot, gb->uniques, gb->unique_ok, gb->first_rows, d.region, gb->gid_of_occ);
  }
  return PDX_OK;
}
