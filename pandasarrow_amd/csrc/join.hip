// join.hip -- hash equi-join of two key columns for gfx950: pdx_join_create / pdx_join_rows / pdx_join_indices.  The
// reference advertises "merging and joining" and has no implementation to cite; the semantics are Arrow's hash join (a null key matches
// nothing) with a fully defined row order (left row, then right row; the unmatched right rows of an OUTER join behind them).
//
// Build (right side): the group-by handle gives the distinct keys in first-occurrence order and, through pdx_groupby_groupings, the rows
// of every key in row order; the distinct keys go into lookup_table.hpp's open-addressing table (key -> group id), probed from LDS up to
// kLkLdsMaxEntries keys and from global memory beyond.  Probe + count: one pass over the left keys writes, per row, where its matches
// start in the grouped row list (-1: none) and how many output rows it makes; OUTER also marks the group as matched (a plain store of 1).
// Offsets: scan.hpp's exclusive scan of the counts; the total is the one value the create call reads back.
// Expand (k_join_expand) is output-parallel: a workgroup owns kJoinTile consecutive OUTPUT rows, finds the left rows that cover them by
// two binary searches of the offsets (one wave each, once per tile), stages that window of offsets in LDS, and every lane then resolves
// and writes its own output rows -- so one hot key is spread over as many workgroups as its matches fill, and left rows without output
// are never visited.  No atomics; the two index columns leave through 16-byte nontemporal stores.
// SEMI / ANTI and the OUTER tail are ordered compactions (compact.hpp) done in the create call, where their sizes are needed anyway.
#include <stdio.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "colview.hpp"
#include "compact.hpp"
#include "lookup_table.hpp"
#include "scan.hpp"
#include "stream_io.hpp"

struct pdx_join {
  int how = 0;
  int64_t nl = 0, nr = 0, G = 0;
  int64_t expand_rows = 0;  // rows the expand kernel writes (INNER / LEFT / the LEFT part of OUTER)
  int64_t list_rows = 0;    // rows of `list`: the OUTER tail, the SEMI / ANTI result
  int64_t right_nulls = 0;  // left rows without a match (LEFT / OUTER: their right index is null)
  int64_t* start = nullptr;     // [nl] where a left row's matches begin in grp_rows, -1: no match
  int64_t* offs = nullptr;      // [nl] the first output row of every left row
  int64_t* grp_rows = nullptr;  // [nr] the right rows, grouped by key, each group ascending
  int64_t* list = nullptr;      // [list_rows] ascending row numbers
  std::string plan = "plan=empty build_rows=0 distinct=0 out_rows=0";
  hipStream_t stream = nullptr;  // the last stream that used the handle's buffers
  std::vector<void*> owned;
  template <typename T>
  T* own(size_t count) {
    T* p = static_cast<T*>(pdx::pool_alloc((count ? count : 1) * sizeof(T)));
    if (p) owned.push_back(p);
    return p;
  }
  int64_t rows() const { return how == PDX_JOIN_SEMI || how == PDX_JOIN_ANTI ? list_rows : expand_rows + list_rows; }
  ~pdx_join() {
    pdx::StreamNote note(stream);
    pdx::pool_free_many(owned.data(), (int)owned.size());
  }
};

namespace pdx {

constexpr int kJoinBlock = 256;
constexpr int kJoinTile = 2048;    // output rows of one workgroup: 4 steps of 256 lanes x 2 neighbouring rows (one 16-byte store per column)
constexpr int kJoinWindow = 2048;  // left rows whose offsets a workgroup stages in LDS (16 KB); a longer window is searched where it lies
constexpr int kJoinSteps = kJoinTile / (2 * kJoinBlock);

// ---------------------------------------------------------------- probe + count
struct JoinProbe {
  const void* keys;      // the left keys, element offset applied
  const uint8_t* valid;  // nullptr: every row is valid
  int64_t voff, n;
  const unsigned long long* tkeys;  // the table: [mask + 1] keys and group ids
  const uint32_t* tpos;
  uint32_t mask;
  const int64_t* grp_offs;  // [G + 1]; nullptr for SEMI / ANTI
  int how;
  int64_t* start;                 // INNER / LEFT / OUTER
  int64_t* cnt;                   // INNER / LEFT / OUTER: output rows of the left row
  uint8_t* flag;                  // SEMI / ANTI: 1 = the row is part of the result
  uint8_t* matched;               // OUTER: [G]
  unsigned long long* unmatched;  // the left rows without a match
};

extern __shared__ __attribute__((aligned(16))) unsigned char join_smem[];

template <typename U, bool LDS>
__global__ void __launch_bounds__(kJoinBlock) k_join_probe(const JoinProbe a) {
  const uint32_t mask = a.mask;
  const unsigned long long* keys = a.tkeys;
  const uint32_t* pos = a.tpos;
  if constexpr (LDS) {
    unsigned long long* skeys = reinterpret_cast<unsigned long long*>(join_smem);
    uint32_t* spos = reinterpret_cast<uint32_t*>(join_smem + ((size_t)mask + 1) * sizeof(unsigned long long));
    for (uint32_t h = threadIdx.x; h <= mask; h += kJoinBlock) {
      skeys[h] = a.tkeys[h];
      spos[h] = a.tpos[h];
    }
    __syncthreads();
    keys = skeys;
    pos = spos;
  }
  const U* __restrict__ v = static_cast<const U*>(a.keys);
  const int64_t stride = (int64_t)gridDim.x * kJoinBlock;
  unsigned long long nc = 0;
  for (int64_t i = (int64_t)blockIdx.x * kJoinBlock + threadIdx.x; i < a.n; i += stride) {
    const bool ok = !a.valid || bit_get(a.valid, a.voff + i);  // (a null key matches nothing)
    const int32_t g = ok ? lk_find<unsigned long long>(keys, pos, mask, (unsigned long long)v[i]) : -1;
    int64_t s0 = -1, c = 0;
    if (g < 0) {
      ++nc;
    } else if (a.grp_offs) {
      s0 = a.grp_offs[g];
      c = a.grp_offs[g + 1] - s0;
    }
    if (a.how == PDX_JOIN_SEMI || a.how == PDX_JOIN_ANTI) {
      a.flag[i] = (uint8_t)((g >= 0) == (a.how == PDX_JOIN_SEMI));
    } else {
      if (g < 0 && a.how != PDX_JOIN_INNER) c = 1;  // the row is kept, with a null right index
      if (g >= 0 && a.how == PDX_JOIN_OUTER) a.matched[g] = 1;  // (every writer stores the same value)
      a.start[i] = s0;
      a.cnt[i] = c;
    }
  }
  wave_add_nulls(a.unmatched, (int)(threadIdx.x & 63), nc);
}

// ---------------------------------------------------------------- expand
struct JoinExpand {
  const int64_t* offs;      // [nl] exclusive scan of the counts
  const int64_t* start;     // [nl]
  const int64_t* grp_rows;  // [nr]
  int64_t nl, nr, total;
  int64_t* out_left;
  int64_t* out_right;
  uint8_t* lvalid;  // may be nullptr
  uint8_t* rvalid;  // may be nullptr
  int vec;          // both outputs start on a 16-byte boundary
};

// the number of entries of offs[0, n) that are <= x (offs ascends).  Every operand is wave-uniform: the whole wave walks one path and
// its loads share an address, 27 steps for 1e8 rows.
__device__ __forceinline__ int64_t join_upper_bound(const int64_t* __restrict__ offs, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (offs[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kJoinBlock) k_join_expand(const JoinExpand a) {
  __shared__ int64_t win[kJoinWindow];
  __shared__ int64_t bound[2];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t t0 = (int64_t)blockIdx.x * kJoinTile;
  const int64_t t1 = t0 + kJoinTile < a.total ? t0 + kJoinTile : a.total;
  // merge-path partition, once per tile: the last left row that starts at or before the tile's first / last output row
  if (wave < 2) {
    const int64_t ub = join_upper_bound(a.offs, a.nl, wave == 0 ? t0 : t1 - 1);
    if (lane == 0) bound[wave] = ub - 1;  // (offs[0] == 0 <= t0: ub >= 1)
  }
  __syncthreads();
  const int64_t i_lo = bound[0], i_hi = bound[1];
  const int64_t W = i_hi - i_lo + 1;
  const bool staged = W <= kJoinWindow;  // (the same in the whole workgroup)
  if (staged) {
    for (int64_t j = threadIdx.x; j < W; j += kJoinBlock) win[j] = a.offs[i_lo + j];
    __syncthreads();
  }
  const int64_t* __restrict__ goffs = a.offs + i_lo;
  // the last row j of the window, from `from` on, with offs[j] <= p; *off = that offset
  auto find = [&](int64_t p, int64_t from, int64_t* off) -> int64_t {
    int64_t lo = from, hi = W - 1;  // (the answer lies in [lo, hi]: offs[from] <= p, and the row behind the window starts behind the tile)
    if (staged) {
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (win[mid] <= p) lo = mid;
        else hi = mid - 1;
      }
      *off = win[lo];
    } else {
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (goffs[mid] <= p) lo = mid;
        else hi = mid - 1;
      }
      *off = goffs[lo];
    }
    return lo;
  };
#pragma unroll 1
  for (int s = 0; s < kJoinSteps; ++s) {
    const int64_t wbase = t0 + (int64_t)s * (2 * kJoinBlock) + (int64_t)wave * 128;  // the wave's 128 rows: two validity words
    if (wbase >= t1) break;                                                           // (wave-uniform)
    const int64_t p = wbase + 2 * lane;
    int64_t li[2] = {0, 0}, ri[2] = {0, 0};
    bool rok[2] = {false, false};
    int64_t from = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      if (p + e < t1) {
        int64_t off;
        const int64_t j = find(p + e, from, &off);
        from = j;
        const int64_t i = i_lo + j;
        const int64_t s0 = a.start[i];
        li[e] = i;
        if (s0 >= 0) {
          int64_t q = s0 + (p + e - off);
          q = q < 0 ? 0 : q >= a.nr ? a.nr - 1 : q;  // (always inside by construction; never read outside whatever the inputs)
          ri[e] = a.grp_rows[q];
          rok[e] = true;
        }
      }
    }
    if (a.vec && p + 1 < t1) {
      i64x2 l, r;
      l.x = li[0];
      l.y = li[1];
      r.x = ri[0];
      r.y = ri[1];
      st_stream<kStreamJoinOut>(reinterpret_cast<i64x2*>(a.out_left + p), l);
      st_stream<kStreamJoinOut>(reinterpret_cast<i64x2*>(a.out_right + p), r);
    } else {
#pragma unroll
      for (int e = 0; e < 2; ++e)
        if (p + e < t1) {
          st_stream<kStreamJoinOut>(a.out_left + p + e, li[e]);
          st_stream<kStreamJoinOut>(a.out_right + p + e, ri[e]);
        }
    }
    const uint64_t b0 = __ballot(rok[0]), b1 = __ballot(rok[1]);
    const int64_t w = wbase >> 6;
    if (a.rvalid) {
      store_bits_wave(a.rvalid, w, a.total, lk_spread(b0) | (lk_spread(b1) << 1), lane);
      store_bits_wave(a.rvalid, w + 1, a.total, lk_spread(b0 >> 32) | (lk_spread(b1 >> 32) << 1), lane);
    }
    if (a.lvalid) {
      store_bits_wave(a.lvalid, w, a.total, ~0ull, lane);
      store_bits_wave(a.lvalid, w + 1, a.total, ~0ull, lane);
    }
  }
}

// ---------------------------------------------------------------- the OUTER tail, and bit ranges of a validity bitmap
__global__ void k_join_tail(const int64_t* __restrict__ list, int64_t m, int64_t* __restrict__ out_left, int64_t* __restrict__ out_right) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    out_left[j] = 0;
    out_right[j] = list[j];
  }
}
// bits [start, start + count) of `bits` := value; a thread owns a byte, the bits of the two edge bytes outside the range are kept
__global__ void k_join_fill_bits(uint8_t* __restrict__ bits, int64_t start, int64_t count, int value) {
  const int64_t b0 = start >> 3, b1 = (start + count - 1) >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = b0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= b1; b += stride) {
    const int64_t lo = start > (b << 3) ? start - (b << 3) : 0;
    const int64_t hi = start + count < (b << 3) + 8 ? start + count - (b << 3) : 8;
    const uint32_t m = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    if (m == 0xFFu) bits[b] = value ? 0xFF : 0;
    else bits[b] = (uint8_t)(value ? (bits[b] | m) : (bits[b] & ~m));
  }
}

struct JoinFlagPred {
  const uint8_t* flag;
  __device__ bool operator()(int64_t i) const { return flag[i] != 0; }
};
struct JoinTailPred {  // a right row whose key no left row matched (the null key's group is never matched)
  const uint32_t* ids;
  const uint8_t* matched;
  __device__ bool operator()(int64_t r) const { return matched[ids[r]] == 0; }
};
struct JoinRowEmit {
  int64_t* out;
  __device__ void operator()(int64_t pos, int64_t i) const { out[pos] = i; }
};
// compact_indices with the total left on the device (the create call reads everything back at once)
template <typename Pred>
static int join_compact(int64_t n, Pred pred, int64_t* out, int64_t* total_dev, Scratch& s, hipStream_t st) {
  if (n <= 0) return PDX_OK;
  const int64_t nblocks = ceil_div(n, kCompactTile);
  int64_t* counts = s.get<int64_t>((size_t)nblocks);
  PDX_SCRATCH_CHECK(s);
  hipLaunchKernelGGL((k_compact_count<Pred>), dim3((unsigned)nblocks), dim3(kCompactBlock), 0, st, n, pred, counts);
  PDX_TRY((device_exclusive_scan<int64_t, SumOp>(counts, counts, nblocks, total_dev, s, st)));
  hipLaunchKernelGGL((k_compact_write<Pred, JoinRowEmit>), dim3((unsigned)nblocks), dim3(kCompactBlock), 0, st, n, pred, JoinRowEmit{out}, counts);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

static bool join_key_dtype(int dt) { return is_int_like(dt) || dt == PDX_INT32; }

// a 4-byte key column as the 8-byte column the group-by takes (zero-extended, the validity keeps its bit offset)
static int join_wide_key(const pdx_column* a, pdx_column* key, Scratch& s, hipStream_t st) {
  *key = *a;
  if (!is_narrow(a->dtype)) return PDX_OK;
  const int64_t off7 = a->offset & 7;
  unsigned long long* wide = s.get<unsigned long long>((size_t)(a->length + off7));
  PDX_SCRATCH_CHECK(s);
  hipLaunchKernelGGL(k_lk_widen, dim3(grid_for(a->length, 256, 4)), dim3(256), 0, st, static_cast<const uint32_t*>(a->values) + a->offset, a->length, wide + off7);
  PDX_LAUNCH_CHECK();
  key->dtype = PDX_UINT64;
  key->values = wide;
  key->offset = off7;
  key->validity = a->validity ? static_cast<const uint8_t*>(a->validity) + (a->offset >> 3) : nullptr;
  return PDX_OK;
}

template <typename U>
static void join_probe_launch(bool lds, size_t shmem, int grid, hipStream_t st, const JoinProbe& p) {
  if (lds) hipLaunchKernelGGL((k_join_probe<U, true>), dim3(grid), dim3(kJoinBlock), shmem, st, p);
  else hipLaunchKernelGGL((k_join_probe<U, false>), dim3(grid), dim3(kJoinBlock), 0, st, p);
}

static int join_create(pdx_join* j, const pdx_column* left, const pdx_column* right, void* stream, hipStream_t st) {
  const int64_t nl = left->length, nr = right->length;
  const int how = j->how;
  const bool listed = how == PDX_JOIN_SEMI || how == PDX_JOIN_ANTI;
  Scratch s;
  PDX_PROFILE("join_create", st);
  // ---- build: the right rows grouped by key
  int64_t G = 0;
  unsigned long long* uniq = nullptr;
  uint8_t* uvalid = nullptr;
  int64_t* grp_offs = nullptr;
  uint32_t* ids = nullptr;
  if (nr > 0) {
    pdx_column key;
    PDX_TRY(join_wide_key(right, &key, s, st));
    pdx_groupby* gb = nullptr;
    PDX_TRY(pdx_groupby_create(&key, stream, &gb));
    struct Closer {
      pdx_groupby* g;
      ~Closer() { pdx_groupby_destroy(g); }
    } closer{gb};
    G = pdx_groupby_num_groups(gb);
    if (G <= 0 || G > nr) return fail(PDX_DEVICE, "pdx_join_create: the group-by returned an impossible group count");
    uniq = s.get<unsigned long long>((size_t)G);
    uvalid = s.get<uint8_t>((size_t)((G + 7) / 8 + 8));
    grp_offs = s.get<int64_t>((size_t)G + 1);
    if (how == PDX_JOIN_OUTER) ids = s.get<uint32_t>((size_t)nr);
    PDX_SCRATCH_CHECK(s);
    if (!listed) {
      j->grp_rows = j->own<int64_t>((size_t)nr);
      if (!j->grp_rows) return PDX_OOM;
    }
    pdx_mut_column um{};
    um.dtype = key.dtype;
    um.length = G;
    um.values = uniq;
    um.validity = uvalid;
    PDX_TRY(pdx_groupby_unique_keys(gb, &um, stream));
    if (!listed) PDX_TRY(pdx_groupby_groupings(gb, j->grp_rows, grp_offs, stream));  // (SEMI / ANTI only ask whether a key occurs)
    if (ids) PDX_TRY(pdx_groupby_group_ids(gb, ids, stream));
    note_stream(st);
  }
  j->G = G;
  // ---- the table: distinct key -> group id
  const uint64_t slots = lk_slots_for(G);
  const uint32_t mask = (uint32_t)(slots - 1);
  const bool lds = G <= lookup_lds_max();
  uint32_t* pos = s.get<uint32_t>((size_t)slots + 1);  // [slots]: the null key's group (not used here)
  unsigned long long* tkeys = s.get<unsigned long long>((size_t)slots);
  unsigned long long* ctl = s.get<unsigned long long>(4);  // [0] expand rows, [1] list rows, [2] left rows without a match
  uint8_t* matched = how == PDX_JOIN_OUTER ? s.get<uint8_t>((size_t)std::max<int64_t>(G, 1)) : nullptr;
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemsetAsync(pos, 0xFF, sizeof(uint32_t) * ((size_t)slots + 1), st));
  PDX_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 4, st));
  if (matched) PDX_HIP(hipMemsetAsync(matched, 0, (size_t)std::max<int64_t>(G, 1), st));
  if (G > 0) hipLaunchKernelGGL(k_lk_insert<unsigned long long>, dim3(grid_for(G, 256, 4)), dim3(256), 0, st, uniq, uvalid, (int64_t)0, G, pos, mask, pos + slots);
  hipLaunchKernelGGL(k_lk_keys<unsigned long long>, dim3(grid_for((int64_t)slots, 256, 4)), dim3(256), 0, st, uniq, pos, slots, tkeys);
  PDX_LAUNCH_CHECK();
  // ---- probe + count
  uint8_t* flag = nullptr;
  if (nl > 0) {
    if (listed) {
      flag = s.get<uint8_t>((size_t)nl);
      j->list = j->own<int64_t>((size_t)nl);
      PDX_SCRATCH_CHECK(s);
      if (!j->list) return PDX_OOM;
    } else {
      j->start = j->own<int64_t>((size_t)nl);
      j->offs = j->own<int64_t>((size_t)nl);
      if (!j->start || !j->offs) return PDX_OOM;
    }
    JoinProbe p{};
    p.keys = static_cast<const char*>(left->values) + (size_t)left->offset * (size_t)dtype_bytes(left->dtype);
    p.valid = validity_or_null(left);
    p.voff = left->offset;
    p.n = nl;
    p.tkeys = tkeys;
    p.tpos = pos;
    p.mask = mask;
    p.grp_offs = listed ? nullptr : grp_offs;
    p.how = how;
    p.start = j->start;
    p.cnt = j->offs;
    p.flag = flag;
    p.matched = matched;
    p.unmatched = &ctl[2];
    const size_t shmem = lds ? (size_t)slots * (sizeof(unsigned long long) + sizeof(uint32_t)) : 0;
    // lds: as many workgroups as stay resident (each one copies the table once), every thread strides over the rows
    const int resident = lds ? (int)std::max<size_t>(1, std::min<size_t>(8, (size_t)(160 * 1024) / std::max<size_t>(shmem, 1))) : 8;
    const int grid = grid_for(nl, kJoinBlock, 4, kCUs * resident);
    if (is_narrow(left->dtype)) join_probe_launch<uint32_t>(lds, shmem, grid, st, p);
    else join_probe_launch<unsigned long long>(lds, shmem, grid, st, p);
    PDX_LAUNCH_CHECK();
    // ---- offsets / the SEMI, ANTI rows
    if (listed) PDX_TRY(join_compact(nl, JoinFlagPred{flag}, j->list, reinterpret_cast<int64_t*>(&ctl[1]), s, st));
    else PDX_TRY((device_exclusive_scan<int64_t, SumOp>(j->offs, j->offs, nl, reinterpret_cast<int64_t*>(&ctl[0]), s, st)));
  }
  // ---- the OUTER tail: the right rows of the groups that no left row matched, in row order
  if (how == PDX_JOIN_OUTER && nr > 0) {
    j->list = j->own<int64_t>((size_t)nr);
    if (!j->list) return PDX_OOM;
    PDX_TRY(join_compact(nr, JoinTailPred{ids, matched}, j->list, reinterpret_cast<int64_t*>(&ctl[1]), s, st));
  }
  unsigned long long h[4];
  PDX_TRY(read_back(h, ctl, sizeof(h), st));  // the one host wait of the join's own kernels
  j->expand_rows = (int64_t)h[0];
  j->list_rows = (int64_t)h[1];
  j->right_nulls = how == PDX_JOIN_LEFT || how == PDX_JOIN_OUTER ? (int64_t)h[2] : 0;
  j->plan = std::string("plan=") + (nr == 0 ? "empty" : lds ? "lds" : "global") + " build_rows=" + std::to_string(nr) + " distinct=" + std::to_string(G) +
            " out_rows=" + std::to_string(j->rows());
  return PDX_OK;
}

}  // namespace pdx

using namespace pdx;

extern "C" int pdx_join_create(const pdx_column* left_key, const pdx_column* right_key, int how, void* stream, pdx_join** out) {
  const char* who = "pdx_join_create";
  if (!left_key || !right_key || !out) return fail(PDX_INVALID, "pdx_join_create: null argument");
  *out = nullptr;
  if (how < PDX_JOIN_INNER || how > PDX_JOIN_ANTI) return fail(PDX_INVALID, "pdx_join_create: how is one of PDX_JOIN_INNER .. PDX_JOIN_ANTI");
  for (const pdx_column* c : {left_key, right_key})
    if (c->dtype == PDX_FLOAT64 || c->dtype == PDX_FLOAT32 || c->dtype == PDX_BOOL)
      return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": " + dtype_name(c->dtype) + " keys are not supported (int64, uint64, timestamp[ns] and int32 are)");
  PDX_TRY(check_column(left_key, who, true));
  PDX_TRY(check_column(right_key, who, true));
  if (!join_key_dtype(left_key->dtype) || !join_key_dtype(right_key->dtype)) return fail(PDX_INVALID, "pdx_join_create: unknown key dtype");
  if (left_key->dtype != right_key->dtype)
    return fail(PDX_INVALID, std::string(who) + ": the left key is " + dtype_name(left_key->dtype) + ", the right key " + dtype_name(right_key->dtype) + " (cast one side first)");
  if (left_key->length > 0x7FFFFFFFll || right_key->length > 0x7FFFFFFFll)
    return fail(PDX_NOT_IMPLEMENTED, "pdx_join_create: more than 2^31-1 rows per side is not supported yet (the group-by handle's row limit)");
  hipStream_t st = as_stream(stream);
  std::unique_ptr<pdx_join> j(new pdx_join());
  j->how = how;
  j->nl = left_key->length;
  j->nr = right_key->length;
  j->stream = st;
  PDX_TRY(join_create(j.get(), left_key, right_key, stream, st));
  *out = j.release();
  return PDX_OK;
}

extern "C" int pdx_join_rows(const pdx_join* j, int64_t* out_rows) {
  if (!j || !out_rows) return fail(PDX_INVALID, "pdx_join_rows: null argument");
  *out_rows = j->rows();
  return PDX_OK;
}

extern "C" int pdx_join_indices(pdx_join* j, pdx_mut_column* out_left, pdx_mut_column* out_right, void* stream) {
  const char* who = "pdx_join_indices";
  if (!j) return fail(PDX_INVALID, "pdx_join_indices: null handle");
  const int how = j->how;
  const bool listed = how == PDX_JOIN_SEMI || how == PDX_JOIN_ANTI;
  const int64_t rows = j->rows();
  PDX_TRY(check_out(who, out_left, PDX_INT64, rows));
  if (listed) {
    if (out_right) return fail(PDX_INVALID, "pdx_join_indices: a SEMI / ANTI join has no right indices (out_right must be NULL)");
  } else {
    PDX_TRY(check_out(who, out_right, PDX_INT64, rows));
    if (how != PDX_JOIN_INNER && !out_right->validity)
      return fail(PDX_INVALID, "pdx_join_indices: out_right needs a validity buffer (a left row without a match has a null right index)");
    if (how == PDX_JOIN_OUTER && !out_left->validity)
      return fail(PDX_INVALID, "pdx_join_indices: out_left needs a validity buffer (an unmatched right row has a null left index)");
  }
  hipStream_t st = as_stream(stream);
  j->stream = st;
  out_left->length = rows;
  out_left->null_count = how == PDX_JOIN_OUTER ? j->list_rows : 0;
  if (out_right) {
    out_right->length = rows;
    out_right->null_count = j->right_nulls;
  }
  if (rows == 0) return PDX_OK;
  PDX_PROFILE("join_indices", st);
  int64_t* ol = static_cast<int64_t*>(out_left->values);
  uint8_t* lv = static_cast<uint8_t*>(out_left->validity);
  if (listed) {
    PDX_HIP(hipMemcpyAsync(ol, j->list, sizeof(int64_t) * (size_t)rows, hipMemcpyDeviceToDevice, st));
    if (lv) hipLaunchKernelGGL(k_join_fill_bits, dim3(grid_for((rows + 7) / 8 + 1, 256)), dim3(256), 0, st, lv, (int64_t)0, rows, 1);
    PDX_LAUNCH_CHECK();
    return PDX_OK;
  }
  int64_t* orr = static_cast<int64_t*>(out_right->values);
  uint8_t* rv = static_cast<uint8_t*>(out_right->validity);
  const int64_t L = j->expand_rows, T = j->list_rows;
  if (L > 0) {
    JoinExpand e{};
    e.offs = j->offs;
    e.start = j->start;
    e.grp_rows = j->grp_rows;
    e.nl = j->nl;
    e.nr = j->nr;
    e.total = L;
    e.out_left = ol;
    e.out_right = orr;
    e.lvalid = lv;
    e.rvalid = rv;
    e.vec = aligned16(ol) && aligned16(orr);
    hipLaunchKernelGGL(k_join_expand, dim3((unsigned)ceil_div(L, kJoinTile)), dim3(kJoinBlock), 0, st, e);
  }
  if (T > 0) {  // OUTER: the unmatched right rows behind the LEFT part
    hipLaunchKernelGGL(k_join_tail, dim3(grid_for(T, 256, 4)), dim3(256), 0, st, j->list, T, ol + L, orr + L);
    hipLaunchKernelGGL(k_join_fill_bits, dim3(grid_for((T + 7) / 8 + 1, 256)), dim3(256), 0, st, lv, L, T, 0);
    hipLaunchKernelGGL(k_join_fill_bits, dim3(grid_for((T + 7) / 8 + 1, 256)), dim3(256), 0, st, rv, L, T, 1);
  }
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

extern "C" int pdx_join_last_plan(const pdx_join* j, char* buf, size_t buf_len) {
  if (!j || !buf || !buf_len) return fail(PDX_INVALID, "pdx_join_last_plan: null argument");
  snprintf(buf, buf_len, "%s", j->plan.c_str());
  return PDX_OK;
}

extern "C" int pdx_join_destroy(pdx_join* j) {
  delete j;
  return PDX_OK;
}
