// colview.hpp -- the layer between the C ABI and the per-row kernels (row_aggregate.hip, multiplex.hip, cumulative.hip, ...): a device
// table of columns, 64-bit windows of Arrow bitmaps and tail-preserving stores of bit-packed outputs, the null counter of an output and
// its read-back, and the checks of a caller's output buffer.  One home for all of them: a fix here reaches every caller.
#pragma once
#include <string.h>
#include <string>
#include <vector>
#include "pdx_common.hpp"

namespace pdx {

// ---------------------------------------------------------------- device side
// one column of a device table: every wave reads its entry with uniform loads
struct ColView {
  const void* values;    // element offset applied (PDX_BOOL: the bitmap's base)
  const uint8_t* valid;  // nullptr: every row is valid
  int64_t voff;          // bit offset into valid
  int64_t boff;          // PDX_BOOL: bit offset into values
};

// Which bitmap window: load_bits64_uniform when bits / bitpos are the same for the whole wave (a wave owns the word: two scalar loads);
// load_bits64 (pdx_common.hpp) when every lane has a word of its own -- byte loads, clamped at limit_bits, any address.
//
// 64 bits starting at bit `bitpos` of `bits`, of which the caller uses the first `nbits` (>= 1): two aligned 64-bit words and a funnel
// shift.  Every word read holds at least one byte of the `nbits` asked for, so no read leaves the pages of the bitmap.  All operands
// are wave-uniform: the loads are scalar.
__device__ __forceinline__ uint64_t load_bits64_uniform(const uint8_t* bits, int64_t bitpos, int nbits) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(bits) + (uintptr_t)(bitpos >> 3);
  // (the inputs are never written while the kernel runs: the constant address space is what lets a uniform address become a scalar load)
  const __attribute__((address_space(4))) uint64_t* p = (const __attribute__((address_space(4))) uint64_t*)(a & ~(uintptr_t)7);
  const int sh = (int)(a & 7) * 8 + (int)(bitpos & 7);
  uint64_t r = p[0] >> sh;
  if (sh + nbits > 64) r |= p[1] << (64 - sh);
  return r;
}
// word w of a bit-packed output, a wave's store: lanes 0..7 write a byte each; the byte that holds row n keeps its bits from n on
__device__ __forceinline__ void store_bits_wave(uint8_t* dst, int64_t w, int64_t n, uint64_t word, int lane) {
  if (lane >= 8) return;
  const int64_t r0 = (w << 6) + lane * 8;
  if (r0 >= n) return;
  uint8_t b = (uint8_t)(word >> (8 * lane));
  const int64_t rem = n - r0;
  if (rem < 8) {
    const uint8_t m = (uint8_t)((1u << rem) - 1u);
    b = (uint8_t)((dst[(w << 3) + lane] & ~m) | (b & m));
  }
  dst[(w << 3) + lane] = b;
}
// the same for a thread that owns the word
__device__ __forceinline__ void store_bits_word(uint8_t* dst, int64_t w, int64_t n, uint64_t word) {
  const int64_t rem = n - (w << 6);
  if (rem >= 64) {
    reinterpret_cast<uint64_t*>(dst)[w] = word;
    return;
  }
  const int nbytes = (int)((rem + 7) >> 3);
  for (int q = 0; q < nbytes; ++q) {
    uint8_t b = (uint8_t)(word >> (8 * q));
    if (q == nbytes - 1 && (rem & 7)) {
      const uint8_t m = (uint8_t)((1u << (rem & 7)) - 1u);
      b = (uint8_t)((dst[(w << 3) + q] & ~m) | (b & m));
    }
    dst[(w << 3) + q] = b;
  }
}
// the wave's first 64-row word (its index in the grid), as a value the compiler knows to be wave-uniform
__device__ __forceinline__ int first_word_of_wave() { return __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)); }
// the first min(rem, 64) bits set (none for rem <= 0)
__device__ __forceinline__ uint64_t in_range_mask(int64_t rem) { return rem >= 64 ? ~0ull : rem > 0 ? (1ull << rem) - 1ull : 0ull; }
// a wave's null rows into the output's counter: the lanes' counts summed, one atomic from lane 0.  Whether there is a counter at all
// (nulls != nullptr, an output bitmap) is the caller's question.
__device__ __forceinline__ void wave_add_nulls(unsigned long long* nulls, int lane, unsigned long long nc) {
  for (int d = 32; d > 0; d >>= 1) nc += __shfl_down(nc, d, 64);
  if (lane == 0 && nc) atomicAdd(nulls, nc);
}

// ---------------------------------------------------------------- host side
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline ColView col_view(const pdx_column& a) {
  ColView e;
  e.values = a.dtype == PDX_BOOL ? a.values : static_cast<const void*>(static_cast<const char*>(a.values) + (size_t)a.offset * (size_t)dtype_bytes(a.dtype));
  e.valid = validity_or_null(&a);
  e.voff = a.offset;
  e.boff = a.offset;
  return e;
}
// the table on the device (scratch of the call)
inline int upload_views(Scratch& s, const std::vector<ColView>& host, hipStream_t st, const ColView** tab) {
  ColView* t = s.get<ColView>(host.size());
  PDX_SCRATCH_CHECK(s);
  if (!host.empty()) PDX_HIP(hipMemcpyAsync(t, host.data(), sizeof(ColView) * host.size(), hipMemcpyHostToDevice, st));
  *tab = t;
  return PDX_OK;
}
// the device word that counts the null rows of the output, zeroed; asked for only when the count has to come from the kernel
inline int open_null_counter(Scratch& s, hipStream_t st, unsigned long long** nulls) {
  *nulls = s.get<unsigned long long>(1);
  PDX_SCRATCH_CHECK(s);
  PDX_HIP(hipMemsetAsync(*nulls, 0, sizeof(**nulls), st));
  return PDX_OK;
}
// device-to-host read that the caller waits for; a small one (<= 64 bytes) goes through this thread's pinned slot: a copy into pageable
// memory is staged by the runtime
inline int read_back(void* dst, const void* dev, size_t bytes, hipStream_t st) {
  void* pin = bytes <= 64 ? pinned_slot() : nullptr;
  PDX_HIP(hipMemcpyAsync(pin ? pin : dst, dev, bytes, hipMemcpyDeviceToHost, st));
  PDX_HIP(hipStreamSynchronize(st));
  if (pin) memcpy(dst, pin, bytes);
  return PDX_OK;
}
// the caller's output column against the result: dtype want, n rows
inline int check_out(const char* who, const pdx_mut_column* out, int want, int64_t n) {
  if (!out) return fail(PDX_INVALID, std::string(who) + ": null output");
  if (out->dtype != want) return fail(PDX_INVALID, std::string(who) + ": output dtype " + dtype_name(out->dtype) + ", the result is " + dtype_name(want));
  if (out->length < n) return fail(PDX_INVALID, std::string(who) + ": output too small");
  if (n > 0 && !out->values) return fail(PDX_INVALID, std::string(who) + ": null output buffer");
  return PDX_OK;
}

}  // namespace pdx
