// stream_io.hpp -- the one place that says how a once-through HBM stream is accessed.
//
// ld_stream<S>(p) / st_stream<S>(p, v) compile to __builtin_nontemporal_load / _store (global_load / global_store ... nt on gfx950)
// or to a plain access, chosen per stream S by the bits of PDX_STREAM_NT below.  A stream is data that a kernel touches exactly once:
// keeping it out of the way of the lines that ARE reused (partly filled output lines of a scatter waiting in L2 for the neighbouring
// tile, first[] and the pass-0 offsets) is the only thing the policy can buy, so every stream is decided alone, by measurement on the
// headline step ("Stream access policy"); a stream whose nt form did not win keeps the plain access and a 0 bit.
// There is no runtime switch: variants are compared by building the library with another -DPDX_STREAM_NT=<mask>.
// The builtins take scalars and ext_vector_type vectors (not HIP's uint4 struct): hence the vector typedefs here.
#pragma once
#include <stdint.h>

namespace pdx {

enum StreamId : unsigned {
  kStreamScatVals = 0,    // a: payload loads of radix_scatter_body
  kStreamScatKeys = 1,    // b: its key loads
  kStreamDenseKeys = 2,   // c: key loads of k_dense_slots / k_dense_slots_tail_hist_lds
  kStreamDenseSlots = 3,  // d: their slot_of_row stores
  kStreamHistKeys = 4,    // e: loads of k_radix_hist
  kStreamFlrTile = 5,     // f: key and value loads of k_flr_reduce's load_tile
  kStreamScatOut = 6,     // g: the scatter's output stores
  kStreamJoinOut = 7,     // h: the two index columns k_join_expand writes
};
#ifndef PDX_STREAM_NT
//                      hgfedcba
#define PDX_STREAM_NT 0b10011001
#endif
constexpr unsigned kStreamNtMask = PDX_STREAM_NT;
constexpr bool stream_nt(StreamId s) { return (kStreamNtMask >> (unsigned)s) & 1u; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <StreamId S, typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
  if constexpr (stream_nt(S)) return __builtin_nontemporal_load(p);
  else return *p;
}
template <StreamId S, typename T, typename U>
__device__ __forceinline__ void st_stream(T* p, U v) {
  if constexpr (stream_nt(S)) __builtin_nontemporal_store((T)v, p);
  else *p = (T)v;
}

}  // namespace pdx
