// elementwise.hip -- element-wise arithmetic, comparison and logical kernels for gfx950.
//
// Replaces the Arrow kernels reached from Series::operator{+,-,*,/,<,<=,...,&&,||,!}
// (reference src/series.cpp:19-33,229-261,319; src/scalar.cpp:24-36) and the DataFrame
// forms (src/dataframe.cpp:233-275).  All kernels are HBM-bound streams:
//   binary  : 2 x w B read + w B write per row  (w = 4 or 8; + 3/8 B with validity)
//   compare : 2 x w B read + 1/8 B write per row
// One kernel family, templated on the operand and result types, serves int64, float64, int32 and float32 (and uint64 for the unary
// ops).  When every array operand and the output start on a 16-byte boundary k_binary_n moves four consecutive rows per lane and
// access (one dwordx4 per 4-byte stream, two per 8-byte stream), and so do k_compare_n and k_unary_n for a pair with a 4-byte side.
// Otherwise a lane takes a row at a time: four independent rows in flight for a misaligned 8-byte k_binary_n pair, eight in an 8-byte
// k_compare_n.  Bit-packed outputs are assembled with wave-wide ballots so every wave stores whole 64-bit words, 64 words (512 B) at a
// time.
#include <limits>
#include <type_traits>
#include "colview.hpp"

namespace pdx {

// ---------------------------------------------------------------- validity: out = va & vb (bit offsets honoured)
// one thread per output 64-bit word
__global__ void k_validity_and(const uint8_t* __restrict__ va, int64_t aoff, int64_t alimit, const uint8_t* __restrict__ vb,
                               int64_t boff, int64_t blimit, int b_broadcast, int64_t n, uint8_t* __restrict__ out) {
  int64_t nwords = (n + 63) >> 6;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool b_all = true;
  if (vb && b_broadcast) b_all = bit_get(vb, boff);
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    int64_t base = w << 6;
    uint64_t x = va ? load_bits64(va, aoff + base, alimit) : ~0ull;
    uint64_t y = ~0ull;
    if (vb) y = b_broadcast ? (b_all ? ~0ull : 0ull) : load_bits64(vb, boff + base, blimit);
    uint64_t r = x & y;
    int64_t remain = n - base;
    if (remain >= 64) {
      reinterpret_cast<uint64_t*>(out)[w] = r;
    } else {
      r &= (1ull << remain) - 1ull;
      int nbytes = (int)((remain + 7) >> 3);
      for (int k = 0; k < nbytes; ++k) out[(w << 3) + k] = (uint8_t)(r >> (8 * k));
    }
  }
}

int launch_validity_and(const pdx_column* a, const pdx_column* b, int b_is_scalar, int64_t n, uint8_t* out, hipStream_t st) {
  const uint8_t* va = validity_or_null(a);
  const uint8_t* vb = b ? validity_or_null(b) : nullptr;
  if (n == 0) return PDX_OK;
  int64_t nwords = (n + 63) >> 6;
  hipLaunchKernelGGL(k_validity_and, dim3(grid_for(nwords, 256)), dim3(256), 0, st, va, a->offset, a->offset + a->length, vb,
                     b ? b->offset : 0, b ? b->offset + b->length : 0, b_is_scalar, n, out);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// ---------------------------------------------------------------- the numeric types
// Arrow's implicit promotion of a mixed pair: any float64 operand -> float64; else any float32 operand -> float32; else the wider integer
template <typename A, typename B>
struct Promote {
  using type = typename std::conditional<
      __is_same(A, double) || __is_same(B, double), double,
      typename std::conditional<__is_same(A, float) || __is_same(B, float), float,
                                typename std::conditional<(sizeof(A) == 8 || sizeof(B) == 8), int64_t, int32_t>::type>::type>::type;
};
template <typename T>
constexpr int dt_of() {
  return __is_same(T, double) ? PDX_FLOAT64 : __is_same(T, float) ? PDX_FLOAT32 : __is_same(T, int64_t) ? PDX_INT64 : PDX_INT32;
}
template <typename T>
constexpr bool is_float_t() { return __is_same(T, double) || __is_same(T, float); }

// Arrow's safe cast of an integer TI to a float TO (the implicit promotion of a mixed pair, the integer sqrt / exp / power, pdx_cast) is
// CHECKED when TO cannot hold every TI: a VALID value outside +-2^digits(TO) -- 0 ... 2^53 for uint64 -- fails the whole call with
// "Integer value V not in range: LO to HI" (pinned against Arrow C++ 25 by tests/cpp/arrow_bridge_test.cpp; null slots are not looked at,
// the bounds themselves pass).  int64 -> float64: +-2^53; int32 / int64 -> float32: +-2^24; int32 -> float64 is exact.  The kernels test
// every row they read and keep the first offending one (note_bad_row); the message names the value there, as Arrow's does.
template <typename TI, typename TO>
constexpr bool checked_cast() { return is_float_t<TO>() && !is_float_t<TI>() && (int)sizeof(TI) * 8 > std::numeric_limits<TO>::digits; }
template <typename TI, typename TO>
__device__ __forceinline__ bool outside_exact(TI x) {
  constexpr TI lim = TI(1) << std::numeric_limits<TO>::digits;
  if constexpr (std::is_unsigned<TI>::value) return x > lim;
  else return x > lim || x < -lim;
}
// error words of a call: [0] divide by zero (1), [1] ~(first row of the checked operand outside its exact range), 0 = none
__device__ __forceinline__ void note_bad_row(unsigned long long* err, int64_t row) { atomicMax(&err[1], ~(unsigned long long)row); }

template <typename T>
using bits_t = typename std::conditional<sizeof(T) == 8, unsigned long long, unsigned>::type;
template <typename T>
constexpr bits_t<T> kQuietBit = bits_t<T>(1) << (std::numeric_limits<T>::digits - 2);
template <typename T>
__device__ __forceinline__ T quieted(T x) { return __builtin_bit_cast(T, __builtin_bit_cast(bits_t<T>, x) | kQuietBit<T>); }

// NaN results carry the bits the reference's x86 host would produce, not CDNA's: SSE hands back the FIRST NaN operand (quieted;
// the second one if only that is NaN -- not negated by a subtraction), and an invalid operation (inf - inf, 0 * inf, 0 / 0,
// inf / inf) yields the negative "real indefinite" (sign, exponent and quiet bit set: 0xFFF8000000000000 / 0xFFC00000), where
// v_add/v_mul/v_div give +qNaN or flip the sign of a negated source.  Three selects on values already in registers: free in an
// HBM-bound kernel.
template <typename T>
__device__ __forceinline__ T x86_nan(T r, T x, T y) {
  if (r == r) return r;
  if (x != x) return quieted(x);
  if (y != y) return quieted(y);
  return __builtin_bit_cast(T, (bits_t<T>)~(kQuietBit<T> - 1));
}

template <typename TO, int OP>
__device__ __forceinline__ TO apply_op(TO x, TO y, bool valid, unsigned long long* err) {
  if constexpr (is_float_t<TO>()) {  // (the bit-wise ops are integer-only: the host never instantiates them for floats)
    if constexpr (OP == PDX_ADD) return x86_nan(x + y, x, y);
    else if constexpr (OP == PDX_SUB) return x86_nan(x - y, x, y);
    else if constexpr (OP == PDX_MUL) return x86_nan(x * y, x, y);
    else return x86_nan(x / y, x, y);
  } else {  // integers wrap at their own width
    using U = typename std::make_unsigned<TO>::type;
    const U ux = (U)x, uy = (U)y;
    if constexpr (OP == PDX_ADD) return (TO)(ux + uy);
    else if constexpr (OP == PDX_SUB) return (TO)(ux - uy);
    else if constexpr (OP == PDX_MUL) return (TO)(ux * uy);
    else if constexpr (OP == PDX_BIT_OR) return (TO)(ux | uy);
    else if constexpr (OP == PDX_BIT_AND) return (TO)(ux & uy);
    else if constexpr (OP == PDX_BIT_XOR) return (TO)(ux ^ uy);
    else if constexpr (OP == PDX_SHIFT_LEFT || OP == PDX_SHIFT_RIGHT) {
      // Arrow's unchecked shifts: an amount outside [0, digits) -- 63 for int64, 31 for int32 -- returns the left operand
      if (y < 0 || y >= std::numeric_limits<TO>::digits) return x;
      if constexpr (OP == PDX_SHIFT_LEFT) return (TO)(ux << y);
      else return x >> y;
    } else {
      // Arrow "divide" (unchecked): truncation toward zero; MIN / -1 -> 0; zero divisor at a valid slot is an error
      if (!valid) return 0;
      if (y == 0) {
        *err = 1ull;
        return 0;
      }
      if (x == std::numeric_limits<TO>::min() && y == -1) return 0;
      return x / y;
    }
  }
}

template <typename T>
struct alignas(16) V4 {
  T v[4];
};

// ---------------------------------------------------------------- binary arithmetic
// SCALAR: 0 = two arrays, 1 = b is one broadcast value (Series op Scalar, src/series.cpp:25-28), 2 = a is one broadcast value
// (Scalar op Series, src/scalar.cpp:24-36: CallFunction(name, {scalar, array}) -- the scalar stays the LEFT operand, which
// matters for subtract / divide and for which NaN payload survives).  vec: every array operand and out start on 16 bytes.
template <typename TA, typename TB, typename TO, int OP, int SCALAR>
__global__ void __launch_bounds__(256) k_binary_n(const TA* __restrict__ a, const TB* __restrict__ b, TO* __restrict__ out, int64_t n, int vec,
                                                  const uint8_t* __restrict__ va, int64_t aoff, const uint8_t* __restrict__ vb, int64_t boff,
                                                  unsigned long long* __restrict__ err) {
  constexpr bool kCheckA = checked_cast<TA, TO>(), kCheckB = checked_cast<TB, TO>();
  constexpr bool kNeedValid = ((OP == PDX_DIV) && !is_float_t<TO>()) || kCheckA || kCheckB;
  constexpr bool SA = SCALAR == 2, SB = SCALAR == 1;
  // Arrow's scalar-array loops for the commutative ops keep the ARRAY element as the first machine operand (measured against
  // Arrow 25.0.0: NaN(scalar) + NaN(array) returns the array's payload in both orders), so add / multiply swap operands
  constexpr bool kSwap = SA && (OP == PDX_ADD || OP == PDX_MUL);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  TO xs = 0, ys = 0;
  bool xs_valid = true, ys_valid = true;
  if constexpr (SB) {
    ys = (TO)b[0];
    if (kNeedValid && vb) ys_valid = bit_get(vb, boff);
    if constexpr (kCheckB)
      if (tid == 0 && ys_valid && outside_exact<TB, TO>(b[0])) note_bad_row(err, 0);
  }
  if constexpr (SA) {
    xs = (TO)a[0];
    if (kNeedValid && va) xs_valid = bit_get(va, aoff);
    if constexpr (kCheckA)
      if (tid == 0 && xs_valid && outside_exact<TA, TO>(a[0])) note_bad_row(err, 0);
  }
  unsigned long long div_err = 0;
  int64_t bad = INT64_MAX;  // first row of the checked operand outside its exact range this lane saw
  auto one = [&](TA ra, TB rb, int64_t i) -> TO {
    bool av = SA ? xs_valid : (!kNeedValid || !va || bit_get(va, aoff + i));
    bool bv = SB ? ys_valid : (!kNeedValid || !vb || bit_get(vb, boff + i));
    if constexpr (kCheckA && !SA)
      if (av && outside_exact<TA, TO>(ra) && i < bad) bad = i;
    if constexpr (kCheckB && !SB)
      if (bv && outside_exact<TB, TO>(rb) && i < bad) bad = i;
    const TO x = SA ? xs : (TO)ra, y = SB ? ys : (TO)rb;
    return kSwap ? apply_op<TO, OP>(y, x, av && bv, &div_err) : apply_op<TO, OP>(x, y, av && bv, &div_err);
  };
  const int64_t n4 = vec ? (n >> 2) : 0;
  for (int64_t g = tid; g < n4; g += stride) {
    const int64_t i = g << 2;
    V4<TA> xa;
    V4<TB> yb;
    if constexpr (!SA) xa = *reinterpret_cast<const V4<TA>*>(a + i);
    if constexpr (!SB) yb = *reinterpret_cast<const V4<TB>*>(b + i);
    V4<TO> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = one(SA ? TA(0) : xa.v[k], SB ? TB(0) : yb.v[k], i + k);
    *reinterpret_cast<V4<TO>*>(out + i) = r;
  }
  // misaligned (or the < 4 rows after the vector loop): a row per lane; 8-byte pairs keep four independent rows in flight (a pair
  // with a 4-byte side does not need them, and they would cost it registers)
  int64_t i = (n4 << 2) + tid;
  if constexpr (sizeof(TA) == 8 && sizeof(TB) == 8) {
    for (; i + 3 * stride < n; i += 4 * stride) {
      TA xa[4];
      TB yb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xa[k] = SA ? TA(0) : a[i + k * stride];
        yb[k] = SB ? TB(0) : b[i + k * stride];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) out[i + k * stride] = one(xa[k], yb[k], i + k * stride);
    }
  }
  for (; i < n; i += stride) out[i] = one(SA ? TA(0) : a[i], SB ? TB(0) : b[i], i);
  if constexpr ((OP == PDX_DIV) && !is_float_t<TO>())
    if (div_err) atomicMax(&err[0], div_err);
  if constexpr (kCheckA || kCheckB)
    if (bad != INT64_MAX) note_bad_row(err, bad);
}

// ---------------------------------------------------------------- comparisons -> bit-packed bools
template <typename T, int OP>
__device__ __forceinline__ bool cmp_op(T x, T y) {
  if constexpr (OP == PDX_EQ) return x == y;
  else if constexpr (OP == PDX_NE) return x != y;
  else if constexpr (OP == PDX_LT) return x < y;
  else if constexpr (OP == PDX_LE) return x <= y;
  else if constexpr (OP == PDX_GT) return x > y;
  else return x >= y;
}

// Each wave owns tiles of 4096 rows.  vec: a lane reads 4 consecutive rows per step (16-byte accesses per 4-byte stream); the four
// ballots of a step hold rows 4 l + j at bit l of ballot j, and are interleaved back into the step's four 64-row words.  Otherwise
// (misaligned, or the ragged last tile): 64 ballots of a row per lane, lane k keeps word k.  Either way one 512-byte store per tile.
__device__ __forceinline__ uint64_t spread4(uint64_t v) {  // bit m of the low 16 bits -> bit 4 m
  uint64_t x = v & 0xFFFFull;
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}
template <typename TA, typename TB, typename TC, int OP, bool SCALAR_B>
__global__ void __launch_bounds__(256) k_compare_n(const TA* __restrict__ a, const TB* __restrict__ b, uint8_t* __restrict__ out, int64_t n, int vec,
                                                   const uint8_t* __restrict__ va, int64_t aoff, const uint8_t* __restrict__ vb, int64_t boff,
                                                   unsigned long long* __restrict__ err) {
  constexpr bool kCheckA = checked_cast<TA, TC>(), kCheckB = checked_cast<TB, TC>();
  // a pair with a 4-byte side reads four rows per lane and access when aligned; 8-byte pairs keep a row per lane and eight rows in
  // flight, which is as fast and stays within 64 VGPRs (8 waves/SIMD)
  constexpr bool kNarrow = sizeof(TA) == 4 || sizeof(TB) == 4;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t ntiles = (n + 4095) >> 12;
  TC ys = 0;
  if constexpr (SCALAR_B) {
    ys = (TC)b[0];
    if constexpr (kCheckB)
      if (wave == 0 && lane == 0 && (!vb || bit_get(vb, boff)) && outside_exact<TB, TC>(b[0])) note_bad_row(err, 0);
  }
  int64_t bad = INT64_MAX;
  auto pred = [&](TA ra, TB rb, int64_t i) -> bool {
    if constexpr (kCheckA)
      if (outside_exact<TA, TC>(ra) && i < bad && (!va || bit_get(va, aoff + i))) bad = i;
    if constexpr (kCheckB && !SCALAR_B)
      if (outside_exact<TB, TC>(rb) && i < bad && (!vb || bit_get(vb, boff + i))) bad = i;
    return cmp_op<TC, OP>((TC)ra, SCALAR_B ? ys : (TC)rb);
  };
  for (int64_t t = wave; t < ntiles; t += nwaves) {
    const int64_t base = t << 12;
    uint64_t myword = 0;
    if (kNarrow && vec && base + 4096 <= n) {
#pragma unroll 4
      for (int s = 0; s < 16; ++s) {
        const int64_t i = base + (s << 8) + (lane << 2);
        const V4<TA> xa = *reinterpret_cast<const V4<TA>*>(a + i);
        V4<TB> yb;
        if constexpr (!SCALAR_B) yb = *reinterpret_cast<const V4<TB>*>(b + i);
        uint64_t bal[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bal[j] = __ballot(pred(xa.v[j], SCALAR_B ? TB(0) : yb.v[j], i + j));
        if ((lane >> 2) == s) {
          const int q = lane & 3;
          myword = spread4(bal[0] >> (16 * q)) | (spread4(bal[1] >> (16 * q)) << 1) | (spread4(bal[2] >> (16 * q)) << 2) |
                   (spread4(bal[3] >> (16 * q)) << 3);
        }
      }
    } else if (!kNarrow && base + 4096 <= n) {
#pragma unroll 8
      for (int k = 0; k < 64; ++k) {
        const int64_t i = base + (k << 6) + lane;
        const uint64_t bal = __ballot(pred(a[i], SCALAR_B ? TB(0) : b[i], i));
        if (lane == k) myword = bal;
      }
    } else {  // a misaligned 4-byte pair, or the ragged last tile
      for (int k = 0; k < 64; ++k) {
        const int64_t i = base + (k << 6) + lane;
        const uint64_t bal = __ballot(i < n && pred(a[i], SCALAR_B ? TB(0) : b[i], i));
        if (lane == k) myword = bal;
      }
    }
    const int64_t wbase = (base >> 6) + lane;
    const int64_t first_row = wbase << 6;
    if (first_row < n) {
      const int64_t remain = n - first_row;
      if (remain >= 64) reinterpret_cast<uint64_t*>(out)[wbase] = myword;
      else
        for (int q = 0; q < (int)((remain + 7) >> 3); ++q) out[(wbase << 3) + q] = (uint8_t)(myword >> (8 * q));
    }
  }
  if constexpr (kCheckA || kCheckB)
    if (bad != INT64_MAX) note_bad_row(err, bad);
}

// ---------------------------------------------------------------- logical on bit-packed bools
// mode 0: and, 1: or, 2: invert(a)
__global__ void k_logical(const uint8_t* __restrict__ a, int64_t aoff, int64_t alimit, const uint8_t* __restrict__ b, int64_t boff,
                          int64_t blimit, int mode, int64_t n, uint8_t* __restrict__ out) {
  int64_t nwords = (n + 63) >> 6;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    int64_t base = w << 6;
    uint64_t x = load_bits64(a, aoff + base, alimit);
    uint64_t r;
    if (mode == 2) r = ~x;
    else {
      uint64_t y = load_bits64(b, boff + base, blimit);
      r = mode == 0 ? (x & y) : (x | y);
    }
    int64_t remain = n - base;
    if (remain >= 64) {
      reinterpret_cast<uint64_t*>(out)[w] = r;
    } else {
      r &= (1ull << remain) - 1ull;
      int nbytes = (int)((remain + 7) >> 3);
      for (int k = 0; k < nbytes; ++k) out[(w << 3) + k] = (uint8_t)(r >> (8 * k));
    }
  }
}

// ---------------------------------------------------------------- if_else(cond, a, b)
// SCALAR as in k_binary_n.  Values: one grid-stride stream (cond bit -> a or b).  Validity: one thread per 64-row output word from the
// words of cond, its validity and the operands' validity: valid = cond_valid & (cond ? a_valid : b_valid).  Arrow casts both operands
// whole before it selects, so every valid row of a checked operand is looked at, chosen or not.
template <typename TA, typename TB, typename TO, int SCALAR>
__global__ void __launch_bounds__(256) k_if_else_n(const uint8_t* __restrict__ cond, int64_t coff, const TA* __restrict__ a,
                                                   const uint8_t* __restrict__ va, int64_t aoff, int64_t alen, const TB* __restrict__ b,
                                                   const uint8_t* __restrict__ vb, int64_t boff, int64_t blen, TO* __restrict__ out, int64_t n,
                                                   const uint8_t* __restrict__ cvalid, uint8_t* __restrict__ out_valid, unsigned long long* __restrict__ err) {
  constexpr bool SA = SCALAR == 2, SB = SCALAR == 1;
  constexpr bool kCheckA = checked_cast<TA, TO>(), kCheckB = checked_cast<TB, TO>();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const TO as = SA ? (TO)a[0] : TO(0), bs = SB ? (TO)b[0] : TO(0);
  const bool as_valid = !SA || !va || bit_get(va, aoff), bs_valid = !SB || !vb || bit_get(vb, boff);
  int64_t bad = INT64_MAX;
  if constexpr (kCheckA && SA)
    if (tid == 0 && as_valid && outside_exact<TA, TO>(a[0])) bad = 0;
  if constexpr (kCheckB && SB)
    if (tid == 0 && bs_valid && outside_exact<TB, TO>(b[0])) bad = 0;
  for (int64_t i = tid; i < n; i += stride) {
    const bool c = bit_get(cond, coff + i);
    if constexpr (kCheckA && !SA)
      if (outside_exact<TA, TO>(a[i]) && i < bad && (!va || bit_get(va, aoff + i))) bad = i;
    if constexpr (kCheckB && !SB)
      if (outside_exact<TB, TO>(b[i]) && i < bad && (!vb || bit_get(vb, boff + i))) bad = i;
    out[i] = c ? (SA ? as : (TO)a[i]) : (SB ? bs : (TO)b[i]);
  }
  if constexpr (kCheckA || kCheckB)
    if (bad != INT64_MAX) note_bad_row(err, bad);
  if (!out_valid) return;
  const int64_t climit = coff + n, alimit = aoff + alen, blimit = boff + blen;
  for (int64_t w = tid; w < ((n + 63) >> 6); w += stride) {
    const int64_t base = w << 6;
    const uint64_t c = load_bits64(cond, coff + base, climit);
    const uint64_t cv = cvalid ? load_bits64(cvalid, coff + base, climit) : ~0ull;
    const uint64_t av = SA ? (as_valid ? ~0ull : 0ull) : (va ? load_bits64(va, aoff + base, alimit) : ~0ull);
    const uint64_t bv = SB ? (bs_valid ? ~0ull : 0ull) : (vb ? load_bits64(vb, boff + base, blimit) : ~0ull);
    uint64_t r = cv & ((c & av) | (~c & bv));
    const int64_t remain = n - base;
    if (remain >= 64) {
      reinterpret_cast<uint64_t*>(out_valid)[w] = r;
    } else {
      r &= (1ull << remain) - 1ull;
      for (int k = 0; k < (int)((remain + 7) >> 3); ++k) out_valid[(w << 3) + k] = (uint8_t)(r >> (8 * k));
    }
  }
}

// ---------------------------------------------------------------- functions of one column (pdx_unary, pdx_power, the casts)
// negate / abs of a float touch the sign bit only, as Arrow's do: a signalling NaN stays signalling.  The bits go through an opaque
// register so that they stay integer instructions: written as -x, hipcc selects v_pk_add_f32 (-x) + (-0) for two negations of the
// row-per-lane loop, a floating-point add, which quiets the NaN (found by tests/test_gpu_elementwise.py, unary negate f32 in the row form).
template <typename T>
__device__ __forceinline__ T sign_bit(T x, bool clear) {
  constexpr bits_t<T> kSign = bits_t<T>(1) << (sizeof(T) * 8 - 1);
  bits_t<T> b = __builtin_bit_cast(bits_t<T>, x);
  b = clear ? (b & ~kSign) : (b ^ kSign);
  asm volatile("" : "+v"(b));
  return __builtin_bit_cast(T, b);
}

constexpr int kPowerOp = 100;  // internal op codes: pdx_power, Arrow's (safe) cast, and the unchecked cast of pdx_cast_f64(checked = 0)
constexpr int kCastOp = 101;
constexpr int kPlainCastOp = 102;
template <int OP, typename TI, typename TO>
__device__ __forceinline__ TO unary_one(TI x, int64_t i, double expo, const uint8_t* valid, int64_t voff, int64_t* bad) {
  using U = typename std::make_unsigned<typename std::conditional<is_float_t<TI>(), int, TI>::type>::type;
  if constexpr (OP == PDX_NEGATE) {
    if constexpr (is_float_t<TI>()) return sign_bit(x, false);
    else return (TO)(U(0) - (U)x);  // wraps at TI's width
  } else if constexpr (OP == PDX_ABS) {
    if constexpr (is_float_t<TI>()) return sign_bit(x, true);
    else if constexpr (std::is_unsigned<TI>::value) return x;
    else return x < 0 ? (TO)(U(0) - (U)x) : x;
  } else if constexpr (OP == PDX_SIGN) {
    if constexpr (is_float_t<TI>()) return x != x ? x : (x > TI(0) ? TI(1) : (x < TI(0) ? TI(-1) : TI(0)));
    else if constexpr (std::is_unsigned<TI>::value) return x != 0;
    else return (TO)((x > 0) - (x < 0));
  } else if constexpr (OP == PDX_BIT_NOT) {
    return (TO)~(U)x;
  } else {  // sqrt / exp / power / cast: Arrow's cast to TO first (checked where it is not exact, unless the call is an unchecked cast)
    if constexpr (checked_cast<TI, TO>() && OP != kPlainCastOp)
      if (outside_exact<TI, TO>(x) && i < *bad && (!valid || bit_get(valid, voff + i))) *bad = i;
    const TO d = (TO)x;
    if constexpr (OP == PDX_SQRT) {
      // Arrow: a negative operand gives the positive quiet NaN; a NaN operand comes back quieted with its payload (x86 sqrtsd / sqrtss)
      if (d < TO(0)) return std::numeric_limits<TO>::quiet_NaN();
      if (d != d) return quieted(d);
      if constexpr (__is_same(TO, float)) return __builtin_sqrtf(d);
      else return __builtin_sqrt(d);
    } else if constexpr (OP == PDX_EXP) {
      if constexpr (__is_same(TO, float)) return expf(d);
      else return exp(d);
    } else if constexpr (OP == kPowerOp) {
      return pow(d, expo);
    } else {
      return d;
    }
  }
}
// vec (16-byte aligned): four rows per lane and access, as k_binary_n, when a stream is 4-byte; else a row per lane (with 8-byte
// streams alone that measured faster, aligned or not)
template <int OP, typename TI, typename TO>
__global__ void __launch_bounds__(256) k_unary_n(const TI* __restrict__ a, TO* __restrict__ out, int64_t n, int vec, double expo,
                                                 const uint8_t* __restrict__ valid, int64_t voff, unsigned long long* __restrict__ err) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  constexpr bool kNarrow = sizeof(TI) == 4 || sizeof(TO) == 4;
  int64_t bad = INT64_MAX;
  const int64_t n4 = kNarrow && vec ? (n >> 2) : 0;
  for (int64_t g = tid; g < n4; g += stride) {
    const int64_t i = g << 2;
    const V4<TI> x = *reinterpret_cast<const V4<TI>*>(a + i);
    V4<TO> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = unary_one<OP, TI, TO>(x.v[k], i + k, expo, valid, voff, &bad);
    *reinterpret_cast<V4<TO>*>(out + i) = r;
  }
  for (int64_t i = (n4 << 2) + tid; i < n; i += stride) out[i] = unary_one<OP, TI, TO>(a[i], i, expo, valid, voff, &bad);
  if (bad != INT64_MAX) note_bad_row(err, bad);
}

// ---------------------------------------------------------------- host side
static int check_numeric_pair(const pdx_column* a, const pdx_column* b, int scalar_side, const char* what) {
  PDX_TRY(check_column(a, what, true));
  PDX_TRY(check_column(b, what, true));
  auto ok = [](int dt) { return dt == PDX_INT64 || dt == PDX_FLOAT64 || is_narrow(dt); };
  if (!ok(a->dtype) || !ok(b->dtype)) return fail(PDX_NOT_IMPLEMENTED, std::string(what) + ": only int64/float64/int32/float32 operands are supported");
  if (scalar_side < 0 || scalar_side > PDX_SCALAR_LHS) return fail(PDX_INVALID, std::string(what) + ": scalar side must be 0 (none), 1 (rhs) or 2 (lhs)");
  if (scalar_side) {
    if ((scalar_side == PDX_SCALAR_LHS ? a : b)->length != 1) return fail(PDX_INVALID, std::string(what) + ": scalar operand must have length 1");
  } else if (a->length != b->length) {
    return fail(PDX_INVALID, std::string(what) + ": array lengths differ: " + std::to_string(a->length) + " vs " + std::to_string(b->length));
  }
  return PDX_OK;
}

template <typename F>
static int with_num_type(int dt, F&& f) {
  switch (dt) {
    case PDX_INT32: return f(int32_t{});
    case PDX_FLOAT32: return f(float{});
    case PDX_INT64: return f(int64_t{});
    default: return f(double{});
  }
}
static int result_dt(int da, int db) {
  return with_num_type(da, [&](auto ta) { return with_num_type(db, [&](auto tb) { return dt_of<typename Promote<decltype(ta), decltype(tb)>::type>(); }); });
}

// The error words of one call.  Only a call whose kernel can fail -- an integer divide, or an operand that goes through a checked cast --
// opens them: a scratch allocation, and one synchronising read-back in status().  Every other call stays asynchronous.
struct CallErrors {
  Scratch scratch;
  unsigned long long* dev = nullptr;
  const pdx_column* checked = nullptr;  // the operand that went through the checked cast (a length-1 column if it is the scalar side)
  int to_dt = PDX_FLOAT64;              // ... and the float type it was cast to
  int open(hipStream_t st) {
    if (dev) return PDX_OK;
    dev = scratch.get<unsigned long long>(2);
    PDX_SCRATCH_CHECK(scratch);
    PDX_HIP(hipMemsetAsync(dev, 0, 2 * sizeof(unsigned long long), st));
    return PDX_OK;
  }
  // opens the words when the cast of operand c (TI) to TO is checked
  template <typename TI, typename TO>
  int check_cast(const pdx_column* c, hipStream_t st) {
    if constexpr (!checked_cast<TI, TO>()) return PDX_OK;
    checked = c;
    to_dt = dt_of<TO>();
    return open(st);
  }
  int status(hipStream_t st) const {
    if (!dev) return PDX_OK;
    unsigned long long h[2] = {0, 0};
    PDX_HIP(hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, st));
    PDX_HIP(hipStreamSynchronize(st));
    if (h[0]) return fail(PDX_INVALID, "divide by zero");
    if (!h[1] || !checked) return PDX_OK;
    const int64_t row = (int64_t)~h[1];
    const char* at = static_cast<const char*>(checked->values) + (size_t)(checked->offset + row) * dtype_bytes(checked->dtype);
    std::string v;
    if (checked->dtype == PDX_INT32) {
      int32_t x = 0;
      PDX_HIP(hipMemcpy(&x, at, 4, hipMemcpyDeviceToHost));
      v = std::to_string(x);
    } else if (checked->dtype == PDX_UINT64) {
      unsigned long long x = 0;
      PDX_HIP(hipMemcpy(&x, at, 8, hipMemcpyDeviceToHost));
      v = std::to_string(x);
    } else {
      long long x = 0;
      PDX_HIP(hipMemcpy(&x, at, 8, hipMemcpyDeviceToHost));
      v = std::to_string(x);
    }
    const long long lim = 1ll << (to_dt == PDX_FLOAT32 ? std::numeric_limits<float>::digits : std::numeric_limits<double>::digits);
    return fail(PDX_INVALID, "Integer value " + v + " not in range: " + (checked->dtype == PDX_UINT64 ? "0" : std::to_string(-lim)) + " to " +
                                 std::to_string(lim));
  }
};

template <typename TA, typename TB, typename TO, int OP>
static int launch_binary(const pdx_column* a, const pdx_column* b, int scalar, TO* out, CallErrors& e, hipStream_t st) {
  PDX_TRY((e.check_cast<TA, TO>(a, st)));
  PDX_TRY((e.check_cast<TB, TO>(b, st)));
  if constexpr (OP == PDX_DIV && !is_float_t<TO>()) PDX_TRY(e.open(st));
  const int64_t n = scalar == 2 ? b->length : a->length;
  const TA* pa = static_cast<const TA*>(a->values) + a->offset;
  const TB* pb = static_cast<const TB*>(b->values) + b->offset;
  const int vec = aligned16(out) && (scalar == 2 || aligned16(pa)) && (scalar == 1 || aligned16(pb));
  const dim3 grid(grid_for(n, 256, 4)), block(256);
#define BN_ARGS pa, pb, out, n, vec, validity_or_null(a), a->offset, validity_or_null(b), b->offset, e.dev
  if (scalar == 1) hipLaunchKernelGGL((k_binary_n<TA, TB, TO, OP, 1>), grid, block, 0, st, BN_ARGS);
  else if (scalar == 2) hipLaunchKernelGGL((k_binary_n<TA, TB, TO, OP, 2>), grid, block, 0, st, BN_ARGS);
  else hipLaunchKernelGGL((k_binary_n<TA, TB, TO, OP, 0>), grid, block, 0, st, BN_ARGS);
#undef BN_ARGS
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

template <typename TA, typename TB, typename TC, int OP>
static int launch_compare(const pdx_column* a, const pdx_column* b, int scalar, uint8_t* out, CallErrors& e, hipStream_t st) {
  PDX_TRY((e.check_cast<TA, TC>(a, st)));
  PDX_TRY((e.check_cast<TB, TC>(b, st)));
  const int64_t n = a->length;
  const TA* pa = static_cast<const TA*>(a->values) + a->offset;
  const TB* pb = static_cast<const TB*>(b->values) + b->offset;
  const int vec = aligned16(pa) && (scalar || aligned16(pb));
  const dim3 grid(grid_for(((n + 4095) >> 12) * 64, 256)), block(256);
#define CN_ARGS pa, pb, out, n, vec, validity_or_null(a), a->offset, validity_or_null(b), b->offset, e.dev
  if (scalar) hipLaunchKernelGGL((k_compare_n<TA, TB, TC, OP, true>), grid, block, 0, st, CN_ARGS);
  else hipLaunchKernelGGL((k_compare_n<TA, TB, TC, OP, false>), grid, block, 0, st, CN_ARGS);
#undef CN_ARGS
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

template <typename TA, typename TB, typename TO>
static int launch_if_else(const pdx_column* cond, const pdx_column* a, const pdx_column* b, int scalar, pdx_mut_column* out, CallErrors& e, hipStream_t st) {
  PDX_TRY((e.check_cast<TA, TO>(a, st)));
  PDX_TRY((e.check_cast<TB, TO>(b, st)));
  const int64_t n = cond->length;
  const dim3 grid(grid_for(n, 256, 4)), block(256);
#define IEN_ARGS static_cast<const uint8_t*>(cond->values), cond->offset, static_cast<const TA*>(a->values) + a->offset, validity_or_null(a), a->offset, \
                 a->length, static_cast<const TB*>(b->values) + b->offset, validity_or_null(b), b->offset, b->length, static_cast<TO*>(out->values), n, \
                 validity_or_null(cond), static_cast<uint8_t*>(out->validity), e.dev
  if (scalar == PDX_SCALAR_RHS) hipLaunchKernelGGL((k_if_else_n<TA, TB, TO, 1>), grid, block, 0, st, IEN_ARGS);
  else if (scalar == PDX_SCALAR_LHS) hipLaunchKernelGGL((k_if_else_n<TA, TB, TO, 2>), grid, block, 0, st, IEN_ARGS);
  else hipLaunchKernelGGL((k_if_else_n<TA, TB, TO, 0>), grid, block, 0, st, IEN_ARGS);
#undef IEN_ARGS
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

template <int OP, typename TI, typename TO>
static int launch_unary(const pdx_column* a, pdx_mut_column* out, double expo, CallErrors& e, hipStream_t st) {
  const TI* in = static_cast<const TI*>(a->values) + a->offset;
  const int vec = aligned16(in) && aligned16(out->values);
  hipLaunchKernelGGL((k_unary_n<OP, TI, TO>), dim3(grid_for(a->length, 256, 4)), dim3(256), 0, st, in, static_cast<TO*>(out->values), a->length,
                     vec, expo, validity_or_null(a), a->offset, e.dev);
  PDX_LAUNCH_CHECK();
  return PDX_OK;
}

// the value casts pdx_cast offers besides the identity: an integer to a wider integer or to a float, a float to a wider float
template <typename TI, typename TO>
constexpr bool safe_cast() { return is_float_t<TI>() ? is_float_t<TO>() && sizeof(TO) > sizeof(TI) : is_float_t<TO>() || sizeof(TO) > sizeof(TI); }

// a (validated) into out, value by value: a copy for the same dtype, else Arrow's cast, range-checked where it is not exact when `checked`
static int cast_values(const pdx_column* a, int checked, pdx_mut_column* out, hipStream_t st) {
  const int64_t n = a->length;
  CallErrors e;
  if (a->dtype == out->dtype) {
    const size_t w = (size_t)dtype_bytes(a->dtype);
    PDX_HIP(hipMemcpyAsync(out->values, static_cast<const char*>(a->values) + (size_t)a->offset * w, (size_t)n * w, hipMemcpyDeviceToDevice, st));
  } else {
    PDX_TRY(with_num_type(a->dtype, [&](auto ti) {
      return with_num_type(out->dtype, [&](auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        if constexpr (safe_cast<TI, TO>()) {
          if constexpr (checked_cast<TI, TO>())
            if (!checked) return launch_unary<kPlainCastOp, TI, TO>(a, out, 0.0, e, st);
          PDX_TRY((e.check_cast<TI, TO>(a, st)));
          return launch_unary<kCastOp, TI, TO>(a, out, 0.0, e, st);
        } else {
          return fail(PDX_INVALID, "internal: cast_values on an unsupported pair");
        }
      });
    }));
  }
  if (out->validity) PDX_TRY(launch_validity_and(a, nullptr, 0, n, static_cast<uint8_t*>(out->validity), st));
  return e.status(st);
}

}  // namespace pdx

using namespace pdx;

static int unary_impl(int op, const pdx_column* a, double expo, pdx_mut_column* out, void* stream, const char* who) {
  PDX_TRY(check_column(a, who, op != kPowerOp));
  if (a->dtype != PDX_INT64 && a->dtype != PDX_UINT64 && a->dtype != PDX_FLOAT64 && !is_narrow(a->dtype))
    return fail(PDX_NOT_IMPLEMENTED, std::string(who) + ": input must be int64, uint64, float64, int32 or float32");
  if (op != kPowerOp && (op < PDX_NEGATE || op > PDX_BIT_NOT)) return fail(PDX_INVALID, std::string(who) + ": unknown op");
  if (op == PDX_BIT_NOT && a->dtype == PDX_FLOAT64) return fail(PDX_NOT_IMPLEMENTED, "Function 'bit_wise_not' has no kernel matching input types (double)");
  if (op == PDX_BIT_NOT && a->dtype == PDX_FLOAT32) return fail(PDX_NOT_IMPLEMENTED, "Function 'bit_wise_not' has no kernel matching input types (float)");
  // sqrt / exp / power compute in float32 for float32 input, else in float64; sign of an integer is int64 (Arrow's int8 has no dtype here)
  const bool to_float = op == PDX_SQRT || op == PDX_EXP || op == kPowerOp;
  const bool is_f = a->dtype == PDX_FLOAT64 || a->dtype == PDX_FLOAT32;
  const int out_dt = to_float ? (a->dtype == PDX_FLOAT32 ? PDX_FLOAT32 : PDX_FLOAT64) : (op == PDX_SIGN && !is_f) ? PDX_INT64 : a->dtype;
  if (!out || out->length < a->length || out->dtype != out_dt) return fail(PDX_INVALID, std::string(who) + ": output dtype / length do not match the result");
  const bool has_nulls = validity_or_null(a) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, std::string(who) + ": input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  const int64_t n = a->length;
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, std::string(who) + ": null output buffer");
  CallErrors e;
  auto go = [&](auto ti) -> int {
    using TI = decltype(ti);
    using TF = typename std::conditional<__is_same(TI, float), float, double>::type;
    using TS = typename std::conditional<is_float_t<TI>(), TI, int64_t>::type;
    switch (op) {
      case PDX_NEGATE: return launch_unary<PDX_NEGATE, TI, TI>(a, out, expo, e, st);
      case PDX_ABS: return launch_unary<PDX_ABS, TI, TI>(a, out, expo, e, st);
      case PDX_SIGN: return launch_unary<PDX_SIGN, TI, TS>(a, out, expo, e, st);
      case PDX_SQRT: PDX_TRY((e.check_cast<TI, TF>(a, st))); return launch_unary<PDX_SQRT, TI, TF>(a, out, expo, e, st);
      case PDX_EXP: PDX_TRY((e.check_cast<TI, TF>(a, st))); return launch_unary<PDX_EXP, TI, TF>(a, out, expo, e, st);
      case PDX_BIT_NOT:
        if constexpr (!is_float_t<TI>()) return launch_unary<PDX_BIT_NOT, TI, TI>(a, out, expo, e, st);
        break;
      default:  // power (8-byte input only: check_column refused the others)
        if constexpr (sizeof(TI) == 8) {
          PDX_TRY((e.check_cast<TI, double>(a, st)));
          return launch_unary<kPowerOp, TI, double>(a, out, expo, e, st);
        }
        break;
    }
    return fail(PDX_INVALID, std::string("internal: ") + who + " on an unsupported dtype");
  };
  PDX_TRY(a->dtype == PDX_UINT64 ? go(uint64_t{}) : with_num_type(a->dtype, go));
  if (out->validity) PDX_TRY(launch_validity_and(a, nullptr, 0, n, static_cast<uint8_t*>(out->validity), st));
  return e.status(st);
}

extern "C" {

int pdx_if_else(const pdx_column* cond, const pdx_column* a, const pdx_column* b, int scalar_side, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_column(cond, "pdx_if_else"));
  if (cond->dtype != PDX_BOOL) return fail(PDX_INVALID, "pdx_if_else: the condition must be PDX_BOOL");
  PDX_TRY(check_column(a, "pdx_if_else", true));
  PDX_TRY(check_column(b, "pdx_if_else", true));
  auto num = [](int dt) { return dt == PDX_INT64 || dt == PDX_FLOAT64 || is_narrow(dt); };
  if (!num(a->dtype) || !num(b->dtype)) return fail(PDX_NOT_IMPLEMENTED, "pdx_if_else: only int64/float64/int32/float32 operands are supported");
  if (scalar_side < 0 || scalar_side > PDX_SCALAR_LHS) return fail(PDX_INVALID, "pdx_if_else: scalar side must be 0 (none), 1 (rhs) or 2 (lhs)");
  const int64_t n = cond->length;
  if ((scalar_side == PDX_SCALAR_LHS ? a->length != 1 : a->length != n) || (scalar_side == PDX_SCALAR_RHS ? b->length != 1 : b->length != n))
    return fail(PDX_INVALID, "pdx_if_else: Array arguments must all be the same length (a scalar operand has length 1)");
  const int out_dt = result_dt(a->dtype, b->dtype);
  if (!out || out->length < n || out->dtype != out_dt) return fail(PDX_INVALID, "pdx_if_else: output dtype / length do not match the result");
  const bool has_nulls = validity_or_null(cond) || validity_or_null(a) || validity_or_null(b);
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_if_else: inputs carry nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, "pdx_if_else: null output buffer");
  CallErrors e;
  PDX_TRY(with_num_type(a->dtype, [&](auto ta) {
    return with_num_type(b->dtype, [&](auto tb) {
      using TA = decltype(ta);
      using TB = decltype(tb);
      return launch_if_else<TA, TB, typename Promote<TA, TB>::type>(cond, a, b, scalar_side, out, e, st);
    });
  }));
  return e.status(st);
}

int pdx_cast_f64(const pdx_column* a, int checked, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_column(a, "pdx_cast_f64"));
  if (a->dtype != PDX_INT64 && a->dtype != PDX_FLOAT64) return fail(PDX_NOT_IMPLEMENTED, "pdx_cast_f64: input must be int64 or float64");
  if (!out || out->length < a->length || out->dtype != PDX_FLOAT64) return fail(PDX_INVALID, "pdx_cast_f64: output must be PDX_FLOAT64 of the input length");
  const bool has_nulls = validity_or_null(a) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_cast_f64: input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = a->length;
  out->null_count = has_nulls ? -1 : 0;
  if (a->length == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, "pdx_cast_f64: null output buffer");
  return cast_values(a, checked, out, st);
}

int pdx_cast(const pdx_column* a, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_column(a, "pdx_cast", true));
  if (!out) return fail(PDX_INVALID, "pdx_cast: null output");
  const int from = a->dtype, to = out->dtype;
  if (from == PDX_INT64 && to == PDX_FLOAT64) return pdx_cast_f64(a, 1, out, stream);
  const bool same = from == to && (from == PDX_INT64 || from == PDX_FLOAT64 || is_narrow(from));
  const bool widen = from == PDX_INT32 ? (to == PDX_INT64 || to == PDX_FLOAT64) : from == PDX_FLOAT32 && to == PDX_FLOAT64;
  const bool to_f32 = to == PDX_FLOAT32 && (from == PDX_INT32 || from == PDX_INT64);
  if (!same && !widen && !to_f32)
    return fail(PDX_NOT_IMPLEMENTED, std::string("pdx_cast: no cast from ") + dtype_name(from) + " to " + dtype_name(to));
  if (out->length < a->length) return fail(PDX_INVALID, "pdx_cast: output too small");
  const bool has_nulls = validity_or_null(a) != nullptr;
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_cast: input carries nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  out->length = a->length;
  out->null_count = has_nulls ? -1 : 0;
  if (a->length == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, "pdx_cast: null output buffer");
  return cast_values(a, 1, out, st);
}

int pdx_unary(int op, const pdx_column* a, pdx_mut_column* out, void* stream) { return unary_impl(op, a, 0.0, out, stream, "pdx_unary"); }
int pdx_power(const pdx_column* a, double exponent, pdx_mut_column* out, void* stream) { return unary_impl(kPowerOp, a, exponent, out, stream, "pdx_power"); }

int pdx_binary(int op, const pdx_column* a, const pdx_column* b, int b_is_scalar, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_numeric_pair(a, b, b_is_scalar, "pdx_binary"));
  if (op < PDX_ADD || op > PDX_SHIFT_RIGHT) return fail(PDX_INVALID, "pdx_binary: unknown op");
  auto int_dt = [](int dt) { return dt == PDX_INT64 || dt == PDX_INT32; };
  if (op >= PDX_BIT_OR && (!int_dt(a->dtype) || !int_dt(b->dtype)))
    return fail(PDX_NOT_IMPLEMENTED, "pdx_binary: bit-wise operators and shifts have no kernel matching floating-point input types");
  const pdx_column* arr = b_is_scalar == PDX_SCALAR_LHS ? b : a;  // the operand that gives the result its length
  if (!out || out->length < arr->length) return fail(PDX_INVALID, "pdx_binary: output too small");
  if (out->dtype != result_dt(a->dtype, b->dtype)) return fail(PDX_INVALID, "pdx_binary: output dtype must be the promoted input dtype");
  const bool has_nulls = validity_or_null(a) || validity_or_null(b);
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_binary: inputs carry nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  int64_t n = arr->length;
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, "pdx_binary: null output buffer");
  CallErrors e;
  PDX_TRY(with_num_type(a->dtype, [&](auto ta) {
    return with_num_type(b->dtype, [&](auto tb) {
      using TA = decltype(ta);
      using TB = decltype(tb);
      using TO = typename Promote<TA, TB>::type;
      TO* o = static_cast<TO*>(out->values);
      switch (op) {
        case PDX_ADD: return launch_binary<TA, TB, TO, PDX_ADD>(a, b, b_is_scalar, o, e, st);
        case PDX_SUB: return launch_binary<TA, TB, TO, PDX_SUB>(a, b, b_is_scalar, o, e, st);
        case PDX_MUL: return launch_binary<TA, TB, TO, PDX_MUL>(a, b, b_is_scalar, o, e, st);
        case PDX_DIV: return launch_binary<TA, TB, TO, PDX_DIV>(a, b, b_is_scalar, o, e, st);
        default:
          if constexpr (!is_float_t<TO>()) {
            switch (op) {
              case PDX_BIT_OR: return launch_binary<TA, TB, TO, PDX_BIT_OR>(a, b, b_is_scalar, o, e, st);
              case PDX_BIT_AND: return launch_binary<TA, TB, TO, PDX_BIT_AND>(a, b, b_is_scalar, o, e, st);
              case PDX_BIT_XOR: return launch_binary<TA, TB, TO, PDX_BIT_XOR>(a, b, b_is_scalar, o, e, st);
              case PDX_SHIFT_LEFT: return launch_binary<TA, TB, TO, PDX_SHIFT_LEFT>(a, b, b_is_scalar, o, e, st);
              default: return launch_binary<TA, TB, TO, PDX_SHIFT_RIGHT>(a, b, b_is_scalar, o, e, st);
            }
          }
          return fail(PDX_INVALID, "internal: bit-wise pdx_binary on a float result");
      }
    });
  }));
  if (out->validity) {  // AND is symmetric: the array operand goes first, the scalar's one bit is broadcast
    if (b_is_scalar == PDX_SCALAR_LHS) PDX_TRY(launch_validity_and(b, a, 1, n, static_cast<uint8_t*>(out->validity), st));
    else PDX_TRY(launch_validity_and(a, b, b_is_scalar, n, static_cast<uint8_t*>(out->validity), st));
  }
  return e.status(st);
}

int pdx_compare(int op, const pdx_column* a, const pdx_column* b, int b_is_scalar, pdx_mut_column* out, void* stream) {
  PDX_TRY(check_numeric_pair(a, b, b_is_scalar, "pdx_compare"));
  if (op < PDX_EQ || op > PDX_GE) return fail(PDX_INVALID, "pdx_compare: unknown op");
  if (b_is_scalar == PDX_SCALAR_LHS) {
    // scalar OP array == array OP' scalar with the mirrored relation (booleans carry no NaN payload, so this is exact)
    static const int mirrored[6] = {PDX_EQ, PDX_NE, PDX_GT, PDX_GE, PDX_LT, PDX_LE};
    const pdx_column* t = a;
    a = b;
    b = t;
    op = mirrored[op];
    b_is_scalar = PDX_SCALAR_RHS;
  }
  if (!out || out->length < a->length || out->dtype != PDX_BOOL) return fail(PDX_INVALID, "pdx_compare: output must be PDX_BOOL of the input length");
  const bool has_nulls = validity_or_null(a) || validity_or_null(b);
  if (has_nulls && !out->validity) return fail(PDX_INVALID, "pdx_compare: inputs carry nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  int64_t n = a->length;
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  if (!out->values) return fail(PDX_INVALID, "pdx_compare: null output buffer");
  CallErrors e;
  uint8_t* o = static_cast<uint8_t*>(out->values);
  PDX_TRY(with_num_type(a->dtype, [&](auto ta) {
    return with_num_type(b->dtype, [&](auto tb) {
      using TA = decltype(ta);
      using TB = decltype(tb);
      using TC = typename Promote<TA, TB>::type;
      switch (op) {
        case PDX_EQ: return launch_compare<TA, TB, TC, PDX_EQ>(a, b, b_is_scalar, o, e, st);
        case PDX_NE: return launch_compare<TA, TB, TC, PDX_NE>(a, b, b_is_scalar, o, e, st);
        case PDX_LT: return launch_compare<TA, TB, TC, PDX_LT>(a, b, b_is_scalar, o, e, st);
        case PDX_LE: return launch_compare<TA, TB, TC, PDX_LE>(a, b, b_is_scalar, o, e, st);
        case PDX_GT: return launch_compare<TA, TB, TC, PDX_GT>(a, b, b_is_scalar, o, e, st);
        default: return launch_compare<TA, TB, TC, PDX_GE>(a, b, b_is_scalar, o, e, st);
      }
    });
  }));
  if (out->validity) PDX_TRY(launch_validity_and(a, b, b_is_scalar, n, static_cast<uint8_t*>(out->validity), st));
  return e.status(st);
}

static int logical_impl(int mode, const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream, const char* what) {
  PDX_TRY(check_column(a, what));
  if (a->dtype != PDX_BOOL) return fail(PDX_INVALID, std::string(what) + ": operands must be PDX_BOOL");
  if (b) {
    PDX_TRY(check_column(b, what));
    if (b->dtype != PDX_BOOL) return fail(PDX_INVALID, std::string(what) + ": operands must be PDX_BOOL");
    if (a->length != b->length) return fail(PDX_INVALID, std::string(what) + ": array lengths differ");
  }
  if (!out || out->length < a->length || out->dtype != PDX_BOOL) return fail(PDX_INVALID, std::string(what) + ": output must be PDX_BOOL of the input length");
  const bool has_nulls = validity_or_null(a) || (b && validity_or_null(b));
  if (has_nulls && !out->validity) return fail(PDX_INVALID, std::string(what) + ": inputs carry nulls but output has no validity buffer");
  hipStream_t st = as_stream(stream);
  int64_t n = a->length;
  out->length = n;
  out->null_count = has_nulls ? -1 : 0;
  if (n == 0) return PDX_OK;
  int64_t nwords = (n + 63) >> 6;
  hipLaunchKernelGGL(k_logical, dim3(grid_for(nwords, 256)), dim3(256), 0, st, static_cast<const uint8_t*>(a->values), a->offset,
                     a->offset + a->length, b ? static_cast<const uint8_t*>(b->values) : nullptr, b ? b->offset : 0,
                     b ? b->offset + b->length : 0, mode, n, static_cast<uint8_t*>(out->values));
  PDX_LAUNCH_CHECK();
  if (out->validity) PDX_TRY(launch_validity_and(a, b, 0, n, static_cast<uint8_t*>(out->validity), st));
  return PDX_OK;
}

int pdx_logical(int op, const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream) {
  if (op != PDX_AND && op != PDX_OR) return fail(PDX_INVALID, "pdx_logical: unknown op");
  if (!b) return fail(PDX_INVALID, "pdx_logical: null column");
  return logical_impl(op == PDX_AND ? 0 : 1, a, b, out, stream, "pdx_logical");
}
int pdx_invert(const pdx_column* a, pdx_mut_column* out, void* stream) { return logical_impl(2, a, nullptr, out, stream, "pdx_invert"); }

}  // extern "C"
