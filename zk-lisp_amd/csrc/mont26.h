// Montgomery arithmetic on 5 x 26-bit limbs shared by the Poseidon kernels (poseidon.hip)
// and the NTT / DEEP kernels (kernels.hip).  Device-inline, no device state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.h"

namespace zkl {

// ---- Montgomery arithmetic on 5 x 26-bit limbs (R = 2^156) ---------------------------
// p = 1 + 0x3F4C000*2^26 + (2^26-1)*2^52 + (2^26-1)*2^78 + (2^24-1)*2^104, and p == 1
// (mod 2^26), so the REDC quotient digit is m = -x mod 2^26 with no multiplication.
// Products accumulate in 64-bit columns by v_mad_u64_u32 with no carry handling: with
// limbs < 2^28 a column holds at most 60 products < 2^56, far below 2^64.  Values are
// kept lazily reduced (< 2^130) inside the permutation and canonicalised on output.

constexpr uint32_t M26 = 0x3FFFFFFu;

__host__ __device__ __forceinline__ void to26(fe a, uint32_t l[5]) {
  l[0] = (uint32_t)a.lo & M26;
  l[1] = (uint32_t)(a.lo >> 26) & M26;
  l[2] = (uint32_t)((a.lo >> 52) | (a.hi << 12)) & M26;
  l[3] = (uint32_t)(a.hi >> 14) & M26;
  l[4] = (uint32_t)(a.hi >> 40);
}

// col[0..9] = X (< 2^262, columns < 2^62); out = X * 2^-156 mod p + (0 or p): normalised
// 26-bit limbs of a value in (0, 2^130).  p = 1 + 45*2^14*2^26 ... written in columns is
// p = 2^0 + 737280*2^26 - 2^24*2^104 (... - 45*2^40 + 2^128), so removing m*p*2^(26i)
// from X touches only three columns: col_i -= m (exact: m = col_i mod 2^26, the rest
// carries), col_{i+1} += 737280*m, col_{i+4} -= 2^24*m.  Columns are signed; adding
// p*2^156 up front (col_6 += 1, col_7 -= 737280, col_9 += 2^50) keeps the result positive.
__host__ __device__ __forceinline__ void redc(uint64_t colu[10], uint32_t out[5]) {
  int64_t col[10];
#pragma unroll
  for (int i = 0; i < 10; i++) col[i] = (int64_t)colu[i];
  col[6] += 1;
  col[7] -= 737280;
  col[9] += (int64_t)1 << 50;
  // opaque copies of the two reduction constants: keeps -2^24*m a single v_mad_i64_i32
  // instead of a 64-bit shift + subtract
  int32_t kneg = -16777216;
  uint32_t k45 = 737280u;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(kneg), "+s"(k45));
#endif
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const uint32_t m = (uint32_t)col[i] & M26;
    col[i + 1] += col[i] >> 26;
    col[i + 1] += (int64_t)((uint64_t)m * k45);
    col[i + 4] += (int64_t)(int32_t)m * (int64_t)kneg;
  }
  int64_t c = 0;
#pragma unroll
  for (int t = 0; t < 3; t++) {
    const int64_t v = col[6 + t] + c;
    out[t] = (uint32_t)v & M26;
    c = v >> 26;
  }
  const int64_t v = col[9] + c;
  out[3] = (uint32_t)v & M26;
  out[4] = (uint32_t)(v >> 26);
}

// REDC with R' = 2^130 (the matrix-core permutation's radix): five digit steps instead of
// six.  col[0..8] = X < 2^262 (columns < 2^62); out = X * 2^-130 mod p + (0 or p), the
// normalised limbs of a value in (0, X / 2^130 + p): inputs < 2^129 give outputs < 2^129
// (2^258 / 2^130 + p < 2^129), inputs < 2^130 outputs < 2^131.  The bias p * 2^130 is
// col_5 += 1, col_6 -= 737280, col_9 += 2^24; limb 4 of the output carries everything
// above bit 104 (< 2^28).
__host__ __device__ __forceinline__ void redc130(uint64_t colu[10], uint32_t out[5]) {
  int64_t col[10];
#pragma unroll
  for (int i = 0; i < 10; i++) col[i] = (int64_t)colu[i];
  col[5] += 1;
  col[6] -= 737280;
  col[9] += (int64_t)1 << 24;
  int32_t kneg = -16777216;
  uint32_t k45 = 737280u;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(kneg), "+s"(k45));
#endif
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint32_t m = (uint32_t)col[i] & M26;
    col[i + 1] += col[i] >> 26;
    col[i + 1] += (int64_t)((uint64_t)m * k45);
    col[i + 4] += (int64_t)(int32_t)m * (int64_t)kneg;
  }
  int64_t c = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int64_t v = col[5 + t] + c;
    out[t] = (uint32_t)v & M26;
    c = v >> 26;
  }
  out[4] = (uint32_t)(col[9] + c);
}

__host__ __device__ __forceinline__ void mac5(const uint32_t a[5], const uint32_t b[5], uint64_t col[10]) {
#pragma unroll
  for (int u = 0; u < 5; u++)
#pragma unroll
    for (int v = 0; v < 5; v++) col[u + v] += (uint64_t)a[u] * b[v];
}

__host__ __device__ __forceinline__ void mont_mul(const uint32_t a[5], const uint32_t b[5], uint32_t out[5]) {
  uint64_t col[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  mac5(a, b, col);
  redc(col, out);
}

__host__ __device__ __forceinline__ void mont_cube(const uint32_t a[5], uint32_t out[5]) {
  uint64_t col[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t d[5];
#pragma unroll
  for (int u = 0; u < 5; u++) d[u] = a[u] << 1;
#pragma unroll
  for (int u = 0; u < 5; u++) {
    col[2 * u] += (uint64_t)a[u] * a[u];
#pragma unroll
    for (int v = u + 1; v < 5; v++) col[u + v] += (uint64_t)d[u] * a[v];
  }
  uint32_t sq[5];
  redc(col, sq);
  mont_mul(sq, a, out);
}

// x^3 R'^-2 (R' = 2^130) with the squaring shortcut; inputs < 2^129 give outputs < 2^129,
// inputs < 2^130 (a state element right after absorbing a message) outputs < 2^131
__host__ __device__ __forceinline__ void mont_cube130(const uint32_t a[5], uint32_t out[5]) {
  uint64_t col[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t d[5];
#pragma unroll
  for (int u = 0; u < 5; u++) d[u] = a[u] << 1;
#pragma unroll
  for (int u = 0; u < 5; u++) {
    col[2 * u] += (uint64_t)a[u] * a[u];
#pragma unroll
    for (int v = u + 1; v < 5; v++) col[u + v] += (uint64_t)d[u] * a[v];
  }
  uint32_t sq[5];
  redc130(col, sq);
  uint64_t c2[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  mac5(sq, a, c2);
  redc130(c2, out);
}

// ---- the matrix-core round's own cube and fold ----------------------------------------
// ZKL_RANGE_CHECK(v, bits) lets a host test assert the bounds derived below where a carry is
// taken in 32 bits (v < 2^bits as an unsigned number, so a negative column fails it too).
#ifndef ZKL_RANGE_CHECK
#define ZKL_RANGE_CHECK(v, bits) ((void)0)
#endif
// carry of a column known to lie in [0, 2^58): col >> 26 < 2^32, one 32-bit funnel shift of the
// column's two halves (v_alignbit_b32) instead of a 64-bit shift
__host__ __device__ __forceinline__ uint32_t carry26(uint64_t col) {
  ZKL_RANGE_CHECK(col, 58);
  return (uint32_t)(col >> 26);
}

// One link of a column's chain: a * b + c as one v_mad_u64_u32 / v_mad_i64_i32.  The result is
// pinned (an empty asm the compiler cannot look through) so that the sum keeps this order:
// reassociated, the products of a column are summed first and the carry that opens the chain
// is added to them with a 64-bit add of its own -- the instruction the chain exists to avoid.
#if defined(__HIP_DEVICE_COMPILE__)
#define ZKL_PIN64(x) asm("" : "+v"(x))
#else
#define ZKL_PIN64(x) ((void)0)
#endif
__host__ __device__ __forceinline__ int64_t mad_link(uint32_t a, uint32_t b, int64_t c) {
  int64_t r = (int64_t)((uint64_t)a * b + (uint64_t)c);
  ZKL_PIN64(r);
  return r;
}
__host__ __device__ __forceinline__ int64_t mad_link_i(int32_t a, int32_t b, int64_t c) {
  int64_t r = (int64_t)a * (int64_t)b + c;
  ZKL_PIN64(r);
  return r;
}

// t + the products of column k: of a^2 on doubled limbs d = 2a (SQ), or of s * a
template <bool SQ>
__host__ __device__ __forceinline__ int64_t cube_col(int k, const uint32_t s[5], const uint32_t d[5],
                                                     const uint32_t a[5], int64_t t) {
#pragma unroll
  for (int u = 0; u < 5; u++) {
    const int v = k - u;
    if (v < 0 || v > 4) continue;
    if (!SQ) t = mad_link(s[u], a[v], t);
    else if (u < v) t = mad_link(d[u], a[v], t);
    else if (u == v) t = mad_link(a[u], a[u], t);
  }
  return t;
}

// Products and redc130 in one pass, column by column: column k + 1 is a chain of multiply-adds
// that STARTS from column k's carry (col_k >> 26, one 64-bit shift), takes its products, then
// m_k * 737280 and -2^24 m_(k-3).  redc130 sums a column's products first and then adds the carry
// to them: a 64-bit add per column and three more for the bias, none of which is left here,
// because a multiply-add has an addend anyway.  The bias p 2^130 (col_5 += 1, col_6 -= 737280,
// col_9 += 2^24) rides on the -2^24 m links, whose multiplicand takes a 32-bit constant:
//   col_4 += (m_0 - 4) (-2^24)            = -2^24 m_0 + 2^26, which reaches column 5 as + 1 and
//                                           leaves m_4 (col_4 mod 2^26) what it was;
//   col_5 += (m_1 + 4 * 737280) (-2^24)   = -2^24 m_1 - 737280 * 2^26, which reaches column 6
//                                           as - 737280 and leaves limb 0 what it was;
//   limb 4 = (col_8 >> 26) + 2^24 in 32 bits (nothing else reaches column 9).
// Columns are signed as in redc130 and stay below 2^62 for limbs < 2^28; the sum of the columns,
// and with it every digit and output limb, is redc130's, so the result is the same integer.
// A dependent v_mad_u64_u32 issues as fast as an independent one (profiles/r01/madbench.txt:
// 10.02 against 10.03 cycles), so the longer chain costs no issue time.
template <bool SQ>
__host__ __device__ __forceinline__ void redc130_chain(const uint32_t s[5], const uint32_t d[5], const uint32_t a[5],
                                                       uint32_t out[5]) {
  int32_t kneg = -16777216;
  uint32_t k45 = 737280u;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(kneg), "+s"(k45));
#endif
  uint32_t m[5];
  int64_t t = cube_col<SQ>(0, s, d, a, 0);
#pragma unroll
  for (int i = 0; i < 5; i++) {
    m[i] = (uint32_t)t & M26;
    t >>= 26;
    t = cube_col<SQ>(i + 1, s, d, a, t);
    t = mad_link(m[i], k45, t);
    if (i == 3) t = mad_link_i((int32_t)m[0] - 4, kneg, t);
    if (i == 4) t = mad_link_i((int32_t)m[1] + 4 * 737280, kneg, t);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {  // t = column 5 + j
    out[j] = (uint32_t)t & M26;
    t >>= 26;
    if (j < 3) {
      t = cube_col<SQ>(6 + j, s, d, a, t);
      t = mad_link_i((int32_t)m[2 + j], kneg, t);
    }
  }
  out[4] = (uint32_t)t + (1u << 24);
}

// mont_cube130 in that form, in its two halves (the round runs the second half of one element
// beside the first half of the next, pm_round): a^2 R'^-1, and sq * a R'^-1
__host__ __device__ __forceinline__ void mont_sq130_chain(const uint32_t a[5], uint32_t sq[5]) {
  uint32_t d[5];
#pragma unroll
  for (int u = 0; u < 5; u++) d[u] = a[u] << 1;
  redc130_chain<true>(a, d, a, sq);
}
__host__ __device__ __forceinline__ void mont_mul130_chain(const uint32_t sq[5], const uint32_t a[5], uint32_t out[5]) {
  redc130_chain<false>(sq, a, a, out);
}
// the same limbs as mont_cube130 for the same input
__host__ __device__ __forceinline__ void mont_cube130_chain(const uint32_t a[5], uint32_t out[5]) {
  uint32_t sq[5];
  mont_sq130_chain(a, sq);
  mont_mul130_chain(sq, a, out);
}

// Fold of the matrix-core round: the 16 digit-column sums Y_c (|Y_c| < 2^22; the MFMA gives
// |Y_c| < 2^21.6) of one element plus its round-constant columns rk -> 26-bit limbs of a value
// < 2^129 congruent to it.  Each digit pair (or lone digit) enters its limb column with one
// v_mad_i64_i32 (the shift as an opaque SGPR multiplier: a constant would become sign-extend +
// shift + add).
// Column bounds.  rk[t] = canonical limb (< 2^26; < 2^24 for t = 4) + the column of p 2^15
// (< 2^26; 2^39 - 1 for t = 4) + PM_NORM_B for t < 4 - PM_NORM_B / 2^26 for t > 0 (pm_build):
// the last two cancel in sum_t rk[t] 2^(26t) and keep every column non-negative.  The digit part
// of column t is below 2^22 (1 + 2^8 + 2^16 + 2^24) < 2^46.01 in magnitude (t = 0; smaller for
// the others, < 2^38.01 for t = 4), so
//   t < 4:  0 < 2^47 - 2^21 - 2^46.01 < col_t < 2^47 + 2^27 + 2^46.01 < 2^48, carry < 2^22
//   t = 4:  0 < 2^39 - 1 - 2^21 - 2^38.01 < col_4 < 2^39 + 2^24 + 2^38.01 < 2^40, top < 2^16
// No carry runs through the columns: limb t is (col_t mod 2^26) + (col_(t-1) >> 26), all in 32
// bits, and the bits of column 4 from 24 up are `top`, folded with 2^128 == 45 2^40 - 1.  The
// limbs are therefore not normalised: x0, x1 < 2^26, x2 < 2^26 + 2^22 + 2^10, x3 < 2^26 + 2^22,
// x4 < 2^24 + 2^22, a value < 2^128.4 (mont_cube130's < 2^129).
constexpr uint64_t PM_NORM_B = (uint64_t)1 << 47;
struct PmShifts {  // 2^s as opaque SGPR multipliers (set once per permutation)
  int32_t k0, k2, k4, k6, k16, k18, k20, k22;
};
__host__ __device__ __forceinline__ PmShifts pm_shifts() {
  PmShifts K{1, 4, 16, 64, 65536, 262144, 1048576, 4194304};
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(K.k0), "+s"(K.k2), "+s"(K.k4), "+s"(K.k6), "+s"(K.k16), "+s"(K.k18), "+s"(K.k20), "+s"(K.k22));
#endif
  return K;
}

template <class V>  // V: 16 int32 digit-column sums, indexed (the MFMA accumulator on the device)
__host__ __device__ __forceinline__ void pm_normalise(const PmShifts& K, const V& Y, const uint64_t rk[5], uint32_t x[5]) {
  const int32_t k0 = K.k0, k2 = K.k2, k4 = K.k4, k6 = K.k6, k16 = K.k16, k18 = K.k18, k20 = K.k20, k22 = K.k22;
  auto mad = [](int32_t a, int32_t k, int64_t c) { return (int64_t)a * (int64_t)k + c; };
  // two neighbouring digits of one limb first combine in 32 bits (|Y_c + 2^8 Y_c+1| < 2^31,
  // one full-rate v_lshl_add_u32), so a limb takes one v_mad_i64_i32 per pair or lone digit:
  // 10 quarter-rate mads per element instead of 16
  auto pair = [](int32_t lo, int32_t hi) { return (int32_t)((uint32_t)lo + ((uint32_t)hi << 8)); };
  // digit c sits at bit 8c = 26t + s
  uint64_t col[5];
  col[0] = (uint64_t)mad(pair(Y[2], Y[3]), k16, mad(pair(Y[0], Y[1]), k0, (int64_t)rk[0]));
  col[1] = (uint64_t)mad(Y[6], k22, mad(pair(Y[4], Y[5]), k6, (int64_t)rk[1]));
  col[2] = (uint64_t)mad(Y[9], k20, mad(pair(Y[7], Y[8]), k4, (int64_t)rk[2]));
  col[3] = (uint64_t)mad(Y[12], k18, mad(pair(Y[10], Y[11]), k2, (int64_t)rk[3]));
  col[4] = (uint64_t)mad(Y[15], k16, mad(pair(Y[13], Y[14]), k0, (int64_t)rk[4]));
  uint32_t lo[4], hi[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    ZKL_RANGE_CHECK(col[t], 48);
    lo[t] = (uint32_t)col[t] & M26;
    hi[t] = carry26(col[t]);
  }
  ZKL_RANGE_CHECK(col[4], 40);
  // value = lo0 + (lo1 + hi0) 2^26 + ... + ((col4 mod 2^24) + hi3 + top 2^24) 2^104, top < 2^16;
  // top 2^128 == top (45 2^40 - 1) = top (2^26 - 1) + top 737279 2^26
  const uint32_t top = (uint32_t)(col[4] >> 24);
  const uint64_t a = (uint64_t)top * M26 + lo[0];
  const uint64_t b = (uint64_t)top * 737279u + (lo[1] + hi[0] + (uint32_t)(a >> 26));
  x[0] = (uint32_t)a & M26;
  x[1] = (uint32_t)b & M26;
  x[2] = lo[2] + hi[1] + (uint32_t)(b >> 26);
  x[3] = lo[3] + hi[2];
  x[4] = ((uint32_t)col[4] & 0xFFFFFFu) + hi[3];
}

// a cube's normalised limbs (< 2^131) as the matrix-core permutation's B words: four words of
// offset bytes (c = sum_j (b_j + 128) 2^(8j) + top 2^128) and the top
__host__ __device__ __forceinline__ void pm_pack_words(const uint32_t c[5], uint32_t w[5]) {
  w[0] = (c[0] | (c[1] << 26)) ^ 0x80808080u;
  w[1] = ((c[1] >> 6) | (c[2] << 20)) ^ 0x80808080u;
  w[2] = ((c[2] >> 12) | (c[3] << 14)) ^ 0x80808080u;
  w[3] = ((c[3] >> 18) | (c[4] << 8)) ^ 0x80808080u;
  w[4] = c[4] >> 24;
}

enum { DOM_ELEMS = 0, DOM_MERGE = 1, DOM_MANY = 2, DOM_INT = 3 };

static inline void limbs26(fe a, uint32_t l[5]) {
  l[0] = (uint32_t)a.lo & M26;
  l[1] = (uint32_t)(a.lo >> 26) & M26;
  l[2] = (uint32_t)((a.lo >> 52) | (a.hi << 12)) & M26;
  l[3] = (uint32_t)(a.hi >> 14) & M26;
  l[4] = (uint32_t)(a.hi >> 40);
}

}  // namespace zkl
