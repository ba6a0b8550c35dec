// Host test of the matrix-core Poseidon round's arithmetic (zk-lisp_amd/csrc/mont26.h):
// mont_cube130_chain (products and REDC as one multiply-add chain per column, bias folded into
// the chain) and pm_normalise (32-bit carries, no carry chain) against mont_cube130, the fold as
// it was before (ref_normalise below, the former pm_normalise with the former table bias) and
// plain arithmetic mod p.  Every column whose carry is taken in 32 bits passes through
// ZKL_RANGE_CHECK, which here fails the run when the column is outside the range derived in
// mont26.h; the largest carry seen per class is printed.
//   pm_carry_test [random inputs, default 100000]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace pmt {
static uint64_t g_max[65];
static int g_range_fail = 0;
static inline void range_check(uint64_t v, int bits) {
  if (v > g_max[bits]) g_max[bits] = v;
  if (v >> bits) g_range_fail++;
}
}  // namespace pmt
#define ZKL_RANGE_CHECK(v, bits) pmt::range_check((uint64_t)(v), bits)

#include "../../zk-lisp_amd/csrc/mont26.h"

using namespace zkl;
typedef unsigned __int128 u128;

static const u128 P = ((u128)P_HI << 64) | P_LO;
static int g_fail = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      if (g_fail++ < 20) {             \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);  \
        fprintf(stderr, "\n");         \
      }                                \
    }                                  \
  } while (0)

// ---- plain arithmetic mod p ------------------------------------------------------------
static u128 addmod(u128 a, u128 b) {
  u128 s = a + b;
  if (s < a) s += C_RED;  // wrapped: 2^128 == C_RED
  if (s >= P) s -= P;
  return s;
}
static u128 submod(u128 a, u128 b) { return addmod(a, b ? P - b : 0); }
static u128 mulmod(u128 a, u128 b) {
  u128 r = 0;
  int top = 127;
  while (top > 0 && !((b >> top) & 1)) top--;
  for (int i = top; i >= 0; i--) {
    r = addmod(r, r);
    if ((b >> i) & 1) r = addmod(r, a);
  }
  return r;
}
static u128 pow2mod(int e) {
  u128 r = 1;
  for (int i = 0; i < e; i++) r = addmod(r, r);
  return r;
}
// sum_t l[t] 2^(26t) mod p for limbs of any 32-bit size
static u128 val(const uint32_t l[5]) {
  const u128 w = (u128)1 << 26;
  u128 acc = 0;
  for (int t = 4; t >= 0; t--) acc = addmod(mulmod(acc, w), (u128)l[t] % P);
  return acc;
}
// the integer itself, when it is below 2^128 + something: (high part, low 128 bits)
static bool below_2_129(const uint32_t l[5]) {
  // sum_t l[t] 2^(26t) < 2^129, computed in two halves
  u128 lo = (u128)l[0] + ((u128)l[1] << 26) + ((u128)l[2] << 52) + ((u128)l[3] << 78);  // < 2^111
  u128 hi = (u128)l[4];                                                                  // times 2^104
  return hi + (lo >> 104) < ((u128)1 << 25);
}

// from_mont130 of poseidon.hip on the host: the canonical field element of limbs a (R' = 2^130)
static u128 from_mont130_host(const uint32_t a[5]) {
  uint64_t col[10] = {a[0], a[1], a[2], a[3], a[4], 0, 0, 0, 0, 0};
  uint32_t l[5];
  redc130(col, l);
  u128 r = (u128)l[0] + ((u128)l[1] << 26) + ((u128)l[2] << 52) + ((u128)l[3] << 78) + ((u128)l[4] << 104);
  if (r >= P) r -= P;
  return r;
}

// ---- the fold as it was before the 32-bit carries (reference) ---------------------------
static void ref_normalise(const int32_t Y[16], const uint64_t rk[5], uint32_t x[5]) {
  auto mad = [](int32_t a, int32_t k, int64_t c) { return (int64_t)a * (int64_t)k + c; };
  auto pair = [](int32_t lo, int32_t hi) { return (int32_t)((uint32_t)lo + ((uint32_t)hi << 8)); };
  int64_t col[5];
  col[0] = mad(pair(Y[2], Y[3]), 65536, mad(pair(Y[0], Y[1]), 1, (int64_t)rk[0]));
  col[1] = mad(Y[6], 4194304, mad(pair(Y[4], Y[5]), 64, (int64_t)rk[1]));
  col[2] = mad(Y[9], 1048576, mad(pair(Y[7], Y[8]), 16, (int64_t)rk[2]));
  col[3] = mad(Y[12], 262144, mad(pair(Y[10], Y[11]), 4, (int64_t)rk[3]));
  col[4] = mad(Y[15], 65536, mad(pair(Y[13], Y[14]), 1, (int64_t)rk[4]));
  uint32_t l[4];
  for (int t = 0; t < 4; t++) {
    col[t + 1] += col[t] >> 26;
    l[t] = (uint32_t)col[t] & M26;
  }
  const uint32_t top = (uint32_t)((uint64_t)col[4] >> 24);
  const uint64_t a = (uint64_t)top * M26 + l[0];
  const uint64_t b = (uint64_t)top * 737279u + (l[1] + (uint32_t)(a >> 26));
  x[0] = (uint32_t)a & M26;
  x[1] = (uint32_t)b & M26;
  x[2] = l[2] + (uint32_t)(b >> 26);
  x[3] = l[3];
  x[4] = (uint32_t)col[4] & 0xFFFFFFu;
}

// rk of a table entry whose canonical limbs are l: the columns of p 2^15 as pm_build writes them,
// without (ref) and with (cur) the PM_NORM_B terms
static void make_rk(const uint32_t l[5], uint64_t ref[5], uint64_t cur[5]) {
  uint64_t bias[5];
  bias[0] = (uint64_t)((P & 0x7FF) << 15);
  for (int t = 1; t < 4; t++) bias[t] = (uint64_t)((P >> (26 * t - 15)) & M26);
  bias[4] = (uint64_t)(P >> 89);
  for (int t = 0; t < 5; t++) ref[t] = cur[t] = (uint64_t)l[t] + bias[t];
  for (int t = 0; t < 4; t++) {
    cur[t] += PM_NORM_B;
    cur[t + 1] -= PM_NORM_B >> 26;
  }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// limb maxima of the two callers of a cube
static const uint32_t ROUND_MAX[5] = {M26, M26, (1u << 26) + (1u << 22) + (1u << 10) - 1, (1u << 26) + (1u << 22) - 1,
                                      (1u << 24) + (1u << 22) - 1};
// right after an absorb: the above plus to_mont130's normalised limbs (value < 2^129: limb 4 < 2^25)
static const uint32_t ABSORB_MAX[5] = {ROUND_MAX[0] + M26, ROUND_MAX[1] + M26, ROUND_MAX[2] + M26, ROUND_MAX[3] + M26,
                                       ROUND_MAX[4] + (1u << 25) - 1};
static const int YMAX = (1 << 22) - 1;  // the bound the column derivation uses; the MFMA gives < 2^21.6

static u128 R260_INV;  // 2^-260: mont_cube130 gives x^3 R'^-2

// cube of limbs within the round's range: new == old limb for limb, normalised, and == x^3 2^-260
static void check_cube_round(const uint32_t x[5], const char* what) {
  uint32_t a[5], b[5];
  mont_cube130(x, a);
  mont_cube130_chain(x, b);
  for (int t = 0; t < 5; t++) CHECK(a[t] == b[t], "%s: cube limb %d: %u != %u", what, t, b[t], a[t]);
  for (int t = 0; t < 4; t++) CHECK(b[t] <= M26, "%s: cube limb %d not normalised", what, t);
  CHECK(b[4] < (1u << 25), "%s: cube limb 4 = %u", what, b[4]);
  const u128 v = val(x);
  CHECK(val(b) == mulmod(mulmod(mulmod(v, v), v), R260_INV), "%s: cube value", what);
  CHECK(from_mont130_host(a) == from_mont130_host(b), "%s: canonical cube", what);
}

// the first cube after an absorb keeps mont_cube130: x^3 2^-260 with limb 4 < 2^27; the chain
// form, which assumes no more of its input than mont_cube130 does, gives the same limbs there too
static void check_cube_absorb(const uint32_t x[5], const char* what) {
  uint32_t a[5], b[5];
  mont_cube130(x, a);
  mont_cube130_chain(x, b);
  for (int t = 0; t < 5; t++) CHECK(a[t] == b[t], "%s: cube limb %d: %u != %u", what, t, b[t], a[t]);
  for (int t = 0; t < 4; t++) CHECK(a[t] <= M26, "%s: cube limb %d not normalised", what, t);
  CHECK(a[4] < (1u << 27), "%s: cube limb 4 = %u", what, a[4]);
  const u128 v = val(x);
  CHECK(val(a) == mulmod(mulmod(mulmod(v, v), v), R260_INV), "%s: cube value", what);
}

// fold of digit columns Y and a table entry with canonical limbs l, then the cube of the result
static void check_fold(const int32_t Y[16], const uint32_t l[5], const char* what) {
  uint64_t rk_ref[5], rk_cur[5];
  make_rk(l, rk_ref, rk_cur);
  uint32_t xr[5], xn[5];
  ref_normalise(Y, rk_ref, xr);
  const PmShifts K = pm_shifts();
  pm_normalise(K, Y, rk_cur, xn);
  for (int t = 0; t < 5; t++) CHECK(xn[t] <= ROUND_MAX[t], "%s: fold limb %d = %u above its bound", what, t, xn[t]);
  CHECK(below_2_129(xn), "%s: fold value not below 2^129", what);
  // sum_c Y_c 2^(8c) + l + p 2^15 (mod p)
  u128 want = val(l);
  for (int c = 0; c < 16; c++) {
    const u128 term = mulmod(pow2mod(8 * c), (u128)(uint32_t)(Y[c] < 0 ? -Y[c] : Y[c]));
    want = Y[c] < 0 ? submod(want, term) : addmod(want, term);
  }
  CHECK(val(xn) == want, "%s: fold value", what);
  CHECK(val(xr) == want, "%s: reference fold value", what);
  CHECK(from_mont130_host(xn) == from_mont130_host(xr), "%s: canonical fold", what);
  uint32_t cr[5], cn[5];
  mont_cube130(xr, cr);
  mont_cube130_chain(xn, cn);
  CHECK(from_mont130_host(cn) == from_mont130_host(cr), "%s: canonical cube of fold", what);
  check_cube_round(xn, what);
}

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 100000;
  // 2^-260 = (2^-1)^260, 2^-1 = (p + 1) / 2
  {
    const u128 half = (P + 1) >> 1;
    u128 r = 1;
    for (int i = 0; i < 260; i++) r = mulmod(r, half);
    R260_INV = r;
    CHECK(mulmod(R260_INV, mulmod(pow2mod(130), pow2mod(130))) == 1, "2^-260");
  }
  const uint32_t zero[5] = {0, 0, 0, 0, 0};
  const uint32_t lmax[5] = {M26, M26, M26, M26, (1u << 24) - 1};  // every table limb at its maximum

  // ---- cube corners ----
  check_cube_round(zero, "zero");
  check_cube_round(ROUND_MAX, "round max");  // every product column at its bound
  check_cube_absorb(ABSORB_MAX, "absorb max");
  check_cube_absorb(zero, "absorb zero");
  {
    uint32_t l[5];
    const u128 v = mulmod(P - 1, pow2mod(130));  // p - 1 in Montgomery form
    l[0] = (uint32_t)v & M26, l[1] = (uint32_t)(v >> 26) & M26, l[2] = (uint32_t)(v >> 52) & M26;
    l[3] = (uint32_t)(v >> 78) & M26, l[4] = (uint32_t)(v >> 104);
    check_cube_round(l, "p - 1");
    check_cube_absorb(l, "absorb p - 1");
    const u128 one = pow2mod(130);
    l[0] = (uint32_t)one & M26, l[1] = (uint32_t)(one >> 26) & M26, l[2] = (uint32_t)(one >> 52) & M26;
    l[3] = (uint32_t)(one >> 78) & M26, l[4] = (uint32_t)(one >> 104);
    check_cube_round(l, "one");
  }
  // most negative columns: a digit m_i near 2^26 takes 2^24 m_i off column i + 4 while the products
  // there are small.  The largest a^2 mod 2^26 over single limbs, alone and beside a full top limb.
  {
    uint32_t best = 0, arg = 0;
    for (uint32_t a = 1; a <= M26; a += 2) {
      const uint32_t m = (uint32_t)((uint64_t)a * a) & M26;
      if (m > best) best = m, arg = a;
    }
    for (int pos = 0; pos < 5; pos++) {
      uint32_t l[5] = {0, 0, 0, 0, 0};
      l[pos] = arg < ROUND_MAX[pos] ? arg : ROUND_MAX[pos];
      check_cube_round(l, "single limb");
      l[4] = ROUND_MAX[4];
      check_cube_round(l, "single limb + top");
    }
    // one limb at its maximum, the others zero; and one limb zero, the others at their maxima
    for (int pos = 0; pos < 5; pos++) {
      uint32_t l[5] = {0, 0, 0, 0, 0}, h[5];
      l[pos] = ROUND_MAX[pos];
      for (int t = 0; t < 5; t++) h[t] = t == pos ? 0 : ROUND_MAX[t];
      check_cube_round(l, "one limb max");
      check_cube_round(h, "one limb zero");
    }
  }

  // ---- fold corners: every column at its highest and lowest ----
  {
    int32_t Y[16];
    for (int s = 0; s < 3; s++) {
      for (int c = 0; c < 16; c++) Y[c] = s == 0 ? YMAX : s == 1 ? -YMAX : 0;
      check_fold(Y, lmax, "fold all/max table");
      check_fold(Y, zero, "fold all/zero table");
    }
    // one limb column at an extreme, the others at the opposite one (carries differ the most)
    static const int first[6] = {0, 4, 7, 10, 13, 16};
    for (int t = 0; t < 5; t++)
      for (int sgn = -1; sgn <= 1; sgn += 2) {
        for (int c = 0; c < 16; c++) Y[c] = (c >= first[t] && c < first[t + 1]) ? sgn * YMAX : -sgn * YMAX;
        check_fold(Y, lmax, "fold one column");
        check_fold(Y, zero, "fold one column/zero table");
      }
  }

  // ---- random inputs ----
  for (long it = 0; it < n_random; it++) {
    uint32_t x[5], xa[5], l[5];
    for (int t = 0; t < 5; t++) {
      x[t] = (uint32_t)(rnd() % ((uint64_t)ROUND_MAX[t] + 1));
      xa[t] = (uint32_t)(rnd() % ((uint64_t)ABSORB_MAX[t] + 1));
    }
    check_cube_round(x, "random");
    check_cube_absorb(xa, "random absorb");
    int32_t Y[16];
    const int span = (it & 1) ? YMAX : 3178688;  // the derivation's bound and the MFMA's 2^21.6
    for (int c = 0; c < 16; c++) Y[c] = (int32_t)(rnd() % (2 * (uint64_t)span + 1)) - span;
    u128 v = (((u128)rnd() << 64) | rnd()) % P;
    l[0] = (uint32_t)v & M26, l[1] = (uint32_t)(v >> 26) & M26, l[2] = (uint32_t)(v >> 52) & M26;
    l[3] = (uint32_t)(v >> 78) & M26, l[4] = (uint32_t)(v >> 104);
    check_fold(Y, l, "random fold");
  }

  CHECK(pmt::g_range_fail == 0, "%d columns outside their derived range", pmt::g_range_fail);
  // the 32-bit carries: class 48 = fold columns 0..3 (carry = col >> 26; the same columns pass
  // carry26's own check, class 58), class 40 = fold column 4 (top = col >> 24)
  printf("max carry fold %llu top %llu\n", (unsigned long long)(pmt::g_max[48] >> 26),
         (unsigned long long)(pmt::g_max[40] >> 24));
  CHECK((pmt::g_max[58] >> 26) < ((uint64_t)1 << 32), "a carry does not fit 32 bits");
  CHECK((pmt::g_max[48] >> 26) < ((uint64_t)1 << 22), "fold carry above 2^22");
  CHECK((pmt::g_max[40] >> 24) < ((uint64_t)1 << 16), "fold top above 2^16");
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok pm carry: %ld random inputs\n", n_random);
  return 0;
}
