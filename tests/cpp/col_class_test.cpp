// Host-only test of the host column classifier (zk-lisp_amd/csrc/col_class.h) on crafted
// columns, and against a restatement of the device scan's bit word (scan_columns_kernel) and its
// decoding (decode_column_scan).  Stand-alone (no device code), so it can be built with
// -fsanitize=address,undefined; tests/test_host_columns_cpu.py does that.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../zk-lisp_amd/csrc/col_class.h"

using namespace zkl;
constexpr uint32_t GEN = CLASS_COL_GENERAL;
struct El {
  uint64_t lo, hi;
};
using Col = std::vector<El>;

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// The scan's word for one column, thread by thread as the kernel forms it: bit 31 = some row
// differs from row i mod R, bit k = the first R rows do not have period 2^k, bit 8 = one of them
// is not zero; then decode_column_scan.  The device reports period R even where R = n; the
// prover's plan treats a period that is not below n as general, and so does the classifier.
static uint32_t scan_restated(const Col& c) {
  const size_t n = c.size();
  const uint32_t R = (uint32_t)(n < 128 ? n : 128);
  uint32_t w = 0;
  for (size_t i = 0; i < n; i++) {
    const El ref = c[i & (R - 1)];
    if (c[i].lo != ref.lo || c[i].hi != ref.hi) w |= 1u << 31;
  }
  for (uint32_t t = 0; t < R; t++) {
    if (c[t].lo | c[t].hi) w |= 1u << 8;
    for (uint32_t k = 0; (1u << k) < R; k++)
      if (t >= (1u << k) && (c[t - (1u << k)].lo != c[t].lo || c[t - (1u << k)].hi != c[t].hi)) w |= 1u << k;
  }
  uint32_t P = GEN;
  if (!(w & (1u << 31))) {
    if (!(w & (1u << 8))) P = 0;
    else {
      P = R;
      for (uint32_t k = 0; (1u << k) < R; k++)
        if (!(w & (1u << k))) { P = 1u << k; break; }
    }
  }
  return (P != 0 && P != GEN && P >= n) ? GEN : P;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// smallest period exactly P: P distinct-looking random values, with entry P / 2 forced apart from
// entry 0 so that no smaller power of two is a period
static Col periodic(size_t n, size_t P) {
  Col base(P);
  for (auto& e : base) e = El{rnd() | 1, rnd()};
  if (P > 1) base[P / 2] = El{base[0].lo + 2, base[0].hi};
  Col c(n);
  for (size_t i = 0; i < n; i++) c[i] = base[i % P];
  return c;
}

static int cases = 0;
static void expect(const Col& c, uint32_t want) {
  // an exact-size heap copy: a read past either end is an error under the address sanitizer
  El* p = (El*)malloc(c.size() * sizeof(El));
  CHECK(p);
  memcpy(p, c.data(), c.size() * sizeof(El));
  const uint32_t got = classify_column(p, c.size());
  free(p);
  if (got != want || scan_restated(c) != want) {
    fprintf(stderr, "case %d (n = %zu): classify %u, scan restated %u, want %u\n", cases, c.size(), got,
            scan_restated(c), want);
    exit(1);
  }
  cases++;
}

int main() {
  for (size_t n : {(size_t)32, (size_t)64, (size_t)128, (size_t)256, (size_t)4096}) {
    const size_t R = n < 128 ? n : 128;
    const Col zero(n, El{0, 0});
    expect(zero, 0);
    CHECK(classify_column((const El*)nullptr, n) == 0);  // NULL: an all-zero column
    {
      Col c = zero;
      c[0] = El{1, 0};
      expect(c, GEN);  // zero except row 0
      c = zero;
      c[n - 1] = El{0, 1};
      expect(c, GEN);  // zero except the last row
    }
    expect(Col(n, El{7, 0}), 1);   // constant, non-zero
    expect(Col(n, El{0, 7}), 1);   // constant in hi alone
    for (size_t P = 2; P <= 128; P <<= 1) {
      if (P > n) break;
      // exact periods; a period that is not below n is general (128 at n = 128, 32 at n = 32)
      const Col c = periodic(n, P);
      expect(c, P < n ? (uint32_t)P : GEN);
      if (P < n) {
        Col d = c;  // periodic everywhere except the last row
        d[n - 1].lo ^= 4;
        expect(d, GEN);
        d = c;  // and except in the hi word of one row in the middle
        d[n / 2 + 1].hi ^= 1ull << 63;
        expect(d, GEN);
      }
    }
    if (n > 128) {  // periodic in rows 0..127 with row 128 different
      for (size_t P : {(size_t)1, (size_t)32, (size_t)128}) {
        Col c = periodic(n, P);
        c[128].lo += 8;
        expect(c, GEN);
      }
    }
    {  // values that differ only in hi: period 2 in hi, constant lo
      Col c(n);
      for (size_t i = 0; i < n; i++) c[i] = El{5, (uint64_t)(i & 1)};
      expect(c, n > 2 ? 2u : GEN);
      // zero lo everywhere, hi set in one row of the first R: not a zero column
      c = zero;
      c[R - 1].hi = 1;
      expect(c, GEN);
      for (size_t i = 0; i < n; i++) c[i] = El{0, (i % R) == R - 1 ? 1ull : 0ull};
      expect(c, R < n ? (uint32_t)R : GEN);
    }
    for (int k = 0; k < 8; k++) {  // random general columns
      Col c(n);
      for (auto& e : c) e = El{rnd(), rnd()};
      expect(c, GEN);
    }
    // random small-alphabet columns: whatever class they have, both statements agree
    for (int k = 0; k < 64; k++) {
      const size_t P = (size_t)1 << (rnd() % 8);
      Col c(n);
      for (size_t i = 0; i < n; i++) c[i] = El{(uint64_t)((i % P) % 3 == 0), 0};
      if (k & 1) c[rnd() % n].lo ^= 1;
      El* p = (El*)malloc(n * sizeof(El));
      CHECK(p);
      memcpy(p, c.data(), n * sizeof(El));
      CHECK(classify_column(p, n) == scan_restated(c));
      free(p);
      cases++;
    }
  }
  printf("col_class_test ok (%d cases)\n", cases);
  return 0;
}
