// Host classifier of one trace column (DESIGN.md §4 "Column structure"): the class the device
// scan (scan_columns_kernel + decode_column_scan) gives the same column, computed by the host
// threads that stage a host trace while they read it.  Pure host code with no device types (the
// element is any 16-byte pair of 64-bit words), shared by the prover (prover.cpp) and built on its
// own by tests/cpp/col_class_test.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace zkl {

constexpr uint32_t CLASS_COL_GENERAL = 0xFFFFFFFFu;  // kernels.h COL_GENERAL
constexpr uint32_t CLASS_P_MAX = 128;                // kernels.h COL_P_MAX

// 0 = every row zero (or col == nullptr), P = the smallest power-of-two row period, at most
// R = min(CLASS_P_MAX, n) and below n (1 = constant, non-zero), CLASS_COL_GENERAL otherwise.
// The rule is the scan's: a column is structured only if every row i equals row i mod R, which
// holds exactly when every row i >= R equals row i - R; the period and the zero test then show in
// the first R rows alone.  Every row is compared (memcmp stops at the first difference, which in a
// general column comes early).  A period that is not below n makes the column general, as
// plan_structured_lde treats it (lde_period_usable): the exact answer matters, a column wrongly
// called structured gives a wrong proof.
template <class E>
inline uint32_t classify_column(const E* col, size_t n) {
  static_assert(sizeof(E) == 16, "a field element is two 64-bit words with no padding");
  if (!col || n == 0) return 0;
  const size_t R = n < CLASS_P_MAX ? n : CLASS_P_MAX;
  if (n > R && memcmp(col + R, col, (n - R) * sizeof(E)) != 0) return CLASS_COL_GENERAL;
  bool nonzero = false;
  for (size_t t = 0; t < R && !nonzero; t++) nonzero = (col[t].lo | col[t].hi) != 0;
  if (!nonzero) return 0;
  for (size_t P = 1; P < R; P <<= 1)  // period P over the first R rows: row t equals row t - P
    if (memcmp(col + P, col, (R - P) * sizeof(E)) == 0) return (uint32_t)P;
  return R < n ? (uint32_t)R : CLASS_COL_GENERAL;
}

}  // namespace zkl
