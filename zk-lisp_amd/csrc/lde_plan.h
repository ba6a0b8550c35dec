// Host plan of the structured trace LDE (DESIGN.md §4 "Column structure"): which columns go
// through the transforms (the column map), which take the periodic shortcut, and which slices of
// the coefficient and LDE buffers have to be cleared first.  Pure host code with no device types,
// shared by the prover and the LDE stage entry point (prover.cpp) and built on its own by
// tests/cpp/lde_plan_test.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace zkl {

constexpr uint32_t LDE_COL_GENERAL = 0xFFFFFFFFu;  // kernels.h COL_GENERAL
constexpr uint32_t LDE_P_MAX = 128;                // kernels.h COL_P_MAX

// What a context knows about the column slices of one (coef, lde) buffer pair because it wrote
// them itself; nothing here is derived from what a trace held.  Valid for the buffers and shape
// of the key only, and invalid (coef == nullptr) while a call is queueing writes.
struct ZeroBook {
  enum : uint8_t {
    UNKNOWN = 0,  // anything (a transform wrote the column, or nothing did yet)
    ZERO = 1,     // the whole coef and lde columns are zero
    TAIL = 2,     // coef entries from min(LDE_P_MAX, n) on are zero (a periodic column was written)
  };
  std::vector<uint8_t> known;
  const void* coef = nullptr;
  const void* lde = nullptr;
  size_t n = 0, N = 0, W = 0;

  void forget() { coef = lde = nullptr; }
  // a write of `bytes` bytes at p (bytes = 0: of unknown length) by anyone else: forget the
  // states if it can reach either buffer (elem = bytes per element)
  void wrote(const void* p, size_t bytes, size_t elem) {
    if (!coef || !p) return;
    const char* a = (const char*)p;
    auto hits = [&](const void* buf, size_t len) {
      const char* b = (const char*)buf;
      return bytes == 0 ? (a < b + len) : (a < b + len && b < a + bytes);
    };
    if (hits(coef, W * n * elem) || hits(lde, W * N * elem)) forget();
  }
  // start of a call on these buffers: keeps the states when the key matches, resets them when
  // not; the key stays invalid until commit()
  void begin(const void* coef_, const void* lde_, size_t n_, size_t N_, size_t W_) {
    const bool ok = coef_ && coef == coef_ && lde == lde_ && n == n_ && N == N_ && W == W_ && known.size() == W_;
    if (!ok) known.assign(W_, UNKNOWN);
    forget();
  }
  void all_unknown() { known.assign(known.size(), UNKNOWN); }
  void commit(const void* coef_, const void* lde_, size_t n_, size_t N_, size_t W_) {
    coef = coef_; lde = lde_; n = n_; N = N_; W = W_;
  }
};

struct LdePlan {
  std::vector<uint32_t> general;  // the column map, ascending
  // periodic columns grouped by period (ascending), with their periods; a period that is no
  // power of two, exceeds LDE_P_MAX or is not below n makes the column general
  std::vector<uint32_t> pcols, pper;
  std::vector<uint32_t> nonzero;  // every column that is not all-zero, ascending
  std::vector<uint8_t> zero;      // per column: 1 = all-zero
  // [a, b) column runs whose whole coef and lde slices must be cleared (zero columns not known to
  // be zero), and whose coef tails [min(LDE_P_MAX, n), n) must be (periodic columns after a
  // transform wrote the column)
  std::vector<std::pair<uint32_t, uint32_t>> clear_all, clear_tail;
};

inline bool lde_period_usable(uint32_t P, size_t n) {
  return P != 0 && P != LDE_COL_GENERAL && P <= LDE_P_MAX && (P & (P - 1)) == 0 && (size_t)P < n;
}

// period[c]: 0 = all-zero, P = row period, LDE_COL_GENERAL.  Updates book.known (W entries) to
// the states the planned writes leave.
inline LdePlan plan_structured_lde(const uint32_t* period, uint32_t W, size_t n, ZeroBook& book) {
  LdePlan pl;
  pl.zero.assign(W, 0);
  if (book.known.size() != W) book.known.assign(W, ZeroBook::UNKNOWN);
  std::vector<uint32_t> by_period[8];  // log2 P
  auto extend = [](std::vector<std::pair<uint32_t, uint32_t>>& runs, uint32_t c) {
    if (!runs.empty() && runs.back().second == c) runs.back().second = c + 1;
    else runs.push_back({c, c + 1});
  };
  for (uint32_t c = 0; c < W; c++) {
    const uint32_t P = period[c];
    uint8_t& st = book.known[c];
    if (P == 0) {
      pl.zero[c] = 1;
      if (st != ZeroBook::ZERO) extend(pl.clear_all, c);
      st = ZeroBook::ZERO;
      continue;
    }
    pl.nonzero.push_back(c);
    if (lde_period_usable(P, n)) {
      int lg = 0;
      while ((1u << lg) < P) lg++;
      by_period[lg].push_back(c);
      if (st == ZeroBook::UNKNOWN && n > LDE_P_MAX) extend(pl.clear_tail, c);
      st = ZeroBook::TAIL;
    } else {
      pl.general.push_back(c);
      st = ZeroBook::UNKNOWN;
    }
  }
  for (int lg = 0; lg < 8; lg++)
    for (uint32_t c : by_period[lg]) {
      pl.pcols.push_back(c);
      pl.pper.push_back(1u << lg);
    }
  return pl;
}

}  // namespace zkl
