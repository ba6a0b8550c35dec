// Trace preflight, host side.  The device pass (kernels.hip,
// constraint_eval_*_kernel_rows) is a filter: it names the first row whose alpha-weighted
// transition sum is non-zero.  The exact answer the reference's preflight.rs gives -- the first
// non-zero constraint of that row, in evaluation order, and its value -- is resolved here from
// the two rows with the same air_transition_sum, one call per constraint with alpha = e_i.
#include <string.h>

#include <stdexcept>

#include "air_eval.h"
#include "host_hash.h"
#include "host_proof.h"
#include "kernels.h"
#include "preflight.h"
#include "proof_view.h"

namespace zkl {

void row_selectors(size_t row, fe per[31]) {
  const size_t pos = row % 32;
  for (int k = 0; k < 31; k++) per[k] = fe_zero();
  if (pos == 0) per[0] = fe_one();
  if (pos >= 1 && pos <= 27) per[pos] = fe_one();
  if (pos == 28) per[28] = fe_one();
  if (pos >= 29) per[29] = fe_one();
  if (pos == 31) per[30] = fe_one();
}

std::vector<fe> row_selector_table() {
  std::vector<fe> t(32 * 31);
  for (size_t r = 0; r < 32; r++) row_selectors(r, t.data() + r * 31);
  return t;
}

std::vector<fe> eval_transition_row(const AirInstance& air, size_t row, const fe* cur, const fe* nxt) {
  fe per[31];
  row_selectors(row, per);
  auto c = [&](int i) { return cur[(size_t)i]; };
  auto x = [&](int i) { return nxt[(size_t)i]; };
  const bool pose = air.dev.pose_block != 0, rm = (air.dev.ram_block | air.dev.merkle_block) != 0;
  const int n_tc = air.n_tc;
  std::vector<fe> e((size_t)n_tc, fe_zero()), out((size_t)n_tc);
  for (int i = 0; i < n_tc; i++) {
    e[(size_t)i] = fe_one();
    const fe* a = e.data();
    // p_last = 0: rows below n - 1 only (row n - 1 is the transition exemption)
    if (pose && rm) out[(size_t)i] = air_transition_sum<true, true>(air.dev, c, x, per, fe_zero(), a);
    else if (pose) out[(size_t)i] = air_transition_sum<true, false>(air.dev, c, x, per, fe_zero(), a);
    else if (rm) out[(size_t)i] = air_transition_sum<false, true>(air.dev, c, x, per, fe_zero(), a);
    else out[(size_t)i] = air_transition_sum<false, false>(air.dev, c, x, per, fe_zero(), a);
    e[(size_t)i] = fe_zero();
  }
  return out;
}

std::vector<fe> preflight_alphas(const zkl_air_public_inputs& pi, uint32_t width, size_t n, uint64_t seed, int n_tc) {
  std::vector<fe> el = pi_elements(pi);
  el.push_back(fe{width, 0});
  el.push_back(fe{(uint64_t)n, 0});
  el.push_back(fe{seed & 0xFFFFFFFFull, 0});
  el.push_back(fe{seed >> 32, 0});
  Coin coin{hasher().hash_elements(el.data(), el.size()), 0};
  std::vector<fe> a((size_t)n_tc);
  for (auto& v : a) v = coin.draw();
  return a;
}

void fill_report_row(const AirInstance& air, uint32_t width, const fe* cur, const fe* nxt, zkl_trace_report& rep) {
  const Layout& C = air.dev.cols;
  auto ok = [&](int c) { return c >= 0 && (uint32_t)c < width; };
  rep.pos = rep.row % 32;
  if (ok(C.g_map)) rep.g_map = to_abi(cur[C.g_map]);
  if (ok(C.g_final)) rep.g_final = to_abi(cur[C.g_final]);
  rep.round_gates = 0;
  for (int j = 0; j < 27; j++)
    if (ok(C.g_r_start + j) && fe_eq(cur[C.g_r_start + j], fe_one())) rep.round_gates |= 1u << j;
  // lanes l, r, c0, c1 = Poseidon lanes 0, 1, 10, 11 (preflight.rs:189-200)
  const int lane[4] = {C.lanes_start, C.lanes_start + 1, C.lanes_start + 10, C.lanes_start + 11};
  for (int k = 0; k < 4; k++)
    if (ok(lane[k])) {
      rep.lanes_cur[k] = to_abi(cur[lane[k]]);
      rep.lanes_next[k] = to_abi(nxt[lane[k]]);
    }
  rep.lanes_exp_valid = 0;
  if (rep.kind == 1 && air.dev.pose_block && rep.index < 27 * 12 && ok(C.lanes_start + 11)) {
    // y = MDS s^3 + rc[j] of round j = index / 12 (preflight.rs:204-229)
    const int j = (int)rep.index / 12;
    fe s3[12];
    for (int k = 0; k < 12; k++) s3[k] = fe_cube(cur[C.lanes_start + k]);
    const int want[4] = {0, 1, 10, 11};
    for (int u = 0; u < 4; u++) {
      fe acc = fe_zero();
      for (int k = 0; k < 12; k++) acc = fe_add(acc, fe_mul(air.dev.pose_mds[want[u]][k], s3[k]));
      rep.lanes_exp[u] = to_abi(fe_add(acc, air.dev.pose_rc[j][want[u]]));
    }
    rep.lanes_exp_valid = 1;
  }
  rep.ram_valid = 0;
  if (air.dev.ram_block && ok(C.ram_sorted) && ok(C.ram_gp_sorted)) {
    // RamSnap in its field order (preflight.rs:232-250)
    const fe v[13] = {cur[C.ram_sorted],       cur[C.ram_s_addr],        nxt[C.ram_s_addr],       cur[C.ram_s_clk],
                      nxt[C.ram_s_clk],        cur[C.ram_s_val],         cur[C.ram_s_is_write],   cur[C.ram_s_last_write],
                      nxt[C.ram_s_last_write], cur[C.ram_gp_unsorted],   nxt[C.ram_gp_unsorted],  cur[C.ram_gp_sorted],
                      nxt[C.ram_gp_sorted]};
    for (int k = 0; k < 13; k++) rep.ram[k] = to_abi(v[k]);
    rep.ram_valid = 1;
  }
}

std::string fe_decimal(fe v) {
  unsigned __int128 x = ((unsigned __int128)v.hi << 64) | v.lo;
  if (!x) return "0";
  std::string s;
  while (x) {
    s.insert(s.begin(), (char)('0' + (int)(x % 10)));
    x /= 10;
  }
  return s;
}

std::string report_message(const zkl_trace_report& r) {
  if (r.kind == 1)
    return "preflight: constraint " + std::to_string(r.index) + " non-zero at row " + std::to_string(r.row) + ": " +
           fe_decimal(fe_from(r.value));
  if (r.kind == 2)
    return "preflight: assertion " + std::to_string(r.index) + " (column " + std::to_string(r.column) +
           ") fails at row " + std::to_string(r.row) + ": trace " + fe_decimal(fe_from(r.value)) + ", expected " +
           fe_decimal(fe_from(r.expected));
  return "";
}

}  // namespace zkl

using namespace zkl;

extern "C" int zkl_eval_transition_row(uint32_t width, uint32_t n_rows, const zkl_air_public_inputs* pi, uint32_t row,
                                       const zkl_f128* cur, const zkl_f128* next, zkl_f128* values, uint32_t cap,
                                       uint32_t* n_tc) {
  if (!pi || !cur || !next || !n_tc) return ZKL_E_INVALID;
  *n_tc = 0;
  return guarded_call([&] {
    const size_t n = n_rows;
    if (n < 32 || (n & (n - 1))) throw std::invalid_argument("trace length must be a power of two >= 32");
    if (pi->n_main_slots > ZKL_MAX_MAIN_SLOTS) throw std::invalid_argument("n_main_slots exceeds ZKL_MAX_MAIN_SLOTS");
    if (width == 0 || width > 4096) throw std::invalid_argument("trace width must be in 1..4096");
    if ((size_t)row + 1 >= n) throw std::invalid_argument("row must be below n_rows - 1 (the last row has no transition)");
    AirInstance air;
    const std::string e = build_air(*pi, width, n, air);
    if (!e.empty()) throw std::invalid_argument(e);
    *n_tc = (uint32_t)air.n_tc;
    if (!values) return;
    if (cap < (uint32_t)air.n_tc) throw std::invalid_argument("values buffer smaller than the number of transition constraints");
    std::vector<fe> c(width), x(width);
    for (uint32_t k = 0; k < width; k++) { c[k] = fe_from(cur[k]); x[k] = fe_from(next[k]); }
    const std::vector<fe> v = eval_transition_row(air, row, c.data(), x.data());
    for (size_t k = 0; k < v.size(); k++) values[k] = to_abi(v[k]);
  });
}
