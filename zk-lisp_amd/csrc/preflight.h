// Trace preflight, host side: the cycle-32 selector values on the trace domain,
// the exact per-constraint values of one frame (the resolution step after the device filter),
// the check coefficients, and the report the reference's preflight.rs builds from the row.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/zkl_hip.h"
#include "air_host.h"
#include "field.h"

namespace zkl {

// the 31 periodic selector values (p_map, p_r[27], p_final, p_pad, p_pad_last) at trace row
// `row`: 0 or 1 by row mod 32 (vm/air/mod.rs:520-592 evaluated on the trace domain)
void row_selectors(size_t row, fe per[31]);
// 32 x 31 table of them, row-major by row mod 32 (the device pass's `rowper`)
std::vector<fe> row_selector_table();
// c_i of frame (cur, nxt) at trace row `row` < n - 1 for every transition constraint, in the
// reference's evaluation order: one call of air_transition_sum per constraint with alpha = e_i
std::vector<fe> eval_transition_row(const AirInstance& air, size_t row, const fe* cur, const fe* nxt);
// n_tc check coefficients: Coin draws from hash_elements(pi_elements | [width, n, seed_lo, seed_hi])
std::vector<fe> preflight_alphas(const zkl_air_public_inputs& pi, uint32_t width, size_t n, uint64_t seed, int n_tc);
// the row-derived fields of the report (gates, lanes, expected lanes, RAM snapshot); kind, index,
// row and value are already set
void fill_report_row(const AirInstance& air, uint32_t width, const fe* cur, const fe* nxt, zkl_trace_report& rep);
// "preflight: constraint 94 non-zero at row 299: 1" / the assertion form; "" for kind 0
std::string report_message(const zkl_trace_report& rep);
std::string fe_decimal(fe v);

}  // namespace zkl
