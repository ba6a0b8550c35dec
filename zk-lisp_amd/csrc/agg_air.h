// ZlAggAir and the arithmetic of its proof's field, shared by the host prover / verifier
// (agg.cpp) and the device prover (agg.hip), the way air_eval.h is shared for the segment AIR.
//
// Quadratic extension (winter-math 0.13.1, f128 `ExtensibleField<2>` [WF-recall]): elements
// a + b*phi with phi^2 = phi - 1, mul = [a0 b0 - a1 b1, (a0 + a1)(b0 + b1) - a0 b0], Frobenius
// (a, b) -> (a + b, -b); serialised as two 16-byte base elements.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef __HIP_DEVICE_COMPILE__
#include <stdexcept>
#endif

#include "field.h"

namespace zkl {

struct fe2 {
  fe a, b;
};
__host__ __device__ inline fe2 E(fe a) { return fe2{a, fe_zero()}; }
__host__ __device__ inline fe2 add(fe2 x, fe2 y) { return {fe_add(x.a, y.a), fe_add(x.b, y.b)}; }
__host__ __device__ inline fe2 sub(fe2 x, fe2 y) { return {fe_sub(x.a, y.a), fe_sub(x.b, y.b)}; }
__host__ __device__ inline fe2 mul(fe2 x, fe2 y) {
  const fe z = fe_mul(x.a, y.a);
  return {fe_sub(z, fe_mul(x.b, y.b)), fe_sub(fe_mul(fe_add(x.a, x.b), fe_add(y.a, y.b)), z)};
}
__host__ __device__ inline fe2 mulb(fe2 x, fe s) { return {fe_mul(x.a, s), fe_mul(x.b, s)}; }
// conj / norm, norm = a^2 + a b + b^2.  The host throws on zero; device code cannot, and gets
// zero (fe_inv(0) = 0): a prover only inverts x - z for a drawn z, which is zero with
// probability ~2^-128 per point.
__host__ __device__ inline fe2 inv(fe2 x) {
  const fe nrm = fe_add(fe_add(fe_mul(x.a, x.a), fe_mul(x.a, x.b)), fe_mul(x.b, x.b));
#ifndef __HIP_DEVICE_COMPILE__
  if (fe_is_zero(nrm)) throw std::runtime_error("inversion of zero in the quadratic extension");
#endif
  const fe ni = fe_inv(nrm);
  return {fe_mul(fe_add(x.a, x.b), ni), fe_mul(fe_sub(fe_zero(), x.b), ni)};
}
__host__ __device__ inline bool is_zero(fe2 x) { return fe_is_zero(x.a) && fe_is_zero(x.b); }
// base-field helpers with the same names, so polynomial and AIR code is generic in the field
__host__ __device__ inline fe add(fe x, fe y) { return fe_add(x, y); }
__host__ __device__ inline fe sub(fe x, fe y) { return fe_sub(x, y); }
__host__ __device__ inline fe mulb(fe x, fe s) { return fe_mul(x, s); }
__host__ __device__ inline fe mul(fe x, fe y) { return fe_mul(x, y); }
__host__ __device__ inline fe inv(fe x) { return fe_inv(x); }
__host__ __device__ inline bool is_zero(fe x) { return fe_is_zero(x); }
template <class T> __host__ __device__ inline T lift(fe x);
template <> __host__ __device__ inline fe lift<fe>(fe x) { return x; }
template <> __host__ __device__ inline fe2 lift<fe2>(fe x) { return E(x); }
template <class T> __host__ __device__ inline T zero();
template <> __host__ __device__ inline fe zero<fe>() { return fe_zero(); }
template <> __host__ __device__ inline fe2 zero<fe2>() { return E(fe_zero()); }

// AggColumns::baseline (agg/layout.rs:97-175)
enum AggCol {
  C_OK, C_V0_SUM, C_V1_SUM, C_VNEXT_SUM, C_FRI_V0, C_FRI_V1, C_FRI_VNEXT, C_FRI_ALPHA, C_FRI_X0, C_FRI_X1, C_FRI_Q1,
  C_COMP_SUM, C_ALPHA_DIV_ZM_SUM, C_MAP_L0_SUM, C_FINAL_LLAST_SUM, C_R, C_ALPHA, C_BETA, C_GAMMA, C_SEG_FIRST,
  C_TRACE_ROOT_ERR, C_CONSTRAINT_ROOT_ERR, C_V_UNITS_ACC, C_V_UNITS_CHILD, C_CHILD_COUNT_ACC, C_VM_CHAIN_ERR,
  C_RAM_U_CHAIN_ERR, C_RAM_S_CHAIN_ERR, C_ROM_CHAIN_ERR_0, C_ROM_CHAIN_ERR_1, C_ROM_CHAIN_ERR_2, AGG_W
};

// ZlAggAir (agg/air.rs): 24 transition constraints, 5 assertions
constexpr int AGG_TC = 24;
constexpr int AGG_NA = 5;
struct Deg { int base; bool cycle; };  // cycle: one periodic column of period trace_len
constexpr Deg kAggDegrees[AGG_TC] = {{1, false}, {2, true}, {1, false}, {1, false}, {1, false}, {1, false},
                                     {1, false}, {1, false}, {1, false}, {1, false}, {1, false}, {1, true},
                                     {1, false}, {1, false}, {1, false}, {1, false}, {1, false}, {1, false},
                                     {1, false}, {1, false}, {1, false}, {1, false}, {1, false}, {1, false}};

// evaluate_transition (agg/air.rs:113-274); T = f128 on the trace / CE domain, the proof's
// field E at the out-of-domain point.  c / nx: the current and next row, anything indexed by
// AggCol that yields T (an array, or an accessor that loads a column on use, as the device
// kernel does to keep the two rows out of registers).  agg_transition_to hands constraint k's
// value to out(k, value), k = 0 .. AGG_TC - 1 in order; agg_transition stores them in r.
template <class T, class RowC, class RowN, class Sink>
__host__ __device__ inline __attribute__((always_inline)) void agg_transition_to(const RowC& c, const RowN& nx, T is_last,
                                                                                Sink&& out) {
  const T nl = sub(lift<T>(fe_one()), is_last);
  auto chain = [&](int col) { return mul(nl, sub(nx[col], c[col])); };
  out(0, c[C_OK]);
  out(1, mul(nl, sub(nx[C_V_UNITS_ACC], add(c[C_V_UNITS_ACC], mul(c[C_V_UNITS_CHILD], c[C_SEG_FIRST])))));
  out(2, c[C_TRACE_ROOT_ERR]);
  out(3, c[C_CONSTRAINT_ROOT_ERR]);
  out(4, chain(C_R));
  out(5, chain(C_ALPHA));
  out(6, chain(C_BETA));
  out(7, chain(C_GAMMA));
  out(8, chain(C_V0_SUM));
  out(9, chain(C_V1_SUM));
  out(10, chain(C_VNEXT_SUM));
  out(11, mul(nl, sub(nx[C_CHILD_COUNT_ACC], add(c[C_CHILD_COUNT_ACC], c[C_SEG_FIRST]))));
  const T xd = sub(c[C_FRI_X1], c[C_FRI_X0]);
  out(12, sub(mul(c[C_FRI_VNEXT], xd), sub(mul(c[C_FRI_V1], sub(c[C_FRI_ALPHA], c[C_FRI_X0])),
                                           mul(c[C_FRI_V0], sub(c[C_FRI_ALPHA], c[C_FRI_X1])))));
  out(13, sub(c[C_FRI_VNEXT], c[C_FRI_Q1]));
  out(14, c[C_COMP_SUM]);
  out(15, c[C_ALPHA_DIV_ZM_SUM]);
  out(16, c[C_MAP_L0_SUM]);
  out(17, c[C_FINAL_LLAST_SUM]);
  out(18, c[C_VM_CHAIN_ERR]);
  out(19, c[C_RAM_U_CHAIN_ERR]);
  out(20, c[C_RAM_S_CHAIN_ERR]);
  out(21, c[C_ROM_CHAIN_ERR_0]);
  out(22, c[C_ROM_CHAIN_ERR_1]);
  out(23, c[C_ROM_CHAIN_ERR_2]);
}
template <class T, class RowC, class RowN>
__host__ __device__ inline void agg_transition(const RowC& c, const RowN& nx, T is_last, T r[AGG_TC]) {
  agg_transition_to<T>(c, nx, is_last, [&](int k, T v) { r[k] = v; });
}

// the five assertions (get_assertions, agg/air.rs:276-304) sorted by (step, column): three at
// row 0 with value 0, two at the last row with the public totals
__host__ __device__ inline int agg_assert_col(int a) {
  return a == 0 ? C_OK : (a == 1 || a == 3) ? C_V_UNITS_ACC : C_CHILD_COUNT_ACC;
}
struct AggAssertion { int col; size_t step; fe value; };
inline void agg_assertions(size_t n, fe v_units_total, fe children_count, AggAssertion out[AGG_NA]) {
  for (int a = 0; a < AGG_NA; a++)
    out[a] = {agg_assert_col(a), a < 3 ? 0 : n - 1, a < 3 ? fe_zero() : a == 3 ? v_units_total : children_count};
}

}  // namespace zkl
