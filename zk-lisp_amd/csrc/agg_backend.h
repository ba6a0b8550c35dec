// The two halves of the ZlAggAir prover: prove_air<T> in agg.cpp is the
// transcript and serialisation skeleton; a backend supplies the arrays -- the host loops
// (agg.cpp) or the kernels of agg.hip on a context's device.  Both fill the same host-side
// members, so the skeleton opens queries from either without knowing which ran.
#pragma once
#include <memory>
#include <stdexcept>
#include <vector>

#include "../../include/zkl_hip.h"
#include "agg_air.h"
#include "agg_ctx.h"

namespace zkl {

struct AggError : std::invalid_argument { using std::invalid_argument::invalid_argument; };

struct AggShape {
  size_t W, n, B, N, ce, Cc;  // trace width / length, blowup, LDE size, CE domain, composition columns
  fe g, gl;                   // the trace domain generator and g^(n-1)
  fe v_units_total, children_count;  // the two last-row assertion values
};

template <class T>
struct AggBackend {
  AggShape sh{};
  // what the skeleton reads
  std::vector<std::vector<fe>> tpoly;  // trace polynomials (after commit_trace)
  std::vector<T> cco;                  // composition coefficients over the CE coset (after compose)
  // what the openings read (after finish)
  std::vector<std::vector<fe>> lde;    // W x N
  std::vector<std::vector<T>> clde;    // Cc x N
  std::vector<fe> ttree, ctree;        // 2N nodes each, root at [1]
  std::vector<std::vector<T>> layers;  // FRI layer evaluations, layer d of N >> d points
  std::vector<std::vector<fe>> ftrees;
  std::vector<T> ev;                   // the evaluations after the last fold (the remainder's)

  virtual ~AggBackend() = default;
  // 1. interpolate, extend and commit the trace; the root
  virtual fe commit_trace(const std::vector<std::vector<fe>>& trace) = 0;
  // 2.-3. constraint composition over the CE coset, interpolated into cco
  virtual void compose(const std::vector<T>& alpha, const std::vector<T>& beta) = 0;
  // 3. split cco into Cc columns, extend and commit; the root
  virtual fe commit_composition() = 0;
  // 5. DEEP composition: frame = t(z) [W] | t(zg) [W] | H(z) [Cc] | H(zg) [Cc], gam [W + Cc]
  virtual void deep(T z, T zg, const std::vector<T>& frame, const std::vector<T>& gam) = 0;
  // 6. commit the current FRI layer (its root), then fold it by alpha
  virtual fe fri_commit() = 0;
  virtual void fri_fold(T alpha) = 0;
  // everything above is in the host-side members
  virtual void finish() = 0;
  // 7. grinding after finish(): the smallest nonce >= 1 whose merge_with_int(seed, nonce) has at
  // least `bits` trailing zero bits.  false: this backend has no search, the skeleton's host
  // threads run it.
  virtual bool grind(fe seed, uint32_t bits, uint64_t* nonce) {
    (void)seed; (void)bits; (void)nonce;
    return false;
  }
};

template <class T>
std::unique_ptr<AggBackend<T>> make_agg_device_backend(zkl_ctx* ctx);

}  // namespace zkl
