// Aggregation proof: what `zk-lisp prove` does after the segment
// proofs exist -- RecursionPublicBuilder::build_public (lib.rs:404-482), RecursionBackend::
// prove (lib.rs:295-344) and RecursionArtifactCodec::encode (lib.rs:486-551) of the
// Winterfell backend:
//   child transcripts      ZlChildTranscript::from_step + verify_child_transcript
//                          (agg/child.rs:159-1023) over the Fiat-Shamir replay (agg/fs.rs:38-245)
//   public inputs          AggAirPublicInputs (agg/pi.rs:20-218)
//   aggregation trace      build_agg_trace_from_transcripts (agg/trace.rs:155-951,996-1685)
//   AIR                    ZlAggAir: 24 transition constraints, 5 assertions, p_last (agg/air.rs)
//   proof                  winterfell 0.13.1 Prover::prove with FieldExtension::Quadratic when
//                          min_security_bits >= 128 (prove.rs:629-719), PoseidonHasher commitments
//   artifact / digest      ZKLRC1 (lib.rs:486-551), recursion_digest_from_agg_pi (prove.rs:585-616)
//
// Where it runs: the aggregation trace has one row per child (>= 8 rows, 64 for BASELINE
// configs[3]).  The ZlAggAir proof (prove_air) is a transcript and serialisation skeleton over a
// backend that supplies the arrays (agg_backend.h): the host loops of this file (zkl_agg_prove,
// a NULL context, or the switch zkl_hip_set_agg_device_prover(0)) or the kernels of agg.hip on
// a context's device (zkl_hip_agg_prove).  The transcript, the AIR pre-check, the out-of-domain
// frame and the grinding search (host threads) stay on the host either way.  The child replays
// before it are ~10^4 permutations per child: their hashing goes through the hash plan of
// proof_view.h, on host threads or on the context's device; DESIGN.md §10 has the measured split.
//
// Quadratic extension: agg_air.h.  RandomCoin::draw::<E> reads the 32 digest bytes as (a, b): the
// PoseidonHasher digest is a value plus 16 zero bytes, so every drawn challenge has b = 0.  The
// arithmetic is nevertheless the full extension field.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zkl_hip.h"
#include "agg_backend.h"
#include "air_host.h"
#include "host_hash.h"
#include "host_proof.h"
#include "proof_view.h"

namespace zkl {

void children_root(const uint8_t suite[32], const uint8_t* digests, const uint8_t* roots, size_t n, uint8_t out[32]);

namespace {

// wall times of the calling thread's last aggregation proof (zkl_agg_last_times)
thread_local double g_agg_ms[6] = {0, 0, 0, 0, 0, 0};
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ------------------------------------------------------------------ quadratic extension (agg_air.h)
void flat(std::vector<fe>& v, fe x) { v.push_back(x); }
void flat(std::vector<fe>& v, fe2 x) { v.push_back(x.a); v.push_back(x.b); }

// ------------------------------------------------------------------ polynomials (small, host)
// in-place radix-2 NTT in natural order over <w_m>; inverse includes 1/m
template <class T>
void ntt(std::vector<T>& a, bool inverse) {
  const size_t m = a.size();
  const int lg = ilog2(m);
  for (size_t i = 0, j = 0; i < m; i++) {
    if (i < j) std::swap(a[i], a[j]);
    size_t bit = m >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j |= bit;
  }
  for (int s = 1; s <= lg; s++) {
    const size_t len = (size_t)1 << s, h = len / 2;
    fe w = root_of_unity((unsigned)s);
    if (inverse) w = fe_inv(w);
    std::vector<fe> tw(h);
    tw[0] = fe_one();
    for (size_t k = 1; k < h; k++) tw[k] = fe_mul(tw[k - 1], w);
    for (size_t i = 0; i < m; i += len)
      for (size_t k = 0; k < h; k++) {
        const T u = a[i + k], v = mulb(a[i + k + h], tw[k]);
        a[i + k] = add(u, v);
        a[i + k + h] = sub(u, v);
      }
  }
  if (inverse) {
    const fe mi = fe_inv(fe{m, 0});
    for (auto& x : a) x = mulb(x, mi);
  }
}
// values over offset * <w_m> -> coefficients
template <class T>
std::vector<T> interpolate(std::vector<T> v, fe offset) {
  ntt(v, true);
  const fe oi = fe_inv(offset);
  fe p = fe_one();
  for (auto& c : v) { c = mulb(c, p); p = fe_mul(p, oi); }
  return v;
}
// coefficients (degree < m) -> values over offset * <w_M>, M >= m
template <class T>
std::vector<T> evaluate(const std::vector<T>& c, size_t M, fe offset) {
  std::vector<T> v(M, zero<T>());
  fe p = fe_one();
  for (size_t k = 0; k < c.size(); k++) { v[k] = mulb(c[k], p); p = fe_mul(p, offset); }
  ntt(v, false);
  return v;
}
fe2 eval_at(const std::vector<fe>& c, fe2 x) {  // Horner, base coefficients at an extension point
  fe2 acc = E(fe_zero());
  for (size_t k = c.size(); k-- > 0;) acc = add(mul(acc, x), E(c[k]));
  return acc;
}
fe2 eval_at(const std::vector<fe2>& c, fe2 x) {
  fe2 acc = E(fe_zero());
  for (size_t k = c.size(); k-- > 0;) acc = add(mul(acc, x), c[k]);
  return acc;
}

// Merkle tree (winter-crypto MerkleTree): nodes[n + i] = leaf i, nodes[i] = merge(2i, 2i+1)
std::vector<fe> merkle(const std::vector<fe>& leaves) {
  const size_t n = leaves.size();
  std::vector<fe> t(2 * n);
  for (size_t i = 0; i < n; i++) t[n + i] = leaves[i];
  for (size_t i = n; i-- > 1;) t[i] = hasher().merge(t[2 * i], t[2 * i + 1]);
  return t;
}
// the BatchMerkleProof of leaves idx of such a tree
void multiproof(ProofWriter& w, const std::vector<fe>& tree, size_t n_leaves, const std::vector<size_t>& idx) {
  Plan plan;
  batch_plan_into(n_leaves, idx.data(), idx.size(), plan);
  w.multiproof(plan, ilog2(n_leaves), [&](size_t i) { return tree[plan.node[i]]; });
}

// ------------------------------------------------------------------ public inputs (agg/pi.rs)
struct AggPi {
  uint8_t program_id[32], program_commitment[32], pi_digest[32], children_root[32], batch_id[32];
  uint64_t v_units_total = 0;
  uint32_t children_count = 0;
  // AggProfileMeta
  uint32_t m = 0, pi_len = 0;
  uint16_t rho = 0, q = 0, o = 0, lambda = 0;
  uint64_t v_units = 0;
  // AggFriProfile
  uint32_t lde_blowup = 0;
  uint8_t folding_factor = 2, redundancy = 1, num_layers = 1;
  // AggQueryProfile
  uint16_t num_queries = 0;
  uint32_t grinding_factor = 0;
  uint8_t suite_id[32];
  std::vector<uint32_t> children_ms;
  uint8_t vm_state_initial[32], vm_state_final[32];
  uint8_t ram_u_initial[32], ram_u_final[32], ram_s_initial[32], ram_s_final[32];
  uint8_t rom_initial[3][32], rom_final[3][32];
};

// AggAirPublicInputs::to_elements (agg/pi.rs:174-218)
std::vector<fe> agg_pi_elements(const AggPi& p) {
  std::vector<fe> o;
  o.push_back(fold_bytes32(p.program_id));
  o.push_back(fold_bytes32(p.program_commitment));
  o.push_back(fold_bytes32(p.pi_digest));
  o.push_back(fold_bytes32(p.children_root));
  o.push_back(fold_bytes32(p.batch_id));
  for (uint64_t v : {(uint64_t)p.m, (uint64_t)p.rho, (uint64_t)p.q, (uint64_t)p.o, (uint64_t)p.lambda, (uint64_t)p.pi_len,
                     p.v_units, (uint64_t)p.lde_blowup, (uint64_t)p.folding_factor, (uint64_t)p.redundancy,
                     (uint64_t)p.num_layers, (uint64_t)p.num_queries, (uint64_t)p.grinding_factor,
                     (uint64_t)p.children_count, p.v_units_total})
    o.push_back(fe{v, 0});
  for (const uint8_t* b : {p.vm_state_initial, p.vm_state_final, p.ram_u_initial, p.ram_u_final, p.ram_s_initial,
                           p.ram_s_final})
    o.push_back(fold_bytes32(b));
  for (int i = 0; i < 3; i++) o.push_back(fold_bytes32(p.rom_initial[i]));
  for (int i = 0; i < 3; i++) o.push_back(fold_bytes32(p.rom_final[i]));
  return o;
}

// zk_lisp_proof::pi::PublicInputs::digest (pi.rs:113-147) over the fields a step proof carries
void pi_digest(const StepDecoded& s, uint8_t out[32]) {
  Bytes b;
  b.raw("zkl/pi/v1", 9);
  b.raw(s.program_id, 32);
  b.raw(s.program_commitment, 32);
  b.raw(s.merkle_root, 32);
  b.u64(s.feature_mask);
  b.u32((uint32_t)s.main_args.size());
  for (const zkl_vm_arg& a : s.main_args) {
    b.u8((uint8_t)a.tag);
    b.raw(a.bytes, a.tag == 0 ? 8 : a.tag == 1 ? 16 : 32);
  }
  blake3_hash(b.v.data(), b.v.size(), out);
}

// RecursionPublicBuilder::build_public (lib.rs:404-482); the caller's PublicInputs are the
// ones every step carries (the builder requires all steps to share them)
AggPi build_public(const std::vector<StepDecoded>& steps) {
  if (steps.empty()) throw AggError("build_recursion_public requires at least one step");
  const StepDecoded& f = steps.front();
  for (const StepDecoded& s : steps) {
    bool same = !memcmp(s.program_id, f.program_id, 32) && !memcmp(s.program_commitment, f.program_commitment, 32) &&
                s.main_args.size() == f.main_args.size();
    for (size_t i = 0; same && i < s.main_args.size(); i++)
      same = s.main_args[i].tag == f.main_args[i].tag && !memcmp(s.main_args[i].bytes, f.main_args[i].bytes, 32);
    if (!same)
      throw AggError(
          "build_recursion_public requires all steps to share the same program_id, program_commitment and main_args "
          "as recursion public inputs");
  }
  AggPi p;
  memcpy(p.program_id, f.program_id, 32);
  memcpy(p.program_commitment, f.program_commitment, 32);
  pi_digest(f, p.pi_digest);
  std::vector<uint8_t> dg, rt;
  for (const StepDecoded& s : steps) {
    p.v_units_total = p.v_units_total + s.v_units < p.v_units_total ? ~0ull : p.v_units_total + s.v_units;
    dg.insert(dg.end(), s.digest, s.digest + 32);
    rt.insert(rt.end(), s.root_trace, s.root_trace + 32);
    p.children_ms.push_back(s.m);
  }
  children_root(f.suite, dg.data(), rt.data(), steps.size(), p.children_root);
  memset(p.batch_id, 0, 32);
  p.children_count = (uint32_t)steps.size();
  p.m = f.m; p.rho = f.rho; p.q = f.q; p.o = f.o; p.lambda = f.lambda; p.pi_len = f.pi_len; p.v_units = f.v_units;
  p.lde_blowup = f.rho; p.folding_factor = 2; p.redundancy = 1; p.num_layers = 1;
  p.num_queries = f.q; p.grinding_factor = 0;
  memcpy(p.suite_id, f.suite, 32);
  const StepDecoded& l = steps.back();
  memcpy(p.vm_state_initial, f.bnd[0], 32);
  memcpy(p.vm_state_final, l.bnd[1], 32);
  memcpy(p.ram_u_initial, f.bnd[2], 32);
  memcpy(p.ram_u_final, l.bnd[3], 32);
  memcpy(p.ram_s_initial, f.bnd[4], 32);
  memcpy(p.ram_s_final, l.bnd[5], 32);
  for (int i = 0; i < 3; i++) {
    memcpy(p.rom_initial[i], f.bnd[6 + i], 32);
    memcpy(p.rom_final[i], l.bnd[9 + i], 32);
  }
  return p;
}

// recursion_digest_from_agg_pi (prove.rs:585-616)
void recursion_digest(const AggPi& p, uint8_t out[32]) {
  Bytes b;
  b.raw("zkl/recursion/agg", 17);
  b.raw(p.suite_id, 32);
  b.raw(p.batch_id, 32);
  b.raw(p.children_root, 32);
  b.u32(p.children_count);
  b.u64(p.v_units_total);
  b.u32(p.m); b.u16(p.rho); b.u16(p.q); b.u16(p.o); b.u16(p.lambda); b.u32(p.pi_len); b.u64(p.v_units);
  b.u32(p.lde_blowup); b.u8(p.folding_factor); b.u8(p.redundancy); b.u8(p.num_layers);
  b.u16(p.num_queries); b.u32(p.grinding_factor);
  blake3_hash(b.v.data(), b.v.size(), out);
}

// RecursionArtifactCodec::encode (lib.rs:486-551)
std::vector<uint8_t> encode_artifact(const AggPi& p, const std::vector<uint8_t>& proof) {
  Bytes b;
  b.raw("ZKLRC1", 6);
  b.raw(p.program_id, 32);
  b.raw(p.program_commitment, 32);
  b.raw(p.pi_digest, 32);
  b.raw(p.children_root, 32);
  b.raw(p.batch_id, 32);
  b.u64(p.v_units_total);
  b.u32(p.children_count);
  b.u32(p.m); b.u16(p.rho); b.u16(p.q); b.u16(p.o); b.u16(p.lambda); b.u32(p.pi_len); b.u64(p.v_units);
  b.u32(p.lde_blowup); b.u8(p.folding_factor); b.u8(p.redundancy); b.u8(p.num_layers);
  b.u16(p.num_queries); b.u32(p.grinding_factor);
  b.raw(p.suite_id, 32);
  b.u32((uint32_t)p.children_ms.size());
  for (uint32_t m : p.children_ms) b.u32(m);
  for (const uint8_t* x : {p.vm_state_initial, p.vm_state_final, p.ram_u_initial, p.ram_u_final, p.ram_s_initial,
                           p.ram_s_final})
    b.raw(x, 32);
  for (int i = 0; i < 3; i++) b.raw(p.rom_initial[i], 32);
  for (int i = 0; i < 3; i++) b.raw(p.rom_final[i], 32);
  b.u32((uint32_t)proof.size());
  b.raw(proof.data(), proof.size());
  return b.v;
}

// ------------------------------------------------------------------ child transcripts
struct Child {
  StepDecoded step;
  SegmentView v;  // parsed and replayed inner proof (agg/child.rs:597-848 + agg/fs.rs:38-245)
};

// AirPublicInputs as replay_fs_from_step rebuilds them (agg/fs.rs:44-65): the step's core
// public inputs, segment_feature_mask 0, boundary values from the zl1 public inputs
zkl_air_public_inputs replay_pi(const StepDecoded& s) {
  zkl_air_public_inputs pi{};
  memcpy(pi.program_id, s.program_id, 32);
  memcpy(pi.program_commitment, s.program_commitment, 32);
  memcpy(pi.merkle_root, s.merkle_root, 32);
  pi.feature_mask = s.feature_mask;
  pi.segment_feature_mask = 0;
  uint32_t k = 0;
  auto slot = [&](fe v) {
    if (k >= ZKL_MAX_MAIN_SLOTS) throw AggError("main_args exceed the supported slot count");
    pi.main_slots[k++] = to_abi(v);
  };
  for (const zkl_vm_arg& a : s.main_args) {  // encode_vmarg_to_elements (utils.rs:79-97)
    if (a.tag == 0) { uint64_t x; memcpy(&x, a.bytes, 8); slot(fe{x, 0}); }
    else if (a.tag == 1) slot(be_from_le16(a.bytes));
    else { slot(be_from_le16(a.bytes)); slot(be_from_le16(a.bytes + 16)); }
  }
  pi.n_main_slots = k;
  for (int i = 0; i < 3; i++) pi.rom_acc[i] = to_abi(s.rom_acc[i]);
  pi.pc_init = to_abi(be_from_le16(s.pc_init));
  pi.ram_gp_unsorted_in = to_abi(be_from_le16(s.bnd[2]));
  pi.ram_gp_unsorted_out = to_abi(be_from_le16(s.bnd[3]));
  pi.ram_gp_sorted_in = to_abi(be_from_le16(s.bnd[4]));
  pi.ram_gp_sorted_out = to_abi(be_from_le16(s.bnd[5]));
  for (int i = 0; i < 3; i++) {
    pi.rom_s_in[i] = to_abi(be_from_le16(s.bnd[6 + i]));
    pi.rom_s_out[i] = to_abi(be_from_le16(s.bnd[9 + i]));
  }
  pi.vm_usage_mask = s.vm_usage_mask;
  pi.ram_delta_clk_bits = s.ram_delta_clk_bits;
  return pi;
}

// ------------------------------------------------------------------ aggregation trace
// AggColumns::baseline: the AggCol enum of agg_air.h
constexpr size_t MIN_AGG_TRACE_ROWS = 8;

// (x1 - x0) vnext == v1 (alpha - x0) - v0 (alpha - x1) at the coset of folded position y of a
// layer of size `size` (constant domain offset, agg/trace.rs:759-821)
fe fri_fold_at(fe v0, fe v1, fe alpha, size_t y, size_t size, fe* x0o = nullptr, fe* x1o = nullptr) {
  const fe xe = fe_mul(fe_pow64(root_of_unity((unsigned)ilog2(size)), y), fe{3, 0});
  const fe x0 = xe, x1 = fe_sub(fe_zero(), xe);
  if (x0o) *x0o = x0;
  if (x1o) *x1o = x1;
  const fe num = fe_sub(fe_mul(v1, fe_sub(alpha, x0)), fe_mul(v0, fe_sub(alpha, x1)));
  return fe_mul(num, fe_inv(fe_sub(x1, x0)));
}
// the value layer d holds at the k-th position of the layer before it (of the query positions
// for d = 0; get_query_values geometry)
fe layer_value(const SegmentView& v, int d, size_t k) {
  const size_t p = d ? v.fri_folds[d - 1].pos[k] : v.positions[k], h = (v.lde >> d) / 2;
  return v.fri_values[d][2 * v.fri_folds[d].slot[k] + (p / h)];
}

// FS weights of the aggregation trace (agg/trace.rs:95-125)
struct Weights { fe beta_deep, beta_fri_layer1, delta_depth, beta_paths; };
Weights agg_weights(const AggPi& p) {
  std::vector<fe> s = agg_pi_elements(p);
  s.push_back(fe{0xA9, 0});
  Coin c{hasher().hash_elements(s.data(), s.size()), 0};
  Weights w;
  w.beta_deep = c.draw();
  w.beta_fri_layer1 = c.draw();
  w.delta_depth = c.draw();
  w.beta_paths = c.draw();
  return w;
}

// compute_deep_agg_over_queries (agg/trace.rs:1126-1257)
fe deep_value(const SegmentView& v, size_t k) {
  const size_t W = v.width, Cc = (size_t)v.comp_cols, N = v.lde;
  const fe x = fe_mul(fe_pow64(root_of_unity((unsigned)ilog2(N)), v.positions[k]), fe{3, 0});
  const fe zg = fe_mul(v.z, root_of_unity((unsigned)ilog2(v.n)));
  const fe iz = fe_inv(fe_sub(x, v.z)), izg = fe_inv(fe_sub(x, zg));
  fe y = fe_zero();
  for (size_t i = 0; i < W; i++) {
    const fe t = v.trace_rows[k * W + i];
    y = fe_add(y, fe_mul(v.deep_coeffs[i], fe_add(fe_mul(fe_sub(t, v.ood_trace_z[i]), iz),
                                                  fe_mul(fe_sub(t, v.ood_trace_zg[i]), izg))));
  }
  for (size_t j = 0; j < Cc; j++) {
    const fe c = v.comp_rows[k * Cc + j];
    y = fe_add(y, fe_mul(v.deep_coeffs[W + j], fe_add(fe_mul(fe_sub(c, v.ood_comp_z[j]), iz),
                                                      fe_mul(fe_sub(c, v.ood_comp_zg[j]), izg))));
  }
  return y;
}
// ---- the per-child part of the overlay (trace.rs:187-235, sample_fri_fold_child :1436-1685)
// The four sums of a child's row are weighted by agg_weights(pi), which hashes the public inputs
// of all children; their terms depend on the child alone.  child_terms computes the terms when
// the child arrives (an aggregation session's add), the weigh_* functions apply the weights once
// every child is known.
//
// one query path through every layer and the remainder (compute_fri_path_agg_over_layers,
// agg/trace.rs:697-951; Horner over the reversed coefficients at the constant offset): the
// terms in the order delta^0, delta^1, ... weighs them
std::vector<fe> fri_path_terms(const SegmentView& v, size_t s) {
  const int nl = (int)v.fri_roots.size();
  std::vector<fe> t;
  fe v_rem = fe_zero();
  size_t size = v.lde, pos_rem = 0;
  for (int d = 0; d < nl; d++) {
    const auto& f = v.fri_folds[d].pos;
    if (s >= f.size()) throw AggError("sample index out of bounds for FRI layer");
    const fe vn = fri_fold_at(v.fri_values[d][2 * s], v.fri_values[d][2 * s + 1], v.fri_alphas[d], f[s], size);
    if (d + 1 < nl) {
      t.push_back(fe_sub(vn, layer_value(v, d + 1, s)));
    } else {
      v_rem = vn;
      pos_rem = f[s];
    }
    size /= 2;
  }
  const fe xl = fe_mul(fe{3, 0}, fe_pow64(root_of_unity((unsigned)ilog2(size)), pos_rem));
  fe r = fe_zero();
  for (const fe& c : v.remainder) r = fe_add(fe_mul(r, xl), c);
  t.push_back(fe_sub(v_rem, r));
  return t;
}
struct ChildTerms {
  fe v0{}, v1{}, vn{}, alpha{}, x0{}, x1{}, q1{};  // the layer-0 sample (no weight)
  std::vector<fe> deep;                // compute_deep_agg_over_queries (agg/trace.rs:1126-1257): per query
  std::vector<fe> layer1;              // compute_fri_layer1_agg_over_queries (agg/trace.rs:1261-1432): per query
  std::vector<fe> path0;               // fri_path_terms of sample 0
  std::vector<std::vector<fe>> paths;  // fri_path_terms of every sample all layers hold
  std::exception_ptr err;              // what the overlay of this child throws (met after the batch checks)
};
void child_terms(const SegmentView& v, ChildTerms& o) {
  try {
    const size_t N = v.lde, y0 = v.fri_folds[0].pos[0];
    o.v0 = v.fri_values[0][0];
    o.v1 = v.fri_values[0][1];
    o.alpha = v.fri_alphas[0];
    o.vn = fri_fold_at(o.v0, o.v1, o.alpha, y0, N, &o.x0, &o.x1);
    o.q1 = layer_value(v, 1, 0);
    for (size_t k = 0; k < v.positions.size(); k++)
      o.deep.push_back(fe_sub(deep_value(v, k), layer_value(v, 0, k)));
    const auto& f0 = v.fri_folds[0].pos;
    const size_t nk = std::min(f0.size(), v.positions.size());
    for (size_t k = 0; k < nk; k++) {
      const fe vn = fri_fold_at(v.fri_values[0][2 * k], v.fri_values[0][2 * k + 1], v.fri_alphas[0], f0[k], N);
      o.layer1.push_back(fe_sub(vn, layer_value(v, 1, k)));
    }
    o.path0 = fri_path_terms(v, 0);
    size_t paths = ~(size_t)0;
    for (const auto& f : v.fri_folds) paths = std::min(paths, f.pos.size());
    for (size_t k = 0; k < paths; k++) o.paths.push_back(k ? fri_path_terms(v, k) : o.path0);
  } catch (...) {
    o.err = std::current_exception();
  }
}
// sum_k w^k t[k]
fe weigh(const std::vector<fe>& t, fe w) {
  fe acc = fe_zero(), p = fe_one();
  for (const fe& x : t) {
    acc = fe_add(acc, fe_mul(p, x));
    p = fe_mul(p, w);
  }
  return acc;
}
fe weigh_paths(const std::vector<std::vector<fe>>& paths, fe delta, fe beta) {
  fe acc = fe_zero(), bp = fe_one();
  for (const auto& t : paths) {
    acc = fe_add(acc, fe_mul(bp, weigh(t, delta)));
    bp = fe_mul(bp, beta);
  }
  return acc;
}

// build_agg_trace_from_transcripts (agg/trace.rs:155-693): column-major AGG_W x rows, in one of
// the two trace modes of include/zkl_hip.h (ZKL_AGG_TRACE_VALID / ZKL_AGG_TRACE_REFERENCE)
// tm[i]: child_terms of ch[i]
std::vector<std::vector<fe>> build_agg_trace(const AggPi& p, const std::vector<Child>& ch, const std::vector<ChildTerms>& tm,
                                          uint32_t mode) {
  const size_t nc = ch.size();
  if (nc == 0) throw AggError("AggTrace requires at least one child proof");
  if (p.children_count != nc) throw AggError("AggAirPublicInputs.children_count must match number of children");
  if (p.children_ms.size() != nc) throw AggError("AggAirPublicInputs.children_ms length must match number of children");
  for (const Child& c : ch)
    if (memcmp(c.step.suite, p.suite_id, 32))
      throw AggError("AggAirPublicInputs.suite_id must match suite_id of all children");
  const uint32_t total = ch[0].step.segments_total;
  std::vector<uint32_t> idx;
  for (const Child& c : ch) {
    if (c.step.segments_total != total) throw AggError("AggTrace requires a uniform segments_total across children");
    idx.push_back(c.step.segment_index);
  }
  if (total > 1) {
    if (total != nc) throw AggError("AggTrace requires a complete contiguous segment chain in batch");
    std::sort(idx.begin(), idx.end());
    for (size_t i = 0; i < nc; i++)
      if (idx[i] != i) throw AggError("AggTrace segment indices must form [0..children_count) without gaps");
  }
  for (const Child& c : ch) {
    if (c.step.rho != p.rho || c.step.o != p.o || c.step.lambda != p.lambda || c.step.pi_len != p.pi_len)
      throw AggError("AggAirPublicInputs.profile_meta is inconsistent with child StepMeta");
    if (c.step.q != p.num_queries)
      throw AggError("AggAirPublicInputs.profile_queries.num_queries is inconsistent with child meta.q");
  }
  {
    std::vector<uint8_t> dg, rt;
    for (const Child& c : ch) {
      dg.insert(dg.end(), c.step.digest, c.step.digest + 32);
      rt.insert(rt.end(), c.step.root_trace, c.step.root_trace + 32);
    }
    uint8_t root[32];
    children_root(p.suite_id, dg.data(), rt.data(), nc, root);
    if (memcmp(root, p.children_root, 32))
      throw AggError("AggAirPublicInputs.children_root is inconsistent with child commitments");
  }
  uint64_t vsum = 0;
  for (size_t i = 0; i < nc; i++) {
    if (p.children_ms[i] == 0) throw AggError("AggAirPublicInputs.children_ms entries must be non-zero");
    if (p.children_ms[i] != ch[i].step.m) throw AggError("AggAirPublicInputs.children_ms entry does not match child meta.m");
    if (vsum + ch[i].step.v_units < vsum) throw AggError("AggAirPublicInputs.v_units_total overflow");
    vsum += ch[i].step.v_units;
  }
  if (vsum != p.v_units_total) throw AggError("AggAirPublicInputs.v_units_total must equal sum of child meta.v_units");

  // rows: next_pow2(max(children, 8)) in the reference (agg/trace.rs:396-405).  With a
  // power-of-two child count >= 8 that leaves no padding row, and the last row then holds the
  // last child's accumulators *before* its increment, so the assertions v_units_acc[last] =
  // v_units_total and child_count_acc[last] = children_count (agg/air.rs:276-304) cannot hold
  // and no valid aggregation proof exists.  The valid mode always keeps one padding row
  // (DESIGN.md §10); other child counts give the reference's trace length.
  const bool ref = mode == ZKL_AGG_TRACE_REFERENCE;
  size_t rows = 1;
  while (rows < std::max(ref ? nc : nc + 1, MIN_AGG_TRACE_ROWS)) rows *= 2;
  std::vector<std::vector<fe>> T(AGG_W, std::vector<fe>(rows, fe_zero()));
  const fe vm0 = fold_bytes32(p.vm_state_initial), vm1 = fold_bytes32(p.vm_state_final);
  const fe ru0 = fold_bytes32(p.ram_u_initial), ru1 = fold_bytes32(p.ram_u_final);
  const fe rs0 = fold_bytes32(p.ram_s_initial), rs1 = fold_bytes32(p.ram_s_final);
  const fe ro0 = fold_bytes32(p.rom_initial[0]), ro1 = fold_bytes32(p.rom_final[0]);
  fe v_acc = fe_zero(), cnt = fe_zero(), pvm{}, pru{}, prs{}, pro{};
  const Weights w = agg_weights(p);
  // the per-child FRI / DEEP terms were computed from each child alone (child_terms); a child's
  // error there is met here, after the batch checks above, and the one of the lowest child thrown
  for (size_t i = 0; i < nc; i++)
    if (tm[i].err) std::rethrow_exception(tm[i].err);
  for (size_t i = 0; i < nc; i++) {
    const StepDecoded& s = ch[i].step;
    const fe vm_in = fold_bytes32(s.bnd[0]), vm_out = fold_bytes32(s.bnd[1]);
    const fe ru_in = fold_bytes32(s.bnd[2]), ru_out = fold_bytes32(s.bnd[3]);
    const fe rs_in = fold_bytes32(s.bnd[4]), rs_out = fold_bytes32(s.bnd[5]);
    const fe ro_in = fold_bytes32(s.bnd[6]), ro_out = fold_bytes32(s.bnd[9]);  // lane 0 only (trace.rs:524-541)
    fe vm_err = fe_sub(vm_in, i ? pvm : vm0), ru_err = fe_sub(ru_in, i ? pru : ru0), rs_err = fe_sub(rs_in, i ? prs : rs0);
    fe ro_err = fe_sub(ro_in, i ? pro : ro0);
    if (i + 1 == nc) {
      ro_err = fe_add(ro_err, fe_sub(ro_out, ro1));
      vm_err = fe_add(vm_err, fe_sub(vm_out, vm1));
      ru_err = fe_add(ru_err, fe_sub(ru_out, ru1));
      rs_err = fe_add(rs_err, fe_sub(rs_out, rs1));
    }
    T[C_SEG_FIRST][i] = fe_one();
    T[C_V_UNITS_CHILD][i] = fe{s.v_units, 0};
    T[C_V_UNITS_ACC][i] = v_acc;
    T[C_CHILD_COUNT_ACC][i] = cnt;
    // trace_root_err / constraint_root_err: sum over queries of the root each opening
    // reproduces minus the committed root (agg/trace.rs:553-600).  The valid mode: the replay
    // verified every opening against its root under the library's row-digest rule, so both
    // sums are zero.  The reference mode rebuilds each leaf with
    // hash_row_poseidon (agg/child.rs:1025-1045) and each path from the batch proof with those
    // leaves (into_openings); every path of one batch then ends on the same root, so the sum
    // is num_queries x (that root - the committed root), roots folded by fold_bytes32_to_fe
    // (the digest value itself).
    const fe nq{(uint64_t)ch[i].v.positions.size(), 0};
    T[C_TRACE_ROOT_ERR][i] = ref ? fe_mul(nq, fe_sub(ch[i].v.trace_root_ref, ch[i].v.trace_root)) : fe_zero();
    T[C_CONSTRAINT_ROOT_ERR][i] =
        ref ? fe_mul(nq, fe_sub(ch[i].v.constraint_root_ref, ch[i].v.constraint_root)) : fe_zero();
    T[C_VM_CHAIN_ERR][i] = vm_err;
    T[C_RAM_U_CHAIN_ERR][i] = ru_err;
    T[C_RAM_S_CHAIN_ERR][i] = rs_err;
    T[C_ROM_CHAIN_ERR_0][i] = ro_err;
    const ChildTerms& o = tm[i];
    T[C_FRI_V0][i] = o.v0;
    T[C_FRI_V1][i] = o.v1;
    T[C_FRI_VNEXT][i] = o.vn;
    T[C_FRI_ALPHA][i] = o.alpha;
    T[C_FRI_X0][i] = o.x0;
    T[C_FRI_X1][i] = o.x1;
    T[C_FRI_Q1][i] = o.q1;
    T[C_COMP_SUM][i] = weigh(o.deep, w.beta_deep);
    T[C_ALPHA_DIV_ZM_SUM][i] = weigh(o.layer1, w.beta_fri_layer1);
    T[C_MAP_L0_SUM][i] = weigh(o.path0, w.delta_depth);
    T[C_FINAL_LLAST_SUM][i] = weigh_paths(o.paths, w.delta_depth, w.beta_paths);
    v_acc = fe_add(v_acc, fe{s.v_units, 0});
    cnt = fe_add(cnt, fe_one());
    pvm = vm_out; pru = ru_out; prs = rs_out; pro = ro_out;
  }
  for (size_t r = nc; r < rows; r++) {
    T[C_V_UNITS_ACC][r] = v_acc;
    T[C_CHILD_COUNT_ACC][r] = cnt;
  }
  return T;
}

// ------------------------------------------------------------------ ZlAggAir (agg/air.rs)
// (AGG_TC, kAggDegrees and agg_transition<T>: agg_air.h, shared with the device prover)

struct AggOpts {
  uint32_t queries, blowup, grind, field_ext;
  bool check_air = true;  // reject a trace that violates ZlAggAir (off in ZKL_AGG_TRACE_REFERENCE mode)
};

// The host backend of prove_air (agg_backend.h): serial loops over the host field arithmetic
// and the host Poseidon.
template <class T>
struct AggHostBackend final : AggBackend<T> {
  using AggBackend<T>::sh;
  static constexpr fe off{3, 0};

  fe commit_trace(const std::vector<std::vector<fe>>& trace) override {
    const Hasher& H = hasher();
    const size_t W = sh.W, N = sh.N;
    this->tpoly.resize(W);
    this->lde.resize(W);
    for (size_t c = 0; c < W; c++) {
      this->tpoly[c] = interpolate(trace[c], fe_one());
      this->lde[c] = evaluate(this->tpoly[c], N, off);
    }
    // one partition (below 2^14 rows): partition_size == width and a row digest is hash_elements(row)
    std::vector<fe> leaves(N), row(W);
    for (size_t i = 0; i < N; i++) {
      for (size_t c = 0; c < W; c++) row[c] = this->lde[c][i];
      leaves[i] = H.hash_elements(row.data(), W);
    }
    this->ttree = merkle(leaves);
    return this->ttree[1];
  }

  void compose(const std::vector<T>& alpha, const std::vector<T>& beta) override {
    const size_t W = sh.W, n = sh.n, N = sh.N, B = sh.B, ce = sh.ce;
    const auto& lde = this->lde;
    AggAssertion asr[AGG_NA];
    agg_assertions(n, sh.v_units_total, sh.children_count, asr);
    std::vector<T> cev(ce);
    const fe wce = root_of_unity((unsigned)ilog2(ce)), g = sh.g, gl = sh.gl;
    fe x = off;
    const size_t step = N / ce;
    std::vector<fe> cur(W), nxt(W);
    fe tc[AGG_TC];
    for (size_t i = 0; i < ce; i++, x = fe_mul(x, wce)) {
      for (size_t c = 0; c < W; c++) {
        cur[c] = lde[c][i * step];
        nxt[c] = lde[c][(i * step + B) % N];
      }
      const fe xn = fe_pow64(x, n), xg = fe_sub(x, gl);
      const fe p_last = fe_mul(fe_mul(gl, fe_sub(xn, fe_one())), fe_inv(fe_mul(fe{n, 0}, xg)));
      agg_transition<fe>(cur.data(), nxt.data(), p_last, tc);
      T t = zero<T>();
      for (int k = 0; k < AGG_TC; k++) t = add(t, mulb(alpha[k], tc[k]));
      t = mulb(t, fe_mul(xg, fe_inv(fe_sub(xn, fe_one()))));
      for (int a = 0; a < AGG_NA; a++)
        t = add(t, mulb(beta[a], fe_mul(fe_sub(cur[asr[a].col], asr[a].value), fe_inv(fe_sub(x, fe_pow64(g, asr[a].step))))));
      cev[i] = t;
    }
    this->cco = interpolate(cev, off);
  }

  fe commit_composition() override {
    const Hasher& H = hasher();
    const size_t n = sh.n, N = sh.N, Cc = sh.Cc;
    this->clde.resize(Cc);
    for (size_t j = 0; j < Cc; j++) {
      const std::vector<T> hp(this->cco.begin() + (long)(j * n), this->cco.begin() + (long)((j + 1) * n));
      this->clde[j] = evaluate(hp, N, off);
    }
    std::vector<fe> cleaves(N), row;
    for (size_t i = 0; i < N; i++) {
      row.clear();
      for (size_t j = 0; j < Cc; j++) flat(row, this->clde[j][i]);
      cleaves[i] = H.hash_elements(row.data(), row.size());  // one partition: the whole row
    }
    this->ctree = merkle(cleaves);
    return this->ctree[1];
  }

  void deep(T z, T zg, const std::vector<T>& frame, const std::vector<T>& gam) override {
    const size_t W = sh.W, N = sh.N, Cc = sh.Cc;
    const T *tz = frame.data(), *tzg = tz + W, *hz = tzg + W, *hzg = hz + Cc;
    this->ev.resize(N);
    const fe wN = root_of_unity((unsigned)ilog2(N));
    fe x = off;
    for (size_t i = 0; i < N; i++, x = fe_mul(x, wN)) {
      const T iz = inv(sub(lift<T>(x), z)), izg = inv(sub(lift<T>(x), zg));
      T y = zero<T>();
      for (size_t c = 0; c < W; c++) {
        const T t = lift<T>(this->lde[c][i]);
        y = add(y, mul(gam[c], add(mul(sub(t, tz[c]), iz), mul(sub(t, tzg[c]), izg))));
      }
      for (size_t j = 0; j < Cc; j++) {
        const T hv = this->clde[j][i];
        y = add(y, mul(gam[W + j], add(mul(sub(hv, hz[j]), iz), mul(sub(hv, hzg[j]), izg))));
      }
      this->ev[i] = y;
    }
  }

  fe fri_commit() override {
    const Hasher& H = hasher();
    const auto& ev = this->ev;
    const size_t h = ev.size() / 2;
    std::vector<fe> lf(h), row;
    for (size_t i = 0; i < h; i++) {
      row.clear();
      flat(row, ev[i]);
      flat(row, ev[i + h]);
      lf[i] = H.hash_elements(row.data(), row.size());
    }
    this->ftrees.push_back(merkle(lf));
    return this->ftrees.back()[1];
  }

  void fri_fold(T a) override {
    auto& ev = this->ev;
    const size_t Nd = ev.size(), h = Nd / 2;
    const fe wd = root_of_unity((unsigned)ilog2(Nd));
    std::vector<T> nx(h);
    fe xe = off;
    for (size_t i = 0; i < h; i++, xe = fe_mul(xe, wd)) {
      const fe x0 = xe, x1 = fe_sub(fe_zero(), xe);
      // (v1 (a - x0) - v0 (a - x1)) / (x1 - x0)
      const T num = sub(mul(ev[i + h], sub(a, lift<T>(x0))), mul(ev[i], sub(a, lift<T>(x1))));
      nx[i] = mulb(num, fe_inv(fe_sub(x1, x0)));
    }
    this->layers.push_back(std::move(ev));
    ev = std::move(nx);
  }

  void finish() override {}
};

// winterfell 0.13.1 Prover::prove for ZlAggAir over E = QuadExtension<f128> (or E = f128 when
// the security target is below 128 bits: FieldExtension::None, prove.rs:647-651).  This is the
// transcript and serialisation skeleton; the arrays come from a backend (agg_backend.h): the
// host loops above (ctx == nullptr) or the kernels of agg.hip on ctx's device.
template <class T>
std::vector<uint8_t> prove_air(const std::vector<std::vector<fe>>& trace, const std::vector<fe>& pi_el,
                               uint64_t v_units_total, uint32_t children_count, const AggOpts& ao, zkl_ctx* ctx,
                               double* grind_ms) {
  const Hasher& H = hasher();
  const size_t W = trace.size(), n = trace[0].size();
  const int logn = ilog2(n);
  const size_t B = ao.blowup, N = n * B;
  if (B < 2 || (B & (B - 1)) || B > 128) throw AggError("aggregation blowup must be a power of two in [2, 128]");
  zkl_proof_options o{};
  o.num_queries = ao.queries;
  o.blowup_factor = ao.blowup;
  o.grinding_factor = ao.grind;
  o.field_extension = ao.field_ext;
  o.fri_folding_factor = 2;
  o.fri_remainder_max_degree = 1;
  o.batching_constraints = 0;
  o.batching_deep = 0;
  zkl_select_partitions((uint32_t)W, (uint32_t)n, &o.num_partitions, &o.hash_rate);
  // RandomCoin::draw::<E>: the 32 digest bytes as (a, b), b = the digest's zero upper half
  auto draw = [](Coin& c) -> T { return lift<T>(c.draw()); };

  // AirContext: evaluation degrees, CE blowup, composition columns (winter-air [WF-recall])
  size_t max_eval = 0, ceb = 2;
  for (const Deg& d : kAggDegrees) {
    max_eval = std::max(max_eval, (size_t)d.base * (n - 1) + (d.cycle ? n - 1 : 0));
    size_t mb = 1;
    while (mb < (size_t)(d.base + (d.cycle ? 1 : 0) - 1)) mb *= 2;
    ceb = std::max(ceb, mb);
  }
  if (B < ceb) throw AggError("aggregation blowup below the constraint-evaluation blowup");
  const size_t Cc = std::max<size_t>(1, (max_eval - (n - 1) + n - 1) / n);
  const size_t ce = n * ceb;
  const fe off{3, 0}, g = root_of_unity((unsigned)logn), gl = fe_pow64(g, n - 1);

  std::vector<fe> seed = context_elements((uint32_t)W, n, o);
  seed.insert(seed.end(), pi_el.begin(), pi_el.end());
  Coin coin{H.hash_elements(seed.data(), seed.size()), 0};

  // 0. the trace must satisfy the AIR (winterfell validates this in debug builds; the
  // composition degree bound C n equals the CE domain here, so a violated constraint would
  // otherwise only surface as a proof the verifier rejects).  The reference-trace mode proves
  // whatever trace the reference builds, as its release prover does.
  if (ao.check_air) {
    std::vector<fe> cur(W), nxt(W);
    fe tc[AGG_TC];
    for (size_t i = 0; i + 1 < n; i++) {  // one transition exemption: the last row is not checked
      for (size_t c = 0; c < W; c++) { cur[c] = trace[c][i]; nxt[c] = trace[c][i + 1]; }
      agg_transition<fe>(cur.data(), nxt.data(), i == n - 1 ? fe_one() : fe_zero(), tc);
      for (int k = 0; k < AGG_TC; k++)
        if (!fe_is_zero(tc[k]))
          throw AggError("aggregation trace does not satisfy ZlAggAir: transition constraint C" + std::to_string(k) +
                         " fails at row " + std::to_string(i));
    }
    AggAssertion asr[AGG_NA];
    agg_assertions(n, fe{v_units_total, 0}, fe{children_count, 0}, asr);
    for (const AggAssertion& a : asr)
      if (!fe_eq(trace[a.col][a.step], a.value)) throw AggError("aggregation trace does not satisfy ZlAggAir: an assertion fails");
  }
  // select_partitions_for_trace gives one partition below 2^14 rows (a batch of <= 2^13
  // children); both backends hash a row whole
  if (o.num_partitions != 1) throw AggError("aggregation traces of 2^14 rows or more are not supported");

  // the arrays: host loops, or the context's device (nothing above launched anything)
  std::unique_ptr<AggBackend<T>> be_p;
  if (ctx) be_p = make_agg_device_backend<T>(ctx);
  else be_p.reset(new AggHostBackend<T>());
  AggBackend<T>& be = *be_p;
  be.sh = AggShape{W, n, B, N, ce, Cc, g, gl, fe{v_units_total, 0}, fe{children_count, 0}};

  // 1. trace LDE + commitment (rows hashed whole: one partition)
  const fe troot = be.commit_trace(trace);
  coin.reseed(troot);

  // 2. constraint composition coefficients, evaluation over the CE coset
  std::vector<T> alpha(AGG_TC), beta(AGG_NA);
  for (auto& a : alpha) a = draw(coin);
  for (auto& b : beta) b = draw(coin);
  be.compose(alpha, beta);
  // 3. composition polynomial: degree check, column split, LDE, commitment
  const std::vector<T>& cco = be.cco;
  for (size_t k = Cc * n; k < ce; k++)
    if (!is_zero(cco[k])) throw AggError("aggregation trace does not satisfy ZlAggAir (composition degree too large)");
  const fe croot = be.commit_composition();
  coin.reseed(croot);

  // 4. out-of-domain frame: Horner on the host over the coefficients (31 + Cc polynomials of
  // n coefficients at two points; the device backend copies them back)
  const std::vector<std::vector<fe>>& tpoly = be.tpoly;
  const T z = draw(coin);
  fe2 z2, zg2;
  if constexpr (sizeof(T) == sizeof(fe2)) z2 = z; else z2 = E(z);
  zg2 = mul(z2, E(g));
  std::vector<fe2> tz(W), tzg(W), hz(Cc), hzg(Cc);
  for (size_t c = 0; c < W; c++) { tz[c] = eval_at(tpoly[c], z2); tzg[c] = eval_at(tpoly[c], zg2); }
  for (size_t j = 0; j < Cc; j++) {
    std::vector<fe2> hp(n);
    for (size_t k = 0; k < n; k++) {
      if constexpr (sizeof(T) == sizeof(fe2)) hp[k] = cco[j * n + k]; else hp[k] = E(cco[j * n + k]);
    }
    hz[j] = eval_at(hp, z2);
    hzg[j] = eval_at(hp, zg2);
  }
  auto as_T = [](fe2 v) -> T {
    if constexpr (sizeof(T) == sizeof(fe2)) return v;
    else return v.a;  // base-field proof: the point is a base element, so are the evaluations
  };
  {
    std::vector<fe> oc;  // trace(z) | H(z) | trace(zg) | H(zg)  (agg/fs.rs:152-164)
    for (auto& v : tz) flat(oc, as_T(v));
    for (auto& v : hz) flat(oc, as_T(v));
    for (auto& v : tzg) flat(oc, as_T(v));
    for (auto& v : hzg) flat(oc, as_T(v));
    coin.reseed(H.hash_elements(oc.data(), oc.size()));
  }
  // 5. DEEP composition over the LDE domain
  std::vector<T> gam(W + Cc);
  for (auto& c : gam) c = draw(coin);
  std::vector<T> frame;  // t(z) | t(zg) | H(z) | H(zg)
  for (auto& v : tz) frame.push_back(as_T(v));
  for (auto& v : tzg) frame.push_back(as_T(v));
  for (auto& v : hz) frame.push_back(as_T(v));
  for (auto& v : hzg) frame.push_back(as_T(v));
  be.deep(as_T(z2), as_T(zg2), frame, gam);
  // 6. FRI (folding 2, constant domain offset, remainder degree 1)
  const int nl = fri_num_layers(N, B, o.fri_remainder_max_degree);
  std::vector<fe> fri_roots;
  for (int d = 0; d < nl; d++) {
    fri_roots.push_back(be.fri_commit());
    coin.reseed(fri_roots.back());
    be.fri_fold(draw(coin));
  }
  be.finish();
  const std::vector<std::vector<fe>>& lde = be.lde;
  const std::vector<std::vector<T>>& clde = be.clde;
  const std::vector<fe>&ttree = be.ttree, &ctree = be.ctree;
  const std::vector<std::vector<T>>& layers = be.layers;
  const std::vector<std::vector<fe>>& ftrees = be.ftrees;
  const std::vector<T>& ev = be.ev;
  std::vector<T> rco = interpolate(ev, off);
  const size_t rlen = o.fri_remainder_max_degree + 1;
  for (size_t k = rlen; k < rco.size(); k++)
    if (!is_zero(rco[k])) throw AggError("FRI remainder degree exceeds the remainder bound");
  std::vector<T> rem(rlen);
  for (size_t k = 0; k < rlen; k++) rem[k] = rco[rlen - 1 - k];
  fe rem_commit;
  {
    std::vector<fe> rf;
    for (auto& v : rem) flat(rf, v);
    rem_commit = H.hash_elements(rf.data(), rf.size());
  }
  coin.reseed(rem_commit);

  // 7. grinding: smallest nonce >= 1 (winterfell without `concurrent` searches sequentially, so
  // the minimum is what it finds): the backend's search (the device backend's ascending windows
  // on the context's stream), else host threads
  uint64_t nonce = 1;
  const auto t_grind = std::chrono::steady_clock::now();
  if (ao.grind > 0 && !be.grind(coin.seed, ao.grind, &nonce)) {
    const fe sd = coin.seed;
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const uint64_t chunk = 4096;
    std::atomic<uint64_t> next{1}, best{~0ull};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
      th.emplace_back([&] {
        for (;;) {
          const uint64_t b0 = next.fetch_add(chunk);
          if (b0 > best.load()) return;
          for (uint64_t x = b0; x < b0 + chunk; x++) {
            const fe d = H.merge_with_int(sd, x);
            const uint32_t tz = d.lo ? (uint32_t)__builtin_ctzll(d.lo) : 64u;
            if (tz >= ao.grind) {
              uint64_t cur = best.load();
              while (x < cur && !best.compare_exchange_weak(cur, x)) {}
              break;
            }
          }
        }
      });
    for (auto& t : th) t.join();
    nonce = best.load();
  }
  if (grind_ms) *grind_ms = ms_since(t_grind);
  // 8. query positions: draw_integers(q, N, nonce), sort, dedup
  std::vector<size_t> pos;
  query_positions(coin, nonce, ao.queries, N, pos);
  const size_t nq = pos.size();

  // 9. Proof::to_bytes (proof_codec.h; an extension element is two base elements)
  Bytes P;
  ProofWriter w{P};
  w.context((uint32_t)W, logn, o, nq);
  w.commitments(ttree[1], ctree[1], fri_roots, rem_commit);
  std::vector<fe> tv;
  std::vector<T> xv;  // a section's values of E
  for (size_t k : pos) for (size_t c = 0; c < W; c++) tv.push_back(lde[c][k]);
  for (size_t k : pos) for (size_t j = 0; j < Cc; j++) xv.push_back(clde[j][k]);
  w.queries();
  w.values(tv.data(), tv.size());
  multiproof(w, ttree, N, pos);
  w.values(xv.data(), xv.size());
  multiproof(w, ctree, N, pos);
  w.ood(frame.data(), frame.data() + W, W, frame.data() + 2 * W, frame.data() + 2 * W + Cc, Cc);
  w.fri_layers(nl);
  FoldStep f;
  for (int d = 0; d < nl; d++) {
    const size_t h = layers[d].size() / 2;
    fold_positions(pos, h, f);
    xv.clear();
    for (size_t y : f.pos) { xv.push_back(layers[d][y]); xv.push_back(layers[d][y + h]); }
    w.values(xv.data(), xv.size());
    multiproof(w, ftrees[d], h, f.pos);
    pos = f.pos;
  }
  w.remainder(rem.data(), rem.size());
  w.finish(nonce);
  return P.v;
}

// ------------------------------------------------------------------ verification
// conjectured security as the reference estimates it (estimate_conjectured_security_bits,
// prove.rs:1177-1195) for the options a proof records
uint32_t conjectured_bits(uint32_t queries, uint32_t blowup, uint32_t grind, uint32_t ext) {
  const uint32_t field = 128 * ext;
  uint32_t qs = (uint32_t)ilog2(blowup) * queries;
  if (qs >= 80) qs += grind;
  return std::min(std::min(field, qs) - 1, 128u);
}

template <class T> bool eq_t(T x, T y);
template <> bool eq_t<fe>(fe x, fe y) { return fe_eq(x, y); }
template <> bool eq_t<fe2>(fe2 x, fe2 y) { return fe_eq(x.a, y.a) && fe_eq(x.b, y.b); }
template <class T> T pow_t(T x, uint64_t e) {
  T r = lift<T>(fe_one());
  for (; e; e >>= 1, x = mul(x, x))
    if (e & 1) r = mul(r, x);
  return r;
}

// winter-verifier 0.13.1 [WF-recall] for a ZlAggAir proof over E = T (verify_agg_proof,
// prove.rs:732-791): transcript replay, out-of-domain identity through the same
// agg_transition, trace / constraint openings, DEEP, FRI folds, remainder, proof of work
template <class T>
std::string verify_air(Rd& r, const AggPi& pi, const ProofContext& cx) {
  const zkl_proof_options& o = cx.opts;
  const uint32_t W = cx.W, logn = cx.logn;
  const Hasher& H = hasher();
  const size_t n = (size_t)1 << logn, B = o.blowup_factor, N = n * B;
  size_t max_eval = 0;
  for (const Deg& d : kAggDegrees) max_eval = std::max(max_eval, (size_t)d.base * (n - 1) + (d.cycle ? n - 1 : 0));
  const size_t Cc = std::max<size_t>(1, (max_eval - (n - 1) + n - 1) / n);
  const int nl = fri_num_layers(N, B, o.fri_remainder_max_degree);
  fe troot, croot, rem_commit;
  std::vector<fe> fri_roots;
  if (const char* e = read_commitments(r, nl, troot, croot, fri_roots, rem_commit)) return e;
  std::vector<fe> seed = context_elements(W, n, o);
  const std::vector<fe> pe = agg_pi_elements(pi);
  seed.insert(seed.end(), pe.begin(), pe.end());
  Coin coin{H.hash_elements(seed.data(), seed.size()), 0};
  auto draw = [&]() -> T { return lift<T>(coin.draw()); };  // draw::<E>: (value, 0)
  coin.reseed(troot);
  std::vector<T> alpha(AGG_TC), beta(AGG_NA);
  for (auto& a : alpha) a = draw();
  for (auto& b : beta) b = draw();
  coin.reseed(croot);
  const T z = draw();
  const fe g = root_of_unity(logn);
  const T zg = mul(z, lift<T>(g));

  QuerySections qs;
  if (const char* e = read_query_sections(r, qs)) return e;
  Rd &tq_v = qs.tq_v, &tq_p = qs.tq_p, &cq_v = qs.cq_v, &cq_p = qs.cq_p, &ood_ts = qs.ood_ts, &ood_es = qs.ood_es;
  const size_t es = sizeof(T) / sizeof(fe) * 16;  // bytes per element of E
  if (ood_ts.len != 2 * W * es || ood_es.len != 2 * Cc * es) return "OOD frame has the wrong shape";
  std::vector<T> tz, tzg, hz, hzg;
  read_values(ood_ts, tz, W);
  read_values(ood_ts, tzg, W);
  read_values(ood_es, hz, Cc);
  read_values(ood_es, hzg, Cc);
  if (ood_ts.bad || ood_es.bad) return "non-canonical OOD values";
  {  // H(z) = sum_j H_j(z) z^(j n) against the transition and boundary compositions at z
    const T zn = pow_t(z, n), gl = lift<T>(fe_pow64(g, n - 1));
    const T p_last = mul(mul(gl, sub(zn, lift<T>(fe_one()))), inv(mul(lift<T>(fe{n, 0}), sub(z, gl))));
    T tc[AGG_TC];
    agg_transition<T>(tz.data(), tzg.data(), p_last, tc);
    T t = zero<T>();
    for (int k = 0; k < AGG_TC; k++) t = add(t, mul(alpha[k], tc[k]));
    t = mul(t, mul(sub(z, gl), inv(sub(zn, lift<T>(fe_one())))));
    AggAssertion asr[AGG_NA];
    agg_assertions(n, fe{pi.v_units_total, 0}, fe{pi.children_count, 0}, asr);
    for (int a = 0; a < AGG_NA; a++)
      t = add(t, mul(beta[a], mul(sub(tz[asr[a].col], lift<T>(asr[a].value)), inv(sub(z, lift<T>(fe_pow64(g, asr[a].step)))))));
    T h = zero<T>(), zj = lift<T>(fe_one());
    for (size_t j = 0; j < Cc; j++) { h = add(h, mul(hz[j], zj)); zj = mul(zj, zn); }
    if (!eq_t(h, t)) return "out-of-domain constraint identity does not hold";
  }
  {
    std::vector<fe> oc;
    for (auto& v : tz) flat(oc, v);
    for (auto& v : hz) flat(oc, v);
    for (auto& v : tzg) flat(oc, v);
    for (auto& v : hzg) flat(oc, v);
    coin.reseed(H.hash_elements(oc.data(), oc.size()));
  }
  std::vector<T> gam(W + Cc);
  for (auto& c : gam) c = draw();
  std::vector<T> falpha(nl);
  for (int d = 0; d < nl; d++) { coin.reseed(fri_roots[d]); falpha[d] = draw(); }
  coin.reseed(rem_commit);
  // FRI layer sections, remainder, PoW nonce
  FriSections fs;
  if (const char* e = read_fri_sections(r, nl, fs)) return e;
  const uint64_t nonce = fs.nonce;
  {
    const fe d = H.merge_with_int(coin.seed, nonce);
    const uint32_t tzb = d.lo ? (uint32_t)__builtin_ctzll(d.lo) : 64u;
    if (tzb < o.grinding_factor) return "proof-of-work nonce does not meet the grinding factor";
  }
  std::vector<size_t> pos;
  query_positions(coin, nonce, o.num_queries, N, pos);
  const size_t nq = pos.size();
  if (nq != cx.nq) return "num_unique_queries does not match the drawn positions";
  // openings
  if (tq_v.len != nq * W * 16 || cq_v.len != nq * Cc * es) return "query value sections have the wrong size";
  std::vector<fe> trows;
  std::vector<T> crows;
  read_values(tq_v, trows, nq * W);
  read_values(cq_v, crows, nq * Cc);
  if (tq_v.bad || cq_v.bad) return "non-canonical query values";
  {
    std::vector<fe> leaves(nq), row;
    fe root;
    for (size_t k = 0; k < nq; k++) leaves[k] = H.hash_elements(&trows[k * W], W);
    if (!batch_merkle_root(tq_p, N, pos, leaves, &root) || !fe_eq(root, troot) || !tq_p.done())
      return "trace Merkle opening does not reproduce the trace commitment";
    for (size_t k = 0; k < nq; k++) {
      row.clear();
      for (size_t j = 0; j < Cc; j++) flat(row, crows[k * Cc + j]);
      leaves[k] = H.hash_elements(row.data(), row.size());
    }
    if (!batch_merkle_root(cq_p, N, pos, leaves, &root) || !fe_eq(root, croot) || !cq_p.done())
      return "constraint Merkle opening does not reproduce the constraint commitment";
  }
  // DEEP values at the query positions
  const fe wN = root_of_unity((unsigned)ilog2(N)), three{3, 0};
  std::vector<T> ev(nq);
  for (size_t k = 0; k < nq; k++) {
    const T x = lift<T>(fe_mul(three, fe_pow64(wN, pos[k])));
    const T iz = inv(sub(x, z)), izg = inv(sub(x, zg));
    T y = zero<T>();
    for (size_t c = 0; c < W; c++) {
      const T t = lift<T>(trows[k * W + c]);
      y = add(y, mul(gam[c], add(mul(sub(t, tz[c]), iz), mul(sub(t, tzg[c]), izg))));
    }
    for (size_t j = 0; j < Cc; j++) {
      const T h = crows[k * Cc + j];
      y = add(y, mul(gam[W + j], add(mul(sub(h, hz[j]), iz), mul(sub(h, hzg[j]), izg))));
    }
    ev[k] = y;
  }
  // FRI
  std::vector<size_t> fpos = pos;
  size_t Nd = N;
  FoldStep fold;
  std::vector<std::pair<size_t, uint32_t>> sorted;  // (folded position, its index in np)
  std::vector<T> lv;
  for (int d = 0; d < nl; d++) {
    const size_t h = Nd / 2;
    fold_positions(fpos, h, fold);
    const std::vector<size_t>& np = fold.pos;
    const size_t m = np.size();
    if (fs.values[d].len != 2 * m * es) return "FRI layer values have the wrong size";
    read_values(fs.values[d], lv, 2 * m);
    if (fs.values[d].bad) return "non-canonical FRI layer values";
    for (size_t k = 0; k < fpos.size(); k++)
      if (!eq_t(lv[2 * fold.slot[k] + (fpos[k] >= h ? 1 : 0)], ev[k])) return "FRI layer opening disagrees with the folded values";
    {
      sorted_fold(np, sorted);
      std::vector<size_t> sp(m);
      std::vector<fe> sl(m), row;
      for (size_t k = 0; k < m; k++) {
        const size_t j = sorted[k].second;
        sp[k] = sorted[k].first;
        row.clear();
        flat(row, lv[2 * j]);
        flat(row, lv[2 * j + 1]);
        sl[k] = H.hash_elements(row.data(), row.size());
      }
      fe root;
      if (!batch_merkle_root(fs.paths[d], h, sp, sl, &root) || !fe_eq(root, fri_roots[d]) || !fs.paths[d].done())
        return "FRI layer Merkle opening does not reproduce the layer commitment";
    }
    const fe gd = root_of_unity((unsigned)ilog2(Nd));
    std::vector<T> next(m);
    for (size_t j = 0; j < m; j++) {
      const fe x0 = fe_mul(three, fe_pow64(gd, np[j])), x1 = fe_sub(fe_zero(), x0);
      const T num = sub(mul(lv[2 * j + 1], sub(falpha[d], lift<T>(x0))), mul(lv[2 * j], sub(falpha[d], lift<T>(x1))));
      next[j] = mulb(num, fe_inv(fe_sub(x1, x0)));
    }
    fpos = np;
    ev.swap(next);
    Nd = h;
  }
  const size_t rlen = o.fri_remainder_max_degree + 1;
  if (fs.remainder.len != rlen * es) return "FRI remainder has the wrong size";
  std::vector<T> rem;
  read_values(fs.remainder, rem, rlen);
  if (fs.remainder.bad) return "non-canonical remainder";
  {
    std::vector<fe> rf;
    for (auto& v : rem) flat(rf, v);
    if (!fe_eq(H.hash_elements(rf.data(), rf.size()), rem_commit)) return "remainder does not match its commitment";
  }
  const fe gr = root_of_unity((unsigned)ilog2(Nd));
  for (size_t k = 0; k < fpos.size(); k++) {
    const T x = lift<T>(fe_mul(three, fe_pow64(gr, fpos[k])));
    T v = zero<T>();
    for (size_t c = 0; c < rlen; c++) v = add(mul(v, x), rem[c]);
    if (!eq_t(v, ev[k])) return "FRI remainder does not match the last layer";
  }
  return "";
}

// RecursionArtifactCodec::decode (lib.rs:552-660)
struct Rdb {
  const uint8_t* p;
  size_t n, off = 0;
  const uint8_t* take(size_t k, const char* what) {
    if (off + k > n) throw AggError(what);
    off += k;
    return p + off - k;
  }
  template <class U> U num(const char* what) { U v; memcpy(&v, take(sizeof(U), what), sizeof(U)); return v; }
};
AggPi decode_artifact(const uint8_t* b, size_t n, const uint8_t** proof, size_t* plen) {
  Rdb r{b, n};
  if (n < 6 || memcmp(b, "ZKLRC1", 6)) throw AggError("invalid recursion artifact magic");
  r.off = 6;
  AggPi p;
  memcpy(p.program_id, r.take(32, "program_id truncated"), 32);
  memcpy(p.program_commitment, r.take(32, "program_commitment truncated"), 32);
  memcpy(p.pi_digest, r.take(32, "pi_digest truncated"), 32);
  memcpy(p.children_root, r.take(32, "children_root truncated"), 32);
  memcpy(p.batch_id, r.take(32, "batch_id truncated"), 32);
  p.v_units_total = r.num<uint64_t>("v_units_total truncated");
  p.children_count = r.num<uint32_t>("children_count truncated");
  p.m = r.num<uint32_t>("u32 truncated");
  p.rho = r.num<uint16_t>("u16 truncated");
  p.q = r.num<uint16_t>("u16 truncated");
  p.o = r.num<uint16_t>("u16 truncated");
  p.lambda = r.num<uint16_t>("u16 truncated");
  p.pi_len = r.num<uint32_t>("u32 truncated");
  p.v_units = r.num<uint64_t>("v_units(meta) truncated");
  p.lde_blowup = r.num<uint32_t>("u32 truncated");
  p.folding_factor = r.num<uint8_t>("u8 truncated");
  p.redundancy = r.num<uint8_t>("u8 truncated");
  p.num_layers = r.num<uint8_t>("u8 truncated");
  p.num_queries = r.num<uint16_t>("u16 truncated");
  p.grinding_factor = r.num<uint32_t>("u32 truncated");
  memcpy(p.suite_id, r.take(32, "suite_id truncated"), 32);
  const uint32_t nms = r.num<uint32_t>("children_ms length truncated");
  if ((size_t)nms * 4 > n) throw AggError("children_ms truncated");
  for (uint32_t i = 0; i < nms; i++) p.children_ms.push_back(r.num<uint32_t>("children_ms truncated"));
  for (uint8_t* x : {p.vm_state_initial, p.vm_state_final, p.ram_u_initial, p.ram_u_final, p.ram_s_initial,
                     p.ram_s_final})
    memcpy(x, r.take(32, "boundary state truncated"), 32);
  for (int i = 0; i < 3; i++) memcpy(p.rom_initial[i], r.take(32, "rom_s_initial truncated"), 32);
  for (int i = 0; i < 3; i++) memcpy(p.rom_final[i], r.take(32, "rom_s_final truncated"), 32);
  const uint32_t pl = r.num<uint32_t>("proof length truncated");
  *proof = r.take(pl, "proof bytes truncated");
  *plen = pl;
  return p;
}

std::string verify_artifact(const uint8_t* art, size_t len, uint32_t min_bits) {
  const uint8_t* pb;
  size_t plen;
  const AggPi pi = decode_artifact(art, len, &pb, &plen);
  Rd r{pb, plen, 0, false};
  ProofContext cx;
  if (const char* e = read_context(r, nullptr, cx)) return e;
  const uint32_t W = cx.W;
  const unsigned logn = cx.logn;
  const zkl_proof_options& o = cx.opts;
  if (W != AGG_W) return "aggregation trace width must be 31 (AggColumns)";
  if (logn < 3 || logn > 13) return "aggregation trace length out of range";
  uint32_t np, rate;
  zkl_select_partitions(W, 1u << logn, &np, &rate);
  if (o.fri_folding_factor != 2 || o.fri_remainder_max_degree != 1 || o.batching_constraints || o.batching_deep ||
      o.num_partitions != np || o.hash_rate != rate || o.blowup_factor < 2 || (o.blowup_factor & (o.blowup_factor - 1)) ||
      o.num_queries == 0)
    return "unsupported aggregation proof options";
  if (o.field_extension != 1 && o.field_extension != 2) return "unsupported field extension";
  // AcceptableOptions::MinConjecturedSecurity(min_bits) (prove.rs:738)
  if (conjectured_bits(o.num_queries, o.blowup_factor, o.grinding_factor, o.field_extension) < min_bits)
    return "aggregation proof does not meet the requested conjectured security";
  return o.field_extension == 2 ? verify_air<fe2>(r, pi, cx) : verify_air<fe>(r, pi, cx);
}

}  // namespace
}  // namespace zkl

// ====================================================================== C ABI
using namespace zkl;

namespace {
// ---- aggregation session (zkl_hip_agg_begin / _add / _finish; the one-shot calls run one) ----
// A child is replayed when it arrives: everything that depends on it alone (decode, replay, the
// replay's hashing, the unweighted overlay terms) happens in add, into the slot of its position;
// finish does what needs every child (the public inputs, the weights, the chain, the proof).
struct Session {
  zkl_ctx* ctx = nullptr;  // nullptr: host executor and host prover
  zkl_agg_options opts{};
  uint32_t n = 0;
  std::mutex mu;  // state, added, finished, ms
  std::vector<uint8_t> state;  // per position: 0 free, 1 being added, 2 added
  uint32_t added = 0;
  bool finished = false;
  std::vector<std::vector<uint8_t>> bytes;  // StepDecoded::inner points into them
  std::vector<Child> ch;
  std::vector<ChildTerms> tm;
  std::vector<std::string> err;  // per position: "" or why the child is refused
  // [0] host time of the adds without the overlay terms, [1] their hashing, [2] trace assembly,
  // [3] proof without grinding, [4] grinding, [5] finish; terms: the overlay terms of the adds
  double ms[6] = {0, 0, 0, 0, 0, 0}, ms_terms = 0;
};

// The option checks of RecursionBackend::prove (prove.rs:645-681)
AggOpts checked_options(const zkl_agg_options& o) {
  AggOpts ao{std::max<uint32_t>(o.queries, 16), o.blowup, o.grind, o.min_security_bits >= 128 ? 2u : 1u};
  if (ao.queries > 255) throw AggError("queries must be at most 255");
  if (ao.grind > 32) throw AggError("grinding factor must be at most 32");  // ProofOptions::new [WF-recall]
  if (o.trace_mode > ZKL_AGG_TRACE_REFERENCE) throw AggError("unknown aggregation trace mode");
  if (o.min_security_bits >= 64) {  // prove.rs:664-681
    if (conjectured_bits(ao.queries, ao.blowup, ao.grind, ao.field_ext) < o.min_security_bits)
      throw AggError(
          "aggregation prover options do not achieve requested min_security_bits; increase --queries/--blowup/--grind "
          "or lower --security-bits");
  }
  ao.check_air = o.trace_mode == ZKL_AGG_TRACE_VALID;
  return ao;
}

const char* const kNoSteps = "RecursionBackend::recursion_prove requires at least one step proof";

void session_init(Session& S, zkl_ctx* ctx, uint32_t n, const zkl_agg_options& opts) {
  S.ctx = ctx;
  S.opts = opts;
  S.n = n;
  S.state.assign(n, 0);
  S.bytes.resize(n);
  S.ch.resize(n);
  S.tm.resize(n);
  S.err.resize(n);
}

// Adds k children at positions pos[0..k): decode and replay plan on host threads, one batch of
// hashing through the session's executor (host threads, or the context's device under its lock
// for the submission alone), the verdicts and the overlay terms.  borrow: the caller's buffers
// outlive the session's use of them (the one-shot calls), so they are not copied and the device
// results are read where the context left them (no other thread adds).  A position out of range
// or taken throws before anything changes.
void session_add(Session& S, const uint32_t* pos, const uint8_t* const* steps, const size_t* lens, size_t k, bool borrow) {
  {
    std::lock_guard<std::mutex> lk(S.mu);
    if (S.finished) throw AggError("aggregation session: add after finish");
    for (size_t j = 0; j < k; j++) {
      if (pos[j] >= S.n)
        throw AggError("aggregation session: position " + std::to_string(pos[j]) + " is out of range (" +
                       std::to_string(S.n) + " step proofs)");
      if (S.state[pos[j]] != 0)
        throw AggError("aggregation session: position " + std::to_string(pos[j]) + " was already added");
      for (size_t i = 0; i < j; i++)
        if (pos[i] == pos[j]) throw AggError("aggregation session: position " + std::to_string(pos[j]) + " given twice");
    }
    for (size_t j = 0; j < k; j++) S.state[pos[j]] = 1;
  }
  double ms[2] = {0, 0}, ms_terms = 0;
  // children replay independently (~10^4 permutations each at 2^16 rows): each replay is
  // verify_segment_ex without the out-of-domain identity (agg/fs.rs:38-245)
  std::vector<zkl_air_public_inputs> pis(k);
  auto t0 = std::chrono::steady_clock::now();
  parallel_for(k, [&](size_t j) {
    const uint32_t i = pos[j];
    try {
      const uint8_t* p = steps[j];
      if (!borrow) {
        S.bytes[i].assign(steps[j], steps[j] + lens[j]);
        p = S.bytes[i].data();
      }
      S.ch[i].step = decode_step(p, lens[j]);
      pis[j] = replay_pi(S.ch[i].step);
    } catch (const std::exception& e) {
      S.err[i] = e.what();
    }
  });
  ms[0] += ms_since(t0);
  std::vector<BatchItem> items;
  std::vector<size_t> who;
  for (size_t j = 0; j < k; j++)
    if (S.err[pos[j]].empty()) {
      Child& c = S.ch[pos[j]];
      items.push_back({c.step.inner, c.step.inner_len, &pis[j], nullptr, &c.v});
      who.push_back(j);
    }
  std::vector<std::string> verr(items.size());
  // an executor per call: each keeps its results until its next call
  const PlanExec exec = !S.ctx ? host_plan_exec() : borrow ? device_plan_exec(S.ctx) : device_plan_exec_owned(S.ctx);
  verify_segments_batch(items.data(), items.size(), false, exec, S.ctx ? PLAN_DEVICE_CAP : 0, verr.data(), ms);
  for (size_t q = 0; q < who.size(); q++) {
    const uint32_t i = pos[who[q]];
    if (!verr[q].empty()) S.err[i] = "child step proof does not replay: " + verr[q];
    else if (S.ch[i].v.fri_roots.size() < 2) S.err[i] = "AggTrace requires at least two FRI layers per child";
  }
  t0 = std::chrono::steady_clock::now();
  parallel_for(k, [&](size_t j) {
    if (S.err[pos[j]].empty()) child_terms(S.ch[pos[j]].v, S.tm[pos[j]]);
  });
  ms_terms = ms_since(t0);
  std::lock_guard<std::mutex> lk(S.mu);
  for (size_t j = 0; j < k; j++) S.state[pos[j]] = 2;
  S.added += (uint32_t)k;
  S.ms[0] += ms[0];
  S.ms[1] += ms[1];
  S.ms_terms += ms_terms;
}

std::string child_error(const Session& S, uint32_t i) { return "child " + std::to_string(i) + ": " + S.err[i]; }

// every position added; the lowest refused child's message; the shared suite
void session_children(Session& S) {
  {
    std::lock_guard<std::mutex> lk(S.mu);
    if (S.finished) throw AggError("aggregation session: finish was already called");
    S.finished = true;
    if (S.added != S.n)
      throw AggError("aggregation session: " + std::to_string(S.added) + " of " + std::to_string(S.n) +
                     " step proofs added");
  }
  for (uint32_t i = 0; i < S.n; i++)
    if (!S.err[i].empty()) throw AggError(child_error(S, i));
  for (const Child& c : S.ch)
    if (memcmp(c.step.suite, S.ch[0].step.suite, 32))
      throw AggError("RecursionBackend::recursion_prove requires all steps to share the same suite_id");
}

AggPi public_of(const std::vector<Child>& ch) {
  std::vector<StepDecoded> st;
  for (const Child& c : ch) st.push_back(c.step);
  return build_public(st);
}

// Process-wide switch of the device ZlAggAir prover (zkl_hip_set_agg_device_prover): -1 = not
// read yet, then ZKL_AGG_DEVICE_PROVER=0 in the environment starts it at 0, anything else at 1.
std::atomic<int> g_agg_device_prover{-1};
bool agg_device_prover_enabled() {
  int v = g_agg_device_prover.load();
  if (v < 0) {
    const char* e = getenv("ZKL_AGG_DEVICE_PROVER");
    v = (e && e[0] == '0' && e[1] == 0) ? 0 : 1;
    int expect = -1;
    if (!g_agg_device_prover.compare_exchange_strong(expect, v)) v = expect;
  }
  return v != 0;
}

// the cross-child checks in their order, the trace, the proof, the artifact
std::vector<uint8_t> session_finish(Session& S, uint8_t digest_out[32]) {
  const auto t_call = std::chrono::steady_clock::now();
  struct Total {
    Session& S;
    std::chrono::steady_clock::time_point t;
    ~Total() { S.ms[5] = ms_since(t); }
  } total{S, t_call};
  session_children(S);
  auto t0 = std::chrono::steady_clock::now();
  const AggPi pi = public_of(S.ch);  // build_public; prove() re-derives suite / count / ms identically
  const auto T = build_agg_trace(pi, S.ch, S.tm, S.opts.trace_mode);
  S.ms[2] = ms_since(t0);
  const AggOpts ao = checked_options(S.opts);
  const std::vector<fe> el = agg_pi_elements(pi);
  t0 = std::chrono::steady_clock::now();
  zkl_ctx* pctx = agg_device_prover_enabled() ? S.ctx : nullptr;
  const std::vector<uint8_t> proof = ao.field_ext == 2
                                         ? prove_air<fe2>(T, el, pi.v_units_total, pi.children_count, ao, pctx, &S.ms[4])
                                         : prove_air<fe>(T, el, pi.v_units_total, pi.children_count, ao, pctx, &S.ms[4]);
  S.ms[3] = ms_since(t0) - S.ms[4];
  if (digest_out) recursion_digest(pi, digest_out);
  return encode_artifact(pi, proof);
}

// the one-shot calls' argument checks, then every child in one add
void session_add_all(Session& S, const uint8_t* const* steps, const size_t* lens, uint32_t n) {
  if (!steps || !lens || n == 0) throw AggError(kNoSteps);
  for (uint32_t i = 0; i < n; i++)
    if (!steps[i]) throw AggError("null step proof");
  std::vector<uint32_t> pos(n);
  for (uint32_t i = 0; i < n; i++) pos[i] = i;
  session_add(S, pos.data(), steps, lens, n, true);
}

int give_bytes(const std::vector<uint8_t>& v, uint8_t** out, size_t* len) {
  *out = (uint8_t*)malloc(std::max<size_t>(v.size(), 1));
  if (!*out) return ZKL_E_OOM;
  memcpy(*out, v.data(), v.size());
  *len = v.size();
  return ZKL_OK;
}
bool canonical_fe(fe v) { return v.hi < P_HI || v.lo < P_LO; }

}  // namespace

extern "C" {

// the one-shot calls: a session that is begun, given every child at once and finished.  The
// children are checked before the options here (in a session begin checks the options first).
static int agg_prove_with(zkl_ctx* ctx, const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps,
                          const zkl_agg_options* opts, uint8_t** artifact_out, size_t* artifact_len,
                          uint8_t digest_out[32]) {
  if (!opts || !artifact_out || !artifact_len) return ZKL_E_INVALID;
  std::vector<uint8_t> art;
  const auto t_call = std::chrono::steady_clock::now();
  for (double& x : g_agg_ms) x = 0;
  Session S;
  const int rc = guarded_call([&] {
    session_init(S, ctx, n_steps, *opts);
    session_add_all(S, steps, step_lens, n_steps);
    art = session_finish(S, digest_out);
  });
  g_agg_ms[0] = S.ms[0];
  g_agg_ms[1] = S.ms[1];
  g_agg_ms[2] = S.ms[2] + S.ms_terms;  // the overlay terms are part of the trace in this call's slots
  g_agg_ms[3] = S.ms[3];
  g_agg_ms[4] = S.ms[4];
  g_agg_ms[5] = ms_since(t_call);
  if (rc) return rc;
  return give_bytes(art, artifact_out, artifact_len);
}

int zkl_agg_prove(const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps, const zkl_agg_options* opts,
                  uint8_t** artifact_out, size_t* artifact_len, uint8_t digest_out[32]) {
  return agg_prove_with(nullptr, steps, step_lens, n_steps, opts, artifact_out, artifact_len, digest_out);
}

int zkl_hip_agg_prove(zkl_ctx* ctx, const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps,
                      const zkl_agg_options* opts, uint8_t** artifact_out, size_t* artifact_len,
                      uint8_t digest_out[32]) {
  return agg_prove_with(ctx, steps, step_lens, n_steps, opts, artifact_out, artifact_len, digest_out);
}

int zkl_hip_agg_begin(zkl_ctx* ctx, uint32_t n_steps, const zkl_agg_options* opts, zkl_agg_session** out) {
  if (!opts || !out) return ZKL_E_INVALID;
  *out = nullptr;
  return guarded_call([&] {
    checked_options(*opts);
    if (n_steps == 0) throw AggError(kNoSteps);
    std::unique_ptr<Session> S(new Session());
    session_init(*S, ctx, n_steps, *opts);
    *out = reinterpret_cast<zkl_agg_session*>(S.release());
  });
}

int zkl_hip_agg_add(zkl_agg_session* s, uint32_t position, const uint8_t* step, size_t len) {
  if (!s) return ZKL_E_INVALID;
  Session& S = *reinterpret_cast<Session*>(s);
  return guarded_call([&] {
    if (!step) throw AggError("null step proof");
    session_add(S, &position, &step, &len, 1, false);
    if (!S.err[position].empty()) throw AggError(child_error(S, position));
  });
}

int zkl_hip_agg_finish(zkl_agg_session* s, uint8_t** artifact_out, size_t* artifact_len, uint8_t digest_out[32]) {
  if (!s || !artifact_out || !artifact_len) return ZKL_E_INVALID;
  Session& S = *reinterpret_cast<Session*>(s);
  std::vector<uint8_t> art;
  const int rc = guarded_call([&] { art = session_finish(S, digest_out); });
  if (rc) return rc;
  return give_bytes(art, artifact_out, artifact_len);
}

int zkl_hip_agg_session_times(const zkl_agg_session* s, double* out_ms, int max_n) {
  if (!s || !out_ms || max_n <= 0) return 0;
  Session& S = *const_cast<Session*>(reinterpret_cast<const Session*>(s));
  std::lock_guard<std::mutex> lk(S.mu);
  const double v[6] = {S.ms[0] + S.ms_terms, S.ms[1], S.ms[2], S.ms[3], S.ms[4], S.ms[5]};
  const int k = std::min(max_n, 6);
  for (int i = 0; i < k; i++) out_ms[i] = v[i];
  return k;
}

void zkl_hip_agg_free(zkl_agg_session* s) { delete reinterpret_cast<Session*>(s); }

int zkl_hip_set_agg_device_prover(int on) {
  if (on != 0 && on != 1) return ZKL_E_INVALID;
  g_agg_device_prover.store(on);
  return ZKL_OK;
}

int zkl_hip_agg_device_prover(void) { return agg_device_prover_enabled() ? 1 : 0; }

int zkl_hip_agg_prove_trace(zkl_ctx* ctx, const zkl_f128* trace, uint32_t rows, const zkl_f128* pi_elements, uint32_t n_pi,
                            uint64_t v_units_total, uint32_t children_count, const zkl_agg_options* opts, int check_air,
                            uint8_t** proof_out, size_t* proof_len) {
  if (!trace || (!pi_elements && n_pi) || !opts || !proof_out || !proof_len) return ZKL_E_INVALID;
  std::vector<uint8_t> proof;
  const int rc = guarded_call([&] {
    if (rows < MIN_AGG_TRACE_ROWS || rows >= (1u << 14) || (rows & (rows - 1)))
      throw AggError("aggregation trace rows must be a power of two in [8, 2^14)");
    AggOpts ao{std::max<uint32_t>(opts->queries, 16), opts->blowup, opts->grind, opts->min_security_bits >= 128 ? 2u : 1u};
    if (ao.queries > 255) throw AggError("queries must be at most 255");
    if (ao.grind > 32) throw AggError("grinding factor must be at most 32");
    ao.check_air = check_air != 0;
    std::vector<std::vector<fe>> T(AGG_W, std::vector<fe>(rows));
    for (size_t c = 0; c < AGG_W; c++)
      for (uint32_t r = 0; r < rows; r++) {
        const fe v = fe_from(trace[c * rows + r]);
        if (!canonical_fe(v)) throw AggError("aggregation trace element is not a canonical field element");
        T[c][r] = v;
      }
    std::vector<fe> el(n_pi);
    for (uint32_t k = 0; k < n_pi; k++) {
      el[k] = fe_from(pi_elements[k]);
      if (!canonical_fe(el[k])) throw AggError("public input element is not a canonical field element");
    }
    proof = ao.field_ext == 2 ? prove_air<fe2>(T, el, v_units_total, children_count, ao, ctx, &g_agg_ms[4])
                              : prove_air<fe>(T, el, v_units_total, children_count, ao, ctx, &g_agg_ms[4]);
  });
  if (rc) return rc;
  *proof_out = (uint8_t*)malloc(proof.size());
  if (!*proof_out) return ZKL_E_OOM;
  memcpy(*proof_out, proof.data(), proof.size());
  *proof_len = proof.size();
  return ZKL_OK;
}

int zkl_agg_last_times(double* out_ms, int max_n) {
  if (!out_ms || max_n <= 0) return 0;
  const int k = std::min(max_n, 6);
  for (int i = 0; i < k; i++) out_ms[i] = g_agg_ms[i];
  return k;
}

int zkl_agg_verify(const uint8_t* artifact, size_t len, uint32_t min_security_bits) {
  if (!artifact) return ZKL_E_INVALID;
  return guarded_call([&] {
    const std::string e = verify_artifact(artifact, len, min_security_bits);
    if (!e.empty()) throw AggError(e);
  });
}

int zkl_agg_trace(const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps, zkl_f128* out,
                  uint32_t max_rows, uint32_t* rows_out) {
  return zkl_agg_trace_mode(steps, step_lens, n_steps, ZKL_AGG_TRACE_VALID, out, max_rows, rows_out);
}

int zkl_agg_trace_mode(const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps, uint32_t trace_mode,
                       zkl_f128* out, uint32_t max_rows, uint32_t* rows_out) {
  if (!rows_out || trace_mode > ZKL_AGG_TRACE_REFERENCE) return ZKL_E_INVALID;
  return guarded_call([&] {
    Session S;
    zkl_agg_options o{};
    o.trace_mode = trace_mode;
    session_init(S, nullptr, n_steps, o);
    session_add_all(S, steps, step_lens, n_steps);
    session_children(S);
    const auto T = build_agg_trace(public_of(S.ch), S.ch, S.tm, trace_mode);
    const uint32_t rows = (uint32_t)T[0].size();
    *rows_out = rows;
    if (!out) return;
    if (rows > max_rows) throw AggError("output buffer too small for the aggregation trace");
    for (size_t c = 0; c < T.size(); c++)
      for (uint32_t r = 0; r < rows; r++) out[c * rows + r] = to_abi(T[c][r]);
  });
}

}  // extern "C"
