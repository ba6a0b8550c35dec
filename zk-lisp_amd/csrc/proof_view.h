// Host-side reading of segment proofs: Proof::to_bytes() of a ZkLispAir proof parsed, its
// Fiat-Shamir transcript replayed and every check of winter-verifier 0.13.1 applied
// (the reference calls it at prove.rs:802-941 and replays the same
// transcript in agg/fs.rs:38-245).  The parsed and replayed values stay available to the
// aggregation (agg.cpp: the child transcripts of agg/child.rs:531-850).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/zkl_hip.h"
#include "air_host.h"
#include "field.h"
#include "proof_codec.h"

namespace zkl {

// BatchMerkleProof::get_root (winter-crypto 0.13) for sorted unique leaf indices with their
// digests; consumes the proof bytes from r.  Returns false if the proof is malformed.
bool batch_merkle_root(Rd& r, size_t n_leaves, const std::vector<size_t>& idx, const std::vector<fe>& leaves,
                       fe* root);

// ---- hash plan: the Poseidon work of a replay as flat jobs over one index
// space of field elements.  An index below PLAN_OUT addresses `in` (values parsed from the
// proof), PLAN_OUT | k the k-th computed digest.  Built only from proofs that passed every
// structural check, so a corrupted proof changes the values in `in`, never an index.
constexpr uint32_t PLAN_OUT = 0x80000000u;
struct HashPlan {
  // row digest of in[src .. src + ncols): chunks of psize columns through hash_elements, then
  // merge_many of the chunk digests when `merge`, else the single chunk's digest (the one-chunk
  // rule is resolved by whoever appends the job).  A FRI leaf is ncols = psize = 2, no merge.
  struct RowJob { uint32_t src, ncols, psize, merge, dst; };
  struct MergeJob { uint32_t left, right, dst; };   // dst = merge(left, right)
  struct DrawJob { fe seed; uint32_t count, dst; };  // dst + k = merge_with_int(seed, k + 1)
  std::vector<fe> in;
  uint32_t n_out = 0;
  std::vector<RowJob> rows;
  std::vector<std::vector<MergeJob>> merges;  // merges[h - 1]: height h above the leaves; reads
                                              // only inputs, row digests and lower heights
  std::vector<DrawJob> draws;
  uint32_t add_in(const fe* v, size_t n) {
    const uint32_t at = (uint32_t)in.size();
    in.insert(in.end(), v, v + n);
    return at;
  }
  uint32_t new_out(uint32_t n = 1) {
    const uint32_t at = PLAN_OUT | n_out;
    n_out += n;
    return at;
  }
  // snapshot / rollback: an opening rejected after some of its jobs were appended leaves none
  struct Mark { size_t in, rows, draws; uint32_t n_out; std::vector<size_t> merges; };
  Mark mark() const {
    Mark m{in.size(), rows.size(), draws.size(), n_out, {}};
    for (const auto& l : merges) m.merges.push_back(l.size());
    return m;
  }
  void rewind(const Mark& m) {
    in.resize(m.in);
    rows.resize(m.rows);
    draws.resize(m.draws);
    n_out = m.n_out;
    for (size_t h = 0; h < merges.size(); h++) merges[h].resize(h < m.merges.size() ? m.merges[h] : 0);
  }
  void add_merge(size_t height, uint32_t l, uint32_t r, uint32_t dst) {
    if (merges.size() < height) merges.resize(height);
    merges[height - 1].push_back({l, r, dst});
  }
};
// The plan of BatchMerkleProof::get_root (winter-crypto 0.13) for sorted unique leaf indices
// whose digests are the plan nodes `leaves`: parses the proof bytes from r, makes every
// structural rejection (depth byte, list shape, sharing, every proof node consumed, final
// index 1) and appends the merges; *root receives the root's node.  Nothing is hashed.
bool plan_batch_merkle(Rd& r, size_t n_leaves, const std::vector<size_t>& idx, const std::vector<uint32_t>& leaves,
                       HashPlan& plan, uint32_t* root);
// Host execution with hasher(): out[k] = value of node PLAN_OUT | k.  par_draws: large draw
// ranges are split over host threads (a single proof; a batch already has a thread per proof).
void run_plan_host(const HashPlan& plan, std::vector<fe>& out, bool par_draws);

struct SegmentView {
  // context
  uint32_t width = 0;
  size_t n = 0, lde = 0;
  int comp_cols = 0;
  zkl_proof_options opts{};
  // commitments
  fe trace_root{}, constraint_root{}, remainder_commit{};
  std::vector<fe> fri_roots;
  // out-of-domain frame: trace at z and z*g, composition columns at z and z*g
  std::vector<fe> ood_trace_z, ood_trace_zg, ood_comp_z, ood_comp_zg;
  // transcript
  fe z{};
  std::vector<fe> deep_coeffs;  // W trace then C composition coefficients
  std::vector<fe> fri_alphas;   // one per FRI layer
  std::vector<size_t> positions;  // unique, sorted query positions in the LDE domain
  uint64_t pow_nonce = 0;
  // openings
  std::vector<fe> trace_rows;   // positions x W
  std::vector<fe> comp_rows;    // positions x C
  std::vector<FoldStep> fri_folds;                 // per layer: folded positions and the slots folded into
  std::vector<std::vector<fe>> fri_values;         // per layer: [e_y, e_{y+h}] per folded position
  std::vector<fe> remainder;                       // reversed coefficients, degree <= rem_deg
  // the roots the trace / constraint openings reproduce when each opened row is hashed as the
  // reference's hash_row_poseidon does (agg/child.rs:1025-1045: a one-chunk row is not merged)
  // and the batch proof is decompressed with those leaves; equal to trace_root /
  // constraint_root unless a row is one chunk narrower than its partition
  fe trace_root_ref{}, constraint_root_ref{};
};

// ProofOptions bounds winterfell enforces when it builds or reads options (ProofOptions::new
// [WF-recall]): queries 1..255, blowup a power of two in 2..128, grinding <= 32, folding 2,
// remainder degree 2^k - 1 below the blowup, partitions 1..16, hash rate 1..255.  "" or the
// first violated bound.
std::string check_proof_options(const zkl_proof_options& o);

// Parses and verifies one segment proof under the given public inputs and options (the
// options must equal those recorded in the proof).  Returns "" when the proof verifies, the
// first failing check otherwise; `view` (optional) receives the parsed/replayed values.
std::string verify_segment(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi,
                           const zkl_proof_options& opts, SegmentView* view);
// The same with the options taken from the proof (opts == nullptr) and, when check_ood is
// false, without the out-of-domain constraint identity: the Fiat-Shamir replay plus every
// opening / DEEP / FRI / remainder / PoW check, which is what the aggregation re-derives from
// a step proof alone (agg/fs.rs:38-245 rebuilds the AIR public inputs without the expected
// VM output, so the identity is not available there either).
std::string verify_segment_ex(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi,
                              const zkl_proof_options* opts, SegmentView* view, bool check_ood);

// ---- deferred replay: verify_segment_ex split into "plan" and "hash" ---------
// replay_segment does everything verify_segment_ex does that needs no opening digest (parsing,
// transcript, positions, DEEP values, FRI folds, remainder) and appends the rest to R.plan,
// recording each deferred check at its place in the check sequence.  A host-side failure ends
// the replay where verify_segment_ex ends (R.host_err; every recorded check precedes it).
// finish_replay, given the plan's results, returns the verdict: the message of the failing
// check with the lowest sequence position -- what verify_segment_ex returns for the same bytes.
struct SegmentReplay {
  HashPlan plan;
  struct Check {
    uint32_t node;    // computed root; PLAN_OUT - 1: the out-of-domain identity over the drawn coefficients
    fe want;          // committed root
    const char* msg;
  };
  std::vector<Check> checks;
  struct Fix { uint32_t node; fe* dst; };  // *dst = node once the proof verifies (SegmentView::*_root_ref)
  std::vector<Fix> fixes;
  std::string host_err;
  AirInstance air;          // kept for the out-of-domain identity
  uint32_t ood_draws = 0;   // node of the first drawn coefficient (alphas, then betas)
  SegmentView local;
  SegmentView* view = nullptr;
};
void replay_segment(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi, const zkl_proof_options* opts,
                    SegmentView* view, bool check_ood, SegmentReplay& R);
std::string finish_replay(SegmentReplay& R, const fe* out);

// Executes plans[0..n): outs[i] receives a pointer to plan i's n_out results, valid until the
// executor's next call.  host_plan_exec runs them on host threads; device_plan_exec
// (prover.cpp) on a context's device under its lock.
using PlanExec = std::function<void(const HashPlan* const* plans, size_t n, const fe** outs)>;
PlanExec host_plan_exec();
PlanExec device_plan_exec(zkl_ctx* ctx);
// the same, with the results copied out of the context under its lock: outs stay valid until this
// executor's next call whatever other threads submit to the context meanwhile
PlanExec device_plan_exec_owned(zkl_ctx* ctx);
// f(i) for i < n on at most 16 host threads; the first exception is rethrown after the join
void parallel_for(size_t n, const std::function<void(size_t)>& f);

// A batch of proofs through replay_segment / exec / finish_replay, in waves of proofs planned
// on host threads and submissions of at most `cap` field elements of input + output (0: a whole
// wave at once, for the host executor, which stages nothing; PLAN_DEVICE_CAP for a device).  errs[i] = verify_segment_ex's message for
// item i.  ms (nullable) accumulates wall time: [0] host replay and verdicts, [1] exec.
struct BatchItem {
  const uint8_t* proof;
  size_t len;
  const zkl_air_public_inputs* pi;
  const zkl_proof_options* opts;  // nullable: taken from the proof
  SegmentView* view;              // nullable
};
constexpr size_t PLAN_DEVICE_CAP = (size_t)1 << 22;  // 64 MiB of device buffer, as much pinned staging
void verify_segments_batch(const BatchItem* items, size_t n, bool check_ood, const PlanExec& exec, size_t cap,
                           std::string* errs, double* ms);

// A decoded ZKLSTP1 step proof (StepProof::from_bytes, proof/step.rs:153-493) with the
// derived StepMeta (step.rs:516-533), zl1 root_trace (format.rs:214-238) and step digest
// (proof/digest.rs:16-68).  `inner` points into the caller's buffer.
struct StepDecoded {
  uint32_t lambda_bits = 0;
  uint8_t suite[32], program_id[32], program_commitment[32], merkle_root[32];
  uint64_t feature_mask = 0;
  std::vector<zkl_vm_arg> main_args;
  uint32_t vm_usage_mask = 0, ram_delta_clk_bits = 0;
  fe rom_acc[3];
  uint32_t segment_index = 0, segments_total = 1;  // new_single_segment normalises to (0, 1)
  uint8_t pc_init[32];
  // state_in, state_out, ram_gp_unsorted_in/out, ram_gp_sorted_in/out, rom_s_in[3], rom_s_out[3]
  uint8_t bnd[12][32];
  const uint8_t* inner = nullptr;
  size_t inner_len = 0;
  uint32_t m = 0, pi_len = 0;
  uint16_t rho = 0, q = 0, o = 0, lambda = 0;
  uint64_t v_units = 0;
  uint8_t digest[32], root_trace[32];
};
StepDecoded decode_step(const uint8_t* p, size_t n);

// runs f, mapping exceptions to ZKL_E_* codes and zkl_hip_last_error(NULL) (prover.cpp)
int guarded_call(const std::function<void()>& f);

}  // namespace zkl
