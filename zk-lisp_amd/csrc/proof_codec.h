// The one definition of winterfell 0.13.1's Proof::to_bytes layout [WF-recall, DESIGN.md §Proof
// bytes] and of the position rules around it, for the segment prover (prover.cpp), the
// aggregation prover and verifier (agg.cpp) and the segment verifier (verifier.cpp):
//   context        TraceInfo (width, 0, 0, log2 n, 0, 0), element size 16, the modulus,
//                  ProofOptions (10 bytes), num_unique_queries
//   commitments    Vec<u8>: trace root, constraint root, FRI layer roots, remainder commitment
//   queries        1 (main segment), then Vec<u8> each: trace rows, trace BatchMerkleProof,
//                  constraint rows, constraint BatchMerkleProof
//   OOD frame      Vec<u8> each: t(z) | t(zg), H(z) | H(zg)
//   FRI            layer count, per layer Vec<u8> values and Vec<u8> BatchMerkleProof, Vec<u8>
//                  remainder, partitions byte (log2 of 1), then the proof-of-work nonce (u64)
// An element of the proof's field E is sizeof(E) / 16 canonical base elements back to back (the
// quadratic extension's fe2 is two).  Host only.
#pragma once
#include "../../include/zkl_hip.h"
#include "field.h"
#include "host_proof.h"

namespace zkl {

// ---- shape
// FriOptions::num_fri_layers at folding factor 2: halvings of N down to the remainder domain
inline int fri_num_layers(size_t N, size_t blowup, size_t rem_deg) {
  const size_t rem_max = (rem_deg + 1) * blowup;
  int nl = 0;
  for (size_t d = N; d > rem_max; d /= 2) nl++;
  return nl;
}
// draw_integers' positions in the LDE domain of N (a power of two), sorted and de-duplicated
inline void query_positions(const fe* draws, size_t q, size_t N, std::vector<size_t>& out) {
  out.resize(q);
  for (size_t k = 0; k < q; k++) out[k] = (size_t)(draws[k].lo & (N - 1));
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}
// the same from the coin reseeded with the proof-of-work nonce (the counter restarts)
inline void query_positions(Coin& coin, uint64_t nonce, size_t q, size_t N, std::vector<size_t>& out) {
  coin.seed = hasher().merge_with_int(coin.seed, nonce);
  coin.counter = 0;
  std::vector<fe> d(q);
  for (auto& v : d) v = coin.draw();
  query_positions(d.data(), q, N, out);
}

// One FRI fold of a position list (fold_positions_usize, agg/child.rs:1072-1100; the order of
// FriProver::build_proof): pos = prev mod h in order of first occurrence, slot[k] = the index in
// pos that prev[k] folded into.  h is a power of two; at most 256 positions (batch_plan_into's
// bound), held in a 512-slot open-addressing set.  The vectors keep their capacity across calls.
struct FoldStep { std::vector<size_t> pos; std::vector<uint32_t> slot; };
inline void fold_positions(const std::vector<size_t>& prev, size_t h, FoldStep& out) {
  if (prev.size() > 256) throw std::invalid_argument("fold_positions: more than 256 query positions");
  uint64_t key[512];
  uint16_t at[512];  // index in pos; 0xFFFF: free
  memset(at, 0xFF, sizeof at);
  out.pos.clear();
  out.slot.resize(prev.size());
  for (size_t i = 0; i < prev.size(); i++) {
    const size_t y = prev[i] & (h - 1);
    size_t k = (size_t)(((uint64_t)y * 0x9E3779B97F4A7C15ull) >> 55);
    while (at[k] != 0xFFFF && key[k] != y) k = (k + 1) & 511;
    if (at[k] == 0xFFFF) {
      key[k] = y;
      at[k] = (uint16_t)out.pos.size();
      out.pos.push_back(y);
    }
    out.slot[i] = at[k];
  }
}

// the folded positions with their indices, ascending: the order of a layer's Merkle opening
inline void sorted_fold(const std::vector<size_t>& pos, std::vector<std::pair<size_t, uint32_t>>& out) {
  out.resize(pos.size());
  for (size_t k = 0; k < pos.size(); k++) out[k] = {pos[k], (uint32_t)k};
  std::sort(out.begin(), out.end());
}

// ---- writer: the sections in order, each written in place (length, then bytes)
struct ProofWriter {
  Bytes& P;
  void context(uint32_t W, int logn, const zkl_proof_options& o, size_t nq) {
    P.u8((uint8_t)W); P.u8(0); P.u8(0); P.u8((uint8_t)logn); P.u8(0); P.u8(0);  // TraceInfo
    P.u8(16); P.felem(fe{P_LO, P_HI});                                           // modulus bytes
    P.u8((uint8_t)o.num_queries); P.u8((uint8_t)o.blowup_factor); P.u8((uint8_t)o.grinding_factor);
    P.u8((uint8_t)o.field_extension); P.u8((uint8_t)o.fri_folding_factor); P.u8((uint8_t)o.fri_remainder_max_degree);
    P.u8((uint8_t)o.batching_constraints); P.u8((uint8_t)o.batching_deep);
    P.u8((uint8_t)o.num_partitions); P.u8((uint8_t)o.hash_rate);
    P.u8((uint8_t)nq);
  }
  void commitments(fe troot, fe croot, const std::vector<fe>& fri_roots, fe rem_commit) {
    P.usize(32 * (3 + fri_roots.size()));
    P.digest(troot); P.digest(croot);
    for (const fe& r : fri_roots) P.digest(r);
    P.digest(rem_commit);
  }
  void queries() { P.usize(1); }  // one trace segment; then values + multiproof, for trace and constraint rows
  // a run of `count` elements of E = T
  template <class T>
  void values(const T* v, size_t count) {
    static_assert(sizeof(T) % sizeof(fe) == 0, "an element is a run of base elements");
    P.usize(count * sizeof(T));
    P.raw(v, count * sizeof(T));
  }
  // BatchMerkleProof of a plan: [depth][lists], per list [len][len digests]; digest_at(i) is the
  // digest of plan.node[i]
  template <class DigestAt>
  void multiproof(const Plan& plan, int depth, DigestAt&& digest_at) {
    const size_t len = 2 + plan.len.size() + 32 * plan.node.size();
    P.usize(len);
    const size_t o = P.v.size();
    P.v.resize(o + len);
    uint8_t* w = P.v.data() + o;
    *w++ = (uint8_t)depth;
    *w++ = (uint8_t)plan.len.size();
    size_t i = 0;
    for (uint32_t l : plan.len) {
      *w++ = (uint8_t)l;
      for (uint32_t k = 0; k < l; k++, w += 32) {  // digest: the 16 value bytes + 16 zero bytes
        const fe d = digest_at(i++);
        memcpy(w, &d, 16);
        memset(w + 16, 0, 16);
      }
    }
  }
  template <class T>
  void ood(const T* tz, const T* tzg, size_t W, const T* hz, const T* hzg, size_t C) {
    P.usize(2 * W * sizeof(T));
    P.raw(tz, W * sizeof(T)); P.raw(tzg, W * sizeof(T));
    P.usize(2 * C * sizeof(T));
    P.raw(hz, C * sizeof(T)); P.raw(hzg, C * sizeof(T));
  }
  // then per layer values ([e_y, e_{y+h}] per folded position) + multiproof
  void fri_layers(int nl) { P.usize((uint64_t)nl); }
  template <class T>
  void remainder(const T* rem, size_t count) {
    values(rem, count);
    P.u8(0);  // FriProof num_partitions (log2 of 1)
  }
  void finish(uint64_t nonce) { P.u64(nonce); }
};

// ---- reader: the steps a verifier takes, with its own checks between them.  Each returns
// nullptr or the message of the first defect.
template <class T>
inline T read_e(Rd& r) {
  fe w[sizeof(T) / sizeof(fe)];
  for (fe& x : w) x = r.felem();
  T v;
  memcpy(&v, w, sizeof(T));
  return v;
}
template <class T>
inline void read_values(Rd& r, std::vector<T>& out, size_t count) {
  out.resize(count);
  for (auto& v : out) v = read_e<T>(r);
}

struct ProofContext { uint32_t W = 0; unsigned logn = 0; zkl_proof_options opts{}; size_t nq = 0; };  // nq: num_unique_queries
// want (nullable): the options the caller expects the proof to record
inline const char* read_context(Rd& r, const zkl_proof_options* want, ProofContext& c) {
  c.W = r.u8();
  if (r.u8() != 0 || r.u8() != 0) return "trace info: auxiliary segments are not supported";
  c.logn = r.u8();
  if (r.u8() != 0 || r.u8() != 0) return "trace info: trace metadata must be empty";
  if (r.u8() != 16) return "context: field element size must be 16";
  if (r.off + 16 > r.len) return "truncated context";
  {
    uint64_t m[2];
    memcpy(m, r.p + r.off, 16);
    if (m[0] != P_LO || m[1] != P_HI) return "field modulus in the context is not f128";
    r.off += 16;
  }
  zkl_proof_options& po = c.opts;
  po = zkl_proof_options{};
  po.num_queries = r.u8(); po.blowup_factor = r.u8(); po.grinding_factor = r.u8();
  po.field_extension = r.u8(); po.fri_folding_factor = r.u8(); po.fri_remainder_max_degree = r.u8();
  po.batching_constraints = r.u8(); po.batching_deep = r.u8();
  po.num_partitions = r.u8(); po.hash_rate = r.u8();
  if (want && memcmp(&po, want, sizeof po) != 0) return "proof options in the proof differ from the expected options";
  c.nq = r.u8();
  if (r.bad) return "truncated context";
  return nullptr;
}

inline const char* read_commitments(Rd& r, int nl, fe& troot, fe& croot, std::vector<fe>& fri_roots, fe& rem_commit) {
  Rd cm = r.vec();
  troot = cm.digest();
  croot = cm.digest();
  fri_roots.resize((size_t)nl);
  for (fe& x : fri_roots) x = cm.digest();
  rem_commit = cm.digest();
  if (!cm.done() || r.bad) return "malformed commitments";
  return nullptr;
}

// trace / constraint query values and paths, OOD frame of the trace and of the constraint columns
struct QuerySections { Rd tq_v, tq_p, cq_v, cq_p, ood_ts, ood_es; };
inline const char* read_query_sections(Rd& r, QuerySections& q) {
  if (r.usize() != 1) return "trace queries: exactly one main segment expected";
  q.tq_v = r.vec(); q.tq_p = r.vec(); q.cq_v = r.vec(); q.cq_p = r.vec(); q.ood_ts = r.vec(); q.ood_es = r.vec();
  if (r.bad) return "malformed query / OOD sections";
  return nullptr;
}

struct FriSections { std::vector<Rd> values, paths; Rd remainder; uint64_t nonce = 0; };  // values, paths: per layer
// everything after the OOD frame, to the end of the proof
inline const char* read_fri_sections(Rd& r, int nl, FriSections& f) {
  if ((int)r.usize() != nl) return "FRI layer count mismatch";
  f.values.resize((size_t)nl);
  f.paths.resize((size_t)nl);
  for (int d = 0; d < nl; d++) { f.values[d] = r.vec(); f.paths[d] = r.vec(); }
  f.remainder = r.vec();
  if (r.u8() != 0) return "FRI remainder partitions must be 1";
  f.nonce = r.u64();
  if (!r.done()) return "malformed FRI section or trailing bytes";
  return nullptr;
}

}  // namespace zkl
