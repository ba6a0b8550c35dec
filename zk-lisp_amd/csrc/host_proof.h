// Host pieces shared by the provers (prover.cpp, agg.cpp) and the verifiers (verifier.cpp,
// agg.cpp): the Fiat-Shamir coin, the winter-utils byte writer and reader and the
// MerkleTree::prove_batch index plan.  All follow winterfell 0.13.1 [WF-recall]; the transcript
// order they serve is pinned by agg/fs.rs:67-237.  The layout of Proof::to_bytes over them is
// proof_codec.h.
#pragma once
#include <string.h>

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <vector>

#include "field.h"
#include "host_hash.h"

namespace zkl {

inline int ilog2(size_t n) { int k = 0; while (((size_t)1 << k) < n) k++; return k; }

// DefaultRandomCoin<PoseidonHasher>: draw = merge_with_int(seed, ++counter) (a Poseidon
// digest value is canonical, so the first try is always accepted)
struct Coin {
  fe seed;
  uint64_t counter = 0;
  void reseed(fe d) { seed = hasher().merge(seed, d); counter = 0; }
  fe draw() { return hasher().merge_with_int(seed, ++counter); }
};

// winter-utils ByteWriter
struct Bytes {
  std::vector<uint8_t> v;
  void u8(uint8_t x) { v.push_back(x); }
  void raw(const void* p, size_t n) {
    const size_t o = v.size();
    v.resize(o + n);
    memcpy(v.data() + o, p, n);
  }
  void u16(uint16_t x) { raw(&x, 2); }  // little-endian host (x86-64 / gfx950 hosts)
  void u32(uint32_t x) { raw(&x, 4); }
  void u64(uint64_t x) { raw(&x, 8); }
  void usize(uint64_t x) {  // winter-utils write_usize (vint64)
    int lz = x ? __builtin_clzll(x) : 64;
    int l = (lz > 0 ? lz - 1 : 0) / 7;
    int len = 9 - std::min(l, 8);
    if (len == 9) { u8(0); u64(x); return; }
    uint64_t enc = ((x << 1) | 1) << (len - 1);
    raw(&enc, (size_t)len);
  }
  void felem(fe x) {
    const uint64_t w[2] = {x.lo, x.hi};
    raw(w, 16);
  }
  void digest(fe x) {
    const uint64_t w[4] = {x.lo, x.hi, 0, 0};
    raw(w, 32);
  }
};

// winter-utils ByteReader over a byte slice; `bad` latches on any overrun or non-canonical value
struct Rd {
  const uint8_t* p = nullptr;
  size_t len = 0, off = 0;
  bool bad = false;
  uint8_t u8() {
    if (off + 1 > len) { bad = true; return 0; }
    return p[off++];
  }
  uint64_t u64() {
    if (off + 8 > len) { bad = true; return 0; }
    uint64_t v;
    memcpy(&v, p + off, 8);
    off += 8;
    return v;
  }
  uint64_t usize() {  // vint64 (ByteReader::read_usize)
    if (off >= len) { bad = true; return 0; }
    const uint8_t b0 = p[off];
    if (b0 == 0) { off++; return u64(); }
    const int l = __builtin_ctz(b0) + 1;
    if (off + (size_t)l > len) { bad = true; return 0; }
    uint64_t enc = 0;
    memcpy(&enc, p + off, (size_t)l);
    off += (size_t)l;
    return enc >> l;
  }
  fe felem() {  // 16-byte LE canonical element
    if (off + 16 > len) { bad = true; return fe_zero(); }
    fe v;
    memcpy(&v.lo, p + off, 8);
    memcpy(&v.hi, p + off + 8, 8);
    off += 16;
    if (v.hi > P_HI || (v.hi == P_HI && v.lo >= P_LO)) bad = true;
    return v;
  }
  fe digest() {  // 32-byte digest: value + 16 zero bytes
    const fe v = felem();
    if (off + 16 > len) { bad = true; return v; }
    for (int i = 0; i < 16; i++) bad |= p[off + (size_t)i] != 0;
    off += 16;
    return v;
  }
  Rd vec() {  // length-prefixed sub-slice
    Rd s;
    const uint64_t l = usize();
    if (bad || off + l > len) { bad = true; s.bad = true; return s; }
    s.p = p + off;
    s.len = (size_t)l;
    off += (size_t)l;
    return s;
  }
  bool done() const { return !bad && off == len; }
};

// MerkleTree::prove_batch node-index plan: per normalized leaf pair, the tree-node indices
// whose digests go into the BatchMerkleProof (leaves are tree nodes n + i)
struct Plan {
  std::vector<uint64_t> node;  // the lists back to back
  std::vector<uint32_t> len;   // entries per list
};
// plan of idx[0..Q) into P (its vectors keep their capacity across calls: no allocation in the
// steady state).  Q <= 256 (ProofOptions' num_queries is a byte).
inline void batch_plan_into(size_t n_leaves, const size_t* idx, size_t Q, Plan& P) {
  if (Q > 256) throw std::invalid_argument("batch_plan: more than 256 query positions");
  const int depth = ilog2(n_leaves);
  // normalised leaf pairs (sorted, unique) and the requested leaves (sorted)
  size_t norm[256], req[256], cur[256], nxt[256];
  uint32_t cnt[256];
  for (size_t k = 0; k < Q; k++) { norm[k] = idx[k] & ~(size_t)1; req[k] = idx[k]; }
  std::sort(norm, norm + Q);
  const size_t L = (size_t)(std::unique(norm, norm + Q) - norm);
  std::sort(req, req + Q);
  // list k takes at most two leaves and one node per level: fixed-stride scratch, compacted
  const size_t stride = (size_t)depth + 2;
  P.node.resize(L * stride);
  uint64_t* tmp = P.node.data();
  size_t r = 0;  // req and norm are both ascending: one merge pass finds the requested leaves
  for (size_t k = 0; k < L; k++) {
    cnt[k] = 0;
    for (size_t j = norm[k]; j < norm[k] + 2; j++) {
      while (r < Q && req[r] < j) r++;
      if (!(r < Q && req[r] == j)) tmp[k * stride + cnt[k]++] = n_leaves + j;
    }
    cur[k] = (norm[k] + n_leaves) >> 1;
  }
  size_t nc = L;
  size_t *a = cur, *b = nxt;
  for (int lvl = 1; lvl < depth; lvl++) {
    size_t nn = 0;
    for (size_t i = 0; i < nc; i++) {
      const size_t sib = a[i] ^ 1;
      if (i + 1 < nc && a[i + 1] == sib) i++;
      else tmp[i * stride + cnt[i]++] = sib;
      b[nn++] = sib >> 1;
    }
    std::swap(a, b);
    nc = nn;
  }
  // compact the lists in place (list k starts at or after where it is moved to)
  P.len.assign(cnt, cnt + L);
  size_t o = 0;
  for (size_t k = 0; k < L; k++) {
    memmove(tmp + o, tmp + k * stride, cnt[k] * sizeof(uint64_t));
    o += cnt[k];
  }
  P.node.resize(o);
}

}  // namespace zkl
