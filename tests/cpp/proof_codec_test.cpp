// Host test of the proof codec (zk-lisp_amd/csrc/proof_codec.h), no library and no device:
//   * a synthetic proof (W 3, 32 rows, blowup 4, 2 composition columns, 5 query positions with an
//     adjacent pair and a pair that folds together) written through ProofWriter and read back
//     through the reader steps, every field compared, over the base field and the quadratic
//     extension; a trailing byte, a cut context, a changed partitions byte and a non-canonical
//     element are refused with their message;
//   * fold_positions against a plain quadratic restatement (pos and slot) over seeded position
//     sets of 1..255 positions and h = 2^1..2^16;
//   * query_positions against sort + unique.
//   proof_codec_test [position sets, default 10000]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../zk-lisp_amd/csrc/agg_air.h"
#include "../../zk-lisp_amd/csrc/proof_codec.h"

using namespace zkl;

static int g_fail = 0;
#define CHECK(c, ...)                                        \
  do {                                                       \
    if (!(c)) {                                              \
      if (g_fail++ < 20) {                                   \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                        \
        fprintf(stderr, "\n");                               \
      }                                                      \
    }                                                        \
  } while (0)

static uint64_t g_rng = 0x5EEDC0DEC0DEull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static fe rnd_fe() { return fe{rnd(), rnd() >> 1}; }  // hi < 2^63 < P_HI: canonical
template <class T> T rnd_e();
template <> fe rnd_e<fe>() { return rnd_fe(); }
template <> fe2 rnd_e<fe2>() { const fe a = rnd_fe(); return fe2{a, rnd_fe()}; }
template <class T>
static std::vector<T> rnd_vec(size_t n) {
  std::vector<T> v(n);
  for (auto& x : v) x = rnd_e<T>();
  return v;
}
static bool same(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }
template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && same(a.data(), b.data(), a.size() * sizeof(T));
}
static std::string str(const char* e) { return e ? e : ""; }

// the digest the synthetic trees hold at a node
static fe node_digest(int tree, uint64_t node) { return fe{node * 0x100000001B3ull + 7, (uint64_t)tree}; }

// reads a BatchMerkleProof section back and compares it with the plan it was written from
static void check_multiproof(Rd s, const Plan& plan, int depth, int tree, const char* what) {
  CHECK(s.u8() == depth, "%s: depth", what);
  CHECK(s.u8() == plan.len.size(), "%s: list count", what);
  size_t i = 0;
  for (uint32_t l : plan.len) {
    CHECK(s.u8() == l, "%s: list length", what);
    for (uint32_t k = 0; k < l; k++, i++) {
      const fe d = s.digest(), want = node_digest(tree, plan.node[i]);
      CHECK(same(&d, &want, sizeof d), "%s: digest %zu", what, i);
    }
  }
  CHECK(i == plan.node.size() && s.done(), "%s: length", what);
}

template <class T>
static void round_trip(uint32_t ext) {
  const uint32_t W = 3;
  const int logn = 5;
  const size_t B = 4, N = ((size_t)1 << logn) * B, Cc = 2;
  zkl_proof_options o{};
  o.num_queries = 6; o.blowup_factor = (uint32_t)B; o.grinding_factor = 3; o.field_extension = ext;
  o.fri_folding_factor = 2; o.fri_remainder_max_degree = 1; o.batching_constraints = 0; o.batching_deep = 0;
  o.num_partitions = 1; o.hash_rate = 8;
  const int nl = fri_num_layers(N, B, o.fri_remainder_max_degree);
  CHECK(nl == 4, "layers of 128 down to 8: %d", nl);
  const std::vector<size_t> pos = {6, 7, 20, 70, 101};  // 6, 7 adjacent; 6 and 70 fold together
  const size_t nq = pos.size();
  const int logN = ilog2(N);

  const fe troot = rnd_fe(), croot = rnd_fe(), rem_commit = rnd_fe();
  const std::vector<fe> fri_roots = rnd_vec<fe>((size_t)nl), trows = rnd_vec<fe>(nq * W);
  const std::vector<T> crows = rnd_vec<T>(nq * Cc), tz = rnd_vec<T>(W), tzg = rnd_vec<T>(W), hz = rnd_vec<T>(Cc),
                       hzg = rnd_vec<T>(Cc), rem = rnd_vec<T>(2);
  const uint64_t nonce = rnd();
  std::vector<FoldStep> folds((size_t)nl);
  std::vector<Plan> fplans((size_t)nl);
  std::vector<std::vector<T>> lvals((size_t)nl);

  Bytes P;
  ProofWriter w{P};
  w.context(W, logn, o, nq);
  w.commitments(troot, croot, fri_roots, rem_commit);
  Plan tplan;
  batch_plan_into(N, pos.data(), pos.size(), tplan);
  w.queries();
  w.values(trows.data(), trows.size());
  w.multiproof(tplan, logN, [&](size_t i) { return node_digest(0, tplan.node[i]); });
  w.values(crows.data(), crows.size());
  w.multiproof(tplan, logN, [&](size_t i) { return node_digest(1, tplan.node[i]); });
  w.ood(tz.data(), tzg.data(), W, hz.data(), hzg.data(), Cc);
  w.fri_layers(nl);
  for (int d = 0; d < nl; d++) {
    const size_t h = (N >> d) / 2;
    fold_positions(d ? folds[d - 1].pos : pos, h, folds[d]);
    batch_plan_into(h, folds[d].pos.data(), folds[d].pos.size(), fplans[d]);
    lvals[d] = rnd_vec<T>(2 * folds[d].pos.size());
    const Plan& fp = fplans[d];
    w.values(lvals[d].data(), lvals[d].size());
    w.multiproof(fp, ilog2(h), [&, d](size_t i) { return node_digest(2 + d, fp.node[i]); });
  }
  CHECK(folds[0].pos.size() == 4 && folds[0].slot[0] == 0 && folds[0].slot[3] == 0, "6 and 70 share a slot of layer 0");
  w.remainder(rem.data(), rem.size());
  w.finish(nonce);

  // ---- read back
  Rd r{P.v.data(), P.v.size(), 0, false};
  ProofContext cx;
  CHECK(str(read_context(r, &o, cx)).empty(), "context");
  CHECK(cx.W == W && cx.logn == (unsigned)logn && cx.nq == nq && same(&cx.opts, &o, sizeof o), "context fields");
  fe g_troot, g_croot, g_rem;
  std::vector<fe> g_roots;
  CHECK(str(read_commitments(r, nl, g_troot, g_croot, g_roots, g_rem)).empty(), "commitments");
  CHECK(same(&g_troot, &troot, 16) && same(&g_croot, &croot, 16) && same(&g_rem, &rem_commit, 16) && same(g_roots, fri_roots),
        "commitment fields");
  QuerySections qs;
  CHECK(str(read_query_sections(r, qs)).empty(), "query sections");
  std::vector<fe> got_f;
  std::vector<T> got;
  CHECK(qs.tq_v.len == trows.size() * 16, "trace rows: length");
  read_values(qs.tq_v, got_f, trows.size());
  CHECK(qs.tq_v.done() && same(got_f, trows), "trace rows");
  check_multiproof(qs.tq_p, tplan, logN, 0, "trace paths");
  CHECK(qs.cq_v.len == crows.size() * sizeof(T), "constraint rows: length");
  read_values(qs.cq_v, got, crows.size());
  CHECK(qs.cq_v.done() && same(got, crows), "constraint rows");
  check_multiproof(qs.cq_p, tplan, logN, 1, "constraint paths");
  CHECK(qs.ood_ts.len == 2 * W * sizeof(T) && qs.ood_es.len == 2 * Cc * sizeof(T), "OOD frame: length");
  read_values(qs.ood_ts, got, W);
  CHECK(same(got, tz), "t(z)");
  read_values(qs.ood_ts, got, W);
  CHECK(same(got, tzg) && qs.ood_ts.done(), "t(zg)");
  read_values(qs.ood_es, got, Cc);
  CHECK(same(got, hz), "H(z)");
  read_values(qs.ood_es, got, Cc);
  CHECK(same(got, hzg) && qs.ood_es.done(), "H(zg)");
  FriSections fs;
  CHECK(str(read_fri_sections(r, nl, fs)).empty(), "FRI sections");
  for (int d = 0; d < nl; d++) {
    CHECK(fs.values[d].len == lvals[d].size() * sizeof(T), "layer %d values: length", d);
    read_values(fs.values[d], got, lvals[d].size());
    CHECK(fs.values[d].done() && same(got, lvals[d]), "layer %d values", d);
    check_multiproof(fs.paths[d], fplans[d], ilog2((N >> d) / 2), 2 + d, "layer paths");
  }
  read_values(fs.remainder, got, rem.size());
  CHECK(fs.remainder.done() && same(got, rem) && fs.nonce == nonce, "remainder and nonce");

  // ---- what the reader refuses
  {
    zkl_proof_options other = o;
    other.num_queries++;
    Rd r2{P.v.data(), P.v.size(), 0, false};
    CHECK(str(read_context(r2, &other, cx)) == "proof options in the proof differ from the expected options", "options");
    Rd r3{P.v.data(), 20, 0, false};
    CHECK(str(read_context(r3, nullptr, cx)) == "truncated context", "cut context");
    std::vector<uint8_t> more(P.v);
    more.push_back(0);
    Rd r4{more.data(), more.size(), 0, false};
    CHECK(!read_context(r4, &o, cx) && !read_commitments(r4, nl, g_troot, g_croot, g_roots, g_rem) && !read_query_sections(r4, qs), "prefix of the longer proof");
    CHECK(str(read_fri_sections(r4, nl, fs)) == "malformed FRI section or trailing bytes", "trailing byte");
    more.pop_back();
    more[more.size() - 9] = 1;
    Rd r5{more.data(), more.size(), 0, false};
    CHECK(!read_context(r5, &o, cx) && !read_commitments(r5, nl, g_troot, g_croot, g_roots, g_rem) && !read_query_sections(r5, qs), "prefix, partitions byte 1");
    CHECK(str(read_fri_sections(r5, nl, fs)) == "FRI remainder partitions must be 1", "partitions byte 1");
    Rd r6{P.v.data(), P.v.size(), 0, false};
    CHECK(!read_context(r6, &o, cx) && str(read_commitments(r6, nl + 1, g_troot, g_croot, g_roots, g_rem)) == "malformed commitments", "layer count");
    uint8_t ones[sizeof(T)];
    memset(ones, 0xFF, sizeof ones);
    Rd r7{ones, sizeof ones, 0, false};
    read_e<T>(r7);
    CHECK(r7.bad, "an all-ones element is not canonical");
  }
}

// fold_positions as the verifiers had it: a linear search per position
static void fold_reference(const std::vector<size_t>& prev, size_t h, std::vector<size_t>& pos, std::vector<uint32_t>& slot) {
  pos.clear();
  slot.clear();
  for (size_t x : prev) {
    size_t j = 0;
    while (j < pos.size() && pos[j] != x % h) j++;
    if (j == pos.size()) pos.push_back(x % h);
    slot.push_back((uint32_t)j);
  }
}

int main(int argc, char** argv) {
  const long sets = argc > 1 ? atol(argv[1]) : 10000;
  round_trip<fe>(1);
  round_trip<fe2>(2);

  FoldStep f;
  std::vector<size_t> prev, pos;
  std::vector<uint32_t> slot;
  size_t most = 0;
  for (long t = 0; t < sets; t++) {
    const size_t nq = 1 + (size_t)(t % 255), h = (size_t)1 << (1 + rnd() % 16);
    // positions of the layer above (below 2h); every fourth set from a narrow range, so that
    // most positions collide
    const size_t range = t % 4 == 3 ? std::min<size_t>(2 * h, 1 + rnd() % 64) : 2 * h;
    prev.resize(nq);
    for (auto& x : prev) x = (size_t)(rnd() % range);
    fold_positions(prev, h, f);
    fold_reference(prev, h, pos, slot);
    CHECK(f.pos == pos && f.slot == slot, "fold_positions: set %ld (nq %zu, h %zu)", t, nq, h);
    most = std::max(most, f.pos.size());
  }
  CHECK(sets < 1000 || most >= 250, "no large folded set was tried (%zu)", most);
  prev.assign(257, 0);
  bool threw = false;
  try { fold_positions(prev, 2, f); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw, "more than 256 positions must be refused");

  for (long t = 0; t < sets / 10 + 1; t++) {
    const size_t q = 1 + (size_t)(rnd() % 255), N = (size_t)1 << (3 + rnd() % 28);
    std::vector<fe> draws(q);
    for (auto& d : draws) d = fe{rnd(), rnd()};
    std::vector<size_t> want;
    for (auto& d : draws) want.push_back((size_t)(d.lo % N));
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    query_positions(draws.data(), q, N, pos);
    CHECK(pos == want, "query_positions: set %ld", t);
  }

  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok proof codec: round trip over both fields, %ld position sets (largest folded set %zu)\n", sets, most);
  return 0;
}
