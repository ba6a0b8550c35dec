// Segment-proof verifier on the host: the checks of winter-verifier
// 0.13.1 for a ZkLispAir proof, which the reference runs as verify_proof (prove.rs:802-941)
// and, for the aggregation, re-runs piecewise over a step proof's transcript (agg/fs.rs:38-245,
// agg/child.rs:905-1023, agg/trace.rs:697-1260).  Order of checks:
//   context / options, commitments, transcript replay (agg/fs.rs:67-237), out-of-domain
//   constraint identity  H(z) = sum_j H_j(z) z^(j n)
//                             = sum_k alpha_k c_k(z) (z - g^(n-1)) / (z^n - 1)
//                               + sum_a beta_a (t_a(z) - v_a) / (z - g^(s_a)),
//   proof of work, query positions, trace / constraint Merkle openings (row digests under
//   the library's row-digest rule), DEEP values at x = 3 w_N^p (agg/trace.rs:1126-1218),
//   every FRI layer opening and fold (agg/trace.rs:697-955, positions agg/child.rs:1072-1100),
//   the remainder and its commitment.
// The transition constraints c_k(z) come from the same air_transition_sum the device
// evaluator uses (air_eval.h); everything else is independent of the prover's code.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "air_eval.h"
#include "air_host.h"
#include "host_hash.h"
#include "kernels.h"
#include "proof_view.h"

namespace zkl {

bool plan_batch_merkle(Rd& r, size_t n_leaves, const std::vector<size_t>& idx, const std::vector<uint32_t>& leaves,
                       HashPlan& plan, uint32_t* root) {
  // a rejected opening leaves the plan as it was: inputs and nodes are rolled back, merges are
  // committed only at the end
  const size_t in0 = plan.in.size();
  const uint32_t out0 = plan.n_out;
  struct M { size_t h; uint32_t l, r, dst; };
  std::vector<M> mg;
  auto reject = [&] {
    plan.in.resize(in0);
    plan.n_out = out0;
    return false;
  };
  const size_t depth = (size_t)ilog2(n_leaves);
  if (r.u8() != depth) return false;
  const size_t m = r.u8();
  std::vector<std::pair<uint32_t, size_t>> lists(m);  // first node, count
  for (size_t k = 0; k < m && !r.bad; k++) {
    const size_t c = r.u8();
    lists[k] = {(uint32_t)plan.in.size(), c};
    for (size_t j = 0; j < c; j++) {
      const fe d = r.digest();
      plan.add_in(&d, 1);
    }
  }
  if (r.bad) return reject();
  // leaf pairs (even index of each requested leaf), in increasing order
  std::vector<size_t> norm;
  for (size_t i : idx) {
    const size_t b = i & ~(size_t)1;
    if (norm.empty() || norm.back() != b) norm.push_back(b);
  }
  if (norm.size() != m) return reject();
  std::vector<size_t> used(m, 0), cur(m), nxt;
  std::vector<uint32_t> cv(m), nv;
  auto pop = [&](size_t k, uint32_t& out) {
    if (used[k] >= lists[k].second) return false;
    out = lists[k].first + (uint32_t)used[k]++;
    return true;
  };
  auto merge = [&](size_t h, uint32_t l, uint32_t rr) {
    const uint32_t dst = plan.new_out();
    mg.push_back({h, l, rr, dst});
    return dst;
  };
  for (size_t k = 0; k < m; k++) {
    uint32_t v[2];
    for (int t = 0; t < 2; t++) {
      const size_t j = norm[k] + (size_t)t;
      auto it = std::lower_bound(idx.begin(), idx.end(), j);
      if (it != idx.end() && *it == j) v[t] = leaves[(size_t)(it - idx.begin())];
      else if (!pop(k, v[t])) return reject();
    }
    cv[k] = merge(1, v[0], v[1]);
    cur[k] = (norm[k] + n_leaves) >> 1;
  }
  size_t cn = m;
  for (size_t lvl = 1; lvl < depth; lvl++) {
    nxt.clear();
    nv.clear();
    for (size_t i = 0; i < cn; i++) {
      const size_t sib = cur[i] ^ 1;
      uint32_t parent;
      if (i + 1 < cn && cur[i + 1] == sib) {
        parent = merge(lvl + 1, cv[i], cv[i + 1]);
        i++;
      } else {
        uint32_t s;
        if (!pop(i, s)) return reject();
        parent = (cur[i] & 1) ? merge(lvl + 1, s, cv[i]) : merge(lvl + 1, cv[i], s);
      }
      nxt.push_back(sib >> 1);
      nv.push_back(parent);
    }
    cn = nxt.size();
    std::copy(nxt.begin(), nxt.end(), cur.begin());
    std::copy(nv.begin(), nv.end(), cv.begin());
  }
  if (cn != 1 || cur[0] != 1) return reject();
  for (size_t k = 0; k < m; k++)
    if (used[k] != lists[k].second) return reject();  // every proof node consumed
  for (const M& x : mg) plan.add_merge(x.h, x.l, x.r, x.dst);
  *root = cv[0];
  return true;
}

void parallel_for(size_t n, const std::function<void(size_t)>& f) {
  const size_t nt = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(16, std::thread::hardware_concurrency()), n));
  if (nt <= 1) {
    for (size_t i = 0; i < n; i++) f(i);
    return;
  }
  std::atomic<size_t> next{0};
  std::exception_ptr ex;
  std::mutex mu;
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; t++)
    th.emplace_back([&] {
      for (size_t i; (i = next.fetch_add(1)) < n;) {
        try {
          f(i);
        } catch (...) {
          std::lock_guard<std::mutex> lk(mu);
          if (!ex) ex = std::current_exception();
        }
      }
    });
  for (auto& x : th) x.join();
  if (ex) std::rethrow_exception(ex);
}

void run_plan_host(const HashPlan& plan, std::vector<fe>& out, bool par_draws) {
  const Hasher& H = hasher();
  out.assign(plan.n_out, fe_zero());
  auto val = [&](uint32_t i) { return (i & PLAN_OUT) ? out[i & ~PLAN_OUT] : plan.in[i]; };
  std::vector<fe> d;
  for (const HashPlan::RowJob& j : plan.rows) {
    const fe* row = &plan.in[j.src];
    d.clear();
    for (size_t s = 0; s < j.ncols; s += j.psize) d.push_back(H.hash_elements(row + s, std::min<size_t>(j.psize, j.ncols - s)));
    out[j.dst & ~PLAN_OUT] = j.merge ? H.merge_many(d.data(), d.size()) : d[0];
  }
  for (const auto& lvl : plan.merges)
    for (const HashPlan::MergeJob& j : lvl) out[j.dst & ~PLAN_OUT] = H.merge(val(j.left), val(j.right));
  for (const HashPlan::DrawJob& j : plan.draws) {
    fe* o = &out[j.dst & ~PLAN_OUT];
    if (par_draws && j.count >= 4096) {
      // independent draws (~2.9e5 for a 2^16-row segment): host threads
      const size_t nt = 16, chunk = (j.count + nt - 1) / nt;
      parallel_for(nt, [&](size_t t) {
        for (size_t k = t * chunk; k < std::min<size_t>(j.count, (t + 1) * chunk); k++) o[k] = H.merge_with_int(j.seed, k + 1);
      });
    } else {
      for (size_t k = 0; k < j.count; k++) o[k] = H.merge_with_int(j.seed, k + 1);
    }
  }
}

bool batch_merkle_root(Rd& r, size_t n_leaves, const std::vector<size_t>& idx, const std::vector<fe>& leaves,
                       fe* root) {
  HashPlan plan;
  std::vector<uint32_t> ln(leaves.size());
  for (size_t k = 0; k < leaves.size(); k++) ln[k] = plan.add_in(&leaves[k], 1);
  uint32_t rn;
  if (!plan_batch_merkle(r, n_leaves, idx, ln, plan, &rn)) return false;
  std::vector<fe> out;
  run_plan_host(plan, out, false);
  *root = out[rn & ~PLAN_OUT];
  return true;
}

namespace {

size_t partition_size(uint32_t np, uint32_t rate, size_t ncols) {
  if (np <= 1) return ncols;
  const size_t a = (ncols + np - 1) / np;
  return std::max<size_t>(a, rate);
}

// Row jobs of the nrows opened rows at in[src ..) (row-major, ncols each) as commit_to_rows
// hashes them under a one-chunk rule (0: winterfell, 1: hash_row_poseidon of
// agg/child.rs:1025-1045): chunks of psize columns, then merge_many unless the
// row is hashed whole or is one chunk under rule 1.  Returns the digests' nodes.
std::vector<uint32_t> plan_rows(HashPlan& plan, uint32_t src, size_t nrows, size_t ncols, size_t psize, int rule) {
  const size_t np_eff = (ncols + psize - 1) / psize;
  const uint32_t merge = psize != ncols && !(np_eff == 1 && rule == 1);
  std::vector<uint32_t> nodes(nrows);
  for (size_t k = 0; k < nrows; k++) {
    nodes[k] = plan.new_out();
    plan.rows.push_back({src + (uint32_t)(k * ncols), (uint32_t)ncols, (uint32_t)std::min(psize, ncols), merge, nodes[k]});
  }
  return nodes;
}

// The root a batch opening reproduces with hash_row_poseidon leaves (SegmentView::*_root_ref).
// The two rules differ only for a partitioned row of one chunk while the library's rule is 0:
// there the rule-1 leaves and a second decompression of the opening (`proof`: a copy of its
// reader taken before it was consumed) are scheduled and *dst is set once the proof verifies;
// elsewhere it is the committed root.
void plan_reference_root(SegmentReplay& R, Rd proof, size_t N, const std::vector<size_t>& pos, uint32_t src, size_t ncols,
                         size_t psize, int rule, fe committed, fe* dst) {
  *dst = committed;
  const size_t np_eff = (ncols + psize - 1) / psize;
  if (!(rule == 0 && psize != ncols && np_eff == 1)) return;
  const HashPlan::Mark mk = R.plan.mark();
  const std::vector<uint32_t> l1 = plan_rows(R.plan, src, pos.size(), ncols, psize, 1);
  uint32_t root;
  if (!plan_batch_merkle(proof, N, pos, l1, R.plan, &root)) {  // cannot happen: the same bytes were accepted
    R.plan.rewind(mk);
    return;
  }
  R.fixes.push_back({root, dst});
}

constexpr uint32_t CHECK_OOD = PLAN_OUT - 1;

fe transition_sum(const AirInstance& air, const std::vector<fe>& cur, const std::vector<fe>& nxt, const fe* per,
                  fe p_last, const fe* alphas) {
  auto c = [&](int i) { return cur[(size_t)i]; };
  auto x = [&](int i) { return nxt[(size_t)i]; };
  const bool pose = air.dev.pose_block != 0, rm = (air.dev.ram_block | air.dev.merkle_block) != 0;
  if (pose && rm) return air_transition_sum<true, true>(air.dev, c, x, per, p_last, alphas);
  if (pose) return air_transition_sum<true, false>(air.dev, c, x, per, p_last, alphas);
  if (rm) return air_transition_sum<false, true>(air.dev, c, x, per, p_last, alphas);
  return air_transition_sum<false, false>(air.dev, c, x, per, p_last, alphas);
}

}  // namespace

std::string check_proof_options(const zkl_proof_options& o) {
  const auto pow2 = [](uint32_t x) { return x && !(x & (x - 1)); };
  if (o.num_queries < 1 || o.num_queries > 255) return "number of queries must be in 1..255";
  if (!pow2(o.blowup_factor) || o.blowup_factor < 2 || o.blowup_factor > 128)
    return "blowup factor must be a power of two in 2..128";
  if (o.grinding_factor > 32) return "grinding factor must be at most 32";
  if (o.field_extension < 1 || o.field_extension > 3) return "unknown field extension";
  if (o.fri_folding_factor != 2) return "FRI folding factor must be 2";
  if (!pow2(o.fri_remainder_max_degree + 1) || o.fri_remainder_max_degree >= o.blowup_factor)
    return "FRI remainder degree must be 2^k - 1 below the blowup factor";
  if (o.num_partitions < 1 || o.num_partitions > 16) return "number of partitions must be in 1..16";
  if (o.hash_rate < 1 || o.hash_rate > 255) return "hash rate must be in 1..255";
  return "";
}

std::string verify_segment(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi,
                           const zkl_proof_options& opts, SegmentView* out) {
  return verify_segment_ex(proof, len, pi, &opts, out, true);
}

namespace {
std::string replay_impl(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi,
                        const zkl_proof_options* want_opts, bool check_ood, SegmentReplay& R) {
  SegmentView& V = *R.view;
  HashPlan& plan = R.plan;
  const int rule = row_digest_rule();
  const Hasher& H = hasher();
  Rd r{proof, len, 0, false};

  // ---- Context (TraceInfo, field modulus, ProofOptions) + num_unique_queries
  ProofContext cx;
  if (const char* e = read_context(r, want_opts, cx)) return e;
  const uint32_t W = cx.W;
  const unsigned logn = cx.logn;
  const zkl_proof_options& opts = cx.opts;
  {
    const std::string e = check_proof_options(opts);  // options decoded from the proof (winterfell reads them so)
    if (!e.empty()) return "proof options: " + e;
  }
  if (logn < 5 || logn > 30) return "trace length out of range";
  if (opts.field_extension != 1 || opts.fri_folding_factor != 2) return "unsupported proof options";
  const size_t n = (size_t)1 << logn, N = n * opts.blowup_factor;
  AirInstance& air = R.air;
  {
    const std::string e = build_air(pi, W, n, air, check_ood);
    if (!e.empty()) return "AIR construction failed: " + e;
  }
  const int C = air.num_comp_cols;
  const fe g = root_of_unity(logn), wN = root_of_unity(ilog2(N));
  const int nl = fri_num_layers(N, opts.blowup_factor, opts.fri_remainder_max_degree);
  V.width = W; V.n = n; V.lde = N; V.comp_cols = C; V.opts = opts;

  // ---- Commitments
  if (const char* e = read_commitments(r, nl, V.trace_root, V.constraint_root, V.fri_roots, V.remainder_commit)) return e;

  // ---- transcript up to the out-of-domain point
  std::vector<fe> seed = context_elements(W, n, opts);
  {
    const std::vector<fe> pe = pi_elements(pi);
    seed.insert(seed.end(), pe.begin(), pe.end());
  }
  Coin coin{H.hash_elements(seed.data(), seed.size()), 0};
  coin.reseed(V.trace_root);
  // composition coefficients: draw k = merge_with_int(seed, k), k = 1.. (alphas then betas).
  // They are independent, so the ~2.9e5 of a 2^16-row segment become one draw-range job of the
  // plan, scheduled where the identity is checked.  The replay without the out-of-domain
  // identity needs none of them: a reseed follows, and draws only advance the counter the
  // reseed resets (agg/fs.rs:132-138 skips them too).
  const fe draw_seed = coin.seed;
  coin.reseed(V.constraint_root);
  V.z = coin.draw();
  const fe z = V.z, zg = fe_mul(z, g);

  // ---- queries / OOD sections
  QuerySections qs;
  if (const char* e = read_query_sections(r, qs)) return e;
  Rd &tq_v = qs.tq_v, &tq_p = qs.tq_p, &cq_v = qs.cq_v, &cq_p = qs.cq_p, &ood_ts = qs.ood_ts, &ood_es = qs.ood_es;
  if (ood_ts.len != 2 * (size_t)W * 16 || ood_es.len != 2 * (size_t)C * 16) return "OOD frame has the wrong shape";
  read_values(ood_ts, V.ood_trace_z, W);
  read_values(ood_ts, V.ood_trace_zg, W);
  read_values(ood_es, V.ood_comp_z, (size_t)C);
  read_values(ood_es, V.ood_comp_zg, (size_t)C);
  if (ood_ts.bad || ood_es.bad) return "non-canonical OOD values";

  // ---- out-of-domain constraint identity: deferred to finish_replay, over the drawn coefficients
  if (check_ood) {
    const size_t tot = (size_t)air.n_tc + air.assertions.size();
    R.ood_draws = plan.new_out((uint32_t)tot);
    plan.draws.push_back({draw_seed, (uint32_t)tot, R.ood_draws});
    R.checks.push_back({CHECK_OOD, fe_zero(), "out-of-domain constraint identity does not hold"});
  }
  {
    std::vector<fe> oc;  // trace(z) | H(z) | trace(zg) | H(zg)  (agg/fs.rs:152-164)
    oc.insert(oc.end(), V.ood_trace_z.begin(), V.ood_trace_z.end());
    oc.insert(oc.end(), V.ood_comp_z.begin(), V.ood_comp_z.end());
    oc.insert(oc.end(), V.ood_trace_zg.begin(), V.ood_trace_zg.end());
    oc.insert(oc.end(), V.ood_comp_zg.begin(), V.ood_comp_zg.end());
    coin.reseed(H.hash_elements(oc.data(), oc.size()));
  }
  V.deep_coeffs.resize((size_t)W + C);
  for (auto& c : V.deep_coeffs) c = coin.draw();
  V.fri_alphas.resize(nl);
  for (int d = 0; d < nl; d++) { coin.reseed(V.fri_roots[d]); V.fri_alphas[d] = coin.draw(); }
  coin.reseed(V.remainder_commit);

  // ---- FRI proof sections, proof of work
  FriSections fs;
  if (const char* e = read_fri_sections(r, nl, fs)) return e;
  V.pow_nonce = fs.nonce;
  {
    const fe h = H.merge_with_int(coin.seed, V.pow_nonce);
    const unsigned tz = h.lo ? (unsigned)__builtin_ctzll(h.lo) : 64u;
    if (tz < opts.grinding_factor) return "proof-of-work nonce does not meet the grinding factor";
  }

  // ---- query positions: draw_integers(q, N, nonce), sorted, de-duplicated
  query_positions(coin, V.pow_nonce, opts.num_queries, N, V.positions);
  const std::vector<size_t>& pos = V.positions;
  const size_t nq = pos.size();
  if (nq != cx.nq) return "num_unique_queries does not match the drawn positions";

  // ---- trace and constraint openings
  if (tq_v.len != nq * W * 16 || cq_v.len != nq * (size_t)C * 16) return "query value sections have the wrong size";
  read_values(tq_v, V.trace_rows, nq * W);
  read_values(cq_v, V.comp_rows, nq * (size_t)C);
  if (tq_v.bad || cq_v.bad) return "non-canonical query values";
  {
    uint32_t root;
    const Rd tq_p0 = tq_p, cq_p0 = cq_p;
    size_t ps = partition_size(opts.num_partitions, opts.hash_rate, W);
    HashPlan::Mark mk = plan.mark();
    uint32_t src = plan.add_in(V.trace_rows.data(), V.trace_rows.size());
    if (!plan_batch_merkle(tq_p, N, pos, plan_rows(plan, src, nq, W, ps, rule), plan, &root) || !tq_p.done()) {
      plan.rewind(mk);
      return "trace Merkle opening does not reproduce the trace commitment";
    }
    R.checks.push_back({root, V.trace_root, "trace Merkle opening does not reproduce the trace commitment"});
    plan_reference_root(R, tq_p0, N, pos, src, W, ps, rule, V.trace_root, &V.trace_root_ref);
    ps = partition_size(opts.num_partitions, opts.hash_rate, (size_t)C);
    mk = plan.mark();
    src = plan.add_in(V.comp_rows.data(), V.comp_rows.size());
    if (!plan_batch_merkle(cq_p, N, pos, plan_rows(plan, src, nq, (size_t)C, ps, rule), plan, &root) || !cq_p.done()) {
      plan.rewind(mk);
      return "constraint Merkle opening does not reproduce the constraint commitment";
    }
    R.checks.push_back({root, V.constraint_root, "constraint Merkle opening does not reproduce the constraint commitment"});
    plan_reference_root(R, cq_p0, N, pos, src, (size_t)C, ps, rule, V.constraint_root, &V.constraint_root_ref);
  }

  // ---- DEEP composition at the query positions
  std::vector<fe> evals(nq);
  {
    const std::vector<fe>& gam = V.deep_coeffs;
    fe sz = fe_zero(), szg = fe_zero();
    for (uint32_t c = 0; c < W; c++) {
      sz = fe_add(sz, fe_mul(gam[c], V.ood_trace_z[c]));
      szg = fe_add(szg, fe_mul(gam[c], V.ood_trace_zg[c]));
    }
    for (int j = 0; j < C; j++) {
      sz = fe_add(sz, fe_mul(gam[W + j], V.ood_comp_z[j]));
      szg = fe_add(szg, fe_mul(gam[W + j], V.ood_comp_zg[j]));
    }
    for (size_t k = 0; k < nq; k++) {
      const fe x = fe_mul(fe{3, 0}, fe_pow64(wN, pos[k]));
      fe s = fe_zero();
      for (uint32_t c = 0; c < W; c++) s = fe_add(s, fe_mul(gam[c], V.trace_rows[k * W + c]));
      for (int j = 0; j < C; j++) s = fe_add(s, fe_mul(gam[W + j], V.comp_rows[k * C + j]));
      evals[k] = fe_add(fe_mul(fe_sub(s, sz), fe_inv(fe_sub(x, z))), fe_mul(fe_sub(s, szg), fe_inv(fe_sub(x, zg))));
    }
  }

  // ---- FRI: layer openings, folds, remainder
  size_t Nd = N;
  const fe inv2 = fe_inv(fe{2, 0}), three{3, 0};
  V.fri_folds.assign(nl, {});
  V.fri_values.assign(nl, {});
  std::vector<std::pair<size_t, uint32_t>> sorted;  // (folded position, its index in np)
  for (int d = 0; d < nl; d++) {
    const size_t h = Nd / 2;
    const std::vector<size_t>& fpos = d ? V.fri_folds[d - 1].pos : pos;
    fold_positions(fpos, h, V.fri_folds[d]);
    const std::vector<size_t>& np = V.fri_folds[d].pos;
    const std::vector<uint32_t>& slot = V.fri_folds[d].slot;
    const size_t m = np.size();
    if (fs.values[d].len != m * 32) return "FRI layer values have the wrong size";
    std::vector<fe>& lv = V.fri_values[d];
    read_values(fs.values[d], lv, 2 * m);
    if (fs.values[d].bad) return "non-canonical FRI layer values";
    for (size_t k = 0; k < fpos.size(); k++)
      if (!fe_eq(lv[2 * slot[k] + (fpos[k] >= h ? 1 : 0)], evals[k])) return "FRI layer opening disagrees with the folded values";
    {
      sorted_fold(np, sorted);
      const HashPlan::Mark mk = plan.mark();
      const uint32_t src = plan.add_in(lv.data(), lv.size());
      std::vector<size_t> sp(m);
      std::vector<uint32_t> sl(m);  // leaf k: hash_elements of the value pair of sorted position k
      for (size_t k = 0; k < m; k++) {
        sp[k] = sorted[k].first;
        sl[k] = plan.new_out();
        plan.rows.push_back({src + 2 * sorted[k].second, 2, 2, 0, sl[k]});
      }
      uint32_t root;
      if (!plan_batch_merkle(fs.paths[d], h, sp, sl, plan, &root) || !fs.paths[d].done()) {
        plan.rewind(mk);
        return "FRI layer Merkle opening does not reproduce the layer commitment";
      }
      R.checks.push_back({root, V.fri_roots[d], "FRI layer Merkle opening does not reproduce the layer commitment"});
    }
    // fold: (v0 + v1)/2 + alpha (v0 - v1) / (2 x0), x0 = 3 w_Nd^y
    const fe gd = root_of_unity(ilog2(Nd));
    std::vector<fe> next(m);
    for (size_t j = 0; j < m; j++) {
      const fe v0 = lv[2 * j], v1 = lv[2 * j + 1];
      const fe x0 = fe_mul(three, fe_pow64(gd, np[j]));
      next[j] = fe_mul(fe_add(fe_add(v0, v1), fe_mul(V.fri_alphas[d], fe_mul(fe_sub(v0, v1), fe_inv(x0)))), inv2);
    }
    evals.swap(next);
    Nd = h;
  }
  const std::vector<size_t>& fpos = nl ? V.fri_folds[nl - 1].pos : pos;
  const size_t rlen = opts.fri_remainder_max_degree + 1;
  if (fs.remainder.len != rlen * 16) return "FRI remainder has the wrong size";
  read_values(fs.remainder, V.remainder, rlen);
  if (fs.remainder.bad) return "non-canonical remainder";
  if (!fe_eq(H.hash_elements(V.remainder.data(), rlen), V.remainder_commit)) return "remainder does not match its commitment";
  const fe gr = root_of_unity(ilog2(Nd));
  for (size_t k = 0; k < fpos.size(); k++) {
    const fe x = fe_mul(three, fe_pow64(gr, fpos[k]));
    fe v = fe_zero(), xp = fe_one();
    for (size_t c = 0; c < rlen; c++) { v = fe_add(v, fe_mul(V.remainder[rlen - 1 - c], xp)); xp = fe_mul(xp, x); }
    if (!fe_eq(v, evals[k])) return "FRI remainder does not match the last layer";
  }
  return "";
}

// the out-of-domain constraint identity of a replayed proof, given its composition coefficients
bool ood_identity_holds(const AirInstance& air, const SegmentView& V, const fe* alphas, const fe* betas) {
  const size_t n = V.n;
  const int C = V.comp_cols;
  const fe z = V.z, g = root_of_unity((unsigned)ilog2(n));
  std::vector<fe> per = periodic_at(n, z);
  const fe gl = fe_pow64(g, n - 1), zn = fe_pow64(z, n);
  const fe p_last = fe_mul(fe_mul(gl, fe_sub(zn, fe_one())), fe_inv(fe_mul(fe{n, 0}, fe_sub(z, gl))));
  fe t = transition_sum(air, V.ood_trace_z, V.ood_trace_zg, per.data(), p_last, alphas);
  t = fe_mul(fe_mul(t, fe_sub(z, gl)), fe_inv(fe_sub(zn, fe_one())));
  // boundary: groups of assertions at one step share the divisor (z - g^step); batch-inverted
  std::vector<fe> num, den;
  for (size_t a = 0; a < air.assertions.size();) {
    size_t e = a;
    fe s = fe_zero();
    for (; e < air.assertions.size() && air.assertions[e].step == air.assertions[a].step; e++)
      s = fe_add(s, fe_mul(betas[e], fe_sub(V.ood_trace_z[air.assertions[e].col], air.assertions[e].value)));
    num.push_back(s);
    den.push_back(fe_sub(z, fe_pow64(g, air.assertions[a].step)));
    a = e;
  }
  std::vector<fe> pre(den.size());
  fe acc = fe_one();
  for (size_t i = 0; i < den.size(); i++) { pre[i] = acc; acc = fe_mul(acc, den[i]); }
  fe inv = fe_inv(acc), b = fe_zero();
  for (size_t i = den.size(); i-- > 0;) {
    b = fe_add(b, fe_mul(num[i], fe_mul(inv, pre[i])));
    inv = fe_mul(inv, den[i]);
  }
  fe h = fe_zero(), zjn = fe_one();
  for (int j = 0; j < C; j++) { h = fe_add(h, fe_mul(V.ood_comp_z[j], zjn)); zjn = fe_mul(zjn, zn); }
  return fe_eq(fe_add(t, b), h);
}

}  // namespace

void replay_segment(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi, const zkl_proof_options* opts,
                    SegmentView* view, bool check_ood, SegmentReplay& R) {
  R.view = view ? view : &R.local;
  R.host_err = replay_impl(proof, len, pi, opts, check_ood, R);
  // only the out-of-domain identity reads the assertions (~2.9e5, 9 MB at 2^16 rows): a batch
  // keeps a wave of replays alive until its hashes are back
  if (!check_ood) std::vector<Assertion>().swap(R.air.assertions);
}

std::string finish_replay(SegmentReplay& R, const fe* out) {
  for (const SegmentReplay::Check& c : R.checks) {
    if (c.node == CHECK_OOD) {
      const fe* al = out + (R.ood_draws & ~PLAN_OUT);
      if (!ood_identity_holds(R.air, *R.view, al, al + R.air.n_tc)) return c.msg;
    } else if (!fe_eq(out[c.node & ~PLAN_OUT], c.want)) {
      return c.msg;
    }
  }
  if (!R.host_err.empty()) return R.host_err;
  for (const SegmentReplay::Fix& f : R.fixes) *f.dst = out[f.node & ~PLAN_OUT];
  return "";
}

std::string verify_segment_ex(const uint8_t* proof, size_t len, const zkl_air_public_inputs& pi,
                              const zkl_proof_options* want_opts, SegmentView* out, bool check_ood) {
  SegmentReplay R;
  replay_segment(proof, len, pi, want_opts, out, check_ood, R);
  std::vector<fe> res;
  run_plan_host(R.plan, res, true);
  return finish_replay(R, res.data());
}

PlanExec host_plan_exec() {
  auto keep = std::make_shared<std::vector<std::vector<fe>>>();
  return [keep](const HashPlan* const* plans, size_t n, const fe** outs) {
    keep->resize(n);
    parallel_for(n, [&](size_t i) { run_plan_host(*plans[i], (*keep)[i], n == 1); });
    for (size_t i = 0; i < n; i++) outs[i] = (*keep)[i].data();
  };
}

void verify_segments_batch(const BatchItem* items, size_t n, bool check_ood, const PlanExec& exec, size_t cap,
                           std::string* errs, double* ms) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  // a wave of proofs is planned on host threads, then submitted in groups of bounded size (field
  // elements of input + output: at 2^16 rows a child is ~3e4, a proof with the out-of-domain
  // identity ~3e5 more), which bounds the staging memory whatever the batch size
  const size_t wave = check_ood ? 16 : 64;
  for (size_t w0 = 0; w0 < n; w0 += wave) {
    const size_t wn = std::min(wave, n - w0);
    std::vector<SegmentReplay> R(wn);
    clk::time_point t0 = clk::now();
    parallel_for(wn, [&](size_t i) {
      const BatchItem& it = items[w0 + i];
      replay_segment(it.proof, it.len, *it.pi, it.opts, it.view, check_ood, R[i]);
    });
    if (ms) ms[0] += since(t0);
    for (size_t g0 = 0; g0 < wn;) {
      size_t g1 = g0, tot = 0;
      do {
        tot += R[g1].plan.in.size() + R[g1].plan.n_out;
        g1++;
      } while (g1 < wn && (!cap || tot + R[g1].plan.in.size() + R[g1].plan.n_out <= cap));
      std::vector<const HashPlan*> plans;
      for (size_t i = g0; i < g1; i++) plans.push_back(&R[i].plan);
      std::vector<const fe*> outs(plans.size());
      t0 = clk::now();
      exec(plans.data(), plans.size(), outs.data());
      if (ms) ms[1] += since(t0);
      t0 = clk::now();
      parallel_for(g1 - g0, [&](size_t i) {
        errs[w0 + g0 + i] = finish_replay(R[g0 + i], outs[i]);
        R[g0 + i] = SegmentReplay();  // released here, on the threads, not at the end of the wave
      });
      if (ms) ms[0] += since(t0);
      g0 = g1;
    }
  }
}

}  // namespace zkl
