// Device backend of the ZlAggAir prover: the arrays of agg.cpp's prove_air<T>
// computed on a context's device, in the base field (E = fe) or the quadratic extension
// (E = fe2, agg_air.h).  The proof is a 31-column trace of 8 .. 8192 rows: every kernel here is
// latency-bound, so each is one thread per point over canonical field.h arithmetic, and the
// transforms are a plain radix-2 pass per launch (sizes from 8 points, below what the segment
// prover's NTT launchers take).  Hashing goes through the launchers of poseidon.hip.
//
// Layouts.  An E-valued vector of M points is stored as X = 1 or 2 base-field planes of M
// elements (an NTT over E is the base NTT on each plane: the twiddles are base elements).
// Composition LDE: column-major 2 Cc base columns (h0.a, h0.b, h1.a, h1.b) of N rows, so a row is
// the flattened E row the commitment hashes.  FRI layer of Nd points, h = Nd / 2: 2 X columns
// of h rows (lo.a, lo.b, hi.a, hi.b) with lo = e_i, hi = e_{i+h}, so row i is the leaf
// (e_i, e_{i+h}) flattened.  All three go to launch_hash_rows as one-partition matrices.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "agg_backend.h"
#include "host_proof.h"
#include "kernels.h"

namespace zkl {
namespace {

constexpr unsigned TPB = 256;
// every kernel is launched with TPB threads: the bound gives each lane the full register budget
// (without it the compiler plans for 1024-thread blocks and the E = fe2 kernels spill to scratch,
// which tests/test_abi.py refuses outside the listed evaluator kernels)
#define AGG_KERNEL __launch_bounds__(256)
inline unsigned blocks_for(size_t items) { return (unsigned)((items + TPB - 1) / TPB); }

__device__ inline size_t gid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

// ---- E <-> planes / FRI layout ------------------------------------------------------------
__device__ inline void st_planes(fe* base, size_t stride, size_t i, fe v) { (void)stride; base[i] = v; }
__device__ inline void st_planes(fe* base, size_t stride, size_t i, fe2 v) { base[i] = v.a; base[stride + i] = v.b; }
template <class E> __device__ inline E ld_cols(const fe* m, size_t ld, uint32_t j, size_t i);
template <> __device__ inline fe ld_cols<fe>(const fe* m, size_t ld, uint32_t j, size_t i) { return m[(size_t)j * ld + i]; }
template <> __device__ inline fe2 ld_cols<fe2>(const fe* m, size_t ld, uint32_t j, size_t i) {
  return fe2{m[(size_t)(2 * j) * ld + i], m[(size_t)(2 * j + 1) * ld + i]};
}
// element i of a FRI layer of Nd points (i < Nd)
template <class E> __device__ inline E fri_load(const fe* base, size_t Nd, size_t i) {
  const size_t h = Nd / 2, half = i >= h ? 1 : 0;
  return ld_cols<E>(base, h, (uint32_t)half, i - half * h);
}
template <class E> __device__ inline void fri_store(fe* base, size_t Nd, size_t i, E v) {
  const size_t h = Nd / 2, half = i >= h ? 1 : 0;
  constexpr size_t X = sizeof(E) / sizeof(fe);
  st_planes(base + half * X * h, h, i - half * h, v);
}

// ---- transforms ---------------------------------------------------------------------------
// out[i] = w^i, i < M
__global__ AGG_KERNEL void agg_roots_kernel(fe w, size_t M, fe* out) {
  const size_t i = gid();
  if (i >= M) return;
  out[i] = fe_pow64(w, i);
}

__device__ inline size_t bitrev_sz(size_t x, int bits) {
  size_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((x >> b) & 1) << (bits - 1 - b);
  return r;
}

// Input permutation of an in-place DIT transform of M = 2^logM points, with zero padding and the
// coset shift: dst column c (M contiguous elements) slot j = src_c[k] * base^k for k =
// bitrev(j) < n_src, zero otherwise.  Source column c starts at (c / inner) * s_outer +
// (c % inner) * s_inner.
__global__ AGG_KERNEL void agg_prep_kernel(const fe* __restrict__ src, size_t s_outer, size_t s_inner, uint32_t inner,
                                           size_t n_src, fe* __restrict__ dst, size_t M, int logM, uint32_t ncols,
                                           fe base, int scaled) {
  const size_t idx = gid();
  if (idx >= (size_t)ncols * M) return;
  const size_t col = idx / M, j = idx - col * M, k = bitrev_sz(j, logM);
  fe v = fe_zero();
  if (k < n_src) {
    v = src[(col / inner) * s_outer + (col % inner) * s_inner + k];
    if (scaled) v = fe_mul(v, fe_pow64(base, k));
  }
  dst[col * M + j] = v;
}

// One radix-2 DIT stage (butterfly span half = 2^s) on ncols contiguous columns of M points;
// roots[e] = w_Ntab^e, Ntab >= M a power of two.  inverse: the conjugate twiddles.
__global__ AGG_KERNEL void agg_ntt_stage_kernel(fe* data, size_t M, int s, uint32_t ncols, const fe* __restrict__ roots,
                                     size_t Ntab, int inverse) {
  const size_t idx = gid(), hm = M / 2;
  if (idx >= (size_t)ncols * hm) return;
  const size_t col = idx / hm, t = idx - col * hm, half = (size_t)1 << s;
  const size_t k = t & (half - 1), i = ((t >> s) << (s + 1)) + k;
  size_t e = k * (Ntab / (2 * half));
  if (inverse && e) e = Ntab - e;
  fe* a = data + col * M;
  const fe u = a[i], v = fe_mul(a[i + half], roots[e]);
  a[i] = fe_add(u, v);
  a[i + half] = fe_sub(u, v);
}

// data[col * M + k] *= mult * base^k
__global__ AGG_KERNEL void agg_scale_kernel(fe* data, size_t M, uint32_t ncols, fe base, fe mult) {
  const size_t idx = gid();
  if (idx >= (size_t)ncols * M) return;
  const size_t k = idx % M;
  data[idx] = fe_mul(data[idx], fe_mul(mult, fe_pow64(base, k)));
}

// ---- constraint composition over the CE coset (prove_air step 2) ----------------------------
// row r of the column-major LDE, a column loaded on use (col < AGG_W, r < N: the caller's bounds)
struct LdeRow {
  const fe* row;  // lde + r
  size_t N;
  __device__ fe operator[](int col) const { return row[(size_t)col * N]; }
};
template <class E>
struct ComposeCoef {
  E alpha[AGG_TC];
  E beta[AGG_NA];
};
template <class E>
__global__ AGG_KERNEL void agg_compose_kernel(const fe* __restrict__ lde, size_t N, size_t n, size_t B, size_t ce,
                                   const fe* __restrict__ roots /* w_N^i */, ComposeCoef<E> K, fe gl, fe inv_n,
                                   fe v_total, fe c_count, fe* __restrict__ out /* X planes of ce */) {
  const size_t i = gid();
  if (i >= ce) return;
  const size_t step = N / ce, r0 = i * step, r1 = (r0 + B) & (N - 1);
  const fe x = fe_mul(fe{3, 0}, roots[r0]);
  const LdeRow cur{lde + r0, N}, nxt{lde + r1, N};
  const fe xn1 = fe_sub(fe_pow64(x, n), fe_one()), xg = fe_sub(x, gl);
  const fe i_xg = fe_inv(xg), i_xn1 = fe_inv(xn1), i_x1 = fe_inv(fe_sub(x, fe_one()));
  const fe p_last = fe_mul(fe_mul(fe_mul(gl, xn1), inv_n), i_xg);
  E t = zero<E>();  // each constraint goes straight into the sum: no array of the 24 values
  agg_transition_to<fe>(cur, nxt, p_last, [&](int k, fe v) { t = add(t, mulb(K.alpha[k], v)); });
  t = mulb(t, fe_mul(xg, i_xn1));
  // assertions: three at step 0 (x - 1), two at the last step (x - g^(n-1))
#pragma unroll
  for (int a = 0; a < AGG_NA; a++) {
    const fe val = a < 3 ? fe_zero() : (a == 3 ? v_total : c_count);
    t = add(t, mulb(K.beta[a], fe_mul(fe_sub(cur[agg_assert_col(a)], val), a < 3 ? i_x1 : i_xg)));
  }
  st_planes(out, ce, i, t);
}

// ---- DEEP composition in E (step 5) ---------------------------------------------------------
// frame: t(z) [W] | t(zg) [W] | H(z) [Cc] | H(zg) [Cc]; gam: W + Cc; out: a FRI layer of N points
template <class E>
__global__ AGG_KERNEL void agg_deep_kernel(const fe* __restrict__ lde, const fe* __restrict__ clde, size_t N, uint32_t W,
                                uint32_t Cc, const fe* __restrict__ roots, const E* __restrict__ frame,
                                const E* __restrict__ gam, E z, E zg, fe* __restrict__ out) {
  const size_t i = gid();
  if (i >= N) return;
  const E x = lift<E>(fe_mul(fe{3, 0}, roots[i]));
  // 1 / (x - z) and 1 / (x - z g) from one inversion of the product
  const E dz = sub(x, z), dzg = sub(x, zg), ip = inv(mul(dz, dzg));
  const E iz = mul(ip, dzg), izg = mul(ip, dz);
  E y = zero<E>();
  for (uint32_t c = 0; c < W; c++) {
    const E t = lift<E>(lde[(size_t)c * N + i]);
    y = add(y, mul(gam[c], add(mul(sub(t, frame[c]), iz), mul(sub(t, frame[W + c]), izg))));
  }
  for (uint32_t j = 0; j < Cc; j++) {
    const E hv = ld_cols<E>(clde, N, j, i);
    y = add(y, mul(gam[W + j], add(mul(sub(hv, frame[2 * W + j]), iz), mul(sub(hv, frame[2 * W + Cc + j]), izg))));
  }
  fri_store<E>(out, N, i, y);
}

// ---- FRI fold in E (step 6): folding 2, constant domain offset 3 ----------------------------
template <class E>
__global__ AGG_KERNEL void agg_fold_kernel(const fe* __restrict__ in, size_t Nd, const fe* __restrict__ roots, size_t Ntab, E a,
                                fe* __restrict__ out) {
  const size_t i = gid(), h = Nd / 2;
  if (i >= h) return;
  const fe x0 = fe_mul(fe{3, 0}, roots[i * (Ntab / Nd)]), x1 = fe_sub(fe_zero(), x0);
  const E v0 = fri_load<E>(in, Nd, i), v1 = fri_load<E>(in, Nd, i + h);
  // (v1 (a - x0) - v0 (a - x1)) / (x1 - x0)
  const E num = sub(mul(v1, sub(a, lift<E>(x0))), mul(v0, sub(a, lift<E>(x1))));
  fri_store<E>(out, h, i, mulb(num, fe_inv(fe_sub(x1, x0))));
}

// ---- the backend --------------------------------------------------------------------------
template <class T>
struct AggDeviceBackend final : AggBackend<T> {
  static constexpr size_t X = sizeof(T) / sizeof(fe);
  using AggBackend<T>::sh;
  zkl_ctx* C;
  hipStream_t s = nullptr;
  bool locked = false;
  fe *d_trace = nullptr, *d_tcoef = nullptr, *d_lde = nullptr, *d_ttree = nullptr, *d_cev = nullptr, *d_ccoef = nullptr,
     *d_clde = nullptr, *d_ctree = nullptr, *d_fri = nullptr, *d_ftree = nullptr, *d_roots = nullptr, *d_const = nullptr;
  struct Layer { size_t off, Nd, tree_off; };
  std::vector<Layer> done;
  size_t cur_off = 0, cur_Nd = 0, tree_off = 0;

  explicit AggDeviceBackend(zkl_ctx* c) : C(c) {
    agg_ctx_lock(C);
    locked = true;
  }
  ~AggDeviceBackend() override { unlock(); }
  void unlock() {
    if (locked) agg_ctx_unlock(C);
    locked = false;
  }
  template <class U>
  U* dbuf(int slot, size_t elems) { return (U*)agg_ctx_dbuf(C, slot, std::max<size_t>(elems, 1) * sizeof(U)); }

  // pinned staging in bounded pieces, so the largest shape (2^20 LDE rows) does not pin its LDE
  static constexpr size_t STAGE = (size_t)16 << 20;
  void upload(fe* d, const fe* h, size_t elems) {
    while (elems) {
      const size_t k = std::min(elems, STAGE / sizeof(fe));
      void* p = agg_ctx_hbuf(C, AGG_H_UP, k * sizeof(fe));
      memcpy(p, h, k * sizeof(fe));
      ZKL_HIPCHECK(hipMemcpyAsync(d, p, k * sizeof(fe), hipMemcpyHostToDevice, s));
      ZKL_HIPCHECK(hipStreamSynchronize(s));
      d += k; h += k; elems -= k;
    }
  }
  void download(fe* h, const fe* d, size_t elems) {
    while (elems) {
      const size_t k = std::min(elems, STAGE / sizeof(fe));
      void* p = agg_ctx_hbuf(C, AGG_H_DOWN, k * sizeof(fe));
      ZKL_HIPCHECK(hipMemcpyAsync(p, d, k * sizeof(fe), hipMemcpyDeviceToHost, s));
      ZKL_HIPCHECK(hipStreamSynchronize(s));
      memcpy(h, p, k * sizeof(fe));
      d += k; h += k; elems -= k;
    }
  }
  fe download_one(const fe* d) {
    fe v;
    download(&v, d, 1);
    return v;
  }

  // in-place transform of ncols columns of M points already in DIT input order
  void stages(fe* d, size_t M, uint32_t ncols, bool inverse) {
    const int lg = ilog2(M);
    for (int st = 0; st < lg; st++)
      agg_ntt_stage_kernel<<<blocks_for((size_t)ncols * (M / 2)), TPB, 0, s>>>(d, M, st, ncols, d_roots, sh.N, inverse ? 1 : 0);
  }

  fe commit_trace(const std::vector<std::vector<fe>>& trace) override {
    const AggCtxView v = agg_ctx_begin(C);
    s = (hipStream_t)v.stream;
    const size_t W = sh.W, n = sh.n, N = sh.N;
    if (W != (size_t)AGG_W) throw std::logic_error("aggregation device prover: trace width");
    d_trace = dbuf<fe>(AGG_D_TRACE, W * n);
    d_tcoef = dbuf<fe>(AGG_D_TCOEF, W * n);
    d_lde = dbuf<fe>(AGG_D_LDE, W * N);
    d_ttree = dbuf<fe>(AGG_D_TTREE, 2 * N);
    d_cev = dbuf<fe>(AGG_D_CEV, X * sh.ce);
    d_ccoef = dbuf<fe>(AGG_D_CCOEF, X * sh.ce);
    d_clde = dbuf<fe>(AGG_D_CLDE, X * sh.Cc * N);
    d_ctree = dbuf<fe>(AGG_D_CTREE, 2 * N);
    d_fri = dbuf<fe>(AGG_D_FRI, 2 * X * N);
    d_ftree = dbuf<fe>(AGG_D_FTREE, 2 * N);
    d_roots = dbuf<fe>(AGG_D_ROOTS, N);
    d_const = dbuf<fe>(AGG_D_CONST, X * 3 * (W + sh.Cc));
    std::vector<fe> flat(W * n);
    for (size_t c = 0; c < W; c++) memcpy(flat.data() + c * n, trace[c].data(), n * sizeof(fe));
    upload(d_trace, flat.data(), W * n);
    agg_roots_kernel<<<blocks_for(N), TPB, 0, s>>>(root_of_unity((unsigned)ilog2(N)), N, d_roots);
    // interpolate over <g>: coefficients
    agg_prep_kernel<<<blocks_for(W * n), TPB, 0, s>>>(d_trace, n, 0, 1, n, d_tcoef, n, ilog2(n), (uint32_t)W, fe_one(), 0);
    stages(d_tcoef, n, (uint32_t)W, true);
    agg_scale_kernel<<<blocks_for(W * n), TPB, 0, s>>>(d_tcoef, n, (uint32_t)W, fe_one(), fe_inv(fe{n, 0}));
    // evaluate over 3 <w_N>
    agg_prep_kernel<<<blocks_for(W * N), TPB, 0, s>>>(d_tcoef, n, 0, 1, n, d_lde, N, ilog2(N), (uint32_t)W, fe{3, 0}, 1);
    stages(d_lde, N, (uint32_t)W, false);
    check_launch("aggregation trace LDE");
    launch_hash_rows(d_lde, (uint32_t)W, N, 1, 8, nullptr, d_ttree + N, s, 0);
    launch_merkle(d_ttree, N, s);
    check_launch("aggregation trace commitment");
    download(flat.data(), d_tcoef, W * n);
    this->tpoly.assign(W, std::vector<fe>(n));
    for (size_t c = 0; c < W; c++) memcpy(this->tpoly[c].data(), flat.data() + c * n, n * sizeof(fe));
    return download_one(d_ttree + 1);
  }

  void compose(const std::vector<T>& alpha, const std::vector<T>& beta) override {
    if (alpha.size() != (size_t)AGG_TC || beta.size() != (size_t)AGG_NA)
      throw std::logic_error("aggregation device prover: coefficient counts");
    ComposeCoef<T> K;
    for (int k = 0; k < AGG_TC; k++) K.alpha[k] = alpha[k];
    for (int k = 0; k < AGG_NA; k++) K.beta[k] = beta[k];
    const size_t ce = sh.ce;
    agg_compose_kernel<T><<<blocks_for(ce), TPB, 0, s>>>(d_lde, sh.N, sh.n, sh.B, ce, d_roots, K, sh.gl,
                                                          fe_inv(fe{sh.n, 0}), sh.v_units_total, sh.children_count, d_cev);
    // interpolate over the coset 3 <w_ce>
    agg_prep_kernel<<<blocks_for(X * ce), TPB, 0, s>>>(d_cev, ce, 0, 1, ce, d_ccoef, ce, ilog2(ce), (uint32_t)X, fe_one(), 0);
    stages(d_ccoef, ce, (uint32_t)X, true);
    agg_scale_kernel<<<blocks_for(X * ce), TPB, 0, s>>>(d_ccoef, ce, (uint32_t)X, fe_inv(fe{3, 0}), fe_inv(fe{ce, 0}));
    check_launch("aggregation constraint composition");
    std::vector<fe> h(X * ce);
    download(h.data(), d_ccoef, X * ce);
    this->cco.resize(ce);
    for (size_t k = 0; k < ce; k++) this->cco[k] = from_planes(h.data(), ce, k);
  }

  static T from_planes(const fe* p, size_t stride, size_t i) {
    if constexpr (X == 2) return T{p[i], p[stride + i]};
    else return p[i];
  }

  fe commit_composition() override {
    const size_t n = sh.n, N = sh.N, cols = sh.Cc * X;
    // column j * X + k = component k of coefficients [j n, (j + 1) n) of the composition polynomial
    agg_prep_kernel<<<blocks_for(cols * N), TPB, 0, s>>>(d_ccoef, n, sh.ce, (uint32_t)X, n, d_clde, N, ilog2(N),
                                                         (uint32_t)cols, fe{3, 0}, 1);
    stages(d_clde, N, (uint32_t)cols, false);
    check_launch("aggregation composition LDE");
    launch_hash_rows(d_clde, (uint32_t)cols, N, 1, 8, nullptr, d_ctree + N, s, 1);
    launch_merkle(d_ctree, N, s);
    check_launch("aggregation composition commitment");
    return download_one(d_ctree + 1);
  }

  void deep(T z, T zg, const std::vector<T>& frame, const std::vector<T>& gam) override {
    const size_t W = sh.W, Cc = sh.Cc, nf = 2 * (W + Cc), ng = W + Cc;
    if (frame.size() != nf || gam.size() != ng) throw std::logic_error("aggregation device prover: frame size");
    std::vector<T> up(frame);
    up.insert(up.end(), gam.begin(), gam.end());
    upload(d_const, (const fe*)up.data(), (nf + ng) * X);
    const T* dc = (const T*)d_const;
    agg_deep_kernel<T><<<blocks_for(sh.N), TPB, 0, s>>>(d_lde, d_clde, sh.N, (uint32_t)W, (uint32_t)Cc, d_roots, dc,
                                                         dc + nf, z, zg, d_fri);
    check_launch("aggregation DEEP composition");
    cur_off = 0;
    cur_Nd = sh.N;
    tree_off = 0;
  }

  fe fri_commit() override {
    const size_t h = cur_Nd / 2;
    fe* tree = d_ftree + tree_off;
    launch_hash_rows(d_fri + cur_off, (uint32_t)(2 * X), h, 1, 8, nullptr, tree + h, s, 1);
    launch_merkle(tree, h, s);
    check_launch("aggregation FRI layer commitment");
    return download_one(tree + 1);
  }

  void fri_fold(T alpha) override {
    const size_t h = cur_Nd / 2, next = cur_off + X * cur_Nd;
    if (next + X * h > 2 * X * sh.N || tree_off + 2 * h > 2 * sh.N)
      throw std::logic_error("aggregation device prover: FRI buffers exhausted");
    agg_fold_kernel<T><<<blocks_for(h), TPB, 0, s>>>(d_fri + cur_off, cur_Nd, d_roots, sh.N, alpha, d_fri + next);
    check_launch("aggregation FRI fold");
    done.push_back({cur_off, cur_Nd, tree_off});
    cur_off = next;
    cur_Nd = h;
    tree_off += 2 * h;
  }

  // a FRI layer in the layout above -> natural order
  std::vector<T> unlayer(const fe* p, size_t Nd) const {
    const size_t h = Nd / 2;
    std::vector<T> v(Nd);
    for (size_t i = 0; i < Nd; i++) {
      const size_t half = i >= h ? 1 : 0;
      v[i] = from_planes(p + half * X * h, h, i - half * h);
    }
    return v;
  }

  void finish() override {
    const size_t W = sh.W, N = sh.N, Cc = sh.Cc;
    this->lde.assign(W, std::vector<fe>(N));
    for (size_t c = 0; c < W; c++) download(this->lde[c].data(), d_lde + c * N, N);
    this->ttree.resize(2 * N);
    download(this->ttree.data(), d_ttree, 2 * N);
    this->ctree.resize(2 * N);
    download(this->ctree.data(), d_ctree, 2 * N);
    {
      std::vector<fe> h(X * Cc * N);
      download(h.data(), d_clde, h.size());
      this->clde.assign(Cc, std::vector<T>(N));
      for (size_t j = 0; j < Cc; j++)
        for (size_t i = 0; i < N; i++) this->clde[j][i] = from_planes(h.data() + j * X * N, N, i);
    }
    {
      const size_t used = cur_off + X * cur_Nd;
      std::vector<fe> h(used), t(std::max<size_t>(tree_off, 1));
      download(h.data(), d_fri, used);
      if (tree_off) download(t.data(), d_ftree, tree_off);
      this->layers.clear();
      this->ftrees.clear();
      for (const Layer& L : done) {
        this->layers.push_back(unlayer(h.data() + L.off, L.Nd));
        this->ftrees.emplace_back(t.begin() + (long)L.tree_off, t.begin() + (long)(L.tree_off + L.Nd));
      }
      this->ev = unlayer(h.data() + cur_off, cur_Nd);
    }
    unlock();
  }

  // The segment prover's nonce search (prover.cpp, step 7) on the context's stream: ascending
  // windows of 2^g, 2^g, 2^(g+1), 2^(g+2) tries per read-back, a window's kernel returning at
  // once when an earlier window holds a solution, so the minimum over the first window with one
  // is the smallest nonce -- what the host search finds.  The coin's seed is a host value in the
  // form the kernels take by argument.  finish() released the context; it is taken again here.
  bool grind(fe seed, uint32_t bits, uint64_t* nonce) override {
    if (bits == 0) {  // the first candidate
      *nonce = 1;
      return true;
    }
    agg_ctx_lock(C);
    locked = true;
    s = (hipStream_t)agg_ctx_begin(C).stream;
    unsigned long long* d_best = dbuf<unsigned long long>(AGG_D_BEST, 2);
    unsigned long long* h_best = (unsigned long long*)agg_ctx_hbuf(C, AGG_H_DOWN, 16);
    uint32_t batch = 1u << std::min<uint32_t>(std::max<uint32_t>(bits, 14), 22);
    // test-only, as in the segment prover: a small first window makes a test take more than one
    // window and more than one read-back
    if (const char* e = getenv("ZKL_TEST_GRIND_FIRST")) batch = (uint32_t)std::max(1L, std::min(atol(e), 1L << 22));
    uint64_t base = 1;
    for (;;) {
      *h_best = ~0ull;
      ZKL_HIPCHECK(hipMemcpyAsync(d_best, h_best, 8, hipMemcpyHostToDevice, s));
      for (int w = 0; w < 4; w++) {
        launch_grind(seed, base, batch, bits, d_best, s, nullptr);
        base += batch;
        if (w >= 1) batch = std::min<uint32_t>(batch * 2, 1u << 22);
      }
      check_launch("aggregation grinding");
      ZKL_HIPCHECK(hipMemcpyAsync(h_best, d_best, 8, hipMemcpyDeviceToHost, s));
      ZKL_HIPCHECK(hipStreamSynchronize(s));
      if (*h_best != ~0ull) break;
    }
    *nonce = *h_best;
    unlock();
    return true;
  }
};

}  // namespace

template <class T>
std::unique_ptr<AggBackend<T>> make_agg_device_backend(zkl_ctx* ctx) {
  return std::unique_ptr<AggBackend<T>>(new AggDeviceBackend<T>(ctx));
}
template std::unique_ptr<AggBackend<fe>> make_agg_device_backend<fe>(zkl_ctx*);
template std::unique_ptr<AggBackend<fe2>> make_agg_device_backend<fe2>(zkl_ctx*);

}  // namespace zkl
