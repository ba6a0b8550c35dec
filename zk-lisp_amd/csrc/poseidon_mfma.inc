// Matrix-core Poseidon permutation (throughput form).  Included by kernels.hip after the
// Montgomery helpers (mont_cube130, to_mont130, from_mont130, limbs26, c_hm) it builds on.
// Its Montgomery radix is R' = 2^130 (five REDC digit steps per reduction, one fewer than the
// R = 2^156 of the lane-group form, ~5% of the round's VALU work): every value entering a
// cube is < 2^130, which R' still reduces below 2^131 (redc130).
//
// For levels with many independent states the 12x12 MDS product (poseidon/hasher.rs:173-190)
// runs on the matrix cores as an exact integer product: v_mfma_i32_32x32x32_i8 over balanced
// base-256 digits.  A wave carries 32 states; lane (h = lane>>5, n = lane&31) owns elements
// 2T+h (T = 0..5) of state n.  Per round each lane cubes its six elements on the VALU
// (Montgomery, as the lane-group form), and writes each cube c (< 2^131) as 16 bytes b_j with
// c = sum_j (b_j + 128) 2^(8j) + top * 2^128: the bytes, offset by -128, ARE the int8 B
// fragment of k-step T (element 2T+h, digit j) and the six `top`s form k-step 6.  The constant
// A operand holds, for output row (element i, digit c), the balanced digits of
// M[i][k] * 2^(8j) mod p (and of M[i][k] * 2^128 mod p for the tops), so accumulator tile T
// returns in lane (h, n), register c, the digit-column sum Y_c of element 2T+h of state n:
// sum_c Y_c 2^(8c) == (M . cube)_i - K_i (mod p) with |Y_c| < 2^21.6, where
// K_i = M_i . (128 sum_j 2^(8j)) undoes the byte offset.  The accumulator layout is the B
// layout of the next round, so no value leaves its lane.  The VALU folds the 16 columns into
// 26-bit limbs (+ rc*R + K_i + p*2^15: one table entry per round and element), reduces the
// bits >= 128 with 2^128 == 45*2^40 - 1 and goes on with the next cube.
//
// Per element and round that is ~190 VALU instructions instead of ~480 (the twelve 5x5-limb
// products of an MDS row), plus 7 MFMAs per tile on the matrix pipe beside the VALU.  The
// Montgomery factor passes through the linear layer unchanged (M.(xR) = (Mx)R), so the A
// digits are those of the plain MDS entries.

typedef int pm_v4i __attribute__((ext_vector_type(4)));
typedef int pm_v16i __attribute__((ext_vector_type(16)));

struct PmTables {
  int8_t afrag[6][7][64][16];  // A fragment of tile t, k-step s, lane
  uint64_t rk[27][12][5];      // limb columns of rc[r][i]*R + K_i (canonical) + p*2^15 + PM_NORM_B terms
};
__device__ PmTables d_pm;

// The 16-state form (pm16, levels of 2^13 and 2^14 states, where the 32-state form leaves SIMDs
// idle and its permutation latency bounds the level): v_mfma_i32_16x16x64_i8, a wave carries 16
// states and lane (g = lane>>4, n = lane&15) owns elements g, g+4, g+8 of state n, i.e. half the
// VALU work per lane and round.  The B fragment of k-step s < 3 is the 16 offset bytes of the
// lane's element 4s + g, k-step 3 holds its three tops; tile (T, q) returns in register r of
// lane (g, n) digit column 4q + r of element 4T + g (C row 4g + r), so the four tiles of T are
// the 16 digit columns the 32-state form's one tile gives.  12 tiles x 4 k-steps = 48 MFMAs
// per round of 16 states (16 cycles each: 768 cycles of matrix pipe, against 42 x 32 for 32).
struct Pm16Tables {
  int8_t afrag[12][4][64][16];  // A fragment of tile T*4+q, k-step s, lane
  uint64_t rk[27][12][5];       // as PmTables::rk
};
__device__ Pm16Tables d_pm16;

// launch bound of the matrix-core kernels other than row hashing (56 KB of tables in LDS per
// workgroup); PM_WIDE_CFG: they may use one workgroup of PM_WAVES waves per CU instead of up
// to two of 4 waves
#ifndef PM_WAVES_CFG
#define PM_WAVES_CFG 8
#endif
#ifndef PM_WIDE_CFG
#define PM_WIDE_CFG 0
#endif
constexpr int PM_WAVES = PM_WAVES_CFG;
constexpr int PM_THREADS = 64 * PM_WAVES;
// row hashing: one workgroup per CU (the LDS holds the tables alone when merge_many fits one
// absorb block).  12 waves (3 per SIMD) beat 8 by ~1% while every MFMA waited on its own LDS
// operand read (profiles/r02/ab_rows); with the operands software-pipelined (pm_round) the
// kernel needs ~206 VGPRs, so 8 waves (2 per SIMD): 31.7 -> 28.0 ms (profiles/r02/ab_pf)
#ifndef PM_ROW_WAVES_CFG
#define PM_ROW_WAVES_CFG 8
#endif
constexpr int PM_ROW_WAVES = PM_ROW_WAVES_CFG;
constexpr int PM_ROW_THREADS = 64 * PM_ROW_WAVES;
constexpr int PM_MAX_PARTS = 16;
constexpr int PM_PFX_PARTS = 9;  // partitions whose digests merge_many absorbs in one block (register form)

// balanced base-256 digits (each in [-128, 127]) of the representative of C mod p in
// [-128 (2^128-1)/255, 127 (2^128-1)/255]
static bool pm_balanced_digits(fe C, int d[16]) {
  typedef unsigned __int128 u128;
  const u128 P = ((u128)P_HI << 64) | P_LO;
  const u128 c = ((u128)C.hi << 64) | C.lo;
  const u128 bplus = (~(u128)0) / 255 * 127;
  const bool neg = c > bplus;
  u128 m = neg ? P - c : c;  // |v|
  for (int i = 0; i < 16; i++) {
    int r = (int)(m & 255);
    if (neg) r = (256 - r) & 255;  // v mod 256
    const int dd = r >= 128 ? r - 256 : r;
    d[i] = dd;
    if (!neg) m = (dd >= 0 ? m - (u128)dd : m + (u128)(-dd)) >> 8;
    else m = (dd >= 0 ? m + (u128)dd : m - (u128)(-dd)) >> 8;
  }
  return m == 0;
}

static fe pm_signed(int v) { return v >= 0 ? fe{(uint64_t)v, 0} : fe_sub(fe_zero(), fe{(uint64_t)(-v), 0}); }

static void pm_build(const HasherConsts& h, PmTables& T, Pm16Tables& T16) {
  fe p2[17];  // 2^(8j) mod p
  p2[0] = fe_one();
  for (int j = 1; j < 17; j++) p2[j] = fe_mul(p2[j - 1], fe{256, 0});
  // dig[i][k][j] = digits of M[i][k] * 2^(8j)
  static int dig[12][12][17][16];
  for (int i = 0; i < 12; i++)
    for (int k = 0; k < 12; k++)
      for (int j = 0; j < 17; j++) {
        const fe C = fe_mul(h.mds[i * 12 + k], p2[j]);
        if (!pm_balanced_digits(C, dig[i][k][j])) throw std::runtime_error("pm tables: digit range");
        fe back = fe_zero();  // self-check: sum_c d_c 2^(8c) == C
        for (int c = 0; c < 16; c++) back = fe_add(back, fe_mul(pm_signed(dig[i][k][j][c]), p2[c]));
        if (!fe_eq(back, C)) throw std::runtime_error("pm tables: digit check");
      }
  for (int t = 0; t < 6; t++)
    for (int s = 0; s < 7; s++)
      for (int lane = 0; lane < 64; lane++) {
        const int hp = lane >> 5, m = lane & 31;
        // accumulator row m holds digit (m&3) + 4(m>>3) of element 2t + ((m>>2)&1)
        const int i = 2 * t + ((m >> 2) & 1), c = (m & 3) + 4 * (m >> 3);
        for (int j = 0; j < 16; j++) {
          int v = 0;
          if (s < 6) v = dig[i][2 * s + hp][j][c];
          else if (j < 6) v = dig[i][2 * j + hp][16][c];
          T.afrag[t][s][lane][j] = (int8_t)v;
        }
      }
  for (int t = 0; t < 12; t++)
    for (int s = 0; s < 4; s++)
      for (int lane = 0; lane < 64; lane++) {
        const int m = lane & 15, kb = lane >> 4;
        // C row m = 4 g + r: digit 4 (t & 3) + r of element 4 (t >> 2) + g
        const int i = 4 * (t >> 2) + (m >> 2), c = 4 * (t & 3) + (m & 3);
        for (int j = 0; j < 16; j++) {
          int v = 0;
          if (s < 3) v = dig[i][4 * s + kb][j][c];
          else if (j < 3) v = dig[i][4 * j + kb][16][c];
          T16.afrag[t][s][lane][j] = (int8_t)v;
        }
      }
  // OFF = 128 sum_j 2^(8j); K_i = OFF * sum_k M[i][k]
  fe off = fe_zero();
  for (int j = 0; j < 16; j++) off = fe_add(off, fe_mul(fe{128, 0}, p2[j]));
  const fe R = fe_pow64(fe{2, 0}, 130);  // the permutation's Montgomery radix R' (redc130)
  // p * 2^15 in limb columns (limbs 0..3 of 26 bits, column 4 the rest): keeps the digit
  // sums (> -2^141.7) positive
  typedef unsigned __int128 u128;
  const u128 P = ((u128)P_HI << 64) | P_LO;
  uint64_t bias[5];
  bias[0] = (uint64_t)((P & 0x7FF) << 15);
  for (int t = 1; t < 4; t++) bias[t] = (uint64_t)((P >> (26 * t - 15)) & M26);
  bias[4] = (uint64_t)(P >> 89);
  // and PM_NORM_B on columns 0..3, taken back from the next column: every column of
  // pm_normalise stays non-negative, so that its carries are 32-bit (bounds in mont26.h)
  for (int t = 0; t < 4; t++) {
    bias[t] += PM_NORM_B;
    bias[t + 1] -= PM_NORM_B >> 26;
  }
  for (int i = 0; i < 12; i++) {
    fe rs = fe_zero();
    for (int k = 0; k < 12; k++) rs = fe_add(rs, h.mds[i * 12 + k]);
    const fe Ki = fe_mul(off, rs);
    for (int r = 0; r < 27; r++) {
      const fe v = fe_add(fe_mul(h.rc[r * 12 + i], R), Ki);
      uint32_t l[5];
      limbs26(v, l);
      for (int t = 0; t < 5; t++) T.rk[r][i][t] = T16.rk[r][i][t] = (uint64_t)l[t] + bias[t];
    }
  }
}

void upload_pm_tables(const HasherConsts& h, hipStream_t s) {
  static PmTables tab;
  static Pm16Tables tab16;
  static std::once_flag once;
  std::call_once(once, [&] { pm_build(h, tab, tab16); });
  ZKL_HIPCHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(d_pm), &tab, sizeof tab, 0, hipMemcpyHostToDevice, s));
  ZKL_HIPCHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(d_pm16), &tab16, sizeof tab16, 0, hipMemcpyHostToDevice, s));
}

// hashing policy: engine 1 = matrix-core permutation on levels of at least pm_min_items
// states (default), 0 = lane groups everywhere.  Defaults from ZKL_HASH_ENGINE=lane|mfma and
// ZKL_PM_MIN_ITEMS; zkl_hip_set_hash_policy changes them (tests, A/B timing).  Small levels
// stay on the latency-optimised lane groups: a permutation takes ~2.5x longer in the
// matrix-core form, which only pays when the level fills the chip.
static std::atomic<int> g_engine{-1};
static std::atomic<size_t> g_pm_min{0};
int hash_engine() {
  int e = g_engine.load(std::memory_order_relaxed);
  if (e < 0) {
    const char* v = getenv("ZKL_HASH_ENGINE");
    e = (v && !strcmp(v, "lane")) ? 0 : 1;
    g_engine.store(e);
  }
  return e;
}
static size_t pm_min_items() {
  size_t m = g_pm_min.load(std::memory_order_relaxed);
  if (!m) {
    const char* v = getenv("ZKL_PM_MIN_ITEMS");
    m = v ? (size_t)strtoull(v, nullptr, 10) : (size_t)1 << 14;
    if (!m) m = 1;
    g_pm_min.store(m);
  }
  return m;
}
void set_hash_policy(int engine, size_t min_items) {
  g_engine.store(engine ? 1 : 0);
  g_pm_min.store(min_items ? min_items : 1);
}

// Pairing of the two waves that share a SIMD (round 3, profiles/r03/ab_pair): a static
// s_setprio for the second half and 256/512-cycle staggers measured within +-0.5%; the
// persistent row loop already desynchronises the partner waves, so neither is built.
__device__ __forceinline__ void pm_load_tables(PmTables* tb) {
  const uint4* src = reinterpret_cast<const uint4*>(&d_pm);
  uint4* dst = reinterpret_cast<uint4*>(tb);
  for (int i = (int)threadIdx.x; i < (int)(sizeof(PmTables) / 16); i += (int)blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// PmShifts, pm_shifts and pm_normalise (digit-column sums + round-constant columns -> limbs) are
// in mont26.h, host and device, beside the cube they feed.

// a cube's normalised limbs as its B fragment (16 offset bytes) and top bits (pm_pack_words)
__device__ __forceinline__ void pm_pack(const uint32_t c[5], pm_v4i& b, uint32_t& top) {
  const uint32_t w0 = c[0] | (c[1] << 26);
  const uint32_t w1 = (c[1] >> 6) | (c[2] << 20);
  const uint32_t w2 = (c[2] >> 12) | (c[3] << 14);
  const uint32_t w3 = (c[3] >> 18) | (c[4] << 8);
  top = c[4] >> 24;
  b = pm_v4i{(int)(w0 ^ 0x80808080u), (int)(w1 ^ 0x80808080u), (int)(w2 ^ 0x80808080u), (int)(w3 ^ 0x80808080u)};
}

// cube of one element, written as its B fragment and top bits
__device__ __forceinline__ void pm_cube_pack(const uint32_t x[5], pm_v4i& b, uint32_t& top) {
  uint32_t c[5];
  mont_cube130(x, c);  // normalised limbs of a value < 2^129 (< 2^131 right after an absorb)
  pm_pack(c, b, top);
}

// The cubes of the round loop (the first cube of a permutation, right after an absorb, keeps the
// form above): mont_cube130_chain gives the same limbs as mont_cube130 in fewer instructions, each
// half of it one dependent chain.  pm_cube_finish is the second half and the packing; the caller
// runs it beside the first half of the next element, so that two independent chains share the
// VALU and neither waits on its own last result.
__device__ __forceinline__ void pm_cube_finish(const uint32_t sq[5], const uint32_t x[5], pm_v4i& b, uint32_t& top) {
  uint32_t c[5];
  mont_mul130_chain(sq, x, c);  // normalised limbs of a value < 2^129
  pm_pack(c, b, top);
}
__device__ __forceinline__ void pm_cube_pack_chain(const uint32_t x[5], pm_v4i& b, uint32_t& top) {
  uint32_t sq[5];
  mont_sq130_chain(x, sq);
  pm_cube_finish(sq, x, b, top);
}

__device__ __forceinline__ pm_v4i pm_tops(const uint32_t t[6]) {
  return pm_v4i{(int)(t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24)), (int)(t[4] | (t[5] << 8)), 0, 0};
}

// One round on the cubes in b: the MFMAs of tile t are followed in program order by the
// VALU work of element t-1 (normalise, then the first half of the next round's cube) and of
// element t-2 (the second half), so the wave's own integer work runs while the matrix pipe
// finishes the later tiles.  The LDS operands are
// software-pipelined: right after tile t's MFMAs are issued, the A fragments of tile t+1
// (of tile 0 for the next round after the last tile) and the round-constant columns of
// element t are requested, and a scheduling barrier keeps the requests ahead of element
// t-1's ~180 VALU instructions, which hide their latency (without it every MFMA waited on
// the LDS read issued just before it).  a[7] holds tile 0's fragments on entry and exit.
// PM_IGLP_CFG >= 0: an llvm.amdgcn.iglp.opt(PM_IGLP_CFG) scheduling hint in the round (-1 =
// none).  Variant 0 (interleave the LDS operand reads with the MFMAs) measured 28.9 against
// 29.0-29.1 ms for the trace row hash and 4.28 against 4.36 for the composition rows on one box
// (two reps each, profiles/r03/ab_iglp); variant 1 does not compile in reasonable memory.
#ifndef PM_IGLP_CFG
#define PM_IGLP_CFG 0
#endif
template <bool NEXT>
__device__ __forceinline__ void pm_round(const PmShifts& K, const pm_v4i* af, const uint64_t* rk, const pm_v4i b[7],
                                         uint32_t x[6][5], pm_v4i nb[7], pm_v4i a[7]) {
#if PM_IGLP_CFG >= 0
  __builtin_amdgcn_iglp_opt(PM_IGLP_CFG);
#endif
  uint32_t tops[6];
  pm_v16i prev;
  uint64_t rkv[5];
  uint32_t sq[5];  // the square of element t-1, multiplied out and packed one tile later
#pragma unroll
  for (int t = 0; t < 6; t++) {
    pm_v16i acc = pm_v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 7; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b[s], acc, 0, 0, 0);
    const int tn = t == 5 ? 0 : t + 1;
    pm_v4i an[7];
    uint64_t rkn[5];
#pragma unroll
    for (int s = 0; s < 7; s++) an[s] = af[(tn * 7 + s) * 64];
#pragma unroll
    for (int l = 0; l < 5; l++) rkn[l] = rk[t * 10 + l];
    __builtin_amdgcn_sched_barrier(0);
    // two independent chains per tile: element t-2's multiply and packing, element t-1's fold and
    // square
    if (NEXT && t > 1) pm_cube_finish(sq, x[t - 2], nb[t - 2], tops[t - 2]);
    if (t > 0) {
      pm_normalise(K, prev, rkv, x[t - 1]);
      if (NEXT) mont_sq130_chain(x[t - 1], sq);
    }
    prev = acc;
#pragma unroll
    for (int s = 0; s < 7; s++) a[s] = an[s];
#pragma unroll
    for (int l = 0; l < 5; l++) rkv[l] = rkn[l];
  }
  if (NEXT) pm_cube_finish(sq, x[4], nb[4], tops[4]);
  pm_normalise(K, prev, rkv, x[5]);
  if (NEXT) {
    pm_cube_pack_chain(x[5], nb[5], tops[5]);
    nb[6] = pm_tops(tops);
  }
}

// Last round of a permutation whose output is state[0] alone (the sponge's digest): only
// tile 0's seven MFMAs (element 2*0 + h) and that element's normalisation run; the other five
// tiles' MFMAs and normalisations would only feed elements nothing reads
// (ro_bytes_sponge_custom_rounds returns state[0], hasher.rs:228).  a[] holds tile 0's fragments.
__device__ __forceinline__ void pm_round_out0(const PmShifts& K, const uint64_t* rk, const pm_v4i b[7], uint32_t x[6][5],
                                              const pm_v4i a[7]) {
  pm_v16i acc = pm_v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < 7; s++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b[s], acc, 0, 0, 0);
  uint64_t rkv[5];
#pragma unroll
  for (int l = 0; l < 5; l++) rkv[l] = rk[l];
  pm_normalise(K, acc, rkv, x[0]);
  // the other elements are dead: overwrite them so the previous round's values do not stay live
#pragma unroll
  for (int T = 1; T < 6; T++)
#pragma unroll
    for (int l = 0; l < 5; l++) x[T][l] = 0;
}

// PM_PRUNE_CFG: bit 0 = first-block constant cubes, bit 1 = state[0]-only last rounds
#ifndef PM_PRUNE_CFG
#define PM_PRUNE_CFG 3
#endif

// B words of a round-1 cube that is a constant of the sponge's first block (HasherMont::pmk0,
// pmkt): element 2T+h holds no message -- zero, or a tag lane for T = 5
__device__ __forceinline__ void pm_const_cube(int T, int h, pm_v4i& b, uint32_t& top) {
  uint32_t w[5];
#pragma unroll
  for (int i = 0; i < 5; i++) w[i] = T == 5 ? (h ? c_hm.pmkt[1][i] : c_hm.pmkt[0][i]) : c_hm.pmk0[i];
  b = pm_v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  top = w[4];
}

// element-group mask of the first absorb block's constant round-1 cubes (matrix-core form,
// T = element pair 2T, 2T+1): elements 1..nmsg hold messages, 10 and 11 the tags, the rest
// zero; T = 0 (the domain element beside message 0) is never constant
__device__ __forceinline__ int pm_first_const_mask(int nmsg) {
  return ((0x3F << min(nmsg / 2 + 1, 6)) | 0x20) & 0x3E;
}

// one permutation of the wave's 32 states; x[T] = limbs of element 2T+h (Montgomery).
// cmask (wave-uniform): element pairs T whose round-1 cubes are the first block's constants
// (pm_first_const_mask), taken from HasherMont instead of cubed; out0 (wave-uniform): only
// state[0] is read afterwards (pm_round_out0).  Both leave every value that is read unchanged.
__device__ __forceinline__ void pm_permute(const PmTables* tb, uint32_t x[6][5], int cmask = 0, bool out0 = false) {
  const int lane = (int)(threadIdx.x & 63);
  const int h = lane >> 5;
  const pm_v4i* af = reinterpret_cast<const pm_v4i*>(&tb->afrag[0][0][0][0]) + lane;
  const uint64_t* rkp = &tb->rk[0][h][0];
  const PmShifts K = pm_shifts();
  pm_v4i a[7];
#pragma unroll
  for (int s = 0; s < 7; s++) a[s] = af[s * 64];
  pm_v4i b[7];
  {
    uint32_t tops[6];
#pragma unroll
    for (int T = 0; T < 6; T++) {
      if ((cmask >> T) & 1)
        pm_const_cube(T, h, b[T], tops[T]);
      else
        pm_cube_pack(x[T], b[T], tops[T]);
    }
    b[6] = pm_tops(tops);
  }
#pragma unroll 1
  for (int r = 0; r < 26; r++, rkp += 60) {
    pm_v4i nb[7];
    pm_round<true>(K, af, rkp, b, x, nb, a);
#pragma unroll
    for (int s = 0; s < 7; s++) b[s] = nb[s];
  }
  if (out0) {
    pm_round_out0(K, rkp, b, x, a);
  } else {
    pm_v4i unused[7];
    pm_round<false>(K, af, rkp, b, x, unused, a);
  }
}

// pg_sponge for the wave's 32 states (state n = lane & 31).  All lanes of the wave call it
// with the same nmsg (MFMAs run on the whole wave); ld(i) is called by the lane absorbing
// message i, and only when live.  The digest is valid in lanes with h == 0.
// OUT0 = false keeps the full last round (the trace row hash's sponges: with run-time message
// counts the state[0]-only round raised the kernel from 206 to 246 VGPRs and measured 0.7% slower;
// the composition rows, one-block sponges, keep it: -0.7%, profiles/r06/prune/summary.md)
// The sponge in two pieces, so that a caller can stop after some absorb blocks and another can
// resume from the saved state (the row hash's prefix table, below): pm_sponge_init sets the
// state a sponge of domain D starts from, pm_sponge_blocks absorbs and permutes the blocks whose
// first index b0 lies in [b_from, b_to) (multiples of 10); h = (lane >> 5) & 1, the caller's.
// pm_sponge keeps its own copy of the eight lines of pm_sponge_init: calling it there cost the row
// kernels 40 VGPRs and a spill, and with the copy they compile to what they were.
template <int D>
__device__ __forceinline__ void pm_sponge_init(uint32_t x[6][5]) {
  const int h = (int)((threadIdx.x >> 5) & 1);
#pragma unroll
  for (int T = 0; T < 6; T++)
#pragma unroll
    for (int l = 0; l < 5; l++) x[T][l] = 0;
#pragma unroll
  for (int l = 0; l < 5; l++) {
    x[0][l] = h ? 0u : c_hm.dfe130[D][l];
    x[5][l] = h ? c_hm.dom130[1][l] : c_hm.dom130[0][l];
  }
}

template <bool OUT0, class Loader>
__device__ __forceinline__ void pm_sponge_blocks(const PmTables* tb, bool live, int nmsg, Loader ld, uint32_t x[6][5],
                                                 int h, int b_from, int b_to) {
  const int total = nmsg + 1;
  for (int b0 = b_from; b0 < b_to; b0 += 10) {
#pragma unroll
    for (int T = 0; T < 5; T++) {
      const int idx = b0 + 2 * T + h;
      if (live && idx >= 1 && idx < total) {
        uint32_t m[5];
        to_mont130(ld(idx - 1), m);
#pragma unroll
        for (int l = 0; l < 5; l++) x[T][l] += m[l];
      }
    }
    pm_permute(tb, x, (PM_PRUNE_CFG & 1) && b0 == 0 ? pm_first_const_mask(nmsg) : 0,
               OUT0 && (PM_PRUNE_CFG & 2) && b0 + 10 >= total);
  }
}

// pm_sponge_blocks<false> of the masked row kernel: the same blocks and the same first-block
// pruning (by nmsg alone), but skip(i) (wave-uniform) says that sponge elements i and i + 1, the two half-waves
// of one T, absorb only zeros, and that T's fold, conversion and limb adds are left out.  A copy and
// not a parameter of the routine above: with the parameter the dense row kernel came out with
// its registers renamed, and its code is to stay what it was.
template <class Loader, class Skip>
__device__ __forceinline__ void pm_sponge_blocks_masked(const PmTables* tb, bool live, int nmsg, Loader ld,
                                                        uint32_t x[6][5], int h, int b_from, int b_to, Skip skip) {
  const int total = nmsg + 1;
  for (int b0 = b_from; b0 < b_to; b0 += 10) {
    // every load of the block is issued before the first fold waits for one: one memory latency
    // per block instead of one per T (the registers are free here, between two permutations)
    fe ca[5], cb[5];
#pragma unroll
    for (int T = 0; T < 5; T++) {
      const int idx = b0 + 2 * T + h;
      ca[T] = cb[T] = fe_zero();
      if (skip(b0 + 2 * T)) continue;
      if (live && idx >= 1 && idx < total) ld(idx - 1, ca[T], cb[T]);
    }
#pragma unroll
    for (int T = 0; T < 5; T++) {
      const int idx = b0 + 2 * T + h;
      if (skip(b0 + 2 * T)) continue;
      if (live && idx >= 1 && idx < total) {
        uint32_t m[5];
        to_mont130(fold_pair(ca[T], cb[T]), m);
#pragma unroll
        for (int l = 0; l < 5; l++) x[T][l] += m[l];
      }
    }
    pm_permute(tb, x, (PM_PRUNE_CFG & 1) && b0 == 0 ? pm_first_const_mask(nmsg) : 0, false);
  }
}

template <int D, bool OUT0 = true, class Loader>
__device__ __forceinline__ fe pm_sponge(const PmTables* tb, bool live, int nmsg, Loader ld) {
  const int h = (int)((threadIdx.x >> 5) & 1);
  uint32_t x[6][5];
#pragma unroll
  for (int T = 0; T < 6; T++)
#pragma unroll
    for (int l = 0; l < 5; l++) x[T][l] = 0;
#pragma unroll
  for (int l = 0; l < 5; l++) {
    x[0][l] = h ? 0u : c_hm.dfe130[D][l];
    x[5][l] = h ? c_hm.dom130[1][l] : c_hm.dom130[0][l];
  }
  pm_sponge_blocks<OUT0>(tb, live, nmsg, ld, x, h, 0, nmsg + 1);
  return from_mont130(x[0]);
}

// ---- the 16-state form ------------------------------------------------------------------------
__device__ __forceinline__ void pm16_load_tables(Pm16Tables* tb) {
  const uint4* src = reinterpret_cast<const uint4*>(&d_pm16);
  uint4* dst = reinterpret_cast<uint4*>(tb);
  for (int i = (int)threadIdx.x; i < (int)(sizeof(Pm16Tables) / 16); i += (int)blockDim.x) dst[i] = src[i];
  __syncthreads();
}

__device__ __forceinline__ pm_v4i pm16_tops(const uint32_t t[3]) {
  return pm_v4i{(int)(t[0] | (t[1] << 8) | (t[2] << 16)), 0, 0, 0};
}

// One round on the cubes in b (k-steps 0..3): the four tiles of element group T, then the VALU
// work of group T-1 (normalise, the next round's cube), the A fragments of the next tile
// requested right after each tile's MFMAs, as pm_round.  rk: round constants of element g.
// The chained cube runs whole here, unpaired: with three groups a round there is little to pair, and
// with mont_cube130 beside the new pm_normalise these kernels need 153-168 VGPRs instead of
// 100-115, a wave per SIMD less (profiles/r10/carry/summary.md).  These levels are bound by one
// permutation's latency, which the serial chain lengthens: merkle_level_pm16_kernel 750 -> 826 us
// per proof.
template <bool NEXT>
__device__ __forceinline__ void pm16_round(const PmShifts& K, const pm_v4i* af, const uint64_t* rk, const pm_v4i b[4],
                                           uint32_t x[3][5], pm_v4i nb[4], pm_v4i a[4]) {
  uint32_t tops[3];
  pm_v16i prev;
  uint64_t rkv[5];
#pragma unroll
  for (int T = 0; T < 3; T++) {
    pm_v16i Y;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      pm_v4i acc = pm_v4i{0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], b[s], acc, 0, 0, 0);
      const int tn = (4 * T + q + 1) % 12;
#pragma unroll
      for (int s = 0; s < 4; s++) a[s] = af[(tn * 4 + s) * 64];
#pragma unroll
      for (int r = 0; r < 4; r++) Y[4 * q + r] = acc[r];
    }
    uint64_t rkn[5];
#pragma unroll
    for (int l = 0; l < 5; l++) rkn[l] = rk[T * 20 + l];
    __builtin_amdgcn_sched_barrier(0);
    if (T > 0) {
      pm_normalise(K, prev, rkv, x[T - 1]);
      if (NEXT) pm_cube_pack_chain(x[T - 1], nb[T - 1], tops[T - 1]);
    }
    prev = Y;
#pragma unroll
    for (int l = 0; l < 5; l++) rkv[l] = rkn[l];
  }
  pm_normalise(K, prev, rkv, x[2]);
  if (NEXT) {
    pm_cube_pack_chain(x[2], nb[2], tops[2]);
    nb[3] = pm16_tops(tops);
  }
}

// last round when only state[0] is read: the four tiles of element group 0 (elements 0..3; the
// digest is element 0 in lanes g == 0) and its normalisation (pm_round_out0).  a[] holds tile 0's
// fragments on entry.
__device__ __forceinline__ void pm16_round_out0(const PmShifts& K, const pm_v4i* af, const uint64_t* rk, const pm_v4i b[4],
                                                uint32_t x[3][5], pm_v4i a[4]) {
  pm_v16i Y;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    pm_v4i acc = pm_v4i{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], b[s], acc, 0, 0, 0);
    if (q < 3) {
#pragma unroll
      for (int s = 0; s < 4; s++) a[s] = af[((q + 1) * 4 + s) * 64];
    }
#pragma unroll
    for (int r = 0; r < 4; r++) Y[4 * q + r] = acc[r];
  }
  uint64_t rkv[5];
#pragma unroll
  for (int l = 0; l < 5; l++) rkv[l] = rk[l];
  pm_normalise(K, Y, rkv, x[0]);
#pragma unroll
  for (int T = 1; T < 3; T++)
#pragma unroll
    for (int l = 0; l < 5; l++) x[T][l] = 0;
}

// first-block constant groups of the 16-state form (group T = elements 4T..4T+3): T = 1 when
// no message reaches element 4 (zeros), T = 2 when none reaches element 8 (zeros and the tags)
__device__ __forceinline__ int pm16_first_const_mask(int nmsg) { return (nmsg < 4 ? 2 : 0) | (nmsg < 8 ? 4 : 0); }

__device__ __forceinline__ void pm16_const_cube(int T, int g, pm_v4i& b, uint32_t& top) {
  uint32_t w[5];
#pragma unroll
  for (int i = 0; i < 5; i++)
    w[i] = (T == 2 && g >= 2) ? (g == 3 ? c_hm.pmkt[1][i] : c_hm.pmkt[0][i]) : c_hm.pmk0[i];
  b = pm_v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  top = w[4];
}

// one permutation of the wave's 16 states; x[T] = limbs of element 4T+g (Montgomery, R');
// cmask / out0 as pm_permute
__device__ __forceinline__ void pm16_permute(const Pm16Tables* tb, uint32_t x[3][5], int cmask = 0, bool out0 = false) {
  const int lane = (int)(threadIdx.x & 63);
  const int g = lane >> 4;
  const pm_v4i* af = reinterpret_cast<const pm_v4i*>(&tb->afrag[0][0][0][0]) + lane;
  const uint64_t* rkp = &tb->rk[0][g][0];
  const PmShifts K = pm_shifts();
  pm_v4i a[4];
#pragma unroll
  for (int s = 0; s < 4; s++) a[s] = af[s * 64];
  pm_v4i b[4];
  {
    uint32_t tops[3];
#pragma unroll
    for (int T = 0; T < 3; T++) {
      if ((cmask >> T) & 1)
        pm16_const_cube(T, g, b[T], tops[T]);
      else
        pm_cube_pack(x[T], b[T], tops[T]);
    }
    b[3] = pm16_tops(tops);
  }
#pragma unroll 1
  for (int r = 0; r < 26; r++, rkp += 60) {
    pm_v4i nb[4];
    pm16_round<true>(K, af, rkp, b, x, nb, a);
#pragma unroll
    for (int s = 0; s < 4; s++) b[s] = nb[s];
  }
  if (out0) {
    pm16_round_out0(K, af, rkp, b, x, a);
  } else {
    pm_v4i unused[4];
    pm16_round<false>(K, af, rkp, b, x, unused, a);
  }
}

// pm_sponge for the wave's 16 states (state n = lane & 15); the digest is valid in lanes with
// g == 0 (element 0)
template <int D, class Loader>
__device__ __forceinline__ fe pm16_sponge(const Pm16Tables* tb, bool live, int nmsg, Loader ld) {
  const int g = (int)((threadIdx.x >> 4) & 3);
  uint32_t x[3][5];
#pragma unroll
  for (int T = 0; T < 3; T++)
#pragma unroll
    for (int l = 0; l < 5; l++) x[T][l] = 0;
#pragma unroll
  for (int l = 0; l < 5; l++) {
    if (g == 0) x[0][l] = c_hm.dfe130[D][l];
    if (g == 2) x[2][l] = c_hm.dom130[0][l];  // element 10
    if (g == 3) x[2][l] = c_hm.dom130[1][l];  // element 11
  }
  const int total = nmsg + 1;
  for (int b0 = 0; b0 < total; b0 += 10) {
#pragma unroll
    for (int T = 0; T < 3; T++) {
      const int e = 4 * T + g;
      const int idx = b0 + e;
      if (live && e < 10 && idx >= 1 && idx < total) {
        uint32_t m[5];
        to_mont130(ld(idx - 1), m);
#pragma unroll
        for (int l = 0; l < 5; l++) x[T][l] += m[l];
      }
    }
    pm16_permute(tb, x, (PM_PRUNE_CFG & 1) && b0 == 0 ? pm16_first_const_mask(nmsg) : 0, (PM_PRUNE_CFG & 2) && b0 + 10 >= total);
  }
  return from_mont130(x[0]);
}

// CUs of the current device (launch shapes of the matrix-core kernels); a failing query is an
// error, not a silent 256
static int pm_cus() {
  static int cus = [] {
    int dev = 0, v = 0;
    ZKL_HIPCHECK(hipGetDevice(&dev));
    ZKL_HIPCHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
    if (v <= 0) throw std::runtime_error("hipDeviceAttributeMultiprocessorCount returned " + std::to_string(v));
    return v;
  }();
  return cus;
}

// Launch shape of a matrix-core kernel over `items` states (32 per wave-batch): row hashing
// uses 8-wave blocks (one per CU, its digest buffer is per wave); the other kernels use the
// largest block of 1, 2 or 4 waves that still puts a block on every CU, two blocks per CU at
// most (the 56 KB of tables per block), so a small level spreads one wave per SIMD instead of
// stacking on a few CUs.
struct PmLaunch {
  unsigned grid, threads;
};
static PmLaunch pm_launch(size_t items, bool rows = false, size_t per_batch = 32) {
  const size_t batches = (items + per_batch - 1) / per_batch, cus = (size_t)pm_cus();
  if (rows) return PmLaunch{(unsigned)std::min<size_t>((batches + PM_ROW_WAVES - 1) / PM_ROW_WAVES, cus), PM_ROW_THREADS};
  if (PM_WIDE_CFG && batches >= (size_t)PM_WAVES * cus) return PmLaunch{(unsigned)cus, PM_THREADS};
  size_t wpb = 4;
  while (wpb > 1 && batches < wpb * cus) wpb /= 2;
  return PmLaunch{(unsigned)std::min<size_t>((batches + wpb - 1) / wpb, 2 * cus), (unsigned)(64 * wpb)};
}
#define PM_GO(kern, items, rows, s) kern<<<pm_launch(items, rows).grid, pm_launch(items, rows).threads, 0, s>>>
#define PM16_GO(kern, items, s) kern<<<pm_launch(items, false, 16).grid, pm_launch(items, false, 16).threads, 0, s>>>

// persistent loop of a wave over batches of 16 items (the 16-state form)
#define PM16_LOOP(items)                                                                      \
  const int pm_lane = (int)(threadIdx.x & 63);                                                \
  const size_t pm_nb = ((items) + 15) / 16;                                                    \
  const size_t pm_wpb = blockDim.x >> 6;                                                       \
  for (size_t pm_b = (size_t)blockIdx.x * pm_wpb + (threadIdx.x >> 6); pm_b < pm_nb;           \
       pm_b += (size_t)gridDim.x * pm_wpb)

// persistent loop of a wave over batches of 32 items (wave-uniform trip count)
#define PM_LOOP(items)                                                                        \
  const int pm_lane = (int)(threadIdx.x & 63);                                                \
  const int pm_h = pm_lane >> 5;                                                               \
  (void)pm_h;                                                                                  \
  const size_t pm_nb = ((items) + 31) / 32;                                                    \
  const size_t pm_wpb = blockDim.x >> 6;                                                       \
  for (size_t pm_b = (size_t)blockIdx.x * pm_wpb + (threadIdx.x >> 6); pm_b < pm_nb;           \
       pm_b += (size_t)gridDim.x * pm_wpb)

// permutations of n states (12 canonical elements each, in place): stage test entry point
__global__ __launch_bounds__(PM_THREADS) void pm_permute_kernel(fe* st, size_t n) {
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  PM_LOOP(n) {
    const size_t i0 = pm_b * 32 + (size_t)(pm_lane & 31);
    const bool live = i0 < n;
    const size_t i = live ? i0 : 0;
    uint32_t x[6][5];
#pragma unroll
    for (int T = 0; T < 6; T++) to_mont130(st[i * 12 + 2 * T + pm_h], x[T]);
    pm_permute(&tb, x);
    if (live) {
#pragma unroll
      for (int T = 0; T < 6; T++) st[i * 12 + 2 * T + pm_h] = from_mont130(x[T]);
    }
  }
}

// row hashing, merge level and FRI leaves in the matrix-core form (see hash_rows_kernel,
// merkle_level_kernel, fri_leaf_kernel for the sponge each item runs)
// BIG = false (at most 9 partitions: merge_many absorbs its digests in one block): each lane
// keeps the digests it absorbs (message i = p goes to element p + 1, i.e. slot (p+1)/2 of the
// lanes with h = (p+1) & 1) in registers, taken from the h = 0 lane of its state by a lane
// shuffle, so the kernel's LDS is the 56 KB of tables alone.  BIG = true keeps the per-wave
// digest buffer in LDS (up to PM_MAX_PARTS partitions).
__device__ __forceinline__ fe pm_from_low_half(fe v) {
  const int src = (int)(threadIdx.x & 31);
  const uint32_t w0 = (uint32_t)__shfl((int)(uint32_t)v.lo, src), w1 = (uint32_t)__shfl((int)(uint32_t)(v.lo >> 32), src);
  const uint32_t w2 = (uint32_t)__shfl((int)(uint32_t)v.hi, src), w3 = (uint32_t)__shfl((int)(uint32_t)(v.hi >> 32), src);
  return fe{(uint64_t)w0 | ((uint64_t)w1 << 32), (uint64_t)w2 | ((uint64_t)w3 << 32)};
}

// Prefix skip (DESIGN.md §4 "Column structure"): when the columns feeding the first lead[p]
// absorb blocks of partition p are all zero, constant or periodic in the row, the sponge state
// after those blocks depends only on (row mod Q[p]), Q[p] a power of two.  hash_rows_pm_table_kernel
// computes that state once per residue (table entry = the 12 state elements as 5 Montgomery limbs
// each, [q][element][limb]); hash_rows_pm_prefix_kernel loads it and resumes at block lead[p].
struct PmRowPrefix {
  const uint32_t* table;
  uint32_t lead[PM_PFX_PARTS];   // leading absorb blocks taken from the table (0: none)
  uint32_t qmask[PM_PFX_PARTS];  // Q[p] - 1
  uint32_t off[PM_PFX_PARTS];    // first table entry of partition p
  // zero mask (hash_rows_pm_prefix_kernel): bit j of zeven[p] = column 2j of partition p is all
  // zero, of zodd[p] = column 2j + 1 is all zero or absent; both 0 = no mask, every column loaded
  uint64_t zeven[PM_PFX_PARTS], zodd[PM_PFX_PARTS];
};
constexpr int PM_PFX_ENTRY_WORDS = 60;

template <int TAG, bool BIG>
__global__ __launch_bounds__(PM_ROW_THREADS) void hash_rows_pm_kernel(const fe* __restrict__ M, uint32_t ncols,
                                                                 size_t nrows, uint32_t psize, uint32_t merge,
                                                                 fe* __restrict__ out, int split) {
  __shared__ PmTables tb;
  __shared__ fe dig[BIG ? PM_ROW_WAVES : 1][BIG ? PM_MAX_PARTS : 1][32];  // partition digests of the wave's rows
  pm_load_tables(&tb);
  const uint32_t np = (ncols + psize - 1) / psize;
  const int w = BIG ? (int)(threadIdx.x >> 6) : 0;
  PM_LOOP(nrows) {
    const int n = pm_lane & 31;
    const size_t row0 = pm_b * 32 + (size_t)n;
    const bool live = row0 < nrows;
    const size_t row = live ? row0 : 0;
    fe d = fe_zero();
    fe msg[5] = {fe_zero(), fe_zero(), fe_zero(), fe_zero(), fe_zero()};
    for (uint32_t p = 0; p < np; p++) {
      const uint32_t c0 = p * psize;
      const uint32_t len = min(psize, ncols - c0);
      const fe* base = M + (size_t)c0 * nrows + row;  // position (split: the row is lde_row)
      d = pm_sponge<DOM_ELEMS, TAG == 1>(&tb, live, (int)((len + 1) / 2), [&](int j) {
        fe a = base[(size_t)(2 * j) * nrows];
        fe b = (2u * j + 1 < len) ? base[(size_t)(2 * j + 1) * nrows] : fe_zero();
        return fold_pair(a, b);
      });
      if (merge) {
        if (BIG) {
          if (pm_h == 0) dig[w][p][n] = d;
        } else {
          const fe v = pm_from_low_half(d);
          const int slot = (int)(p + 1) >> 1;
          if ((int)((p + 1) & 1) == pm_h) {
#pragma unroll
            for (int t = 0; t < 5; t++)
              if (t == slot) msg[t] = v;
          }
        }
      }
    }
    if (merge) {
      if (BIG) {
        wave_sync();
        d = pm_sponge<DOM_MANY, TAG == 1>(&tb, live, (int)np, [&](int i) { return dig[w][i][n]; });
        wave_sync();
      } else {
        d = pm_sponge<DOM_MANY, TAG == 1>(&tb, live, (int)np, [&](int i) {
          const int slot = (i + 1) >> 1;
          fe r = msg[0];
#pragma unroll
          for (int t = 1; t < 5; t++)
            if (t == slot) r = msg[t];
          return r;
        });
      }
    }
    if (live && pm_h == 0) out[lde_row(row, nrows, split)] = d;
  }
}

// hash_rows_pm_kernel<0, false> (the trace rows, at most PM_PFX_PARTS partitions, their digests in
// registers) with the partitions the plan names resumed from the prefix table; the others, and
// merge_many, run as there
__global__ __launch_bounds__(PM_ROW_THREADS) void hash_rows_pm_prefix_kernel(const fe* __restrict__ M, uint32_t ncols,
                                                                        size_t nrows, uint32_t psize, uint32_t merge,
                                                                        fe* __restrict__ out, int split, PmRowPrefix A) {
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  const uint32_t np = (ncols + psize - 1) / psize;
  PM_LOOP(nrows) {
    const int n = pm_lane & 31;
    const size_t row0 = pm_b * 32 + (size_t)n;
    const bool live = row0 < nrows;
    const size_t row = live ? row0 : 0;
    fe d = fe_zero();
    fe msg[5] = {fe_zero(), fe_zero(), fe_zero(), fe_zero(), fe_zero()};
    for (uint32_t p = 0; p < np; p++) {
      const uint32_t c0 = p * psize;
      const uint32_t len = min(psize, ncols - c0);
      const fe* base = M + (size_t)c0 * nrows + row;  // position (split: the row is lde_row)
      const int nmsg = (int)((len + 1) / 2);
      const uint32_t lead = A.lead[p];  // wave-uniform
      uint32_t x[6][5];
      if (lead) {
        const size_t q = lde_row(row, nrows, split) & (size_t)A.qmask[p];
        const uint32_t* e = A.table + ((size_t)A.off[p] + q) * PM_PFX_ENTRY_WORDS + pm_h * 5;
#pragma unroll
        for (int T = 0; T < 6; T++)
#pragma unroll
          for (int l = 0; l < 5; l++) x[T][l] = e[T * 10 + l];
      } else {
        pm_sponge_init<DOM_ELEMS>(x);
      }
      // a masked column's load does not issue; where both pairs of a T are zero (scalar test of the
      // mask: pair j is sponge element j + 1) the T is skipped whole
      const uint64_t ze = A.zeven[p], zo = A.zodd[p], zpair = ze & zo;  // wave-uniform
      // first-block pruning applies only to a sponge that starts at block 0 (pm_sponge_blocks)
      pm_sponge_blocks_masked(&tb, live, nmsg, [&](int j, fe& a, fe& b) {  // a, b zero on entry
        if (!((ze >> (j & 63)) & 1)) a = base[(size_t)(2 * j) * nrows];
        if (!(((zo >> (j & 63)) & 1) || 2u * j + 1 >= len)) b = base[(size_t)(2 * j + 1) * nrows];
      }, x, pm_h, 10 * (int)lead, nmsg + 1, [&](int i) {
        const bool z0 = i < 1 || i > nmsg || ((zpair >> ((i - 1) & 63)) & 1);
        const bool z1 = i >= nmsg || ((zpair >> (i & 63)) & 1);
        return z0 && z1;
      });
      d = from_mont130(x[0]);
      if (merge) {
        const fe v = pm_from_low_half(d);
        const int slot = (int)(p + 1) >> 1;
        if ((int)((p + 1) & 1) == pm_h) {
#pragma unroll
          for (int t = 0; t < 5; t++)
            if (t == slot) msg[t] = v;
        }
      }
    }
    if (merge) {
      d = pm_sponge<DOM_MANY, false>(&tb, live, (int)np, [&](int i) {
        const int slot = (i + 1) >> 1;
        fe r = msg[0];
#pragma unroll
        for (int t = 1; t < 5; t++)
          if (t == slot) r = msg[t];
        return r;
      });
    }
    if (live && pm_h == 0) out[lde_row(row, nrows, split)] = d;
  }
}

// Prefix table of the kernel above: for every partition p with lead[p] > 0 and every natural row
// q < Q[p] (stored at position lde_pos(q)), the sponge state after lead[p] absorb blocks, by the
// row kernel's own sponge code.  Partition p owns ceil(Q[p] / 32) batches of 32 rows.
__global__ __launch_bounds__(PM_THREADS) void hash_rows_pm_table_kernel(const fe* __restrict__ M, uint32_t ncols,
                                                                       size_t nrows, uint32_t psize, PmRowPrefix A,
                                                                       uint32_t* __restrict__ table, int split) {
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  const uint32_t np = (ncols + psize - 1) / psize;
  size_t batches = 0;
  for (uint32_t p = 0; p < np; p++) batches += A.lead[p] ? ((size_t)A.qmask[p] + 32) >> 5 : 0;
  PM_LOOP(batches * 32) {
    size_t b = pm_b;
    uint32_t p = 0;
    for (; p + 1 < np; p++) {
      const size_t nb = A.lead[p] ? ((size_t)A.qmask[p] + 32) >> 5 : 0;
      if (b < nb) break;
      b -= nb;
    }
    const size_t q0 = b * 32 + (size_t)(pm_lane & 31);
    const bool live = q0 <= (size_t)A.qmask[p];
    const size_t q = live ? q0 : 0;
    const uint32_t c0 = p * psize;
    const uint32_t len = min(psize, ncols - c0);
    const fe* base = M + (size_t)c0 * nrows + lde_pos(q, nrows, split);
    uint32_t x[6][5];
    pm_sponge_init<DOM_ELEMS>(x);
    pm_sponge_blocks<false>(&tb, live, (int)((len + 1) / 2), [&](int j) {
      fe a = base[(size_t)(2 * j) * nrows];
      fe b2 = (2u * j + 1 < len) ? base[(size_t)(2 * j + 1) * nrows] : fe_zero();
      return fold_pair(a, b2);
    }, x, pm_h, 0, 10 * (int)A.lead[p]);
    if (live) {
      uint32_t* e = table + ((size_t)A.off[p] + q) * PM_PFX_ENTRY_WORDS + pm_h * 5;
#pragma unroll
      for (int T = 0; T < 6; T++)
#pragma unroll
        for (int l = 0; l < 5; l++) e[T * 10 + l] = x[T][l];
    }
  }
}

__global__ __launch_bounds__(PM_THREADS) void merkle_level_pm_kernel(fe* nodes, size_t lvl) {
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  PM_LOOP(lvl) {
    const size_t it = pm_b * 32 + (size_t)(pm_lane & 31);
    const bool live = it < lvl;
    const size_t i = lvl + (live ? it : 0);
    fe d = pm_sponge<DOM_MERGE>(&tb, live, 2, [&](int j) { return nodes[2 * i + j]; });
    if (live && pm_h == 0) nodes[i] = d;
  }
}

__global__ __launch_bounds__(PM_THREADS) void fri_leaf_pm_kernel(const fe* ev, size_t half, fe* leaves) {
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  PM_LOOP(half) {
    const size_t it = pm_b * 32 + (size_t)(pm_lane & 31);
    const bool live = it < half;
    const size_t i = live ? it : 0;
    fe d = pm_sponge<DOM_ELEMS>(&tb, live, 1, [&](int) { return fold_pair(ev[i], ev[i + half]); });
    if (live && pm_h == 0) leaves[i] = d;
  }
}

// transcript draws merge_with_int(seed, base + 1 + i) and grinding tries (see draw_kernel,
// grind_kernel)
__global__ __launch_bounds__(PM_THREADS) void draw_pm_kernel(fe seed, const fe* seed_p, uint64_t base, size_t k,
                                                             fe* out) {
  if (seed_p) seed = *seed_p;
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  PM_LOOP(k) {
    const size_t it = pm_b * 32 + (size_t)(pm_lane & 31);
    const bool live = it < k;
    const uint64_t ctr = base + 1 + (live ? it : 0);
    fe d = pm_sponge<DOM_INT>(&tb, live, 2, [&](int j) { return j == 0 ? seed : fe{ctr, 0}; });
    if (live && pm_h == 0) out[it] = d;
  }
}

__global__ __launch_bounds__(PM_THREADS) void grind_pm_kernel(fe seed, const fe* seed_p, uint64_t base, uint32_t count,
                                                             uint32_t bits, unsigned long long* best) {
  if (seed_p) seed = *seed_p;
  // an earlier window found one (every nonce of an earlier window is below base; a solution
  // this window's other blocks have already found is not a reason to stop)
  if (*(volatile unsigned long long*)best < base) return;
  __shared__ PmTables tb;
  pm_load_tables(&tb);
  PM_LOOP(count) {
    const size_t it = pm_b * 32 + (size_t)(pm_lane & 31);
    const bool live = it < count;
    const uint64_t nonce = base + (live ? it : 0);
    fe hv = pm_sponge<DOM_INT>(&tb, live, 2, [&](int j) { return j == 0 ? seed : fe{nonce, 0}; });
    if (live && pm_h == 0) {
      const uint32_t tz = hv.lo ? (uint32_t)__builtin_ctzll(hv.lo) : 64u;
      if (tz >= bits) atomicMin(best, (unsigned long long)nonce);
    }
  }
}

// ---- 16-state kernels: Merkle levels, FRI leaves, the stage permutation ----------------------
__global__ __launch_bounds__(PM_THREADS) void merkle_level_pm16_kernel(fe* nodes, size_t lvl) {
  __shared__ Pm16Tables tb;
  pm16_load_tables(&tb);
  PM16_LOOP(lvl) {
    const size_t it = pm_b * 16 + (size_t)(pm_lane & 15);
    const bool live = it < lvl;
    const size_t i = lvl + (live ? it : 0);
    fe d = pm16_sponge<DOM_MERGE>(&tb, live, 2, [&](int j) { return nodes[2 * i + j]; });
    if (live && pm_lane < 16) nodes[i] = d;
  }
}

__global__ __launch_bounds__(PM_THREADS) void fri_leaf_pm16_kernel(const fe* ev, size_t half, fe* leaves) {
  __shared__ Pm16Tables tb;
  pm16_load_tables(&tb);
  PM16_LOOP(half) {
    const size_t it = pm_b * 16 + (size_t)(pm_lane & 15);
    const bool live = it < half;
    const size_t i = live ? it : 0;
    fe d = pm16_sponge<DOM_ELEMS>(&tb, live, 1, [&](int) { return fold_pair(ev[i], ev[i + half]); });
    if (live && pm_lane < 16) leaves[i] = d;
  }
}

__global__ __launch_bounds__(PM_THREADS) void pm16_permute_kernel(fe* st, size_t n) {
  __shared__ Pm16Tables tb;
  pm16_load_tables(&tb);
  PM16_LOOP(n) {
    const int g = pm_lane >> 4;
    const size_t i0 = pm_b * 16 + (size_t)(pm_lane & 15);
    const bool live = i0 < n;
    const size_t i = live ? i0 : 0;
    uint32_t x[3][5];
#pragma unroll
    for (int T = 0; T < 3; T++) to_mont130(st[i * 12 + 4 * T + g], x[T]);
    pm16_permute(&tb, x);
    if (live) {
#pragma unroll
      for (int T = 0; T < 3; T++) st[i * 12 + 4 * T + g] = from_mont130(x[T]);
    }
  }
}
