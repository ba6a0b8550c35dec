// Device trace builder: one workgroup per level writes the level's 32 rows of
// every column of the segment from the level's record (tracegen_dev.h).
//
// A level's rows depend on no other level, and a column's 32 rows of one level are 512
// contiguous bytes, so rows sit on lanes: a wavefront stores two columns x 32 rows per
// instruction.  What the host builder computes while writing is recomputed first, by three
// wavefronts side by side, into LDS: the 27 t=12 Poseidon rounds of a squeeze or Merkle level
// (one lane per state element, cubes exchanged by lane shuffles), the 27 t=3 ROM rounds, and the
// four inversions a level can show (eq_inv of the op, and of its three sorted RAM rows).  After
// one barrier every cell is a function of (column, row) over the record and those tables, so
// every cell is written whatever the caller's buffer held.
#include "tracegen_dev.h"

namespace zkl {
namespace {

constexpr int TG_THREADS = 256;

__device__ inline fe shfl_fe(fe v, int lane) {
  return fe{(uint64_t)__shfl((unsigned long long)v.lo, lane), (uint64_t)__shfl((unsigned long long)v.hi, lane)};
}
__host__ __device__ inline fe fe_bit(bool b) { return fe{b ? 1ull : 0ull, 0}; }

// The sorted RAM table as rows (ram.rs:43-271, ram_row in tracegen.cpp): the event shown on
// position p of level lv, -1 for none; *sorted: p is a sorted row.  Event k of the table is
// ev[k - k_base].
__host__ __device__ inline long long ram_row_dev(const TraceGenHeader* H, const RamEventDev* ev, uint64_t lv, int p,
                                        bool* sorted) {
  const uint64_t E = H->n_sorted;
  *sorted = false;
  if (p >= 29) {
    const uint64_t k = 3 * lv + (uint64_t)(p - 29);
    if (k < E) { *sorted = true; return (long long)k; }
    return -1;
  }
  if (lv == 0) return -1;
  const uint64_t i = 3 * lv - 1;
  if (i + 1 < E && fe_eq(ev[i - H->k_base].addr, ev[i + 1 - H->k_base].addr)) return (long long)i;
  return -1;
}

// What sorted RAM row 29 + j of level lv inverts into eq_inv: the address on the next row of the
// full trace (ram.rs:180-230) minus its own; *dbits: its delta_clk bits.  Zero when the row is
// not a sorted row or is the full trace's last.
__host__ __device__ inline fe tg_ram_ahead(const TraceGenHeader* H, const RamEventDev* ev, uint64_t lv, int j,
                                           uint32_t* dbits) {
  const uint64_t E = H->n_sorted, k = 3 * lv + (uint64_t)j, row = lv * 32 + 29 + (uint64_t)j;
  *dbits = 0;
  if (k >= E || row + 1 >= H->n_full) return fe_zero();
  const RamEventDev* e = ev + (k - H->k_base);
  fe an = fe_zero();
  if (k + 1 < E) {
    const RamEventDev* en = e + 1;
    if (j < 2) {  // rows 29, 30: the next sorted event
      an = en->addr;
      if (fe_eq(an, e->addr)) {  // delta_clk bits (saturating difference of level indices)
        const bool pos = e->clk.hi != en->clk.hi ? e->clk.hi < en->clk.hi : e->clk.lo < en->clk.lo;
        *dbits = pos ? (uint32_t)(en->clk.lo - e->clk.lo) : 0u;
      }
    } else if (fe_eq(en->addr, e->addr)) {  // row 31: the next level's map row mirrors this event
      an = e->addr;
    }
  }
  return fe_sub(an, e->addr);
}

struct Tables {
  const fe* lanes;  // [28][12]: state before round j, [27] the output
  const fe* rom;    // [28][3]
  const fe* inv;    // [4]: the op's eq_inv, then rows 29..31
  const uint32_t* dbits;  // [2]: delta_clk bits of rows 29, 30
};

__host__ __device__ inline fe tg_cell(const TraceGenHeader* H, const LevelRec* R, const RamEventDev* ev, const fe* gps,
                      const fe* lws, const Tables& T, uint64_t lv, int c, int p) {
  const Layout& L = H->L;
  const bool mf = p == 0 || p == 28;  // map or final row
  const uint32_t cls = R->cls;
  const bool pose = (cls & (TG_SQUEEZE | TG_MERKLE)) != 0;
  const int st = p == 0 ? 0 : (p - 1 < 27 ? p - 1 : 27);  // row -> round state
  if (c < 12) {
    if (pose) return T.lanes[st * 12 + c];
    return (p == 0 && c >= 10) ? H->dom[c - 10] : fe_zero();
  }
  if (c == L.g_map) return fe_bit(p == 0);
  if (c == L.g_final) return fe_bit(p == 28);
  if (c < L.mask) return fe_bit(p == 1 + (c - L.g_r_start));
  if (c == L.mask) return fe_zero();
  if (c < L.op[0]) return p <= 28 ? R->regs[c - L.r_start] : R->next[c - L.r_start];
  if (c < L.sel_dst0) return fe_bit(mf && (c - L.op[0]) == (int)R->oh);
  if (c < L.sel_s_bits) {
    const int g = (c - L.sel_dst0) >> 3, i = (c - L.sel_dst0) & 7;
    const int d0 = p == 0 ? R->d0_map : R->d0_fin;
    const int reg = g == 0 ? d0 : g == 1 ? R->sa : g == 2 ? R->sb : g == 3 ? R->sc : R->d1;
    return fe_bit(mf && reg == i);
  }
  if (c < L.imm) {
    const bool on = mf && (cls & TG_SPONGE_SEL);
    if (c < L.sel_s_active) {
      const int q = c - L.sel_s_bits, lane = q / 3, bit = q % 3;
      return fe_bit(on && lane < (int)R->nsel && ((R->sel[lane] >> bit) & 1));
    }
    return fe_bit(on && (c - L.sel_s_active) < (int)R->nsel);
  }
  if (c == L.imm) return mf ? R->imm : fe_zero();
  if (c == L.eq_inv) return mf ? T.inv[0] : (p >= 29 ? T.inv[p - 28] : fe_zero());
  if (H->has_ram_cols && c < L.ram_sorted + 8) {
    bool sorted;
    const long long k = ram_row_dev(H, ev, lv, p, &sorted);
    const int f = c - L.ram_sorted;
    if (f == 0) return fe_bit(sorted);
    if (f <= 4) {
      if (k < 0) return fe_zero();
      const RamEventDev* e = ev + ((uint64_t)k - H->k_base);
      return f == 1 ? e->addr : f == 2 ? e->clk : f == 3 ? e->val : e->w;
    }
    if (f == 6) return R->gu[p >= 29];
    const uint64_t E = H->n_sorted;
    uint64_t kb = 3 * lv + (uint64_t)(p > 29 ? p - 29 : 0);  // sorted rows above this one
    if (kb > E) kb = E;
    return f == 5 ? lws[kb - H->k_base] : gps[kb - H->k_base];
  }
  if (H->has_merkle_cols && c >= L.merkle_g && c < L.merkle_g + 7) {
    const bool mk = (cls & TG_MERKLE) != 0;
    const int f = c - L.merkle_g;
    switch (f) {
      case 0: return fe_bit(mk);
      case 1: return (mk && p == 0) ? R->regs[R->mdir] : fe_zero();
      case 2: return (mk && p == 0) ? R->regs[R->msib] : fe_zero();
      case 3: return mk ? (p < 28 ? R->macc : T.lanes[27 * 12]) : fe_zero();
      case 4: return fe_bit(p == 0 && (cls & TG_MFIRST));
      case 5: return fe_bit(p == 28 && (cls & TG_MLAST));
      default: return (p == 0 && (cls & TG_MFIRST)) ? R->macc : fe_zero();
    }
  }
  if (c == L.pi_prog) return (lv == 0 && p == 0 && (cls & TG_VM)) ? H->pi_prog : fe_zero();
  if (c == L.pc) return fe{lv, 0};
  if (c < L.pose_active) return fe_bit(p == 0 && (c - L.rom_op_start) == (int)R->oh);
  if (c == L.pose_active) return fe_bit(pose);
  if (c < L.rom_s) {
    const int i = c - L.gadget_b;
    const uint32_t w = mf ? R->gbits : (p == 29 || p == 30) ? T.dbits[p - 29] : 0u;
    return fe_bit((w >> i) & 1u);
  }
  return T.rom[st * 3 + (c - L.rom_s)];
}

__global__ void __launch_bounds__(TG_THREADS)
trace_fill_kernel(const unsigned char* __restrict__ blob, uint32_t n_levels, uint32_t width, fe* __restrict__ out) {
  __shared__ fe s_lanes[28 * 12];
  __shared__ fe s_rom[28 * 3];
  __shared__ fe s_inv[4];
  __shared__ uint32_t s_dbits[2];
  const TraceGenHeader* H = (const TraceGenHeader*)blob;
  const uint32_t li = blockIdx.x;
  if (li >= n_levels) return;
  const LevelRec* R = (const LevelRec*)(blob + H->off_recs) + li;
  const RamEventDev* ev = (const RamEventDev*)(blob + H->off_sorted);
  const fe* gps = (const fe*)(blob + H->off_gp_sorted);
  const fe* lws = (const fe*)(blob + H->off_last_write);
  const uint64_t lv = (uint64_t)H->level0 + li;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t cls = R->cls;

  if (wave == 0) {
    // t=12 Poseidon lanes (vm/trace/poseidon.rs:9-87): the whole wavefront runs the rounds, lane
    // i < 12 owns state element i (the others repeat element 11 and store nothing)
    if (cls & (TG_SQUEEZE | TG_MERKLE)) {
      const int i = lane < 12 ? lane : 11;
      fe s = fe_zero();
      if (i >= 10) {
        s = H->dom[i - 10];
      } else if (cls & TG_MERKLE) {  // (1 - d) acc + d sib, (1 - d) sib + d acc
        if (i < 2) {
          const fe d = R->regs[R->mdir], sib = R->regs[R->msib], acc = R->macc, nd = fe_sub(fe_one(), d);
          s = i == 0 ? fe_add(fe_mul(nd, acc), fe_mul(d, sib)) : fe_add(fe_mul(nd, sib), fe_mul(d, acc));
        }
      } else if (i < (int)R->nsel) {
        s = R->regs[R->sel[i]];
      }
      if (lane < 12) s_lanes[i] = s;
      for (int j = 0; j < 27; j++) {
        const fe s3 = fe_cube(s);
        uint32_t acc[9];
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] = 0;
        for (int k = 0; k < 12; k++) mul_acc(H->mds[i][k], shfl_fe(s3, k), acc);
        s = fe_add(reduce288(acc), H->rc[j][i]);
        if (lane < 12) s_lanes[(j + 1) * 12 + i] = s;
      }
    }
  } else if (wave == 1) {
    // t=3 ROM rounds (rom.rs:37-106) of every level
    const int i = lane < 3 ? lane : 2;
    fe s = R->rom[i];
    if (lane < 3) s_rom[i] = s;
    for (int j = 0; j < 27; j++) {
      const fe s3 = fe_cube(s);
      uint32_t acc[9];
#pragma unroll
      for (int q = 0; q < 9; q++) acc[q] = 0;
      for (int k = 0; k < 3; k++) mul_acc(H->mds3[i][k], shfl_fe(s3, k), acc);
      s = fe_add(reduce288(acc), H->rc3[j][i]);
      if (lane < 3) s_rom[(j + 1) * 3 + i] = s;
    }
  } else if (wave == 2) {
    // eq_inv: lane 0 the op's (Eq, DivMod, DivMod128; 64-bit range stages stage 1), lanes 1..3
    // the sorted RAM rows 29..31, which look one row ahead in the full trace (ram.rs:180-230)
    if (lane < 4) {
      fe x = fe_zero();
      uint32_t dbits = 0;
      if (lane == 0) {
        x = R->inv_in;
      } else if (H->prog_ram) {
        x = tg_ram_ahead(H, ev, lv, lane - 1, &dbits);
      }
      s_inv[lane] = fe_inv(x);
      if (lane == 1 || lane == 2) s_dbits[lane - 1] = dbits;
    }
  }
  __syncthreads();

  const Tables T{s_lanes, s_rom, s_inv, s_dbits};
  const size_t m = (size_t)n_levels * 32;
  const int p = tid & 31;
  for (uint32_t c = (uint32_t)tid >> 5; c < width; c += TG_THREADS / 32)
    out[(size_t)c * m + (size_t)li * 32 + p] = tg_cell(H, R, ev, gps, lws, T, lv, (int)c, p);
}

}  // namespace

// The same fill on the host: the tables of a level by plain loops, then the kernel's own cell
// function over every (column, row).
void trace_fill_host(const void* blob_v, fe* out) {
  const unsigned char* blob = (const unsigned char*)blob_v;
  const TraceGenHeader* H = (const TraceGenHeader*)blob;
  const RamEventDev* ev = (const RamEventDev*)(blob + H->off_sorted);
  const fe* gps = (const fe*)(blob + H->off_gp_sorted);
  const fe* lws = (const fe*)(blob + H->off_last_write);
  const size_t m = (size_t)H->n_levels * 32;
  for (uint32_t li = 0; li < H->n_levels; li++) {
    const LevelRec* R = (const LevelRec*)(blob + H->off_recs) + li;
    const uint64_t lv = (uint64_t)H->level0 + li;
    fe lanes[28 * 12], rom[28 * 3], inv[4];
    uint32_t dbits[2] = {0, 0};
    if (R->cls & (TG_SQUEEZE | TG_MERKLE)) {
      fe* s = lanes;
      for (int i = 0; i < 12; i++) s[i] = fe_zero();
      if (R->cls & TG_MERKLE) {
        const fe d = R->regs[R->mdir], sib = R->regs[R->msib], acc = R->macc, nd = fe_sub(fe_one(), d);
        s[0] = fe_add(fe_mul(nd, acc), fe_mul(d, sib));
        s[1] = fe_add(fe_mul(nd, sib), fe_mul(d, acc));
      } else {
        for (int i = 0; i < (int)R->nsel; i++) s[i] = R->regs[R->sel[i]];
      }
      s[10] = H->dom[0];
      s[11] = H->dom[1];
      for (int j = 0; j < 27; j++, s += 12)
        for (int i = 0; i < 12; i++) {
          fe acc = fe_zero();
          for (int k = 0; k < 12; k++) acc = fe_add(acc, fe_mul(H->mds[i][k], fe_cube(s[k])));
          s[12 + i] = fe_add(acc, H->rc[j][i]);
        }
    }
    for (int i = 0; i < 3; i++) rom[i] = R->rom[i];
    for (int j = 0; j < 27; j++)
      for (int i = 0; i < 3; i++) {
        fe acc = fe_zero();
        for (int k = 0; k < 3; k++) acc = fe_add(acc, fe_mul(H->mds3[i][k], fe_cube(rom[3 * j + k])));
        rom[3 * (j + 1) + i] = fe_add(acc, H->rc3[j][i]);
      }
    inv[0] = fe_inv(R->inv_in);
    for (int j = 0; j < 3; j++) {
      uint32_t db = 0;
      inv[1 + j] = H->prog_ram ? fe_inv(tg_ram_ahead(H, ev, lv, j, &db)) : fe_zero();
      if (j < 2) dbits[j] = db;
    }
    const Tables T{lanes, rom, inv, dbits};
    for (uint32_t c = 0; c < H->width; c++)
      for (int p = 0; p < 32; p++) out[(size_t)c * m + (size_t)li * 32 + p] = tg_cell(H, R, ev, gps, lws, T, lv, (int)c, p);
  }
}

void launch_trace_fill(const void* d_blob, uint32_t n_levels, uint32_t width, fe* d_out, hipStream_t s) {
  hipLaunchKernelGGL(trace_fill_kernel, dim3(n_levels), dim3(TG_THREADS), 0, s, (const unsigned char*)d_blob, n_levels,
                     width, d_out);
}

}  // namespace zkl
