// Device trace builder: what the host stages for one segment (tracegen.cpp), and
// the kernel that fills the segment's trace from it (tracegen.hip).
//
// The serial part of a program -- the VM carry, ROM lane 0, the sorted RAM table -- is done once
// by zkl_program_new.  Per segment the host writes one LevelRec per level (what the level's 32
// rows are a function of), the slices of the sorted RAM table and its prefix sums the window's
// rows show, and the program's constants into one blob; the kernel recomputes the Poseidon and
// ROM rounds, the inversions and the bit columns and writes every cell of the output.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/zkl_hip.h"
#include "air_host.h"
#include "field.h"

namespace zkl {

// One level (32 rows).  Registers a level does not show (padding levels) are staged as zeros.
struct alignas(16) LevelRec {
  fe regs[8];      // r0..r7 on rows 0..28
  fe next[8];      // ... and on rows 29..31
  fe macc;         // Merkle accumulator entering the level (the leaf for a first step)
  fe imm;          // the imm column on the map and final rows (a load's value rides here)
  fe inv_in;       // eq_inv on the map and final rows is 1 / inv_in (zero stays zero)
  fe rom[3];       // ROM state on the map row: lane 0 carried in, the op's two encodings
  fe gu[2];        // ram_gp_unsorted on rows 0..28 and on rows 29..31
  uint32_t gbits;  // the 32 gadget bits of the map and final rows
  int8_t oh;       // op / ROM one-hot index, -1 for none
  uint8_t cls;     // TG_* flags
  // the register each selector group names, -1 for none: dst0 on the map row, dst0 on the final
  // row (a squeeze sets it there alone), a, b, c, dst1 on both
  int8_t d0_map, d0_fin, sa, sb, sc, d1;
  uint8_t nsel;     // sponge lanes in use on this level
  uint8_t sel[10];  // ... and the register each reads
  uint8_t mdir, msib;  // Merkle direction and sibling registers
};
enum : uint8_t {
  TG_SPONGE_SEL = 1,  // absorb or squeeze: lane selectors on the map and final rows
  TG_SQUEEZE = 2,     // the t=12 permutation over the selected registers
  TG_MERKLE = 4,      // the t=12 permutation over the ordered (accumulator, sibling) pair
  TG_MFIRST = 8,
  TG_MLAST = 16,
  TG_VM = 32,  // not a padding level: registers and (level 0) the program word are shown
};

struct RamEventDev {
  fe addr, clk, val, w;
};

// Blob header; the arrays follow at the byte offsets it names (all multiples of 16).
struct alignas(16) TraceGenHeader {
  Layout L;  // the segment's layout
  uint32_t width, n_levels, level0, has_ram_cols, has_merkle_cols, prog_ram;
  uint64_t n_full;     // rows of the program's full trace (the RAM builder's `n`)
  uint64_t n_sorted;   // events in the sorted RAM table
  uint64_t k_base;     // first sorted event / prefix index in the slices
  uint64_t off_recs, off_sorted, off_gp_sorted, off_last_write;
  fe pi_prog, dom[2];
  fe mds[12][12], rc[27][12], mds3[3][3], rc3[27][3];
};

struct TraceGenStage {
  uint32_t width = 0, rows = 0;
  size_t bytes = 0;  // of the blob
};

// Shape and blob size of rows [r_start, r_end) (no other work); ZKL_E_INVALID as
// zkl_build_segment_trace.
int tracegen_stage_size(const zkl_program* p, uint32_t r_start, uint32_t r_end, TraceGenStage* st);
// Fills blob (st->bytes, 16-byte aligned) and the segment's public inputs and state hashes.
int tracegen_stage(const zkl_program* p, uint32_t r_start, uint32_t r_end, const TraceGenStage* st, void* blob,
                   zkl_air_public_inputs* pi, uint8_t state_in[32], uint8_t state_out[32]);

// out[width x 32 n_levels] (column-major) <- the segment d_blob describes; every cell is written.
void launch_trace_fill(const void* d_blob, uint32_t n_levels, uint32_t width, fe* d_out, hipStream_t s);

// The same fill on the host through the kernel's cell function (no device): what the CPU suite
// compares with the host builder.
void trace_fill_host(const void* blob, fe* out);

}  // namespace zkl

// Test hook, not part of the public ABI: zkl_build_segment_trace's contract, computed by staging
// the segment as for the device and running trace_fill_host.
extern "C" int zkl_tracegen_host_fill(const zkl_program* prog, uint32_t r_start, uint32_t r_end, zkl_f128* trace_out,
                                      zkl_air_public_inputs* pi_out, uint32_t* width_out, uint8_t state_in[32],
                                      uint8_t state_out[32]);
