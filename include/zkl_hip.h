/*
 * zkl_hip.h — C ABI of the MI355X-native zk-lisp segment prover (libzkl_hip.so).
 *
 * One call proves one zk-lisp execution segment and returns the bytes of the
 * inner STARK proof, i.e. what the reference gets from
 *   ZkWinterfellProver.prove(trace)           zk-lisp-proof-winterfell/src/prove.rs:225
 * inside
 *   prove_segment(...)                        zk-lisp-proof-winterfell/src/prove.rs:1057-1175
 * (the call at prove.rs:1142, `prover.prove(trace)?`).  The Rust side would
 * `Proof::from_bytes` the result and continue at prove.rs:1144.  The binding a
 * maintainer adds on the Rust side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - field elements are f128 (p = 2^128 - 45*2^40 + 1), canonical (< p),
 *    little-endian limbs {lo, hi}; the same value `BaseElement::as_int()` gives.
 *  - traces are column-major: element (col, row) at trace[col * n_rows + row].
 *  - every function returns 0 on success and a negative ZKL_E_* code on failure;
 *    zkl_hip_last_error() then returns a message (the reference maps failures to
 *    prove::Error::Backend(String), prove.rs:225-227; same shape here).
 *  - the library owns nothing the caller passed in; proof buffers it returns are
 *    released with zkl_hip_free().
 *  - one zkl_ctx per device; calls on one ctx are serialised internally, calls
 *    on different ctx run concurrently (reference calls prove_segment from a
 *    rayon pool, prove.rs:1020-1048).
 */
#ifndef ZKL_HIP_H
#define ZKL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKL_ABI_VERSION 1

enum {
  ZKL_OK = 0,
  ZKL_E_INVALID = -1,   /* bad argument / unsupported configuration */
  ZKL_E_DEVICE = -2,    /* HIP runtime error */
  ZKL_E_OOM = -3,       /* device or host allocation failed */
  ZKL_E_INTERNAL = -4,  /* internal consistency check failed */
};

typedef struct { uint64_t lo, hi; } zkl_f128;

/* winterfell::ProofOptions as built at prove.rs:963-972 + with_partitions(prove.rs:1121).
 * field_extension: 1 = None (FieldExtension discriminant); only None is supported for
 * step proofs.  batching_*: 0 = Linear (BatchingMethod discriminant). */
typedef struct {
  uint32_t num_queries;              /* CLI default 64 (zk-lisp-cli/src/main.rs:124-132) */
  uint32_t blowup_factor;            /* 16 */
  uint32_t grinding_factor;          /* 16 */
  uint32_t field_extension;          /* 1 = None */
  uint32_t fri_folding_factor;       /* 2 */
  uint32_t fri_remainder_max_degree; /* 1 */
  uint32_t batching_constraints;     /* 0 = Linear */
  uint32_t batching_deep;            /* 0 = Linear */
  uint32_t num_partitions;           /* select_partitions_for_trace, utils.rs:394-409 */
  uint32_t hash_rate;                /* idem */
} zkl_proof_options;

#define ZKL_MAX_MAIN_SLOTS 8

/* crate::AirPublicInputs (zk-lisp-proof-winterfell/src/lib.rs:75-95) flattened.
 * `core` fields are the subset of zk_lisp_proof::pi::PublicInputs (pi.rs:62-88)
 * that ZkLispAir::new / get_assertions / to_elements read.  main_args are given
 * already flattened into base-field slots (utils::encode_main_args_to_slots). */
typedef struct {
  uint8_t program_id[32];
  uint8_t program_commitment[32];
  uint8_t merkle_root[32];
  uint64_t feature_mask;          /* core.feature_mask (FM_* bits, pi.rs:23-28) */
  uint64_t segment_feature_mask;  /* effective per-segment mask (prove.rs:1078-1083) */
  uint32_t n_main_slots;
  zkl_f128 main_slots[ZKL_MAX_MAIN_SLOTS];
  uint32_t vm_out_reg;
  uint32_t vm_out_row;
  uint8_t vm_expected_bytes[32];
  zkl_f128 rom_acc[3];
  zkl_f128 pc_init;
  zkl_f128 ram_gp_unsorted_in, ram_gp_unsorted_out, ram_gp_sorted_in, ram_gp_sorted_out;
  zkl_f128 rom_s_in[3];
  zkl_f128 rom_s_out[3];
  uint32_t vm_usage_mask;
  uint32_t ram_delta_clk_bits;
} zkl_air_public_inputs;

/* ---- zl1 step proof (a18) --------------------------------------------------------
 * zk_lisp_proof::pi::VmArg (pi.rs) for the ZKLSTP1 encoding: tag 0 = U64 (bytes[0..8] LE),
 * 1 = U128 (bytes[0..16] LE), 2 = Bytes32. */
typedef struct {
  uint32_t tag;
  uint8_t bytes[32];
} zkl_vm_arg;

/* What prove_segment (prove.rs:1057-1175) feeds Proof::new_multi_segment (format.rs:105-148)
 * and StepProof besides the inner proof and the AirPublicInputs: the suite id (= program_id,
 * prove.rs:985), the security target echoed as lambda (opts.min_security_bits, prove.rs:634),
 * the segment position, the VM state hashes from the trace builder and the
 * SegmentBoundaryBytes (prove.rs:1112), and the typed main_args of the core public inputs. */
typedef struct {
  uint8_t suite_id[32];
  uint32_t lambda_bits;
  uint32_t segment_index, segments_total;
  uint8_t pc_init[32];
  uint8_t state_in_hash[32], state_out_hash[32];
  uint8_t ram_gp_unsorted_in[32], ram_gp_unsorted_out[32], ram_gp_sorted_in[32], ram_gp_sorted_out[32];
  uint8_t rom_s_in[3][32];
  uint8_t rom_s_out[3][32];
  uint32_t n_main_args;
  zkl_vm_arg main_args[ZKL_MAX_MAIN_SLOTS];
} zkl_step_info;

/* Per-stage wall times of the last proof on a ctx, milliseconds; stage names follow
 * the reference's tracing events (prove.rs:464-513): trace_lde, trace_commit,
 * coefficients, evaluator, constraint_commitment, ood, deep, fri, grind, queries. */
#define ZKL_NUM_STAGES 10

typedef struct zkl_ctx zkl_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int zkl_hip_init(int device, zkl_ctx** out);
void zkl_hip_destroy(zkl_ctx* ctx);
const char* zkl_hip_last_error(const zkl_ctx* ctx); /* ctx may be NULL */
void zkl_hip_free(uint8_t* buf);
int zkl_hip_abi_version(void);
/* compiled-in tuning values of the kernels ("NAME=value;..."): every value is a supported,
 * parity-tested configuration (no timing probes are compiled in; tests/test_abi.py) */
const char* zkl_hip_build_config(void);

/* ---- process-level settings (opt-in) --------------------------------------------------
 * zkl_hip_init changes nothing outside the library.  These process-wide settings helped the
 * prover on some hosts and are the embedding application's choice:
 *   ZKL_TUNE_SPIN    hipSetDeviceFlags(hipDeviceScheduleSpin) on every visible device: host waits
 *                    on the device spin instead of sleeping (a blocking wait was seen to wake
 *                    20-30 ms late); costs one host core per waiting context.  Takes effect only
 *                    before the first zkl_hip_init / HIP context of the process.
 *   ZKL_TUNE_MALLOC  glibc mallopt: mmap threshold 32 MiB, top pad 64 MiB, trim threshold 2 GiB --
 *                    the process keeps freed heap memory instead of returning it to the kernel
 *                    (memory returned while a proof ran was followed by idle GPU time).
 *                    Changes the allocator of the whole host process.
 * *applied receives the flags that took effect; ZKL_OK if all requested did. */
#define ZKL_TUNE_SPIN 1u
#define ZKL_TUNE_MALLOC 2u
int zkl_hip_process_tuning(uint32_t flags, uint32_t* applied);

/* ---- the drop-in: one segment proof ----------------------------------------
 * Replaces ZkProver::prove -> winterfell::Prover::prove (prove.rs:174-257) for
 * ZkLispAir + PoseidonHasher + MerkleTree + DefaultRandomCoin (prove.rs:425-437).
 * trace: host pointer, column-major width x n_rows.  Output: Proof::to_bytes(). */
int zkl_hip_prove_segment(zkl_ctx* ctx, const zkl_f128* trace, uint32_t width, uint32_t n_rows,
                          const zkl_air_public_inputs* pi, const zkl_proof_options* opts,
                          uint8_t** proof_out, size_t* proof_len);

/* The same proof from the trace as a Winterfell TraceTable holds it: columns[c] is a host pointer
 * to the n_rows elements of column c, or NULL for an all-zero column, so a binding passes
 * trace.get_column(c).as_ptr() per column and builds no contiguous copy.  The caller must not
 * write the columns during the call.  The request checks of zkl_hip_check_request that concern
 * the shape (options, n_rows, width = the segment layout's width) run before any device work and
 * before a column pointer is read; a NULL `columns` is ZKL_E_INVALID.  Same bytes as
 * zkl_hip_prove_segment of the flattened trace; they stay available through zkl_hip_last_proof.
 *
 * Both host entry points stage the trace the same way (zkl_hip_prove_segment is this call with
 * columns[c] = trace + c * n_rows): host threads classify every column while they read it (the
 * rule of zkl_hip_scan_columns; a period that is not below n_rows counts as general), copy only
 * the general columns into pinned memory and upload those, plus the first min(128, n_rows) rows
 * of the periodic ones; the device then runs the structured trace LDE of a resident trace.  A
 * trace inside a zkl_hip_trace_buffer is DMA'd in place instead and keeps the dense LDE. */
int zkl_hip_prove_segment_columns(zkl_ctx* ctx, const zkl_f128* const* columns, uint32_t width, uint32_t n_rows,
                                  const zkl_air_public_inputs* pi, const zkl_proof_options* opts,
                                  uint8_t** proof_out, size_t* proof_len);
/* What the last host-trace proof or zkl_hip_lde_columns_host call on ctx staged: the classes the
 * host found, the trace bytes copied into pinned memory and the trace bytes DMA'd (both
 * (general x n_rows + periodic x min(128, n_rows)) x 16 on the staged path), and the chunks of
 * general columns issued.  A call that read nothing on the host (a pinned trace buffer, the
 * preflight's whole upload) reports width general columns, width x n_rows x 16 bytes DMA'd and 0
 * bytes pinned. */
typedef struct {
  uint32_t cols_zero, cols_periodic, cols_general, chunks;
  uint64_t bytes_pinned, bytes_dma;
} zkl_upload_stats;
int zkl_hip_upload_stats(const zkl_ctx* ctx, zkl_upload_stats* out);
/* General columns per staged chunk for the following host-trace calls on ctx: 0 (default) = what
 * a pinned slot holds (slot bytes / column bytes), k > 0 = at most k, clamped so that a chunk
 * fits a slot.  Results do not depend on it; small shapes use it to run the multi-chunk ring. */
int zkl_hip_set_upload_chunk_columns(zkl_ctx* ctx, uint32_t k);

/* Pinned host buffers owned by ctx for the next traces: slot 0 .. ZKL_TRACE_BUFFERS - 1, each at
 * least `bytes` (grown when needed, kept across proofs, freed by zkl_hip_destroy).  The caller
 * fills one -- zkl_build_segment_trace can write a segment straight into it -- and passes it as
 * `trace` to zkl_hip_prove_segment, which then DMAs the columns from it with no staging copy and no
 * per-proof host allocation on the caller's side (prove.rs:1103-1142 allocates a fresh TraceTable
 * per segment and drops it after the proof).  Two slots let the next segment be built while the
 * current one proves.  A slot must not be written while a proof reads it; valid until the next
 * call that grows it. */
#define ZKL_TRACE_BUFFERS 2
int zkl_hip_trace_buffer(zkl_ctx* ctx, uint32_t slot, size_t bytes, zkl_f128** out);
/* Pinned host memory the library holds across all contexts of the process (trace buffers,
 * upload slots, transcript / gather / proof staging): bytes now and the peak since load.  No
 * device work; for capacity planning (8 ranks x in-flight contexts on one host). */
int zkl_hip_pinned_bytes(uint64_t* current, uint64_t* peak);

/* Same, with the trace already resident in HBM (device pointer on ctx's device,
 * column-major).  Used by the multi-segment pipeline and by bench.py. */
int zkl_hip_prove_segment_device(zkl_ctx* ctx, const void* d_trace, uint32_t width, uint32_t n_rows,
                                 const zkl_air_public_inputs* pi, const zkl_proof_options* opts,
                                 uint8_t** proof_out, size_t* proof_len);

/* The same proof written into caller memory (no allocation, one copy): for a binding that keeps
 * one buffer across segments (e.g. a Vec<u8> reserved once and set_len'd; the reference's
 * Proof::to_bytes at prove.rs:1142 allocates per proof).  *proof_len receives the size; with
 * cap too small (or buf NULL, a size query) the call returns ZKL_E_INVALID (NULL: ZKL_OK) and
 * the bytes stay on the context for zkl_hip_last_proof. */
int zkl_hip_prove_segment_device_into(zkl_ctx* ctx, const void* d_trace, uint32_t width, uint32_t n_rows,
                                      const zkl_air_public_inputs* pi, const zkl_proof_options* opts,
                                      uint8_t* buf, size_t cap, size_t* proof_len);

/* The last proof made on ctx (any zkl_hip_prove_segment* call), valid until the next one:
 * *len = its size; copied into buf when buf != NULL and cap >= *len (ZKL_E_INVALID when cap is
 * too small or no proof is held). */
int zkl_hip_last_proof(zkl_ctx* ctx, uint8_t* buf, size_t cap, size_t* len);

/* The request checks zkl_hip_prove_segment* run before any device work, without a device:
 * ProofOptions / PartitionOptions bounds (num_queries 1..255, blowup a power of two >= 2 and
 * >= the AIR's constraint-evaluation blowup, num_partitions 1..16, hash_rate 1..256, FRI
 * folding 2, remainder degree 2^k - 1), the supported options (FieldExtension::None,
 * BatchingMethod::Linear), the trace shape (n_rows a power of two >= 32, width = the segment
 * layout's width) and the public-input shape (n_main_slots <= ZKL_MAX_MAIN_SLOTS, assertion
 * count = AirContext::num_assertions).  ZKL_OK or ZKL_E_INVALID + zkl_hip_last_error(NULL). */
int zkl_hip_check_request(uint32_t width, uint32_t n_rows, const zkl_air_public_inputs* pi,
                          const zkl_proof_options* opts);

/* ---- trace preflight (the reference's preflight.rs:73-440, run from prove.rs:188-212) --------
 * A trace check on the device that names what is wrong with a trace: the first row (below
 * n_rows - 1; the last row is the transition exemption) with a non-zero transition constraint
 * of ZkLispAir, the first such constraint in evaluation order and its value -- what
 * preflight.rs reports -- or, when every transition holds, the first assertion of the AIR
 * (Winterfell order) whose trace cell differs, which winterfell's debug `validate` covers.
 *
 * The device pass is a filter: a row fails iff sum_j alpha_j c_j != 0 for n_tc coefficients
 * drawn from hash_elements(pi_elements | [width, n_rows, seed_lo, seed_hi]); the failing row is
 * then resolved exactly on the host, constraint by constraint.  A row with some c_j != 0 is
 * missed with probability 2^-128 for a trace fixed independently of `seed` (default 0, so runs
 * reproduce).  This is a diagnostic, not a soundness argument: a trace built to fit one seed's
 * coefficients passes the filter under that seed; the proof itself still fails for it.
 *
 * The report mirrors PreflightReport (preflight.rs:29-70) without its VmSnap, which keys on
 * literal constraint indices of one layout, and without the compiler statistics. */
typedef struct {
  uint32_t kind;            /* 0 none, 1 transition constraint, 2 assertion */
  uint32_t index;           /* constraint index, or position in the AIR's assertion order */
  uint32_t row, pos;        /* failing row; pos = row % 32 */
  zkl_f128 value;           /* c_index at that row, or the trace cell of a failing assertion */
  uint32_t column;          /* assertions: the asserted column ... */
  uint32_t lanes_exp_valid; /* lanes_exp is set (Poseidon block present and index < 27 * 12) */
  zkl_f128 expected;        /* ... and the asserted value */
  zkl_f128 g_map, g_final;  /* the schedule gate columns of the row */
  uint32_t round_gates;     /* bit j: round gate j of the row is 1 (27 bits) */
  uint32_t ram_valid;       /* ram is set (the layout has RAM columns) */
  zkl_f128 lanes_cur[4], lanes_next[4]; /* lanes l, r, c0, c1 of the row and the next */
  zkl_f128 lanes_exp[4];    /* MDS s^3 + rc[index / 12] for those lanes (preflight.rs:204-229) */
  /* RamSnap: sorted, addr cur/next, clk cur/next, val, is_write, last_write cur/next,
   * gp_unsorted cur/next, gp_sorted cur/next (preflight.rs:232-250) */
  zkl_f128 ram[13];
} zkl_trace_report;

/* Check a trace resident on ctx's device (column-major).  The request's shape checks run first
 * (n_rows a power of two >= 32, width = the segment layout's, the public-input shape):
 * ZKL_E_INVALID.  Otherwise ZKL_OK with out->kind = 0 or a finding; a finding is not an error of
 * the call.  ZKL_E_INTERNAL if the device flags a row in which the host finds no violation. */
int zkl_hip_check_trace_device(zkl_ctx* ctx, const void* d_trace, uint32_t width, uint32_t n_rows,
                               const zkl_air_public_inputs* pi, uint64_t seed, zkl_trace_report* out);
/* The same for a host trace, uploaded whole into a device buffer the context owns. */
int zkl_hip_check_trace(zkl_ctx* ctx, const zkl_f128* trace, uint32_t width, uint32_t n_rows,
                        const zkl_air_public_inputs* pi, uint64_t seed, zkl_trace_report* out);
/* Per context, default off (the reference's PreflightMode::Off).  When on, every
 * zkl_hip_prove_segment_device* call checks d_trace first (seed 0), and zkl_hip_prove_segment
 * uploads the host trace whole, checks it and proves from that resident copy (the chunked upload
 * transforms chunks in place, so it cannot be checked row-wise).  A finding returns
 * ZKL_E_INVALID with no proof and no LDE work; zkl_hip_last_error is the reference's text with
 * the value as a decimal integer,
 *   preflight: constraint 94 non-zero at row 299: 1
 *   preflight: assertion {k} (column {c}) fails at row {r}: trace {v}, expected {e}
 * and the report stays readable through zkl_hip_last_trace_report.  Proof bytes are the same
 * with it on or off. */
int zkl_hip_set_preflight(zkl_ctx* ctx, int on);
int zkl_hip_preflight(const zkl_ctx* ctx);
/* The report of the last check on ctx (either entry point above, or a prove call's preflight);
 * ZKL_E_INVALID when none was made. */
int zkl_hip_last_trace_report(zkl_ctx* ctx, zkl_trace_report* out);
/* Host only, no ctx: the values c_0 .. c_(n_tc - 1) of ZkLispAir's transition constraints on the
 * frame (cur, next) = rows (row, row + 1) of a width x n_rows trace, row < n_rows - 1, in the
 * reference's evaluation order.  *n_tc receives their number; values NULL only queries it,
 * otherwise cap >= *n_tc entries are written.  The preflight's exact resolution step. */
int zkl_eval_transition_row(uint32_t width, uint32_t n_rows, const zkl_air_public_inputs* pi, uint32_t row,
                            const zkl_f128* cur, const zkl_f128* next, zkl_f128* values, uint32_t cap,
                            uint32_t* n_tc);

/* Host-side wall times (ms) of the last proof on ctx: [0] host setup before the first
 * kernel (AIR instance, assertions, uploads), [1] host time between the first and last
 * stage marks not covered by device work, [2] the whole call, [3] the host-trace upload loop
 * of zkl_hip_prove_segment (pinned staging + DMA issue; 0 for the device entry point).
 * Returns number written. */
int zkl_hip_host_times(const zkl_ctx* ctx, double* out_ms, int max_n);

/* Stage timings (ms) of the last proof on ctx; returns number written.  Recorded only for
 * proofs run with zkl_hip_set_kernel_timing(ctx, 2) (zeros otherwise: each stage event
 * costs queue time on the proof stream). */
int zkl_hip_stage_times(const zkl_ctx* ctx, double* out_ms, int max_n);

/* Per-kernel-family device time of the last proof, measured with HIP events on the
 * ctx stream around each launch: out_ms[i] = summed ms, out_launches[i] = launches.
 * *names receives a static '\n'-separated list of the family names. */
#define ZKL_NUM_KFAMILIES 9
int zkl_hip_kernel_times(const zkl_ctx* ctx, double* out_ms, int* out_launches, int max_n, const char** names);
/* Which kernel families zkl_hip_kernel_times covers for the following proofs: 0 none,
 * 1 the trace row hash only (default: every bracket costs ~10 us of queue time), 2 all
 * families and the stage boundaries of zkl_hip_stage_times. */
int zkl_hip_set_kernel_timing(zkl_ctx* ctx, int mode);

/* ---- device memory (the library's own HIP runtime; callers need no torch) --- */
int zkl_hip_device_count(int* count);
int zkl_hip_device_alloc(zkl_ctx* ctx, size_t bytes, void** d_ptr);
int zkl_hip_device_free(zkl_ctx* ctx, void* d_ptr);
/* kind: 1 = host->device, 2 = device->host, 3 = device->device; synchronous */
int zkl_hip_memcpy(zkl_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
int zkl_hip_synchronize(zkl_ctx* ctx);

/* ---- reference helpers the host needs on its side ------------------------ */
/* utils::select_partitions_for_trace (utils.rs:394-409). */
void zkl_select_partitions(uint32_t trace_width, uint32_t trace_length,
                           uint32_t* num_partitions, uint32_t* hash_rate);

/* ---- stage entry points (parity tests call these through the same ABI) ----- */
/* PoseidonHasher::hash_elements over each row of a column-major matrix, with the
 * row partitioning Winterfell applies (partition_size, merge_many); d_* are device
 * pointers on ctx's device.  digests_out: n_rows field elements (digest low 16 B). */
int zkl_hip_hash_rows(zkl_ctx* ctx, const void* d_matrix, uint32_t n_cols, uint32_t n_rows,
                      uint32_t num_partitions, uint32_t hash_rate, void* d_digests_out);
/* MerkleTree::new over n_leaves digests (field-element form); writes all 2*n nodes
 * (nodes[1] = root, nodes[n+i] = leaf i) to d_nodes_out. */
int zkl_hip_merkle_tree(zkl_ctx* ctx, const void* d_leaves, uint32_t n_leaves, void* d_nodes_out);
/* n_states Poseidon permutations (poseidon/hasher.rs:173-190, suite [0;32]) of 12-element
 * canonical states, in place.  engine 1 = matrix-core form (the one the commitment kernels
 * use on large levels), 2 = its 16-state form (levels of 2^13 and 2^14 states), 0 = lane-group
 * form.  Stage entry point for parity tests. */
int zkl_hip_poseidon_permute(zkl_ctx* ctx, void* d_states, uint32_t n_states, int engine);
/* Process-wide hashing policy: engine 1 (default) runs Poseidon levels of at least
 * pm_min_items states (default 16384) on the 32-state matrix-core permutation, and Merkle
 * levels and FRI leaf layers inside the 16-state band (default [2^13, 2^15) states,
 * ZKL_PM16=lo,hi moves it, ZKL_PM16=0 disables it) on the 16-state matrix-core form whatever
 * pm_min_items is; engine 0 keeps every level on lane groups.  All forms give identical
 * digests; this only moves time. */
int zkl_hip_set_hash_policy(int engine, uint32_t pm_min_items);
/* Process-wide row-digest rule for partitioned rows that form a single chunk (partition
 * size > row width: the 7-column composition rows from 2^14 trace rows up, any matrix
 * narrower than its partition size).  0 (default): winterfell 0.13.1
 * RowMatrix::commit_to_rows — merge_many over the chunk digests whenever partition_size !=
 * num_cols, even of one digest; 1: the reference's own re-implementation
 * hash_row_poseidon (agg/child.rs:1025-1045), which returns a single chunk digest as is.
 * Rows of several chunks and unpartitioned rows hash identically under both (DESIGN.md
 * §3.1).  zkl_hip_row_digest_rule() returns the rule in force. */
int zkl_hip_set_row_digest_rule(int rule);
int zkl_hip_row_digest_rule(void);
/* Process-wide NTT form for evaluation (DIT) passes: 1 (default) lazily reduced 26-bit limbs
 * inside a pass, 0 the canonical-form kernel, 2 the lazy form with its 8-stage passes on the
 * matrix cores (slower on gfx950).  Identical results; for parity tests /
 * A-B. */
int zkl_hip_set_ntt_mode(int mode);
/* Coset low-degree extension of column-major n_cols x n_rows evaluations over
 * GENERATOR * <w_{n*blowup}>; writes coefficients (n_cols x n_rows) and the LDE
 * (n_cols x n_rows*blowup), both column-major, natural order. */
int zkl_hip_lde(zkl_ctx* ctx, const void* d_values, uint32_t n_cols, uint32_t n_rows,
                uint32_t blowup, void* d_coeffs_out, void* d_lde_out);

/* ---- column structure (zero, constant and periodic trace columns) ----
 * A column's row period is 0 (every row zero), a power of two P (smallest period; 1 = constant,
 * non-zero) or ZKL_COL_GENERAL.  The prover scans each proof's trace (every row compared, periods
 * up to 128), skips the transforms of zero columns and resumes the row hash of partitions whose
 * leading absorb blocks hold only structured columns from a table of sponge states.  Proof bytes
 * do not depend on it. */
#define ZKL_COL_GENERAL 0xFFFFFFFFu
/* Process-wide switch, default 1 (ZKL_COLSTRUCT=0 in the environment starts it at 0); 0 treats
 * every column as general.  A proof reads it once when it starts. */
int zkl_hip_set_column_structure(int on);
int zkl_hip_column_structure(void);
/* The scan on a column-major device matrix (n_rows a power of two): period_out[n_cols]. */
int zkl_hip_scan_columns(zkl_ctx* ctx, const void* d_matrix, uint32_t n_cols, uint32_t n_rows, uint32_t* period_out);
/* Prefix plan of the partitioned row hash of an LDE of n_lde_rows rows (host code, no device):
 * per partition p < *n_parts_out, lead_out[p] = leading absorb blocks (10 sponge elements: the
 * domain element, then one per folded column pair) whose columns are all structured, and
 * q_out[p] = blowup * their largest period (1 when they are all zero or constant), the row period
 * of the sponge state after those blocks.  lead is 0 where q would exceed n_lde_rows / 64 and for
 * rows of more than 9 partitions.  period: per trace column, before the blowup.  lead_out and
 * q_out have 16 entries. */
int zkl_hip_plan_row_prefix(const uint32_t* period, uint32_t n_cols, uint64_t n_lde_rows, uint32_t blowup,
                            uint32_t num_partitions, uint32_t hash_rate, uint32_t* lead_out, uint32_t* q_out,
                            uint32_t* n_parts_out);
/* Zero mask of the same plan (host code, no device): in the blocks a partition still absorbs the
 * row kernel does not load columns the scan found zero.  Per partition p < *n_parts_out, bit j of
 * even_out[p] = column 2j of the partition is zero, bit j of odd_out[p] = column 2j + 1 is zero or
 * absent (the lone last column of an odd partition).  A partition of more than 64 pairs gets an
 * empty mask (both words 0) and loads everything; rows of more than 9 partitions have no plan
 * (*n_parts_out = 0).  even_out and odd_out have 16 entries. */
int zkl_hip_plan_row_zero_mask(const uint32_t* period, uint32_t n_cols, uint32_t num_partitions, uint32_t hash_rate,
                               uint64_t* even_out, uint64_t* odd_out, uint32_t* n_parts_out);
/* Process-wide switch of the zero mask alone, default 1 (ZKL_ROW_ZERO_MASK=0 in the environment
 * starts it at 0); 0 makes the prefix row kernel load every column.  For A/B runs; digests do not
 * depend on it. */
int zkl_hip_set_row_zero_mask(int on);
int zkl_hip_row_zero_mask(void);
/* zkl_hip_hash_rows with per-column row periods the caller asserts (in rows of d_matrix, natural
 * row order); split = 1: d_matrix is an LDE in the split layout (zkl_hip_lde_columns) and the
 * digests are written in natural row order.  The plan is zkl_hip_plan_row_prefix's with blowup 1,
 * except that any q <= n_rows is taken (the caller asked for it; the prover's n_rows / 64 only
 * bounds the table's cost).  *resumed_out (nullable): partitions that were resumed from the
 * table, 0 when the dense kernels ran (switch off, nothing to skip, lane-group engine, more than
 * 9 partitions). */
int zkl_hip_hash_rows_periodic(zkl_ctx* ctx, const void* d_matrix, uint32_t n_cols, uint32_t n_rows,
                               uint32_t num_partitions, uint32_t hash_rate, const uint32_t* row_period, int split,
                               void* d_digests_out, uint32_t* resumed_out);
/* The prover's trace LDE stage: period = NULL scans d_values, otherwise the caller's classes are
 * taken as given; this is the routine the prover runs.  Zero columns are cleared instead of
 * transformed, columns of a power-of-two period below n_rows get a small LDE tiled over the
 * column, the others go through the transforms in one launch group.  d_coeffs_out holds the
 * prover's working form (coefficient k times 3^k at index bitrev(k)); d_lde_out is in the split
 * layout when want_split is set and the shape supports it (*split_out says which).
 * The context remembers which slices of this (d_coeffs_out, d_lde_out) pair its last call left
 * zero and does not clear them again while the pair, n_cols, n_rows and blowup stay the same.  A
 * write into either buffer through this context's other entry points is noticed; a caller that
 * writes them by other means (its own kernels, another context) must use another pair for the
 * next call or run that call with the switch off. */
int zkl_hip_lde_columns(zkl_ctx* ctx, const void* d_values, uint32_t n_cols, uint32_t n_rows, uint32_t blowup,
                        const uint32_t* period, int want_split, void* d_coeffs_out, void* d_lde_out, int* split_out);

/* The same stage from host columns (columns[c]: n_rows elements, or NULL for an all-zero column):
 * the staging routine of zkl_hip_prove_segment_columns writing into caller device buffers.
 * period_out[n_cols] (nullable) receives the classes the host found.  The book of what the
 * context left zero in (d_coeffs_out, d_lde_out) is the one zkl_hip_lde_columns keeps, under the
 * rules stated there. */
int zkl_hip_lde_columns_host(zkl_ctx* ctx, const zkl_f128* const* columns, uint32_t n_cols, uint32_t n_rows,
                             uint32_t blowup, int want_split, void* d_coeffs_out, void* d_lde_out,
                             uint32_t* period_out, int* split_out);

/* The classes the staging threads give host columns (host code, no ctx, no device): the encoding
 * of zkl_hip_scan_columns, except that a period that is not below n_rows is ZKL_COL_GENERAL, as
 * the LDE plan treats it.  Every row is compared; a NULL column is period 0. */
int zkl_classify_columns(const zkl_f128* const* columns, uint32_t n_cols, uint32_t n_rows, uint32_t* period_out);

/* Raw in-place radix-2 NTT on n_cols contiguous device columns of length n (stage test
 * entry point).  dif != 0: natural order in, bit-reversed out (Gentleman-Sande);
 * dif == 0: bit-reversed in, natural out (Cooley-Tukey).  inverse selects w_n^-1; no 1/n
 * scaling.  out[k] = sum_j in[j] * w^(j*k) in the respective orders. */
int zkl_hip_ntt(zkl_ctx* ctx, void* d_data, uint32_t n_cols, uint32_t n, int dif, int inverse);

/* ---- verification (host, no device work) ------------------------------------
 * winter-verifier 0.13.1 for one segment proof (verify_proof, prove.rs:802-941): context and
 * options (must equal opts), commitments, transcript replay (agg/fs.rs:67-237), the
 * out-of-domain constraint identity (transition constraints of ZkLispAir + every assertion),
 * proof of work, query positions, trace / constraint / FRI Merkle openings, DEEP values, FRI
 * folds and remainder.  ZKL_OK when the proof verifies; ZKL_E_INVALID with
 * zkl_hip_last_error(NULL) naming the first failing check otherwise. */
int zkl_verify_segment(const uint8_t* proof, size_t len, const zkl_air_public_inputs* pi,
                       const zkl_proof_options* opts);

/* ---- workload generator (host, not the measured path) -------------------- */
/* Synthetic VM-only straight-line segment: 2^log_n rows, width 204
 * ({vm, rom} layout), ops cycling Const/Add/Mov/Mul over r0..r7 with splitmix64
 * immediates; trace built the way vm/trace/{mod,vm,rom}.rs build it.  Writes the
 * column-major trace (204 x 2^log_n) and the AIR public inputs. */
int zkl_synth_vm_segment(uint64_t seed, uint32_t log_n, zkl_f128* trace_out,
                         zkl_air_public_inputs* pi_out, uint32_t* width_out);
/* Same with program flags (flags = 0 is zkl_synth_vm_segment); the trace is built in the
 * segment layout the features imply ({vm, rom} 204, {vm, ram, rom} 212, {vm, merkle, rom} 211,
 * all 219, vm/layout.rs:183-313):
 *   ZKL_SYN_SPONGE  SAbsorbN / SSqueeze ops (vm/trace/vm.rs:565-672): FM_SPONGE | FM_POSEIDON,
 *                   PoseidonAir block (vm/air/poseidon.rs:26-162)
 *   ZKL_SYN_RAM     Load / Store over 8 addresses (vm.rs:803-842): FM_RAM, RamAir block
 *                   (vm/air/ram.rs:26-236) incl. the delta_clk range gadget
 *   ZKL_SYN_MERKLE  one MerkleStepFirst/Step/Last path (vm.rs:675-800): FM_MERKLE | FM_POSEIDON,
 *                   MerkleAir block (vm/air/merkle.rs:26-134); needs log_n >= 8 */
#define ZKL_SYN_SPONGE 1u
#define ZKL_SYN_RAM 2u
#define ZKL_SYN_MERKLE 4u
int zkl_synth_vm_segment_ex(uint64_t seed, uint32_t log_n, uint32_t flags, zkl_f128* trace_out,
                            zkl_air_public_inputs* pi_out, uint32_t* width_out);
/* Same with the program identity taken from program_seed (the ops still from seed) and ROM
 * lane 0 entering the first level at *rom0_in (NULL: 0), so that consecutive synthetic
 * segments are segments of one program and form the accumulator chain the aggregation checks
 * (agg/trace.rs:524-541: rom_s_in[0] of segment i+1 == rom_s_out[0] of segment i). */
int zkl_synth_vm_segment_chain(uint64_t program_seed, uint64_t seed, uint32_t log_n, uint32_t flags, const zkl_f128* rom0_in,
                               zkl_f128* trace_out, zkl_air_public_inputs* pi_out, uint32_t* width_out);

/* ---- op-list trace builder ------------------------------------------
 * zk_lisp_compiler::builder::Op (builder.rs:25-158), one op per 32-row level.  Field use:
 *   CONST dst imm | MOV dst a(=src) | ADD/SUB/MUL/EQ dst a b | NEG dst a | SELECT dst c a b
 *   ASSERT dst c | ASSERT_BIT, ASSERT_RANGE_LO, ASSERT_RANGE_HI dst c(=r)
 *   ASSERT_RANGE dst c(=r) bits | DIVMOD dst(=dst_q) dst2(=dst_r) a b
 *   DIVMOD128 a(=a_hi) c(=a_lo) b dst(=dst_q) dst2(=dst_r) | MULWIDE dst(=dst_lo) dst2(=dst_hi) a b
 *   LOAD dst a(=addr) | STORE a(=addr) b(=src) | SABSORBN n_regs regs[] | SSQUEEZE dst
 *   MERKLE_FIRST dst(=leaf_reg) a(=dir_reg) b(=sib_reg) | MERKLE_STEP, MERKLE_LAST a(=dir) b(=sib)
 *   END
 * Register indices < 8. */
enum {
  ZKL_OP_CONST = 0, ZKL_OP_MOV, ZKL_OP_ADD, ZKL_OP_SUB, ZKL_OP_MUL, ZKL_OP_NEG, ZKL_OP_EQ, ZKL_OP_SELECT,
  ZKL_OP_ASSERT, ZKL_OP_ASSERT_BIT, ZKL_OP_ASSERT_RANGE, ZKL_OP_ASSERT_RANGE_LO, ZKL_OP_ASSERT_RANGE_HI,
  ZKL_OP_DIVMOD, ZKL_OP_DIVMOD128, ZKL_OP_MULWIDE, ZKL_OP_LOAD, ZKL_OP_STORE, ZKL_OP_SABSORBN, ZKL_OP_SSQUEEZE,
  ZKL_OP_MERKLE_FIRST, ZKL_OP_MERKLE_STEP, ZKL_OP_MERKLE_LAST, ZKL_OP_END
};
typedef struct {
  uint32_t kind;
  uint8_t dst, dst2, a, b, c, bits, n_regs, reserved;
  uint8_t regs[10];
  uint64_t imm;
} zkl_op;
/* build_full_trace (vm/trace/mod.rs:434-524) of a program: n_rows = 32 * next_pow2(n_ops)
 * (levels past the last op keep only the schedule gates, pc and domain tags), initial registers
 * from secret_args (u64, r0..) and main_args flattened into slots in the tail registers
 * (vm.rs:64-104), the VM, RAM and ROM builders (vm.rs, ram.rs, rom.rs), written in the segment
 * layout of the features the ops use (sponge ops: FM_SPONGE | FM_POSEIDON, Load / Store:
 * FM_RAM, Merkle steps: FM_MERKLE | FM_POSEIDON; vm/layout.rs:183-313).  Also the AIR public
 * inputs prove_segment derives for the whole trace as one segment (prove.rs:292-423; merkle_root
 * = the accumulator after the last MerkleStepLast).  rom0_in: ROM lane 0 entering the first
 * level (NULL: 0).  trace_out NULL: only *width_out / *n_rows_out.  ZKL_E_INVALID on a register
 * index > 7, more than 10 pending absorbs (push_absorb, vm.rs:925-935), more than 8 main-arg
 * slots, or an unknown kind. */
int zkl_build_trace(const zkl_op* ops, uint32_t n_ops, const uint8_t program_id[32],
                    const uint8_t program_commitment[32], const uint64_t* secret_args, uint32_t n_secret,
                    const zkl_vm_arg* main_args, uint32_t n_main, const zkl_f128* rom0_in, zkl_f128* trace_out,
                    zkl_air_public_inputs* pi_out, uint32_t* width_out, uint32_t* n_rows_out);
/* rom_acc_from_program (romacc.rs:22-80): the t=3 ROM accumulator over the ops' virtual map rows
 * (opcode bit + register selectors, romacc.rs:82-260), next_pow2(n_ops) levels from state 0 —
 * what the verifier recomputes for pi.rom_acc when the commitment is non-zero (prove.rs:815-821,
 * lib.rs:210-214).  Equals the trace's rom_acc for a one-segment trace built from rom0 = 0. */
int zkl_rom_acc_from_program(const zkl_op* ops, uint32_t n_ops, const uint8_t program_id[32], zkl_f128 out[3]);

/* WinterfellSegmentPlanner::plan_segments (segment_planner.rs:93-276): the row ranges
 * [r_starts[i], r_ends[i]) of the segments of an n_ops program with at most max_rows rows per
 * segment (the reference's default is 1 << 12, ZKL_MAX_SEGMENT_ROWS).  r_starts / r_ends NULL:
 * only *count; otherwise cap >= *count entries are written. */
int zkl_plan_segments(uint32_t n_ops, uint32_t max_rows, uint32_t* r_starts, uint32_t* r_ends, uint32_t cap,
                      uint32_t* count);
/* prove_segment's inputs for rows [r_start, r_end) of a zkl_build_trace trace (prove.rs:1057-1134):
 * the segment feature mask from the ops of its levels (segment_planner.rs:283-334), the columns of
 * that layout (slice_trace_segment_with_layout), the AIR public inputs with the boundary values
 * (compute_segment_boundary_bytes, prove.rs:1197-1287) and the segment-local VM output / usage
 * mask (build_air_pi_for_trace), and the VM state hashes of its first and last rows
 * (utils::vm_state_hash_row_with_layout, for the zl1 step).  r_start, r_end multiples of 32,
 * r_end - r_start a power of two.  trace_out NULL: only *width_out. */
int zkl_slice_segment(const zkl_f128* full, uint32_t full_width, uint32_t n_full, const zkl_op* ops, uint32_t n_ops,
                      const zkl_air_public_inputs* pi_full, uint32_t r_start, uint32_t r_end, zkl_f128* trace_out,
                      zkl_air_public_inputs* pi_out, uint32_t* width_out, uint8_t state_in[32], uint8_t state_out[32]);

/* Per-segment trace builder: what prove_segment's input side (prove.rs:1057-1134,
 * build_segment_trace_with_state_without_full mod.rs:316-365 over build_full_trace mod.rs:434-524)
 * produces, without the full trace in memory.  zkl_program_new executes the program once (same
 * arguments as zkl_build_trace) and keeps the VM carry every 32 levels, the RAM event log with the
 * sorted table's running sums, ROM lane 0, rom_acc and the Merkle root; *full_width_out /
 * *n_rows_out receive the full trace's shape.  zkl_build_segment_trace then writes rows [r_start,
 * r_end) in the segment's layout with its AIR public inputs and VM state hashes -- bit for bit
 * what zkl_slice_segment(zkl_build_trace(..), .., r_start, r_end, ..) returns (same alignment
 * rules; trace_out NULL: only *width_out).  Calls on one program may run concurrently.
 * examples/fib-2pow16.zlisp (2^24 rows) is built this way segment by segment. */
typedef struct zkl_program zkl_program;
int zkl_program_new(const zkl_op* ops, uint32_t n_ops, const uint8_t program_id[32],
                    const uint8_t program_commitment[32], const uint64_t* secret_args, uint32_t n_secret,
                    const zkl_vm_arg* main_args, uint32_t n_main, const zkl_f128* rom0_in, zkl_program** out,
                    uint32_t* full_width_out, uint32_t* n_rows_out);
int zkl_build_segment_trace(const zkl_program* prog, uint32_t r_start, uint32_t r_end, zkl_f128* trace_out,
                            zkl_air_public_inputs* pi_out, uint32_t* width_out, uint8_t state_in[32],
                            uint8_t state_out[32]);
void zkl_program_free(zkl_program* prog);
/* The same public inputs, width and state hashes with no trace: what the caller of a device build
 * needs on the host.  Everything comes from the ops and zkl_program_new's pre-pass (which also
 * logs ROM lane 0 and the one or two register values each level writes, 48 B per level), so a
 * call runs one t=3 permutation (rom_s_out), no inversion, and reads or writes no trace cell.
 * Same window rules as zkl_build_segment_trace; pi_out NULL: only *width_out.  Calls on one
 * program may run concurrently. */
int zkl_segment_inputs(const zkl_program* prog, uint32_t r_start, uint32_t r_end, zkl_air_public_inputs* pi_out,
                       uint32_t* width_out, uint8_t state_in[32], uint8_t state_out[32]);
/* zkl_build_segment_trace on the device: replaces the input side of prove_segment
 * (prove.rs:1057-1134, build_segment_trace_with_state_without_full mod.rs:316-365) with a fill of
 * caller memory on ctx's device (e.g. from zkl_hip_device_alloc), so a segment costs an upload of
 * a few hundred bytes per level instead of width x rows x 16.  The host stages one record per
 * level (op fields, registers before and after, sponge selectors, Merkle accumulator, load value,
 * ROM lane 0), the slices of the sorted RAM table and its running sums the rows show, and the
 * program's constants, through a pinned buffer the context owns; the kernel recomputes the
 * Poseidon and ROM rounds, the inversions and the bit columns and writes every cell of the
 * column-major width x (r_end - r_start) trace: bit for bit zkl_build_segment_trace's, with the
 * same pi, width and state hashes.  The fill runs on ctx's stream, so a following
 * zkl_hip_prove_segment_device* or zkl_hip_check_trace_device on ctx is ordered after it; other
 * readers call zkl_hip_synchronize first.  cap_bytes < width x rows x 16: ZKL_E_INVALID, nothing
 * written.  d_trace_out NULL: only *width_out.  Nothing is kept per program: prog may be freed
 * after the call.  Calls on one program from several contexts may run concurrently. */
int zkl_hip_build_segment_trace_device(zkl_ctx* ctx, const zkl_program* prog, uint32_t r_start, uint32_t r_end,
                                       void* d_trace_out, size_t cap_bytes, zkl_air_public_inputs* pi_out,
                                       uint32_t* width_out, uint8_t state_in[32], uint8_t state_out[32]);
/* Device time (ms) of the last zkl_hip_build_segment_trace_device on ctx, upload and fill, by HIP
 * events on its stream; waits for the fill.  Recorded only for builds made with
 * zkl_hip_set_kernel_timing(ctx, 2) (ZKL_E_INVALID otherwise). */
int zkl_hip_build_device_ms(zkl_ctx* ctx, double* ms_out);

/* n segment proofs verified as zkl_verify_segment verifies each (same checks, same verdict, same
 * message), with the Poseidon hashing of the openings and the composition-coefficient draws on
 * ctx's device.  ctx NULL: the same batch on host threads.  status_out[i] = ZKL_OK or
 * ZKL_E_INVALID; errors_out (nullable) receives n NUL-terminated messages of
 * ZKL_VERIFY_MSG_LEN bytes each ("" for a proof that verifies).  The call itself returns ZKL_OK
 * when every proof got a verdict, a ZKL_E_* code when the batch could not be run.  opts[i] must
 * equal the options recorded in proof i.  The replay is split into a host plan (parsing,
 * transcript, every structural check) and flat hash jobs: only proofs that
 * passed the structural checks contribute jobs, so corrupt bytes change values, never addresses. */
#define ZKL_VERIFY_MSG_LEN 160
int zkl_hip_verify_segments(zkl_ctx* ctx, const uint8_t* const* proofs, const size_t* lens,
                            const zkl_air_public_inputs* pis, const zkl_proof_options* opts, uint32_t n,
                            int32_t* status_out, char* errors_out);

/* ---- zl1 step proof (host-side, no device work) ----------------------------------
 * StepProof::to_bytes (proof/step.rs:79-151) of the step proof prove_segment builds around
 * an inner proof from zkl_hip_prove_segment*: "ZKLSTP1" | lambda | suite | core pi |
 * main_args | vm_usage_mask | ram_delta_clk_bits | rom_acc | segment index/total | pc_init |
 * state hashes | boundary bytes | inner proof (length-prefixed).  Buffer released with
 * zkl_hip_free. */
int zkl_step_proof_encode(const zkl_air_public_inputs* pi, const zkl_step_info* info, const uint8_t* inner,
                          size_t inner_len, uint8_t** out, size_t* out_len);
/* Decode a ZKLSTP1 encoding (StepProof::from_bytes, step.rs:153-493) and return the zl1
 * commitment echo root_trace = BLAKE3("zkl/step/root_trace" | suite | trace roots |
 * constraint root | FRI roots) (format.rs:214-238) and the step digest
 * (proof/digest.rs:16-68).  Either output may be NULL.  Errors: ZKL_E_INVALID with
 * zkl_hip_last_error(NULL) naming the truncated/invalid field, as step.rs does. */
int zkl_step_proof_digest(const uint8_t* step, size_t len, uint8_t digest_out[32], uint8_t root_trace_out[32]);
/* agg::child::children_root_from_compact (agg/child.rs:853-895): the aggregation's root
 * over n children given as n x 32-byte step digests and n x 32-byte zl1 root_trace values
 * (what zkl_step_proof_digest returns), under the Poseidon suite of suite_id.  Rank 0 of
 * a multi-GPU run computes it after gathering the step proofs. */
int zkl_children_root(const uint8_t suite_id[32], const uint8_t* digests, const uint8_t* root_traces, uint32_t n,
                      uint8_t root_out[32]);

/* ---- aggregation proof -------------------------------------
 * zk_lisp_proof::ProverOptions as the aggregation reads it (zk-lisp-proof/src/lib.rs:40-66). */
typedef struct {
  uint32_t queries;           /* the aggregation proves with max(queries, 16) (prove.rs:645) */
  uint32_t blowup;
  uint32_t grind;
  uint32_t min_security_bits; /* >= 128: FieldExtension::Quadratic, else None (prove.rs:647-651);
                                 >= 64: conjectured-security check (prove.rs:664-681) */
  uint32_t trace_mode;        /* ZKL_AGG_TRACE_VALID (0) or ZKL_AGG_TRACE_REFERENCE (1), below */
} zkl_agg_options;

/* Aggregation trace modes.
 * ZKL_AGG_TRACE_VALID: next_pow2(max(children + 1, 8)) rows (one padding row always, so the
 *   last-row assertions of agg/air.rs:276-304 can hold) and zero root-error columns (every
 *   opening was verified against its root under the library's row-digest rule); the batch must
 *   satisfy ZlAggAir, otherwise ZKL_E_INVALID.  This is what zkl_agg_prove writes to proof.bin.
 * ZKL_AGG_TRACE_REFERENCE: the trace agg/trace.rs:397-398,553-690 builds -- PARITY UNPINNED:
 *   checked only against the Python restatement oracle/agg_ref.py (no fixture from the reference
 *   exists; its batch-proof decompression order and partition_size are [WF-recall] rules), so
 *   "the reference's trace" means "the restatement of agg/trace.rs", not bytes seen from it:
 *   next_pow2(max(children, 8)) rows and root-error columns sum_k(root_k - root) where root_k is
 *   reproduced from the opening's row under hash_row_poseidon (agg/child.rs:1025-1045, one chunk
 *   not merged).  No AIR check, like the reference's release prover: for a power-of-two child
 *   count >= 8, or children whose composition rows are one chunk (n >= 2^14), the proof does
 *   not verify, as the reference's would not. */
#define ZKL_AGG_TRACE_VALID 0u
#define ZKL_AGG_TRACE_REFERENCE 1u

/* What `zk-lisp prove` does after the segment proofs (replaces the Rust calls
 * RecursionPublicBuilder::build_public lib.rs:404-482, RecursionBackend::prove lib.rs:295-344
 * -> prove_agg_proof prove.rs:629-719, RecursionArtifactCodec::encode lib.rs:486-551):
 * n ZKLSTP1 step proofs in, the ZKLRC1 artifact (the aggregation proof inside) out, plus the
 * recursion digest (recursion_digest_from_agg_pi, prove.rs:585-616) when digest_out != NULL.
 * Each child's Fiat-Shamir transcript is replayed from its step proof alone (agg/fs.rs:38-245)
 * and every opening, DEEP value, FRI fold, remainder and PoW is checked; a child that fails
 * is rejected (ZKL_E_INVALID) rather than aggregated into an unsatisfiable trace.  The
 * artifact is freed with zkl_hip_free.  Host-only (no ctx, no device); zkl_hip_agg_prove below
 * hashes the child replays on a context's device. */
int zkl_agg_prove(const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps,
                  const zkl_agg_options* opts, uint8_t** artifact_out, size_t* artifact_len,
                  uint8_t digest_out[32]);
/* zkl_agg_prove on ctx's device: the child replay's hashing and the ZlAggAir proof itself (trace
 * LDE, commitments, constraint composition, DEEP and FRI in the proof's field, the quadratic
 * extension included), and the proof's grinding (the segment prover's ascending
 * nonce windows on ctx's stream: the smallest nonce, as the host search finds).  The transcript, the
 * AIR pre-check and the out-of-domain frame stay on the host, so a batch that violates ZlAggAir is
 * rejected before any launch of the prover.  Same arguments, same artifact bytes, same digest, same rejections.  ctx NULL is
 * zkl_agg_prove.  Rank 0 of a multi-GPU run holds a context after proving its own segments and
 * can pass it here. */
int zkl_hip_agg_prove(zkl_ctx* ctx, const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps,
                      const zkl_agg_options* opts, uint8_t** artifact_out, size_t* artifact_len,
                      uint8_t digest_out[32]);
/* ---- aggregation session: aggregate while the segments prove ----
 * zkl_agg_prove / zkl_hip_agg_prove in three steps, so that everything that depends on one child
 * alone runs when that child's step proof exists rather than after the last one.  For step proofs
 * st[0..n): begin(ctx, n, opts), add(p, st[p]) for every p in any order and from any number of
 * threads, then finish, give the artifact and the recursion digest that
 * zkl_hip_agg_prove(ctx, st, lens, n, opts, ..) gives, byte for byte, in both trace modes and both
 * field choices; the one-shot calls are this sequence over the same code.  ctx NULL: the host
 * executor and the host prover (zkl_agg_prove).
 *   begin   checks the options first (queries above 255, grind above 32, unknown trace mode, the
 *           conjectured-security check: ZKL_E_INVALID with the one-shot calls' texts) and refuses
 *           n_steps == 0.  The one-shot calls check the children before the options, so a batch
 *           that is wrong in both ways is refused with another text there.
 *   add     copies the bytes, decodes and replays the child (its hashing on the session's
 *           executor: ctx's device when a context was given), checks its two FRI layers and
 *           computes the unweighted terms of its aggregation trace row, all before it returns.
 *           Returns the child's own verdict: ZKL_OK, or ZKL_E_INVALID with the one-shot text
 *           ("child <position>: child step proof does not replay: ...").  A refused child counts
 *           as added and does not stop later adds.  A position >= n_steps or added before is
 *           ZKL_E_INVALID and changes nothing.
 *   finish  is called once, after every add has returned.  Fewer than n_steps positions added is
 *           ZKL_E_INVALID ("aggregation session: k of n step proofs added"); otherwise the message
 *           of the lowest refused position, then the cross-child checks in the one-shot order (the
 *           shared suite, the batch checks of the trace builder, the AIR pre-check in the valid
 *           mode), the trace and the ZlAggAir proof on ctx.  The artifact is freed with
 *           zkl_hip_free.  After finish, whether it succeeded or not, only free is valid.
 *   times   [0] summed host time of the adds, [1] their summed hashing time, [2] trace assembly in
 *           finish, [3] the proof without grinding, [4] grinding, [5] the whole of finish (ms).
 *           Returns the number written.
 *   free    releases the session, finished or not.
 * Locking: add takes the context's lock only around its device submission, finish around the
 * proof's launches.  A context that is also proving segments serialises with them, so a session
 * that runs beside the segment provers should be given a context of its own. */
typedef struct zkl_agg_session zkl_agg_session;
int zkl_hip_agg_begin(zkl_ctx* ctx, uint32_t n_steps, const zkl_agg_options* opts, zkl_agg_session** out);
int zkl_hip_agg_add(zkl_agg_session* s, uint32_t position, const uint8_t* step, size_t len);
int zkl_hip_agg_finish(zkl_agg_session* s, uint8_t** artifact_out, size_t* artifact_len, uint8_t digest_out[32]);
int zkl_hip_agg_session_times(const zkl_agg_session* s, double* out_ms, int max_n);
void zkl_hip_agg_free(zkl_agg_session* s);
/* Process-wide switch of the device ZlAggAir prover, default 1 (ZKL_AGG_DEVICE_PROVER=0 in the
 * environment starts it at 0).  0: zkl_hip_agg_prove keeps the host prover while the context's
 * device still hashes the child replays -- same bytes, for A/B runs.  The setter takes 0 or 1
 * (otherwise ZKL_E_INVALID).  zkl_hip_agg_prove_trace is not affected: its ctx argument chooses. */
int zkl_hip_set_agg_device_prover(int on);
int zkl_hip_agg_device_prover(void);
/* Stage entry point: the ZlAggAir proof (the inner proof bytes that end the ZKLRC1 artifact) of
 * a caller's trace, without any child.  trace: 31 columns x rows, column-major, host memory,
 * rows a power of two in [8, 2^14); pi_elements: AggAirPublicInputs::to_elements, absorbed into
 * the transcript seed; v_units_total / children_count: the values of the two last-row
 * assertions.  Of opts, queries (max(queries, 16), at most 255), blowup (a power of two in
 * [2, 128]) and grind (at most 32) are the proof options, min_security_bits >= 128 selects the
 * quadratic extension and is not otherwise enforced here, trace_mode is ignored.  check_air != 0
 * rejects a trace that violates ZlAggAir, on the host, before anything runs; 0 proves any trace
 * (as ZKL_AGG_TRACE_REFERENCE does): the DEEP polynomial has degree below rows whatever the
 * trace holds, so the proof is always produced, though a verifier rejects it when the trace
 * is invalid.  ctx NULL: the host backend; otherwise ctx's device, same bytes.  ZKL_E_INVALID
 * names the offending argument in zkl_hip_last_error(NULL).  The proof is freed with zkl_hip_free. */
int zkl_hip_agg_prove_trace(zkl_ctx* ctx, const zkl_f128* trace, uint32_t rows, const zkl_f128* pi_elements,
                            uint32_t n_pi, uint64_t v_units_total, uint32_t children_count,
                            const zkl_agg_options* opts, int check_air, uint8_t** proof_out, size_t* proof_len);
/* Wall times (ms) of the calling thread's last zkl_agg_prove / zkl_hip_agg_prove: [0] step decode +
 * child replay on the host (parse, transcript, DEEP / FRI arithmetic, plan), [1] hashing of the
 * replay (host executor or device incl. copies), [2] build_public + aggregation trace, [3] the
 * ZlAggAir proof without grinding, [4] its grinding, [5] the whole call.  Returns number written. */
int zkl_agg_last_times(double* out_ms, int max_n);
/* RecursionArtifactCodec::decode (lib.rs:552-660) + RecursionBackend::verify (lib.rs:346-372)
 * -> verify_agg_proof (prove.rs:732-791): decodes a ZKLRC1 artifact and verifies the
 * aggregation proof under ZlAggAir and the artifact's public inputs, accepting proof options
 * whose conjectured security (estimate_conjectured_security_bits, prove.rs:1177-1195) is at
 * least min_security_bits.  ZKL_OK, or ZKL_E_INVALID with zkl_hip_last_error(NULL) naming the
 * failing check.  Host-only. */
int zkl_agg_verify(const uint8_t* artifact, size_t len, uint32_t min_security_bits);
/* The aggregation trace of the same batch (build_agg_trace_from_transcripts,
 * agg/trace.rs:155-238): 31 columns x rows, column-major; rows_out receives the row count
 * (a power of two >= 8); out may be NULL to query it.  zkl_agg_trace builds the
 * ZKL_AGG_TRACE_VALID trace; zkl_agg_trace_mode takes the mode. */
int zkl_agg_trace(const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps,
                  zkl_f128* out, uint32_t max_rows, uint32_t* rows_out);
int zkl_agg_trace_mode(const uint8_t* const* steps, const size_t* step_lens, uint32_t n_steps,
                       uint32_t trace_mode, zkl_f128* out, uint32_t max_rows, uint32_t* rows_out);

/* ---- multi-GPU boundary exchange --------------------------
 * One process per GPU proves its own segments; the step proofs (zl1 ZKLSTP1 bytes with the
 * boundary fields the aggregation chains: state hashes, RAM grand products, ROM lanes) are
 * gathered on the aggregating rank with RCCL point-to-point transfers over xGMI.  Replaces the
 * reference's in-process Vec<StepProof> hand-off (prove.rs:1018-1050 -> lib.rs:382-482).
 * RCCL is opened at run time; without it these calls fail with ZKL_E_INVALID and
 * zkl_hip_last_error(NULL) says why (the single-GPU path does not need it). */
typedef struct zkl_comm zkl_comm;
/* ZKL_OK when RCCL can be opened here (checked by every rank before the collective init, so
 * that no rank enters ncclCommInitRank alone). */
int zkl_comm_available(void);
/* ncclGetUniqueId on the root rank; the 128 bytes go to the other ranks out of band
 * (bench.py / zkl_hip.dist use the torch.distributed store). */
int zkl_comm_unique_id(uint8_t id_out[128]);
/* ncclCommInitRank on `device` (collective over the world). */
int zkl_comm_init(int device, int world, int rank, const uint8_t id[128], zkl_comm** out);
/* Collective: every rank contributes `len` host bytes; on `root`, *out (free with
 * zkl_hip_free) receives the world blobs concatenated in rank order and lens_out[world] their
 * lengths (other ranks may pass NULL).  Lengths are all-gathered first, then each rank's blob
 * is sent to the root (grouped ncclSend / ncclRecv on the comm's stream). */
int zkl_comm_gather_bytes(zkl_comm* comm, const uint8_t* data, size_t len, int root, uint8_t** out,
                          size_t* lens_out);
/* Device time (ms, HIP events on the comm stream) of the last gather: length exchange + sends. */
double zkl_comm_last_ms(const zkl_comm* comm);
void zkl_comm_destroy(zkl_comm* comm);

#ifdef __cplusplus
}
#endif
#endif
