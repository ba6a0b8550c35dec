// Context access for the device ZlAggAir prover (agg.hip); prover.cpp owns zkl_ctx.
// Device / pinned buffers of the aggregation prover live in the context, are reused across
// calls and, the pinned ones, counted by zkl_hip_pinned_bytes.
#pragma once
#include <stddef.h>

#include "../../include/zkl_hip.h"

namespace zkl {

enum AggDBufSlot {
  AGG_D_TRACE, AGG_D_TCOEF, AGG_D_LDE, AGG_D_TTREE, AGG_D_CEV, AGG_D_CCOEF, AGG_D_CLDE, AGG_D_CTREE, AGG_D_FRI,
  AGG_D_FTREE, AGG_D_ROOTS, AGG_D_CONST, AGG_D_BEST, AGG_D_SLOTS
};
enum AggHBufSlot { AGG_H_UP, AGG_H_DOWN, AGG_H_SLOTS };
struct AggCtxView {
  int device;
  void* stream;  // hipStream_t
};
void agg_ctx_lock(zkl_ctx* ctx);  // ctx->mu
void agg_ctx_unlock(zkl_ctx* ctx);
// the calls below: the caller holds the lock
AggCtxView agg_ctx_begin(zkl_ctx* ctx);  // hipSetDevice + the hasher constants on the device
void* agg_ctx_dbuf(zkl_ctx* ctx, int slot, size_t bytes);  // grown to at least bytes, contents undefined
void* agg_ctx_hbuf(zkl_ctx* ctx, int slot, size_t bytes);

}  // namespace zkl
