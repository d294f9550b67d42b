// pileup_gapped_stage.h -- what pileup_gapped.hip, pileup.hip, indel_call.hip and the entry points of real_hip_api.hip share of
// the gapped placements in the pileup and the calls (include/real_hip.h, "gapped placements in the pileup and the calls"): the
// stage's state and its steps.
// The state is a member of the ctx, real_hip_ctx::pileup_gapped (real_hip_ctx.h).
// rh_pileup_gapped_release ends the stage and keeps the record (the pileup's begin and end call it).
#pragma once
#include "host_buf.h"

struct RhPileupGappedStage {
    // the second difference array (n + 1 u32; scanned in place into gdepth[] by the pileup's finish), there from the first
    // add_gapped of a pileup on; when the caller's gap records are host memory, their staged copy
    DevBuf gdiff, rec;
    bool have_gdiff = false;
    RhStage add, call; // the pileup leg's statistics and the call leg's
};
void rh_pileup_gapped_release(real_hip_ctx *ctx); // ends the stage: gdiff and the staged records go, the statistics stay

// the placements of n fragments into the begun pileup (all arrays on the device; asynchronous on the ctx's stream); the first
// one of a pileup allocates and zeroes gdiff: REAL_HIP_E_NOMEM with a message when that fails, the pileup stays valid
int rh_pileup_gapped_add(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n);
// the evidence of the same placements over the finished pileup's sites (snp_call.hip's bitmap, rank array and evidence)
int rh_call_gapped_add(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n);
// gdiff of the begun pileup (its finish scans it in place, as it scans the depth's) = gdepth[] of the finished one; null when
// no gapped add was made
uint32_t *rh_pileup_gapped_array(real_hip_ctx *ctx);
int rh_pileup_gapped_stats(real_hip_ctx *ctx, real_hip_pileup_gapped_stats *out, int reset);
