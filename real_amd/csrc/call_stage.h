// call_stage.h -- what snp_call.hip, pileup_gapped.hip and the entry points of real_hip_api.hip share of the variant calls on
// top of the finished pileup: the stage's state (real_hip_ctx::call) and its steps.
#pragma once
#include "host_buf.h"

// the site bitmap (a bit per text position) and its rank array (sites before each 64-bit word), the evidence table (32 bytes
// per site), the per-block call counts and their scan, the call list, het / hom of finish (striped), the staged records when
// the caller's are host memory
struct RhCallStage {
    DevBuf bits, rank, ev, blk, calls, fin, rec;
    RhStage stage;
    int      state = 0;   // 0 none, 1 begun (adds), 2 finished (evidence / variants; finish again)
    uint64_t n_calls = 0, het = 0, hom = 0; // the last finish
};

int rh_call_begin(real_hip_ctx *ctx); // bitmap, rank array and zeroed evidence from the pileup's site list; synchronises
// the evidence of a batch (d_info) or of mate `mate` of a batch of pairs (d_pairs), all arrays on the device; asynchronous
int rh_launch_call_add(real_hip_ctx *ctx, const DevBatch &b, const uint64_t *d_info, const real_hip_pair *d_pairs, uint32_t mate);
int rh_call_finish(real_hip_ctx *ctx, uint32_t min_call_qual, uint32_t min_depth, uint64_t *n_calls); // synchronises
void rh_call_release(real_hip_ctx *ctx); // (no synchronisation: the caller's)
int rh_call_stats(real_hip_ctx *ctx, real_hip_call_stats *out, int reset);
