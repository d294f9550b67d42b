// pileup_stage.h -- what pileup.hip, the stages on top of the pileup (snp_call.hip, pileup_gapped.hip, indel_call.hip) and the
// entry points of real_hip_api.hip share of the pileup: the stage's state (real_hip_ctx::pileup) and its steps.
#pragma once
#include "host_buf.h"

// the depth's difference array (n + 1 u32, scanned in place by finish), the alt table (4 u32 per position), the per-block
// site counts and their scan, the site list, covered / max_depth of finish (striped), the staged records when the caller's
// are host memory
struct RhPileupStage {
    DevBuf diff, alt, blk, sites, fin, rec;
    RhStage stage;
    int      state = 0;   // 0 none, 1 begun (adds), 2 finished (depth / sites)
    uint64_t n = 0, n_sites = 0, covered = 0, max_depth = 0; // the text begin saw; the last finish
    uint32_t fileid = 0, min_qual = 0;
};

int rh_pileup_begin(real_hip_ctx *ctx, uint32_t min_qual);
// the placements of a batch (d_info) or of mate `mate` of a batch of pairs (d_pairs), all arrays on the device; asynchronous
int rh_launch_pileup_add(real_hip_ctx *ctx, const DevBatch &b, const uint64_t *d_info, const real_hip_pair *d_pairs, uint32_t mate);
int rh_pileup_finish(real_hip_ctx *ctx, uint64_t *n_sites); // synchronises
void rh_pileup_end(real_hip_ctx *ctx);
int rh_pileup_stats(real_hip_ctx *ctx, real_hip_pileup_stats *out, int reset);
