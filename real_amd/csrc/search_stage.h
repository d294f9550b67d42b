// search_stage.h -- what mate_search.hip and the entry points of real_hip_api.hip share of the mate search: the stage's state
// (real_hip_ctx::search) and its launchers.
#pragma once
#include "host_buf.h"

// the kernel's error flags lie behind its statistics
struct RhSearchStage {
    RhStage stage;
    uint32_t err = 0;     // the flags of the last launch, copied back behind it
};

// asynchronous on the ctx's stream; after the stream was synchronised rh_mate_search_finish reports what the kernel flagged
int rh_launch_mate_search(real_hip_ctx *ctx, const real_hip_pair_params &pp, const real_hip_mate_search_params &sp, const DevBatch &b1,
                          const DevBatch &b2, const MateLists &L, uint64_t n, uint32_t fileid, int fresh, real_hip_pair *d_pairs);
int rh_mate_search_finish(real_hip_ctx *ctx);
int rh_mate_search_stats(real_hip_ctx *ctx, real_hip_mate_search_stats *out, int reset);
