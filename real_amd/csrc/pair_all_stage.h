// pair_all_stage.h -- what pair_all.hip and the entry points of real_hip_api.hip share of the enumeration of every concordant
// pair of a fragment: the stage's state (real_hip_ctx::pair_all) and its steps.
#pragma once
#include "host_buf.h"

// counts per fragment, their scan and the staged records when the caller's outputs are host memory
struct RhPairAllStage {
    DevBuf cnt, off, out;
    RhStage stage;
    uint64_t pairs_out = 0;
};

// count + scan into d_off (n + 1, device) + the total read back (synchronises); then, if it fits, the records (asynchronous)
int rh_pair_all_count(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint64_t *d_off, uint64_t *total);
int rh_pair_all_emit(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint32_t fileid, const uint64_t *d_off,
                     real_hip_pair_hit *d_out, uint64_t cap, uint64_t total);
int rh_pair_all_stats(real_hip_ctx *ctx, real_hip_pair_all_stats *out, int reset);
