// mapq_stage.h -- what mapq.hip and the entry points of real_hip_api.hip share of the mapping quality stage (include/real_hip.h,
// "mapping quality"): the stage's state and its launchers.
// The state is a member of the ctx, real_hip_ctx::mapq (real_hip_ctx.h).
#pragma once
#include "host_buf.h"

struct MateLists; // pair_state.h

// the hand-over lists of the two folds' wave kernels, and when the caller's arrays are host memory the staged accumulators
// (single-end / the pair's, mate 1's, mate 2's), records, scores, singles and qualities; the stage record
struct RhMapqStage {
    DevBuf list, pair_list, acc[3], rec, score, sg[2], out;
    RhStage stage;
};

// the folds of `lists` (1 or 2) hit lists / of the concordant pairs into the in/out accumulators, and the finish (d_pairs null:
// single-end, d_acc[0] alone; else d_acc = the pair's, mate 1's, mate 2's and d_singles nullable); all arrays on the device;
// asynchronous on the ctx's stream
int rh_launch_mapq_fold(real_hip_ctx *ctx, int lists, const MateLists &L, uint64_t n, int fresh, real_hip_mapq_acc *const d_acc[2]);
int rh_launch_mapq_pair_fold(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, int fresh, real_hip_mapq_acc *d_acc);
int rh_launch_mapq_finish(real_hip_ctx *ctx, const uint64_t *d_info, const float *d_score, const real_hip_pair *d_pairs,
                          const real_hip_single *const d_singles[2], const real_hip_mapq_acc *const d_acc[3], uint64_t n, uint8_t *d_out);
int rh_mapq_stats(real_hip_ctx *ctx, real_hip_mapq_stats *out, int reset);
