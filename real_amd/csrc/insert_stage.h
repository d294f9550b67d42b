// insert_stage.h -- what insert_hist.hip and the entry points of real_hip_api.hip share of the insert-size histogram: the
// stage's state (real_hip_ctx::insert) and its launcher.
#pragma once
#include "host_buf.h"

// the staged records, lengths and histogram when the caller's are host memory
struct RhInsertStage {
    DevBuf rec, len[2], hist;
    RhStage stage;
};

// d_hist += the histogram of n records, all arrays on the device; asynchronous on the ctx's stream
int rh_launch_insert_hist(real_hip_ctx *ctx, const real_hip_pair *d_pairs, const uint32_t *d_len1, const uint32_t *d_len2, uint64_t n,
                          uint32_t n_bins, uint64_t *d_hist);
int rh_insert_stats(real_hip_ctx *ctx, real_hip_insert_stats *out, int reset);
