// dup_stage.h -- what duplicates.hip and the entry points of real_hip_api.hip share of the duplicate marking: the stage's
// state (real_hip_ctx::dup) and its launchers.  The joint marking over info words and gap records adds dup_gapped_stage.h.
#pragma once
#include "host_buf.h"

// the two buffers of the sort's keys and values, the paired key's two words in record order, and when the caller's arrays are
// host memory the staged records, summaries and marks
struct RhDupStage {
    DevBuf key[2], val[2], lo, hi, rec, sum[2], out;
    RhStage stage;
};

// {len, qsum} of every read of b (qual, off, upatl, n_reads; the bases are not read), all arrays on the device; asynchronous
int rh_launch_read_summary(real_hip_ctx *ctx, const DevBatch &b, uint32_t min_qual, real_hip_read_sum *d_out);
// dup[] of n records, all arrays on the device: d_info and d_sum1 (single-end) or d_pairs, d_sum1 and d_sum2; asynchronous
int rh_launch_mark_duplicates(real_hip_ctx *ctx, const uint64_t *d_info, const real_hip_pair *d_pairs, const real_hip_read_sum *d_sum1,
                              const real_hip_read_sum *d_sum2, uint64_t n, uint8_t *d_dup);
int rh_dup_stats(real_hip_ctx *ctx, real_hip_dup_stats *out, int reset);
