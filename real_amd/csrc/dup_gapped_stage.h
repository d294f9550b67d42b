// dup_gapped_stage.h -- what duplicates.hip and the entry point of real_hip_api.hip share of the joint duplicate marking over
// info words and gap records (include/real_hip.h, "duplicates", SINGLE-END WITH GAPPED PLACEMENTS): the stage's
// state and its launcher.
// The state is a member of the ctx, real_hip_ctx::dup_gapped (real_hip_ctx.h).  The keys, the sort's buffers and the statistics
// are the marking's own (real_hip_ctx::dup, dup_stage.h): only what the joint marking adds to them is here.
#pragma once
#include "host_buf.h"

struct RhDupGappedStage {
    DevBuf rec; // when the caller's gap records are host memory, their staged copy
};

// dup[i] of n reads, all arrays on the device: info words, gap records (16-byte aligned) and summaries; asynchronous
int rh_launch_mark_duplicates_gapped(real_hip_ctx *ctx, const uint64_t *d_info, const real_hip_gap_place *d_gaps, const real_hip_read_sum *d_sum,
                                     uint64_t n, uint8_t *d_dup);
