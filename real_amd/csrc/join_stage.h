// join_stage.h -- what pair_kernel.hip and the entry points of real_hip_api.hip share of the paired-end join: the stage's
// state (real_hip_ctx::join) and its launchers.
#pragma once
#include "host_buf.h"

// the two mates' hit lists, offsets and read lengths, staged records, the hand-over list of the wave kernel; its two kernels
// are timed under their public ids, stage.launches / kernel_ms stay 0
struct RhJoinStage {
    DevBuf hits[2], off[2], len[2], rec, list;
    uint64_t cap = 0;   // hits each of hits[] holds (grown when a match overflowed it)
    RhStage stage;
};

int rh_pair_lens(real_hip_ctx *ctx, const uint64_t *d_off, uint32_t upatl, uint64_t n, uint32_t *d_len);
int rh_launch_pair(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint32_t fileid, int fresh, real_hip_pair *d_pairs);
int rh_pair_stats(real_hip_ctx *ctx, real_hip_pair_stats *out, int reset);
