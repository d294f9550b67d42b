// single_stage.h -- what single_fold.hip and the entry points of real_hip_api.hip share of the single placements of a mate:
// the stage's state (real_hip_ctx::single) and its launcher.
#pragma once
#include "host_buf.h"

// the staged records of the two lists when the caller's are host memory, the hand-over list of the wave kernel
struct RhSingleStage {
    DevBuf rec[2], list;
    RhStage stage;
};

int rh_launch_single(real_hip_ctx *ctx, int lists, const MateLists &L, uint64_t n, uint32_t fileid, int fresh, real_hip_single *const d_out[2]);
int rh_single_stats(real_hip_ctx *ctx, real_hip_single_stats *out, int reset);
