// mismatch_stage.h -- what mismatch_list.hip and the entry points of real_hip_api.hip share of the mismatch lists: the
// stage's state (real_hip_ctx::mismatch) and its steps.
#pragma once
#include "host_buf.h"

// the counts per list, and when the caller's arrays are host memory the staged records (info or pairs, the two mates'
// singles), the offsets and the lists
struct RhMismatchStage {
    DevBuf cnt, off, out, rec, sg[2];
    RhStage stage;
};

// one launch: the reads and the records that place them, all arrays on the device: info (single-end), or pairs and -- nullable --
// this mate's singles
struct RhMismatchLaunch {
    DevBatch b;
    const uint64_t *info;
    const real_hip_pair *pairs;
    const real_hip_single *singles;
};
// l[0] (single-end: n lists) or l[0], l[1] = mate 1, mate 2 (pairs: 2n lists, mate m of fragment i is list 2i + m).  count +
// scan into d_off (lists + 1, device) + the total read back (synchronises); then, if it fits, the records (asynchronous)
int rh_mismatch_count(real_hip_ctx *ctx, const RhMismatchLaunch l[], int n_launch, uint64_t *d_off, uint64_t *total);
int rh_mismatch_emit(real_hip_ctx *ctx, const RhMismatchLaunch l[], int n_launch, const uint64_t *d_off, real_hip_mismatch *d_out, uint64_t total);
int rh_mismatch_stats(real_hip_ctx *ctx, real_hip_mismatch_stats *out, int reset);
