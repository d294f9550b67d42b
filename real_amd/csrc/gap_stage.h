// gap_stage.h -- what gap_rescue.hip and the entry points of real_hip_api.hip share of the gap rescue (include/real_hip.h, "gap
// rescue"): the stage's state and its launcher.
// The state lives BESIDE the ctx, in a table keyed by it, as the mapping quality's does and for its reason (mapq_stage.h):
// real_hip_internal.h is among the sources bench.py hashes.  rh_gap_stage creates the entry on first use; real_hip_destroy
// releases it (rh_gap_release).
#pragma once
#include "real_hip_internal.h"

// the list of the fragments to search, and when the caller's arrays are host memory the staged pair records, singles and gap
// records; the stage record with the kernels' error flags behind its statistics
struct RhGapStage {
    DevBuf list, rec, sg[2], out;
    RhStage stage;
    uint32_t err = 0; // the flags of the last launch, copied back behind it
    // gapped mismatch lists (gapped_list.hip): the counts per list and the scan's room, and when the caller's arrays are host
    // memory the staged gap records, offsets and lists; a stage record of its own
    DevBuf gl_cnt, gl_tmp, gl_rec, gl_off, gl_out;
    RhStage lists;
};
RhGapStage &rh_gap_stage(real_hip_ctx *ctx);
void rh_gap_release(real_hip_ctx *ctx);

// select + search over n fragments, all arrays on the device; asynchronous on the ctx's stream.  After the stream was
// synchronised rh_gap_finish reports what the kernels flagged
int rh_launch_gap_rescue(real_hip_ctx *ctx, const real_hip_pair_params &pp, const real_hip_gap_params &gp, const DevBatch &b1, const DevBatch &b2,
                         const real_hip_pair *d_pairs, const real_hip_single *const d_singles[2], uint64_t n, int fresh, real_hip_gap_place *d_out);
int rh_gap_finish(real_hip_ctx *ctx);
int rh_gap_stats(real_hip_ctx *ctx, real_hip_gap_stats *out, int reset);

// ---- gapped mismatch lists (gapped_list.hip): list i belongs to fragment i's gap record, all arrays on the device.  count +
// scan into d_off (n + 1, device) + the total read back (synchronises); then, if it fits, the records (asynchronous)
int rh_gapped_list_count(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n, uint64_t *d_off,
                         uint64_t *total);
int rh_gapped_list_emit(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n, const uint64_t *d_off,
                        real_hip_mismatch *d_out, uint64_t total);
int rh_gapped_list_stats(real_hip_ctx *ctx, real_hip_gapped_list_stats *out, int reset);
