// gap_stage.h -- what gap_rescue.hip and the entry points of real_hip_api.hip share of the gap rescue (include/real_hip.h, "gap
// rescue"): the stage's state and its launcher.
// The state is a member of the ctx, real_hip_ctx::gap (real_hip_ctx.h).
#pragma once
#include "host_buf.h"

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
    // anchored gap placement (gap_anchor.hip): the list of the reads to search, the sub-reads of the composite (bases and
    // qualities as a byte batch), its hit lists and their offsets, and when the caller's arrays are host memory the staged
    // info words and gap records; a stage record of its own with the kernels' error flags behind its statistics
    DevBuf an_list, an_bases, an_qual, an_hits, an_off, an_info, an_out;
    RhStage anchor;
    uint32_t an_err = 0;
};

// select + search over n fragments, all arrays on the device; asynchronous on the ctx's stream.  After the stream was
// synchronised rh_gap_finish reports what the kernels flagged
int rh_launch_gap_rescue(real_hip_ctx *ctx, const real_hip_pair_params &pp, const real_hip_gap_params &gp, const DevBatch &b1, const DevBatch &b2,
                         const real_hip_pair *d_pairs, const real_hip_single *const d_singles[2], uint64_t n, int fresh, real_hip_gap_place *d_out);
int rh_gap_finish(real_hip_ctx *ctx);
int rh_gap_stats(real_hip_ctx *ctx, real_hip_gap_stats *out, int reset);

// ---- anchored gap placement (gap_anchor.hip; include/real_hip.h, "anchored gap placement"), all arrays on the device
struct RhAnchorRun {
    real_hip_gap_params gp;
    real_hip_gap_anchor_params ap;
    DevBatch b;
    const uint64_t *d_info; // nullable: every read is eligible
    uint64_t n;
    int fresh;
    real_hip_gap_place *d_out;
};
// select: the eligible, not skipped reads into the stage's list (and, fresh, the NoMatch records of the others).  count
// (nullable): the number listed, read back -- that synchronises the stream
int rh_gap_anchor_select(real_hip_ctx *ctx, const RhAnchorRun &r, uint64_t *count);
// the sub-reads of the `count` listed reads into the stage's byte batch: 2 * count reads of anchor_len bases, slot w's prefix
// and suffix at 2w and 2w + 1; *d_bases, *d_qual (null when the batch has no qualities): where they lie
int rh_gap_anchor_extract(real_hip_ctx *ctx, const RhAnchorRun &r, uint64_t count, const uint8_t **d_bases, const uint8_t **d_qual);
// search: the listed reads against the anchors of hit lists d_hits / d_off (`total` hits).  compact: the lists are those of the
// extracted sub-reads (2 per list slot), else of S(b, A) (2 per read of the batch).  Asynchronous; after the stream was
// synchronised rh_gap_anchor_finish reports what the kernels flagged
int rh_gap_anchor_search(real_hip_ctx *ctx, const RhAnchorRun &r, const real_hip_hit *d_hits, const uint64_t *d_off, uint64_t total, bool compact);
int rh_gap_anchor_finish(real_hip_ctx *ctx);
int rh_gap_anchor_stats(real_hip_ctx *ctx, real_hip_gap_anchor_stats *out, int reset);

// ---- gapped mismatch lists (gapped_list.hip): list i belongs to fragment i's gap record, all arrays on the device.  count +
// scan into d_off (n + 1, device) + the total read back (synchronises); then, if it fits, the records (asynchronous)
int rh_gapped_list_count(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n, uint64_t *d_off,
                         uint64_t *total);
int rh_gapped_list_emit(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n, const uint64_t *d_off,
                        real_hip_mismatch *d_out, uint64_t total);
int rh_gapped_list_stats(real_hip_ctx *ctx, real_hip_gapped_list_stats *out, int reset);
