// indel_stage.h -- what indel_call.hip and the entry points of real_hip_api.hip share of the indel calls (include/real_hip.h,
// "indel calls"): the stage's state and its steps.
// The state is a member of the ctx, real_hip_ctx::indel (real_hip_ctx.h).  rh_indel_release ends the stage and keeps the
// record (the pileup's end calls it).
#pragma once
#include "host_buf.h"

struct RhIndelStage {
    // the event list (16 bytes an event, key and payload; sorted in place by the first finish) with its counter in front of the
    // statistics' stripes, the sort's key buffers and second event buffer, the heads' block counts and their scan, the groups'
    // first events, the grouped table, the event list and the call list as the caller reads them, the counts of finish (striped)
    DevBuf ev, ev2, key[2], blk, starts, table, events, calls, fin, count;
    // when the caller's gap records are host memory, their staged copy
    DevBuf rec;
    RhStage stage;
    int      state = 0;        // 0 none, 1 begun (adds), 2 finished (events / calls; finish again)
    bool     grouped = false;  // the first finish has sorted and grouped the events
    uint64_t n_ev = 0;         // events appended so far (read back behind every add)
    uint64_t n_groups = 0, n_calls = 0, het = 0, hom = 0, dels = 0, ins = 0; // the last finish
};
void rh_indel_release(real_hip_ctx *ctx); // ends the stage: its device memory goes, its statistics stay

int rh_indel_begin(real_hip_ctx *ctx);
// the events of n fragments, all arrays on the device; synchronises (the number of events is read back)
int rh_indel_add(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n);
int rh_indel_finish(real_hip_ctx *ctx, const real_hip_indel_params &p, uint64_t *n_events, uint64_t *n_calls);
int rh_indel_stats(real_hip_ctx *ctx, real_hip_indel_stats *out, int reset);
