// ctx_side.h -- the state of the stages behind the matcher that lives BESIDE the ctx: mapping quality (mapq_stage.h), the gap
// stages (gap_stage.h), the indel calls (indel_stage.h), the gapped placements in the pileup and the calls
// (pileup_gapped_stage.h) and the joint duplicate marking (dup_gapped_stage.h), as ONE record in one table keyed by the ctx (side_table.h).
// Why beside and not in real_hip_ctx: real_hip_internal.h is among the sources bench.py hashes to tie profiles/traffic.json to
// the matcher it was measured on, and a stage that does not touch the matcher stays out of them.
// Two words, one meaning each: DROP -- the entry goes, with everything in it (real_hip_destroy: rh_side_drop, its only
// caller); RELEASE -- a stage's device memory goes, its statistics stay (rh_indel_release, rh_pileup_gapped_release).
#pragma once
#include "mapq_stage.h"
#include "gap_stage.h"
#include "indel_stage.h"
#include "pileup_gapped_stage.h"
#include "dup_gapped_stage.h"

struct RhCtxSide {
    RhMapqStage mapq;
    RhGapStage gap;
    RhIndelStage indel;
    RhPileupGappedStage pileup_gapped;
    RhDupGappedStage dup_gapped;
};
RhCtxSide &rh_side(real_hip_ctx *ctx);    // made on first use
RhCtxSide *rh_side_if(real_hip_ctx *ctx); // null: no stage has made it (nothing to release)
void rh_side_drop(real_hip_ctx *ctx);     // (its DevBufs go with it)

static inline RhMapqStage &rh_mapq_stage(real_hip_ctx *ctx) { return rh_side(ctx).mapq; }
static inline RhGapStage &rh_gap_stage(real_hip_ctx *ctx) { return rh_side(ctx).gap; }
static inline RhIndelStage &rh_indel_stage(real_hip_ctx *ctx) { return rh_side(ctx).indel; }
static inline RhPileupGappedStage &rh_pileup_gapped_stage(real_hip_ctx *ctx) { return rh_side(ctx).pileup_gapped; }
static inline RhDupGappedStage &rh_dup_gapped_stage(real_hip_ctx *ctx) { return rh_side(ctx).dup_gapped; }
