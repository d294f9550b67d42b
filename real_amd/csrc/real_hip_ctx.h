// real_hip_ctx.h -- the host context of libreal_hip.so: the matcher's own state as direct members, one record per stage behind
// the matcher (<stage>_stage.h: the record and the stage's host entry points), the timing scopes, the matcher's launchers.
// Host translation units and the launch code at the bottom of the kernel files include this; the headers that only kernels
// read include real_hip_internal.h (the device views) alone.
#pragma once

#include <string>
#include <vector>

#include "host_buf.h"
#include "join_stage.h"
#include "search_stage.h"
#include "pair_all_stage.h"
#include "single_stage.h"
#include "insert_stage.h"
#include "pileup_stage.h"
#include "call_stage.h"
#include "mismatch_stage.h"
#include "dup_stage.h"
#include "mapq_stage.h"
#include "gap_stage.h"
#include "indel_stage.h"
#include "pileup_gapped_stage.h"
#include "dup_gapped_stage.h"

struct real_hip_ctx {
    real_hip_params prm;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;

    // text
    DevBuf text, wild, frag;
    uint64_t n_bases = 0;
    uint64_t n_wild = 0;
    uint32_t n_frag = 0, fileid = 0;
    bool have_text = false;

    // index
    DevBuf ent[6], bkt[6];
    uint64_t n_entries = 0;
    uint32_t pb = 0;
    RhLayout layout = RH_LAYOUT_STARTS;
    bool no_rows = false; // bucket rows did not fit the device memory once: stay with directory tables
    bool have_index = false;

    // tables / counters
    DevBuf LL, counters;

    // batch staging (host batches), hand-over list of the repeat kernel
    BatchBufs stage[2];
    DevBuf s_info, s_score;
    RhSlot slot[REAL_HIP_SLOTS];                    // submit / wait
    hipStream_t copy_stream = nullptr, down_stream = nullptr;
    DevBuf maxpatl, ovf_list, ovf2_list, ovf_count, qspill;
    unsigned long long *h_state = nullptr; // pinned: {reads handed over, error flags} of the last launch of slot 0, slot 1, the synchronous calls
    // read ingestion (read_parse.hip)
    DevBuf p_text, p_nl, p_scal, p_spans, p_off, p_len1, p_bases, p_qual;
    // matchAll workspace
    DevBuf raw, raw_count, hit_cnt, big_list, all_cursor, keys_a, keys_b, vals_a, vals_b, sort_tmp, hit_off, s_hits;

    // the stages behind the matcher, one record each: what a record holds is said in its header
    RhJoinStage join;                  // paired-end join (pair_kernel.hip)
    RhSearchStage search;              // mate search (mate_search.hip)
    RhPairAllStage pair_all;           // every concordant pair of a fragment (pair_all.hip)
    RhSingleStage single;              // single placements of a mate (single_fold.hip)
    RhInsertStage insert;              // insert-size histogram (insert_hist.hip)
    RhPileupStage pileup;              // pileup (pileup.hip)
    RhCallStage call;                  // variant calls (snp_call.hip)
    RhMismatchStage mismatch;          // mismatch lists (mismatch_list.hip)
    RhDupStage dup;                    // duplicate marking (duplicates.hip)
    RhMapqStage mapq;                  // mapping quality (mapq.hip)
    RhGapStage gap;                    // gap rescue, anchored gap placement, gapped mismatch lists (gap_rescue.hip, gap_anchor.hip, gapped_list.hip)
    RhIndelStage indel;                // indel calls (indel_call.hip)
    RhPileupGappedStage pileup_gapped; // gapped placements in the pileup and the calls (pileup_gapped.hip)
    RhDupGappedStage dup_gapped;       // joint duplicate marking over info words and gap records (duplicates.hip)

    // where the wall time of an index build goes (real_hip_index_build_stats)
    double   alloc_ms = 0, free_ms = 0, build_wall_ms = 0;
    uint64_t alloc_bytes = 0, alloc_calls = 0, free_calls = 0;

    // multi-GPU (gather.hip): an RCCL communicator over the ranks' devices, one process per GPU
    void *comm = nullptr;
    int comm_rank = 0, comm_size = 1;
    DevBuf comm_counts, comm_scratch;

    // timing
    bool timing = true;
    double   k_ms[REAL_HIP_K_COUNT] = {};
    uint64_t k_n[REAL_HIP_K_COUNT] = {};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // asynchronous timing of pipelined launches: event pairs resolved at the next synchronisation point
    struct Pending { hipEvent_t a, b; double *ms; uint64_t *n; }; // where the time goes: a k_ms / k_n slot, or a stage's kernel_ms (n null)
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
};

struct RhTimer { // HIP events on the ctx stream around a group of launches
    real_hip_ctx *c;
    int which;
    RhTimer(real_hip_ctx *ctx, int w);
    ~RhTimer();
};

// the launch of a kernel that takes one thread per element, 256 to a block; nothing is launched for n = 0.  The arguments
// convert as they do in a plain launch: implicitly, so a pointer of another type does not compile
template <typename... P, typename... A>
static inline void rh_launch_each(void (*kernel)(P...), uint64_t n, hipStream_t st, const A &...args)
{
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    if (n) hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, args...);
}

// ---- kernels launchers (match_kernels.hip) -----------------------------------
void rh_comm_destroy(real_hip_ctx *ctx);
int rh_launch_match(real_hip_ctx *ctx, const MatchArgs &a, bool all, int state_slot);
int rh_match_finish(real_hip_ctx *ctx, int state_slot); // after the launch has completed: errors the kernels flagged

// asynchronous kernel timing (no host synchronisation at the launch site)
void rh_time_begin(real_hip_ctx *ctx, hipStream_t st, int which);   // a public kernel id: k_ms / k_n
void rh_time_begin(real_hip_ctx *ctx, hipStream_t st, RhStage &stage); // a paired stage: its kernel_ms
void rh_time_end(real_hip_ctx *ctx, hipStream_t st);
void rh_time_resolve(real_hip_ctx *ctx); // call after the streams were synchronised
// the bracket as a scope: a return between begin and end (RH_HIP) still closes it, so no Pending record stays without its end
// event.  The end is recorded where the scope ends: braces where that is before a host synchronisation.
struct RhTimed {
    real_hip_ctx *c;
    hipStream_t st;
    RhTimed(real_hip_ctx *ctx, hipStream_t s, int which) : c(ctx), st(s) { rh_time_begin(c, st, which); }
    RhTimed(real_hip_ctx *ctx, hipStream_t s, RhStage &stage) : c(ctx), st(s) { rh_time_begin(c, st, stage); }
    RhTimed(const RhTimed &) = delete;
    RhTimed &operator=(const RhTimed &) = delete;
    ~RhTimed() { rh_time_end(c, st); }
};
// synchronises the ctx's stream on the way out of a scope, whichever way: declared BEHIND the ScopedBufs a function's kernels
// use, it runs before they are released
struct RhSyncOnExit {
    real_hip_ctx *c;
    explicit RhSyncOnExit(real_hip_ctx *ctx) : c(ctx) {}
    RhSyncOnExit(const RhSyncOnExit &) = delete;
    RhSyncOnExit &operator=(const RhSyncOnExit &) = delete;
    ~RhSyncOnExit() { (void)hipStreamSynchronize(c->stream); }
};
int rh_max_patl(real_hip_ctx *ctx, const uint64_t *d_off, uint64_t n_reads, uint32_t *out);
int rh_parse_reads(real_hip_ctx *ctx, const char *d_text, uint64_t n_bytes, int fastq, int qoff, real_hip_parsed *out);
int rh_all_finish(real_hip_ctx *ctx, uint64_t n_raw, uint64_t n_reads, real_hip_hit *d_out,
                  uint64_t *d_hit_offsets);

// ---- text + index (index_build.hip; the plan itself: index_plan.h) ---------------
int rh_pack_text(real_hip_ctx *ctx, const uint8_t *d_sym, uint64_t n);
int rh_count_wild(real_hip_ctx *ctx, uint64_t n); // n_wild of a text that was set packed
int rh_index_from_host_lists(real_hip_ctx *ctx, uint64_t n, const void *const sign[6], const uint32_t *const pos[6], unsigned sig_bytes);
int rh_index_build_device(real_hip_ctx *ctx, uint64_t first_window, uint64_t max_entries,
                          uint64_t *n_entries, int *have_next);
void rh_choose_tables(real_hip_ctx *ctx, uint64_t n_entries); // sets ctx->pb and ctx->layout (rh_plan_tables for this device)
// ---- read-back of the resident index (index_readback.hip: tests, CPU baseline) ----
int rh_rows_unpack(real_hip_ctx *ctx, int list, uint2 *d_entries, uint32_t *d_starts, bool canonical);
int rh_index_export(real_hip_ctx *ctx, int list, void *h_sign, uint32_t *h_pos);
