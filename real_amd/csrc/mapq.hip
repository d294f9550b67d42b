// mapq.hip -- mapping quality (include/real_hip.h, "mapping quality"): per read (fragment) the histogram of ALL its candidates'
// levels, folded into the in/out accumulator, and the finish that turns final records and accumulators into one byte per read.
//
// The folds have the structure of single_fold.hip and pair_kernel.hip.  mapq_lane_kernel: one lane per read walks a list of at
// most RH_SINGLE_LANE_BUDGET hits (up to two lists: blockIdx.y, the two mates of real_hip_match_pairs_mapq); longer lists go
// to a hand-over list (pair_hand_over: one atomic per wave) and mapq_wave_kernel gives each a wave: the lanes stride over the
// list (coalesced 16-byte loads), a 6-step butterfly merges their states and lane 0 folds the in/out record.
// mapq_pair_lane_kernel / mapq_pair_wave_kernel do the same over the product of the two mates' lists, a cell being a candidate
// iff it is concordant (pair_concordant), with the join's budget RH_PAIR_LANE_BUDGET.
// The finish kernels are one lane per read / fragment.
//
// Nothing depends on the order of the hits, the lanes or the waves: the merge (mapq_state.h) is associative and commutative.
// No LDS, no scratch memory; plain C++ and vector stores.
#include "real_hip_ctx.h"
#include "single_state.h" // RH_SINGLE_LANE_BUDGET, pair_state.h
#include "mapq_state.h"

#include <cstring>

typedef unsigned long long mq_word;

static __device__ __forceinline__ void mq_load(MapqState &s, const mq_word *acc, uint64_t i)
{
    const mq_word *r = acc + i * 5;
    mq_from_words(s, r[0], r[1], r[2], r[3], r[4]);
}
static __device__ __forceinline__ void mq_store(const MapqState &s, mq_word *acc, uint64_t i)
{
    mq_word *r = acc + i * 5;
    r[0] = mq_word0(s); r[1] = s.c0; r[2] = s.c1; r[3] = s.c2; r[4] = s.c3;
}
// butterfly: every lane ends with the wave's state
static __device__ __forceinline__ void mq_butterfly(MapqState &st)
{
    for (int d = 32; d; d >>= 1) {
        MapqState o;
        o.level = __shfl_xor(st.level, d); o.n = __shfl_xor(st.n, d);
        o.c0 = __shfl_xor((mq_word)st.c0, d); o.c1 = __shfl_xor((mq_word)st.c1, d);
        o.c2 = __shfl_xor((mq_word)st.c2, d); o.c3 = __shfl_xor((mq_word)st.c3, d);
        mq_merge(st, o);
    }
}
// real_hip_hit as a uint4: x read, y pos, z score bits, w frag:16 | k:8 | inverted:8
static __device__ __forceinline__ int32_t mq_hit_level(const uint4 h, uint32_t scores)
{
    return scores ? mq_level_of_value((double)__uint_as_float(h.z)) : mq_level_of_k((h.w >> 16) & 0xffu);
}

// ---- the fold of hit lists ------------------------------------------------------------------------------------------
struct MapqArgs {
    MateLists L;                   // the hit lists of list 0 / list 1 (pair_state.h; the lengths are not read)
    mq_word *acc[2];               // real_hip_mapq_acc records as five words, in/out
    uint64_t n;                    // reads per list
    mq_word *list;                 // reads handed to the wave kernel: list << 32 | read
    mq_word *list_count;
    mq_word *stats;                // RH_PAIR_STRIPES x 16 words: [0] candidates walked, [1] handed over, [2] placements, [3] unlisted
    uint32_t fresh, scores;
};

__global__ void __launch_bounds__(256) mapq_lane_kernel(const MapqArgs A)
{
    const uint32_t m = blockIdx.y; // (uniform; selects between the two constant slots, as in single_lane_kernel)
    const uint4 *h = m ? A.L.h[1] : A.L.h[0];
    mq_word *acc = m ? A.acc[1] : A.acc[0];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < A.n;
    uint64_t lo = 0, hi = 0;
    if (live) { if (m) A.L.range(1, i, lo, hi); else A.L.range(0, i, lo, hi); }
    const unsigned long long cnt = hi - lo;
    const bool big = cnt > RH_SINGLE_LANE_BUDGET;
    if (live && !big) {
        MapqState st;
        mq_clear(st);
        if (!A.fresh) mq_load(st, acc, i);
        for (uint64_t x = lo; x < hi; ++x) mq_add_level(st, mq_hit_level(h[x], A.scores));
        mq_store(st, acc, i);
    }
    pair_hand_over(live && big, ((mq_word)m << 32) | i, cnt, blockIdx.x + blockIdx.y, A.list, A.list_count, A.stats);
}

__global__ void __launch_bounds__(256) mapq_wave_kernel(const MapqArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long count = *A.list_count;
    for (uint64_t w = wave; w < count; w += n_waves) {
        const unsigned long long e = A.list[w];
        const uint32_t m = (uint32_t)(e >> 32);
        const uint64_t i = e & 0xffffffffull;
        const uint4 *h = m ? A.L.h[1] : A.L.h[0];
        mq_word *acc = m ? A.acc[1] : A.acc[0];
        uint64_t lo, hi;
        if (m) A.L.range(1, i, lo, hi); else A.L.range(0, i, lo, hi);
        MapqState st;
        mq_clear(st);
        for (uint64_t x = lo + lane; x < hi; x += 64) mq_add_level(st, mq_hit_level(h[x], A.scores));
        mq_butterfly(st);
        if (lane == 0) {
            if (!A.fresh) { MapqState in; mq_load(in, acc, i); mq_merge(st, in); }
            mq_store(st, acc, i);
        }
    }
}

// the fold of n reads of each of `lists` (1 or 2) lists on device arrays; asynchronous on the ctx's stream
int rh_launch_mapq_fold(real_hip_ctx *ctx, int lists, const MateLists &L, uint64_t n, int fresh, real_hip_mapq_acc *const d_acc[2])
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one call", hipSuccess);
    RhMapqStage &S = ctx->mapq;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, S.list, (size_t)lists * n * 8 + 8))) return rc;
    const int l1 = lists > 1 ? 1 : 0; // (one list: both slots describe it, slot 1 is never selected)
    MapqArgs A;
    A.L = L;
    A.L.h[1] = L.h[l1]; A.L.o[1] = L.o[l1]; A.L.len[1] = L.len[l1]; A.L.total[1] = L.total[l1];
    A.acc[0] = (mq_word *)d_acc[0]; A.acc[1] = (mq_word *)d_acc[l1];
    A.n = n;
    A.list_count = (mq_word *)S.list.p; A.list = (mq_word *)S.list.p + 1;
    A.stats = (mq_word *)S.stage.stats.p;
    A.fresh = fresh ? 1u : 0u; A.scores = ctx->prm.scores ? 1u : 0u;
    RH_HIP(ctx, hipMemsetAsync(S.list.p, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, S.stage);
    hipLaunchKernelGGL(mapq_lane_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)lists), dim3(256), 0, ctx->stream, A);
    RH_HIP(ctx, hipGetLastError());
    // a fixed grid of waves takes the handed-over reads in turn (their number stays on the device)
    const uint64_t work = (uint64_t)lists * n;
    hipLaunchKernelGGL(mapq_wave_kernel, dim3(rh_wave_blocks(work)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    S.stage.items += work;
    S.stage.launches += 2;
    return REAL_HIP_OK;
}

// ---- the fold of the concordant pairs ------------------------------------------------------------------------------------
struct MapqPairArgs {
    MateLists L;                   // the hit lists of mate 1 / mate 2
    uint64_t n;                    // fragments
    mq_word *acc;
    uint32_t *list;                // fragments handed to the wave kernel
    mq_word *list_count;
    mq_word *stats;                // as MapqArgs: [0] product cells walked, [1] handed over
    uint32_t fresh, scores, min_insert, max_insert;
};

// one cell of the product: a concordant pair (pair_state.h) is a candidate
static __device__ __forceinline__ void mapq_pair_cell(MapqState &st, const uint4 a, const uint4 b, uint32_t la, uint32_t lb, const MapqPairArgs &A)
{
    uint64_t outer;
    if (!pair_concordant(a, b, la, lb, A.min_insert, A.max_insert, outer)) return;
    const int32_t level = A.scores ? mq_level_of_value((double)__uint_as_float(a.z) + (double)__uint_as_float(b.z))
                                   : mq_level_of_k(((a.w >> 16) & 0xffu) + ((b.w >> 16) & 0xffu));
    mq_add_level(st, level);
}

__global__ void __launch_bounds__(256) mapq_pair_lane_kernel(const MapqPairArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < A.n;
    uint64_t lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
    if (live) { A.L.range(0, i, lo1, hi1); A.L.range(1, i, lo2, hi2); }
    const uint64_t n1 = hi1 - lo1, n2 = hi2 - lo2;
    const unsigned long long cells = (n1 && n2) ? ((n1 > 0xffffffffull || n2 > 0xffffffffull) ? ~0ull : n1 * n2) : 0ull;
    const bool big = cells > RH_PAIR_LANE_BUDGET;
    if (live && !big) {
        const uint32_t la = A.L.len[0][i], lb = A.L.len[1][i];
        MapqState st;
        mq_clear(st);
        if (!A.fresh) mq_load(st, A.acc, i);
        for (uint64_t x = lo1; cells && x < hi1; ++x) {
            const uint4 a = A.L.h[0][x];
            for (uint64_t y = lo2; y < hi2; ++y) mapq_pair_cell(st, a, A.L.h[1][y], la, lb, A);
        }
        mq_store(st, A.acc, i);
    }
    pair_hand_over(live && big, (uint32_t)i, cells, blockIdx.x, A.list, A.list_count, A.stats);
}

__global__ void __launch_bounds__(256) mapq_pair_wave_kernel(const MapqPairArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long count = *A.list_count;
    for (uint64_t w = wave; w < count; w += n_waves) {
        const uint64_t i = A.list[w];
        uint64_t lo1, hi1, lo2, hi2;
        A.L.range(0, i, lo1, hi1);
        A.L.range(1, i, lo2, hi2);
        const uint32_t la = A.L.len[0][i], lb = A.L.len[1][i];
        MapqState st;
        mq_clear(st);
        if (hi2 - lo2 >= hi1 - lo1) { // lanes over the longer list
            for (uint64_t x = lo1; x < hi1; ++x) {
                const uint4 a = A.L.h[0][x];
                for (uint64_t y = lo2 + lane; y < hi2; y += 64) mapq_pair_cell(st, a, A.L.h[1][y], la, lb, A);
            }
        } else {
            for (uint64_t y = lo2; y < hi2; ++y) {
                const uint4 b = A.L.h[1][y];
                for (uint64_t x = lo1 + lane; x < hi1; x += 64) mapq_pair_cell(st, A.L.h[0][x], b, la, lb, A);
            }
        }
        mq_butterfly(st);
        if (lane == 0) {
            if (!A.fresh) { MapqState in; mq_load(in, A.acc, i); mq_merge(st, in); }
            mq_store(st, A.acc, i);
        }
    }
}

// the fold of n fragments' concordant pairs on device arrays; asynchronous on the ctx's stream
int rh_launch_mapq_pair_fold(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, int fresh, real_hip_mapq_acc *d_acc)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    RhMapqStage &S = ctx->mapq;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, S.pair_list, n * 4 + 8))) return rc;
    MapqPairArgs A;
    A.L = L; A.n = n; A.acc = (mq_word *)d_acc;
    A.list_count = (mq_word *)S.pair_list.p; A.list = (uint32_t *)S.pair_list.p + 2;
    A.stats = (mq_word *)S.stage.stats.p;
    A.fresh = fresh ? 1u : 0u; A.scores = ctx->prm.scores ? 1u : 0u;
    A.min_insert = pp.min_insert; A.max_insert = pp.max_insert;
    RH_HIP(ctx, hipMemsetAsync(S.pair_list.p, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, S.stage);
    hipLaunchKernelGGL(mapq_pair_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    RH_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(mapq_pair_wave_kernel, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    S.stage.items += n;
    S.stage.launches += 2;
    return REAL_HIP_OK;
}

// ---- the finish ------------------------------------------------------------------------------------------------------------
struct MapqFinishArgs {
    const uint64_t *info;          // single-end: the info words and their scores (scores on)
    const float *score;
    const uint2 *pairs;            // paired: real_hip_pair records as five 8-byte words (final_record.h), the mates' singles (nullable)
    const uint4 *singles[2];
    const mq_word *acc[3];         // single-end: [0]; paired: the pair's, mate 1's, mate 2's
    uint64_t n;
    uint8_t *out;                  // n bytes; paired: 2n, mate m of fragment i at 2i + m
    mq_word *stats;
    uint32_t scores;
};

// the quality of a placement of level lp against record i of acc; counts it in s[2] (placements) and s[3] (unlisted)
static __device__ __forceinline__ uint32_t mapq_placement(const mq_word *acc, uint64_t i, int32_t lp, uint32_t (&s)[4])
{
    MapqState st;
    mq_load(st, acc, i);
    bool unlisted;
    const uint32_t q = mq_quality(st, lp, unlisted);
    s[2] += 1; s[3] += unlisted ? 1u : 0u;
    return q;
}

__global__ void __launch_bounds__(256) mapq_finish_kernel(const MapqFinishArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s[4] = {0, 0, 0, 0}; // (words 0 and 1 of the stripe are the folds')
    if (i < A.n) {
        const RhPlace c = rh_place_info(A.info[i]);
        uint32_t q = REAL_HIP_MAPQ_NONE;
        if (c.place) q = mapq_placement(A.acc[0], i, A.scores ? mq_level_of_value((double)A.score[i]) : mq_level_of_k(c.k), s);
        A.out[i] = (uint8_t)q;
    }
    rh_stats_add(A.stats, s);
}

__global__ void __launch_bounds__(256) mapq_finish_pairs_kernel(const MapqFinishArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s[4] = {0, 0, 0, 0};
    if (i < A.n) {
        const uint2 tail = A.pairs[i * 5 + 4];
        const uint32_t state = rh_pair_state(tail.y);
        uint32_t q1 = REAL_HIP_MAPQ_NONE, q2 = REAL_HIP_MAPQ_NONE;
        if (state == REAL_HIP_PAIR_UNIQUE) {
            const uint2 b = A.pairs[i * 5]; // `best`
            const double best = __longlong_as_double((long long)(((uint64_t)b.y << 32) | b.x));
            const int32_t lp = A.scores ? mq_level_of_value(best) : mq_level_of_k(rh_pair_k1(tail.x) + rh_pair_k2(tail.y));
            q1 = q2 = mapq_placement(A.acc[0], i, lp, s);
            s[2] *= 2; s[3] *= 2; // (both mates are placements; this lane has counted nothing else)
        } else if (state == REAL_HIP_PAIR_NOMATCH && A.singles[0]) {
            const uint4 r1 = A.singles[0][i], r2 = A.singles[1][i];
            const RhPlace c1 = rh_place_single(r1.z, r1.w), c2 = rh_place_single(r2.z, r2.w);
            if (c1.place) q1 = mapq_placement(A.acc[1], i, A.scores ? mq_level_of_value((double)__uint_as_float(r1.x)) : mq_level_of_k(c1.k), s);
            if (c2.place) q2 = mapq_placement(A.acc[2], i, A.scores ? mq_level_of_value((double)__uint_as_float(r2.x)) : mq_level_of_k(c2.k), s);
        }
        A.out[2 * i] = (uint8_t)q1;
        A.out[2 * i + 1] = (uint8_t)q2;
    }
    rh_stats_add(A.stats, s);
}

// out[] of n reads (pairs null) or n fragments, all arrays on the device; asynchronous on the ctx's stream
int rh_launch_mapq_finish(real_hip_ctx *ctx, const uint64_t *d_info, const float *d_score, const real_hip_pair *d_pairs,
                          const real_hip_single *const d_singles[2], const real_hip_mapq_acc *const d_acc[3], uint64_t n, uint8_t *d_out)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 records in one call", hipSuccess);
    RhMapqStage &S = ctx->mapq;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    MapqFinishArgs A;
    A.info = d_info; A.score = d_score; A.pairs = (const uint2 *)d_pairs;
    for (int m = 0; m < 2; ++m) A.singles[m] = d_singles ? (const uint4 *)d_singles[m] : nullptr;
    for (int m = 0; m < 3; ++m) A.acc[m] = (const mq_word *)d_acc[m];
    A.n = n; A.out = d_out; A.stats = (mq_word *)S.stage.stats.p;
    A.scores = ctx->prm.scores ? 1u : 0u;
    rh_time_begin(ctx, ctx->stream, S.stage);
    if (d_pairs) hipLaunchKernelGGL(mapq_finish_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL(mapq_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    S.stage.launches += 1;
    return REAL_HIP_OK;
}

int rh_mapq_stats(real_hip_ctx *ctx, real_hip_mapq_stats *out, int reset)
{
    uint64_t h[4];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->mapq.stage, RH_PAIR_STRIPES, 4, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->folded = was.items; out->candidates = h[0]; out->handed_over = h[1]; out->placements = h[2]; out->unlisted = h[3];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}

// ---- host only: the same arithmetic without a ctx ------------------------------------------------------------------------
static void mq_from_acc(MapqState &s, const real_hip_mapq_acc &a)
{
    uint64_t w[5];
    memcpy(w, &a, sizeof w);
    mq_from_words(s, w[0], w[1], w[2], w[3], w[4]);
}
extern "C" int real_hip_mapq_acc_merge(real_hip_mapq_acc *a, const real_hip_mapq_acc *b)
{
    if (!a || !b) return REAL_HIP_E_INVALID;
    MapqState x, y;
    mq_from_acc(x, *a);
    mq_from_acc(y, *b);
    mq_merge(x, y);
    const uint64_t w[5] = {mq_word0(x), x.c0, x.c1, x.c2, x.c3};
    memcpy(a, w, sizeof w);
    return REAL_HIP_OK;
}
extern "C" int real_hip_mapq_of(const real_hip_mapq_acc *acc, int32_t level, int *unlisted)
{
    if (!acc) return REAL_HIP_E_INVALID;
    MapqState x;
    mq_from_acc(x, *acc);
    bool u;
    const uint32_t q = mq_quality(x, level, u);
    if (unlisted) *unlisted = u ? 1 : 0;
    return (int)q;
}
