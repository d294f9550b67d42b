// single_fold.hip -- the single placements of a mate: per read, the best and the second-best of its hits, folded into the
// read's in/out record (include/real_hip.h, "single placements of a mate").  The structure is the join's (pair_kernel.hip).
//
// Two kernels, each covering up to two lists (the two mates of real_hip_match_pairs_singles: blockIdx.y of the lane kernel,
// bit 32 of a hand-over entry).  single_lane_kernel: one lane per read walks a list of at most RH_SINGLE_LANE_BUDGET hits;
// longer lists are appended to a hand-over list (one atomic per wave) and single_wave_kernel gives each a wave: the lanes
// stride over the list (coalesced 16-byte loads) and a 6-step butterfly merges their states.
//
// Nothing depends on the order of the hits, the lanes or the waves: merging two states (single_state.h) is associative and
// commutative.  No LDS, no scratch memory; plain C++ and vector stores.
#include "real_hip_ctx.h"
#include "single_state.h"

struct SingleArgs {
    MateLists L;                   // the hit lists of list 0 / list 1 (pair_state.h)
    uint4 *out[2];                 // real_hip_single records, in/out
    uint64_t n;                    // reads per list
    unsigned long long *list;      // reads handed to the wave kernel: list << 32 | read
    unsigned long long *list_count;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] hits walked, [1] handed over
    double filter_mult;
    uint32_t fresh, fileid, scores;
};

static __device__ __forceinline__ double single_eps(const SingleArgs &A, uint32_t len)
{
    return A.scores ? (double)(float)(A.filter_mult * (double)len) : 0.0;
}

__global__ void __launch_bounds__(256) single_lane_kernel(const SingleArgs A)
{
    // (uniform.  The list is picked by selects between the two constant slots, which sit in scalar registers: A.L.h[m] is a
    // load from the argument segment in every wave, and the fold's kernels measured about 1 % slower with it)
    const uint32_t m = blockIdx.y;
    const uint4 *h = m ? A.L.h[1] : A.L.h[0];
    uint4 *out = m ? A.out[1] : A.out[0];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < A.n;
    uint64_t lo = 0, hi = 0;
    if (live) { if (m) A.L.range(1, i, lo, hi); else A.L.range(0, i, lo, hi); }
    unsigned long long cnt = hi - lo;
    const bool big = cnt > RH_SINGLE_LANE_BUDGET;
    if (live && !big) {
        SingleState st;
        ss_clear(st);
        if (!A.fresh) ss_from_record(st, out[i], A.scores);
        for (uint64_t x = lo; x < hi; ++x) {
            SingleState c;
            ss_from_hit(c, h[x], A.fileid, A.scores);
            ss_merge(st, c);
        }
        out[i] = ss_to_record(st, single_eps(A, (m ? A.L.len[1] : A.L.len[0])[i]));
    }
    pair_hand_over(live && big, ((unsigned long long)m << 32) | i, cnt, blockIdx.x + blockIdx.y, A.list, A.list_count, A.stats);
}

__global__ void __launch_bounds__(256) single_wave_kernel(const SingleArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long count = *A.list_count;
    for (uint64_t w = wave; w < count; w += n_waves) {
        const unsigned long long e = A.list[w];
        const uint32_t m = (uint32_t)(e >> 32);
        const uint64_t i = e & 0xffffffffull;
        const uint4 *h = m ? A.L.h[1] : A.L.h[0];
        uint4 *out = m ? A.out[1] : A.out[0];
        uint64_t lo, hi;
        if (m) A.L.range(1, i, lo, hi); else A.L.range(0, i, lo, hi);
        SingleState st;
        ss_clear(st);
        for (uint64_t x = lo + lane; x < hi; x += 64) {
            SingleState c;
            ss_from_hit(c, h[x], A.fileid, A.scores);
            ss_merge(st, c);
        }
        for (int d = 32; d; d >>= 1) { // butterfly: every lane ends with the wave's state
            SingleState b;
            b.best = __shfl_xor(st.best, d); b.second = __shfl_xor(st.second, d);
            b.loc = __shfl_xor((unsigned long long)st.loc, d);
            b.s = __shfl_xor(st.s, d); b.k = __shfl_xor(st.k, d);
            ss_merge(st, b);
        }
        if (lane == 0) {
            if (!A.fresh) { SingleState in; ss_from_record(in, out[i], A.scores); ss_merge(st, in); }
            out[i] = ss_to_record(st, single_eps(A, (m ? A.L.len[1] : A.L.len[0])[i]));
        }
    }
}

// the fold of n reads of each of `lists` (1 or 2) lists on device arrays; asynchronous on the ctx's stream
int rh_launch_single(real_hip_ctx *ctx, int lists, const MateLists &L, uint64_t n, uint32_t fileid, int fresh, real_hip_single *const d_out[2])
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 reads in one call", hipSuccess);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->single.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, ctx->single.list, (size_t)lists * n * 8 + 8))) return rc;
    const int l1 = lists > 1 ? 1 : 0; // (one list: both slots describe it, slot 1 is never selected)
    SingleArgs A;
    A.L = L;
    A.L.h[1] = L.h[l1]; A.L.o[1] = L.o[l1]; A.L.len[1] = L.len[l1]; A.L.total[1] = L.total[l1];
    A.out[0] = (uint4 *)d_out[0]; A.out[1] = (uint4 *)d_out[l1];
    A.n = n;
    A.list_count = (unsigned long long *)ctx->single.list.p; A.list = (unsigned long long *)ctx->single.list.p + 1;
    A.stats = (unsigned long long *)ctx->single.stage.stats.p;
    A.filter_mult = ctx->prm.filter_mult;
    A.fresh = fresh ? 1u : 0u; A.fileid = fileid; A.scores = ctx->prm.scores ? 1u : 0u;
    RH_HIP(ctx, hipMemsetAsync(ctx->single.list.p, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, ctx->single.stage);
    hipLaunchKernelGGL(single_lane_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)lists), dim3(256), 0, ctx->stream, A);
    RH_HIP(ctx, hipGetLastError());
    // a fixed grid of waves takes the handed-over reads in turn (their number stays on the device)
    const uint64_t work = (uint64_t)lists * n;
    hipLaunchKernelGGL(single_wave_kernel, dim3(rh_wave_blocks(work)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->single.stage.items += work;
    ctx->single.stage.launches += 2;
    return REAL_HIP_OK;
}

int rh_single_stats(real_hip_ctx *ctx, real_hip_single_stats *out, int reset)
{
    uint64_t h[2];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->single.stage, RH_PAIR_STRIPES, 2, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->reads = was.items; out->hits = h[0]; out->handed_over = h[1];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
