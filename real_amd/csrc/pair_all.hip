// pair_all.hip -- paired-end reads, every concordant pair of a fragment: the cells of (hits of mate 1) x (hits of mate 2)
// that pass the join's concordance test (pair_state.h), one 32-byte real_hip_pair_hit each, in row-major order of the
// product (include/real_hip.h, "every concordant pair").
//
// Count, scan, emit.  The count is known before a record is written, so a too small output is reported with the size
// needed and nothing is emitted.  The lane / wave split is the join's (pair_kernel.hip): a lane walks a product of at most
// RH_PAIR_LANE_BUDGET cells itself, larger fragments go to a list (one atomic per wave) and a fixed grid of waves takes
// them in turn.  A wave walks the FLATTENED cell index c = x * n2 + y, 64 consecutive cells per turn: the lanes are
// full whichever list is the long one, and a ballot with a prefix popcount gives every concordant cell its slot in cell
// order -- the output order is a function of the input order alone.  x and y are carried along (one small division per
// fragment, none per cell).  No LDS, no scratch memory; plain C++ and 16-byte vector stores.
#include "real_hip_ctx.h"
#include "pair_state.h"
#include "rocprim_call.h"

#include <rocprim/device/device_scan.hpp>

struct PairAllArgs {
    MateLists L;                   // the hit lists of mate 1 / mate 2
    uint64_t n;                    // fragments
    uint64_t *cnt;                 // n + 1: concordant pairs per fragment (count kernels; cnt[n] = 0)
    const uint64_t *off;           // n + 1: their exclusive scan (emit kernels)
    uint4 *out;                    // real_hip_pair_hit records, two uint4 each
    uint64_t cap;                  // records out holds
    uint32_t *list;                // fragments handed to the wave kernels
    unsigned long long *list_count;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] products, [1] handed over
    uint32_t fileid, min_insert, max_insert;
};

static __device__ __forceinline__ unsigned long long pair_all_cells(uint64_t n1, uint64_t n2)
{
    return (n1 && n2) ? ((n1 > 0xffffffffull || n2 > 0xffffffffull) ? ~0ull : n1 * n2) : 0ull;
}

// real_hip_pair_hit as two uint4: {pair, pos1, pos2, outer}, {score1, score2, frag:16 | fileid:8 | inverted1:8, k1:8 | k2:8 | 0:16}
static __device__ __forceinline__ void pair_all_store(const PairAllArgs &A, uint64_t slot, uint32_t i, const uint4 a, const uint4 b, uint64_t outer)
{
    if (slot >= A.cap) return; // (cannot happen while the lists stay as the count saw them)
    A.out[2 * slot] = make_uint4(i, a.y, b.y, (uint32_t)outer);
    A.out[2 * slot + 1] = make_uint4(a.z, b.z, (a.w & 0xffffu) | ((A.fileid & 0xffu) << 16) | ((a.w >> 24) ? 1u << 24 : 0u),
                                     ((a.w >> 16) & 0xffu) | (((b.w >> 16) & 0xffu) << 8));
}

// one lane per fragment: EMIT = false counts the concordant cells of a small product into cnt[] and hands the large ones
// over; EMIT = true writes the records of the small ones behind off[]
template <bool EMIT>
__global__ void __launch_bounds__(256) pair_all_lane_kernel(const PairAllArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < A.n;
    uint64_t lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
    if (live) { A.L.range(0, i, lo1, hi1); A.L.range(1, i, lo2, hi2); }
    unsigned long long cells = pair_all_cells(hi1 - lo1, hi2 - lo2);
    const bool big = cells > RH_PAIR_LANE_BUDGET;
    if (live && !big) {
        uint64_t found = 0, slot = EMIT ? A.off[i] : 0;
        if (cells) {
            const uint32_t la = A.L.len[0][i], lb = A.L.len[1][i];
            for (uint64_t x = lo1; x < hi1; ++x) {
                const uint4 a = A.L.h[0][x];
                for (uint64_t y = lo2; y < hi2; ++y) {
                    const uint4 b = A.L.h[1][y];
                    uint64_t outer;
                    if (!pair_concordant(a, b, la, lb, A.min_insert, A.max_insert, outer)) continue;
                    if (EMIT) pair_all_store(A, slot++, (uint32_t)i, a, b, outer);
                    else ++found;
                }
            }
        }
        if (!EMIT) A.cnt[i] = found;
    }
    if (EMIT) return;
    if (i == A.n) A.cnt[i] = 0; // (the grid covers n + 1 lanes)
    pair_hand_over(live && big, (uint32_t)i, cells, blockIdx.x, A.list, A.list_count, A.stats);
}

// one wave per handed-over fragment, 64 consecutive cells of the flattened product per turn
template <bool EMIT>
__global__ void __launch_bounds__(256) pair_all_wave_kernel(const PairAllArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long count = *A.list_count;
    for (uint64_t w = wave; w < count; w += n_waves) {
        const uint32_t i = A.list[w];
        uint64_t lo1, hi1, lo2, hi2;
        A.L.range(0, i, lo1, hi1);
        A.L.range(1, i, lo2, hi2);
        const uint64_t n1 = hi1 - lo1, n2 = hi2 - lo2;
        const unsigned long long cells = pair_all_cells(n1, n2);
        const uint32_t la = A.L.len[0][i], lb = A.L.len[1][i];
        // cell lane of the first turn, and the step of 64 cells as (rows, columns): y + ystep < 2 * n2
        uint64_t x, y, xstep, ystep;
        if (n2 > 64) { x = 0; y = lane; xstep = 0; ystep = 64; }
        else { const uint32_t m = (uint32_t)n2; x = lane / m; y = lane % m; xstep = 64u / m; ystep = 64u % m; }
        uint64_t found = EMIT ? A.off[i] : 0; // EMIT: the next free slot
        for (unsigned long long c0 = 0; c0 < cells; c0 += 64) {
            bool ok = false;
            uint4 a = make_uint4(0, 0, 0, 0), b = a;
            uint64_t outer = 0;
            if (x < n1) { // (c0 + lane < cells)
                a = A.L.h[0][lo1 + x]; b = A.L.h[1][lo2 + y];
                ok = pair_concordant(a, b, la, lb, A.min_insert, A.max_insert, outer);
            }
            const unsigned long long mask = __ballot(ok);
            if (EMIT && ok) pair_all_store(A, found + __popcll(mask & ((1ull << lane) - 1ull)), i, a, b, outer);
            found += __popcll(mask);
            x += xstep; y += ystep;
            if (y >= n2) { y -= n2; ++x; }
        }
        if (!EMIT && lane == 0) A.cnt[i] = found;
    }
}

// Phase 1 of the enumeration of n fragments on device arrays: counts, their scan into d_off (n + 1 entries, device) and the
// total, read back (the stream is synchronised).  Phase 2, rh_pair_all_emit, writes the records; the caller decides in
// between whether they fit.
static PairAllArgs pair_all_args(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint32_t fileid, const uint64_t *d_off)
{
    PairAllArgs A;
    A.L = L; A.n = n;
    A.cnt = (uint64_t *)ctx->pair_all.cnt.p; A.off = d_off; A.out = nullptr; A.cap = 0;
    A.list_count = (unsigned long long *)ctx->join.list.p; A.list = (uint32_t *)ctx->join.list.p + 2;
    A.stats = (unsigned long long *)ctx->pair_all.stage.stats.p;
    A.fileid = fileid; A.min_insert = pp.min_insert; A.max_insert = pp.max_insert;
    return A;
}

int rh_pair_all_count(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint64_t *d_off, uint64_t *total)
{
    *total = 0;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->pair_all.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, ctx->join.list, n * 4 + 8))) return rc;
    if ((rc = rh_reserve(ctx, ctx->pair_all.cnt, (n + 1) * 8))) return rc;
    const PairAllArgs A = pair_all_args(ctx, pp, L, n, 0, d_off);
    RH_HIP(ctx, hipMemsetAsync(ctx->join.list.p, 0, 8, ctx->stream));
    { // (the bracket ends before the read-back)
        RhTimed timed(ctx, ctx->stream, ctx->pair_all.stage);
        rh_launch_each(pair_all_lane_kernel<false>, n + 1, ctx->stream, A);
        RH_HIP(ctx, hipGetLastError());
        if (n) {
            hipLaunchKernelGGL(pair_all_wave_kernel<false>, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
            RH_HIP(ctx, hipGetLastError());
            ctx->pair_all.stage.launches += 1;
        }
        ctx->pair_all.stage.launches += 1;
        auto scan = [&](void *tmp, size_t &bytes) { return rocprim::exclusive_scan(tmp, bytes, A.cnt, d_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), ctx->stream); };
        if ((rc = rh_prim_run(ctx, ctx->sort_tmp, scan, "pair count scan"))) return rc;
    }
    RH_HIP(ctx, hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pair_all.stage.items += n;
    return REAL_HIP_OK;
}

// the records of the fragments counted last, behind d_off into d_out (cap records, 16-byte aligned); asynchronous on the
// ctx's stream.  The lists must be what rh_pair_all_count saw.
int rh_pair_all_emit(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint32_t fileid, const uint64_t *d_off,
                     real_hip_pair_hit *d_out, uint64_t cap, uint64_t total)
{
    if (!n || !total) return REAL_HIP_OK;
    PairAllArgs A = pair_all_args(ctx, pp, L, n, fileid, d_off);
    A.out = (uint4 *)d_out; A.cap = cap;
    {
        RhTimed timed(ctx, ctx->stream, ctx->pair_all.stage);
        rh_launch_each(pair_all_lane_kernel<true>, n, ctx->stream, A);
        RH_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(pair_all_wave_kernel<true>, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
    }
    RH_HIP(ctx, hipGetLastError());
    ctx->pair_all.stage.launches += 2;
    ctx->pair_all.pairs_out += total;
    return REAL_HIP_OK;
}

int rh_pair_all_stats(real_hip_ctx *ctx, real_hip_pair_all_stats *out, int reset)
{
    uint64_t h[2];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->pair_all.stage, RH_PAIR_STRIPES, 2, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->fragments = was.items; out->products = h[0]; out->pairs_out = ctx->pair_all.pairs_out; out->handed_over = h[1];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    if (reset) ctx->pair_all.pairs_out = 0;
    return REAL_HIP_OK;
}
