// pair_kernel.hip -- the paired-end join: per fragment, the best and the second-best concordant pair among
// (hits of mate 1) x (hits of mate 2), folded into the fragment's in/out record (include/real_hip.h, "paired-end reads").
//
// Two kernels.  pair_lane_kernel: one lane per fragment walks the whole product when it has at most RH_PAIR_LANE_BUDGET
// cells (the i.i.d. case: about one hit per mate, one cell).  A lane with a product of P cells keeps its whole wave for
// P turns, a wave of its own finishes it in ceil(P / 64) turns plus a 6-step butterfly over the ten words of a fold state
// (about twenty turns' worth): beyond a few dozen cells the wave is cheaper, so such fragments are appended to a list
// (one atomic per wave) and pair_wave_kernel gives each a wave.  It walks the shorter list one hit at a time (the same
// hit in every lane) and strides the lanes over the longer one (coalesced 16-byte loads).
//
// Nothing depends on the order of the hits or of the lanes: the fold state is the top two of a set under the total
// order (value descending, location ascending), and merging two states is associative and commutative.  No LDS, no
// scratch memory; plain C++ and vector stores.
#include "real_hip_ctx.h"
#include "pair_state.h"

struct PairArgs {
    MateLists L;                   // the hit lists of mate 1 / mate 2
    uint64_t n;                    // fragments
    real_hip_pair *pairs;
    uint32_t *list;                // fragments handed to the wave kernel
    unsigned long long *list_count;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] products, [1] handed over
    double filter_mult;
    uint32_t fresh, fileid, scores, min_insert, max_insert;
};

// one cell of the product: a concordant pair (pair_state.h) is folded into the state
static __device__ __forceinline__ void pair_cell(PairState &st, const uint4 a, const uint4 b, uint32_t la, uint32_t lb, const PairArgs &A)
{
    uint64_t outer;
    if (!pair_concordant(a, b, la, lb, A.min_insert, A.max_insert, outer)) return;
    PairState c;
    ps_candidate(c, A.scores, A.fileid, a.w & 0xffffu, a.y, b.y, (a.w >> 24) ? 1u : 0u, a.z, b.z, (a.w >> 16) & 0xffu, (b.w >> 16) & 0xffu);
    ps_merge(st, c);
}

__global__ void __launch_bounds__(256) pair_lane_kernel(const PairArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < A.n;
    uint64_t lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
    if (live) { A.L.range(0, i, lo1, hi1); A.L.range(1, i, lo2, hi2); }
    const uint64_t n1 = hi1 - lo1, n2 = hi2 - lo2;
    unsigned long long cells = (n1 && n2) ? ((n1 > 0xffffffffull || n2 > 0xffffffffull) ? ~0ull : n1 * n2) : 0ull;
    const bool big = cells > RH_PAIR_LANE_BUDGET;
    if (live && !big) {
        const uint32_t la = A.L.len[0][i], lb = A.L.len[1][i];
        PairState st;
        ps_clear(st);
        if (!A.fresh) ps_from_record(st, A.pairs[i]);
        for (uint64_t x = lo1; cells && x < hi1; ++x) {
            const uint4 a = A.L.h[0][x];
            for (uint64_t y = lo2; y < hi2; ++y) pair_cell(st, a, A.L.h[1][y], la, lb, A);
        }
        real_hip_pair r;
        ps_to_record(st, ps_eps(A.scores, A.filter_mult, la, lb), r);
        A.pairs[i] = r;
    }
    pair_hand_over(live && big, (uint32_t)i, cells, blockIdx.x, A.list, A.list_count, A.stats);
}

__global__ void __launch_bounds__(256) pair_wave_kernel(const PairArgs A)
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
        PairState st;
        ps_clear(st);
        if (hi2 - lo2 >= hi1 - lo1) { // lanes over the longer list
            for (uint64_t x = lo1; x < hi1; ++x) {
                const uint4 a = A.L.h[0][x];
                for (uint64_t y = lo2 + lane; y < hi2; y += 64) pair_cell(st, a, A.L.h[1][y], la, lb, A);
            }
        } else {
            for (uint64_t y = lo2; y < hi2; ++y) {
                const uint4 b = A.L.h[1][y];
                for (uint64_t x = lo1 + lane; x < hi1; x += 64) pair_cell(st, A.L.h[0][x], b, la, lb, A);
            }
        }
        ps_butterfly(st);
        if (lane == 0) {
            if (!A.fresh) { PairState in; ps_from_record(in, A.pairs[i]); ps_merge(st, in); }
            real_hip_pair r;
            ps_to_record(st, ps_eps(A.scores, A.filter_mult, la, lb), r);
            A.pairs[i] = r;
        }
    }
}

// read lengths of a staged batch (offsets, or the uniform length)
__global__ void pair_len_kernel(const uint64_t *__restrict__ off, uint32_t upatl, uint64_t n, uint32_t *__restrict__ len)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t l = upatl;
    if (off) l = off[i + 1] >= off[i] ? off[i + 1] - off[i] : 0;
    len[i] = l > 0xffffffffull ? 0xffffffffu : (uint32_t)l;
}

int rh_pair_lens(real_hip_ctx *ctx, const uint64_t *d_off, uint32_t upatl, uint64_t n, uint32_t *d_len)
{
    if (!n) return REAL_HIP_OK;
    hipLaunchKernelGGL(pair_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_off, upatl, n, d_len);
    RH_HIP(ctx, hipGetLastError());
    return REAL_HIP_OK;
}

// the join of n fragments on device arrays; asynchronous on the ctx's stream
int rh_launch_pair(real_hip_ctx *ctx, const real_hip_pair_params &pp, const MateLists &L, uint64_t n, uint32_t fileid, int fresh, real_hip_pair *d_pairs)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->join.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, ctx->join.list, n * 4 + 8))) return rc;
    PairArgs A;
    A.L = L; A.n = n; A.pairs = d_pairs;
    A.list_count = (unsigned long long *)ctx->join.list.p; A.list = (uint32_t *)ctx->join.list.p + 2;
    A.stats = (unsigned long long *)ctx->join.stage.stats.p;
    A.filter_mult = ctx->prm.filter_mult;
    A.fresh = fresh ? 1u : 0u; A.fileid = fileid; A.scores = ctx->prm.scores ? 1u : 0u;
    A.min_insert = pp.min_insert; A.max_insert = pp.max_insert;
    RH_HIP(ctx, hipMemsetAsync(ctx->join.list.p, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, REAL_HIP_K_PAIR);
    hipLaunchKernelGGL(pair_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    rh_time_begin(ctx, ctx->stream, REAL_HIP_K_PAIR_WAVE);
    hipLaunchKernelGGL(pair_wave_kernel, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->join.stage.items += n;
    return REAL_HIP_OK;
}

int rh_pair_stats(real_hip_ctx *ctx, real_hip_pair_stats *out, int reset)
{
    uint64_t h[2];
    int rc;
    if ((rc = rh_stats_read(ctx, ctx->join.stage.stats, RH_PAIR_STRIPES, 2, reset, h))) return rc; // (its times are read by real_hip_kernel_time)
    if (out) { out->pairs = ctx->join.stage.items; out->products = h[0]; out->handed_over = h[1]; }
    if (reset) ctx->join.stage.items = 0;
    return REAL_HIP_OK;
}
