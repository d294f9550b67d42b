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
#include "real_hip_internal.h"
#include "pair_state.h"

struct PairArgs {
    const uint4 *h1, *h2;          // real_hip_hit records of mate 1 / mate 2
    const uint64_t *o1, *o2;       // n + 1 offsets into them
    const uint32_t *len1, *len2;   // read lengths
    uint64_t n, total1, total2;    // fragments; an upper bound of the hits in h1 / h2 inside their buffers (real_hip_match_pairs passes the
                                   // matcher's count before duplicates go): the offsets are clamped to it, o[n] is the real end
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
    const uint32_t inva = a.w >> 24;
    const uint32_t ka = (a.w >> 16) & 0xffu, kb = (b.w >> 16) & 0xffu;
    PairState c;
    c.best = A.scores ? (double)__uint_as_float(a.z) + (double)__uint_as_float(b.z) : -(double)(ka + kb);
    c.second = pair_neg_inf();
    c.lhi = ((uint64_t)A.fileid << 48) | ((uint64_t)(a.w & 0xffffu) << 32) | a.y;
    c.llo = ((uint64_t)b.y << 1) | (inva ? 1u : 0u);
    c.s1 = a.z; c.s2 = b.z; c.k = ka | (kb << 8);
    ps_merge(st, c);
}

static __device__ __forceinline__ double pair_eps(const PairArgs &A, uint32_t la, uint32_t lb)
{
    return A.scores ? (double)(float)(A.filter_mult * (double)((uint64_t)la + lb)) : 0.0;
}

__global__ void __launch_bounds__(256) pair_lane_kernel(const PairArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < A.n;
    uint64_t lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
    if (live) { pair_range(A.o1, i, A.total1, lo1, hi1); pair_range(A.o2, i, A.total2, lo2, hi2); }
    const uint64_t n1 = hi1 - lo1, n2 = hi2 - lo2;
    unsigned long long cells = (n1 && n2) ? ((n1 > 0xffffffffull || n2 > 0xffffffffull) ? ~0ull : n1 * n2) : 0ull;
    const bool big = cells > RH_PAIR_LANE_BUDGET;
    if (live && !big) {
        const uint32_t la = A.len1[i], lb = A.len2[i];
        PairState st;
        ps_clear(st);
        if (!A.fresh) ps_from_record(st, A.pairs[i]);
        for (uint64_t x = lo1; cells && x < hi1; ++x) {
            const uint4 a = A.h1[x];
            for (uint64_t y = lo2; y < hi2; ++y) pair_cell(st, a, A.h2[y], la, lb, A);
        }
        real_hip_pair r;
        ps_to_record(st, pair_eps(A, la, lb), r);
        A.pairs[i] = r;
    }
    // hand-over list (one atomic per wave) and statistics (one stripe per block)
    const unsigned long long mask = __ballot(live && big);
    const uint32_t lane = threadIdx.x & 63u;
    if (mask) {
        unsigned long long base = 0;
        const int leader = __ffsll((long long)mask) - 1;
        if ((int)lane == leader) base = atomicAdd(A.list_count, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader);
        if (live && big) A.list[base + __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
    for (int d = 32; d; d >>= 1) cells += __shfl_xor(cells, d);
    if (lane == 0) {
        unsigned long long *s = A.stats + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16;
        if (cells) atomicAdd(s, cells);
        if (mask) atomicAdd(s + 1, (unsigned long long)__popcll(mask));
    }
}

__global__ void __launch_bounds__(256) pair_wave_kernel(const PairArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long count = *A.list_count;
    for (uint64_t w = wave; w < count; w += n_waves) {
        const uint64_t i = A.list[w];
        uint64_t lo1, hi1, lo2, hi2;
        pair_range(A.o1, i, A.total1, lo1, hi1);
        pair_range(A.o2, i, A.total2, lo2, hi2);
        const uint32_t la = A.len1[i], lb = A.len2[i];
        PairState st;
        ps_clear(st);
        if (hi2 - lo2 >= hi1 - lo1) { // lanes over the longer list
            for (uint64_t x = lo1; x < hi1; ++x) {
                const uint4 a = A.h1[x];
                for (uint64_t y = lo2 + lane; y < hi2; y += 64) pair_cell(st, a, A.h2[y], la, lb, A);
            }
        } else {
            for (uint64_t y = lo2; y < hi2; ++y) {
                const uint4 b = A.h2[y];
                for (uint64_t x = lo1 + lane; x < hi1; x += 64) pair_cell(st, A.h1[x], b, la, lb, A);
            }
        }
        for (int d = 32; d; d >>= 1) { // butterfly: every lane ends with the wave's state
            PairState o;
            o.best = __shfl_xor(st.best, d); o.second = __shfl_xor(st.second, d);
            o.lhi = __shfl_xor((unsigned long long)st.lhi, d); o.llo = __shfl_xor((unsigned long long)st.llo, d);
            o.s1 = __shfl_xor(st.s1, d); o.s2 = __shfl_xor(st.s2, d); o.k = __shfl_xor(st.k, d);
            ps_merge(st, o);
        }
        if (lane == 0) {
            if (!A.fresh) { PairState in; ps_from_record(in, A.pairs[i]); ps_merge(st, in); }
            real_hip_pair r;
            ps_to_record(st, pair_eps(A, la, lb), r);
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
int rh_launch_pair(real_hip_ctx *ctx, const real_hip_pair_params &pp, const real_hip_hit *d_h1, const uint64_t *d_o1, const uint32_t *d_len1,
                   uint64_t total1, const real_hip_hit *d_h2, const uint64_t *d_o2, const uint32_t *d_len2, uint64_t total2, uint64_t n,
                   uint32_t fileid, int fresh, real_hip_pair *d_pairs)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    int rc;
    if (!ctx->pair_stats.p) {
        if ((rc = rh_reserve(ctx, ctx->pair_stats, (size_t)RH_PAIR_STRIPES * 16 * 8))) return rc;
        RH_HIP(ctx, hipMemsetAsync(ctx->pair_stats.p, 0, (size_t)RH_PAIR_STRIPES * 16 * 8, ctx->stream));
    }
    if ((rc = rh_reserve(ctx, ctx->pair_list, n * 4 + 8))) return rc;
    PairArgs A;
    A.h1 = (const uint4 *)d_h1; A.h2 = (const uint4 *)d_h2; A.o1 = d_o1; A.o2 = d_o2; A.len1 = d_len1; A.len2 = d_len2;
    A.n = n; A.total1 = total1; A.total2 = total2; A.pairs = d_pairs;
    A.list_count = (unsigned long long *)ctx->pair_list.p; A.list = (uint32_t *)ctx->pair_list.p + 2;
    A.stats = (unsigned long long *)ctx->pair_stats.p;
    A.filter_mult = ctx->prm.filter_mult;
    A.fresh = fresh ? 1u : 0u; A.fileid = fileid; A.scores = ctx->prm.scores ? 1u : 0u;
    A.min_insert = pp.min_insert; A.max_insert = pp.max_insert;
    RH_HIP(ctx, hipMemsetAsync(ctx->pair_list.p, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, REAL_HIP_K_PAIR);
    hipLaunchKernelGGL(pair_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    // a fixed grid of waves takes the handed-over fragments in turn (their number stays on the device)
    const uint64_t blocks = (n + 3) / 4 < 2048 ? (n + 3) / 4 : 2048;
    rh_time_begin(ctx, ctx->stream, REAL_HIP_K_PAIR_WAVE);
    hipLaunchKernelGGL(pair_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->pair_count += n;
    return REAL_HIP_OK;
}

int rh_pair_stats(real_hip_ctx *ctx, real_hip_pair_stats *out, int reset)
{
    uint64_t h[2] = {0, 0};
    if (ctx->pair_stats.p) {
        std::vector<uint64_t> all((size_t)RH_PAIR_STRIPES * 16);
        RH_HIP(ctx, hipMemcpyAsync(all.data(), ctx->pair_stats.p, all.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (reset) RH_HIP(ctx, hipMemsetAsync(ctx->pair_stats.p, 0, all.size() * 8, ctx->stream));
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t st = 0; st < RH_PAIR_STRIPES; ++st) { h[0] += all[st * 16]; h[1] += all[st * 16 + 1]; }
    }
    if (out) { out->pairs = ctx->pair_count; out->products = h[0]; out->handed_over = h[1]; }
    if (reset) ctx->pair_count = 0;
    return REAL_HIP_OK;
}
