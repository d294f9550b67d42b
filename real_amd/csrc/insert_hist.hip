// insert_hist.hip -- the histogram of the Unique fragments' outer distances, computed where the pair records live
// (include/real_hip.h, "insert sizes").
//
// One grid-stride kernel.  A lane reads of a 40-byte record the two positions (8 bytes at offset 16) and the tail word with
// inverted1 and state (8 bytes at offset 32; final_record.h names its fields), and of the lengths the reverse mate's; the two
// FP64 values are not loaded.
// Each block keeps a private histogram of 32-bit counts in LDS and flushes its non-zero bins with 64-bit global atomic adds
// at the end: insert sizes sit on a few hundred values, and one global atomic per record onto them would run at the
// contention rate of those few lines, not at the rate of the memory.
//
// The same concentration makes lanes of a wave meet in one LDS word.  Measured (DESIGN.md 7a, 25 M records): with ALL records
// in one bin the kernel takes 0.98 of its time on the workload's distribution, whether the block keeps 16, 8 or 1 copies of
// its histogram -- the LDS adds hide behind the record loads.  So there is one copy and no reduction inside the wave.  Nor
// does a second instance with half the LDS (four blocks of 512 lanes per CU instead of two) gain anything: 0.222 against
// 0.214 ms.  One kernel with room for REAL_HIP_INSERT_HIST_MAX_BINS counts: 64 KiB, two blocks per CU (0.207 ms).
//
// Counts are integers: nothing depends on the order of the records, the lanes or the blocks.  No scratch memory; plain C++
// and vector stores.
#include "real_hip_ctx.h"
#include "pair_state.h"

#define RH_IH_BLOCK 512u
#define RH_IH_UNROLL 4u /* records a lane has in flight */

struct InsertArgs {
    const uint2 *rec;              // real_hip_pair records as five 8-byte words: word 2 = pos1, pos2; word 4 = the tail (final_record.h)
    const uint32_t *len[2];
    uint64_t n;
    unsigned long long *hist;      // n_bins counts, added to
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] counted, [1] overflow, [2] invalid
    uint32_t n_bins;               // <= REAL_HIP_INSERT_HIST_MAX_BINS
};

__global__ void __launch_bounds__(RH_IH_BLOCK) insert_hist_kernel(const InsertArgs A)
{
    __shared__ uint32_t bins[REAL_HIP_INSERT_HIST_MAX_BINS];
    for (uint32_t w = threadIdx.x; w < A.n_bins; w += RH_IH_BLOCK) bins[w] = 0;
    __syncthreads();
    const uint32_t last = A.n_bins - 1;
    uint32_t counted = 0, over = 0, invalid = 0; // (a lane sees fewer than 2^32 records: n is below 2^32)
    const uint64_t stride = (uint64_t)gridDim.x * RH_IH_BLOCK;
    for (uint64_t base = (uint64_t)blockIdx.x * RH_IH_BLOCK + threadIdx.x; base < A.n; base += stride * RH_IH_UNROLL) {
        uint2 tail[RH_IH_UNROLL], pos[RH_IH_UNROLL];
        uint32_t len_r[RH_IH_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < RH_IH_UNROLL; ++u) {
            const uint64_t i = base + u * stride;
            tail[u] = make_uint2(0, 0); pos[u] = make_uint2(0, 0); len_r[u] = 0;
            if (i < A.n) {
                tail[u] = A.rec[i * 5 + 4];
                pos[u] = A.rec[i * 5 + 2];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < RH_IH_UNROLL; ++u) { // (state 0 of the lanes beyond the end: NoMatch)
            const uint64_t i = base + u * stride;
            const bool unique = rh_pair_state(tail[u].y) == REAL_HIP_PAIR_UNIQUE;
            const bool fwd1 = !rh_pair_inverted1(tail[u].y); // the forward mate is mate 1 iff inverted1 == 0: the reverse one is then mate 2
            if (unique) len_r[u] = (fwd1 ? A.len[1] : A.len[0])[i];
        }
#pragma unroll
        for (uint32_t u = 0; u < RH_IH_UNROLL; ++u) {
            if (rh_pair_state(tail[u].y) != REAL_HIP_PAIR_UNIQUE) continue;
            const bool fwd1 = !rh_pair_inverted1(tail[u].y);
            const uint64_t fp = fwd1 ? pos[u].x : pos[u].y, rp = fwd1 ? pos[u].y : pos[u].x;
            if (fp > rp || rp + len_r[u] < fp) { ++invalid; continue; }
            const uint64_t outer = pair_outer(fp, rp, len_r[u]);
            const uint32_t bin = outer < last ? (uint32_t)outer : last;
            atomicAdd(&bins[bin], 1u);
            ++counted;
            over += outer >= last;
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < A.n_bins; b += RH_IH_BLOCK) // the flush
        if (bins[b]) atomicAdd(A.hist + b, (unsigned long long)bins[b]);
    uint32_t s[3] = {counted, over, invalid}; // (32-bit sums: the lanes of a wave together see at most the n < 2^32 records of the call)
    rh_stats_add(A.stats, s);
}

int rh_launch_insert_hist(real_hip_ctx *ctx, const real_hip_pair *d_pairs, const uint32_t *d_len1, const uint32_t *d_len2, uint64_t n,
                          uint32_t n_bins, uint64_t *d_hist)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    if (n_bins < 2 || n_bins > REAL_HIP_INSERT_HIST_MAX_BINS) return rh_fail(ctx, REAL_HIP_E_INVALID, "n_bins out of range", hipSuccess);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->insert.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    InsertArgs A;
    A.rec = (const uint2 *)d_pairs; A.len[0] = d_len1; A.len[1] = d_len2;
    A.n = n; A.hist = (unsigned long long *)d_hist; A.stats = (unsigned long long *)ctx->insert.stage.stats.p;
    A.n_bins = n_bins;
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n_cu < 1) n_cu = 256;
    const uint64_t resident = (uint64_t)n_cu * 2, need = (n + RH_IH_BLOCK - 1) / RH_IH_BLOCK;
    const unsigned blocks = (unsigned)(need < resident ? need : resident);
    rh_time_begin(ctx, ctx->stream, ctx->insert.stage);
    hipLaunchKernelGGL(insert_hist_kernel, dim3(blocks), dim3(RH_IH_BLOCK), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->insert.stage.items += n;
    ctx->insert.stage.launches += 1;
    return REAL_HIP_OK;
}

int rh_insert_stats(real_hip_ctx *ctx, real_hip_insert_stats *out, int reset)
{
    uint64_t h[3];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->insert.stage, RH_PAIR_STRIPES, 3, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->records = was.items; out->counted = h[0]; out->overflow = h[1]; out->invalid = h[2];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
