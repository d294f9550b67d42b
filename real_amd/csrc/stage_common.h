// stage_common.h -- what the kernels and launchers of the stages behind the matcher share: the striped
// statistics line and the wave's add to it, the device view of the resident text, the emit slot of a flagged lane in a
// count / scan / emit pass; and, through final_record.h, the decoder of the records these stages consume.
#pragma once
#include "real_hip_ctx.h"
#include "final_record.h"

#define RH_PAIR_STRIPES 256u      /* the statistics are striped over this many 128-byte lines (see RH_CSTRIPES) */

// The end of a kernel that counts: every lane of the wave calls it with its N counters; the wave's sums are added to words
// 0 .. N-1 of the block's stripe of `stats`, one atomic per non-zero sum, from lane 0.  32-bit sums: the caller says why a
// wave's stay below 2^32.  s[] is a register array: every index is a constant once the loops are unrolled.
template <int N>
static __device__ __forceinline__ void rh_stats_add(unsigned long long *stats, uint32_t (&s)[N])
{
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int d = 32; d; d >>= 1) s[k] += (uint32_t)__shfl_xor((int)s[k], d);
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long *line = stats + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16;
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (s[k]) atomicAdd(line + k, (unsigned long long)s[k]);
    }
}

// Count / scan / emit over one lane per item, blocks of 64 * WAVES lanes: `mask` is the wave's ballot of the flagged lanes,
// wave_cnt[] the block's LDS.  Every lane of the block calls it (it holds the barrier).
// the count pass: the block's number of flagged lanes, valid in thread 0
template <uint32_t WAVES>
static __device__ __forceinline__ uint32_t rh_block_count(unsigned long long mask, uint32_t (&wave_cnt)[WAVES])
{
    if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t c = 0;
    if (threadIdx.x == 0)
        for (uint32_t k = 0; k < WAVES; ++k) c += wave_cnt[k];
    return c;
}
// the emit pass: the slot of a flagged lane behind the block's offset -- the waves in front of its own, then the flagged lanes
// below it
template <uint32_t WAVES>
static __device__ __forceinline__ uint64_t rh_emit_slot(unsigned long long mask, uint64_t block_off, uint32_t (&wave_cnt)[WAVES])
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint64_t slot = block_off;
    for (uint32_t k = 0; k < wave; ++k) slot += wave_cnt[k];
    return slot + __popcll(mask & ((1ull << lane) - 1ull));
}

// the device view of the resident text, as file `fileid`
static inline DevText rh_dev_text(const real_hip_ctx *ctx, uint32_t fileid)
{
    DevText t;
    t.text = (const uint64_t *)ctx->text.p; t.wild = (const uint64_t *)ctx->wild.p; t.frag_start = (const uint64_t *)ctx->frag.p;
    t.n = ctx->n_bases; t.n_frag = ctx->n_frag; t.has_wild = ctx->n_wild ? 1 : 0; t.fileid = fileid;
    return t;
}
