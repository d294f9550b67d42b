// all_order.hip -- the matchAll post-pass (the `order` leg): the raw hit records of a batch put into the per-read order of
// unifyMatches (matchAllImplementation.cpp:122-161).  Nothing of the index is touched here.
#include "real_hip_ctx.h"
#include "rocprim_call.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

// ---------------------------------------------------------------------------
// matchAll post-pass: order the raw hit records per read as unifyMatches does
// (operator<, matchAllImplementation.cpp:122-136: k, pos, file, frag, score, inverted;
// file is constant inside a call and frag is a monotone function of pos).
// The matcher appends hits in wave order and counts them per read; a read has a handful of
// hits (the reads that have more, on both sides of ALL_SMALL and ALL_HUGE: tests/test_gpu_all_order.py), so: offsets = exclusive scan of the counts, scatter every raw record into its read's
// segment, rank the records of a segment against each other (one thread per read; one
// workgroup per read with more than ALL_SMALL hits).  No global sort.  A read with one hit -- most
// of those that have any -- needs neither: its record goes straight from the raw list to its place.
// ---------------------------------------------------------------------------
#define ALL_SMALL 32u

struct U32ToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};

__device__ __forceinline__ bool hit_less(const uint4 &x, const uint4 &y)
{
    const uint32_t kx = x.w & 0xffu, ky = y.w & 0xffu;
    if (kx != ky) return kx < ky;
    if (x.y != y.y) return x.y < y.y;
    const float sx = __uint_as_float(x.z), sy = __uint_as_float(y.z);
    if (sx != sy) return sx < sy;
    return ((x.w >> 8) & 1u) < ((y.w >> 8) & 1u);
}
__device__ __forceinline__ real_hip_hit hit_record(const uint4 &h)
{
    real_hip_hit o;
    o.read = h.x; o.pos = h.y; o.score = __uint_as_float(h.z);
    o.frag = (uint16_t)(h.w >> 16); o.k = (uint8_t)(h.w & 0xff); o.inverted = (uint8_t)((h.w >> 8) & 1);
    return o;
}

// most reads that have a hit have exactly one: its record goes straight to its place.  The hits of the others are
// collected in their segment (cursor[] counts them; it is all zero between two calls) and the read is listed once.
__global__ void all_scatter_kernel(const uint4 *__restrict__ raw, uint64_t n, const uint64_t *__restrict__ off, const uint32_t *__restrict__ cnt,
                                   uint32_t *__restrict__ cursor, uint4 *__restrict__ seg, real_hip_hit *__restrict__ out,
                                   uint32_t *__restrict__ multi_list, unsigned long long *multi_count)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 h = raw[i];
    const uint64_t o = off[h.x];
    if (cnt[h.x] == 1u) { out[o] = hit_record(h); return; }
    const uint32_t slot = atomicAdd(&cursor[h.x], 1u);
    seg[o + slot] = h;
    if (slot == 0) multi_list[atomicAdd(multi_count, 1ull)] = h.x;
}

// (The quadratic stable rank -- record i goes to the place of its rank, the records less than it plus the equal ones in front of
// it -- stands in both rank kernels on purpose: as one __device__ function it cost all_rank_kernel three VGPRs and both kernels
// six or seven SGPRs, and the order leg of C3 did not stay inside the parent's range)
__global__ void all_rank_kernel(const uint4 *__restrict__ seg, const uint64_t *__restrict__ off, const uint32_t *__restrict__ multi_list,
                                const unsigned long long *__restrict__ multi_count, uint32_t *__restrict__ cursor,
                                real_hip_hit *__restrict__ out, uint32_t *__restrict__ big_list, unsigned long long *big_count)
{
    const uint64_t nm = *multi_count;
    for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < nm; m += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = multi_list[m];
        cursor[r] = 0; // (for the next call)
        const uint64_t o = off[r];
        const uint32_t c = (uint32_t)(off[r + 1] - o);
        if (c > ALL_SMALL) { big_list[atomicAdd(big_count, 1ull)] = (uint32_t)r; continue; }
        for (uint32_t i = 0; i < c; ++i) {
            const uint4 h = seg[o + i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < c; ++j) {
                const uint4 g = seg[o + j];
                rank += (hit_less(g, h) || (j < i && !hit_less(h, g))) ? 1u : 0u;
            }
            out[o + rank] = hit_record(h);
        }
    }
}

// reads with many hits (repeats): one workgroup per read.  Up to ALL_HUGE hits the same quadratic ranking; beyond
// (a read on a low-complexity locus has 10^5 hits) a stable LSD radix sort of the segment by (k, pos) -- ten passes of
// four bits between the segment and the same range of the raw array, which is free once the records are scattered --
// and a look at the neighbours for the one tie (k, pos) leaves open: the same position on both strands.
#define ALL_HUGE 1024u
__device__ __forceinline__ uint64_t hit_key40(const uint4 &h) { return ((uint64_t)(h.w & 0xffu) << 32) | (uint64_t)h.y; }

__global__ __launch_bounds__(256) void all_rank_big_kernel(uint4 *__restrict__ seg, uint4 *__restrict__ scratch, const uint64_t *__restrict__ off,
                                                           const uint32_t *__restrict__ big_list, const unsigned long long *__restrict__ big_count,
                                                           real_hip_hit *__restrict__ out)
{
    __shared__ uint32_t hist[16 * 256];
    __shared__ uint32_t tot[16];
    const uint32_t t = threadIdx.x;
    const uint64_t nb = *big_count;
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint64_t r = big_list[b], o = off[r];
        const uint32_t c = (uint32_t)(off[r + 1] - o);
        if (c <= ALL_HUGE) {
            for (uint32_t i = t; i < c; i += blockDim.x) {
                const uint4 h = seg[o + i];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < c; ++j) {
                    const uint4 g = seg[o + j];
                    rank += (hit_less(g, h) || (j < i && !hit_less(h, g))) ? 1u : 0u;
                }
                out[o + rank] = hit_record(h);
            }
            continue;
        }
        uint4 *A = seg + o, *B = scratch + o;
        const uint32_t chunk = (c + 255u) / 256u, lo = min(c, t * chunk), hi = min(c, lo + chunk);
        for (uint32_t pass = 0; pass < 10; ++pass) { // (every thread of the workgroup makes the same trips)
            const uint32_t sh = 4 * pass;
            uint32_t cnt[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) cnt[d] = 0;
            for (uint32_t i = lo; i < hi; ++i) {
                const uint32_t dg = (uint32_t)(hit_key40(A[i]) >> sh) & 15u;
#pragma unroll
                for (int d = 0; d < 16; ++d) cnt[d] += (dg == (uint32_t)d) ? 1u : 0u;
            }
#pragma unroll
            for (int d = 0; d < 16; ++d) hist[d * 256 + t] = cnt[d];
            __syncthreads();
            if (t < 16) { // exclusive scan of digit t's counts over the threads (= over the chunks, in order: stable)
                uint32_t run = 0;
                for (uint32_t j = 0; j < 256; ++j) { const uint32_t v = hist[t * 256 + j]; hist[t * 256 + j] = run; run += v; }
                tot[t] = run;
            }
            __syncthreads();
            if (t == 0) {
                uint32_t run = 0;
                for (int d = 0; d < 16; ++d) { const uint32_t v = tot[d]; tot[d] = run; run += v; }
            }
            __syncthreads();
#pragma unroll
            for (int d = 0; d < 16; ++d) cnt[d] = tot[d] + hist[d * 256 + t];
            for (uint32_t i = lo; i < hi; ++i) {
                const uint4 h = A[i];
                const uint32_t dg = (uint32_t)(hit_key40(h) >> sh) & 15u;
                uint32_t dst = 0;
#pragma unroll
                for (int d = 0; d < 16; ++d) if (dg == (uint32_t)d) dst = cnt[d]++;
                B[dst] = h;
            }
            __threadfence_block();
            __syncthreads();
            uint4 *x = A; A = B; B = x;
        }
        // (ten passes: the sorted records are in the segment again)
        for (uint32_t i = t; i < c; i += blockDim.x) {
            const uint4 h = A[i];
            uint32_t rank = i;
            if (i + 1 < c) { const uint4 g = A[i + 1]; if (hit_key40(g) == hit_key40(h) && hit_less(g, h)) rank = i + 1; }
            if (i > 0) { const uint4 g = A[i - 1]; if (hit_key40(g) == hit_key40(h) && hit_less(h, g)) rank = i - 1; }
            out[o + rank] = hit_record(h);
        }
        __syncthreads();
    }
}

int rh_all_finish(real_hip_ctx *ctx, uint64_t n_raw, uint64_t n_reads, real_hip_hit *d_out, uint64_t *d_hit_offsets)
{
    RhTimer tm(ctx, REAL_HIP_K_ALL_SORT);
    int rc;
    if (!n_reads) {
        if (d_hit_offsets) RH_HIP(ctx, hipMemsetAsync(d_hit_offsets, 0, 8, ctx->stream));
        return REAL_HIP_OK;
    }
    uint64_t *off = d_hit_offsets;
    if (!off) {
        if ((rc = rh_reserve(ctx, ctx->hit_off, (n_reads + 1) * 8))) return rc;
        off = (uint64_t *)ctx->hit_off.p;
    }
    uint32_t *cnt = (uint32_t *)ctx->hit_cnt.p; // written by the matcher for every read of the batch
    RH_HIP(ctx, hipMemsetAsync(cnt + n_reads, 0, 4, ctx->stream));
    {
        rocprim::transform_iterator<const uint32_t *, U32ToU64, uint64_t> in((const uint32_t *)cnt, U32ToU64());
        auto scan = [&](void *tmp, size_t &bytes) { return rocprim::exclusive_scan(tmp, bytes, in, off, (uint64_t)0, (size_t)(n_reads + 1), rocprim::plus<uint64_t>(), ctx->stream); };
        if ((rc = rh_prim_run(ctx, ctx->sort_tmp, scan, "hit offsets scan"))) return rc;
    }
    if (n_raw) {
        if ((rc = rh_reserve(ctx, ctx->keys_a, n_raw * sizeof(uint4)))) return rc;       // the per-read segments
        if (n_reads * 4 > ctx->all_cursor.cap) {                                          // scatter cursors: zero between two calls
            if ((rc = rh_reserve(ctx, ctx->all_cursor, n_reads * 4))) return rc;
            RH_HIP(ctx, hipMemsetAsync(ctx->all_cursor.p, 0, ctx->all_cursor.cap, ctx->stream));
        }
        if ((rc = rh_reserve(ctx, ctx->big_list, n_reads * 8 + 16))) return rc;          // reads with more than one hit; with more than ALL_SMALL
        uint32_t *multi_list = (uint32_t *)ctx->big_list.p, *big_list = multi_list + n_reads;
        unsigned long long *counts = (unsigned long long *)((uint8_t *)ctx->big_list.p + n_reads * 8);
        RH_HIP(ctx, hipMemsetAsync(counts, 0, 16, ctx->stream));
        const uint4 *raw = (const uint4 *)ctx->raw.p;
        uint4 *seg = (uint4 *)ctx->keys_a.p;
        rh_launch_each(all_scatter_kernel, n_raw, ctx->stream, raw, n_raw, off, cnt, (uint32_t *)ctx->all_cursor.p, seg, d_out, multi_list, counts);
        hipLaunchKernelGGL(all_rank_kernel, dim3(2048), dim3(256), 0, ctx->stream, (const uint4 *)seg, (const uint64_t *)off,
                           (const uint32_t *)multi_list, (const unsigned long long *)counts, (uint32_t *)ctx->all_cursor.p, d_out, big_list, counts + 1);
        hipLaunchKernelGGL(all_rank_big_kernel, dim3(1024), dim3(256), 0, ctx->stream, seg, (uint4 *)ctx->raw.p, (const uint64_t *)off,
                           (const uint32_t *)big_list, (const unsigned long long *)(counts + 1), d_out);
    }
    RH_HIP(ctx, hipGetLastError());
    return REAL_HIP_OK;
}
