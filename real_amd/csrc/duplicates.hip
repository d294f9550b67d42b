// duplicates.hip -- duplicate marking: the placed reads (fragments) grouped by their 5' ends, the copy of the highest quality sum
// kept, every other one marked (include/real_hip.h, "duplicates").
//
// Five kernels and rocPRIM's stable radix sort:
//   read_summary_kernel   one lane per read walks the read's quality bytes in place, an aligned 16-byte chunk per load (rows at
//                         any byte address, by the rule of read_walk.h's DwordRow) and writes {len, qsum}; a read beyond
//                         REAL_HIP_MAX_PATL is summed by the whole wave it falls into (ballot, then 64 chunks per step) -- no
//                         list, no second launch.
//   dup_key_kernel        one lane per info record: key = fileid:6 | reverse:1 | END5:36 | (2^20 - 1 - qsum):20, value = index;
//                         an unplaced record gets the all-ones sentinel (bit 63: no placed key has it).
//   dup_gapped_key_kernel the same key for a read with an info word and a gap record: the info word's placement, else the Unique
//                         gap record's (END5 over the span len + gap); only an unplaced lane loads its gap record.
//   dup_pair_key_kernel   one lane per pair record: low word END:33 | (2^21 - 1 - qsum1 - qsum2):21, high word
//                         unplaced:1 | fileid:8 | inverted1:1 | START:32; two stable passes, low word first (the high words are
//                         gathered into the first pass' order by dup_gather_kernel in between).
//   dup_mark_kernel       one lane per sorted place: a place whose group part equals its predecessor's is a duplicate.
// The tie-breaker sits inside the key: the sort is stable and the values start as 0 .. n-1, so inside a group the largest qsum
// comes first and among equal qsum the smallest index.  The work per element is constant, whatever the group sizes; nothing
// is hashed.  dup[] is cleared beforehand (the unplaced records), the marks are byte stores.  The key kernels read their
// records through final_record.h's decoders; placed and groups go to the striped line with stage_common.h's rh_stats_add.
// No LDS of our own, no scratch memory, plain C++.
#include "real_hip_ctx.h"
#include "read_walk.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>

#define RH_DUP_BLOCK 256u

// ---- the key budget ---------------------------------------------------------------------------------------------
#define RH_DUP_Q_BITS 20u    /* qsum of one read */
#define RH_DUP_E5_BITS 36u   /* END5 = pos + len - 1 */
#define RH_DUP_FI_BITS 6u    /* the info word's file id */
#define RH_DUP_PQ_BITS 21u   /* qsum1 + qsum2 */
#define RH_DUP_PE_BITS 33u   /* END = r.pos + len_r - 1 */
#define RH_DUP_PHI_BITS 42u  /* START:32, inverted1:1, fileid:8, unplaced:1 */
static_assert((uint64_t)REAL_HIP_MAX_PATL_LONG * 63u < (1ull << RH_DUP_Q_BITS), "qsum of the longest read in 20 bits");
static_assert(2ull * REAL_HIP_MAX_PATL_LONG * 63u < (1ull << RH_DUP_PQ_BITS), "qsum1 + qsum2 in 21 bits");
static_assert(POS_MASK + REAL_HIP_MAX_PATL_LONG - 1 < (1ull << RH_DUP_E5_BITS), "END5 of a 35-bit position in 36 bits");
static_assert(0xffffffffull + REAL_HIP_MAX_PATL_LONG - 1 < (1ull << RH_DUP_PE_BITS), "END of a 32-bit position in 33 bits");
static_assert(RH_DUP_FI_BITS + 1 + RH_DUP_E5_BITS + RH_DUP_Q_BITS <= 63, "the single-end key leaves bit 63 to the sentinel");
static_assert(RH_DUP_PE_BITS + RH_DUP_PQ_BITS <= 64 && RH_DUP_PHI_BITS <= 64, "the two words of the paired key");
static_assert(FI_SHIFT == 35 && ER_SHIFT - FI_SHIFT == RH_DUP_FI_BITS, "the file id of an info word has six bits");
#define RH_DUP_SENTINEL (~0ull)

// ---- read summaries -----------------------------------------------------------------------------------------------
struct SummaryArgs {
    DevBatch b;        // qual, off, upatl, n_reads (the bases are not read)
    uint32_t min_qual;
    uint2 *out;        // real_hip_read_sum as one 8-byte store: x = len, y = qsum
};

// The quality bytes of a read in place, an aligned 16-byte chunk per load: 100 qualities are seven loads of a lane, where a dword
// per load (read_walk.h's DwordRow, what the first build walked with) is twenty-five -- a wave's load touches 64 lines either
// way, and the kernel ran at the rate of its load instructions, not of the memory.  The rule is DwordRow's:
// never a chunk without a byte of the row in it (an aligned chunk does not cross a page, so nothing outside the pages of the
// caller's allocation is touched); the bytes of a chunk in front of the row and behind it are masked by position.
// the qualities >= mq among bytes [lo, hi) of the chunk v
static __device__ __forceinline__ uint32_t dup_qsum_chunk(const uint4 v, uint32_t lo, uint32_t hi, uint32_t mq)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t q = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        if (k >= lo && k < hi && q >= mq) s += q;
    }
    return s;
}
// chunk number c (0 = the one that holds the row's first byte) of the row of L bytes at address a; 0 behind the row's end
static __device__ __forceinline__ uint32_t dup_qsum_at(uintptr_t a, uint32_t L, uint32_t c, uint32_t mq)
{
    const uintptr_t p = (a & ~(uintptr_t)15) + 16u * (uintptr_t)c, end = a + L;
    if (p >= end) return 0;
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    return dup_qsum_chunk(v, p < a ? (uint32_t)(a - p) : 0u, end - p < 16 ? (uint32_t)(end - p) : 16u, mq);
}

__global__ void __launch_bounds__(RH_DUP_BLOCK) read_summary_kernel(const SummaryArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_DUP_BLOCK + threadIdx.x;
    const bool have = i < A.b.n_reads;
    uint64_t start = 0;
    uint32_t L = 0;
    if (have) {
        L = read_extent(A.b, i, start);
        if (L == 0xffffffffu) L = 0; // (offsets that run backwards or span more than the longest read: an empty summary)
    }
    const bool wave_read = have && A.b.qual && L > REAL_HIP_MAX_PATL;
    if (have && !wave_read) {
        uint32_t s = 0;
        if (!A.b.qual) {
            s = 30u >= A.min_qual ? 30u * L : 0u;
        } else if (L) {
            const uintptr_t a = (uintptr_t)(A.b.qual + start);
            const uint32_t chunks = (uint32_t)(((a & 15u) + L + 15u) >> 4);
            for (uint32_t c = 0; c < chunks; ++c) s += dup_qsum_at(a, L, c, A.min_qual);
        }
        A.out[i] = make_uint2(L, s);
    }
    // the long reads of this wave's 64, one after the other, by all lanes
    unsigned long long m = __ballot(wave_read);
    const uint32_t lane = threadIdx.x & 63u;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint32_t Ls = (uint32_t)__shfl((int)L, src);
        const uint64_t ss = ((uint64_t)(uint32_t)__shfl((int)(start >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)start, src);
        const uintptr_t a = (uintptr_t)(A.b.qual + ss);
        const uint32_t chunks = (uint32_t)(((a & 15u) + Ls + 15u) >> 4);
        uint32_t s = 0;
        for (uint32_t c = lane; c < chunks; c += 64) s += dup_qsum_at(a, Ls, c, A.min_qual);
        for (int d = 32; d; d >>= 1) s += (uint32_t)__shfl_xor((int)s, d);
        if ((int)lane == src) A.out[i] = make_uint2(Ls, s);
    }
}

// ---- keys ---------------------------------------------------------------------------------------------------------
struct DupArgs {
    const uint64_t *info;          // single-end records, or
    const uint2 *pairs;            // real_hip_pair records as five 8-byte words (final_record.h)
    const uint2 *sum[2];           // real_hip_read_sum {len, qsum} of the reads / of mate 1 and mate 2
    uint64_t n;
    uint64_t *key;                 // single-end key / low word of the paired key: what the sort takes
    uint64_t *lo, *hi;             // pairs: the low word once more and the high word, both staying in record order
    uint32_t *val;                 // the record's index
    const uint4 *gaps;             // dup_gapped_key_kernel: real_hip_gap_place records beside the info words, a uint4 each
};

__global__ void __launch_bounds__(RH_DUP_BLOCK) dup_key_kernel(const DupArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_DUP_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const RhPlace r = rh_place_info(A.info[i]);
    uint64_t key = RH_DUP_SENTINEL;
    if (r.place) {
        const uint2 s = A.sum[0][i];
        const uint64_t end5 = (r.inv ? r.pos + s.x - 1 : r.pos) & ((1ull << RH_DUP_E5_BITS) - 1);
        const uint32_t qmax = (1u << RH_DUP_Q_BITS) - 1;
        key = ((((uint64_t)r.file << 1 | (r.inv ? 1u : 0u)) << RH_DUP_E5_BITS | end5) << RH_DUP_Q_BITS) | (qmax - min(s.y, qmax));
    }
    A.key[i] = key;
    A.val[i] = (uint32_t)i;
}

// The joint key of a read that has an info word and a gap record: the info word's placement where it has one --
// dup_key_kernel's key, bit for bit --, else the gap record's where that is Unique: END5 = p forward, p + len + g - 1 reverse
// (len + g is the span on the text), in 64 bits.  Only a lane whose read the matcher did not place loads the gap record, as
// one 16-byte load; one key space for both kinds, so that the copies of a molecule meet in one group whichever way they were placed.
__global__ void __launch_bounds__(RH_DUP_BLOCK) dup_gapped_key_kernel(const DupArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_DUP_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const RhPlace r = rh_place_info(A.info[i]);
    bool place = r.place, inv = r.inv;
    uint32_t file = r.file;
    uint64_t pos = r.pos;
    int64_t g = 0;
    if (!place) {
        const uint4 w = A.gaps[i];
        const RhGapRecord q = rh_place_gap(w.x, w.y, w.z, w.w);
        place = q.state == REAL_HIP_PAIR_UNIQUE; inv = q.inv != 0; file = q.file & ((1u << RH_DUP_FI_BITS) - 1); pos = q.p; g = q.g;
    }
    uint64_t key = RH_DUP_SENTINEL;
    if (place) {
        const uint2 s = A.sum[0][i];
        const uint64_t end5 = (inv ? pos + s.x + (uint64_t)g - 1 : pos) & ((1ull << RH_DUP_E5_BITS) - 1);
        const uint32_t qmax = (1u << RH_DUP_Q_BITS) - 1;
        key = ((((uint64_t)file << 1 | (inv ? 1u : 0u)) << RH_DUP_E5_BITS | end5) << RH_DUP_Q_BITS) | (qmax - min(s.y, qmax));
    }
    A.key[i] = key;
    A.val[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(RH_DUP_BLOCK) dup_pair_key_kernel(const DupArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_DUP_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const uint2 tail = A.pairs[i * 5 + 4];
    uint64_t lo = RH_DUP_SENTINEL >> (64 - RH_DUP_PE_BITS - RH_DUP_PQ_BITS), hi = 1ull << (RH_DUP_PHI_BITS - 1);
    if (rh_pair_state(tail.y) == REAL_HIP_PAIR_UNIQUE) {
        const uint2 pos = A.pairs[i * 5 + 2];
        const uint2 s1 = A.sum[0][i], s2 = A.sum[1][i];
        const uint32_t inv1 = rh_pair_inverted1(tail.y) ? 1u : 0u; // the forward mate is mate 1 iff inverted1 == 0
        const uint64_t start = inv1 ? pos.y : pos.x;
        const uint64_t end = ((inv1 ? (uint64_t)pos.x + s1.x : (uint64_t)pos.y + s2.x) - 1) & ((1ull << RH_DUP_PE_BITS) - 1);
        const uint32_t q1max = (1u << RH_DUP_Q_BITS) - 1, qmax = (1u << RH_DUP_PQ_BITS) - 1;
        lo = end << RH_DUP_PQ_BITS | (qmax - (min(s1.y, q1max) + min(s2.y, q1max)));
        hi = ((uint64_t)rh_pair_fileid(tail.x) << 1 | inv1) << 32 | start;
    }
    A.key[i] = lo;
    A.lo[i] = lo;
    A.hi[i] = hi;
    A.val[i] = (uint32_t)i;
}

// the high words in the order the first pass left the records in
__global__ void __launch_bounds__(RH_DUP_BLOCK) dup_gather_kernel(const uint64_t *hi, const uint32_t *val, uint64_t n, uint64_t *out)
{
    const uint64_t j = (uint64_t)blockIdx.x * RH_DUP_BLOCK + threadIdx.x;
    if (j < n) out[j] = hi[val[j]];
}

// ---- marks --------------------------------------------------------------------------------------------------------
struct MarkArgs {
    const uint64_t *key;           // sorted: the single-end keys, or the high words of the paired keys
    const uint64_t *lo;            // pairs: the low words in RECORD order (null for single-end)
    const uint32_t *val;           // sorted with the keys
    uint64_t n;
    uint8_t *dup;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] groups
};

template <bool PAIRS>
__global__ void __launch_bounds__(RH_DUP_BLOCK) dup_mark_kernel(const MarkArgs A)
{
    const uint64_t j = (uint64_t)blockIdx.x * RH_DUP_BLOCK + threadIdx.x;
    uint32_t placed = 0, first = 0;
    if (j < A.n) {
        const uint64_t k = A.key[j];
        const bool live = PAIRS ? (k >> (RH_DUP_PHI_BITS - 1)) == 0 : k != RH_DUP_SENTINEL;
        if (live) { // (the unplaced records sort behind the placed ones: a placed record's predecessor is placed)
            const uint32_t idx = A.val[j];
            bool same = false;
            if (j) {
                if (PAIRS) same = A.key[j - 1] == k && (A.lo[A.val[j - 1]] >> RH_DUP_PQ_BITS) == (A.lo[idx] >> RH_DUP_PQ_BITS);
                else same = (A.key[j - 1] >> RH_DUP_Q_BITS) == (k >> RH_DUP_Q_BITS);
            }
            A.dup[idx] = same ? 1 : 0;
            placed = 1; first = same ? 0u : 1u;
        }
    }
    uint32_t s[2] = {placed, first}; // (a wave's sums are at most 64)
    rh_stats_add(A.stats, s);
}

// ---- host side ----------------------------------------------------------------------------------------------------
static inline dim3 dup_grid(uint64_t n) { return dim3((unsigned)((n + RH_DUP_BLOCK - 1) / RH_DUP_BLOCK)); }

// out[i] = {len, qsum} of read i of b (device arrays: qual -- nullable --, off -- nullable --, upatl); asynchronous
int rh_launch_read_summary(real_hip_ctx *ctx, const DevBatch &b, uint32_t min_qual, real_hip_read_sum *d_out)
{
    static_assert(sizeof(real_hip_read_sum) == 8 && offsetof(real_hip_read_sum, qsum) == 4, "a read summary is one 8-byte store: len, qsum");
    if (!b.n_reads) return REAL_HIP_OK;
    SummaryArgs A;
    memset(&A, 0, sizeof A);
    A.b = b; A.min_qual = min_qual; A.out = (uint2 *)d_out;
    rh_time_begin(ctx, ctx->stream, ctx->dup.stage);
    hipLaunchKernelGGL(read_summary_kernel, dup_grid(b.n_reads), dim3(RH_DUP_BLOCK), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->dup.stage.launches += 1;
    return REAL_HIP_OK;
}

// The tail every marking shares: the buffers, `key_kernel` over K's records (K.n, K.key, K.lo, K.hi and K.val are set here), the
// sort -- pairs: low word, gather, high word -- and the marks into d_dup; asynchronous
static int dup_sort_mark(real_hip_ctx *ctx, DupArgs K, void (*key_kernel)(const DupArgs), bool pairs, uint64_t n, uint8_t *d_dup)
{
    if (!n) return REAL_HIP_OK;
    if (n > (1ull << 32)) return rh_fail(ctx, REAL_HIP_E_INVALID, "duplicates: more than 2^32 records in one call", hipSuccess);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->dup.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = rh_reserve(ctx, ctx->dup.key[k], (size_t)n * 8))) return rc;
        if ((rc = rh_reserve(ctx, ctx->dup.val[k], (size_t)n * 4))) return rc;
    }
    if (pairs && ((rc = rh_reserve(ctx, ctx->dup.hi, (size_t)n * 8)) || (rc = rh_reserve(ctx, ctx->dup.lo, (size_t)n * 8)))) return rc;
    rocprim::double_buffer<uint64_t> keys((uint64_t *)ctx->dup.key[0].p, (uint64_t *)ctx->dup.key[1].p);
    rocprim::double_buffer<uint32_t> vals((uint32_t *)ctx->dup.val[0].p, (uint32_t *)ctx->dup.val[1].p);
    const unsigned bits0 = pairs ? RH_DUP_PE_BITS + RH_DUP_PQ_BITS : 64u; // (single-end: bit 63 is the sentinel's)
    size_t tmp = 0, tmp1 = 0;
    RH_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp, keys, vals, (size_t)n, 0u, bits0, ctx->stream));
    if (pairs) RH_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp1, keys, vals, (size_t)n, 0u, RH_DUP_PHI_BITS, ctx->stream));
    if (tmp1 > tmp) tmp = tmp1;
    if ((rc = rh_reserve(ctx, ctx->sort_tmp, tmp ? tmp : 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(d_dup, 0, (size_t)n, ctx->stream));

    K.n = n; K.key = keys.current(); K.lo = (uint64_t *)ctx->dup.lo.p; K.hi = (uint64_t *)ctx->dup.hi.p; K.val = vals.current();
    const dim3 grid = dup_grid(n), block(RH_DUP_BLOCK);
    uint64_t launches = 0;
    rh_time_begin(ctx, ctx->stream, ctx->dup.stage); // (no return inside the bracket: a failing step is reported behind rh_time_end)
    hipLaunchKernelGGL(key_kernel, grid, block, 0, ctx->stream, K);
    hipError_t e = hipGetLastError();
    ++launches;
    if (e == hipSuccess) { e = rocprim::radix_sort_pairs(ctx->sort_tmp.p, tmp, keys, vals, (size_t)n, 0u, bits0, ctx->stream); ++launches; }
    if (e == hipSuccess && pairs) {
        // the second pass sorts the high words, brought into the first pass' order: the gather writes the buffer the sort has
        // finished with
        uint64_t *lo_sorted = keys.current(), *spare = keys.alternate();
        hipLaunchKernelGGL(dup_gather_kernel, grid, block, 0, ctx->stream, (const uint64_t *)ctx->dup.hi.p, (const uint32_t *)vals.current(), n, spare);
        e = hipGetLastError();
        ++launches;
        if (e == hipSuccess) {
            keys = rocprim::double_buffer<uint64_t>(spare, lo_sorted);
            e = rocprim::radix_sort_pairs(ctx->sort_tmp.p, tmp1, keys, vals, (size_t)n, 0u, RH_DUP_PHI_BITS, ctx->stream);
            ++launches;
        }
    }
    if (e == hipSuccess) {
        MarkArgs M;
        memset(&M, 0, sizeof M);
        M.key = keys.current(); M.lo = pairs ? (const uint64_t *)ctx->dup.lo.p : nullptr; M.val = vals.current();
        M.n = n; M.dup = d_dup; M.stats = (unsigned long long *)ctx->dup.stage.stats.p;
        if (pairs) hipLaunchKernelGGL(dup_mark_kernel<true>, grid, block, 0, ctx->stream, M);
        else hipLaunchKernelGGL(dup_mark_kernel<false>, grid, block, 0, ctx->stream, M);
        e = hipGetLastError();
        ++launches;
    }
    rh_time_end(ctx, ctx->stream);
    ctx->dup.stage.launches += launches;
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "duplicates: key / sort / mark", e);
    ctx->dup.stage.items += n;
    return REAL_HIP_OK;
}

// dup[i] of n records, all arrays on the device: info and sum1 (single-end), or pairs, sum1 and sum2; asynchronous
int rh_launch_mark_duplicates(real_hip_ctx *ctx, const uint64_t *d_info, const real_hip_pair *d_pairs, const real_hip_read_sum *d_sum1,
                              const real_hip_read_sum *d_sum2, uint64_t n, uint8_t *d_dup)
{
    const bool pairs = d_pairs != nullptr;
    DupArgs K;
    memset(&K, 0, sizeof K);
    K.info = d_info; K.pairs = (const uint2 *)d_pairs; K.sum[0] = (const uint2 *)d_sum1; K.sum[1] = (const uint2 *)d_sum2;
    return dup_sort_mark(ctx, K, pairs ? dup_pair_key_kernel : dup_key_kernel, pairs, n, d_dup);
}

// the same over info words AND gap records (dup_gapped_stage.h): one key space, one sort, one marking
int rh_launch_mark_duplicates_gapped(real_hip_ctx *ctx, const uint64_t *d_info, const real_hip_gap_place *d_gaps, const real_hip_read_sum *d_sum,
                                     uint64_t n, uint8_t *d_dup)
{
    DupArgs K;
    memset(&K, 0, sizeof K);
    K.info = d_info; K.gaps = (const uint4 *)d_gaps; K.sum[0] = (const uint2 *)d_sum;
    return dup_sort_mark(ctx, K, dup_gapped_key_kernel, false, n, d_dup);
}

int rh_dup_stats(real_hip_ctx *ctx, real_hip_dup_stats *out, int reset)
{
    uint64_t h[2];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->dup.stage, RH_PAIR_STRIPES, 2, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->reads = was.items; out->placed = h[0]; out->groups = h[1]; out->duplicates = h[0] - h[1];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
