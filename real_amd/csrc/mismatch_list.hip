// mismatch_list.hip -- where each finally placed read differs from the resident text: one list of {offset, text base, oriented
// read base} per read (include/real_hip.h, "mismatch lists"); what NM / MD of a SAM line are written from.
//
// Count, scan, emit (the pattern of pair_all.hip and of the pileup's sites).  One lane per placement in both passes (wave64,
// blocks of 256).  The lane takes its record -- an info word, a pair record, or the mate's single record where the pair
// record has no placement -- as a placement on the text with read_walk.h's placed_read, the step the pileup and the calls
// take, then walks its read word by word with read_walk.h, the walk of pileup_add_kernel: 32 bases per step, the oriented
// read XOR the funnel-shifted text, one flag per differing base.  Where
// the text holds an N at all, the N bits of the same 32 positions are ORed in: an N of the text is listed whatever the read
// shows.  The count pass takes the popcount and writes it; rocPRIM's exclusive scan of the counts is mm_offsets; the emit
// pass repeats the walk and writes every flagged base with one 4-byte vector store behind the lane's offset, in ascending
// offset.  The statistics are taken in the count pass and added to the striped line by stage_common.h's rh_stats_add.
//
// The output is a function of records, reads and text alone.  No LDS, no scratch memory, plain C++.
#include "real_hip_ctx.h"
#include "read_walk.h"

#include <rocprim/device/device_scan.hpp>

#include <cstring>

#define RH_MM_BLOCK 256u

struct MismatchArgs {
    DevText  t;
    DevBatch b;                    // the reads of this launch (mate `mate` of a pair launch)
    const uint64_t *info;          // single-end records, or
    const uint2 *pairs;            // real_hip_pair records as five 8-byte words (final_record.h) and
    const uint4 *singles;          // this mate's real_hip_single records (nullable)
    uint32_t mate;                 // pair launches: 0 = mate 1, 1 = mate 2
    uint32_t stride;               // read i of the launch is list i * stride + mate: 1 single-end, 2 pairs
    uint64_t *cnt;                 // count pass: entries per list
    const uint64_t *off;           // emit pass: their exclusive scan (lists + 1)
    uint32_t *out;                 // emit pass: real_hip_mismatch records as one word each
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] other_file, [2] invalid, [3] bases, [4] mismatches,
                                   // [5] on_n, [6] disagree
};

template <bool PAIRS, bool EMIT>
__global__ void __launch_bounds__(RH_MM_BLOCK) mismatch_list_kernel(const MismatchArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_MM_BLOCK + threadIdx.x;
    uint32_t placed = 0, other = 0, invalid = 0, bases = 0, mism = 0, on_n = 0, disagree = 0;
    if (i < A.b.n_reads) {
        const uint64_t list = i * A.stride + A.mate;
        uint64_t at = 0, end = 0;
        bool live = true;
        if (EMIT) { at = A.off[list]; end = A.off[list + 1]; live = end > at; }
        if (live) { // (a lane of the emit pass whose list is empty decodes nothing)
            const PlacedRead c = placed_read<PAIRS>(A.t, A.b, A.info, A.pairs, A.singles, A.mate, i);
            other = c.other; invalid = c.bad;
            if (c.place) {
                const uint32_t p = c.p, L = c.L;
                const uint64_t start = c.start;
                const uint32_t nw = (L + 31u) >> 5;
                ReadWalk walk;
                walk.begin(A.t.text, p, L);
                for (uint32_t j = 0; j < nw; ++j) {
                    uint32_t nb;
                    uint64_t al, o;
                    uint64_t flags = walk.step(A.b, start, L, c.inv, j, nb, al, o);
                    uint64_t nf = 0;
                    if (A.t.has_wild) {
                        nf = mm_n_flags(A.t.wild, (uint64_t)p + 32u * j);
                        if (nb < 32) nf &= ~0ull << (64 - 2 * nb);
                        flags |= nf;
                    }
                    if (!EMIT) {
                        mism += (uint32_t)__popcll(flags);
                        on_n += (uint32_t)__popcll(nf);
                    } else {
                        while (flags && at < end) {
                            const uint32_t u = (uint32_t)__clzll((long long)flags) >> 1; // base u of the word: its flag is bit 62 - 2u
                            const uint64_t bit = 1ull << (62 - 2 * u);
                            flags &= ~bit;
                            const uint32_t ref = (nf & bit) ? 4u : (uint32_t)(al >> (62 - 2 * u)) & 3u;
                            A.out[at++] = (32u * j + u) | (ref << 16) | (((uint32_t)(o >> (62 - 2 * u)) & 3u) << 24);
                        }
                    }
                }
                placed = 1; bases = L;
                disagree = mism != c.k ? 1u : 0u;
            }
        }
        if (!EMIT) A.cnt[list] = mism;
    }
    if (EMIT) return;
    uint32_t s[7] = {placed, other, invalid, bases, mism, on_n, disagree}; // (a wave's sums stay below 2^32: 64 reads of at most 2^14 bases)
    rh_stats_add(A.stats, s);
}

// ---- host side --------------------------------------------------------------------------------------------------
static MismatchArgs mismatch_args(real_hip_ctx *ctx, const RhMismatchLaunch &l, uint32_t mate, uint32_t stride)
{
    static_assert(sizeof(real_hip_mismatch) == 4 && offsetof(real_hip_mismatch, ref) == 2 && offsetof(real_hip_mismatch, base) == 3,
                  "a mismatch is one 4-byte store: off | ref << 16 | base << 24");
    MismatchArgs A;
    memset(&A, 0, sizeof A);
    A.t = rh_dev_text(ctx, ctx->fileid);
    A.b = l.b;
    A.b.qual = nullptr; // (not read)
    A.info = l.info; A.pairs = (const uint2 *)l.pairs; A.singles = (const uint4 *)l.singles;
    A.mate = mate; A.stride = stride;
    A.cnt = (uint64_t *)ctx->mismatch.cnt.p;
    A.stats = (unsigned long long *)ctx->mismatch.stage.stats.p;
    return A;
}

template <bool EMIT>
static void mismatch_launch(real_hip_ctx *ctx, const MismatchArgs &A)
{
    const unsigned blocks = (unsigned)((A.b.n_reads + RH_MM_BLOCK - 1) / RH_MM_BLOCK);
    if (A.pairs) hipLaunchKernelGGL((mismatch_list_kernel<true, EMIT>), dim3(blocks), dim3(RH_MM_BLOCK), 0, ctx->stream, A);
    else hipLaunchKernelGGL((mismatch_list_kernel<false, EMIT>), dim3(blocks), dim3(RH_MM_BLOCK), 0, ctx->stream, A);
}

// Phase 1 on device arrays: l[0] alone (single-end) or l[0], l[1] = the two mates (pairs); the counts of the n_launch * n
// lists, their scan into d_off (lists + 1 entries, device) and the total, read back (the stream is synchronised).  Phase 2,
// rh_mismatch_emit, writes the records; the caller decides in between whether they fit.
int rh_mismatch_count(real_hip_ctx *ctx, const RhMismatchLaunch l[], int n_launch, uint64_t *d_off, uint64_t *total)
{
    *total = 0;
    const uint64_t n = l[0].b.n_reads, lists = n * (uint64_t)n_launch;
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->mismatch.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, ctx->mismatch.cnt, (size_t)(lists + 1) * 8))) return rc;
    uint64_t *cnt = (uint64_t *)ctx->mismatch.cnt.p;
    size_t tmp = 0;
    RH_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, cnt, d_off, (uint64_t)0, (size_t)(lists + 1), rocprim::plus<uint64_t>(), ctx->stream));
    if ((rc = rh_reserve(ctx, ctx->sort_tmp, tmp ? tmp : 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(cnt + lists, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, ctx->mismatch.stage); // (no return inside the bracket: a failing step is reported behind rh_time_end)
    hipError_t e = hipSuccess;
    for (int m = 0; m < n_launch && e == hipSuccess && n; ++m) {
        mismatch_launch<false>(ctx, mismatch_args(ctx, l[m], (uint32_t)m, (uint32_t)n_launch));
        e = hipGetLastError();
        ctx->mismatch.stage.launches += 1;
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(ctx->sort_tmp.p, tmp, cnt, d_off, (uint64_t)0, (size_t)(lists + 1), rocprim::plus<uint64_t>(), ctx->stream);
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "mismatch lists: count / scan", e);
    ctx->mismatch.stage.launches += 1;
    ctx->mismatch.stage.items += lists;
    RH_HIP(ctx, hipMemcpyAsync(total, d_off + lists, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return REAL_HIP_OK;
}

// the records of the lists counted last, behind d_off into d_out (room for `total` of them); asynchronous on the ctx's stream.
// Records, reads and text must be what rh_mismatch_count saw.
int rh_mismatch_emit(real_hip_ctx *ctx, const RhMismatchLaunch l[], int n_launch, const uint64_t *d_off, real_hip_mismatch *d_out, uint64_t total)
{
    if (!total) return REAL_HIP_OK;
    rh_time_begin(ctx, ctx->stream, ctx->mismatch.stage);
    hipError_t e = hipSuccess;
    for (int m = 0; m < n_launch && e == hipSuccess; ++m) {
        MismatchArgs A = mismatch_args(ctx, l[m], (uint32_t)m, (uint32_t)n_launch);
        A.off = d_off; A.out = (uint32_t *)d_out;
        mismatch_launch<true>(ctx, A);
        e = hipGetLastError();
        ctx->mismatch.stage.launches += 1;
    }
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "mismatch lists: emit", e);
    return REAL_HIP_OK;
}

int rh_mismatch_stats(real_hip_ctx *ctx, real_hip_mismatch_stats *out, int reset)
{
    uint64_t h[7];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->mismatch.stage, RH_PAIR_STRIPES, 7, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->reads = was.items; out->placed = h[0]; out->other_file = h[1]; out->invalid = h[2]; out->bases = h[3];
        out->mismatches = h[4]; out->on_n = h[5]; out->disagree = h[6];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
