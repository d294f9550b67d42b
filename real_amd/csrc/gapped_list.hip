// gapped_list.hip -- where a gap-rescued mate differs from the resident text, in the text coordinates of its placement: one
// list of {text offset, text base, oriented read base} per fragment (include/real_hip.h, "gapped mismatch lists"); what CIGAR,
// NM and MD of such a mate's SAM line are written from.
//
// Count, scan, emit, the shape of mismatch_list.hip.  One lane per fragment in both passes (wave64, blocks of 256).  The lane
// takes its gap record to a placement with read_walk.h's placed_gap (about one fragment in four is placed, one in fifty with a
// gap: DESIGN.md 7h) -- every check comes before the first byte of read or text is touched.  A gapped placement is two
// diagonals joined at the split, where placed_gap says they lie.  Each is a SEGMENT of read_walk.h's walk: 32 bases a step, the oriented read
// taken from an arbitrary offset (a byte- or base-shifted pack), the text funnel-shifted to the segment's first position, XOR,
// one flag per differing base; the N bits of the same 32 positions are ORed in as in the ungapped lists.  Between the two
// segments the g <= 16 deleted text positions are one more word of the text, every position flagged.  The count pass takes
// popcounts; rocPRIM's exclusive scan of the counts is mm_offsets; the emit pass repeats the walk and writes each flagged
// position with one 4-byte vector store, in ascending text offset.
//
// The output is a function of records, reads and text alone.  No LDS, no scratch memory (no mask of the read is kept: a
// register array indexed at run time would go there), plain C++.
#include "read_walk.h"

#include <rocprim/device/device_scan.hpp>

#include <cstring>

#define RH_GL_BLOCK 256u

struct GappedArgs : GapRecordArgs {
    uint64_t *cnt;                 // count pass: entries per list
    const uint64_t *off;           // emit pass: their exclusive scan (n + 1)
    uint32_t *out;                 // emit pass: real_hip_mismatch records as one word each
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] other_file, [2] invalid, [3] aligned bases, [4] mismatches,
                                   // [5] deleted, [6] inserted, [7] on_n, [8] disagree
};

// the entries of the flagged positions of one word, text offset t0 + u for base u; `base`: the oriented read's word, or null
// for deleted positions
template <bool DELETED>
static __device__ __forceinline__ void gl_emit(uint32_t *__restrict__ out, uint64_t &at, uint64_t end, uint64_t flags, uint64_t nf, uint64_t al, uint64_t o,
                                               uint32_t t0)
{
    while (flags && at < end) {
        const uint32_t u = (uint32_t)__clzll((long long)flags) >> 1; // base u of the word: its flag is bit 62 - 2u
        const uint64_t bit = 1ull << (62 - 2 * u);
        flags &= ~bit;
        const uint32_t ref = (nf & bit) ? 4u : (uint32_t)(al >> (62 - 2 * u)) & 3u;
        const uint32_t base = DELETED ? (uint32_t)REAL_HIP_MISMATCH_DELETED : (uint32_t)(o >> (62 - 2 * u)) & 3u;
        out[at++] = (t0 + u) | (ref << 16) | (base << 24);
    }
}

// one segment: `len` bases of the oriented read from offset r0 on text offsets t0 .. t0 + len - 1 of the placement at p
template <bool EMIT>
static __device__ __forceinline__ void gl_segment(const GappedArgs &A, const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t p, uint32_t r0,
                                                  uint32_t t0, uint32_t len, uint32_t &mism, uint32_t &on_n, uint64_t &at, uint64_t end)
{
    const uint32_t nw = (len + 31u) >> 5;
    ReadWalk walk;
    walk.begin(A.t.text, p + t0, len);
    for (uint32_t w = 0; w < nw; ++w) {
        uint32_t nb;
        uint64_t al, o;
        uint64_t flags = walk.step_from(b, start, L, inv, r0, len, w, nb, al, o);
        uint64_t nf = 0;
        if (A.t.has_wild) {
            nf = mm_n_flags(A.t.wild, (uint64_t)p + t0 + 32u * w);
            if (nb < 32) nf &= ~0ull << (64 - 2 * nb);
            flags |= nf;
        }
        if (!EMIT) {
            mism += (uint32_t)__popcll(flags);
            on_n += (uint32_t)__popcll(nf);
        } else {
            gl_emit<false>(A.out, at, end, flags, nf, al, o, t0 + 32u * w);
        }
    }
}

template <bool EMIT>
__global__ void __launch_bounds__(RH_GL_BLOCK) gapped_list_kernel(const GappedArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_GL_BLOCK + threadIdx.x;
    uint32_t placed = 0, other = 0, invalid = 0, bases = 0, mism = 0, deleted = 0, inserted = 0, on_n = 0, disagree = 0;
    if (i < A.n) {
        uint64_t at = 0, end = 0;
        bool live = true;
        if (EMIT) { at = A.off[i]; end = A.off[i + 1]; live = end > at; }
        uint32_t entries = 0;
        if (live) { // (a lane of the emit pass whose list is empty decodes nothing)
            const PlacedGap c = placed_gap(A, i);
            other = c.other; invalid = c.bad;
            if (c.place) {
                const DevBatch b = A.mate(c.second);
                const uint32_t p = c.p, del = c.del;
                gl_segment<EMIT>(A, b, c.start, c.L, c.inv, p, 0u, 0u, c.len1(), mism, on_n, at, end);
                if (del) { // between the two segments: one more word of the text, every position flagged
                    const uint32_t j = c.len1();
                    ReadWalk walk;
                    walk.begin(A.t.text, p + j, del);
                    const uint64_t al = walk.text_step(0);
                    const uint64_t flags = M55 & (~0ull << (64 - 2 * del));
                    const uint64_t nf = A.t.has_wild ? mm_n_flags(A.t.wild, (uint64_t)p + j) & flags : 0ull;
                    if (!EMIT) on_n += (uint32_t)__popcll(nf);
                    else gl_emit<true>(A.out, at, end, flags, nf, al, 0ull, j);
                }
                if (c.gapped()) gl_segment<EMIT>(A, b, c.start, c.L, c.inv, p, c.r2(), c.t2(), c.len2(), mism, on_n, at, end);
                placed = 1; bases = c.L - c.d; deleted = del; inserted = c.d;
                disagree = mism != c.k ? 1u : 0u;
                entries = mism + del;
            }
        }
        if (!EMIT) A.cnt[i] = entries;
    }
    if (EMIT) return;
    // (a wave's sums stay below 2^32: 64 reads of at most REAL_HIP_MAX_PATL bases)
    uint32_t s[9] = {placed, other, invalid, bases, mism, deleted, inserted, on_n, disagree};
    rh_stats_add(A.stats, s);
}

// ---- host side --------------------------------------------------------------------------------------------------
static GappedArgs gapped_args(real_hip_ctx *ctx, RhGapStage &S, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n)
{
    static_assert(sizeof(real_hip_mismatch) == 4 && offsetof(real_hip_mismatch, ref) == 2 && offsetof(real_hip_mismatch, base) == 3,
                  "a mismatch is one 4-byte store: off | ref << 16 | base << 24");
    GappedArgs A;
    memset(&A, 0, sizeof A);
    rh_gap_record_args(A, ctx, b1, b2, d_gaps, n);
    A.b[0].qual = A.b[1].qual = nullptr; // (not read)
    A.cnt = (uint64_t *)S.gl_cnt.p;
    A.stats = (unsigned long long *)S.lists.stats.p;
    return A;
}

// Phase 1 on device arrays: the counts of the n lists, their scan into d_off (n + 1 entries, device) and the total, read back
// (the stream is synchronised).  Phase 2, rh_gapped_list_emit, writes the records; the caller decides in between whether they
// fit.
int rh_gapped_list_count(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n, uint64_t *d_off,
                         uint64_t *total)
{
    *total = 0;
    RhGapStage &S = ctx->gap;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.lists.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, S.gl_cnt, (size_t)(n + 1) * 8))) return rc;
    uint64_t *cnt = (uint64_t *)S.gl_cnt.p;
    size_t tmp = 0;
    RH_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, cnt, d_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), ctx->stream));
    if ((rc = rh_reserve(ctx, S.gl_tmp, tmp ? tmp : 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(cnt + n, 0, 8, ctx->stream));
    rh_time_begin(ctx, ctx->stream, S.lists); // (no return inside the bracket: a failing step is reported behind rh_time_end)
    hipError_t e = hipSuccess;
    if (n) {
        hipLaunchKernelGGL((gapped_list_kernel<false>), dim3((unsigned)((n + RH_GL_BLOCK - 1) / RH_GL_BLOCK)), dim3(RH_GL_BLOCK), 0, ctx->stream,
                           gapped_args(ctx, S, b1, b2, d_gaps, n));
        e = hipGetLastError();
        S.lists.launches += 1;
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(S.gl_tmp.p, tmp, cnt, d_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), ctx->stream);
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "gapped mismatch lists: count / scan", e);
    S.lists.launches += 1;
    S.lists.items += n;
    RH_HIP(ctx, hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return REAL_HIP_OK;
}

// the records of the lists counted last, behind d_off into d_out (room for `total` of them); asynchronous on the ctx's stream.
// Records, reads and text must be what rh_gapped_list_count saw.
int rh_gapped_list_emit(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n, const uint64_t *d_off,
                        real_hip_mismatch *d_out, uint64_t total)
{
    if (!total) return REAL_HIP_OK;
    RhGapStage &S = ctx->gap;
    GappedArgs A = gapped_args(ctx, S, b1, b2, d_gaps, n);
    A.off = d_off; A.out = (uint32_t *)d_out;
    rh_time_begin(ctx, ctx->stream, S.lists);
    hipLaunchKernelGGL((gapped_list_kernel<true>), dim3((unsigned)((n + RH_GL_BLOCK - 1) / RH_GL_BLOCK)), dim3(RH_GL_BLOCK), 0, ctx->stream, A);
    const hipError_t e = hipGetLastError();
    S.lists.launches += 1;
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "gapped mismatch lists: emit", e);
    return REAL_HIP_OK;
}

int rh_gapped_list_stats(real_hip_ctx *ctx, real_hip_gapped_list_stats *out, int reset)
{
    uint64_t h[9];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->gap.lists, RH_PAIR_STRIPES, 9, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->fragments = was.items; out->placed = h[0]; out->other_file = h[1]; out->invalid = h[2]; out->aligned_bases = h[3];
        out->mismatches = h[4]; out->deleted = h[5]; out->inserted = h[6]; out->on_n = h[7]; out->disagree = h[8];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
