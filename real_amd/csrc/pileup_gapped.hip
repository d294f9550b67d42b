// pileup_gapped.hip -- the gapped placements (gap rescue's mates, anchored gap placement's reads) in the per-position accounting:
// their depth and mismatch base counts into the begun pileup, their evidence into the calls of the finished one
// (include/real_hip.h, "gapped placements in the pileup and the calls").
//
// One lane per record in both kernels (wave64, blocks of 256), the shape of gapped_list.hip: read_walk.h's placed_gap takes the
// lane's gap record to a placement -- every check comes before the first byte of read or text is touched -- and says where its
// two diagonals lie; a deleted text position is covered by nothing.
//
// pileup_gapped_add_kernel: the depth goes into the pileup's difference array AND into a second one, gdiff, with the same
// wrap-around increments -- +1 at p, -1 behind the span, and for a deletion -1 / +1 round the deleted range: four atomics per
// array for a deletion, two otherwise.  Then each diagonal is a SEGMENT of read_walk.h's walk (32 bases a step, XOR against the
// funnel-shifted text, one flag per differing base), and every flagged base does pileup_add_kernel's sequence: quality (one
// byte, loaded only when min_qual > 0), then the text's N bit, then one atomicAdd into the alt table.
//
// pileup_gapped_call_kernel: call_add_kernel's shape on the same two segments -- per turn of 32 text positions the lane first
// takes the site bitmap's bits under the segment and loads read bases only where one is set.
//
// Everything is an integer sum: nothing depends on the order of records, lanes, blocks or calls.  No LDS, no scratch memory,
// plain C++ with vector stores and atomics.
#include "read_walk.h"

#include <cstring>

#define RH_PG_BLOCK 256u

// ---- the stage's state (real_hip_ctx::pileup_gapped) -----------------------------------------------------------------------
void rh_pileup_gapped_release(real_hip_ctx *ctx)
{
    RhPileupGappedStage &s = ctx->pileup_gapped; // (releasing a buffer that was never made does nothing)
    rh_release(ctx, s.gdiff); rh_release(ctx, s.rec);
    s.have_gdiff = false;
}
uint32_t *rh_pileup_gapped_array(real_hip_ctx *ctx)
{
    return ctx->pileup_gapped.have_gdiff ? (uint32_t *)ctx->pileup_gapped.gdiff.p : nullptr;
}

// ---- the pileup leg ----------------------------------------------------------------------------------------------------------
struct PileupGappedArgs : GapRecordArgs {
    uint32_t min_qual;
    uint32_t *diff;                // n + 1: the depth's difference array (the pileup's)
    uint32_t *gdiff;               // n + 1: the same increments, of the gapped placements alone
    uint32_t *alt;                 // 4 per text position (the pileup's)
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] other_file, [2] invalid, [3] ungapped, [4] aligned bases,
                                   // [5] deleted, [6] inserted, [7] mismatches, [8] low_qual, [9] n_dropped
};

// one segment: `len` bases of the oriented read from offset r0 on text positions x0 .. x0 + len - 1
static __device__ __forceinline__ void pg_add_segment(const PileupGappedArgs &A, const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t x0,
                                                      uint32_t r0, uint32_t len, uint32_t &mism, uint32_t &lowq, uint32_t &ndrop)
{
    const uint32_t nw = (len + 31u) >> 5;
    ReadWalk walk;
    walk.begin(A.t.text, x0, len);
    for (uint32_t w = 0; w < nw; ++w) {
        uint32_t nb;
        uint64_t al, o;
        uint64_t flags = walk.step_from(b, start, L, inv, r0, len, w, nb, al, o); // one flag per base that differs from the text
        while (flags) {
            const uint32_t u = (uint32_t)__clzll((long long)flags) >> 1; // base u of the word: its flag is bit 62 - 2u
            flags &= ~(1ull << (62 - 2 * u));
            const uint32_t k = r0 + 32u * w + u;                         // base k of the oriented read
            const uint64_t tp = (uint64_t)x0 + 32u * w + u;
            // quality first, then the N bit (each counter is added to on every path: a counter picked by the path taken would be
            // an array in scratch memory)
            uint32_t low = 0, on_n = 0;
            if (A.min_qual) {
                const uint32_t q = b.qual ? b.qual[start + (inv ? L - 1 - k : k)] : 30u;
                low = q < A.min_qual ? 1u : 0u;
            }
            if (!low && A.t.has_wild) on_n = (uint32_t)(A.t.wild[tp >> 6] >> (63 - (tp & 63))) & 1u;
            const uint32_t hit = 1u - (low | on_n);
            if (hit) atomicAdd(A.alt + 4 * tp + ((uint32_t)(o >> (62 - 2 * u)) & 3u), 1u);
            lowq += low; ndrop += on_n; mism += hit;
        }
    }
}

__global__ void __launch_bounds__(RH_PG_BLOCK) pileup_gapped_add_kernel(const PileupGappedArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_PG_BLOCK + threadIdx.x;
    uint32_t placed = 0, other = 0, invalid = 0, ungapped = 0, bases = 0, deleted = 0, inserted = 0, mism = 0, lowq = 0, ndrop = 0;
    if (i < A.n) {
        const PlacedGap c = placed_gap(A, i);
        other = c.other; invalid = c.bad;
        if (c.place) {
            const DevBatch b = A.mate(c.second);
            const uint32_t p = c.p, L = c.L, d = c.d, del = c.del;
            placed = 1; ungapped = c.gapped() ? 0u : 1u; bases = L - d; deleted = del; inserted = d;
            // the depth: [p, p + L - d), or for a deletion [p, p + j) and [p + j + del, p + L + del) (all <= n: the record fits)
            const uint64_t end = (uint64_t)p + L - d + del;
            atomicAdd(A.diff + p, 1u);
            atomicAdd(A.gdiff + p, 1u);
            if (del) {
                const uint64_t x = (uint64_t)p + c.len1();
                atomicAdd(A.diff + x, 0xffffffffu);
                atomicAdd(A.gdiff + x, 0xffffffffu);
                atomicAdd(A.diff + x + del, 1u);
                atomicAdd(A.gdiff + x + del, 1u);
            }
            atomicAdd(A.diff + end, 0xffffffffu);
            atomicAdd(A.gdiff + end, 0xffffffffu);
            // the aligned pairs: the first segment; the second starts behind the gap
            pg_add_segment(A, b, c.start, L, c.inv, p, 0u, c.len1(), mism, lowq, ndrop);
            if (c.gapped()) pg_add_segment(A, b, c.start, L, c.inv, p + c.t2(), c.r2(), c.len2(), mism, lowq, ndrop);
        }
    }
    // (a wave's sums stay below 2^32: 64 reads of at most REAL_HIP_MAX_PATL bases)
    uint32_t s[10] = {placed, other, invalid, ungapped, bases, deleted, inserted, mism, lowq, ndrop};
    rh_stats_add(A.stats, s);
}

// ---- the call leg ------------------------------------------------------------------------------------------------------------
struct CallGappedArgs : GapRecordArgs {
    uint32_t min_qual;
    const uint64_t *bits;          // the site bitmap: n / 64 + 2 words (snp_call.hip)
    const uint32_t *rank;          // sites before each bitmap word
    uint32_t *ev;                  // 8 per site: cnt[4], qsum[4]
    uint64_t n_sites;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] site_bases, [1] site_low_qual
};

static __device__ __forceinline__ void pg_call_segment(const CallGappedArgs &A, const DevBatch &b, uint64_t start, uint32_t L, bool inv, uint32_t xs,
                                                       uint32_t r0, uint32_t len, uint32_t &sbases, uint32_t &lowq)
{
    const uint32_t nw = (len + 31u) >> 5;
    for (uint32_t w = 0; w < nw; ++w) {
        // the 32 bitmap bits under text positions x0 .. x0 + 31 (x0 + 31 may lie behind the segment: masked off; the bitmap has a
        // word behind the one of the text's last position)
        const uint64_t x0 = (uint64_t)xs + 32u * w;
        const uint32_t left = min(32u, len - 32u * w), s = (uint32_t)(x0 & 63u);
        uint64_t v = A.bits[x0 >> 6] << s;
        if (s > 32u) v |= A.bits[(x0 >> 6) + 1] >> (64u - s);
        uint32_t m = (uint32_t)(v >> 32);
        if (left < 32u) m &= ~0u << (32u - left);
        if (!m) continue;
        const uint64_t o = ReadWalk::oriented_from(b, start, L, inv, r0 + 32u * w, left);
        while (m) {
            const uint32_t u = (uint32_t)__clz((int)m);                  // base u of the word: its bit is 31 - u
            m &= ~(0x80000000u >> u);
            const uint32_t k = r0 + 32u * w + u;                         // base k of the oriented read
            const uint32_t q = b.qual ? b.qual[start + (inv ? L - 1 - k : k)] : 30u;
            const uint32_t low = q < A.min_qual ? 1u : 0u; // (both counters are added to on every path: see pg_add_segment)
            uint32_t hit = 0;
            if (!low) {
                const uint64_t tp = x0 + u;
                const uint32_t ts = (uint32_t)(tp & 63u);
                const uint64_t slot = (uint64_t)A.rank[tp >> 6] + (ts ? (uint64_t)__popcll(A.bits[tp >> 6] >> (64u - ts)) : 0ull);
                if (slot < A.n_sites) { // (always: the bitmap is the site list's)
                    const uint32_t base = (uint32_t)(o >> (62 - 2 * u)) & 3u;
                    atomicAdd(A.ev + 8 * slot + base, 1u);
                    atomicAdd(A.ev + 8 * slot + 4 + base, q);
                    hit = 1;
                }
            }
            lowq += low; sbases += hit;
        }
    }
}

__global__ void __launch_bounds__(RH_PG_BLOCK) pileup_gapped_call_kernel(const CallGappedArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_PG_BLOCK + threadIdx.x;
    uint32_t sbases = 0, lowq = 0;
    if (i < A.n) {
        const PlacedGap c = placed_gap(A, i);
        if (c.place) {
            const DevBatch b = A.mate(c.second);
            pg_call_segment(A, b, c.start, c.L, c.inv, c.p, 0u, c.len1(), sbases, lowq);
            if (c.gapped()) pg_call_segment(A, b, c.start, c.L, c.inv, c.p + c.t2(), c.r2(), c.len2(), sbases, lowq);
        }
    }
    uint32_t s[2] = {sbases, lowq}; // (a wave's sums stay below 2^32: 64 reads of at most REAL_HIP_MAX_PATL bases)
    rh_stats_add(A.stats, s);
}

// ---- host side --------------------------------------------------------------------------------------------------
int rh_pileup_gapped_add(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n)
{
    if (!n) return REAL_HIP_OK;
    RhPileupGappedStage &S = ctx->pileup_gapped;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.add.stats, RH_PAIR_STRIPES, 0))) return rc;
    if (!S.have_gdiff) {
        const size_t bytes = (size_t)(ctx->pileup.n + 1) * 4;
        if (rh_reserve(ctx, S.gdiff, bytes))
            return rh_fail(ctx, REAL_HIP_E_NOMEM, "pileup: the gapped placements' difference array (4 bytes per base of the text) does not fit the device memory",
                           hipSuccess);
        RH_HIP(ctx, hipMemsetAsync(S.gdiff.p, 0, bytes, ctx->stream));
        S.have_gdiff = true;
    }
    PileupGappedArgs A;
    memset(&A, 0, sizeof A);
    rh_gap_record_args(A, ctx, b1, b2, d_gaps, n);
    if (!ctx->pileup.min_qual) A.b[0].qual = A.b[1].qual = nullptr; // (not loaded)
    A.min_qual = ctx->pileup.min_qual;
    A.diff = (uint32_t *)ctx->pileup.diff.p; A.gdiff = (uint32_t *)S.gdiff.p; A.alt = (uint32_t *)ctx->pileup.alt.p;
    A.stats = (unsigned long long *)S.add.stats.p;
    rh_time_begin(ctx, ctx->stream, S.add);
    hipLaunchKernelGGL(pileup_gapped_add_kernel, dim3((unsigned)((n + RH_PG_BLOCK - 1) / RH_PG_BLOCK)), dim3(RH_PG_BLOCK), 0, ctx->stream, A);
    const hipError_t e = hipGetLastError();
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "pileup: add of the gapped placements", e);
    S.add.items += n;
    S.add.launches += 1;
    return REAL_HIP_OK;
}

int rh_call_gapped_add(real_hip_ctx *ctx, const DevBatch &b1, const DevBatch &b2, const real_hip_gap_place *d_gaps, uint64_t n)
{
    if (!n) return REAL_HIP_OK;
    RhPileupGappedStage &S = ctx->pileup_gapped;
    int rc;
    if ((rc = rh_stats_reserve(ctx, S.call.stats, RH_PAIR_STRIPES, 0))) return rc;
    CallGappedArgs A;
    memset(&A, 0, sizeof A);
    rh_gap_record_args(A, ctx, b1, b2, d_gaps, n);
    A.min_qual = ctx->pileup.min_qual;
    A.bits = (const uint64_t *)ctx->call.bits.p; A.rank = (const uint32_t *)ctx->call.rank.p; A.ev = (uint32_t *)ctx->call.ev.p;
    A.n_sites = ctx->pileup.n_sites;
    A.stats = (unsigned long long *)S.call.stats.p;
    rh_time_begin(ctx, ctx->stream, S.call);
    hipLaunchKernelGGL(pileup_gapped_call_kernel, dim3((unsigned)((n + RH_PG_BLOCK - 1) / RH_PG_BLOCK)), dim3(RH_PG_BLOCK), 0, ctx->stream, A);
    const hipError_t e = hipGetLastError();
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "calls: add of the gapped placements", e);
    S.call.items += n;
    S.call.launches += 1;
    return REAL_HIP_OK;
}

int rh_pileup_gapped_stats(real_hip_ctx *ctx, real_hip_pileup_gapped_stats *out, int reset)
{
    uint64_t h[10], c[2];
    RhStageCount was, wasc;
    RhPileupGappedStage &S = ctx->pileup_gapped;
    int rc;
    if ((rc = rh_stage_read(ctx, S.add, RH_PAIR_STRIPES, 10, reset, h, was)) || (rc = rh_stage_read(ctx, S.call, RH_PAIR_STRIPES, 2, reset, c, wasc))) return rc;
    if (out) {
        out->reserved = 0;
        out->records = was.items; out->placed = h[0]; out->other_file = h[1]; out->invalid = h[2]; out->ungapped = h[3];
        out->aligned_bases = h[4]; out->deleted = h[5]; out->inserted = h[6];
        out->mismatches = h[7]; out->low_qual = h[8]; out->n_dropped = h[9];
        out->site_bases = c[0]; out->site_low_qual = c[1];
        out->launches = was.launches + wasc.launches; out->kernel_ms = was.kernel_ms + wasc.kernel_ms;
    }
    return REAL_HIP_OK;
}
