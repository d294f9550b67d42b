// pileup.hip -- the pileup of the final placements over the resident text: per-position depth, and at every position where a
// placed read shows another base than the text, how often each base was seen (include/real_hip.h, "pileup").
//
// pileup_add_kernel: one lane per read, and the lane WALKS ITS READ WORD BY WORD -- 32 bases at a time, whatever the length
// (up to REAL_HIP_MAX_PATL_LONG): no register array of the read, no second kernel for long reads (the record's decode into a
// placement and the walk itself are read_walk.h's, shared with snp_call.hip and mismatch_list.hip).  Per word the lane packs
// the 32 read bases that lie over the next 32 text positions with match_common.h's pack_read / pack_read_packed (W = 1; a
// packed read may start inside a byte) -- on the reverse strand those are the read's LAST unvisited bases, turned round with
// revcomp_words -- loads the 2-bit text funnel-shifted to the placement and takes XOR: one flag per base.  Every flagged
// base checks its quality (one byte, loaded only when min_qual > 0), then the text's N bit, then does one atomicAdd into the
// alt table (4 x u32 per text position).  The depth is a difference array of n + 1 u32: +1 at p, -1 at p + L in wrap-around
// arithmetic -- two atomics per read, not one per base.
//
// finish: rocPRIM's inclusive scan turns the difference array into depth[] in place (and, where real_hip_pileup_add_gapped made
// one, the gapped placements' second difference array into gdepth[]: pileup_gapped.hip); then count, scan, emit over the
// positions (the pattern of pair_all.hip; the block's count and a site's slot are stage_common.h's): a block of 256
// positions counts its sites (alt sum > 0), the block counts are scanned, and the emit pass writes the 32-byte site records
// in ascending position.  The count pass also sums `covered` and takes `max_depth`.
//
// Everything is an integer sum: nothing depends on the order of reads, lanes, blocks or calls.  No LDS in the add kernel,
// no scratch memory; plain C++ and vector stores.
#include "real_hip_ctx.h"
#include "read_walk.h"

#include <rocprim/device/device_scan.hpp>

#include <cstring>

#define RH_PU_BLOCK 256u

struct PileupArgs {
    DevText  t;
    DevBatch b;                    // the reads of this launch (mate `mate` of a pair launch)
    const uint64_t *info;          // single-end records, or
    const uint2 *pairs;            // real_hip_pair records as five 8-byte words (final_record.h)
    uint32_t mate;                 // pair launches: 0 = mate 1, 1 = mate 2
    uint32_t min_qual;
    uint32_t *diff;                // n + 1: the depth's difference array
    uint32_t *alt;                 // 4 per text position
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] other_file, [2] invalid, [3] bases, [4] mismatches,
                                   // [5] low_qual, [6] n_dropped
};

template <bool PAIRS>
__global__ void __launch_bounds__(RH_PU_BLOCK) pileup_add_kernel(const PileupArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_PU_BLOCK + threadIdx.x;
    uint32_t placed = 0, other = 0, invalid = 0, bases = 0, mism = 0, lowq = 0, ndrop = 0;
    if (i < A.b.n_reads) {
        // the record: is it a placement in this file, where, on which strand (read_walk.h)
        const PlacedRead r = placed_read<PAIRS>(A.t, A.b, A.info, A.pairs, nullptr, A.mate, i);
        other = r.other; invalid = r.bad;
        const bool inv = r.inv;
        const uint32_t p = r.p, L = r.L;
        const uint64_t start = r.start;
        if (r.place) {
            placed = 1; bases = L;
            atomicAdd(A.diff + p, 1u);
            atomicAdd(A.diff + (uint64_t)p + L, 0xffffffffu);
            const uint32_t nw = (L + 31u) >> 5;
            ReadWalk walk;
            walk.begin(A.t.text, p, L);
            for (uint32_t j = 0; j < nw; ++j) {
                uint32_t nb;
                uint64_t al, o;
                uint64_t flags = walk.step(A.b, start, L, inv, j, nb, al, o); // one flag per base that differs from the text
                while (flags) {
                    const uint32_t u = (uint32_t)__clzll((long long)flags) >> 1; // base u of the word: its flag is bit 62 - 2u
                    flags &= ~(1ull << (62 - 2 * u));
                    const uint32_t k = 32u * j + u;                              // base k of the oriented read
                    const uint64_t tp = (uint64_t)p + k;
                    if (A.min_qual) {
                        const uint32_t q = A.b.qual ? A.b.qual[start + (inv ? L - 1 - k : k)] : 30u;
                        if (q < A.min_qual) { ++lowq; continue; }
                    }
                    if (A.t.has_wild && ((A.t.wild[tp >> 6] >> (63 - (tp & 63))) & 1ull)) { ++ndrop; continue; }
                    atomicAdd(A.alt + 4 * tp + ((uint32_t)(o >> (62 - 2 * u)) & 3u), 1u);
                    ++mism;
                }
            }
        }
    }
    uint32_t s[7] = {placed, other, invalid, bases, mism, lowq, ndrop}; // (a wave's sums stay below 2^32: 64 reads of at most 2^14 bases)
    rh_stats_add(A.stats, s);
}

// ---- finish: the sites ------------------------------------------------------------------------------------------
struct PileupFinArgs {
    const uint64_t *text;
    const uint32_t *depth;         // n: the scanned difference array
    const uint4 *alt;              // n
    uint64_t n;
    uint64_t *blk;                 // count pass: sites per block (blocks + 1, the last one 0)
    const uint64_t *blk_off;       // emit pass: their exclusive scan
    uint4 *out;                    // real_hip_pileup_site records, two uint4 each
    uint64_t cap;
    unsigned long long *fin;       // RH_PAIR_STRIPES x 16 words: [0] covered (sum), [1] max_depth (max)
};

// one lane per position; EMIT = false counts the block's sites, EMIT = true writes them behind the block's offset
template <bool EMIT>
__global__ void __launch_bounds__(RH_PU_BLOCK) pileup_sites_kernel(const PileupFinArgs A)
{
    __shared__ uint32_t wave_cnt[RH_PU_BLOCK / 64];
    __shared__ uint32_t wave_cov[RH_PU_BLOCK / 64];
    __shared__ uint32_t wave_max[RH_PU_BLOCK / 64];
    const uint64_t x = (uint64_t)blockIdx.x * RH_PU_BLOCK + threadIdx.x;
    uint4 a = make_uint4(0, 0, 0, 0);
    uint32_t d = 0;
    if (x < A.n) { a = A.alt[x]; d = A.depth[x]; }
    const bool site = (a.x | a.y | a.z | a.w) != 0;
    const unsigned long long mask = __ballot(site);
    if (!EMIT) {
        const unsigned long long cov = __ballot(d != 0);
        uint32_t m = d;
        for (int k = 32; k; k >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, k));
        if ((threadIdx.x & 63u) == 0) { wave_cov[threadIdx.x >> 6] = (uint32_t)__popcll(cov); wave_max[threadIdx.x >> 6] = m; }
        const uint32_t c = rh_block_count(mask, wave_cnt); // (its barrier is wave_cov's and wave_max's too)
        if (threadIdx.x == 0) {
            uint32_t v = 0, mx = 0;
            for (uint32_t k = 0; k < RH_PU_BLOCK / 64; ++k) { v += wave_cov[k]; mx = max(mx, wave_max[k]); }
            A.blk[blockIdx.x] = c;
            if (blockIdx.x + 1 == gridDim.x) A.blk[gridDim.x] = 0;
            unsigned long long *line = A.fin + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16;
            if (v) atomicAdd(line, (unsigned long long)v);
            if (mx) atomicMax(line + 1, (unsigned long long)mx);
        }
        return;
    }
    const uint64_t slot = rh_emit_slot(mask, A.blk_off[blockIdx.x], wave_cnt);
    if (!site || slot >= A.cap) return; // (the latter cannot happen: the table is what the count saw)
    const uint32_t ref = (uint32_t)(A.text[x >> 5] >> (62 - 2 * (x & 31))) & 3u;
    A.out[2 * slot] = make_uint4((uint32_t)x, d, a.x, a.y);
    A.out[2 * slot + 1] = make_uint4(a.z, a.w, ref, 0u);
}

// ---- host side --------------------------------------------------------------------------------------------------
static void pileup_release(real_hip_ctx *ctx)
{
    rh_call_release(ctx); // (the calls stand on this pileup's sites: they go with it)
    rh_indel_release(ctx); // (the indel calls on its depth)
    rh_pileup_gapped_release(ctx); // (the gapped placements' share of its depth)
    rh_release(ctx, ctx->pileup.diff); rh_release(ctx, ctx->pileup.alt); rh_release(ctx, ctx->pileup.blk); rh_release(ctx, ctx->pileup.sites);
    ctx->pileup.state = 0; ctx->pileup.n_sites = 0; ctx->pileup.covered = 0; ctx->pileup.max_depth = 0;
}

int rh_pileup_begin(real_hip_ctx *ctx, uint32_t min_qual)
{
    static_assert(sizeof(real_hip_pileup_site) == 32, "a site is two 16-byte stores");
    const uint64_t n = ctx->n_bases;
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pileup_release(ctx);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->pileup.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, ctx->pileup.fin, (size_t)RH_PAIR_STRIPES * 16 * 8))) return rc;
    if ((rc = rh_reserve(ctx, ctx->pileup.diff, (size_t)(n + 1) * 4)) || (rc = rh_reserve(ctx, ctx->pileup.alt, (size_t)(n ? n : 1) * 16))) {
        pileup_release(ctx);
        return rh_fail(ctx, REAL_HIP_E_NOMEM, "pileup: the accumulators (20 bytes per base of the text) do not fit the device memory", hipSuccess);
    }
    RH_HIP(ctx, hipMemsetAsync(ctx->pileup.diff.p, 0, (size_t)(n + 1) * 4, ctx->stream));
    RH_HIP(ctx, hipMemsetAsync(ctx->pileup.alt.p, 0, (size_t)(n ? n : 1) * 16, ctx->stream));
    RH_HIP(ctx, hipMemsetAsync(ctx->pileup.fin.p, 0, (size_t)RH_PAIR_STRIPES * 16 * 8, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pileup.n = n; ctx->pileup.fileid = ctx->fileid; ctx->pileup.min_qual = min_qual;
    ctx->pileup.state = 1;
    return REAL_HIP_OK;
}

void rh_pileup_end(real_hip_ctx *ctx)
{
    (void)hipStreamSynchronize(ctx->stream);
    pileup_release(ctx);
}

// the placements of one batch (d_info) or of mate `mate` of a batch of pairs (d_pairs); all arrays on the device;
// asynchronous on the ctx's stream
int rh_launch_pileup_add(real_hip_ctx *ctx, const DevBatch &b, const uint64_t *d_info, const real_hip_pair *d_pairs, uint32_t mate)
{
    const uint64_t n = b.n_reads;
    if (!n) return REAL_HIP_OK;
    PileupArgs A;
    memset(&A, 0, sizeof A);
    A.t = rh_dev_text(ctx, ctx->fileid);
    A.b = b;
    if (!ctx->pileup.min_qual) A.b.qual = nullptr; // (not loaded)
    A.info = d_info; A.pairs = (const uint2 *)d_pairs; A.mate = mate; A.min_qual = ctx->pileup.min_qual;
    A.diff = (uint32_t *)ctx->pileup.diff.p; A.alt = (uint32_t *)ctx->pileup.alt.p;
    A.stats = (unsigned long long *)ctx->pileup.stage.stats.p;
    const unsigned blocks = (unsigned)((n + RH_PU_BLOCK - 1) / RH_PU_BLOCK);
    rh_time_begin(ctx, ctx->stream, ctx->pileup.stage);
    if (d_pairs) hipLaunchKernelGGL(pileup_add_kernel<true>, dim3(blocks), dim3(RH_PU_BLOCK), 0, ctx->stream, A);
    else hipLaunchKernelGGL(pileup_add_kernel<false>, dim3(blocks), dim3(RH_PU_BLOCK), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->pileup.stage.items += n;
    ctx->pileup.stage.launches += 1;
    return REAL_HIP_OK;
}

int rh_pileup_finish(real_hip_ctx *ctx, uint64_t *n_sites)
{
    const uint64_t n = ctx->pileup.n;
    const uint64_t blocks = (n + RH_PU_BLOCK - 1) / RH_PU_BLOCK;
    uint32_t *depth = (uint32_t *)ctx->pileup.diff.p;
    int rc;
    ctx->pileup.n_sites = 0; ctx->pileup.covered = 0; ctx->pileup.max_depth = 0;
    if (!n) { ctx->pileup.state = 2; if (n_sites) *n_sites = 0; return REAL_HIP_OK; }
    if ((rc = rh_reserve(ctx, ctx->pileup.blk, (size_t)(blocks + 1) * 16))) return rc;
    size_t tmp = 0, tmp2 = 0;
    RH_HIP(ctx, rocprim::inclusive_scan(nullptr, tmp, depth, depth, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream));
    uint64_t *blk = (uint64_t *)ctx->pileup.blk.p, *blk_off = blk + blocks + 1;
    RH_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp2, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream));
    if (tmp2 > tmp) tmp = tmp2;
    if ((rc = rh_reserve(ctx, ctx->sort_tmp, tmp ? tmp : 8))) return rc;
    PileupFinArgs F;
    F.text = (const uint64_t *)ctx->text.p; F.depth = depth; F.alt = (const uint4 *)ctx->pileup.alt.p; F.n = n;
    F.blk = blk; F.blk_off = blk_off; F.out = nullptr; F.cap = 0; F.fin = (unsigned long long *)ctx->pileup.fin.p;
    rh_time_begin(ctx, ctx->stream, ctx->pileup.stage); // (no return inside the bracket: a failing step is reported behind rh_time_end)
    size_t t = tmp;
    hipError_t e = rocprim::inclusive_scan(ctx->sort_tmp.p, t, depth, depth, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream);
    uint32_t *gdepth = rh_pileup_gapped_array(ctx); // (the gapped placements' difference array, when an add_gapped made one)
    if (e == hipSuccess && gdepth) {
        t = tmp;
        e = rocprim::inclusive_scan(ctx->sort_tmp.p, t, gdepth, gdepth, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream);
        ctx->pileup.stage.launches += 1;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pileup_sites_kernel<false>, dim3((unsigned)blocks), dim3(RH_PU_BLOCK), 0, ctx->stream, F);
        e = hipGetLastError();
    }
    t = tmp;
    if (e == hipSuccess) e = rocprim::exclusive_scan(ctx->sort_tmp.p, t, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream);
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "pileup: scan of the depth / count of the sites", e);
    ctx->pileup.stage.launches += 3;
    uint64_t total = 0;
    std::vector<uint64_t> fin((size_t)RH_PAIR_STRIPES * 16);
    RH_HIP(ctx, hipMemcpyAsync(&total, blk_off + blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipMemcpyAsync(fin.data(), ctx->pileup.fin.p, fin.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t s = 0; s < RH_PAIR_STRIPES; ++s) {
        ctx->pileup.covered += fin[s * 16];
        if (fin[s * 16 + 1] > ctx->pileup.max_depth) ctx->pileup.max_depth = fin[s * 16 + 1];
    }
    if (total) {
        if ((rc = rh_reserve(ctx, ctx->pileup.sites, (size_t)total * sizeof(real_hip_pileup_site)))) return rc;
        F.out = (uint4 *)ctx->pileup.sites.p; F.cap = total;
        rh_time_begin(ctx, ctx->stream, ctx->pileup.stage);
        hipLaunchKernelGGL(pileup_sites_kernel<true>, dim3((unsigned)blocks), dim3(RH_PU_BLOCK), 0, ctx->stream, F);
        rh_time_end(ctx, ctx->stream);
        RH_HIP(ctx, hipGetLastError());
        ctx->pileup.stage.launches += 1;
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    rh_time_resolve(ctx);
    ctx->pileup.n_sites = total;
    ctx->pileup.state = 2; // (only now: a finish that failed leaves nothing to read, real_hip_pileup_finish releases the accumulators)
    if (n_sites) *n_sites = total;
    return REAL_HIP_OK;
}

int rh_pileup_stats(real_hip_ctx *ctx, real_hip_pileup_stats *out, int reset)
{
    uint64_t h[7];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->pileup.stage, RH_PAIR_STRIPES, 7, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->reads = was.items; out->placed = h[0]; out->other_file = h[1]; out->invalid = h[2]; out->bases = h[3];
        out->mismatches = h[4]; out->low_qual = h[5]; out->n_dropped = h[6];
        out->covered = ctx->pileup.covered; out->sites = ctx->pileup.n_sites; out->max_depth = ctx->pileup.max_depth;
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
