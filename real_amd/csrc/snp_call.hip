// snp_call.hip -- from the finished pileup to genotype calls (include/real_hip.h, "variant calls"): the evidence of every
// site -- how often each base was seen there with sufficient quality, the reference base too, and the sums of those
// qualities -- gathered from the reads, then the ten genotype likelihoods per site and the compacted call list.
//
// Two passes, so that the per-base work happens only where a site is.  The pileup has found the sites; begin turns its
// site list into a BITMAP of one bit per text position (MSB first, as the text's N bits) and a RANK array, the number of
// sites before each 64-bit bitmap word, so that slot(x) = rank[x >> 6] + popcount(the word's bits before x) is the site's
// index.  call_bitmap_kernel: one lane per bitmap word finds its first site by binary search in the (ascending) site list
// and ORs its own bits together -- no atomics, no scan.
//
// call_add_kernel: one lane per read, the placement and the word-by-word walk of pileup_add_kernel (read_walk.h: the same
// records are placed, skipped and counted in both), but per turn of 32 bases
// the lane first takes the 32 bitmap bits under the placement, funnel-shifted from at most two 64-bit words.  Most turns
// find none and load nothing else: no read bases, no text (the calls need no text at all: the reference base is the site
// record's).  For a set bit the lane takes the oriented base from the walk's oriented word, the quality byte (the reverse
// strand indexing L-1-k) and the slot, and does two atomicAdds into the evidence record.
//
// finish: count, scan, emit over the SITES (the pattern of pileup_sites_kernel): one lane per site reads its site record
// and its evidence record, computes the ten PLs and decides; a block counts its calls by ballot, rocPRIM scans the block
// counts, the emit pass writes the 32-byte call records in ascending position.  finish only reads the evidence: it may
// run again with other thresholds.
//
// Everything is an integer sum or a function of one.  No LDS in the add kernel, no scratch memory; plain C++ and vector
// stores.
#include "real_hip_ctx.h"
#include "read_walk.h"

#include <rocprim/device/device_scan.hpp>

#include <cstring>

#define RH_CL_BLOCK 256u

// ---- begin: bitmap and rank array from the site list -----------------------------------------------------------------
// one lane per bitmap word w: rank[w] = the first site with pos >= 64 w, bits[w] = the sites in [64 w, 64 w + 64)
__global__ void __launch_bounds__(RH_CL_BLOCK) call_bitmap_kernel(const uint4 *sites, uint64_t n_sites, uint64_t n_words, uint64_t *bits, uint32_t *rank)
{
    const uint64_t w = (uint64_t)blockIdx.x * RH_CL_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    const uint64_t lo = w << 6, hi = lo + 64;
    uint64_t x = 0, y = n_sites;
    while (x < y) { const uint64_t mid = x + ((y - x) >> 1); if (sites[2 * mid].x < lo) x = mid + 1; else y = mid; }
    uint64_t word = 0;
    for (uint64_t k = x; k < n_sites; ++k) {
        const uint64_t pos = sites[2 * k].x;
        if (pos >= hi) break;
        word |= 1ull << (63 - (pos & 63));
    }
    bits[w] = word;
    rank[w] = (uint32_t)x;
}

// ---- add: the evidence of the placements --------------------------------------------------------------------------------
struct CallArgs {
    DevText  t;
    DevBatch b;                    // the reads of this launch (mate `mate` of a pair launch)
    const uint64_t *info;          // single-end records, or
    const uint2 *pairs;            // real_hip_pair records as five 8-byte words (final_record.h)
    uint32_t mate;                 // pair launches: 0 = mate 1, 1 = mate 2
    uint32_t min_qual;
    const uint64_t *bits;          // the site bitmap: n / 64 + 2 words
    const uint32_t *rank;          // sites before each bitmap word
    uint32_t *ev;                  // 8 per site: cnt[4], qsum[4]
    uint64_t n_sites;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] placed, [1] other_file, [2] invalid, [3] site_bases, [4] low_qual
};

template <bool PAIRS>
__global__ void __launch_bounds__(RH_CL_BLOCK) call_add_kernel(const CallArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RH_CL_BLOCK + threadIdx.x;
    uint32_t placed = 0, other = 0, invalid = 0, sbases = 0, lowq = 0;
    if (i < A.b.n_reads) {
        const PlacedRead r = placed_read<PAIRS>(A.t, A.b, A.info, A.pairs, nullptr, A.mate, i);
        other = r.other; invalid = r.bad;
        if (r.place) {
            placed = 1;
            const uint32_t L = r.L, nw = (L + 31u) >> 5;
            for (uint32_t j = 0; j < nw; ++j) {
                // the 32 bitmap bits under text positions x0 .. x0 + 31 (x0 + 31 may lie behind the read: masked off; the bitmap
                // has a word behind the one of the text's last position)
                const uint64_t x0 = (uint64_t)r.p + 32u * j;
                const uint32_t left = min(32u, L - 32u * j), s = (uint32_t)(x0 & 63u);
                uint64_t v = A.bits[x0 >> 6] << s;
                if (s > 32u) v |= A.bits[(x0 >> 6) + 1] >> (64u - s);
                uint32_t m = (uint32_t)(v >> 32);
                if (left < 32u) m &= ~0u << (32u - left);
                if (!m) continue;
                uint32_t nb;
                const uint64_t o = ReadWalk::oriented(A.b, r.start, L, r.inv, j, nb);
                while (m) {
                    const uint32_t u = (uint32_t)__clz((int)m);                  // base u of the word: its bit is 31 - u
                    m &= ~(0x80000000u >> u);
                    const uint32_t k = 32u * j + u;                              // base k of the oriented read
                    const uint32_t q = A.b.qual ? A.b.qual[r.start + (r.inv ? L - 1 - k : k)] : 30u;
                    if (q < A.min_qual) { ++lowq; continue; }
                    const uint64_t tp = x0 + u;
                    const uint32_t ts = (uint32_t)(tp & 63u);
                    const uint64_t slot = (uint64_t)A.rank[tp >> 6] + (ts ? (uint64_t)__popcll(A.bits[tp >> 6] >> (64u - ts)) : 0ull);
                    if (slot >= A.n_sites) continue; // (cannot happen: the bitmap is the site list's)
                    const uint32_t base = (uint32_t)(o >> (62 - 2 * u)) & 3u;
                    atomicAdd(A.ev + 8 * slot + base, 1u);
                    atomicAdd(A.ev + 8 * slot + 4 + base, q);
                    ++sbases;
                }
            }
        }
    }
    uint32_t s[5] = {placed, other, invalid, sbases, lowq}; // (a wave's sums stay below 2^32: 64 reads of at most 2^14 bases)
    rh_stats_add(A.stats, s);
}

// ---- finish: the genotypes and the calls ----------------------------------------------------------------------------------
struct Genotype {
    uint32_t a1, a2, qual, gq;
};

// the best of the ten genotypes from one site's evidence (real_hip.h: (ref, ref) first, then ascending (a, b); the first of
// minimal PL).  64-bit sums: E of 2^26 bases of quality 63 is beyond 2^32.  Every index is a constant once the loops are
// unrolled: no array lives in scratch memory.
static __device__ __forceinline__ Genotype call_genotype(uint32_t ref, const uint32_t cnt[4], const uint32_t qsum[4])
{
    uint64_t E[4], sum = 0, e_ref = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
        E[d] = (uint64_t)qsum[d] + (uint64_t)REAL_HIP_CALL_ERR * cnt[d];
        sum += E[d];
        if (d == ref) e_ref = E[d];
    }
    const uint64_t pl_ref = sum - e_ref;
    uint64_t best = pl_ref, second = ~0ull;
    Genotype g;
    g.a1 = g.a2 = ref;
#pragma unroll
    for (uint32_t a = 0; a < 4; ++a) {
#pragma unroll
        for (uint32_t b = a; b < 4; ++b) {
            if (a == b && a == ref) continue;
            const uint64_t pl = a == b ? sum - E[a] + REAL_HIP_CALL_PRIOR_HOM
                                       : (uint64_t)REAL_HIP_CALL_HET * ((uint64_t)cnt[a] + cnt[b]) + sum - E[a] - E[b] +
                                             (a == ref || b == ref ? REAL_HIP_CALL_PRIOR_HET : REAL_HIP_CALL_PRIOR_HET2);
            if (pl < best) { second = best; best = pl; g.a1 = a; g.a2 = b; }
            else if (pl < second) second = pl;
        }
    }
    const uint64_t q = pl_ref - best, gq = second - best;
    g.qual = q > 0xffffffffull ? 0xffffffffu : (uint32_t)q;
    g.gq = gq > 99 ? 99u : (uint32_t)gq;
    return g;
}

struct CallFinArgs {
    const uint4 *sites;            // real_hip_pileup_site records, two uint4 each
    const uint4 *ev;               // the evidence records, two uint4 each
    uint64_t n_sites;
    uint32_t min_call_qual, min_depth;
    uint64_t *blk;                 // count pass: calls per block (blocks + 1, the last one 0)
    const uint64_t *blk_off;       // emit pass: their exclusive scan
    uint4 *out;                    // real_hip_call records, two uint4 each
    uint64_t cap;
    unsigned long long *fin;       // RH_PAIR_STRIPES x 16 words: [0] het, [1] hom
};

// one lane per site; EMIT = false counts the block's calls, EMIT = true writes them behind the block's offset
template <bool EMIT>
__global__ void __launch_bounds__(RH_CL_BLOCK) call_sites_kernel(const CallFinArgs A)
{
    __shared__ uint32_t wave_cnt[RH_CL_BLOCK / 64];
    __shared__ uint32_t wave_het[RH_CL_BLOCK / 64];
    const uint64_t s = (uint64_t)blockIdx.x * RH_CL_BLOCK + threadIdx.x;
    uint4 s0 = make_uint4(0, 0, 0, 0), s1 = s0, e0 = s0, e1 = s0;
    if (s < A.n_sites) { s0 = A.sites[2 * s]; s1 = A.sites[2 * s + 1]; e0 = A.ev[2 * s]; e1 = A.ev[2 * s + 1]; }
    const uint32_t cnt[4] = {e0.x, e0.y, e0.z, e0.w}, qsum[4] = {e1.x, e1.y, e1.z, e1.w};
    const uint32_t ref = s1.z & 3u;
    const Genotype g = call_genotype(ref, cnt, qsum);
    const uint32_t dp = e0.x + e0.y + e0.z + e0.w;
    const bool call = s < A.n_sites && (g.a1 != ref || g.a2 != ref) && g.qual >= A.min_call_qual && dp >= A.min_depth;
    const unsigned long long mask = __ballot(call);
    if (!EMIT) {
        const unsigned long long het = __ballot(call && g.a1 != g.a2);
        if ((threadIdx.x & 63u) == 0) wave_het[threadIdx.x >> 6] = (uint32_t)__popcll(het);
        const uint32_t c = rh_block_count(mask, wave_cnt); // (its barrier is wave_het's too)
        if (threadIdx.x == 0) {
            uint32_t h = 0;
            for (uint32_t k = 0; k < RH_CL_BLOCK / 64; ++k) h += wave_het[k];
            A.blk[blockIdx.x] = c;
            if (blockIdx.x + 1 == gridDim.x) A.blk[gridDim.x] = 0;
            unsigned long long *line = A.fin + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16;
            if (h) atomicAdd(line, (unsigned long long)h);
            if (c - h) atomicAdd(line + 1, (unsigned long long)(c - h));
        }
        return;
    }
    const uint64_t slot = rh_emit_slot(mask, A.blk_off[blockIdx.x], wave_cnt);
    if (!call || slot >= A.cap) return; // (the latter cannot happen: the table is what the count saw)
    A.out[2 * slot] = make_uint4(s0.x, s0.y, e0.x, e0.y);
    A.out[2 * slot + 1] = make_uint4(e0.z, e0.w, g.qual, ref | (g.a1 << 8) | (g.a2 << 16) | (g.gq << 24));
}

// ---- host side --------------------------------------------------------------------------------------------------
void rh_call_release(real_hip_ctx *ctx)
{
    rh_release(ctx, ctx->call.bits); rh_release(ctx, ctx->call.rank); rh_release(ctx, ctx->call.ev); rh_release(ctx, ctx->call.blk);
    rh_release(ctx, ctx->call.calls);
    ctx->call.state = 0; ctx->call.n_calls = 0; ctx->call.het = 0; ctx->call.hom = 0;
}

static uint64_t call_bitmap_words(const real_hip_ctx *ctx) { return (ctx->pileup.n >> 6) + 2; } // (one behind the last position's: the funnel shift)

int rh_call_begin(real_hip_ctx *ctx)
{
    static_assert(sizeof(real_hip_call_evidence_rec) == 32 && sizeof(real_hip_call) == 32 && offsetof(real_hip_call, qual) == 24 &&
                      offsetof(real_hip_call, ref) == 28 && offsetof(real_hip_call, gq) == 31,
                  "evidence and call records are two 16-byte stores");
    static_assert(offsetof(real_hip_pileup_site, pos) == 0 && offsetof(real_hip_pileup_site, ref) == 24, "the kernels read pos and ref of a site record");
    const uint64_t words = call_bitmap_words(ctx), n_sites = ctx->pileup.n_sites;
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rh_call_release(ctx);
    int rc;
    if ((rc = rh_stats_reserve(ctx, ctx->call.stage.stats, RH_PAIR_STRIPES, 0))) return rc;
    if ((rc = rh_reserve(ctx, ctx->call.fin, (size_t)RH_PAIR_STRIPES * 16 * 8))) return rc;
    if ((rc = rh_reserve(ctx, ctx->call.bits, (size_t)words * 8)) || (rc = rh_reserve(ctx, ctx->call.rank, (size_t)words * 4)) ||
        (rc = rh_reserve(ctx, ctx->call.ev, (size_t)(n_sites ? n_sites : 1) * sizeof(real_hip_call_evidence_rec)))) {
        rh_call_release(ctx);
        return rh_fail(ctx, REAL_HIP_E_NOMEM, "calls: the site bitmap, its rank array and the evidence (n/8 + n/16 + 32 bytes per site) do not fit the device memory",
                       hipSuccess);
    }
    RH_HIP(ctx, hipMemsetAsync(ctx->call.ev.p, 0, (size_t)(n_sites ? n_sites : 1) * sizeof(real_hip_call_evidence_rec), ctx->stream));
    rh_time_begin(ctx, ctx->stream, ctx->call.stage);
    hipLaunchKernelGGL(call_bitmap_kernel, dim3((unsigned)((words + RH_CL_BLOCK - 1) / RH_CL_BLOCK)), dim3(RH_CL_BLOCK), 0, ctx->stream,
                       (const uint4 *)ctx->pileup.sites.p, n_sites, words, (uint64_t *)ctx->call.bits.p, (uint32_t *)ctx->call.rank.p);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->call.stage.launches += 1;
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rh_time_resolve(ctx);
    ctx->call.state = 1;
    return REAL_HIP_OK;
}

int rh_launch_call_add(real_hip_ctx *ctx, const DevBatch &b, const uint64_t *d_info, const real_hip_pair *d_pairs, uint32_t mate)
{
    const uint64_t n = b.n_reads;
    if (!n) return REAL_HIP_OK;
    CallArgs A;
    memset(&A, 0, sizeof A);
    A.t = rh_dev_text(ctx, ctx->fileid);
    A.b = b;
    A.info = d_info; A.pairs = (const uint2 *)d_pairs; A.mate = mate; A.min_qual = ctx->pileup.min_qual;
    A.bits = (const uint64_t *)ctx->call.bits.p; A.rank = (const uint32_t *)ctx->call.rank.p; A.ev = (uint32_t *)ctx->call.ev.p;
    A.n_sites = ctx->pileup.n_sites;
    A.stats = (unsigned long long *)ctx->call.stage.stats.p;
    const unsigned blocks = (unsigned)((n + RH_CL_BLOCK - 1) / RH_CL_BLOCK);
    rh_time_begin(ctx, ctx->stream, ctx->call.stage);
    if (d_pairs) hipLaunchKernelGGL(call_add_kernel<true>, dim3(blocks), dim3(RH_CL_BLOCK), 0, ctx->stream, A);
    else hipLaunchKernelGGL(call_add_kernel<false>, dim3(blocks), dim3(RH_CL_BLOCK), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    ctx->call.stage.items += n;
    ctx->call.stage.launches += 1;
    return REAL_HIP_OK;
}

int rh_call_finish(real_hip_ctx *ctx, uint32_t min_call_qual, uint32_t min_depth, uint64_t *n_calls)
{
    const uint64_t n_sites = ctx->pileup.n_sites;
    const uint64_t blocks = (n_sites + RH_CL_BLOCK - 1) / RH_CL_BLOCK;
    int rc;
    ctx->call.n_calls = 0; ctx->call.het = 0; ctx->call.hom = 0;
    if (!n_sites) { ctx->call.state = 2; if (n_calls) *n_calls = 0; return REAL_HIP_OK; } // (no kernel over an empty table)
    if ((rc = rh_reserve(ctx, ctx->call.blk, (size_t)(blocks + 1) * 16))) return rc;
    uint64_t *blk = (uint64_t *)ctx->call.blk.p, *blk_off = blk + blocks + 1;
    size_t tmp = 0;
    RH_HIP(ctx, rocprim::exclusive_scan(nullptr, tmp, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream));
    if ((rc = rh_reserve(ctx, ctx->sort_tmp, tmp ? tmp : 8))) return rc;
    RH_HIP(ctx, hipMemsetAsync(ctx->call.fin.p, 0, (size_t)RH_PAIR_STRIPES * 16 * 8, ctx->stream));
    CallFinArgs F;
    F.sites = (const uint4 *)ctx->pileup.sites.p; F.ev = (const uint4 *)ctx->call.ev.p; F.n_sites = n_sites;
    F.min_call_qual = min_call_qual; F.min_depth = min_depth;
    F.blk = blk; F.blk_off = blk_off; F.out = nullptr; F.cap = 0; F.fin = (unsigned long long *)ctx->call.fin.p;
    rh_time_begin(ctx, ctx->stream, ctx->call.stage); // (no return inside the bracket: a failing step is reported behind rh_time_end)
    hipLaunchKernelGGL(call_sites_kernel<false>, dim3((unsigned)blocks), dim3(RH_CL_BLOCK), 0, ctx->stream, F);
    hipError_t e = hipGetLastError();
    size_t t = tmp;
    if (e == hipSuccess) e = rocprim::exclusive_scan(ctx->sort_tmp.p, t, blk, blk_off, (uint64_t)0, (size_t)(blocks + 1), rocprim::plus<uint64_t>(), ctx->stream);
    rh_time_end(ctx, ctx->stream);
    if (e != hipSuccess) return rh_fail(ctx, REAL_HIP_E_DEVICE, "calls: count of the calls / scan of the block counts", e);
    ctx->call.stage.launches += 2;
    uint64_t total = 0;
    std::vector<uint64_t> fin((size_t)RH_PAIR_STRIPES * 16);
    RH_HIP(ctx, hipMemcpyAsync(&total, blk_off + blocks, 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipMemcpyAsync(fin.data(), ctx->call.fin.p, fin.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t het = 0, hom = 0;
    for (size_t s = 0; s < RH_PAIR_STRIPES; ++s) { het += fin[s * 16]; hom += fin[s * 16 + 1]; }
    if (total) {
        if ((rc = rh_reserve(ctx, ctx->call.calls, (size_t)total * sizeof(real_hip_call)))) return rc;
        F.out = (uint4 *)ctx->call.calls.p; F.cap = total;
        rh_time_begin(ctx, ctx->stream, ctx->call.stage);
        hipLaunchKernelGGL(call_sites_kernel<true>, dim3((unsigned)blocks), dim3(RH_CL_BLOCK), 0, ctx->stream, F);
        rh_time_end(ctx, ctx->stream);
        RH_HIP(ctx, hipGetLastError());
        ctx->call.stage.launches += 1;
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    rh_time_resolve(ctx);
    ctx->call.n_calls = total; ctx->call.het = het; ctx->call.hom = hom;
    ctx->call.state = 2;
    if (n_calls) *n_calls = total;
    return REAL_HIP_OK;
}

int rh_call_stats(real_hip_ctx *ctx, real_hip_call_stats *out, int reset)
{
    uint64_t h[5];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->call.stage, RH_PAIR_STRIPES, 5, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->reads = was.items; out->placed = h[0]; out->other_file = h[1]; out->invalid = h[2]; out->site_bases = h[3]; out->low_qual = h[4];
        out->calls = ctx->call.n_calls; out->het = ctx->call.het; out->hom = ctx->call.hom;
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
