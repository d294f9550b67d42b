// gap_rescue.hip -- gap rescue (include/real_hip.h, "gap rescue"): per fragment with one mate placed uniquely and the other
// nowhere, every start of the window the insert bounds allow is tested for an alignment of the other mate with at most one
// insertion or deletion, and the best one becomes the fragment's record.
//
// gap_select_kernel: one lane per fragment decides from the final records whether the fragment is eligible in the resident
// file and not skipped, and appends it to the list of the search (pair_hand_over: one atomic per wave); it writes the NoMatch
// records of the fragments the search will not write.
// gap_search_kernel: a fixed grid of waves takes the listed fragments in turn, a wave each, so a record has one writer.  The
// wave packs the oriented target into words of 32 bases in LDS and stages the text words of the window there.  Lane t of a
// tile owns start p = first + 64 tile + t.  First every diagonal q of the tile and of its max_gap neighbours on either side
// gets three numbers from one pass over its words (funnel-shifted text XOR read, popcount): the mismatches of the first
// min_flank bases, of the last min_flank bases and of the whole read, into LDS (gap_core.h, shared with gap_anchor.hip).
// A candidate (p, g, j) is the prefix of
// diagonal p plus the suffix of diagonal p + g, and whatever j is, the first min_flank bases of p and the last min_flank of
// p + g are part of it: a pair of diagonals whose two numbers already exceed what max_cost allows is dropped -- exact, and on
// random text about one pair in a thousand passes.  A pair that passes walks the split points once, one base a step, adding
// the base that joins the prefix and taking off the one that leaves the suffix, both read from LDS (a mask of 320 bits in
// registers would be a run-time indexed array: scratch memory); it keeps the leftmost minimum.
// The lane keeps the smallest key (cost, |g|, p, g, j) of its starts and writes the smallest cost of each start into LDS.  A
// butterfly gives every lane the wave's best key; `second` is then the minimum over the starts more than max_gap away from
// the best one, from LDS, and a second butterfly.  Lane 0 writes the record with one 16-byte store.
//
// Nothing depends on lanes, tiles or the order of the list.  No scratch memory; plain C++ and vector stores.
#include "gap_core.h"   // read_words.h; gap_mm, gap_diagonal, gap_best_split, the record packing
#include "pair_state.h" // pair_hand_over, stage_common.h

#include <cstdio>
#include <cstring>

// ---- the kernels ------------------------------------------------------------------------------------------------------------
#define RH_GAP_NP (REAL_HIP_MATE_SEARCH_MAX_INSERT + 2u * REAL_HIP_GAP_MAX + 1u) /* examined starts of a window: hi - lo <= max_insert */
#define RH_GAP_TW ((RH_GAP_NP + 2u * REAL_HIP_GAP_MAX + REAL_HIP_MAX_PATL + 31u) / 32u + 3u) /* its text words: the neighbours' diagonals, the read behind the last, the funnel shift */
#define RH_GAP_HT (64u + 2u * REAL_HIP_GAP_MAX) /* diagonals of a tile */
#define RH_GAP_NOKEY (~0ull)

struct GapArgs {
    DevText t;
    DevBatch b[2];                 // the mates' reads
    const uint2 *pairs;            // real_hip_pair records as five 8-byte words (final_record.h)
    const uint4 *singles[2];
    uint64_t n;                    // fragments
    uint4 *out;                    // real_hip_gap_place records: x pos, y frag:16 | fileid:8 | tag:8, z split:16 | gap:8 | k:8, w cost:16 | second:16
    uint32_t *list;                // fragments to search
    unsigned long long *list_count;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] eligible, [1] listed, [2] other file, [3] positions, [4] placed, [5] unique, [6] gapped
    uint32_t *err_flags;           // bit 0: a window wider than the LDS regions
    uint32_t fresh, min_insert, max_insert, max_gap, min_flank, cost_mismatch, cost_open, cost_extend, max_cost, margin;
};
// what the two single records say of a fragment whose pair record is NoMatch: true iff exactly one is Unique and the other
// NoMatch; *tm: the target mate (0 = mate 1), *ra: the anchor's record
static __device__ __forceinline__ bool gap_roles(const uint4 r1, const uint4 r2, uint32_t *tm, uint4 *ra)
{
    const uint32_t st1 = REAL_HIP_SINGLE_STATE(r1.w >> 24), st2 = REAL_HIP_SINGLE_STATE(r2.w >> 24);
    const bool u1 = st1 == REAL_HIP_PAIR_UNIQUE, u2 = st2 == REAL_HIP_PAIR_UNIQUE;
    if (u1 == u2 || (u1 ? st2 : st1) != REAL_HIP_PAIR_NOMATCH) return false;
    *tm = u1 ? 1u : 0u;
    *ra = u1 ? r1 : r2;
    return true;
}

__global__ void __launch_bounds__(256) gap_select_kernel(const GapArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool eligible = false, listed = false, other = false;
    if (i < A.n) {
        uint32_t tm = 0;
        uint4 ra = make_uint4(0, 0, 0, 0);
        if (rh_pair_state(A.pairs[i * 5 + 4].y) == REAL_HIP_PAIR_NOMATCH && gap_roles(A.singles[0][i], A.singles[1][i], &tm, &ra)) {
            if (((ra.w >> 16) & 0xffu) != A.t.fileid) {
                other = true;
            } else {
                eligible = true;
                const DevBatch &bt = tm ? A.b[1] : A.b[0], &ba = tm ? A.b[0] : A.b[1];
                uint64_t o0, oa;
                const uint64_t L = gap_read_span(bt, i, &o0), La = gap_read_span(ba, i, &oa);
                const uint32_t frag = ra.w & 0xffffu;
                bool skip = L > (uint64_t)REAL_HIP_MAX_PATL || L < 2ull * A.min_flank + A.max_gap + 1ull || frag >= A.t.n_frag;
                if (!skip) skip = (uint64_t)ra.z < A.t.frag_start[frag] || (uint64_t)ra.z + La > A.t.frag_start[frag + 1];
                if (!skip) { // a symbol > 3
                    if (bt.packed) {
                        skip = bt.nflags && ((bt.nflags[i >> 3] >> (i & 7)) & 1);
                    } else {
                        for (uint64_t x = 0; x < L; ++x) skip = skip || bt.bases[o0 + x] > 3;
                    }
                }
                listed = !skip;
            }
        }
        if (!listed && (A.fresh || eligible)) A.out[i] = gap_empty_record();
    }
    pair_hand_over(listed, (uint32_t)i, eligible ? 1ull : 0ull, blockIdx.x, A.list, A.list_count, A.stats);
    const unsigned long long om = __ballot(other);
    if ((threadIdx.x & 63u) == 0 && om) atomicAdd(A.stats + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16 + 2, (unsigned long long)__popcll(om));
}

// the key of a candidate: cost:16 | |g|:5 | p - first:13 | deletion:1 | j:9 | k:4 -- ascending keys are ascending (cost, |g|, p, g, j)
static __device__ __forceinline__ uint64_t gap_key(uint32_t cost, uint32_t ag, uint32_t prel, bool deletion, uint32_t j, uint32_t k)
{
    return ((uint64_t)cost << 32) | ((uint64_t)ag << 27) | ((uint64_t)prel << 14) | ((uint64_t)(deletion ? 1u : 0u) << 13) | ((uint64_t)j << 4) | k;
}

__global__ void __launch_bounds__(256) gap_search_kernel(const GapArgs A)
{
    __shared__ uint64_t sRead[4][2][RH_MAXW];   // per wave: the target's words, straight and reverse-complemented
    __shared__ uint64_t sText[4][RH_GAP_TW];    // per wave: the text words of the window
    __shared__ uint32_t sDiag[4][RH_GAP_HT];    // per wave: gap_diagonal of the tile's diagonals
    __shared__ uint16_t sMin[4][RH_GAP_NP + 1]; // per wave: the smallest cost of every examined start
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const uint64_t *__restrict__ T = A.t.text;
    uint64_t *const sT = sText[wv];
    uint32_t *const sD = sDiag[wv];
    uint16_t *const sM = sMin[wv];
    const int64_t G = (int64_t)A.max_gap;
    const uint32_t m = A.min_flank;
    const unsigned long long count = *A.list_count;
    unsigned long long cP = 0, cF = 0, cU = 0, cG = 0; // (wave-uniform)

    for (uint64_t wi = (uint64_t)blockIdx.x * 4 + wv; wi < count; wi += n_waves) { // (wave-uniform trip count)
        const uint64_t i = A.list[wi]; // (the same entry in every lane)
        uint32_t tm = 0;
        uint4 ra = make_uint4(0, 0, 0, 0);
        (void)gap_roles(A.singles[0][i], A.singles[1][i], &tm, &ra); // (the select kernel listed it)
        tm = (uint32_t)__builtin_amdgcn_readfirstlane((int)tm);
        const int64_t a = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)ra.z);
        const uint32_t aw = (uint32_t)__builtin_amdgcn_readfirstlane((int)ra.w);
        const uint32_t frag = aw & 0xffffu;
        const bool inva = REAL_HIP_SINGLE_INVERTED(aw >> 24) != 0;
        const DevBatch &bt = tm ? A.b[1] : A.b[0], &ba = tm ? A.b[0] : A.b[1];
        uint64_t o0, oa;
        const uint32_t L = (uint32_t)gap_read_span(bt, i, &o0); // (<= REAL_HIP_MAX_PATL: the select kernel)
        const int64_t La = (int64_t)gap_read_span(ba, i, &oa), Ls = (int64_t)L;
        const int64_t fs = (int64_t)A.t.frag_start[frag], fe = (int64_t)A.t.frag_start[frag + 1];
        // the window: where an ungapped hit of the target on the opposite strand would be concordant with the anchor
        int64_t lo, hi;
        if (!inva) {
            lo = max(a, max(a + La - Ls, a + (int64_t)A.min_insert - Ls));
            hi = a + (int64_t)A.max_insert - Ls;
        } else {
            lo = a + La - (int64_t)A.max_insert;
            hi = min(a, min(a + La - Ls, a + La - (int64_t)A.min_insert));
        }
        const int64_t P0 = max(lo - G, fs), P1 = min(hi + G, fe - 1);
        const int64_t nP = (lo <= hi && P0 <= P1) ? P1 - P0 + 1 : 0;
        const int64_t w0 = (P0 - G) >> 5; // (floor: the first diagonal may lie in front of the text)
        const int64_t nwd = ((P1 + G + Ls - 1) >> 5) - w0 + 2;
        uint64_t best = RH_GAP_NOKEY;
        uint32_t second = REAL_HIP_GAP_NONE;
        if (nP > (int64_t)RH_GAP_NP || (nP > 0 && nwd > (int64_t)RH_GAP_TW)) { // (max_insert is checked on the host)
            if (lane == 0) atomicOr(A.err_flags, 1u);
        } else if (nP > 0) {
            cP += (unsigned long long)nP;
            const uint32_t nw = (L + 31u) >> 5;
            wave_lds_sync(); // (the previous fragment's words are no longer in use)
            bool bad = false;
            for (uint32_t j = lane; j < nw; j += 64) sRead[wv][0][j] = ms_word(bt, o0, L, j, &bad); // (no symbol > 3: the select kernel)
            for (uint32_t j = lane; j < (uint32_t)nwd; j += 64) { // words in front of and behind the text read as zeros
                const int64_t x = w0 + (int64_t)j;
                sT[j] = (x >= 0 && (uint64_t)x * 32ull < A.t.n) ? T[x] : 0ull;
            }
            wave_lds_sync();
            if (!inva) ms_revcomp(sRead[wv][0], sRead[wv][1], L, lane); // anchor forward: the target lies on '-'
            wave_lds_sync();
            const uint64_t *const R = sRead[wv][inva ? 0 : 1];
            for (int64_t base = P0; base <= P1; base += 64) { // (wave-uniform trip count)
                wave_lds_sync(); // (the previous tile's diagonals are no longer in use)
                for (int64_t s = lane; s < 64 + 2 * G; s += 64) {
                    const int64_t q = base - G + s;
                    if (q <= P1 + G) sD[s] = gap_diagonal(R, sT, (uint32_t)(q - 32 * w0), L, m);
                }
                wave_lds_sync();
                const int64_t p = base + lane;
                if (p <= P1) {
                    const uint32_t prel = (uint32_t)(p - 32 * w0), dp = sD[lane + (uint32_t)G];
                    uint32_t minc = REAL_HIP_GAP_NONE;
                    for (int64_t g = -G; g <= G; ++g) {
                        const uint32_t ag = (uint32_t)(g < 0 ? -g : g);
                        if (p + Ls + g > fe) continue; // the span leaves the fragment
                        const uint32_t gc = g ? A.cost_open + A.cost_extend * ag : 0u;
                        if (gc > A.max_cost) continue;
                        const uint32_t kmax = A.cost_mismatch ? min(15u, (A.max_cost - gc) / A.cost_mismatch) : 15u;
                        const uint32_t dq = sD[(uint32_t)((int64_t)lane + G + g)];
                        const uint32_t head = (dp >> 8) & 0xffu;
                        if ((g ? head + (dq & 0xffu) : dp >> 16) > kmax) continue; // these bases are aligned whatever j is
                        if (A.t.has_wild && !wild_free(A.t.wild, (uint32_t)p, (uint32_t)(Ls + g))) continue;
                        uint32_t k = dp >> 16, bj = 0;
                        if (g) // the split points, left to right (gap_core.h)
                            k = gap_best_split(R, sT, prel, (uint32_t)((int64_t)prel + g), L, m, g < 0 ? ag : 0u, head, dq >> 16, &bj);
                        if (k > kmax) continue;
                        const uint32_t cost = A.cost_mismatch * k + gc;
                        const uint64_t key = gap_key(cost, ag, (uint32_t)(p - P0), g > 0, bj, k);
                        if (key < best) best = key;
                        if (cost < minc) minc = cost;
                    }
                    sM[p - P0] = (uint16_t)minc;
                }
            }
            for (int d = 32; d; d >>= 1) { const uint64_t o = __shfl_xor((unsigned long long)best, d); if (o < best) best = o; }
            wave_lds_sync();
            if (best != RH_GAP_NOKEY) { // the smallest cost among the starts more than max_gap away from the best one
                const int64_t bp = (int64_t)((best >> 14) & 0x1fffu);
                for (int64_t x = lane; x < nP; x += 64)
                    if (x - bp > G || bp - x > G) second = min(second, (uint32_t)sM[x]);
                for (int d = 32; d; d >>= 1) second = min(second, (uint32_t)__shfl_xor((int)second, d));
            }
        }
        uint4 r = gap_empty_record();
        if (best != RH_GAP_NOKEY) {
            const uint32_t cost = (uint32_t)(best >> 32), ag = (uint32_t)(best >> 27) & 31u, k = (uint32_t)best & 15u, bj = (uint32_t)(best >> 4) & 0x1ffu;
            const int32_t g = ((best >> 13) & 1u) ? (int32_t)ag : -(int32_t)ag;
            const bool rival = second != REAL_HIP_GAP_NONE && second <= cost + A.margin;
            const uint32_t state = rival ? REAL_HIP_PAIR_NONUNIQUE : REAL_HIP_PAIR_UNIQUE;
            const uint32_t tag = tm | ((inva ? 0u : 1u) << 4) | (state << 5);
            r = gap_pack_record((uint32_t)(P0 + (int64_t)((best >> 14) & 0x1fffu)), frag, A.t.fileid, tag, bj, g, k, cost, second);
            cF += 1; cU += rival ? 0 : 1; cG += ag ? 1 : 0;
        }
        if (lane == 0) A.out[i] = r;
    }
    if (lane == 0 && (cP | cF)) {
        unsigned long long *s = A.stats + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16;
        if (cP) atomicAdd(s + 3, cP);
        if (cF) atomicAdd(s + 4, cF);
        if (cU) atomicAdd(s + 5, cU);
        if (cG) atomicAdd(s + 6, cG);
    }
}

// ---- the launcher ----------------------------------------------------------------------------------------------------------
int rh_launch_gap_rescue(real_hip_ctx *ctx, const real_hip_pair_params &pp, const real_hip_gap_params &gp, const DevBatch &b1, const DevBatch &b2,
                         const real_hip_pair *d_pairs, const real_hip_single *const d_singles[2], uint64_t n, int fresh, real_hip_gap_place *d_out)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "gap rescue: more than 2^32 fragments in one call", hipSuccess);
    RhGapStage &S = ctx->gap;
    int rc;
    const size_t stat_bytes = (size_t)RH_PAIR_STRIPES * 16 * 8;
    if ((rc = rh_stats_reserve(ctx, S.stage.stats, RH_PAIR_STRIPES, 8))) return rc; // (the error flags behind the stripes)
    if ((rc = rh_reserve(ctx, S.list, n * 4 + 8))) return rc;
    GapArgs A;
    memset(&A, 0, sizeof A);
    A.t = rh_dev_text(ctx, ctx->fileid);
    A.b[0] = b1; A.b[1] = b2;
    A.pairs = (const uint2 *)d_pairs;
    A.singles[0] = (const uint4 *)d_singles[0]; A.singles[1] = (const uint4 *)d_singles[1];
    A.n = n; A.out = (uint4 *)d_out;
    A.list_count = (unsigned long long *)S.list.p; A.list = (uint32_t *)S.list.p + 2;
    A.stats = (unsigned long long *)S.stage.stats.p;
    A.err_flags = (uint32_t *)((char *)S.stage.stats.p + stat_bytes);
    A.fresh = fresh ? 1u : 0u; A.min_insert = pp.min_insert; A.max_insert = pp.max_insert;
    A.max_gap = gp.max_gap; A.min_flank = gp.min_flank; A.cost_mismatch = gp.cost_mismatch; A.cost_open = gp.cost_open;
    A.cost_extend = gp.cost_extend; A.max_cost = gp.max_cost; A.margin = gp.margin;
    RH_HIP(ctx, hipMemsetAsync(S.list.p, 0, 8, ctx->stream));
    RH_HIP(ctx, hipMemsetAsync(A.err_flags, 0, 4, ctx->stream));
    rh_time_begin(ctx, ctx->stream, S.stage);
    hipLaunchKernelGGL(gap_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    RH_HIP(ctx, hipGetLastError());
    // a fixed grid of waves takes the listed fragments in turn (their number stays on the device)
    hipLaunchKernelGGL(gap_search_kernel, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    RH_HIP(ctx, hipMemcpyAsync(&S.err, A.err_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    S.stage.items += n;
    S.stage.launches += 2;
    return REAL_HIP_OK;
}

int rh_gap_finish(real_hip_ctx *ctx)
{
    RhGapStage &S = ctx->gap;
    const uint32_t e = S.err;
    S.err = 0;
    if (e & 1u) return rh_fail(ctx, REAL_HIP_E_INVALID, "gap rescue: a window wider than REAL_HIP_MATE_SEARCH_MAX_INSERT allows", hipSuccess);
    return REAL_HIP_OK;
}

int rh_gap_stats(real_hip_ctx *ctx, real_hip_gap_stats *out, int reset)
{
    uint64_t h[7];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->gap.stage, RH_PAIR_STRIPES, 7, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->fragments = was.items; out->eligible = h[0]; out->other_file = h[2]; out->skipped = h[0] - h[1]; out->positions = h[3];
        out->placed = h[4]; out->unique = h[5]; out->gapped = h[6];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}

// ---- host only ---------------------------------------------------------------------------------------------------------------
extern "C" int real_hip_gap_cigar(const real_hip_gap_place *g, uint32_t len, char *buf, size_t cap)
{
    if (!g || !buf) return REAL_HIP_E_INVALID;
    if (REAL_HIP_GAP_STATE(g->tag) == REAL_HIP_PAIR_NOMATCH) return REAL_HIP_E_INVALID;
    char tmp[48];
    int n;
    const uint32_t j = g->split;
    if (g->gap == 0) {
        if (!len || j) return REAL_HIP_E_INVALID;
        n = snprintf(tmp, sizeof tmp, "%uM", len);
    } else if (g->gap > 0) {
        if (!j || j >= len) return REAL_HIP_E_INVALID;
        n = snprintf(tmp, sizeof tmp, "%uM%dD%uM", j, (int)g->gap, len - j);
    } else {
        const uint32_t d = (uint32_t)(-(int)g->gap);
        if (!j || j + d >= len) return REAL_HIP_E_INVALID;
        n = snprintf(tmp, sizeof tmp, "%uM%uI%uM", j, d, len - j - d);
    }
    if ((size_t)n + 1 > cap) return REAL_HIP_E_OVERFLOW;
    memcpy(buf, tmp, (size_t)n + 1);
    return n;
}
