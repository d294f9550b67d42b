// gap_anchor.hip -- anchored gap placement (include/real_hip.h, "anchored gap placement"): a single read that differs from the
// text by one insertion or deletion is placed around the ungapped hits of its first and of its last anchor_len bases.  Without
// a mate the matcher itself names the locus: whenever 2 A + max_gap <= L one of the two sub-reads lies wholly on one diagonal.
//
// gap_anchor_select_kernel: one lane per read decides from the final info words whether the read is eligible and not skipped
// and appends it to the list of the search (pair_hand_over: one atomic per wave); with `fresh` it writes the NoMatch records
// of the reads the search will not write.
// gap_anchor_extract_kernel (the composite only): one lane per base of the listed reads' sub-reads, bases and qualities, into
// a byte batch the matcher takes as any other.
// gap_anchor_search_kernel: a fixed grid of waves takes the listed reads in turn, a wave each, so a record has one writer.  A
// read has at most max_anchors <= 64 hits: lane a decodes hit a -- validity, the diagonal c, the window [P0, P1] -- and the
// wave walks the anchors one at a time (their fields by a shuffle).  An anchor that names the diagonal, strand and fragment of
// an earlier one adds nothing to the SET of candidates and is not searched again (one ballot); its starts still count.
// Both orientations of the read are packed into words of 32 bases in LDS once per read; per anchor the few text words of
// [P0 - G, P1 + G + L) are staged and every diagonal of that span (at most 4 G + 1) gets gap_diagonal's three numbers.
// The work of an anchor is then (start, g) pairs, (2 G + 1)^2 at the most, FLATTENED OVER THE 64 LANES: a window has at most
// 33 starts, so a lane per start would leave half the wave idle and make every lane loop over 33 gaps; a read has one or two
// distinct anchors far more often than many, so flattening (anchor, start) would fill the wave no better.  A pair is pruned by
// the flank test and, if it passes, walks its split points once (gap_core.h), exactly as in gap_rescue.hip.  The smallest
// cost of a start is the minimum over lanes: an LDS atomic into the anchor's 33 words, copied behind the anchor into the
// read's table of max_anchors * (2 G + 1) 16-bit entries.  A lane keeps the smallest key of its pairs in two words --
// cost:16 | |g|:5 | p:32, then v:1 | deletion:1 | j:9 | k:4 | frag:16: the absolute start no longer leaves room for k beside
// it -- and a butterfly gives every lane the wave's best; `second` is then the minimum over the table's entries on the other
// strand or more than G away from the best start, and a second butterfly.  For fresh == 0 the record is merged into the
// one in memory (gap_fold: the header's M); lane 0 writes it with one 16-byte store.
//
// Nothing depends on lanes, waves, the order of a hit list or of the list of reads.  No scratch memory; plain C++ and vector
// stores.
#include "gap_core.h"   // read_words.h; gap_mm, gap_diagonal, gap_best_split, the record packing
#include "pair_state.h" // pair_hand_over, stage_common.h

#include <cstring>

#define RH_GA_WD (2u * REAL_HIP_GAP_MAX + 1u)                       /* examined starts of an anchor at the most */
#define RH_GA_ND (4u * REAL_HIP_GAP_MAX + 1u)                       /* its diagonals */
#define RH_GA_TW ((RH_GA_ND + REAL_HIP_MAX_PATL + 31u) / 32u + 3u)  /* its text words: the read behind the last diagonal, a word that begins inside, the funnel shift */
static_assert(REAL_HIP_GAP_ANCHORS_MAX == 64, "lane a of the wave decodes hit a");

struct AnchorArgs {
    DevText t;
    DevBatch b;
    const uint64_t *info;          // final info words, nullable
    uint64_t n;                    // reads
    uint4 *out;                    // real_hip_gap_place records (gap_core.h)
    uint32_t *list;                // reads to search
    unsigned long long *list_count;
    unsigned long long *stats;     // RH_PAIR_STRIPES x 16 words: [0] eligible, [1] listed, [2] crowded, [3] unanchored, [4] anchors, [5] invalid anchors, [6] positions, [7] placed, [8] unique, [9] gapped
    uint32_t *err_flags;           // bit 0: an anchor whose text does not fit the LDS region
    const uint4 *hits;             // real_hip_hit records (pair_state.h)
    const uint64_t *hoff;          // two lists per read (compact: per list slot)
    uint64_t total;                // hits
    uint8_t *sub_bases, *sub_qual; // the extracted sub-reads
    uint64_t sub_count;            // listed reads to extract
    uint32_t compact, fresh, anchor_len, max_anchors, max_gap, min_flank, cost_mismatch, cost_open, cost_extend, max_cost, margin;
};

__global__ void __launch_bounds__(256) gap_anchor_select_kernel(const AnchorArgs A)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool eligible = false, listed = false;
    if (i < A.n) {
        eligible = !A.info || (A.info[i] >> RH_INFO_ST_SHIFT) == 0; // NoMatch, the state of a fresh record
        if (eligible) {
            uint64_t o0;
            const uint64_t L = gap_read_span(A.b, i, &o0);
            bool skip = L > (uint64_t)REAL_HIP_MAX_PATL || L < 2ull * A.min_flank + A.max_gap + 1ull || L < (uint64_t)A.anchor_len;
            if (!skip) { // a symbol > 3
                if (A.b.packed) {
                    skip = A.b.nflags && ((A.b.nflags[i >> 3] >> (i & 7)) & 1);
                } else {
                    for (uint64_t x = 0; x < L; ++x) skip = skip || A.b.bases[o0 + x] > 3;
                }
            }
            listed = !skip;
        }
        if (!listed && A.fresh) A.out[i] = gap_empty_record();
    }
    pair_hand_over(listed, (uint32_t)i, eligible ? 1ull : 0ull, blockIdx.x, A.list, A.list_count, A.stats);
}

// base x of sub-read 2 w + e of list slot w: one lane per base (the host knows how many reads were listed)
__global__ void __launch_bounds__(256) gap_anchor_extract_kernel(const AnchorArgs A)
{
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, per = 2ull * A.anchor_len;
    if (idx >= A.sub_count * per) return;
    const uint64_t w = idx / per, r = idx - w * per, e = r / A.anchor_len, x = r - e * A.anchor_len;
    const uint64_t i = A.list[w];
    uint64_t o0;
    const uint64_t L = gap_read_span(A.b, i, &o0); // (>= anchor_len: the select kernel)
    const uint64_t src = o0 + (e ? L - A.anchor_len : 0) + x;
    A.sub_bases[idx] = A.b.packed ? (uint8_t)((A.b.bases[src >> 2] >> (6u - 2u * (uint32_t)(src & 3))) & 3u) : A.b.bases[src];
    if (A.sub_qual) A.sub_qual[idx] = A.b.qual[src];
}

// The header's M: the record of this call, r (not NoMatch), merged into the one in memory, o (not NoMatch).  The winner is
// the smaller by (cost, |g|, fileid, pos, v, g, j); the loser's cost is a rival unless it lies at the winner's locus
static __device__ __forceinline__ uint4 gap_fold(const uint4 o, const uint4 r, uint32_t G, uint32_t margin)
{
    uint64_t k1[2], k2[2];
    const uint4 *const rec[2] = {&o, &r};
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const uint4 q = *rec[x];
        const int32_t g = (int32_t)(int8_t)((q.z >> 16) & 0xffu);
        const uint32_t ag = (uint32_t)(g < 0 ? -g : g);
        k1[x] = ((uint64_t)(q.w & 0xffffu) << 45) | ((uint64_t)ag << 40) | ((uint64_t)((q.y >> 16) & 0xffu) << 32) | q.x;
        k2[x] = ((uint64_t)REAL_HIP_GAP_INVERTED(q.y >> 24) << 32) | ((uint64_t)(uint32_t)(g + 128) << 16) | (q.z & 0xffffu);
    }
    const bool r_wins = k1[1] < k1[0] || (k1[1] == k1[0] && k2[1] < k2[0]);
    const uint4 w = r_wins ? r : o, l = r_wins ? o : r;
    const int64_t dp = (int64_t)w.x - (int64_t)l.x;
    const bool same = ((w.y >> 16) & 0xffu) == ((l.y >> 16) & 0xffu) && REAL_HIP_GAP_INVERTED(w.y >> 24) == REAL_HIP_GAP_INVERTED(l.y >> 24) &&
                      dp <= (int64_t)G && -dp <= (int64_t)G;
    uint32_t second = min(w.w >> 16, l.w >> 16);
    if (!same) second = min(second, l.w & 0xffffu);
    const uint32_t cost = w.w & 0xffffu;
    const bool rival = second != REAL_HIP_GAP_NONE && second <= cost + margin;
    const uint32_t tag = (REAL_HIP_GAP_INVERTED(w.y >> 24) << 4) | ((rival ? REAL_HIP_PAIR_NONUNIQUE : REAL_HIP_PAIR_UNIQUE) << 5);
    return make_uint4(w.x, (w.y & 0x00ffffffu) | (tag << 24), w.z, cost | (second << 16));
}

__global__ void __launch_bounds__(256) gap_anchor_search_kernel(const AnchorArgs A)
{
    __shared__ uint64_t sRead[4][2][RH_MAXW];                               // per wave: the read's words, straight and reverse-complemented
    __shared__ uint64_t sText[4][RH_GA_TW];                                 // per wave: the text words of the anchor
    __shared__ uint32_t sDiag[4][RH_GA_ND + 1];                             // per wave: gap_diagonal of the anchor's diagonals
    __shared__ uint32_t sCur[4][RH_GA_WD + 1];                              // per wave: the smallest cost of the anchor's starts
    __shared__ uint32_t sWin[4][REAL_HIP_GAP_ANCHORS_MAX];                  // per wave and anchor: P0
    __shared__ uint32_t sMeta[4][REAL_HIP_GAP_ANCHORS_MAX];                 // per wave and anchor: searched starts:8 | strand << 8 (0: none)
    __shared__ uint16_t sMin[4][REAL_HIP_GAP_ANCHORS_MAX * RH_GA_WD];       // per wave: the smallest cost of every searched start
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const uint64_t *__restrict__ T = A.t.text;
    uint64_t *const sT = sText[wv];
    uint32_t *const sD = sDiag[wv], *const sC = sCur[wv], *const sW = sWin[wv], *const sA = sMeta[wv];
    uint16_t *const sM = sMin[wv];
    const int64_t G = (int64_t)A.max_gap, AL = (int64_t)A.anchor_len;
    const uint32_t m = A.min_flank, Wd = 2u * A.max_gap + 1u;
    const unsigned long long count = *A.list_count;
    unsigned long long cCr = 0, cUn = 0, cAn = 0, cIv = 0, cP = 0, cF = 0, cU = 0, cG = 0; // (wave-uniform)

    for (uint64_t wi = (uint64_t)blockIdx.x * 4 + wv; wi < count; wi += n_waves) { // (wave-uniform trip count)
        const uint64_t i = A.list[wi]; // (the same entry in every lane)
        const uint64_t hb = 2ull * (A.compact ? wi : i);
        uint64_t h0 = A.hoff[hb], h1 = A.hoff[hb + 1], h2 = A.hoff[hb + 2]; // (clamped: no hit outside the list is read)
        if (h2 > A.total) h2 = A.total;
        if (h1 > h2) h1 = h2;
        if (h0 > h1) h0 = h1;
        const uint64_t nh = h2 - h0;
        uint64_t o0;
        const uint32_t L = (uint32_t)gap_read_span(A.b, i, &o0); // (anchor_len <= L <= REAL_HIP_MAX_PATL: the select kernel)
        const int64_t Ls = (int64_t)L;
        uint64_t bhi = ~0ull, blo = ~0ull;
        uint32_t second = REAL_HIP_GAP_NONE;
        if (nh == 0) {
            cUn += 1;
        } else if (nh > (uint64_t)A.max_anchors) {
            cCr += 1;
        } else {
            // lane a: hit a
            bool valid = false;
            int64_t c = 0, P0 = 0, P1 = -1;
            uint32_t v = 0, f = 0;
            if (lane < nh) {
                const uint4 h = A.hits[h0 + lane];
                const uint32_t e = h0 + lane >= h1 ? 1u : 0u;
                const int64_t q = (int64_t)h.y;
                v = (h.w >> 24) ? 1u : 0u;
                f = h.w & 0xffffu;
                if (f < A.t.n_frag) {
                    const int64_t fs = (int64_t)A.t.frag_start[f], fe = (int64_t)A.t.frag_start[f + 1];
                    if (q >= fs && q + AL <= fe) {
                        valid = true;
                        c = e == v ? q : q - (Ls - AL); // the sub-read is the head of the oriented read, or its tail
                        P0 = max(c - G, fs);
                        P1 = min(c + G, fe - 1);
                    }
                }
            }
            const uint32_t nP = valid && P0 <= P1 ? (uint32_t)(P1 - P0 + 1) : 0u;
            const uint32_t nv = (uint32_t)__popcll(__ballot(valid));
            uint32_t sumP = nP;
            for (int d = 32; d; d >>= 1) sumP += (uint32_t)__shfl_xor((int)sumP, d);
            cAn += nv; cIv += nh - nv; cP += sumP;

            const uint32_t nw = (L + 31u) >> 5;
            wave_lds_sync(); // (the previous read's words and tables are no longer in use)
            bool bad = false;
            for (uint32_t j = lane; j < nw; j += 64) sRead[wv][0][j] = ms_word(A.b, o0, L, j, &bad); // (no symbol > 3: the select kernel)
            sA[lane] = 0u;
            wave_lds_sync();
            ms_revcomp(sRead[wv][0], sRead[wv][1], L, lane);

            for (uint32_t a = 0; a < (uint32_t)nh; ++a) { // (wave-uniform trip count)
                const uint32_t nPa = (uint32_t)__shfl((int)nP, (int)a);
                if (!nPa) continue;
                const int64_t ca = (int64_t)__shfl((unsigned long long)c, (int)a), P0a = (int64_t)__shfl((unsigned long long)P0, (int)a);
                const uint32_t va = (uint32_t)__shfl((int)v, (int)a), fa = (uint32_t)__shfl((int)f, (int)a);
                // the diagonal, strand and fragment of an earlier anchor: the same candidates once more
                const unsigned long long same = __ballot(nP != 0 && c == ca && v == va && f == fa);
                if ((uint32_t)(__ffsll((long long)same) - 1) < a) continue;
                const int64_t P1a = P0a + (int64_t)nPa - 1;
                const int64_t fe = (int64_t)A.t.frag_start[fa + 1];
                const int64_t w0 = (P0a - G) >> 5; // (floor: the first diagonal may lie in front of the text)
                const int64_t nwd = ((P1a + G + Ls - 1) >> 5) - w0 + 2;
                if (nwd > (int64_t)RH_GA_TW || nPa > Wd) { // (max_gap and the read's length are checked: it does not happen)
                    if (lane == 0) atomicOr(A.err_flags, 1u);
                    continue;
                }
                const uint64_t *const R = sRead[wv][va];
                wave_lds_sync(); // (the previous anchor's text, diagonals and costs are no longer in use; the read's words are written)
                for (uint32_t j = lane; j < (uint32_t)nwd; j += 64) { // words in front of and behind the text read as zeros
                    const int64_t x = w0 + (int64_t)j;
                    sT[j] = (x >= 0 && (uint64_t)x * 32ull < A.t.n) ? T[x] : 0ull;
                }
                if (lane < nPa) sC[lane] = REAL_HIP_GAP_NONE;
                wave_lds_sync();
                for (uint32_t s = lane; s < nPa + 2u * A.max_gap; s += 64) // diagonal q = P0 - G + s
                    sD[s] = gap_diagonal(R, sT, (uint32_t)(P0a - G + (int64_t)s - 32 * w0), L, m);
                wave_lds_sync();
                for (uint32_t x = lane; x < nPa * Wd; x += 64) { // pair x: start s, gap g
                    const uint32_t s = x / Wd, gi = x - s * Wd;
                    const int64_t g = (int64_t)gi - G, p = P0a + (int64_t)s;
                    const uint32_t ag = (uint32_t)(g < 0 ? -g : g);
                    if (p + Ls + g > fe) continue; // the span leaves the fragment
                    const uint32_t gc = g ? A.cost_open + A.cost_extend * ag : 0u;
                    if (gc > A.max_cost) continue;
                    const uint32_t kmax = A.cost_mismatch ? min(15u, (A.max_cost - gc) / A.cost_mismatch) : 15u;
                    const uint32_t dp = sD[s + A.max_gap], dq = sD[s + gi];
                    const uint32_t head = (dp >> 8) & 0xffu;
                    if ((g ? head + (dq & 0xffu) : dp >> 16) > kmax) continue; // these bases are aligned whatever j is
                    if (A.t.has_wild && !wild_free(A.t.wild, (uint32_t)p, (uint32_t)(Ls + g))) continue;
                    const uint32_t prel = (uint32_t)(p - 32 * w0);
                    uint32_t k = dp >> 16, bj = 0;
                    if (g) k = gap_best_split(R, sT, prel, (uint32_t)((int64_t)prel + g), L, m, g < 0 ? ag : 0u, head, dq >> 16, &bj);
                    if (k > kmax) continue;
                    const uint32_t cost = A.cost_mismatch * k + gc;
                    const uint64_t khi = ((uint64_t)cost << 37) | ((uint64_t)ag << 32) | (uint64_t)(uint32_t)p;
                    const uint64_t klo = ((uint64_t)va << 30) | ((uint64_t)(g > 0 ? 1u : 0u) << 29) | ((uint64_t)bj << 20) | ((uint64_t)k << 16) | fa;
                    if (khi < bhi || (khi == bhi && klo < blo)) { bhi = khi; blo = klo; }
                    atomicMin(&sC[s], cost);
                }
                wave_lds_sync();
                if (lane < nPa) sM[a * Wd + lane] = (uint16_t)sC[lane];
                if (lane == 0) { sW[a] = (uint32_t)P0a; sA[a] = nPa | (va << 8); }
            }
            for (int d = 32; d; d >>= 1) {
                const uint64_t ohi = __shfl_xor((unsigned long long)bhi, d), olo = __shfl_xor((unsigned long long)blo, d);
                if (ohi < bhi || (ohi == bhi && olo < blo)) { bhi = ohi; blo = olo; }
            }
            wave_lds_sync();
            if (bhi != ~0ull) { // the smallest cost among the starts on the other strand or more than max_gap away from the best one
                const int64_t bp = (int64_t)(uint32_t)bhi;
                const uint32_t bv = (uint32_t)(blo >> 30) & 1u;
                for (uint32_t x = lane; x < (uint32_t)nh * Wd; x += 64) {
                    const uint32_t a = x / Wd, s = x - a * Wd, meta = sA[a];
                    if (s >= (meta & 0xffu)) continue;
                    const int64_t p = (int64_t)sW[a] + (int64_t)s;
                    if ((meta >> 8) != bv || p - bp > G || bp - p > G) second = min(second, (uint32_t)sM[x]);
                }
                for (int d = 32; d; d >>= 1) second = min(second, (uint32_t)__shfl_xor((int)second, d));
            }
        }
        if (bhi != ~0ull) {
            const uint32_t cost = (uint32_t)(bhi >> 37), ag = (uint32_t)(bhi >> 32) & 31u, k = (uint32_t)(blo >> 16) & 15u, bj = (uint32_t)(blo >> 20) & 0x1ffu;
            const uint32_t bv = (uint32_t)(blo >> 30) & 1u;
            const int32_t g = ((blo >> 29) & 1u) ? (int32_t)ag : -(int32_t)ag;
            const bool rival = second != REAL_HIP_GAP_NONE && second <= cost + A.margin;
            const uint32_t tag = (bv << 4) | ((rival ? REAL_HIP_PAIR_NONUNIQUE : REAL_HIP_PAIR_UNIQUE) << 5);
            uint4 r = gap_pack_record((uint32_t)bhi, (uint32_t)blo & 0xffffu, A.t.fileid, tag, bj, g, k, cost, second);
            cF += 1; cU += rival ? 0 : 1; cG += ag ? 1 : 0;
            if (!A.fresh) {
                const uint4 o = A.out[i]; // (this wave is the record's one writer)
                if (REAL_HIP_GAP_STATE(o.y >> 24) != REAL_HIP_PAIR_NOMATCH) r = gap_fold(o, r, A.max_gap, A.margin);
            }
            if (lane == 0) A.out[i] = r;
        } else if (A.fresh && lane == 0) {
            A.out[i] = gap_empty_record();
        }
    }
    if (lane == 0) {
        unsigned long long *s = A.stats + (size_t)(blockIdx.x % RH_PAIR_STRIPES) * 16;
        if (cCr) atomicAdd(s + 2, cCr);
        if (cUn) atomicAdd(s + 3, cUn);
        if (cAn) atomicAdd(s + 4, cAn);
        if (cIv) atomicAdd(s + 5, cIv);
        if (cP) atomicAdd(s + 6, cP);
        if (cF) atomicAdd(s + 7, cF);
        if (cU) atomicAdd(s + 8, cU);
        if (cG) atomicAdd(s + 9, cG);
    }
}

// ---- the launchers ---------------------------------------------------------------------------------------------------------
static int anchor_args(real_hip_ctx *ctx, const RhAnchorRun &r, AnchorArgs &A)
{
    RhGapStage &S = ctx->gap;
    int rc;
    const size_t stat_bytes = (size_t)RH_PAIR_STRIPES * 16 * 8;
    if ((rc = rh_stats_reserve(ctx, S.anchor.stats, RH_PAIR_STRIPES, 8))) return rc; // (the error flags behind the stripes)
    if ((rc = rh_reserve(ctx, S.an_list, r.n * 4 + 8))) return rc;
    memset(&A, 0, sizeof A);
    A.t = rh_dev_text(ctx, ctx->fileid);
    A.b = r.b;
    A.info = r.d_info; A.n = r.n; A.out = (uint4 *)r.d_out;
    A.list_count = (unsigned long long *)S.an_list.p; A.list = (uint32_t *)S.an_list.p + 2;
    A.stats = (unsigned long long *)S.anchor.stats.p;
    A.err_flags = (uint32_t *)((char *)S.anchor.stats.p + stat_bytes);
    A.fresh = r.fresh ? 1u : 0u; A.anchor_len = r.ap.anchor_len; A.max_anchors = r.ap.max_anchors;
    A.max_gap = r.gp.max_gap; A.min_flank = r.gp.min_flank; A.cost_mismatch = r.gp.cost_mismatch; A.cost_open = r.gp.cost_open;
    A.cost_extend = r.gp.cost_extend; A.max_cost = r.gp.max_cost; A.margin = r.gp.margin;
    return REAL_HIP_OK;
}

int rh_gap_anchor_select(real_hip_ctx *ctx, const RhAnchorRun &r, uint64_t *count)
{
    if (count) *count = 0;
    if (!r.n) return REAL_HIP_OK;
    if (r.n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "anchored gap placement: more than 2^32 reads in one call", hipSuccess);
    RhGapStage &S = ctx->gap;
    AnchorArgs A;
    int rc;
    if ((rc = anchor_args(ctx, r, A))) return rc;
    RH_HIP(ctx, hipMemsetAsync(S.an_list.p, 0, 8, ctx->stream));
    RH_HIP(ctx, hipMemsetAsync(A.err_flags, 0, 4, ctx->stream));
    rh_time_begin(ctx, ctx->stream, S.anchor);
    hipLaunchKernelGGL(gap_anchor_select_kernel, dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    S.anchor.items += r.n;
    S.anchor.launches += 1;
    if (count) {
        unsigned long long c = 0;
        RH_HIP(ctx, hipMemcpyAsync(&c, S.an_list.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        RH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *count = c;
    }
    return REAL_HIP_OK;
}

int rh_gap_anchor_extract(real_hip_ctx *ctx, const RhAnchorRun &r, uint64_t count, const uint8_t **d_bases, const uint8_t **d_qual)
{
    *d_bases = *d_qual = nullptr;
    if (!count) return REAL_HIP_OK;
    RhGapStage &S = ctx->gap;
    AnchorArgs A;
    int rc;
    if ((rc = anchor_args(ctx, r, A))) return rc;
    const uint64_t bytes = count * 2ull * r.ap.anchor_len;
    if ((rc = rh_reserve(ctx, S.an_bases, bytes + 16))) return rc; // (the matcher reads whole words)
    if (r.b.qual && (rc = rh_reserve(ctx, S.an_qual, bytes + 16))) return rc;
    A.sub_bases = (uint8_t *)S.an_bases.p; A.sub_qual = r.b.qual ? (uint8_t *)S.an_qual.p : nullptr; A.sub_count = count;
    rh_time_begin(ctx, ctx->stream, S.anchor);
    hipLaunchKernelGGL(gap_anchor_extract_kernel, dim3((unsigned)((bytes + 255) / 256)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    S.anchor.launches += 1;
    *d_bases = A.sub_bases; *d_qual = A.sub_qual;
    return REAL_HIP_OK;
}

int rh_gap_anchor_search(real_hip_ctx *ctx, const RhAnchorRun &r, const real_hip_hit *d_hits, const uint64_t *d_off, uint64_t total, bool compact)
{
    if (!r.n) return REAL_HIP_OK;
    RhGapStage &S = ctx->gap;
    AnchorArgs A;
    int rc;
    if ((rc = anchor_args(ctx, r, A))) return rc;
    A.hits = (const uint4 *)d_hits; A.hoff = d_off; A.total = total; A.compact = compact ? 1u : 0u;
    rh_time_begin(ctx, ctx->stream, S.anchor);
    // a fixed grid of waves takes the listed reads in turn (their number stays on the device)
    hipLaunchKernelGGL(gap_anchor_search_kernel, dim3(rh_wave_blocks(r.n)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    RH_HIP(ctx, hipMemcpyAsync(&S.an_err, A.err_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    S.anchor.launches += 1;
    return REAL_HIP_OK;
}

int rh_gap_anchor_finish(real_hip_ctx *ctx)
{
    RhGapStage &S = ctx->gap;
    const uint32_t e = S.an_err;
    S.an_err = 0;
    if (e & 1u) return rh_fail(ctx, REAL_HIP_E_INVALID, "anchored gap placement: an anchor wider than REAL_HIP_GAP_MAX and REAL_HIP_MAX_PATL allow", hipSuccess);
    return REAL_HIP_OK;
}

int rh_gap_anchor_stats(real_hip_ctx *ctx, real_hip_gap_anchor_stats *out, int reset)
{
    uint64_t h[10];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->gap.anchor, RH_PAIR_STRIPES, 10, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->reads = was.items; out->eligible = h[0]; out->skipped = h[0] - h[1]; out->crowded = h[2]; out->unanchored = h[3];
        out->anchors = h[4]; out->invalid_anchors = h[5]; out->positions = h[6]; out->placed = h[7]; out->unique = h[8]; out->gapped = h[9];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
