// mate_search.hip -- paired-end mate search: per fragment, every position of every anchor's window is tested for a
// placement of the other mate (whole-read Hamming compare, no seed filter), and the pairs (anchor, placement) are folded
// into the fragment's in/out record (include/real_hip.h, "mate search").
//
// One wave per fragment, so a record has one writer.  The wave walks the fragment's anchors (mate 1's hits, then mate
// 2's).  Per anchor it copies the text words of the window plus the read length (at most max_insert bases) into its LDS
// region; lane j takes window position lo + 64 t + j, funnel-shifts its text words out of LDS, XOR / popcounts them
// against the searched read's words and leaves at the first word that takes it past totalkmax -- on random text nearly
// every lane after one word.  The read's words (both mates, straight and reverse-complemented) sit in LDS too: every
// lane reads the same address, a broadcast.  Survivors are rare: they check the N bits on the resident vector, score
// with the wave matcher's long_score (sequential FP64 sum: the bits real_hip_match_all gives; qualities staged in LDS as
// there, one global load per base would be a round trip each) and merge a candidate into the lane's fold state.  After the last anchor the states are merged by a butterfly and lane 0 stores the record.
//
// Nothing depends on the order of the anchors or of the lanes (pair_state.h).  Plain C++ and vector stores.
#include "match_common.h"
#include "pair_state.h"
#include "read_words.h"

#include <cstring>

#define RH_MS_STRIPES 256u /* the statistics are striped over this many 128-byte lines (see RH_CSTRIPES) */
#define RH_MS_TW (REAL_HIP_MATE_SEARCH_MAX_INSERT / 32u + 2u) /* text words of a window: max_insert bases from anywhere inside a word, one more for the funnel shift */

struct MateSearchArgs {
    DevText t;
    DevBatch b[2];                 // the mates' reads
    MateLists L;                   // the hit lists of mate 1 / mate 2: the anchors (len[] is not read: the lengths come from the batches)
    uint64_t n;                    // fragments
    real_hip_pair *pairs;
    const double *LL;
    unsigned long long *stats;     // RH_MS_STRIPES x 16 words: [0] anchors, [1] anchors skipped, [2] positions, [3] placements
    uint32_t *err_flags;           // bit 0: a read longer than REAL_HIP_MAX_PATL, bit 1: a window wider than the LDS region
    double filter_mult;
    uint32_t fresh, fileid, scores, min_insert, max_insert, seedl, totalkmax, max_anchors;
};

template <bool SCORES>
__global__ void __launch_bounds__(256) mate_search_kernel(const MateSearchArgs A)
{
    __shared__ double sLL[SCORES ? RH_LL_SLOTS : 1];
    __shared__ uint64_t sRead[4][2][2][RH_MAXW]; // per wave, mate, strand: the words of the oriented read
    __shared__ uint64_t sText[4][RH_MS_TW];      // per wave: the text words of the anchor's window
    __shared__ uint8_t sQual[SCORES ? 4 : 1][2][SCORES ? REAL_HIP_MAX_PATL : 1]; // per wave and mate: the qualities (the scorer reads one per base)
    if (SCORES) {
        for (int i = threadIdx.x; i < 1024; i += 256) sLL[i] = A.LL[i];
        if (threadIdx.x == 0) sLL[RH_LL_ZERO] = 0.0;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const uint64_t *__restrict__ T = A.t.text;
    uint64_t *const sT = sText[wv];
    const uint32_t kmax = A.totalkmax;
    unsigned long long cA = 0, cS = 0, cP = 0, cF = 0; // (wave-uniform)

    for (uint64_t fi = (uint64_t)blockIdx.x * 4 + wv; fi < A.n; fi += n_waves) { // (wave-uniform trip count)
        const uint64_t i = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)fi); // (n <= 2^32: rh_launch_mate_search)
        uint64_t hlo[2], hhi[2], o0[2];
        uint32_t len[2];
        bool elig = true;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const DevBatch &b = A.b[m];
            A.L.range(m, i, hlo[m], hhi[m]);
            o0[m] = b.off ? b.off[i] : i * (uint64_t)b.upatl;
            const uint64_t span = b.off ? (b.off[i + 1] >= o0[m] ? b.off[i + 1] - o0[m] : 0) : (uint64_t)b.upatl;
            if (span > (uint64_t)REAL_HIP_MAX_PATL) { // (the host has refused the batches it could measure)
                if (lane == 0) atomicOr(A.err_flags, 1u);
                elig = false;
            }
            len[m] = elig ? (uint32_t)span : 0u;
            // a mate the matcher skips (matchUniqueImplementation.cpp:376-394) is neither anchor nor searched for
            if (len[m] < A.seedl) elig = false;
            if (elig && b.packed && b.nflags && ((b.nflags[i >> 3] >> (i & 7)) & 1)) elig = false;
        }
        if (hhi[0] == hlo[0] && hhi[1] == hlo[1]) elig = false; // no anchors
        if (elig) { // the reads as words of 32 bases, straight and reverse-complemented
            wave_lds_sync(); // (the previous fragment's words are no longer in use)
            bool bad = false;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const uint32_t nw = (len[m] + 31) >> 5;
                for (uint32_t j = lane; j < nw; j += 64) sRead[wv][m][0][j] = ms_word(A.b[m], o0[m], len[m], j, &bad);
            }
            elig = !__any(bad);
            if (SCORES) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    if (A.b[m].qual)
                        for (uint32_t j = lane; j < len[m]; j += 64) sQual[wv][m][j] = A.b[m].qual[o0[m] + j];
            }
            wave_lds_sync();
#pragma unroll
            for (int m = 0; m < 2; ++m) ms_revcomp(sRead[wv][m][0], sRead[wv][m][1], len[m], lane);
            wave_lds_sync();
        }
        PairState st;
        ps_clear(st);
#pragma unroll
        for (int m = 0; m < 2; ++m) { // the anchors of mate m: the other mate is searched for
            const uint64_t cnt = elig ? hhi[m] - hlo[m] : 0;
            if (A.max_anchors && cnt > A.max_anchors) { cS += cnt; continue; }
            const int om = 1 - m;
            const int64_t la = len[m], lb = len[om];
            const uint32_t nwb = ((uint32_t)lb + 31) >> 5;
            const uint64_t lastmask = ~0ull << (64 - 2 * ((uint32_t)lb - 32 * (nwb - 1)));
            for (uint64_t x = hlo[m]; x < hlo[m] + cnt; ++x) {
                const uint4 a = A.L.h[m][x]; // (the same record in every lane)
                const uint32_t aw = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.w), az = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.z);
                const int64_t pa = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)a.y);
                const uint32_t frag = aw & 0xffffu, ka = (aw >> 16) & 0xffu;
                const bool inva = (aw >> 24) != 0;
                if (frag >= A.t.n_frag) continue; // (not a hit of this text)
                const int64_t fs = (int64_t)A.t.frag_start[frag], fe = (int64_t)A.t.frag_start[frag + 1];
                if (pa < fs || pa + la > fe) continue;
                cA++;
                // the window: where a hit of the other mate on the opposite strand is concordant with the anchor and lies inside its fragment
                int64_t lo, hi;
                if (!inva) { // the anchor is the forward mate: pa <= p, pa + la <= p + lb, min <= p + lb - pa <= max
                    lo = max(pa, max(pa + la - lb, pa + (int64_t)A.min_insert - lb));
                    hi = min(pa + (int64_t)A.max_insert - lb, fe - lb);
                } else {     // the reverse one: p <= pa, p + lb <= pa + la, min <= pa + la - p <= max
                    lo = max(pa + la - (int64_t)A.max_insert, fs);
                    hi = min(pa, min(pa + la - lb, pa + la - (int64_t)A.min_insert));
                }
                if (lo > hi) continue;
                const uint64_t w0 = (uint64_t)lo >> 5;
                const uint32_t nwd = (uint32_t)((((uint64_t)hi + (uint64_t)lb - 1) >> 5) - w0) + 2;
                if (nwd > RH_MS_TW) { // (max_insert is checked on the host: hi - lo + lb <= max_insert)
                    if (lane == 0) atomicOr(A.err_flags, 2u);
                    continue;
                }
                cP += (unsigned long long)(hi - lo + 1);
                wave_lds_sync(); // (the previous window is no longer in use)
                for (uint32_t j = lane; j < nwd; j += 64) sT[j] = T[w0 + j]; // (the text is padded behind its last word)
                wave_lds_sync();
                const uint32_t invb = inva ? 0u : 1u;
                const uint64_t *const cur = sRead[wv][om][invb];
                for (int64_t base = lo; base <= hi; base += 64) { // (wave-uniform trip count)
                    const int64_t p = base + lane;
                    bool ok = p <= hi;
                    uint32_t total = 0;
                    if (ok) {
                        const uint32_t bo = (uint32_t)((uint64_t)p - 32 * w0), wi = bo >> 5, sh = 2u * (bo & 31u);
                        uint64_t t0 = sT[wi];
                        for (uint32_t j = 0; j < nwb && total <= kmax; ++j) {
                            const uint64_t t1 = sT[wi + j + 1];
                            const uint64_t al = sh ? ((t0 << sh) | (t1 >> (64 - sh))) : t0;
                            const uint64_t xw = al ^ cur[j];
                            uint64_t d = ((xw >> 1) | xw) & M55;
                            if (j + 1 == nwb) d &= lastmask;
                            total += __popcll(d);
                            t0 = t1;
                        }
                        ok = total <= kmax;
                    }
                    if (ok && A.t.has_wild) ok = wild_free(A.t.wild, (uint32_t)p, (uint32_t)lb); // (the position is valid: the window lies inside the fragment)
                    cF += (unsigned long long)__popcll(__ballot(ok));
                    if (ok) {
                        const float sc = SCORES ? long_score(sLL, T, cur, (uint32_t)p, (uint32_t)lb, A.b[om].qual ? sQual[SCORES ? wv : 0][om] : nullptr, invb) : 1.0f;
                        const uint32_t sb = __float_as_uint(sc);
                        const uint32_t s1 = m == 0 ? az : sb, s2 = m == 0 ? sb : az;
                        const uint32_t k1 = m == 0 ? ka : total, k2 = m == 0 ? total : ka;
                        const uint32_t pos1 = m == 0 ? (uint32_t)pa : (uint32_t)p, pos2 = m == 0 ? (uint32_t)p : (uint32_t)pa;
                        const uint32_t inv1 = m == 0 ? (inva ? 1u : 0u) : invb;
                        PairState c;
                        ps_candidate(c, A.scores, A.fileid, frag, pos1, pos2, inv1, s1, s2, k1, k2);
                        ps_merge(st, c);
                    }
                }
            }
        }
        if (elig) ps_butterfly(st);
        // the record: in/out records the search adds nothing to stay as they are
        if (lane == 0 && (A.fresh || st.best != pair_neg_inf())) {
            if (!A.fresh) { PairState in; ps_from_record(in, A.pairs[i]); ps_merge(st, in); }
            real_hip_pair r;
            ps_to_record(st, ps_eps(A.scores, A.filter_mult, len[0], len[1]), r); // (an empty record needs no eps)
            A.pairs[i] = r;
        }
    }
    if (lane == 0 && (cA | cS | cP | cF)) {
        unsigned long long *s = A.stats + (size_t)(blockIdx.x % RH_MS_STRIPES) * 16;
        if (cA) atomicAdd(s, cA);
        if (cS) atomicAdd(s + 1, cS);
        if (cP) atomicAdd(s + 2, cP);
        if (cF) atomicAdd(s + 3, cF);
    }
}

// the search over n fragments on device arrays; asynchronous on the ctx's stream
int rh_launch_mate_search(real_hip_ctx *ctx, const real_hip_pair_params &pp, const real_hip_mate_search_params &sp, const DevBatch &b1,
                          const DevBatch &b2, const MateLists &L, uint64_t n, uint32_t fileid, int fresh, real_hip_pair *d_pairs)
{
    if (!n) return REAL_HIP_OK;
    if (n > 0xffffffffull) return rh_fail(ctx, REAL_HIP_E_INVALID, "more than 2^32 pairs in one call", hipSuccess);
    int rc;
    const size_t stat_bytes = (size_t)RH_MS_STRIPES * 16 * 8;
    if ((rc = rh_stats_reserve(ctx, ctx->search.stage.stats, RH_MS_STRIPES, 8))) return rc; // (the error flags behind the stripes)
    MateSearchArgs A;
    memset(&A, 0, sizeof A);
    A.t = rh_dev_text(ctx, fileid);
    A.b[0] = b1; A.b[1] = b2;
    A.L = L; // (its len[] may be null: the kernel takes the read lengths from the batches)
    A.n = n; A.pairs = d_pairs; A.LL = (const double *)ctx->LL.p;
    A.stats = (unsigned long long *)ctx->search.stage.stats.p;
    A.err_flags = (uint32_t *)((char *)ctx->search.stage.stats.p + stat_bytes);
    A.filter_mult = ctx->prm.filter_mult;
    A.fresh = fresh ? 1u : 0u; A.fileid = fileid; A.scores = ctx->prm.scores ? 1u : 0u;
    A.min_insert = pp.min_insert; A.max_insert = pp.max_insert; A.seedl = ctx->prm.seedl; A.totalkmax = ctx->prm.totalkmax;
    A.max_anchors = sp.max_anchors;
    RH_HIP(ctx, hipMemsetAsync(A.err_flags, 0, 4, ctx->stream));
    rh_time_begin(ctx, ctx->stream, ctx->search.stage);
    if (A.scores) hipLaunchKernelGGL(mate_search_kernel<true>, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL(mate_search_kernel<false>, dim3(rh_wave_blocks(n)), dim3(256), 0, ctx->stream, A);
    rh_time_end(ctx, ctx->stream);
    RH_HIP(ctx, hipGetLastError());
    RH_HIP(ctx, hipMemcpyAsync(&ctx->search.err, A.err_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    ctx->search.stage.items += n;
    ctx->search.stage.launches += 1;
    return REAL_HIP_OK;
}

int rh_mate_search_finish(real_hip_ctx *ctx)
{
    const uint32_t e = ctx->search.err;
    ctx->search.err = 0;
    if (e & 1u) return rh_fail(ctx, REAL_HIP_E_INVALID, "mate search: a read is longer than the declared bound and REAL_HIP_MAX_PATL", hipSuccess);
    if (e & 2u) return rh_fail(ctx, REAL_HIP_E_INVALID, "mate search: a window wider than REAL_HIP_MATE_SEARCH_MAX_INSERT", hipSuccess);
    return REAL_HIP_OK;
}

int rh_mate_search_stats(real_hip_ctx *ctx, real_hip_mate_search_stats *out, int reset)
{
    uint64_t h[4];
    RhStageCount was;
    int rc;
    if ((rc = rh_stage_read(ctx, ctx->search.stage, RH_MS_STRIPES, 4, reset, h, was))) return rc;
    if (out) {
        out->reserved = 0;
        out->fragments = was.items; out->anchors = h[0]; out->anchors_skipped = h[1]; out->positions = h[2]; out->placements = h[3];
        out->launches = was.launches; out->kernel_ms = was.kernel_ms;
    }
    return REAL_HIP_OK;
}
